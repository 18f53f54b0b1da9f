"""GPU tests of the I3D trunk behind the Frechet Video Distance (csrc/i3d.hip through rfn_hip.ops) against the float64
restatement of tests/test_i3d_host.py (seeded random weights: no pretrained ones exist here): single units at the shapes
where the implicit GEMM can go wrong, writes at a channel offset, the SAME max pool with all-negative windows, the legacy
resize, one inception block, the head, the whole trunk on the smallest legal input, the bit rules of the public path, and
Evaluator.get_fvd_values."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_i3d_host import (TRUNK_SHAPE, UNIT_CASES, bound, cf, cl, error_figures, fp32_layer_errors,
                                 fp32_trunk_errors, layer_cases, make_net, randn_map, ref_pool, ref_preprocess, ref_unit,
                                 rms, state_a, state_b, trunk_case)

pytestmark = pytest.mark.gpu

# Tolerance of the kernels against the float64 restatement: |got - ref64| <= A rms(ref64) + R |ref64| entry by entry
# (error_figures / bound of tests/test_i3d_host.py: the absolute part is scaled to the RMS of the compared tensor because
# logits and pre-activation sums cross zero).  Measured, not chosen: the same restatement run in float32 on the CPU over
# exactly the inputs of layer_cases() is off by at most FP32_LAYER_A of the RMS on entries below the RMS and by at most
# FP32_LAYER_R relative on the others, and over trunk_case() by FP32_TRUNK_A and FP32_TRUNK_R; the factor 8 covers the
# summation order (up to 5184 exact fp32 products added in MFMA k order here, in the CPU library's blocking there) and
# the rounding of the folded weights to float32.  test_fp32_cpu_errors_match_the_recorded_ones keeps the figures from
# going stale.
FP32_LAYER_A, FP32_LAYER_R = 2.05e-6, 1.63e-6
FP32_TRUNK_A, FP32_TRUNK_R = 1.03e-6, 8.06e-7
MARGIN = 8
# RMS of the 400 random-weight logits of the trunk case: the initialisation neither collapses nor blows up
LOGITS_RMS = 6.34
# Resize: |got - ref64| <= RESIZE_BOUND on values in [-1, 1].  The weights are the same float32 numbers on both sides.
# On the 0..255 scale every lerp a + (b - a) w rounds twice (product, sum), the difference of the two row results once
# more; every rounding is at most ulp(255) / 2 = 2^-17 and the row errors enter the column lerp with weights that add up
# to 1: 2 + 3 = 5 roundings.  2 v / 255 - 1 scales that by 2 / 255 and rounds twice more below 2 (2^-24 each).
RESIZE_BOUND = 5 * 2.0 ** -17 * 2 / 255 + 2 * 2.0 ** -24


@pytest.fixture(scope="module")
def weights():
    from rfn_hip import ops
    return ops.i3d_pack(state_a(make_net()), "cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got, ref, A, R, what):
    got = got.cpu().double()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    a, r = error_figures(got, ref)
    worst = float(((got - ref).abs() / bound(ref, MARGIN * A, MARGIN * R)).max())
    print(what, "rms %.4g  kernel A %.3g R %.3g  (float32 CPU: A %.3g R %.3g)  worst |err| / bound %.3f" %
          (rms(ref), a, r, A, R, worst))
    assert bool(((got - ref).abs() <= bound(ref, MARGIN * A, MARGIN * R)).all()), (what, a, r)


def test_fp32_cpu_errors_match_the_recorded_ones():
    la, lr = fp32_layer_errors()
    ta, tr = fp32_trunk_errors()
    c = trunk_case()
    print("fp32 CPU restatement: layers A %.3g R %.3g (recorded %.3g %.3g), trunk A %.3g R %.3g (recorded %.3g %.3g); "
          "logits rms %.4g (recorded %.3g); float64 trunk restatement %.1f s" %
          (la, lr, FP32_LAYER_A, FP32_LAYER_R, ta, tr, FP32_TRUNK_A, FP32_TRUNK_R, rms(c["ref"]), LOGITS_RMS, c["seconds"]))
    for got, rec in ((la, FP32_LAYER_A), (lr, FP32_LAYER_R), (ta, FP32_TRUNK_A), (tr, FP32_TRUNK_R)):
        assert rec / 2 <= got <= 2 * rec, (got, rec)
    assert abs(rms(c["ref"]) - LOGITS_RMS) <= 0.01 * LOGITS_RMS


# ---------------------------------------------------------------------------------------------------- one unit
@pytest.mark.parametrize("k", range(len(UNIT_CASES)), ids=["%s-%dx%dx%dx%d" % c for c in UNIT_CASES])
def test_unit_vs_restatement(weights, k):
    from rfn_hip import ops
    c = layer_cases()[k]
    got = ops.i3d_unit(weights, c["what"][1], c["x"].cuda())
    if c["what"][1] == "logits":
        assert float(c["ref"].min()) < 0       # bias, no ReLU
    _check(got, c["ref"], FP32_LAYER_A, FP32_LAYER_R, c["what"])


def test_unit_writes_only_its_columns(weights):
    """Mixed_3b's 3x3x3 unit of branch 1 (96 -> 128) lands at channel offset 64 of the block's 256-wide output"""
    from rfn_hip import ops
    x = randn_map((1, 2, 4, 4, 96), 400)
    ref = cl(ref_unit(make_net(), "Mixed_3b.b1b", cf(x.double())))
    sentinel = -12345.678
    out = torch.full((1, 2, 4, 4, 256), sentinel, device="cuda")
    before = _bits(out).clone()
    assert ops.i3d_unit(weights, "Mixed_3b.b1b", x.cuda(), out, 64) is out
    _check(out[..., 64:192], ref, FP32_LAYER_A, FP32_LAYER_R, "offset 64")
    after = _bits(out)
    assert torch.equal(after[..., :64], before[..., :64]) and torch.equal(after[..., 192:], before[..., 192:])
    with pytest.raises(ValueError, match="out must be"):
        ops.i3d_unit(weights, "Mixed_3b.b1b", x.cuda(), out, 129)


# ---------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("kt,khw,st,shw", [(1, 3, 1, 2), (3, 3, 2, 2), (3, 3, 1, 1), (2, 2, 2, 2)])
def test_maxpool_vs_restatement_ignores_padding(kt, khw, st, shw):
    """inputs are mostly negative, so every map has windows that hold only negative values: a pool that read its
    padding as zero would return 0 there.  A maximum is exact: the comparison is for equality."""
    from rfn_hip import ops
    for THW in ((3, 5, 7), (1, 1, 1), (2, 4, 4)):
        for C in (5, 64):
            x = randn_map((2,) + THW + (C,), 500 + C + THW[1]) - 2.0
            ref = cl(ref_pool(cf(x.double()), (kt, khw, khw), (st, shw, shw)))
            assert bool((ref < 0).any()) and bool(torch.isfinite(ref).all())
            got = ops.i3d_maxpool(x.cuda(), kt, khw, st, shw)
            assert tuple(got.shape) == tuple(ref.shape), (THW, C, got.shape, ref.shape)
            assert torch.equal(got.cpu().double(), ref), (THW, C)


# ---------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("shape", [(2, 2, 1, 64, 64), (2, 2, 3, 64, 64), (1, 2, 3, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_preprocess_vs_restatement(shape):
    from rfn_hip import ops
    g = torch.Generator().manual_seed(sum(shape))
    v = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    ref = ref_preprocess(v)
    got = ops.i3d_preprocess(v.cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape) == shape[:2] + (224, 224, 3)
    err = float((got.cpu().double() - ref).abs().max())
    print(shape, "largest |got - ref64| %.3g, bound %.3g" % (err, RESIZE_BOUND))
    assert err <= RESIZE_BOUND
    if shape[2] == 1:
        assert torch.equal(_bits(got), _bits(ops.i3d_preprocess(v.cuda().repeat(1, 1, 3, 1, 1))))


# ---------------------------------------------------------------------------------------------------- block, head
def test_inception_block_vs_restatement(weights):
    from rfn_hip import ops
    c = layer_cases()[len(UNIT_CASES)]
    assert c["what"] == ("mixed", "Mixed_3b")
    got = ops.i3d_inception(weights, "Mixed_3b", c["x"].cuda())
    for lo, hi in ((0, 64), (64, 192), (192, 224), (224, 256)):      # every branch on its own, then the whole map
        _check(got[..., lo:hi], c["ref"][..., lo:hi], FP32_LAYER_A, FP32_LAYER_R, ("Mixed_3b", lo, hi))
    _check(got, c["ref"], FP32_LAYER_A, FP32_LAYER_R, "Mixed_3b")


def test_head_vs_restatement(weights):
    from rfn_hip import ops
    c = layer_cases()[len(UNIT_CASES) + 1]
    assert c["what"][0] == "head" and tuple(c["x"].shape) == (2, 3, 7, 7, 1024)
    got = ops.i3d_head(weights, c["x"].cuda())
    assert tuple(got.shape) == (2, 400)
    _check(got, c["ref"], FP32_LAYER_A, FP32_LAYER_R, "head")
    with pytest.raises(ValueError, match="last map"):
        ops.i3d_head(weights, c["x"][:, :1].contiguous().cuda())


# ---------------------------------------------------------------------------------------------------- whole trunk
@pytest.fixture(scope="module")
def trunk(weights):
    from rfn_hip import ops
    c = trunk_case()
    return c, ops.i3d_logits(weights, c["x"].cuda())


def test_whole_trunk_vs_restatement(trunk):
    """i3d_logits on (1, 9, 193, 193, 3), the smallest legal input; all 400 logits are compared"""
    c, got = trunk
    assert tuple(c["x"].shape) == TRUNK_SHAPE and tuple(got.shape) == (1, 400)
    _check(got, c["ref"], FP32_TRUNK_A, FP32_TRUNK_R, "trunk")


def test_trunk_size_rules_on_the_device(weights):
    from rfn_hip import ops
    for shape, rule in (((1, 8, 193, 193, 3), "T must be at least 9"), ((1, 9, 192, 193, 3), r"193\.\.224"),
                        ((1, 9, 193, 225, 3), r"193\.\.224")):
        with pytest.raises(ValueError, match=rule):
            ops.i3d_logits(weights, torch.zeros(shape, device="cuda"))
    with pytest.raises(ValueError, match="T must be at least 9"):
        ops.i3d_embed(weights, torch.zeros((1, 8, 1, 16, 16), dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------------------------------- public path
@pytest.mark.parametrize("C", [1, 3])
def test_embed_bit_rules(weights, C):
    from rfn_hip import ops
    g = torch.Generator().manual_seed(600 + C)
    v = torch.randint(0, 256, (2, 9, C, 64, 64), generator=g, dtype=torch.uint8).cuda()
    e = ops.i3d_embed(weights, v)
    assert tuple(e.shape) == (2, 400) and e.dtype == torch.float32 and bool(torch.isfinite(e).all())
    assert not torch.equal(e[0], e[1])
    # the public path is preprocess + trunk
    assert torch.equal(_bits(e), _bits(ops.i3d_logits(weights, ops.i3d_preprocess(v))))
    # a video alone, any chunk, two launches
    for i in range(2):
        assert torch.equal(_bits(ops.i3d_embed(weights, v[i:i + 1])), _bits(e[i:i + 1])), i
    assert torch.equal(_bits(ops.i3d_embed(weights, v, chunk=1)), _bits(e))
    assert torch.equal(_bits(ops.i3d_embed(weights, v)), _bits(e))
    if C == 1:      # one channel gives the bits of three identical channels
        assert torch.equal(_bits(ops.i3d_embed(weights, v.repeat(1, 1, 3, 1, 1))), _bits(e))
    with pytest.raises(ValueError, match="chunk"):
        ops.i3d_embed(weights, v, chunk=0)
    assert tuple(ops.i3d_embed(weights, v[:0]).shape) == (0, 400)


# ---------------------------------------------------------------------------------------------------- Evaluator
def _preprocess(x, reverse=False):
    """the solver's 8-bit preprocess on grey levels 0..255 (powers of two only: an exact round trip)"""
    if not reverse:
        return x / 256 - 0.5
    return torch.clamp(torch.floor((x + 0.5) * 256), 0, 255).byte()


def test_get_fvd_values(tmp_path):
    """get_fvd_values with a stub model (prepared predictions, no flow kernel) on the synthetic dataset: 16 sequences in
    batches of 6, 6 and 4 (the short one padded for predict and cut again), 2 conditioning + 9 predicted frames of
    1 x 32 x 32, weight files in both formats.  The two FVDs are recomputed here from the same draws."""
    from data_generators.synthetic import SyntheticMovingMNIST
    from evaluation_metrics import Evaluator
    from rfn_hip import ops
    B, start, n_pred, n_seq = 6, 2, 9, 16
    T = start + n_pred
    net = make_net()
    # the stem as a state dict, everything else as an .npz of the TF variables
    torch.save({k: v for k, v in state_a(net).items() if k.startswith("Conv3d_")}, tmp_path / "stem.pt")
    np.savez(tmp_path / "rest.npz", **{k: v.numpy() for k, v in state_b(net, gamma=True, quirk=True).items()
                                       if "/Conv3d_1a" not in k and "/Conv3d_2" not in k})
    ds = SyntheticMovingMNIST(seq_len=T, image_size=32, digit_size=12, length=n_seq, seed=3)
    data = torch.stack([ds[i] for i in range(n_seq)])
    data = (data * 255).round()                                        # grey levels [16, T, 1, 32, 32]
    batches = [data[0:6], data[6:12], data[12:16]]
    g = torch.Generator().manual_seed(41)
    draws = []          # per pass and batch: predictions of a full batch in model space [n_pred, B, C, H, W]
    for p in range(2):
        for b in batches:
            full = torch.cat([b, torch.zeros((B - b.shape[0],) + tuple(b.shape[1:]))])
            noise = (torch.rand(full[:, start:].shape, generator=g) * 2 - 1) * (30 + 30 * p)
            draws.append(_preprocess((full[:, start:] + noise).round().clamp(0, 255)).permute(1, 0, 2, 3, 4).contiguous())
    calls = []

    class Model(object):
        def eval(self):
            return self

        def predict(self, image, n_predicts, n_conditions):
            assert (n_predicts, n_conditions) == (n_pred, start) and int(image.shape[0]) == B
            calls.append(tuple(image.shape))
            return None, draws[len(calls) - 1].cuda()

    solver = SimpleNamespace(model=Model(), args=SimpleNamespace(n_frames=T, n_conditions=start, choose_data="mnist",
                                                                 batch_size=B),
                             device=torch.device("cuda"), preprocess=_preprocess)
    ev = Evaluator(solver, settings=SimpleNamespace(n_frames=T, start_predictions=start, fvd_weights=str(tmp_path)))
    assert ev._i3d is None
    mean, std = ev.get_fvd_values("rfn.pt", n_pred, loader=batches)
    assert len(calls) == 6 and ev._i3d is not None

    w = ops.i3d_pack(state_a(net), "cuda")
    assert torch.equal(ev._i3d.data, w.data)
    gt = ops.i3d_embed(w, data[:, start:].to(torch.uint8).cuda())
    fvds = []
    for p in range(2):
        pred = torch.cat([_preprocess(draws[3 * p + j], reverse=True).permute(1, 0, 2, 3, 4)[:batches[j].shape[0]]
                          for j in range(3)])
        assert tuple(pred.shape) == (n_seq, n_pred, 1, 32, 32)
        fvds.append(ops.frechet_distance(gt, ops.i3d_embed(w, pred.cuda())))
    print("FVD of the two passes", fvds, "evaluator", mean, std)
    assert min(fvds) > 0 and fvds[0] != fvds[1]
    assert abs(mean - np.mean(fvds)) <= 1e-9 * np.mean(fvds) and abs(std - np.std(fvds)) <= 1e-9 * np.mean(fvds)
    assert isinstance(mean, float) and isinstance(std, float)
    # too few sequences for a Frechet distance
    calls.clear()
    with pytest.raises(ValueError, match="at least 16"):
        ev.get_fvd_values("rfn.pt", n_pred, loader=batches[:2])


def test_get_fvd_values_without_weights():
    from evaluation_metrics import Evaluator
    solver = SimpleNamespace(model=None, args=SimpleNamespace(n_frames=11), device=torch.device("cuda"))
    with pytest.raises(RuntimeError, match="fvd_weights"):
        Evaluator(solver, settings=SimpleNamespace(start_predictions=2)).get_fvd_values("rfn.pt", 9)
