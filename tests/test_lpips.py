"""GPU tests of LPIPS on the AlexNet trunk: rfn_lpips_alex_features_u8 / rfn_lpips_alex_distance through rfn_hip.ops
against the float64 restatement of tests/test_lpips_host.py (seeded random weights: no pretrained ones exist here), the
bit rules of csrc/lpips.hip (zero on identical frames, symmetry, one channel = three, independence of batch position, batch
size and chunking, repeatability), views and leading shapes, and Evaluator.get_lpips / get_eval_values with weights."""
from types import SimpleNamespace

import pytest
import torch

from tests.test_lpips_host import (SHAPES, cases, edge_pairs, fp32_errors, make_pairs, make_state, merged_state,
                                   ref_lpips)

pytestmark = pytest.mark.gpu

# Tolerance of the kernels against the float64 restatement: |got - ref64| <= A + R * ref64 on every per-tap value and on
# their sum.  Measured, not chosen: the same restatement run in float32 on the CPU over exactly the inputs of cases()
# (tests/test_lpips_host.py fp32_errors) is off by at most FP32_ABS_SMALL on quantities below 1e-5 (the pairs one grey
# level apart) and by at most FP32_REL_LARGE relative on quantities from 1e-3 up; the factor 8 covers the summation
# order (up to 3456 exact fp32 products added in MFMA k order here, in the CPU library's blocking there; both under the
# same K * 2^-24 bound).  test_fp32_cpu_errors_match_the_recorded_ones keeps the two figures from going stale.
FP32_ABS_SMALL = 4.14e-11
FP32_REL_LARGE = 1.92e-6
A = 8 * FP32_ABS_SMALL
R = 8 * FP32_REL_LARGE


@pytest.fixture(scope="module")
def weights():
    from rfn_hip import ops
    return ops.lpips_alex_pack(merged_state(), "cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got_d, got_taps, ref_taps, ref_d, what):
    got = torch.cat([got_taps.cpu().double(), got_d.cpu().double()[:, None]], 1)
    ref = torch.cat([ref_taps, ref_d[:, None]], 1)
    err = (got - ref).abs()
    print(what, "largest |got - ref64| / (A + R ref64): %.3f" % float((err / (A + R * ref)).max()),
          "largest abs err below 1e-5: %.3g" % float(err[ref < 1e-5].max() if (ref < 1e-5).any() else 0.0),
          "largest rel err from 1e-3: %.3g" % float((err / ref)[ref >= 1e-3].max() if (ref >= 1e-3).any() else 0.0))
    assert bool((err <= A + R * ref).all()), (what, err, ref)


def test_fp32_cpu_errors_match_the_recorded_ones():
    abs_small, rel_large = fp32_errors()
    print("fp32 CPU restatement: abs %.3g (recorded %.3g), rel %.3g (recorded %.3g)" %
          (abs_small, FP32_ABS_SMALL, rel_large, FP32_REL_LARGE))
    assert FP32_ABS_SMALL / 2 <= abs_small <= 2 * FP32_ABS_SMALL
    assert FP32_REL_LARGE / 2 <= rel_large <= 2 * FP32_REL_LARGE


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_lpips_vs_restatement(weights, k):
    from rfn_hip import ops
    c = cases()[k]
    d, taps = ops.lpips_alex(weights, c["a"].cuda(), c["b"].cuda(), per_layer=True)
    N = c["shape"][0]
    assert tuple(d.shape) == (N,) and tuple(taps.shape) == (N, 5) and d.dtype == taps.dtype == torch.float32
    _check(d, taps, c["taps"], c["d"], c["shape"])


@pytest.mark.parametrize("C,H,W", [(1, 31, 31), (3, 35, 47)])
def test_lpips_edge_pairs(weights, C, H, W):
    """an identical pair (exactly 0 in every tap), all 0 against all 255, a constant frame against a random one"""
    from rfn_hip import ops
    a, b = edge_pairs(C, H, W, seed=5)
    ref_taps, ref_d = ref_lpips(merged_state(), a, b)
    d, taps = ops.lpips_alex(weights, a.cuda(), b.cuda(), per_layer=True)
    assert float(d[0]) == 0.0 and bool((taps[0] == 0).all())
    _check(d, taps, ref_taps, ref_d, ("edge", C, H, W))


def test_lpips_bit_rules(weights):
    from rfn_hip import ops
    c = cases()[1]                                   # the batch of 5, 3 x 35 x 47
    a, b = c["a"].cuda(), c["b"].cuda()
    d, taps = ops.lpips_alex(weights, a, b, per_layer=True)
    # identical frames
    d_aa, t_aa = ops.lpips_alex(weights, a, a.clone(), per_layer=True)
    assert bool((d_aa == 0).all()) and bool((t_aa == 0).all())
    # symmetry
    d_ba, t_ba = ops.lpips_alex(weights, b, a, per_layer=True)
    assert torch.equal(_bits(d), _bits(d_ba)) and torch.equal(_bits(taps), _bits(t_ba))
    # a pair alone, and after a permutation of the batch
    for i in range(5):
        d_i, t_i = ops.lpips_alex(weights, a[i:i + 1], b[i:i + 1], per_layer=True)
        assert torch.equal(_bits(d_i), _bits(d[i:i + 1])) and torch.equal(_bits(t_i), _bits(taps[i:i + 1])), i
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    d_p, t_p = ops.lpips_alex(weights, a[perm], b[perm], per_layer=True)
    assert torch.equal(_bits(d_p), _bits(d[perm])) and torch.equal(_bits(t_p), _bits(taps[perm]))
    # chunk = 2: a chunk boundary and a last partial chunk; the features themselves carry the same bits
    f_all = ops.lpips_alex_features(weights, a)
    f_two = ops.lpips_alex_features(weights, a, chunk=2)
    assert torch.equal(_bits(f_all.data), _bits(f_two.data))
    d_c, t_c = ops.lpips_alex(weights, a, b, per_layer=True, chunk=2)
    assert torch.equal(_bits(d_c), _bits(d)) and torch.equal(_bits(t_c), _bits(taps))
    # two launches
    d_2, t_2 = ops.lpips_alex(weights, a, b, per_layer=True)
    assert torch.equal(_bits(d_2), _bits(d)) and torch.equal(_bits(t_2), _bits(taps))


@pytest.mark.parametrize("k", [0, 2], ids=["3x1x31x31", "4x1x64x64"])
def test_one_channel_equals_three_identical_channels(weights, k):
    from rfn_hip import ops
    c = cases()[k]
    a, b = c["a"].cuda(), c["b"].cuda()
    f1 = ops.lpips_alex_features(weights, a)
    f3 = ops.lpips_alex_features(weights, a.repeat(1, 3, 1, 1))
    assert torch.equal(_bits(f1.data), _bits(f3.data))
    d1, t1 = ops.lpips_alex(weights, a, b, per_layer=True)
    d3, t3 = ops.lpips_alex(weights, a.repeat(1, 3, 1, 1), b.repeat(1, 3, 1, 1), per_layer=True)
    assert torch.equal(_bits(d1), _bits(d3)) and torch.equal(_bits(t1), _bits(t3))


def test_lpips_views_and_leading_shapes(weights):
    from rfn_hip import ops
    a, b = make_pairs(8, 3, 31, 33, seed=11)
    ref_taps, ref_d = ref_lpips(merged_state(), a, b)
    a5, b5 = a.view(2, 4, 3, 31, 33).cuda(), b.view(2, 4, 3, 31, 33).cuda()
    d, taps = ops.lpips_alex(weights, a5, b5, per_layer=True)
    assert tuple(d.shape) == (2, 4) and tuple(taps.shape) == (2, 4, 5)
    _check(d.reshape(-1), taps.reshape(-1, 5), ref_taps, ref_d, "5-D")
    # x[:, 2:] of [B, T, C, H, W]
    d_v = ops.lpips_alex(weights, a5[:, 2:], b5[:, 2:])
    assert tuple(d_v.shape) == (2, 2) and torch.equal(_bits(d_v), _bits(d[:, 2:]))
    # a channel slice of a 3-channel tensor is a one-channel frame batch
    a1, b1 = a[:, 1:2].contiguous(), b[:, 1:2].contiguous()
    t1, d1 = ref_lpips(merged_state(), a1, b1)
    d_s, t_s = ops.lpips_alex(weights, a.cuda()[:, 1:2], b.cuda()[:, 1:2], per_layer=True)
    _check(d_s, t_s, t1, d1, "channel slice")
    d_c = ops.lpips_alex(weights, a1.cuda(), b1.cuda())
    assert torch.equal(_bits(d_s), _bits(d_c))
    # an empty batch is no launch
    e = torch.zeros(0, 1, 32, 32, dtype=torch.uint8, device="cuda")
    d_e, t_e = ops.lpips_alex(weights, e, e, per_layer=True)
    assert tuple(d_e.shape) == (0,) and tuple(t_e.shape) == (0, 5)
    e5 = torch.zeros(2, 0, 3, 32, 32, dtype=torch.uint8, device="cuda")
    assert tuple(ops.lpips_alex(weights, e5, e5).shape) == (2, 0)


# ---------------------------------------------------------------------------------------------------- Evaluator
def _weight_files(tmp_path):
    alex, lin = make_state(0)
    torch.save(alex, tmp_path / "alexnet-owt-test.pth")
    torch.save(lin, tmp_path / "alex.pth")
    return str(tmp_path)


def _preprocess(x, reverse=False):
    """the solver's 8-bit preprocess on grey levels 0..255 (powers of two only: an exact round trip)"""
    if not reverse:
        return x / 256 - 0.5
    return torch.clamp(torch.floor((x + 0.5) * 256), 0, 255).byte()


def test_get_lpips_vs_restatement(tmp_path):
    from evaluation_metrics import Evaluator
    solver = SimpleNamespace(model=None, args=SimpleNamespace(n_frames=4), device=torch.device("cuda"))
    ev = Evaluator(solver, settings=SimpleNamespace(lpips_weights=_weight_files(tmp_path)))
    a, b = make_pairs(6, 1, 32, 32, seed=21)
    ref_taps, ref_d = ref_lpips(merged_state(), a, b)
    X, Y = a.view(2, 3, 1, 32, 32), b.view(2, 3, 1, 32, 32)
    got = ev.get_lpips(X.cuda(), Y.cuda())
    assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (2, 3)
    err = (got.double().reshape(-1) - ref_d).abs()
    assert bool((err <= A + R * ref_d).all()), (err, ref_d)
    # integer-valued float input, as the reference passes it, gives the same numbers
    assert torch.equal(ev.get_lpips(X.float().cuda(), Y.float().cuda()), got)
    with pytest.raises(ValueError):
        ev.get_lpips(X.float().cuda() + 0.5, Y.cuda())


def test_get_eval_values_with_lpips(tmp_path, monkeypatch):
    """get_eval_values with a stub model (prepared predictions and losses, no flow kernel): 2 batches of B = 3 sequences,
    2 conditioning + 2 predicted frames of 1 x 32 x 32, 3 draws.  Best-of-N on the time-mean LPIPS (strictly lower wins),
    the reference's aliasing of draw 0 with the best-so-far tensor in the mean over draws, shapes, dtypes, CPU placement,
    and resample + 1 trunk passes per batch."""
    from evaluation_metrics import Evaluator
    from rfn_hip import ops
    B, T, start, R_, n_batches = 3, 4, 2, 3, 2
    g = torch.Generator().manual_seed(31)
    batches = [torch.randint(0, 256, (B, T, 1, 32, 32), generator=g).float() for _ in range(n_batches)]
    # draw r of sequence i: the ground truth plus noise of an amplitude that orders the draws differently per sequence
    amp = torch.tensor([[[40, 10, 25], [10, 25, 40], [25, 40, 10]], [[10, 40, 25], [40, 25, 10], [25, 10, 40]]])
    preds = []
    for bi in range(n_batches):
        for r in range(R_):
            gt = batches[bi][:, start:]
            noise = (torch.rand(gt.shape, generator=g) * 2 - 1) * amp[bi, r].view(B, 1, 1, 1, 1)
            p = (gt + noise).round().clamp(0, 255)
            preds.append(_preprocess(p).permute(1, 0, 2, 3, 4).contiguous())       # [n_pred, B, C, H, W], model space
    calls = {"predict": 0, "loss": 0}

    class Model(object):
        def eval(self):
            return self

        def predict(self, image, n_pred, n_cond):
            assert (n_pred, n_cond) == (T - start, start)
            calls["predict"] += 1
            return None, preds[calls["predict"] - 1].cuda()

        def loss(self, image, _):
            calls["loss"] += 1
            return None, torch.tensor(1.0 * calls["loss"]), torch.tensor(2.0 * calls["loss"])

    solver = SimpleNamespace(model=Model(), args=SimpleNamespace(n_frames=T, n_conditions=start, choose_data="mnist"),
                             device=torch.device("cuda"), preprocess=_preprocess)
    ev = Evaluator(solver, settings=SimpleNamespace(n_frames=T, start_predictions=start, resample=R_, n_trained=T,
                                                    lpips_weights=_weight_files(tmp_path)))
    trunk_calls = []
    plain_features = ops.lpips_alex_features

    def features_spy(w, frames, **k):
        trunk_calls.append(tuple(frames.shape))
        return plain_features(w, frames, **k)

    monkeypatch.setattr(ops, "lpips_alex_features", features_spy)
    out = ev.get_eval_values("rfn.pt", loader=batches)
    mse_v, psnr_v, ssim_v, lpips_v, bpd, dkl, recon, ssim_std, psnr_std, lpips_std = out
    assert calls == {"predict": n_batches * R_, "loss": n_batches * R_}
    assert trunk_calls == [(B, T - start, 1, 32, 32)] * (n_batches * (R_ + 1))
    for t in (mse_v, psnr_v, ssim_v, lpips_v, ssim_std, psnr_std, lpips_std):
        assert tuple(t.shape) == (n_batches * B, T - start) and t.dtype == torch.float32 and t.device.type == "cpu"

    exp_best, exp_std, quirk_seen = [], [], False
    for bi in range(n_batches):
        gt = batches[bi][:, start:].to(torch.uint8)
        draws = []
        for r in range(R_):
            p = _preprocess(preds[bi * R_ + r], reverse=True).permute(1, 0, 2, 3, 4)
            draws.append(ref_lpips(merged_state(), p.reshape(-1, 1, 32, 32), gt.reshape(-1, 1, 32, 32))[1]
                         .view(B, T - start))
        means = torch.stack([d.mean(-1) for d in draws])
        for i in range(R_):     # the selection compares time-means: no near-ties between draws
            for j in range(i):
                assert bool(((means[i] - means[j]).abs() >= 1e-4).all()), means
        best = draws[0].clone()
        for r in range(1, R_):
            sel = best.mean(-1) > draws[r].mean(-1)
            best[sel] = draws[r][sel]
        exp_best.append(best)
        # draw 0 of the mean over draws IS the best-so-far tensor in the reference: it holds the final best values
        exp_std.append((best + sum(draws[1:])) / R_)
        quirk_seen = quirk_seen or bool(((exp_std[-1] - sum(draws) / R_).abs() > 1e-4).any())
        assert bool((torch.stack(draws).argmin(0) != 0).any())
    exp_best, exp_std = torch.cat(exp_best), torch.cat(exp_std)
    assert bool(((lpips_v.double() - exp_best).abs() <= A + R * exp_best).all()), (lpips_v, exp_best)
    assert bool(((lpips_std.double() - exp_std).abs() <= A + R * exp_std).all()), (lpips_std, exp_std)
    assert quirk_seen
