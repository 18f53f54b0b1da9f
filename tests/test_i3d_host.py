"""CPU tests of the Frechet Video Distance (csrc/i3d.hip, rfn_hip/i3d.py, Evaluator.get_fvd_values), and the float64
restatement of the I3D network that the GPU tests (tests/test_i3d.py) compare against: SAME-padding arithmetic and map
sizes, block widths, TF1's legacy bilinear resize against hand-computed values, the BatchNorm fold, the loader on both
weight-file formats, the Frechet distance against closed forms, and the size rules.

No pretrained weights exist here: all weights are seeded random ones.  The restatement below is test infrastructure with
its own copy of the layer table (from the definition in DESIGN.md section 14): the product never imports it."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

EPS = 1e-3
# inception block -> (Cin, (a, b, c, d, e, f))
MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))
MIXED_OUT = {"Mixed_3b": 256, "Mixed_3c": 480, "Mixed_4b": 512, "Mixed_4c": 512, "Mixed_4d": 512, "Mixed_4e": 528,
             "Mixed_4f": 832, "Mixed_5b": 832, "Mixed_5c": 1024}
# pools in front of a block: (kernel (t, h, w), stride)
POOL_BEFORE = {"Mixed_4b": ((3, 3, 3), (2, 2, 2)), "Mixed_5b": ((2, 2, 2), (2, 2, 2))}
# branch unit -> (PyTorch-port name, TF scope)
BRANCH = (("b0", "Branch_0/Conv3d_0a_1x1"), ("b1a", "Branch_1/Conv3d_0a_1x1"), ("b1b", "Branch_1/Conv3d_0b_3x3"),
          ("b2a", "Branch_2/Conv3d_0a_1x1"), ("b2b", "Branch_2/Conv3d_0b_3x3"), ("b3b", "Branch_3/Conv3d_0b_1x1"))


def unit_specs():
    """unit -> (Cin, Cout, k, stride), the 57 units in network order (PyTorch-port names)"""
    s = {"Conv3d_1a_7x7": (3, 64, 7, 2), "Conv3d_2b_1x1": (64, 64, 1, 1), "Conv3d_2c_3x3": (64, 192, 3, 1)}
    for name, cin, (a, b, c, d, e, f) in MIXED:
        for br, spec in zip(BRANCH, ((cin, a, 1), (cin, b, 1), (b, c, 3), (cin, d, 1), (d, e, 3), (cin, f, 1))):
            s[name + "." + br[0]] = spec + (1,)
    return s


# ---------------------------------------------------------------------------------------------------- weights
@functools.lru_cache(maxsize=None)
def make_net(seed=0):
    """seeded random network: unit -> dict(w [O, I, k, k, k], gamma, beta, mean, var), "logits" -> dict(w, b); float32.
    Convolutions randn * sqrt(2 / (Cin k^3)), gamma and var uniform [0.5, 1.5], beta and mean randn * 0.1, the logits
    bias randn * 0.1."""
    g = torch.Generator().manual_seed(seed)
    net = {}
    for name, (cin, cout, k, _) in unit_specs().items():
        net[name] = dict(w=torch.randn(cout, cin, k, k, k, generator=g) * (2.0 / (cin * k ** 3)) ** 0.5,
                         gamma=torch.rand(cout, generator=g) + 0.5, beta=torch.randn(cout, generator=g) * 0.1,
                         mean=torch.randn(cout, generator=g) * 0.1, var=torch.rand(cout, generator=g) + 0.5)
    net["logits"] = dict(w=torch.randn(400, 1024, 1, 1, 1, generator=g) * (2.0 / 1024) ** 0.5,
                         b=torch.randn(400, generator=g) * 0.1)
    return net


def state_a(net, gamma=True):
    """format A: the state dict of the common PyTorch port (plus a key the loader must ignore)"""
    sd = {"extra.num_batches_tracked": torch.zeros(1)}
    for name, p in net.items():
        sd[name + ".conv3d.weight"] = p["w"]
        if name == "logits":
            sd[name + ".conv3d.bias"] = p["b"]
            continue
        if gamma:
            sd[name + ".bn.weight"] = p["gamma"]
        sd[name + ".bn.bias"], sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"] = p["beta"], p["mean"], p["var"]
    return sd


def state_b(net, gamma=False, quirk=False):
    """format B: the TF variable names; quirk: Mixed_5b's 3x3x3 unit of branch 2 under its upstream name Conv3d_0a_3x3"""
    tf_of = dict(BRANCH)
    sd = {}
    for name, p in net.items():
        if name == "logits":
            scope = "Logits/Conv3d_0c_1x1"
        elif "." in name:
            block, br = name.split(".")
            scope = block + "/" + tf_of[br]
            if quirk and name == "Mixed_5b.b2b":
                scope = "Mixed_5b/Branch_2/Conv3d_0a_3x3"
        else:
            scope = name
        scope = "RGB/inception_i3d/" + scope
        sd[scope + "/conv_3d/w"] = p["w"].permute(2, 3, 4, 1, 0).contiguous()
        if name == "logits":
            sd[scope + "/conv_3d/b"] = p["b"]
            continue
        for key, src in (("beta", "beta"), ("moving_mean", "mean"), ("moving_variance", "var")) + \
                ((("gamma", "gamma"),) if gamma else ()):
            sd[scope + "/batch_norm/" + key] = p[src].view(1, 1, 1, 1, -1)
    return sd


# ---------------------------------------------------------------------------------------------------- restatement
def same(n, k, s):
    """(out, pad before, pad after) of TF "SAME" padding on one axis"""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


def _pad(x, k3, s3, value):
    """x [N, C, T, H, W] padded as SAME for kernel k3 and stride s3"""
    p = [same(n, k, s) for n, k, s in zip(x.shape[2:], k3, s3)]
    return F.pad(x, (p[2][1], p[2][2], p[1][1], p[1][2], p[0][1], p[0][2]), value=value)


def ref_unit(net, name, x, dtype=torch.float64):
    """convolution without bias, inference BatchNorm (unfolded), ReLU; "logits": convolution with bias only.
    x [N, C, T, H, W] in `dtype`"""
    p = net[name]
    k = p["w"].shape[2]
    stride = 1 if name == "logits" else unit_specs()[name][3]
    y = F.conv3d(_pad(x, (k,) * 3, (stride,) * 3, 0.0), p["w"].to(dtype), stride=stride)
    v = lambda t: t.to(dtype).view(1, -1, 1, 1, 1)
    if name == "logits":
        return y + v(p["b"])
    return F.relu((y - v(p["mean"])) / torch.sqrt(v(p["var"]) + EPS) * v(p["gamma"]) + v(p["beta"]))


def ref_pool(x, k3, s3):
    """SAME max pool: padded cells are -inf, so they never win"""
    return F.max_pool3d(_pad(x, k3, s3, float("-inf")), k3, s3)


def ref_mixed(net, name, x, dtype=torch.float64):
    u = lambda br, t: ref_unit(net, name + "." + br, t, dtype)
    return torch.cat([u("b0", x), u("b1b", u("b1a", x)), u("b2b", u("b2a", x)),
                      u("b3b", ref_pool(x, (3, 3, 3), (1, 1, 1)))], 1)


def ref_head(net, x, dtype=torch.float64):
    """x [N, 1024, T', 7, 7] -> [N, 400]"""
    y = ref_unit(net, "logits", F.avg_pool3d(x, (2, 7, 7), 1), dtype)
    return y.squeeze(4).squeeze(3).mean(2)


def ref_trunk(net, x, dtype=torch.float64, stages=None):
    """x [N, 3, T, H, W] -> the last map [N, 1024, T', 7, 7]; `stages`, a list, receives every stage's output"""
    keep = (lambda t: stages.append(t)) if stages is not None else (lambda t: None)
    x = ref_unit(net, "Conv3d_1a_7x7", x, dtype); keep(x)
    x = ref_pool(x, (1, 3, 3), (1, 2, 2)); keep(x)
    x = ref_unit(net, "Conv3d_2b_1x1", x, dtype); keep(x)
    x = ref_unit(net, "Conv3d_2c_3x3", x, dtype); keep(x)
    x = ref_pool(x, (1, 3, 3), (1, 2, 2)); keep(x)
    for name, _, _ in MIXED:
        if name in POOL_BEFORE:
            x = ref_pool(x, *POOL_BEFORE[name]); keep(x)
        x = ref_mixed(net, name, x, dtype); keep(x)
    return x


def cl(x):
    """[N, C, T, H, W] -> channels-last [N, T, H, W, C]"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def cf(x):
    """channels-last [N, T, H, W, C] -> [N, C, T, H, W]"""
    return x.permute(0, 4, 1, 2, 3).contiguous()


def ref_logits(net, x_cl, dtype=torch.float64):
    """channels-last input [N, T, H, W, 3] -> logits [N, 400]"""
    return ref_head(net, ref_trunk(net, cf(x_cl.to(dtype)), dtype), dtype)


def ref_resize(v, out_hw, dtype=torch.float64):
    """TF1 resize_bilinear (align_corners=False, no half-pixel centres) of [..., H, W] to out_hw, written out by hand:
    src = dst * (in / out) and the weight src - floor(src) in float32 as TF computes them, i1 = min(i0 + 1, in - 1); the
    two rows are interpolated along x, then the two results along y, in `dtype`"""
    H, W = v.shape[-2:]

    def axis(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        src = np.arange(n_out, dtype=np.float32) * scale
        i0 = np.floor(src)
        w = (src - i0).astype(np.float32)
        i0 = i0.astype(np.int64)
        return torch.from_numpy(i0), torch.from_numpy(np.minimum(i0 + 1, n_in - 1)), torch.from_numpy(w).to(dtype)

    y0, y1, wy = axis(H, out_hw[0])
    x0, x1, wx = axis(W, out_hw[1])
    v = v.to(dtype)
    top, bot = v[..., y0, :], v[..., y1, :]
    top = top[..., x0] + (top[..., x1] - top[..., x0]) * wx
    bot = bot[..., x0] + (bot[..., x1] - bot[..., x0]) * wx
    return top + (bot - top) * wy[:, None]


def ref_preprocess(videos_u8, dtype=torch.float64):
    """uint8 [N, T, C, H, W] -> [N, T, 224, 224, 3] in `dtype`: resize, one channel repeated, 2 v / 255 - 1"""
    v = ref_resize(videos_u8, (224, 224), dtype)
    if v.shape[2] == 1:
        v = v.repeat(1, 1, 3, 1, 1)
    return (2 * v / 255 - 1).permute(0, 1, 3, 4, 2).contiguous()


# ---------------------------------------------------------------------------------------------------- tolerance
def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def error_figures(got, ref):
    """(A, R) of a result against its float64 reference: A = the largest |got - ref| over the entries with
    |ref| < rms(ref), as a fraction of rms(ref) (logits and pre-ReLU sums cross zero: no relative figure exists there);
    R = the largest |got - ref| / |ref| over the other entries"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    s = rms(ref)
    err, small = (got - ref).abs(), ref.abs() < s
    a = float(err[small].max()) / s if small.any() else 0.0
    r = float((err[~small] / ref[~small].abs()).max()) if (~small).any() else 0.0
    return a, r


def bound(ref, A, R):
    """|got - ref| must stay under A rms(ref) + R |ref| entry by entry"""
    ref = ref.double()
    return A * rms(ref) + R * ref.abs()


# The GPU test cases (tests/test_i3d.py), with their inputs and float64 references computed once.
# unit cases: (unit, N, T, H, W); the unit fixes Cin -> Cout, k and stride
UNIT_CASES = (("Conv3d_1a_7x7", 2, 3, 5, 7), ("Conv3d_1a_7x7", 1, 4, 6, 8), ("Mixed_4b.b2b", 1, 1, 3, 3),
              ("Mixed_4c.b2b", 2, 2, 5, 5), ("Mixed_3b.b2a", 1, 2, 9, 9), ("Mixed_3b.b1a", 1, 2, 9, 9),
              ("logits", 1, 2, 3, 3))
TRUNK_SHAPE = (1, 9, 193, 193, 3)      # the smallest legal trunk input


def randn_map(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def layer_cases():
    """tuple of dicts (what, x channels-last float32, ref float64 channels-last) for the units, Mixed_3b and the head"""
    net, out = make_net(), []
    for j, (name, N, T, H, W) in enumerate(UNIT_CASES):
        cin = net[name]["w"].shape[1]
        x = randn_map((N, T, H, W, cin), 100 + j)
        out.append(dict(what=("unit", name), x=x, ref=cl(ref_unit(net, name, cf(x.double())))))
    x = randn_map((1, 2, 4, 4, 192), 200)
    out.append(dict(what=("mixed", "Mixed_3b"), x=x, ref=cl(ref_mixed(net, "Mixed_3b", cf(x.double())))))
    x = randn_map((2, 3, 7, 7, 1024), 201)
    out.append(dict(what=("head", None), x=x, ref=ref_head(net, cf(x.double()))))
    return tuple(out)


def layer_fp32(case):
    """the restatement of a layer case in float32 on the CPU"""
    net, (kind, name), x = make_net(), case["what"], cf(case["x"])
    if kind == "unit":
        return cl(ref_unit(net, name, x, torch.float32))
    if kind == "mixed":
        return cl(ref_mixed(net, name, x, torch.float32))
    return ref_head(net, x, torch.float32)


def fp32_layer_errors():
    """the worst (A, R) of the float32 CPU restatement over the layer cases"""
    figs = [error_figures(layer_fp32(c), c["ref"]) for c in layer_cases()]
    return max(f[0] for f in figs), max(f[1] for f in figs)


@functools.lru_cache(maxsize=None)
def trunk_case():
    """dict(x channels-last float32 uniform in [-1, 1), ref = the 400 float64 logits, seconds = time of the restatement)"""
    import time
    g = torch.Generator().manual_seed(300)
    x = torch.rand(TRUNK_SHAPE, generator=g) * 2 - 1
    t0 = time.time()
    ref = ref_logits(make_net(), x)
    return dict(x=x, ref=ref, seconds=time.time() - t0)


def fp32_trunk_errors():
    c = trunk_case()
    return error_figures(ref_logits(make_net(), c["x"], torch.float32), c["ref"])


# ---------------------------------------------------------------------------------------------------- SAME, sizes
def test_same_arithmetic_and_map_sizes():
    from rfn_hip import i3d as i3d_mod, ops
    assert same(224, 7, 2) == (112, 2, 3) and ops.i3d_same(224, 7, 2) == (112, 2)
    for n in (1, 2, 3, 5, 7, 8, 9, 193, 224):
        for k, s in ((1, 1), (2, 2), (3, 1), (3, 2), (7, 2)):
            assert ops.i3d_same(n, k, s) == same(n, k, s)[:2], (n, k, s)
    maps, main, scratch = ops.i3d_sizes(16, 224, 224)
    names = ["Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2c_3x3", "MaxPool3d_3a_3x3", "Mixed_3b",
             "Mixed_3c", "MaxPool3d_4a_3x3", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "MaxPool3d_5a_2x2",
             "Mixed_5b", "Mixed_5c"]
    got = dict(zip(names, maps))
    assert len(maps) == len(names)
    assert got["Conv3d_1a_7x7"] == (8, 112, 112, 64)
    assert got["MaxPool3d_2a_3x3"] == (8, 56, 56, 64)
    assert got["MaxPool3d_3a_3x3"] == (8, 28, 28, 192)
    assert got["MaxPool3d_4a_3x3"] == (4, 14, 14, 480)
    assert got["MaxPool3d_5a_2x2"] == (2, 7, 7, 832)
    for name, width in MIXED_OUT.items():
        assert got[name][3] == width and i3d_mod.mixed_width(name) == width, name
    assert main == 8 * 112 * 112 * 64
    assert scratch == (8 * 28 * 28 * 128, 8 * 28 * 28 * 32, 8 * 28 * 28 * 256)
    # the restatement agrees on the smallest legal input
    assert ops.i3d_sizes(9, 193, 193)[0][-1] == (2, 7, 7, 1024)


def test_block_widths_and_unit_table_match_the_definition():
    from rfn_hip import i3d as i3d_mod
    specs = unit_specs()
    assert len(specs) == 57 and len(i3d_mod.UNITS) == 58
    for name, (cin, cout, k, stride) in specs.items():
        u = i3d_mod.UNITS[name]
        assert (u["cin"], u["cout"], u["k"], u["stride"], u["relu"], u["bn"]) == (cin, cout, k, stride, True, True), name
    u = i3d_mod.UNITS["logits"]
    assert (u["cin"], u["cout"], u["k"], u["stride"], u["relu"], u["bn"]) == (1024, 400, 1, 1, False, False)
    for name, cin, (a, b, c, d, e, f) in MIXED:
        assert a + c + e + f == MIXED_OUT[name] and i3d_mod.MIXED[name] == (cin, (a, b, c, d, e, f))


def test_size_rules():
    from rfn_hip import ops
    with pytest.raises(ValueError, match="T must be at least 9"):
        ops.i3d_sizes(8, 224, 224)
    for side in (192, 225):
        with pytest.raises(ValueError, match=r"193\.\.224"):
            ops.i3d_sizes(9, side, 224)
        with pytest.raises(ValueError, match=r"193\.\.224"):
            ops.i3d_sizes(9, 224, side)
    for side in (193, 224):
        assert ops.i3d_sizes(9, side, side)[0][-1] == (2, 7, 7, 1024)
    assert ops.i3d_sizes(16, 200, 224)[0][-1] == (2, 7, 7, 1024)


def test_restatement_map_sizes_on_a_small_clip():
    """the restatement's own SAME arithmetic, on random weights: stage shapes at T = 9, 193 x 193 down to 2 x 7 x 7 would
    cost seconds, so the stem alone here (the trunk case of the GPU tests covers the rest)"""
    net = make_net()
    x = torch.zeros(1, 3, 4, 17, 18, dtype=torch.float64)
    y = ref_unit(net, "Conv3d_1a_7x7", x)
    assert tuple(y.shape) == (1, 64, 2, 9, 9)
    assert tuple(ref_pool(y, (1, 3, 3), (1, 2, 2)).shape) == (1, 64, 2, 5, 5)
    assert tuple(ref_pool(y, (3, 3, 3), (2, 2, 2)).shape) == (1, 64, 1, 5, 5)
    assert tuple(ref_pool(y, (2, 2, 2), (2, 2, 2)).shape) == (1, 64, 1, 5, 5)


# ---------------------------------------------------------------------------------------------------- resize
def test_legacy_resize_hand_values_and_convention():
    v = torch.tensor([[0., 10., 20.], [30., 40., 50.]])
    want = torch.tensor([[0., 5., 10., 15., 20., 20.], [15., 20., 25., 30., 35., 35.], [30., 35., 40., 45., 50., 50.],
                         [30., 35., 40., 45., 50., 50.]], dtype=torch.float64)
    got = ref_resize(v, (4, 6))
    assert torch.equal(got, want), got
    half_pixel = F.interpolate(v.double()[None, None], size=(4, 6), mode="bilinear", align_corners=False)[0, 0]
    assert float((half_pixel - want).abs().max()) >= 2.0       # F.interpolate's convention is another one
    # up-sampling 64 -> 224 keeps the corners and stays inside the range
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 256, (1, 1, 1, 64, 64), generator=g, dtype=torch.uint8)
    r = ref_resize(u, (224, 224))
    assert float(r[0, 0, 0, 0, 0]) == float(u[0, 0, 0, 0, 0]) and 0 <= float(r.min()) and float(r.max()) <= 255
    p = ref_preprocess(u)
    assert tuple(p.shape) == (1, 1, 224, 224, 3) and torch.equal(p[..., 0], p[..., 2])
    assert -1 <= float(p.min()) and float(p.max()) <= 1


# ---------------------------------------------------------------------------------------------------- BatchNorm fold
def test_batchnorm_fold_equals_conv_then_batchnorm():
    net = make_net()
    for name, shape in (("Mixed_4c.b2b", (2, 24, 2, 5, 5)), ("Conv3d_1a_7x7", (1, 3, 4, 9, 8))):
        p = {k: v.double() for k, v in net[name].items()}
        x = randn_map(shape, 7).double()
        k, stride = p["w"].shape[2], unit_specs()[name][3]
        g = p["gamma"] / torch.sqrt(p["var"] + EPS)
        wf, bf = p["w"] * g.view(-1, 1, 1, 1, 1), p["beta"] - p["mean"] * g
        folded = F.relu(F.conv3d(_pad(x, (k,) * 3, (stride,) * 3, 0.0), wf, bf, stride=stride))
        assert float((folded - ref_unit(net, name, x)).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------- loader
def _save_a(path, sd):
    torch.save(sd, path)


def _save_b(path, sd):
    np.savez(path, **{k: v.numpy() for k, v in sd.items()})


def test_loader_formats_agree_and_pack_layout(tmp_path):
    from rfn_hip import ops
    net = make_net()
    da, db, dq = tmp_path / "a", tmp_path / "b", tmp_path / "q"
    for d in (da, db, dq):
        d.mkdir()
    _save_a(da / "rgb_imagenet.pt", state_a(net))
    _save_b(db / "i3d.npz", state_b(net, gamma=True))
    _save_b(dq / "i3d.npz", state_b(net, gamma=True, quirk=True))
    wa = ops.i3d_load(str(da), "cpu")
    wb = ops.i3d_load([str(db / "i3d.npz")], "cpu")
    wq = ops.i3d_load(str(dq), "cpu")
    assert wa.data.dtype == torch.float32 and wa.layout == wb.layout == wq.layout
    assert torch.equal(wa.data, wb.data) and torch.equal(wa.data, wq.data)
    # a missing gamma means 1, in both formats
    ones = {k: dict(v, gamma=torch.ones_like(v["gamma"])) if "gamma" in v else v for k, v in net.items()}
    w1 = ops.i3d_pack(state_a(ones), "cpu")
    assert torch.equal(ops.i3d_pack(state_b(net, gamma=False), "cpu").data, w1.data)
    assert torch.equal(ops.i3d_pack(state_a(net, gamma=False), "cpu").data, w1.data)
    assert not torch.equal(w1.data, wa.data)
    # the two formats merge: the stem from a state dict, the rest from the TF names
    part_a = {k: v for k, v in state_a(net).items() if k.startswith("Conv3d_")}
    part_b = {k: v for k, v in state_b(net, gamma=True).items() if "/Conv3d_1a" not in k and "/Conv3d_2" not in k}
    assert torch.equal(ops.i3d_pack({**part_a, **part_b}, "cpu").data, wa.data)
    # layout: [Kpad][Coutpad], k = ((kt k + ky) k + kx) Cin + ci, folded in float64, zero padding
    end = 0
    for name, (wo, bo, kpad, cpad) in wa.layout.items():
        p = net[name]
        cout, cin, k = p["w"].shape[:3]
        K = cin * k ** 3
        assert wo == end and bo == wo + kpad * cpad and kpad == -(-K // 16) * 16 and cpad == -(-cout // 64) * 64, name
        end = bo + cpad
        if name in ("Conv3d_1a_7x7", "Mixed_4c.b2b", "Mixed_3b.b2a", "logits"):
            w, b = wa.unit(name)
            w = w.view(kpad, cpad)
            if name == "logits":
                wf, bf = p["w"].double(), p["b"].double()
            else:
                g = p["gamma"].double() / torch.sqrt(p["var"].double() + EPS)
                wf, bf = p["w"].double() * g.view(-1, 1, 1, 1, 1), p["beta"].double() - p["mean"].double() * g
            assert torch.equal(w[:K, :cout], wf.permute(2, 3, 4, 1, 0).reshape(K, cout).float()), name
            assert torch.equal(b[:cout], bf.float()), name
            assert (w[K:] == 0).all() and (w[:, cout:] == 0).all() and (b[cout:] == 0).all(), name
    assert end == wa.data.numel()
    assert wa.layout["Conv3d_1a_7x7"][2:] == (1040, 64) and wa.layout["Mixed_4c.b2b"][2:] == (656, 64)
    assert wa.layout["logits"][2:] == (1024, 448)


def test_loader_names_a_missing_or_misshaped_key(tmp_path):
    from rfn_hip import ops
    net = make_net()
    small = {k: v for k, v in net.items() if k.startswith("Conv3d_1a")}
    # one unit only: the next one's weight is named in both formats, with the files
    torch.save(state_a(small), tmp_path / "part.pt")
    with pytest.raises(ValueError, match=r"Conv3d_2b_1x1\.conv3d\.weight.*RGB/inception_i3d/Conv3d_2b_1x1/conv_3d/w.*part\.pt"):
        ops.i3d_load(str(tmp_path), "cpu")
    sd = state_a(net)
    del sd["Mixed_4e.b1b.bn.running_var"]
    with pytest.raises(ValueError, match=r"Mixed_4e\.b1b\.bn\.running_var \(expected shape \(288,\)\) is missing"):
        ops.i3d_pack(sd, "cpu")
    sd = state_a(net)
    sd["Mixed_3c.b2a.conv3d.weight"] = torch.zeros(32, 256, 1, 1)
    with pytest.raises(ValueError, match=r"Mixed_3c\.b2a\.conv3d\.weight has shape \(32, 256, 1, 1\), expected \(32, 256, 1, 1, 1\)"):
        ops.i3d_pack(sd, "cpu")
    sd = state_b(net)
    del sd["RGB/inception_i3d/Mixed_5b/Branch_2/Conv3d_0b_3x3/batch_norm/beta"]
    with pytest.raises(ValueError, match=r"Mixed_5b/Branch_2/Conv3d_0b_3x3/batch_norm/beta .*is missing"):
        ops.i3d_pack(sd, "cpu")
    sd = state_b(net)
    sd["RGB/inception_i3d/Logits/Conv3d_0c_1x1/conv_3d/b"] = torch.zeros(1, 400)
    with pytest.raises(ValueError, match=r"Logits/Conv3d_0c_1x1/conv_3d/b has shape \(1, 400\)"):
        ops.i3d_pack(sd, "cpu")


# ---------------------------------------------------------------------------------------------------- Frechet distance
def _cov(x):
    x = x - x.mean(0)
    return x.T @ x / (x.shape[0] - 1)


def test_frechet_identical_sets_rank_deficient():
    """n = 20 embeddings of dimension 400, as in real use: the covariance has rank 19"""
    from rfn_hip import ops
    x = np.random.default_rng(0).normal(size=(20, 400)) * 3 + 1
    d = ops.frechet_distance(x, x.copy())
    assert abs(d) <= 1e-6 * np.trace(_cov(x)), d
    assert abs(ops.frechet_distance(torch.from_numpy(x), torch.from_numpy(x).float().double())) <= 1e-6 * np.trace(_cov(x))


def test_frechet_closed_form_on_diagonal_covariances():
    """sets built to have exactly diagonal sample covariances diag(a) and diag(b) and means m_r, m_g: the distance is
    sum_i (sqrt a_i - sqrt b_i)^2 + |m_r - m_g|^2"""
    from rfn_hip import ops
    rng = np.random.default_rng(1)
    n, d = 40, 12
    q, _ = np.linalg.qr(rng.normal(size=(n, d + 1)))
    q = q[:, 1:] - q[:, 1:].mean(0)
    q, _ = np.linalg.qr(np.concatenate([np.ones((n, 1)), q], 1))
    basis = q[:, 1:] * math.sqrt(n - 1)               # centred columns, basis^T basis / (n - 1) = I
    a, b = rng.uniform(0.5, 4.0, d), rng.uniform(0.5, 4.0, d)
    m_r, m_g = rng.normal(size=d), rng.normal(size=d)
    real, fake = basis * np.sqrt(a) + m_r, basis * np.sqrt(b) + m_g
    assert np.allclose(_cov(real), np.diag(a), atol=1e-12) and np.allclose(real.mean(0), m_r, atol=1e-12)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((m_r - m_g) ** 2).sum()
    got = ops.frechet_distance(real, fake)
    assert abs(got - want) <= 1e-9 * want, (got, want)


def test_frechet_symmetric_and_refuses_small_sets():
    from rfn_hip import ops
    rng = np.random.default_rng(2)
    x, y = rng.normal(size=(20, 400)), rng.normal(size=(24, 400)) * 1.5 + 0.2
    d_xy, d_yx = ops.frechet_distance(x, y), ops.frechet_distance(y, x)
    assert d_xy > 0 and abs(d_xy - d_yx) <= 1e-9 * d_xy, (d_xy, d_yx)
    with pytest.raises(ValueError, match="at least 16"):
        ops.frechet_distance(x[:15], y)
    with pytest.raises(ValueError, match="at least 16"):
        ops.frechet_distance(x, y[:15])
    with pytest.raises(ValueError, match="dimension"):
        ops.frechet_distance(x, y[:, :399])


# ---------------------------------------------------------------------------------------------------- library, refusals
def test_library_exports_and_refuses_bad_arguments_before_any_launch():
    import ctypes
    from rfn_hip import lib
    L = lib.load()
    for name in ("rfn_i3d_same", "rfn_i3d_conv_pack_dims", "rfn_i3d_conv3d_f32", "rfn_i3d_maxpool3d_f32",
                 "rfn_i3d_resize_u8", "rfn_i3d_head_f32"):
        assert hasattr(L, name) and name in lib.SIGNATURES, name
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)   # never dereferenced
    big = 1 << 40
    # kernel side 5, stride 2 on a 1x1x1 kernel, columns past the pitch, buffers too small
    assert L.rfn_i3d_conv3d_f32(buf, big, 1, 2, 3, 3, 4, buf, big, buf, 8, 5, 1, 1, buf, big, 0, 8, None) != 0
    assert L.rfn_i3d_conv3d_f32(buf, big, 1, 2, 3, 3, 4, buf, big, buf, 8, 1, 2, 1, buf, big, 0, 8, None) != 0
    assert L.rfn_i3d_conv3d_f32(buf, big, 1, 2, 3, 3, 4, buf, big, buf, 8, 3, 1, 1, buf, big, 4, 8, None) != 0
    assert L.rfn_i3d_conv3d_f32(buf, 71, 1, 2, 3, 3, 4, buf, big, buf, 8, 3, 1, 1, buf, big, 0, 8, None) != 0
    assert L.rfn_i3d_conv3d_f32(buf, big, 1, 2, 3, 3, 4, buf, 112 * 64 - 1, buf, 8, 3, 1, 1, buf, big, 0, 8, None) != 0
    assert L.rfn_i3d_conv3d_f32(buf, big, 1, 2, 3, 3, 4, buf, big, buf, 8, 3, 1, 1, buf, 143, 0, 8, None) != 0
    assert b"rfn_i3d_conv3d_f32" in L.rfn_last_error()
    assert L.rfn_i3d_maxpool3d_f32(buf, big, 1, 2, 3, 3, 4, 1, 3, 2, 2, buf, big, None) != 0       # stride over the window
    assert L.rfn_i3d_maxpool3d_f32(buf, big, 1, 2, 3, 3, 4, 3, 3, 2, 2, buf, 15, None) != 0
    assert L.rfn_i3d_resize_u8(buf, 64, 1, 2, 8, 8, buf, big, None) != 0
    assert L.rfn_i3d_resize_u8(buf, 63, 1, 1, 8, 8, buf, big, None) != 0
    assert L.rfn_i3d_head_f32(buf, big, 1, 1, 49, 1024, buf, big, buf, 400, buf, None) != 0         # one time step
    assert L.rfn_i3d_head_f32(buf, big, 1, 2, 49, 1025, buf, big, buf, 400, buf, None) != 0
    # nothing to do is no launch
    assert L.rfn_i3d_conv3d_f32(None, 0, 0, 2, 3, 3, 4, None, 0, None, 8, 3, 1, 1, None, 0, 0, 8, None) == 0


def test_wrappers_refuse_bad_inputs():
    from rfn_hip import ops
    w = ops.i3d_pack(state_a(make_net()), "cpu")
    v = torch.zeros(2, 9, 1, 16, 16, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        ops.i3d_embed(w, v.float())
    with pytest.raises(ValueError, match="1 or 3 channels"):
        ops.i3d_embed(w, torch.zeros(2, 9, 2, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[N, T, C, H, W\]"):
        ops.i3d_embed(w, v[0])
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.i3d_embed(w, v)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.i3d_logits(w, torch.zeros(1, 9, 224, 224, 3))
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.i3d_unit(w, "Conv3d_2b_1x1", torch.zeros(1, 2, 3, 3, 64))


def test_evaluator_without_weights_refuses_fvd(monkeypatch):
    from evaluation_metrics import Evaluator
    from rfn_hip import ops
    loads = []
    monkeypatch.setattr(ops, "i3d_load", lambda *a, **k: loads.append(a))
    solver = SimpleNamespace(model=None, args=SimpleNamespace(n_frames=4), device=torch.device("cpu"))
    for settings in (None, SimpleNamespace(resample=2)):
        ev = Evaluator(solver, settings=settings)
        assert ev.fvd_weights is None
        with pytest.raises(RuntimeError, match="fvd_weights"):
            ev.get_fvd_values("rfn.pt", 9)
        assert ev._i3d is None
    assert loads == []
    ev = Evaluator(solver, settings=SimpleNamespace(fvd_weights="/some/where"))
    assert loads == [] and ev.fvd_weights == "/some/where"
