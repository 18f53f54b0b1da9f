"""CPU tests of LPIPS on the AlexNet trunk (csrc/lpips.hip, rfn_hip/lpips.py, Evaluator.get_lpips): the float64
restatement that the GPU tests compare against checks itself (symmetry, zero on identical frames, one channel = three
identical channels, two hand-computed cases), the test inputs keep every tap visible in the sum, the loader reads the two
upstream namings from local files, the library exports and binds the entry points and answers the host-only size query,
and the wrappers and the Evaluator refuse what they cannot score.

No pretrained weights exist here: all weights are seeded random ones in the upstream key naming.  The restatement below is
test infrastructure: the product never imports it."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CHANNELS = (64, 192, 384, 256, 256)
# (index in torchvision's AlexNet.features, Cin, kernel size, stride, padding)
CONVS = ((0, 3, 11, 4, 2), (3, 64, 5, 1, 2), (6, 192, 3, 1, 1), (8, 384, 3, 1, 1), (10, 256, 3, 1, 1))
# (N, C, H, W) of the GPU tests: the smallest shapes at which each mechanism can go wrong (tests/test_lpips.py)
SHAPES = ((3, 1, 31, 31), (5, 3, 35, 47), (4, 1, 64, 64), (2, 3, 64, 64))


# ---------------------------------------------------------------------------------------------------- weights, inputs
def make_state(seed=0):
    """(alexnet state dict, lpips state dict) in the two upstream namings from a seeded generator: convolution weights
    randn * sqrt(2 / (Cin k k)), biases randn * 0.1, lin weights rand in [0, 1); plus keys the loader must ignore"""
    g = torch.Generator().manual_seed(seed)
    alex, lin = {}, {}
    for l, (idx, cin, ks, _, _) in enumerate(CONVS):
        cout = CHANNELS[l]
        alex["features.%d.weight" % idx] = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        alex["features.%d.bias" % idx] = torch.randn(cout, generator=g) * 0.1
    for l, c in enumerate(CHANNELS):
        lin["lin%d.model.1.weight" % l] = torch.rand(1, c, 1, 1, generator=g)
    alex["classifier.1.weight"] = torch.zeros(4, 9)
    alex["classifier.1.bias"] = torch.zeros(4)
    return alex, lin


@functools.lru_cache(maxsize=None)
def merged_state(seed=0):
    alex, lin = make_state(seed)
    return {**alex, **lin}


def make_pairs(N, C, H, W, seed):
    """uint8 frames a and b = clamp(a + randint(-40, 40)); pair 0 differs in one pixel by one grey level"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 256, (N, C, H, W), generator=g, dtype=torch.int64)
    b = (a + torch.randint(-40, 41, (N, C, H, W), generator=g)).clamp(0, 255)
    b[0] = a[0]
    v = int(a[0, C - 1, H // 2, W // 3])
    b[0, C - 1, H // 2, W // 3] = v + 1 if v < 255 else v - 1
    return a.to(torch.uint8), b.to(torch.uint8)


def edge_pairs(C, H, W, seed):
    """an identical pair, an all-0 frame against an all-255 frame, a constant frame against a random frame"""
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 256, (2, C, H, W), generator=g, dtype=torch.uint8)
    a = torch.stack([r[0], torch.zeros_like(r[0]), torch.full_like(r[0], 77)])
    b = torch.stack([r[0], torch.full_like(r[0], 255), r[1]])
    return a, b


# ---------------------------------------------------------------------------------------------------- restatement
def ref_features(state, x, dtype=torch.float64):
    """the five taps [N, C_l, H_l, W_l] of uint8 frames [N, C, H, W] (`lpips` 0.1.3, net='alex'), computed in `dtype`"""
    x = x.to(dtype)
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    x = x / 255 * 2 - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    taps = []
    for l, (idx, _, _, stride, pad) in enumerate(CONVS):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, state["features.%d.weight" % idx].to(dtype), state["features.%d.bias" % idx].to(dtype),
                            stride=stride, padding=pad))
        taps.append(x)
    return taps


def ref_lpips(state, a, b, dtype=torch.float64):
    """(per-tap values [N, 5], their sum [N]) of uint8 frames a, b [N, C, H, W], computed in `dtype` on the CPU"""
    fa, fb = ref_features(state, a, dtype), ref_features(state, b, dtype)
    taps = []
    for l, (x, y) in enumerate(zip(fa, fb)):
        nx = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + 1e-10)
        ny = y / (torch.sqrt((y * y).sum(1, keepdim=True)) + 1e-10)
        w = state["lin%d.model.1.weight" % l].to(dtype).view(1, -1, 1, 1)
        taps.append((w * (nx - ny) ** 2).sum(1).mean((1, 2)))
    taps = torch.stack(taps, 1)
    return taps, taps.sum(1)


@functools.lru_cache(maxsize=None)
def cases():
    """the inputs of the GPU tests with their float64 reference, computed once: a list of dicts (shape, a, b, taps, d)"""
    out = []
    for N, C, H, W in SHAPES:
        a, b = make_pairs(N, C, H, W, seed=N * 1000 + C * 100 + H + W)
        taps, d = ref_lpips(merged_state(), a, b)
        out.append(dict(shape=(N, C, H, W), a=a, b=b, taps=taps, d=d))
    return tuple(out)


def fp32_errors():
    """(largest absolute error on quantities with ref64 < 1e-5, largest relative error on quantities with ref64 >= 1e-3)
    of the restatement run in float32 on the CPU over cases(); the quantities are the per-tap values and their sums"""
    abs_small, rel_large = 0.0, 0.0
    for c in cases():
        taps32, d32 = ref_lpips(merged_state(), c["a"], c["b"], dtype=torch.float32)
        got = torch.cat([taps32.double(), d32.double()[:, None]], 1)
        ref = torch.cat([c["taps"], c["d"][:, None]], 1)
        err = (got - ref).abs()
        small, large = ref < 1e-5, ref >= 1e-3
        if small.any():
            abs_small = max(abs_small, float(err[small].max()))
        if large.any():
            rel_large = max(rel_large, float((err[large] / ref[large]).max()))
    return abs_small, rel_large


# ---------------------------------------------------------------------------------------------------- restatement checks
def test_restatement_symmetric_zero_on_identical_and_one_channel_is_three():
    st = merged_state()
    a, b = make_pairs(2, 1, 33, 40, seed=1)
    t_ab, d_ab = ref_lpips(st, a, b)
    t_ba, d_ba = ref_lpips(st, b, a)
    assert torch.equal(t_ab, t_ba) and torch.equal(d_ab, d_ba)
    assert (d_ab > 0).all()
    t_aa, d_aa = ref_lpips(st, a, a)
    assert (t_aa == 0).all() and (d_aa == 0).all()
    t3, d3 = ref_lpips(st, a.repeat(1, 3, 1, 1), b.repeat(1, 3, 1, 1))
    assert torch.equal(t3, t_ab) and torch.equal(d3, d_ab)


def _constant_state(bias):
    """all-zero convolution weights with a constant bias: every feature vector is bias * (1, ..., 1)"""
    st = dict(merged_state())
    for idx, _, _, _, _ in CONVS:
        st["features.%d.weight" % idx] = torch.zeros_like(st["features.%d.weight" % idx])
        st["features.%d.bias" % idx] = torch.full_like(st["features.%d.bias" % idx], bias)
    return st


def test_restatement_hand_case_constant_features():
    """zero weights and a constant bias make all normalised feature vectors equal: d = 0 for any two frames"""
    a, b = make_pairs(2, 3, 31, 37, seed=2)
    taps, d = ref_lpips(_constant_state(0.25), a, b)
    assert (taps == 0).all() and (d == 0).all()


def test_restatement_hand_case_delta_kernel():
    """first convolution: one weight 1 at (co 0, ci 0, ky 2, kx 2), no bias: channel 0 of tap 1 at (oy, ox) is
    relu(s(p[4 oy, 4 ox])), s(p) = ((p/255*2 - 1) + 0.030) / 0.458, every other channel 0.  With a all 255 and b 255 except
    0 at k of the P sampled pixels the normalised channel is 1 - 1e-10/s(255) against 0 there and equal elsewhere:
    d_1 = w_1[0] * (1 - 1e-10/s(255))^2 * k / P; the deeper taps see constant features and add 0."""
    st = _constant_state(0.5)
    st["features.0.bias"] = torch.zeros(64)
    w = torch.zeros(64, 3, 11, 11)
    w[0, 0, 2, 2] = 1.0
    st["features.0.weight"] = w
    H = W = 31                                   # tap 1 is 7x7: P = 49 sampled pixels (4 oy, 4 ox)
    a = torch.full((1, 3, H, W), 255, dtype=torch.uint8)
    b = a.clone()
    for oy, ox in ((0, 0), (3, 5), (6, 6)):
        b[0, 0, 4 * oy, 4 * ox] = 0
    b[0, 0, 1, 1] = 0                            # not sampled
    b[0, 1, 4, 4] = 0                            # another input channel
    taps, d = ref_lpips(st, a, b)
    s255 = (1.0 + 0.030) / 0.458
    want = float(st["lin0.model.1.weight"][0, 0, 0, 0]) * (1.0 - 1e-10 / s255) ** 2 * 3 / 49
    assert abs(float(taps[0, 0]) - want) <= 1e-14
    assert (taps[0, 1:] == 0).all() and abs(float(d[0]) - want) <= 1e-14


def test_every_tap_is_visible_in_the_test_inputs():
    """a condition on the inputs of the GPU tests, not on the kernel: every tap carries >= 2 % of d on every pair, so a
    dead tap cannot hide in the sum"""
    for c in cases():
        share = c["taps"] / c["d"][:, None]
        assert (c["d"] > 0).all() and float(share.min()) >= 0.02, (c["shape"], share.min(1).values)
        assert 1e-9 < float(c["d"][0]) < 1e-5 and (c["d"][1:] >= 1e-3).all(), (c["shape"], c["d"])


# ---------------------------------------------------------------------------------------------------- loader
def _save(tmp_path):
    alex, lin = make_state(0)
    pa, pl = tmp_path / "alexnet-owt-test.pth", tmp_path / "alex.pth"
    torch.save(alex, pa)
    torch.save(lin, pl)
    return alex, lin, pa, pl


def test_loader_reads_both_namings_and_round_trips(tmp_path):
    from rfn_hip import lib, ops
    alex, lin, pa, pl = _save(tmp_path)
    w_dir = ops.lpips_alex_load(str(tmp_path), "cpu")
    w_list = ops.lpips_alex_load([str(pl), pa], "cpu")
    assert torch.equal(w_dir.trunk, w_list.trunk) and torch.equal(w_dir.lin, w_list.lin)
    lay = (ctypes.c_longlong * 16)()
    assert lib.load().rfn_lpips_alex_weight_layout(ctypes.cast(lay, ctypes.c_void_p)) == 0
    assert w_dir.trunk.dtype == torch.float32 and w_dir.trunk.numel() == lay[15]
    assert list(lay[10:15]) == [368, 1600, 1728, 3456, 2304]
    end = 0
    for l, (idx, cin, ks, _, _) in enumerate(CONVS):
        cout, K = CHANNELS[l], cin * ks * ks
        assert lay[l] == end and lay[5 + l] == lay[l] + lay[10 + l] * cout
        end = lay[5 + l] + cout
        packed = w_dir.trunk[lay[l]:lay[5 + l]].view(lay[10 + l], cout)
        back = packed[:K].view(ks, ks, cin, cout).permute(3, 2, 0, 1)          # k = (ky*ks + kx)*Cin + ci
        assert torch.equal(back, alex["features.%d.weight" % idx])
        assert (packed[K:] == 0).all()
        assert torch.equal(w_dir.trunk[lay[5 + l]:lay[5 + l] + cout], alex["features.%d.bias" % idx])
    assert end == lay[15]
    assert torch.equal(w_dir.lin, torch.cat([lin["lin%d.model.1.weight" % l].reshape(-1) for l in range(5)]))


def test_loader_names_a_missing_or_misshaped_key(tmp_path):
    from rfn_hip import ops
    alex, lin, pa, pl = _save(tmp_path)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight.*alexnet-owt-test"):
        ops.lpips_alex_load([pa], "cpu")
    broken = dict(alex)
    del broken["features.6.bias"]
    torch.save(broken, pa)
    with pytest.raises(ValueError, match=r"features\.6\.bias is missing"):
        ops.lpips_alex_load(str(tmp_path), "cpu")
    broken = dict(lin)
    broken["lin3.model.1.weight"] = torch.zeros(256)
    torch.save(alex, pa)
    torch.save(broken, pl)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight has shape \(256,\)"):
        ops.lpips_alex_load(str(tmp_path), "cpu")


# ---------------------------------------------------------------------------------------------------- library
def test_library_exports_and_binds_lpips():
    from rfn_hip import lib
    L = lib.load()
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    want = {"rfn_lpips_alex_sizes": [i, i, p], "rfn_lpips_alex_weight_layout": [p],
            "rfn_lpips_alex_features_u8": [p, l, i, i, i, i, p, l, p, p, l, p],
            "rfn_lpips_alex_distance": [p, p, p, i, i, i, p, p, p]}
    for name, sig in want.items():
        assert hasattr(L, name) and lib.SIGNATURES[name] == sig, name


def test_sizes_query_needs_no_gpu():
    from rfn_hip import lib, ops
    L = lib.load()
    out = (ctypes.c_longlong * 12)()
    q = lambda H, W: L.rfn_lpips_alex_sizes(H, W, ctypes.cast(out, ctypes.c_void_p))
    for (H, W), maps in (((31, 31), ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1))),
                         ((35, 47), ((8, 11), (3, 5), (1, 2), (1, 2), (1, 2))),
                         ((64, 64), ((15, 15), (7, 7), (3, 3), (3, 3), (3, 3)))):
        assert q(H, W) == 0
        assert tuple((out[2 * k], out[2 * k + 1]) for k in range(5)) == maps
        assert out[10] == sum(h * w * c for (h, w), c in zip(maps, CHANNELS))
        assert ops.lpips_alex_sizes(H, W)[:2] == (maps, out[10])
    assert ops.lpips_alex_sizes(64, 64)[1] == 31872
    for H, W in ((30, 64), (64, 30)):
        assert q(H, W) != 0 and b"rfn_lpips_alex_sizes" in L.rfn_last_error()
        with pytest.raises(ValueError, match="31x31"):
            ops.lpips_alex_sizes(H, W)
    # the launching entry points answer argument errors before any launch
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)   # never dereferenced
    assert L.rfn_lpips_alex_features_u8(buf, 3 * 64 * 64, 1, 2, 64, 64, buf, 0, buf, buf, 0, None) != 0
    assert L.rfn_lpips_alex_features_u8(buf, 30 * 64, 1, 1, 30, 64, buf, 0, buf, buf, 0, None) != 0
    assert L.rfn_lpips_alex_features_u8(buf, 64 * 64, 1, 1, 64, 64, buf, 5, buf, buf, 1 << 20, None) != 0
    assert L.rfn_lpips_alex_distance(buf, buf, buf, 1, 64, 30, buf, buf, None) != 0
    assert L.rfn_lpips_alex_features_u8(None, 0, 0, 1, 64, 64, None, 0, None, None, 0, None) == 0


# ---------------------------------------------------------------------------------------------------- refusals
def test_wrappers_refuse_bad_inputs():
    from rfn_hip import ops
    w = ops.lpips_alex_pack(merged_state(), "cpu")
    a = torch.zeros(2, 1, 32, 32, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        ops.lpips_alex(w, a.float(), a.float())
    with pytest.raises(TypeError, match="uint8"):
        ops.lpips_alex_features(w, a.float())
    with pytest.raises(ValueError, match="shapes differ"):
        ops.lpips_alex(w, a, torch.zeros(2, 1, 32, 33, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 or 3 channels"):
        ops.lpips_alex_features(w, torch.zeros(2, 2, 32, 32, dtype=torch.uint8))
    for shape in ((2, 1, 30, 32), (2, 3, 32, 30)):
        small = torch.zeros(shape, dtype=torch.uint8)
        with pytest.raises(ValueError, match="31x31"):
            ops.lpips_alex(w, small, small)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.lpips_alex(w, a, a)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.lpips_alex_features(w, a)
    with pytest.raises(TypeError, match="lpips_alex_features"):
        ops.lpips_alex_distance(w, a, a)


def test_evaluator_without_weights_computes_no_lpips(monkeypatch):
    from evaluation_metrics import Evaluator
    from rfn_hip import ops
    loads = []
    monkeypatch.setattr(ops, "lpips_alex_load", lambda *a, **k: loads.append(a))
    solver = SimpleNamespace(model=None, args=SimpleNamespace(n_frames=4), device=torch.device("cpu"))
    for settings in (None, SimpleNamespace(resample=2)):
        ev = Evaluator(solver, settings=settings)
        assert ev.lpips_weights is None
        x = torch.zeros(2, 3, 1, 32, 32, dtype=torch.uint8)
        with pytest.raises(RuntimeError, match="lpips_weights"):
            ev.get_lpips(x, x)
        assert ev._lpips is None
    assert loads == []
    # with the setting, the weights are loaded once, on first use
    ev = Evaluator(solver, settings=SimpleNamespace(lpips_weights="/some/where"))
    assert loads == [] and ev.lpips_weights == "/some/where"
