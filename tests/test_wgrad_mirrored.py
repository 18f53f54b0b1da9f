"""The mirrored 3x3 weight gradient of the coupling nets' last convolution (256 -> C, C = 4 / 8 / 16):
gw[co][ci][t] = sum_p go[co][p] h2[ci][p + t] = sum_q h2[ci][q] go[co][q - t], so h2 is the plain 256-row operand of the
implicit ring kernel and the C planes of go are shifted by the MIRRORED tap while staging -- one launch
(rfn_conv3x3_wgrad_mirrored[_grouped]_bf16x3) that writes [Cin][C][3][3], one transposing copy, and no tap-scattered
copy of go in memory.  Each case is the smallest shape at which one part of it can go wrong, against one fp64 F.conv2d
weight gradient per group on random (asymmetric) data at the bound the project holds these kernels to
(relerr < 2e-5, as test_wgrad_level_split.py and test_conv2d_wgrad_grouped): a tap left unmirrored or a transpose gone
wrong is an error of order 1.  The scatter + GEMM route (conv2d_wgrad_grouped / conv2d_wgrad) is held to the same bound
on the same data."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUERY = "rfn_conv3x3_wgrad_mirrored_kernel_label_bf16x3"
RING_64 = "gemm_wgrad_dma_impl_kernel<4,2,2,1>"      # 9 C <= 64 columns, two workgroups per CU
RING_128 = "gemm_wgrad_dma_impl_kernel<4,2,2,2>"     # 72 columns
RING_192 = "gemm_wgrad_dma_impl_kernel<4,2,2,3>"     # 144 columns
REG_128 = "gemm_wgrad_b3_kernel<2,2,2,2,64,1>"       # below the ring thresholds: register-staged
REG_256 = "gemm_wgrad_b3_kernel<4,2,2,3,64,1>"


def _label(Cin, h_ns, C, G, N, H, W):
    from rfn_hip import lib
    return getattr(lib.load(), QUERY)(Cin, h_ns, C, G, N, H, W).decode()


# ---------------------------------------------------------------------------------------------------- host only
# (Cin, channels of the tensor h2 is a slice of, C, G, N, H, W) -> label
LABELS = [
    ((256, 256, 4, 10, 608, 32, 32), RING_64),       # flow level 0
    ((256, 256, 8, 10, 608, 16, 16), RING_128),      # level 1
    ((256, 256, 16, 10, 608, 8, 8), RING_192),       # level 2
    ((256, 256, 4, 10, 76, 32, 32), RING_64),        # batch 4
    ((256, 256, 5, 3, 131, 16, 16), RING_64),        # 45 columns
    ((256, 256, 7, 3, 131, 16, 16), RING_64),        # 63 columns: the last that fit 64
    ((256, 256, 14, 3, 131, 16, 16), RING_128),      # 126 columns
    ((256, 256, 15, 3, 131, 16, 16), RING_192),      # 135
    ((200, 256, 4, 3, 131, 16, 16), RING_64),        # a channel slice, fewer rows than the tile
    ((256, 256, 4, 0, 391, 16, 16), RING_64),        # 100096 pixels: the smallest single launch on the ring
    ((256, 256, 4, 0, 390, 16, 16), REG_128),        # 99840 pixels: below it
    ((256, 256, 4, 3, 130, 16, 16), REG_128),        # G * pixels = 99840
    ((256, 256, 4, 16, 7, 16, 16), REG_128),         # pixels per group < 2048
    ((256, 256, 4, 0, 4200, 3, 8), REG_256),         # HW = 24: no whole 32-pixel stages, many pixels
    ((64, 64, 8, 0, 21, 8, 8), REG_128),
    ((128, 128, 4, 10, 608, 32, 32), REG_128),       # <= 128 rows: not the 256-row ring tile
    ((256, 256, 16, 10, 608, 4, 4), ""),             # rows of 4 pixels: no mirrored route
    ((256, 256, 4, 0, 50, 12, 12), ""),
]


@pytest.mark.parametrize("shape,label", LABELS)
def test_label_query(shape, label):
    Cin, Ctot, C, G, N, H, W = shape
    assert _label(Cin, Ctot * H * W, C, G, N, H, W) == label


def test_label_query_grouped_and_single_agree():
    """one group of F frames and a single launch of F frames are the same problem: the same kernel (ops.py adds the
    'grouped' prefix to the label of a grouped launch)"""
    for (Cin, Ctot, C, G, N, H, W), _ in LABELS:
        assert _label(Cin, Ctot * H * W, C, 1, N, H, W) == _label(Cin, Ctot * H * W, C, 0, N, H, W)


# ---------------------------------------------------------------------------------------------------- device
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert ops.bwd_b3(), "the ring kernels are the split-precision gradient path"
    return ops


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _profiled(fn):
    """fn() with the library's call profile on: (result, [(entry point, kernel label or shell name)] of all launches)"""
    from rfn_hip import lib
    old, lib.PROFILE = lib.PROFILE, []
    try:
        out = fn()
        torch.cuda.synchronize()
        calls = [(name, meta[1]) for (name, meta, _, _) in lib.PROFILE if meta is not None]
    finally:
        lib.PROFILE = old
    return out, calls


def _case(K, G, N, Cin, C, H, W, Ctot=None):
    """zeros_conv_wgrad_grouped (G >= 1) / zeros_conv_wgrad (G = 0) and the scatter + GEMM route on the same random data:
    (launches of the new route, launches of the old one, worst relerr of each over the groups, the queried label)"""
    Ctot = Ctot or Cin
    g = torch.Generator().manual_seed(7000 + 100 * G + N)
    n = max(G, 1)
    wide = [torch.randn(N, Ctot, H, W, generator=g) for _ in range(n)]
    go = torch.randn(n, N, C, H, W, generator=g)
    c0 = Ctot - Cin                                   # h2 = the LAST Cin channels: a base that is not the tensor's
    refs = []
    for i in range(n):
        w = torch.zeros(C, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(wide[i][:, c0:].double(), w, padding=1).backward(go[i].double())
        refs.append(w.grad)
    h2 = [t.cuda()[:, c0:] for t in wide]
    goc = go.cuda()
    gl = [goc[i] for i in range(n)]
    if G:
        new, calls = _profiled(lambda: K.zeros_conv_wgrad_grouped(h2, gl, C, g_stacked=goc))
        old, calls_old = _profiled(lambda: K.conv2d_wgrad_grouped(h2, None, gl, C, 3, g_stacked=goc))
    else:
        new, calls = _profiled(lambda: [K.zeros_conv_wgrad(h2[0], gl[0], C, 3)])
        old, calls_old = _profiled(lambda: [K.conv2d_wgrad(h2[0], None, gl[0], C, 3)])
    for t in new:
        assert tuple(t.shape) == (C, Cin, 3, 3) and t.is_contiguous()
    e_new = max(relerr(new[i], refs[i]) for i in range(n))
    e_old = max(relerr(old[i], refs[i]) for i in range(n))
    label = _label(Cin, Ctot * H * W, C, G, N, H, W)
    print("G%d N%d %d(of %d)->%d %dx%d: %s relerr %.3g | scatter + GEMM %s relerr %.3g" % (
        G, N, Cin, Ctot, C, H, W, calls, e_new, calls_old, e_old))
    return calls, calls_old, e_new, e_old, label


def _check_mirrored(K, G, N, Cin, C, H, W, want, Ctot=None):
    calls, calls_old, e_new, e_old, label = _case(K, G, N, Cin, C, H, W, Ctot)
    assert label == want
    entry = "rfn_conv3x3_wgrad_mirrored_grouped_bf16x3" if G else "rfn_conv3x3_wgrad_mirrored_bf16x3"
    wg = [c for c in calls if c[0] != "rfn_tap_scatter_f32" and "wgrad" in c[0]]
    assert wg == [(entry, label.replace("<", "<grouped ") if G else label)], calls
    assert not any(c[0] == "rfn_tap_scatter_f32" for c in calls), calls
    assert any(c[0] == "rfn_tap_scatter_f32" for c in calls_old), calls_old
    assert e_new < 2e-5, e_new
    assert e_old < 2e-5, e_old


def _crossings(G, n_stages, slots):
    """(workgroups per tile, workgroups whose range crosses a group boundary) of a grouped one-tile ring launch that may
    start `slots` workgroups: min(slots, G n_stages / 8), the rule of rfn_wgrad_split_workgroups with its 256 replaced"""
    from rfn_hip import lib
    Wt = min(slots, G * n_stages // 8)
    return Wt, sum(lib.load().rfn_wgrad_split_parts(G, n_stages, Wt, w, None, 0) > 1 for w in range(Wt))


@gpu
def test_narrow_tile_three_groups(K):
    """G = 3, 131 frames of 16x16, 256 -> 4: 36 columns, 1048 stages per group.  The narrow tile may start 512
    workgroups; the 8-stage minimum leaves 393 of 8 stages each, and the group boundaries are the edges of workgroups
    131 and 262: every workgroup starts in the right group at the right stage.  (On the 256 workgroups of the wider
    tiles this shape has both boundaries inside a range; the next test has them there for the narrow tile.)"""
    assert _crossings(3, 1048, 512) == (393, 0)
    _check_mirrored(K, 3, 131, 256, 4, 16, 16, RING_64)


@gpu
def test_narrow_tile_changes_group_inside_a_workgroup(K):
    """G = 5 of the same shape: 5240 stages over 512 workgroups, 10 or 11 each, boundary g at workgroup 102.4 g -- all
    four inside a workgroup's range (operand bases re-based, accumulators flushed and cleared in mid-range)"""
    assert _crossings(5, 1048, 512) == (512, 4)
    _check_mirrored(K, 5, 131, 256, 4, 16, 16, RING_64)


@gpu
def test_narrow_tile_32_pixel_rows(K):
    """G = 4, 25 frames of 32x32, 256 -> 4: a stage is one image row -- both edge elements of every row come from the
    edge masks, the first and last row of every frame from the row masks"""
    _check_mirrored(K, 4, 25, 256, 4, 32, 32, RING_64)


@gpu
def test_72_columns(K):
    _check_mirrored(K, 3, 131, 256, 8, 16, 16, RING_128)


@gpu
def test_144_columns_on_8x8(K):
    """G = 10, 160 frames of 8x8, 256 -> 16: a stage is four rows (half a frame), every stage touches a frame edge"""
    _check_mirrored(K, 10, 160, 256, 16, 8, 8, RING_192)


@gpu
def test_columns_that_do_not_fill_the_tile(K):
    """45 of 64 columns: the rows of the shifted operand past 9 C are zero and their products are not written"""
    _check_mirrored(K, 3, 131, 256, 5, 16, 16, RING_64)


@gpu
def test_fewer_rows_than_the_tile_from_a_channel_slice(K):
    """h2 = the last 200 channels of a 256-channel tensor: M < 256 (the DMA rows past M are clamped, their products not
    written), a frame stride that is not Cin HW and a base that is not the tensor's"""
    _check_mirrored(K, 3, 131, 200, 4, 16, 16, RING_64, Ctot=256)


@gpu
def test_ungrouped_smallest_ring_launch(K):
    """391 frames of 16x16, 256 -> 4: 100096 pixels, the smallest single launch on the ring (interleaved stages)"""
    _check_mirrored(K, 0, 391, 256, 4, 16, 16, RING_64)


@gpu
def test_channel_slice_of_a_wider_tensor_72_columns(K):
    _check_mirrored(K, 3, 131, 256, 8, 16, 16, RING_128, Ctot=264)


@gpu
def test_below_the_ring_thresholds(K):
    """21 frames of 8x8, 64 -> 8: the register-staged implicit kernel with the mirror flag, single and grouped"""
    _check_mirrored(K, 0, 21, 64, 8, 8, 8, REG_128)
    _check_mirrored(K, 3, 21, 64, 8, 8, 8, REG_128)


@gpu
def test_4x4_map_keeps_scatter_and_gemm(K):
    """rows of 4 pixels: the query names no kernel and the launches are the scatter + GEMM of conv2d_wgrad_grouped"""
    calls, calls_old, e_new, e_old, label = _case(K, 3, 40, 256, 16, 4, 4)
    assert label == ""
    assert calls == calls_old and calls[0] == ("rfn_tap_scatter_f32", "tap_scatter"), (calls, calls_old)
    assert e_new < 2e-5 and e_old < 2e-5, (e_new, e_old)


@gpu
def test_plan_is_what_runs_fp32_taps_and_unstacked_group(K, monkeypatch):
    """ops.wgrad_plan against execution on the two forms no other test pins launch by launch.  fp32 arithmetic,
    x [3, 16, 6, 6], C = 4: tap scatter + the fp32 kernel as a 1x1 conv to 36 channels, within 1e-4 of fp64 F.conv2d (the
    bound of test_tap_expanded_zeros_conv_fwd_wgrad).  Split precision, G = 2 gradients 20 -> 4 on 3 frames of 4x4 given
    as a list with no stacked buffer: a tap scatter each and one grouped GEMM, relerr < 2e-5."""
    def case(G, N, Cin, C, H, W, seed):
        g = torch.Generator().manual_seed(seed)
        n = max(G, 1)
        x, go = torch.randn(n, N, Cin, H, W, generator=g), torch.randn(n, N, C, H, W, generator=g)
        refs = []
        for i in range(n):
            w = torch.zeros(C, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
            F.conv2d(x[i].double(), w, padding=1).backward(go[i].double())
            refs.append(w.grad)
        xs, gos = [t.cuda() for t in x], [t.cuda() for t in go]   # separate allocations: nothing stacked
        plan = K.wgrad_plan(G, N, Cin, 0, C, H, W, 3, few_out=True)
        if G:
            got, calls = _profiled(lambda: K.zeros_conv_wgrad_grouped(xs, gos, C))
        else:
            got, calls = _profiled(lambda: [K.zeros_conv_wgrad(xs[0], gos[0], C, 3)])
        assert calls == plan.launches, (calls, plan)
        for t in got:
            assert tuple(t.shape) == (C, Cin, 3, 3) and t.is_contiguous()
        e = max(relerr(got[i], refs[i]) for i in range(n))
        print("G%d N%d %d->%d %dx%d: %s %s relerr %.3g" % (G, N, Cin, C, H, W, plan.form, calls, e))
        return plan, e

    plan, e = case(2, 3, 20, 4, 4, 4, 7100)
    assert plan.form == "scatter" and [name for name, _ in plan.launches] == [
        "rfn_tap_scatter_f32", "rfn_tap_scatter_f32", "rfn_gemm_wgrad_grouped_bf16x3"], plan
    assert e < 2e-5, e
    monkeypatch.setattr(K, "CONV_PRECISION", "f32")
    plan, e = case(0, 3, 16, 4, 6, 6, 7101)
    assert plan.form == "scatter_f32" and [name for name, _ in plan.launches] == [
        "rfn_tap_scatter_f32", "rfn_conv2d_wgrad_f32"], plan
    assert e < 1e-4, e


# ---- one level node end to end: the mirrored route against RFN_WGRAD_MIRRORED=0 (fresh child process)
LEVEL = dict(N=200, C=8, Cc=32, S=16, Kn=2, Hd=256)


def _level_param_grads(Kn=None):
    """parameter gradients of one GlowLevelFn node (K = 2 steps, 16x16 maps, 200 frames: pixels x K >= 100000) with
    deferred (grouped) weight gradients on seeded inputs, and all the launches of its backward"""
    from rfn_hip import ops as K
    N, C, Cc, S, Hd = (LEVEL[k] for k in ("N", "C", "Cc", "S", "Hd"))
    Kn = Kn or LEVEL["Kn"]
    Ch = C // 2
    g = torch.Generator().manual_seed(78)

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda().requires_grad_(True)

    x, cond = leaf(N, C, S, S), leaf(N, Cc, S, S)
    Wst = (torch.eye(C).expand(Kn, C, C) + 0.2 * torch.randn(Kn, C, C, generator=g)).cuda().requires_grad_(True)
    steps = []
    for _ in range(Kn):
        steps.append([leaf(1, C, 1, 1, scale=0.1), leaf(1, C, 1, 1, scale=0.1),
                      leaf(Hd, Ch + Cc, 3, 3, scale=0.05), leaf(1, Hd, 1, 1, scale=0.1), leaf(1, Hd, 1, 1, scale=0.1),
                      leaf(Hd, Hd, 1, 1, scale=0.05), leaf(1, Hd, 1, 1, scale=0.1), leaf(1, Hd, 1, 1, scale=0.1),
                      leaf(C, Hd, 3, 3, scale=0.02), leaf(C, scale=0.1), leaf(C, 1, 1, scale=0.1),
                      leaf(Ch, 1, 1, scale=0.5), leaf(Ch, 1, 1, scale=0.1)])
    plan = K.POPackPlan([(st[2].detach(), st[5].detach(), st[8].detach()) for st in steps])
    plan.run()
    packs = [K.StepPacks(po_fwd=plan.bufs[k], po_bwd=plan.bwd_bufs[k]) for k in range(Kn)]
    gout = torch.randn(N, C, S, S, generator=g).cuda()
    gdl = torch.randn(N, generator=g).cuda()
    out, dl = K.GlowLevelFn.apply(x, cond, Wst, K.ACT["leakyrelu"], K.CLAMP["realnvp"], packs,
                                  *[t for st in steps for t in st])
    _, calls = _profiled(lambda: ((out * gout).sum() + (dl * gdl).sum()).backward())
    return [t.grad.detach().cpu() for t in [Wst] + [t for st in steps for t in st]], calls


def _child_main(path):
    grads, calls = _level_param_grads()
    torch.save({"grads": grads, "calls": calls}, path)


@gpu
def test_level_node_takes_the_mirrored_launch_from_2_17_pixels(K, monkeypatch):
    """the level node's own rule (ops.level_mirrored_min_pixels, no knob set): K = 3 steps of 200 frames of 16x16 are
    153600 pixels -- one mirrored launch, no tap_scatter in the backward; K = 2 (102400 pixels, on the ring but below
    2^17) keeps tap scatter + GEMM, the route the level node had"""
    monkeypatch.delenv("RFN_WGRAD_MIRRORED_MIN_PIXELS", raising=False)
    assert K.level_mirrored_min_pixels() == 1 << 17
    _, calls = _level_param_grads(3)
    assert ("rfn_conv3x3_wgrad_mirrored_grouped_bf16x3", RING_128.replace("<", "<grouped ")) in calls, calls
    assert not any(name == "rfn_tap_scatter_f32" for name, _ in calls), calls
    _, calls = _level_param_grads(2)
    assert sum(name == "rfn_tap_scatter_f32" for name, _ in calls) == 1, calls
    assert not any("mirrored" in name for name, _ in calls), calls


@gpu
def test_level_node_mirrored_equals_scatter_and_gemm(K, tmp_path, monkeypatch):
    """the level node's conv3 gradients (one mirrored launch for the K steps, no tap_scatter in the backward's launch
    list) against the same node with RFN_WGRAD_MIRRORED=0 in a fresh child process (scatter + GEMM): within 2e-5
    relative -- both sum the same products in fp32, in another order.  K = 2 steps of 200 frames are 102400 pixels, on
    the ring but below the size from which the level node takes the mirrored launch by itself:
    RFN_WGRAD_MIRRORED_MIN_PIXELS=0 sends this small level through it."""
    assert os.environ.get("RFN_WGRAD_MIRRORED") != "0" and os.environ.get("RFN_WGRAD_GROUPED") != "0"
    monkeypatch.setenv("RFN_WGRAD_MIRRORED_MIN_PIXELS", "0")
    grads, calls = _level_param_grads()
    Kn = LEVEL["Kn"]
    assert ("rfn_conv3x3_wgrad_mirrored_grouped_bf16x3", RING_128.replace("<", "<grouped ")) in calls, calls
    assert not any(name == "rfn_tap_scatter_f32" for name, _ in calls), calls
    path = str(tmp_path / "scatter.pt")
    env = dict(os.environ, RFN_WGRAD_MIRRORED="0")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import tests.conftest; "
                        "from tests.test_wgrad_mirrored import _child_main; _child_main(%r)" % (ROOT, path)],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    old = torch.load(path, weights_only=False)
    assert any(name == "rfn_tap_scatter_f32" for name, _ in old["calls"]), old["calls"]
    assert not any("mirrored" in name for name, _ in old["calls"]), old["calls"]
    assert len(old["grads"]) == len(grads)
    worst = 0.0
    for k in range(Kn):
        i = 1 + 13 * k + 8                                # w3 of step k (after Wst, 13 parameters per step)
        assert tuple(grads[i].shape) == (LEVEL["C"], LEVEL["Hd"], 3, 3)
        e = relerr(grads[i], old["grads"][i])
        worst = max(worst, e)
        assert e < 2e-5, (k, e)
    for i, (a, b) in enumerate(zip(grads, old["grads"])):   # and nothing else moved
        assert relerr(a, b) < 2e-5, i
    print("level node, mirrored vs scatter + GEMM: worst conv3 relerr %.3g" % worst)
