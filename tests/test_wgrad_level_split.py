"""Grouped weight gradients on the LDS-DMA ring kernels with the even K split: the G groups' stages form one flat
range per output tile, every workgroup owns a contiguous share of it and changes group (operand bases, accumulator,
atomic flush) wherever its share crosses a group boundary.  Each case is the smallest shape at which that can go wrong,
against one fp64 F.conv2d weight gradient per group at the bound the project holds these kernels to (relerr < 2e-5, as
test_conv2d_wgrad_grouped).  On a ring route (G * pixels >= 100000, pixels >= 2048, HW % 32 == 0) a stage is 32 pixels of
a few hundred to a few thousand stages per group: one dropped, repeated or misattributed stage is an error of 1e-3 to
1e-2 for random data, far outside the bound."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RING_256 = "gemm_wgrad_dma_kernel<grouped 2,4,4,2,32,2>"
RING_64 = "gemm_wgrad_dma_kernel<grouped 1,8,2,1,32,3>"
RING_IMPL = "gemm_wgrad_dma_impl_kernel<grouped 4,2,2,3>"
B3_128 = "gemm_wgrad_b3_kernel<grouped 2,2,2,2,64>"


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
    """fn() with the library's call profile on: (result, [(entry point, kernel label)] of the weight-gradient launches)"""
    from rfn_hip import lib
    old, lib.PROFILE = lib.PROFILE, []
    try:
        out = fn()
        torch.cuda.synchronize()
        calls = [(name, meta[1]) for (name, meta, _, _) in lib.PROFILE if meta is not None and meta[0] == "wgrad"]
    finally:
        lib.PROFILE = old
    return out, calls


def _grouped_case(K, G, N, C1, C2, Cout, S, ks, slice_in1=False):
    """conv2d_wgrad_grouped on random data: (launch labels, worst relerr over the groups) against fp64 F.conv2d"""
    g = torch.Generator().manual_seed(1000 * G + N)
    wide = [torch.randn(N, 2 * C1 if slice_in1 else C1, S, S, generator=g) for _ in range(G)]
    in1 = [t[:, :C1] for t in wide]
    in2 = [torch.randn(N, C2, S, S, generator=g) for _ in range(G)] if C2 else None
    gy = torch.randn(G, N, Cout, S, S, generator=g)
    refs = []
    for i in range(G):
        xin = in1[i] if in2 is None else torch.cat((in1[i], in2[i]), 1)
        w = torch.zeros(Cout, C1 + C2, ks, ks, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin.double(), w, padding=ks // 2).backward(gy[i].double())
        refs.append(w.grad)
    gyc = gy.cuda()
    in1c = [t.cuda()[:, :C1] for t in wide]          # (slice_in1: a channel slice of a wider device tensor)
    in2c = None if in2 is None else [t.cuda() for t in in2]
    gws, calls = _profiled(lambda: K.conv2d_wgrad_grouped(in1c, in2c, [gyc[i] for i in range(G)], Cout, ks,
                                                          g_stacked=gyc))
    errs = [relerr(gws[i], refs[i]) for i in range(G)]
    print("G%d N%d %d+%d->%d %dx%d k%d: %s relerr max %.3g" % (G, N, C1, C2, Cout, S, S, ks, calls, max(errs)))
    return calls, errs


def _split(G, pixels, tiles):
    """(workgroups per tile, stages per group, workgroups that change group) of the grouped ring launch"""
    from rfn_hip import lib
    L = lib.load()
    n_stages = pixels // 32
    Wt = L.rfn_wgrad_split_workgroups(tiles, G, n_stages)
    crossing = sum(L.rfn_wgrad_split_parts(G, n_stages, Wt, w, None, 0) > 1 for w in range(Wt))
    return Wt, n_stages, crossing


def test_plain_ring_256x256(K):
    """G = 10, 40 frames of 16x16, 1x1 conv 256 -> 256: 320 stages per group, 3200 over 256 workgroups = 12.5 each.
    Boundary g lies at workgroup 25.6 g: inside a workgroup's range for every g but 5 (the edge of workgroup 128)."""
    assert _split(10, 40 * 256, 1) == (256, 320, 8)
    calls, errs = _grouped_case(K, 10, 40, 256, 0, 256, 16, 1)
    assert calls == [("rfn_gemm_wgrad_grouped_bf16x3", RING_256)]
    assert max(errs) < 2e-5, errs


def test_plain_ring_64_rows_tap_scattered(K):
    """G = 3, 131 frames of 16x16, 3x3 conv 256 -> 4: the tap-scattered 36 x 256 gradient through g_stacked on the
    three-slot ring with lookahead, 1048 stages per group (3144 over 256 workgroups: 12 or 13 each), both boundaries
    inside a workgroup's range"""
    assert _split(3, 131 * 256, 1) == (256, 1048, 2)
    calls, errs = _grouped_case(K, 3, 131, 256, 0, 4, 16, 3)
    assert calls == [("rfn_gemm_wgrad_grouped_bf16x3", RING_64)]
    assert max(errs) < 2e-5, errs


def test_implicit_ring_two_column_tiles(K):
    """G = 4, 100 frames of 16x16, in1 a channel slice (4 of 8) of a wider tensor, 32 conditioning channels, 256 output
    channels: 324 columns = two column tiles, Wt = 128 per tile, 25 stages per workgroup (boundaries at workgroups 32 g:
    each workgroup starts in the middle of the flat range, in the right group, and none changes group)"""
    assert _split(4, 100 * 256, 2) == (128, 800, 0)
    calls, errs = _grouped_case(K, 4, 100, 4, 32, 256, 16, 3, slice_in1=True)
    assert calls == [("rfn_conv3x3_wgrad_implicit_grouped_bf16x3", RING_IMPL)]
    assert max(errs) < 2e-5, errs


def test_implicit_ring_changes_group_inside_a_workgroup(K):
    """the same convolution with G = 3 and 131 frames: 1048 stages per group, 3144 over 128 workgroups per tile = 24 or
    25 each, both boundaries inside a workgroup's range (two workgroups per column tile re-base the gradient image, both
    input sources and the output, and flush twice)"""
    assert _split(3, 131 * 256, 2) == (128, 1048, 2)
    calls, errs = _grouped_case(K, 3, 131, 4, 32, 256, 16, 3, slice_in1=True)
    assert calls == [("rfn_conv3x3_wgrad_implicit_grouped_bf16x3", RING_IMPL)]
    assert max(errs) < 2e-5, errs


def test_most_groups_fewest_stages(K):
    """G = 16, 25 frames of 16x16, 256 x 256: 200 stages per group, the fewest a ring route allows, ranges of 12 - 13
    stages.  (With 16 groups over 256 workgroups every boundary is the edge of workgroup 16 g; 15 groups are next.)"""
    assert _split(16, 25 * 256, 1) == (256, 200, 0)
    calls, errs = _grouped_case(K, 16, 25, 256, 0, 256, 16, 1)
    assert calls == [("rfn_gemm_wgrad_grouped_bf16x3", RING_256)]
    assert max(errs) < 2e-5, errs


def test_fifteen_groups_boundaries_inside_workgroups(K):
    """G = 15, 27 frames of 16x16, 256 x 256: 216 stages per group, 3240 over 256 workgroups = 12 or 13 each, boundary g
    at workgroup 17.07 g: 13 of the 14 inside a workgroup's range (the floor puts one on an edge), at 13 different
    offsets"""
    assert _split(15, 27 * 256, 1) == (256, 216, 13)
    calls, errs = _grouped_case(K, 15, 27, 256, 0, 256, 16, 1)
    assert calls == [("rfn_gemm_wgrad_grouped_bf16x3", RING_256)]
    assert max(errs) < 2e-5, errs


def test_two_groups_64_frames(K):
    """G = 2, 256 x 256, 64 frames of 16x16: 512 stages per group; 256 workgroups would get 4 stages each, the 8-stage
    minimum gives Wt = 128 and 8 each, the boundary exactly at the edge of workgroup 64.  At G * pixels = 32768 < 100000
    the chooser does not take a ring route (no grouped ring launch has fewer than 12 stages per workgroup: fewer needs
    G * pixels < 65536), so what this shape pins is the label of the route it does take, a right result there, and the
    ring launcher's arithmetic for it; the same boundary-at-an-edge situation ON the ring is the next test."""
    assert _split(2, 64 * 256, 1) == (128, 512, 0)
    calls, errs = _grouped_case(K, 2, 64, 256, 0, 256, 16, 1)
    assert calls == [("rfn_gemm_wgrad_grouped_bf16x3", B3_128)]
    assert max(errs) < 2e-5, errs


def test_two_groups_boundary_at_a_workgroup_edge_on_the_ring(K):
    """G = 2, 256 x 256, 200 frames of 16x16 (G = 2 needs 196 frames for the ring): 1600 stages per group, 3200 over 256
    workgroups = 12.5 each, the boundary exactly between workgroups 127 and 128 -- no workgroup changes group, and the
    first stage of workgroup 128 is stage 0 of group 1"""
    assert _split(2, 200 * 256, 1) == (256, 1600, 0)
    calls, errs = _grouped_case(K, 2, 200, 256, 0, 256, 16, 1)
    assert calls == [("rfn_gemm_wgrad_grouped_bf16x3", RING_256)]
    assert max(errs) < 2e-5, errs


# ---- one level node end to end: grouped against one launch per step (fresh child process)
LEVEL = dict(N=140, C=8, Cc=32, S=16, Kn=3, Hd=256)


def _level_param_grads():
    """parameter gradients of one GlowLevelFn node (K = 3 steps, 16x16 maps, 140 frames: pixels x K >= 100000) on seeded
    inputs, with the fused coupling kernels as the trainer runs them, and the weight-gradient launches it made"""
    from rfn_hip import ops as K
    N, C, Cc, S, Kn, Hd = (LEVEL[k] for k in ("N", "C", "Cc", "S", "Kn", "Hd"))
    Ch = C // 2
    g = torch.Generator().manual_seed(77)

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


def test_level_node_grouped_equals_one_launch_per_step(K, tmp_path):
    """the level node with grouped weight gradients (three launches for the 3 K gradients, conv1 and conv2 on the ring
    kernels with the even split) against the same node with RFN_WGRAD_GROUPED=0 in a fresh child process (one launch
    per step and gradient): every parameter gradient within 2e-5 relative -- both runs sum the same products in fp32,
    in another order"""
    assert os.environ.get("RFN_WGRAD_GROUPED") != "0"
    grads, calls = _level_param_grads()
    Kn = LEVEL["Kn"]
    assert sorted(calls) == sorted([("rfn_conv3x3_wgrad_implicit_grouped_bf16x3", RING_IMPL),
                                    ("rfn_gemm_wgrad_grouped_bf16x3", RING_256),
                                    ("rfn_gemm_wgrad_grouped_bf16x3", B3_128)]), calls
    path = str(tmp_path / "single.pt")
    env = dict(os.environ, RFN_WGRAD_GROUPED="0")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import tests.conftest; "
                        "from tests.test_wgrad_level_split import _child_main; _child_main(%r)" % (ROOT, path)],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    single = torch.load(path, weights_only=False)
    assert len(single["calls"]) == 3 * Kn and not any("grouped" in n for n, _ in single["calls"]), single["calls"]
    assert len(single["grads"]) == len(grads)
    worst = 0.0
    for i, (a, b) in enumerate(zip(grads, single["grads"])):
        assert a.shape == b.shape
        e = relerr(a, b)
        worst = max(worst, e)
        assert e < 2e-5, (i, e)
    print("level node, grouped vs single launches: worst relerr %.3g over %d gradients" % (worst, len(grads)))
