"""The pointwise and reduction kernels of the recurrent and likelihood path, called directly, against fp64.

rfn_stepbn_{fwd,bwd,apply}_f32, rfn_convlstm_gates_{fwd,bwd}_f32, rfn_latent_step_{fwd,bwd}_f32,
rfn_gauss_{logp,logp_bwd,sample}_f32 and rfn_channel_stats_f32 through lib.call with ctypes arguments.  The shapes, the
route each is there for and the fp64 references (plain torch from the formulas of include/rfn_hip.h, autograd for the
backwards, each checked against an independent formulation) are in tests/test_recurrent_shell_host.py; the route labels
are printed here next to the measured errors.  References run on the CPU, except for the two BatchNorm rows above 4M
elements, where torch's own fp64 ops run on the device.

Every written output is a NaN-filled buffer (an unwritten element fails), views live in sentinel-filled parents that are
checked outside the view after the call, the accumulated logp starts nonzero, the BatchNorm scratch is NaN-filled with a
sentinel tail, and every BatchNorm / Gaussian launch runs twice and must repeat bit for bit (no atomics).

Bounds (the suite's, not fitted to the kernels):
  elementwise outputs     max|d| / max|ref| < 1e-5
  statistics              max|d| / max|ref| < 1e-5      (mean, biased var, running mean / var, channel stats)
  reduced gradients       max|d| / max|ref| < 1e-4      (ggamma, gbeta)
  sums of signed terms    |d| <= 1e-5 * A, A = the fp64 sum of the absolute values of the terms: the per-frame logp (A_n
                          includes the |logp| it is added to) and the elementwise KL (0.5 (r^2 + d^2 + 1 + |log r^2|))
  offset row              x = 1000 + randn: the fp32 mean is rounded to half an ulp of 1000, which moves every xhat of a
                          plane by up to 2^-24 * 1000 / std; y, gx and ggamma (a sum of g' xhat) get the derived term
                          2^-23 * max|mean| / min std added to their bound (gbeta, mean, var do not depend on it)
  exact                   x a multiple of 1/2 in [-2, 2], g of 1/8, no activation: every fp32 sum is exact in any order,
                          so gbeta is torch.equal to the fp64 value on every small row, and so is mean where B*HW is a
                          power of two (frame-to-block and partial-buffer indexing, bit for bit)
Where planted extreme values (softplus / sigmoid thresholds, saturated gates) dominate a tensor's largest magnitude, the
elementwise bound is also asserted over the remaining elements alone, with their own max|ref|.

Measured on an MI355X (max over the cases, activations and affine / plain launches of a row):
  per-step BatchNorm  (S x B x C x H x W; route)                                 elementwise  statistics  reduced
    3x4x6x8x8          ny=4  stats=vec    apply=vec4 grid=5     sweeps=1           3.1e-7       4.4e-7      1.3e-7
    2x3x5x3x5          ny=3  stats=scalar apply=vec1 grid=2     sweeps=1           4.7e-7       3.8e-7      2.4e-7
    5x2x16x2x2         ny=2  stats=vec    apply=vec4 grid=1     sweeps=1           2.9e-7       2.5e-7      1.9e-7
    2x37x8x4x4 plane   ny=16 stats=vec    apply=vec4 grid=10    sweeps=1           3.3e-7       5.5e-7      1.6e-7
    9x7x64x2x2         ny=3  stats=vec    apply=vec4 grid=16    sweeps=1           5.2e-7       6.1e-7      2.3e-7
    9x7x64x2x2 offset  ny=3  stats=vec    apply=vec4 grid=16    sweeps=1           1.2e-5       4.5e-7      1.9e-5
    9x5x256x2x2        ny=1  stats=vec    apply=vec4 grid=45    sweeps=1           5.8e-7       8.7e-7      1.7e-7
    9x5x256x1x2        ny=1  stats=scalar apply=vec1 grid=90    sweeps=1           6.6e-7       6.9e-7      1.7e-7
    3x4x6x8x8 y, gx off ny=4 stats=vec    apply=vec1 grid=18    sweeps=1           2.7e-7       4.6e-7      4.1e-7
    3x4x6x8x8 x off    ny=4  stats=scalar apply=vec1 grid=18    sweeps=1           1.4e-7       1.3e-7      1.4e-7
    2x8x65x128x128     ny=8  stats=vec    apply=vec4 grid=16384 sweeps=2           5.3e-7       1.0e-6      1.9e-7
    1x4x16x257x257     ny=4  stats=scalar apply=vec1 grid=16384 sweeps=2           2.6e-7       4.4e-7      2.6e-7
    (the offset row against 1e-5 / 1e-4 + the derived term, 2.0e-4 for its inputs: the plain 1e-5 does not hold there)
  synchronised  3x2x6x4x4 world 2 / 2x3x5x3x5 world 3 / 9x4x64x2x2 world 2         4.2e-7       6.1e-7      1.7e-7
  ConvLSTM gates  3x5x6 grid=1 / 4x60x64 grid=60 / 33x64x256 grid=2048 sweeps=2    2.0e-7 (with and without peepholes)
  latent step     3x28 grid=1 / 5x63 grid=2 / 4x66000 grid=1024 sweeps=2           2.4e-7 whole tensors, 2.8e-7 without
                                                                                   the planted elements; KL / A 4.5e-7
  Gaussian        five rows x two layouts x two std modes x two regimes            2.4e-7, logp / A_n 3.4e-7 (70x2x16)
  channel stats   7x5x18, 5x3x100, 2x4x4096, dense and sliced                                   1.1e-7
  The exact tests hold on all seven small rows; every repeated launch was bit-identical.
  Wall time of the module on the MI355X machine: 4 s for 96 tests, the slowest (2x8x65x128x128, with its fp64 reference
  on the device) 0.8 s.
"""
import ctypes

import pytest
import torch

from tests.test_glow_shell import NAN, SENT, untouched, view_of
from tests.test_recurrent_shell_host import (ACTS, BN_EPS, BN_MOMENTUM, BN_ROWS, GATES_CASES, GAUSS_CASES, LATENT_CASES,
                                             STATS_CASES, SYNC_ROWS, Bag, bn_aligned_mask, bn_id, bn_inputs, bn_label,
                                             bn_ref, bn_sync_ref, channel_stats_ref, ema_ref, gates_label, gates_ref,
                                             gauss_ref, gauss_sample_ref, latent_label, latent_ref, sync_inputs)

pytestmark = pytest.mark.gpu

_i, _l, _f = ctypes.c_int, ctypes.c_long, ctypes.c_float
EW_BOUND, STAT_BOUND, RED_BOUND, SUM_BOUND = 1e-5, 1e-5, 1e-4, 1e-5
ids = lambda c: "x".join(map(str, c))


@pytest.fixture(scope="module")
def L():
    from rfn_hip import lib
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return lib


# ------------------------------------------------------------------------------------------------ helpers
def relerr(got, ref, mask=None):
    """max|got - ref| / max|ref| in fp64 on the device of ref (NaN if anything was left unwritten); mask selects elements"""
    ref = ref.detach()
    d = (got.detach().to(ref.device).double() - ref).abs()
    a = ref.abs()
    if mask is not None:
        d, a = d[mask], a[mask]
    return float(d.max() / a.max().clamp_min(1e-300))


def nan_buf(shape, off=0):
    """a NaN-filled device tensor of `shape` whose first element is `off` floats past a 16-byte boundary"""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((n + 4,), NAN, device="cuda", dtype=torch.float32)
    return flat[off:off + n].view(shape)


def put(t, off=0):
    """a CPU tensor on the device, `off` floats past a 16-byte boundary"""
    b = nan_buf(tuple(t.shape), off)
    b.copy_(t)
    return b


def aligned_bits(stats_ptrs, apply_ptrs):
    m = lambda ts: all(t.data_ptr() % 16 == 0 for t in ts)
    return (1 if m(stats_ptrs) else 0) | (2 if m(apply_ptrs) else 0)


def scratch(L, S, B, C):
    """NaN-filled scratch of exactly rfn_stepbn_scratch_floats + a sentinel tail -> (whole, n)"""
    n = int(L.load().rfn_stepbn_scratch_floats(S, B, C))
    buf = torch.full((n + 8,), NAN, device="cuda", dtype=torch.float32)
    buf[n:] = SENT
    return buf, n


def tail_ok(buf, n):
    return bool((buf[n:] == SENT).all()) and not bool(torch.isnan(buf[:n]).any())


# ------------------------------------------------------------------------------------------------ per-step BatchNorm
def bn_launch(L, I, x, g, affine, act, slope, mis, running=True):
    """forward + backward of one layer into fresh NaN-filled outputs -> Bag of device tensors"""
    from Utils.modules import _ema_coef
    S, B, C, HW = I.S, I.B, I.C, I.HW
    oy = 1 if mis == "y" else 0
    y, gx = nan_buf(tuple(x.shape), oy), nan_buf(tuple(x.shape), oy)
    mean, var = nan_buf((S, C)), nan_buf((S, C))
    gamma, beta = (I.gamma.cuda(), I.beta.cuda()) if affine else (None, None)
    acc, n = scratch(L, S, B, C)
    rm = rv = cf = cfu = nbt = None
    decay = 1.0
    if running:
        rm, rv = I.rm.cuda(), I.rv.cuda()
        cf, cfu = _ema_coef(S, BN_MOMENTUM, B * HW, x.device)
        decay = (1.0 - BN_MOMENTUM) ** S
        nbt = torch.full((1,), I.nbt, device="cuda", dtype=torch.int64)
    masks = (aligned_bits([x], [x, y]), aligned_bits([x, g], [x, g, gx]))
    L.call("rfn_stepbn_fwd_f32", L.dev(x), L.dev(gamma), L.dev(beta), L.dev(y), L.dev(mean), L.dev(var), L.dev(acc),
           L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cfu), _f(decay), None if nbt is None else ctypes.c_void_p(nbt.data_ptr()),
           _i(S), _i(B), _i(C), _i(HW), _f(BN_EPS), _i(act), _f(slope))
    sums, _ = scratch(L, S, B, C)
    ggamma, gbeta = (nan_buf((C,)), nan_buf((C,))) if affine else (None, None)
    L.call("rfn_stepbn_bwd_f32", L.dev(x), L.dev(gamma), L.dev(beta), L.dev(g), L.dev(mean), L.dev(var), L.dev(sums),
           L.dev(gx), L.dev(ggamma), L.dev(gbeta), _i(S), _i(B), _i(C), _i(HW), _f(BN_EPS), _i(act), _f(slope), _i(0), _i(1))
    torch.cuda.synchronize()
    return Bag(y=y, gx=gx, mean=mean, var=var, ggamma=ggamma, gbeta=gbeta, rm=rm, rv=rv, nbt=nbt, masks=masks,
               scratch_ok=tail_ok(acc, n) and tail_ok(sums, n))


def bn_same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in ("y", "gx", "mean", "var", "ggamma",
                                                                                    "gbeta", "rm", "rv", "nbt"))


@pytest.fixture(scope="module")
def bn_row_inputs():
    cache = {}

    def get(row):
        k = bn_id(row)
        if k not in cache:
            cache.clear()           # rows arrive grouped: one row's inputs at a time (the large rows are 2 x 68 MB)
            I = bn_inputs(row)
            ox = 1 if row["mis"] == "x" else 0
            cache[k] = (I, put(I.x, ox), put(I.g))
        return cache[k]
    return get


@pytest.mark.parametrize("affine", (True, False), ids=("affine", "plain"))
@pytest.mark.parametrize("row", BN_ROWS, ids=bn_id)
def test_batchnorm_vs_fp64(L, bn_row_inputs, row, affine):
    I, x, g = bn_row_inputs(row)
    big = bool(row.get("big"))
    xr, gr = (x, g) if big else (I.x, I.g)                 # the reference's device
    ga, be = (I.gamma.to(xr.device), I.beta.to(xr.device)) if affine else (None, None)
    n = I.B * I.HW
    for a in row["acts"]:
        act, slope = ACTS[a]
        got = bn_launch(L, I, x, g, affine, act, slope, row["mis"])
        again = bn_launch(L, I, x, g, affine, act, slope, row["mis"])
        ref = bn_ref(xr, ga, be, gr, I.S, act, slope)
        extra = 0.0
        if row.get("kind") == "offset":     # a rounded fp32 mean moves xhat: see the module docstring
            extra = 2.0 ** -23 * float(ref.mean.abs().max()) / float(ref.var.min().sqrt())
        e = Bag(y=relerr(got.y, ref.y), gx=relerr(got.gx, ref.gx), mean=relerr(got.mean, ref.mean),
                var=relerr(got.var, ref.var))
        if affine:
            e.update(ggamma=relerr(got.ggamma, ref.ggamma), gbeta=relerr(got.gbeta, ref.gbeta))
        rm, rv = ema_ref(ref.mean, ref.var, n, I.rm.to(xr.device), I.rv.to(xr.device))
        e.update(rm=relerr(got.rm, rm), rv=relerr(got.rv, rv))
        print("\nBN %s %s act=%s %s | %s" % (bn_id(row), "affine" if affine else "plain", a, bn_label(L, row),
                                           " ".join("%s %.1e" % kv for kv in e.items())))
        assert got.masks == (bn_aligned_mask(row),) * 2, got.masks      # the route the label was asked about
        assert got.scratch_ok, "a partial sum was left unwritten, or the scratch was overrun"
        assert e.y < EW_BOUND + extra and e.gx < EW_BOUND + extra, e
        assert e.mean < STAT_BOUND and e.var < STAT_BOUND and e.rm < STAT_BOUND and e.rv < STAT_BOUND, e
        if affine:
            assert e.ggamma < RED_BOUND + extra and e.gbeta < RED_BOUND, e
        assert int(got.nbt) == I.nbt + I.S
        assert bn_same_bits(got, again), "two runs differ"
        if row.get("kind") == "plane":
            assert float(got.var[I.S - 1, I.C // 2]) == 0.0 and float(ref.var[I.S - 1, I.C // 2]) == 0.0
            assert bool(torch.isfinite(got.gx).all()) and bool(torch.isfinite(got.y).all())
    # without running statistics the same launch leaves everything else as it was
    if not big:
        plain = bn_launch(L, I, x, g, affine, act, slope, row["mis"], running=False)
        assert torch.equal(plain.y, got.y) and torch.equal(plain.mean, got.mean) and torch.equal(plain.gx, got.gx)


@pytest.mark.parametrize("row", [r for r in BN_ROWS if not r.get("big") and not r.get("kind")], ids=bn_id)
def test_batchnorm_sums_are_exact_on_dyadic_inputs(L, row):
    """x a multiple of 1/2 in [-2, 2], g of 1/8 in [-1, 1], no activation: gbeta = sum g is exact in any order, and so
    is mean = K + sum(x - K) / (B HW) where B HW is a power of two; every frame has its own values, so a wrong frame,
    block or partial index moves a sum"""
    I = bn_inputs(dict(row, kind="dyadic"))
    x, g = put(I.x, 1 if row["mis"] == "x" else 0), put(I.g)
    got = bn_launch(L, I, x, g, True, 0, 0.0, row["mis"])
    n = I.B * I.HW
    xv = I.x.double().view(I.S, I.B, I.C, I.HW)
    gbeta = I.g.double().sum((0, 2, 3))
    assert torch.equal(got.gbeta.cpu().double(), gbeta), (got.gbeta.cpu().double() - gbeta).abs().max()
    if n & (n - 1) == 0:
        mean = xv.sum((1, 3)) / n
        assert torch.equal(mean.float().double(), mean)                      # representable: the test's own premise
        assert torch.equal(got.mean.cpu().double(), mean), (got.mean.cpu().double() - mean).abs().max()
    else:
        assert relerr(got.mean, xv.mean((1, 3))) < 1e-6
    assert got.scratch_ok


@pytest.mark.parametrize("affine", (True, False), ids=("affine", "plain"))
@pytest.mark.parametrize("row", SYNC_ROWS, ids=lambda r: ids(r["shape"]) + "-w%d" % r["world"])
def test_synchronised_batchnorm_vs_fp64_on_the_global_batch(L, row, affine):
    """`world` ranks emulated in one process, step for step as StepBatchNormActFn._forward_sync / backward do: local
    moments (rfn_stepbn_fwd_f32), the host's equal-count combination, rfn_stepbn_apply_f32 with the given statistics;
    stage 1 per rank, the sums added over the ranks, stage 2 with `world`"""
    ranks, gamma, beta = sync_inputs(row)
    S, B, C, H, W = row["shape"]
    HW, world = H * W, row["world"]
    act, slope = ACTS[row["act"]]
    ga, be = (gamma.cuda(), beta.cuda()) if affine else (None, None)
    xs, gs = [put(I.x) for I in ranks], [put(I.g) for I in ranks]
    stats = []
    for x in xs:
        y, mean, var = nan_buf(tuple(x.shape)), nan_buf((S, C)), nan_buf((S, C))
        acc, n = scratch(L, S, B, C)
        L.call("rfn_stepbn_fwd_f32", L.dev(x), L.dev(ga), L.dev(be), L.dev(y), L.dev(mean), L.dev(var), L.dev(acc), None,
               None, None, None, _f(1.0), None, _i(S), _i(B), _i(C), _i(HW), _f(BN_EPS), _i(act), _f(slope))
        stats.append(torch.stack((mean, var)))
    st = torch.stack(stats)                                                    # [world, 2, S, C]
    mean = st[:, 0].mean(0).contiguous()
    var = (st[:, 1].mean(0) + (st[:, 0] - mean).pow(2).mean(0)).contiguous()
    ys, sums = [], []
    for x, g in zip(xs, gs):
        y = nan_buf(tuple(x.shape))
        L.call("rfn_stepbn_apply_f32", L.dev(x), L.dev(ga), L.dev(be), L.dev(y), L.dev(mean), L.dev(var), _i(S), _i(B),
               _i(C), _i(HW), _f(BN_EPS), _i(act), _f(slope))
        ys.append(y)
        sm, n = scratch(L, S, B, C)
        sums.append(sm)
    out = [Bag(gx=nan_buf(tuple(x.shape)), ggamma=nan_buf((C,)) if affine else None,
               gbeta=nan_buf((C,)) if affine else None) for x in xs]
    args = lambda k: (L.dev(xs[k]), L.dev(ga), L.dev(be), L.dev(gs[k]), L.dev(mean), L.dev(var), L.dev(sums[k]),
                      L.dev(out[k].gx), L.dev(out[k].ggamma), L.dev(out[k].gbeta), _i(S), _i(B), _i(C), _i(HW), _f(BN_EPS),
                      _i(act), _f(slope))
    for k in range(world):
        L.call("rfn_stepbn_bwd_f32", *args(k), _i(1), _i(world))
    torch.cuda.synchronize()
    assert all(tail_ok(sm, n) for sm in sums) and all(bool(torch.isnan(o.gx).all()) for o in out)   # stage 1 writes no gx
    total = torch.stack([sm[:n] for sm in sums]).sum(0)                        # the all-reduce
    for sm in sums:
        sm[:n] = total
    for k in range(world):
        L.call("rfn_stepbn_bwd_f32", *args(k), _i(2), _i(world))
    torch.cuda.synchronize()
    ref = bn_sync_ref([I.x for I in ranks], gamma if affine else None, beta if affine else None, [I.g for I in ranks], S,
                      act, slope)
    e = Bag(mean=relerr(mean, ref.mean), var=relerr(var, ref.var), y=max(relerr(ys[k], ref.y[k]) for k in range(world)),
            gx=max(relerr(out[k].gx, ref.gx[k]) for k in range(world)))
    if affine:
        e.update(ggamma=max(relerr(o.ggamma, ref.ggamma / world) for o in out),
                 gbeta=max(relerr(o.gbeta, ref.gbeta / world) for o in out))
    print("\nSYNC %s world=%d %s | %s" % (ids(row["shape"]), world, "affine" if affine else "plain",
                                        " ".join("%s %.1e" % kv for kv in e.items())))
    assert e.mean < STAT_BOUND and e.var < STAT_BOUND and e.y < EW_BOUND and e.gx < EW_BOUND, e
    if affine:
        assert e.ggamma < RED_BOUND and e.gbeta < RED_BOUND, e


# ------------------------------------------------------------------------------------------------ ConvLSTM gates
def gates_inputs(case):
    N, Hc, HW = case
    gen = torch.Generator().manual_seed(400 + list(GATES_CASES).index(case))
    r = lambda *s: torch.randn(*s, generator=gen)
    cc = 2 * r(N, 4 * Hc, HW)
    flat = cc.view(-1)
    pos = torch.randperm(flat.numel(), generator=gen)[:8]
    flat[pos[:4]], flat[pos[4:]] = 30.0, -30.0               # saturated gates
    sat = torch.zeros(N * 4 * Hc * HW, dtype=torch.bool)
    sat[pos] = True
    return Bag(N=N, Hc=Hc, HW=HW, cc=cc, c_prev=r(N, Hc, HW), gh=r(N, Hc, HW), gc=r(N, Hc, HW),
               pe=[0.5 * r(Hc * HW) for _ in range(3)], sat=sat.view(N, 4, Hc * HW).any(1).view(N, Hc, HW))


@pytest.mark.parametrize("pe", (False, True), ids=("nopeephole", "peephole"))
@pytest.mark.parametrize("case", list(GATES_CASES), ids=ids)
def test_convlstm_gates_vs_fp64(L, case, pe):
    I = gates_inputs(case)
    N, Hc, HW = case
    wc = I.pe if pe else [None, None, None]
    wcd = [None if t is None else t.cuda() for t in wc]
    cc = I.cc.cuda()
    cppar, cp = view_of(I.c_prev)
    cpp, cpns = L.frames(cp, "c_prev")
    leaves = [I.cc.double().requires_grad_(), I.c_prev.double().requires_grad_()]
    h64, c64, g64 = gates_ref(leaves[0], leaves[1], *[None if t is None else t.double() for t in wc])
    e = Bag()
    for with_gates in (True, False):
        hpar, h = view_of((N, Hc, HW))
        copar, co = view_of((N, Hc, HW))
        gates = nan_buf((N, 4 * Hc, HW)) if with_gates else None
        hp, hns = L.frames(h, "h_out")
        cop, cons = L.frames(co, "c_out")
        L.call("rfn_convlstm_gates_fwd_f32", L.dev(cc), cpp, _l(cpns), *[L.dev(t) for t in wcd], hp, _l(hns), cop,
               _l(cons), L.dev(gates), _i(N), _i(Hc), _i(HW))
        torch.cuda.synchronize()
        assert untouched(hpar) and untouched(copar) and untouched(cppar), "wrote outside a channel slice"
        k = "" if with_gates else "(no gates)"
        e["h" + k], e["c" + k] = relerr(h, h64), relerr(co, c64)
        if with_gates:
            e["gates"] = relerr(gates, g64)
    # backward: the saved gates and c_out are the fp64 reference's, rounded, not the kernel's own
    gates_in, (c_par, c_in) = g64.detach().float().cuda(), view_of(c64.detach().float())
    cip, cins = L.frames(c_in, "c_out")
    rest = ~I.sat
    for name, use_gh, use_gc in (("both", True, True), ("gh", True, False), ("gc", False, True)):
        loss = (h64 * I.gh.double()).sum() * (1 if use_gh else 0) + (c64 * I.gc.double()).sum() * (1 if use_gc else 0)
        gcc64, gcp64 = torch.autograd.grad(loss, leaves, retain_graph=True)
        (ghpar, gh), (gcpar, gc) = view_of(I.gh), view_of(I.gc)
        gppar, gcp = view_of((N, Hc, HW))
        gcc = nan_buf((N, 4 * Hc, HW))
        ghp, ghns = L.frames(gh, "gh") if use_gh else (None, 0)
        gcnp, gcns = L.frames(gc, "gc_next") if use_gc else (None, 0)
        gpp, gpns = L.frames(gcp, "gc_prev")
        L.call("rfn_convlstm_gates_bwd_f32", L.dev(gates_in), cpp, _l(cpns), cip, _l(cins), ghp, _l(ghns), gcnp, _l(gcns),
               *[L.dev(t) for t in wcd], L.dev(gcc), gpp, _l(gpns), _i(N), _i(Hc), _i(HW))
        torch.cuda.synchronize()
        assert all(untouched(p) for p in (gppar, ghpar, gcpar, c_par, cppar)), "wrote outside a channel slice"
        e["gcc:" + name], e["gc_prev:" + name] = relerr(gcc, gcc64), relerr(gcp, gcp64)
        e["gc_prev:" + name + "/rest"] = relerr(gcp, gcp64, rest)
    print("\nGATES %s %s %s | %s" % (ids(case), "peephole" if pe else "nopeephole", gates_label(L, *case),
                                   " ".join("%s %.1e" % kv for kv in e.items())))
    for k, v in e.items():
        assert v < EW_BOUND, (k, v)


# ------------------------------------------------------------------------------------------------ latent step
LATENT_SUBSETS = {"all": (0, 1, 2, 3, 4), "kl_only": (2,), "no_kl": (0, 1, 3, 4), "zt_only": (0,)}
PLANTED = (-15.0, 19.9, 20.1, 30.0)                 # softplus / sigmoid thresholds of the raw scales
PAD = 37                                            # g_zt / g_zxt row stride = ZHW + PAD


def latent_inputs(case):
    B, ZHW = case
    gen = torch.Generator().manual_seed(500 + list(LATENT_CASES).index(case))
    r = lambda *s: torch.randn(*s, generator=gen)
    enc, pri = 1.5 * r(B, 2 * ZHW), 1.5 * r(B, 2 * ZHW)
    planted = torch.zeros(B, ZHW, dtype=torch.bool)
    pos = torch.randperm(B * ZHW, generator=gen)[:2 * len(PLANTED)]
    for k, v in enumerate(PLANTED):                  # each value once in the encoder's and once in the prior's scales
        for t, p in ((enc, int(pos[2 * k])), (pri, int(pos[2 * k + 1]))):
            t[p // ZHW, ZHW + p % ZHW] = v
            planted[p // ZHW, p % ZHW] = True
    return Bag(B=B, ZHW=ZHW, enc=enc, pri=pri, ep=r(B, ZHW), eq=r(B, ZHW), gouts=[r(B, ZHW) for _ in range(5)],
               planted=planted)


@pytest.mark.parametrize("res_q", (0, 1), ids=("plain", "res_q"))
@pytest.mark.parametrize("case", list(LATENT_CASES), ids=ids)
def test_latent_step_vs_fp64(L, case, res_q):
    I = latent_inputs(case)
    B, ZHW = case
    enc, pri, ep, eq = I.enc.cuda(), I.pri.cuda(), I.ep.cuda(), I.eq.cuda()
    le, lp = I.enc.double().requires_grad_(), I.pri.double().requires_grad_()
    ref = latent_ref(le, lp, I.ep.double(), I.eq.double(), res_q)
    names = ("zt", "zxt", "kl", "em", "es")
    outs = [nan_buf((B, ZHW)) for _ in names]
    L.call("rfn_latent_step_fwd_f32", L.dev(enc), L.dev(pri), L.dev(ep), L.dev(eq), *[L.dev(o) for o in outs], _i(B),
           _i(ZHW), _i(res_q))
    torch.cuda.synchronize()
    rest = ~I.planted
    e = Bag()
    for nm, o in zip(names, outs):
        if nm == "kl":
            e["kl/A"] = float(((o.cpu().double() - ref.kl.detach()).abs() / ref.A.detach()).max())
        else:
            e[nm], e[nm + "/rest"] = relerr(o, ref[nm]), relerr(o, ref[nm], rest)
    rest2 = torch.cat([rest, rest], 1)
    for sub, sel in LATENT_SUBSETS.items():
        loss = sum((ref[names[k]] * I.gouts[k].double()).sum() for k in sel)
        g_enc64, g_pri64 = torch.autograd.grad(loss, (le, lp), retain_graph=True, allow_unused=True)
        if g_enc64 is None:                          # zt does not depend on the encoder
            g_enc64 = torch.zeros_like(le)
        strided, parents = [], []
        for k in (0, 1):     # channel slices [:, 5 : 5 + ZHW] of a wider [B, ZHW + PAD] gradient: the row-stride read
            if k in sel:
                parent = torch.full((B, ZHW + PAD), SENT, device="cuda", dtype=torch.float32)
                parent[:, 5:5 + ZHW] = I.gouts[k].cuda()
                v = parent[:, 5:5 + ZHW]
                assert v.stride(0) == ZHW + PAD and v[0].is_contiguous()
                parents.append(parent)
                strided += [ctypes.c_void_p(v.data_ptr()), _l(v.stride(0))]
            else:
                strided += [None, _l(0)]
        dense = [I.gouts[k].cuda() if k in sel else None for k in (2, 3, 4)]
        g_enc, g_pri = nan_buf((B, 2 * ZHW)), nan_buf((B, 2 * ZHW))
        L.call("rfn_latent_step_bwd_f32", L.dev(enc), L.dev(pri), L.dev(ep), L.dev(eq), *strided,
               *[L.dev(t) for t in dense], L.dev(g_enc), L.dev(g_pri), _i(B), _i(ZHW), _i(res_q))
        torch.cuda.synchronize()
        for nm, got, want in (("g_enc", g_enc, g_enc64), ("g_pri", g_pri, g_pri64)):
            if float(want.abs().max()) == 0.0:       # (zt only: the encoder gets no gradient)
                assert float(got.abs().max()) == 0.0, (sub, nm)
                continue
            e["%s:%s" % (nm, sub)], e["%s:%s/rest" % (nm, sub)] = relerr(got, want), relerr(got, want, rest2)
    print("\nLATENT %s res_q=%d %s | %s" % (ids(case), res_q, latent_label(L, *case),
                                          " ".join("%s %.1e" % kv for kv in e.items())))
    assert e["kl/A"] <= SUM_BOUND, e["kl/A"]
    for k, v in e.items():
        assert v < EW_BOUND, (k, v)


# ------------------------------------------------------------------------------------------------ Gaussian
def gauss_inputs(case, std_mode, regime):
    N, Cz, HW = case
    gen = torch.Generator().manual_seed(600 + list(GAUSS_CASES).index(case) * 4 + std_mode * 2 + (regime == "edge"))
    r = lambda *s: torch.randn(*s, generator=gen)
    o = r(N, 2 * Cz, HW)
    raw = r(N, Cz, HW)
    if regime == "edge":
        lo, hi = (-12.0, 25.0) if std_mode == 0 else (-4.0, 4.0)
        raw = lo + (hi - lo) * torch.rand(N, Cz, HW, generator=gen)
    return Bag(z=r(N, Cz, HW), o=o, raw=raw, eps=r(N, Cz, HW), glogp=r(N), init=0.5 + r(N).abs())


@pytest.mark.parametrize("regime", ("typical", "edge"))
@pytest.mark.parametrize("std_mode", (0, 1), ids=("softplus", "exp"))
@pytest.mark.parametrize("layout", (0, 1), ids=("cross", "split"))
@pytest.mark.parametrize("case", list(GAUSS_CASES), ids=ids)
def test_gauss_vs_fp64(L, case, layout, std_mode, regime):
    N, Cz, HW = case
    I = gauss_inputs(case, std_mode, regime)
    o = I.o.clone()
    if layout == 0:
        o[:, 1::2] = I.raw
    else:
        o[:, Cz:] = I.raw
    zl, ol = I.z.double().requires_grad_(), o.double().requires_grad_()
    logp64, A = gauss_ref(zl, ol, layout, std_mode)
    gz64, go64 = torch.autograd.grad((logp64 * I.glogp.double()).sum(), (zl, ol))
    (zpar, z), (opar, od) = view_of(I.z), view_of(o)
    zp, zns = L.frames(z, "z")
    op, ons = L.frames(od, "o")
    runs = []
    for _ in range(2):
        logp = I.init.cuda()
        L.call("rfn_gauss_logp_f32", zp, _l(zns), op, _l(ons), L.dev(logp), _i(layout), _i(std_mode), _i(N), _i(Cz), _i(HW))
        (gzpar, gz), (gopar, go) = view_of((N, Cz, HW)), view_of((N, 2 * Cz, HW))
        gzp, gzns = L.frames(gz, "gz")
        gop, gons = L.frames(go, "go")
        L.call("rfn_gauss_logp_bwd_f32", zp, _l(zns), op, _l(ons), L.dev(I.glogp.cuda()), gzp, _l(gzns), gop, _l(gons),
               _i(layout), _i(std_mode), _i(N), _i(Cz), _i(HW))
        (spar, smp) = view_of((N, Cz, HW))
        sp, sns = L.frames(smp, "z")
        L.call("rfn_gauss_sample_f32", op, _l(ons), L.dev(I.eps.cuda()), sp, _l(sns), _f(0.7), _i(layout), _i(std_mode),
               _i(N), _i(Cz), _i(HW))
        torch.cuda.synchronize()
        assert all(untouched(p) for p in (zpar, opar, gzpar, gopar, spar)), "wrote outside a channel slice"
        runs.append((logp.cpu(), gz.cpu(), go.cpu(), smp.cpu()))
    logp, gz, go, smp = runs[0]
    e = Bag(logp=float(((logp.double() - (I.init.double() + logp64.detach())).abs() / (A.detach() + I.init.double())).max()),
            gz=relerr(gz, gz64), go=relerr(go, go64),
            sample=relerr(smp, gauss_sample_ref(o.double(), I.eps.double(), 0.7, layout, std_mode)))
    print("\nGAUSS %s %s %s %s | %s" % (ids(case), ("cross", "split")[layout], ("softplus", "exp")[std_mode], regime,
                                      " ".join("%s %.1e" % kv for kv in e.items())))
    assert e.logp <= SUM_BOUND, e
    assert e.gz < EW_BOUND and e.go < EW_BOUND and e.sample < EW_BOUND, e
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ"


@pytest.mark.parametrize("view", (False, True), ids=("dense", "slice"))
@pytest.mark.parametrize("case", list(STATS_CASES), ids=ids)
def test_channel_stats_vs_fp64(L, case, view):
    N, C, HW = case
    gen = torch.Generator().manual_seed(700 + list(STATS_CASES).index(case))
    x = 1.5 * torch.randn(N, C, HW, generator=gen) + torch.randn(1, C, 1, generator=gen)
    if view:
        par, xd = view_of(x)
    else:
        par, xd = None, x.cuda()
    xp, xns = L.frames(xd, "x")
    mean, var = nan_buf((C,)), nan_buf((C,))
    L.call("rfn_channel_stats_f32", xp, _l(xns), L.dev(mean), L.dev(var), _i(N), _i(C), _i(HW))
    torch.cuda.synchronize()
    m64, v64 = channel_stats_ref(x.double())
    e = Bag(mean=relerr(mean, m64), var=relerr(var, v64))
    print("\nSTATS %s %s | mean %.1e var %.1e" % (ids(case), "slice" if view else "dense", e.mean, e.var))
    assert par is None or untouched(par)
    assert e.mean < STAT_BOUND and e.var < STAT_BOUND, e
