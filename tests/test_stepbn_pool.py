"""rfn_stepbn_pool_{fwd,bwd}_f32 (per-step BatchNorm + activation + 2x2 max-pool in two launches each way) on the GPU:
the rows of tests/test_stepbn_pool_host.py, on the routes that module holds the library to.

Forward: p, mean, var, the running statistics and num_batches_tracked are bit-equal to the composed path
(StepBatchNormActFn, then F.max_pool2d on the GPU), also on the rows built to tie (dyadic inputs; tanhf saturated at +-1;
relu's zeros): the winner rule is max_pool2d's.

Backward: against the same composed path gx is equal up to the differently ordered sums k1, k2 (the winners are the same by
construction), and on the rows whose seed gives every window a winner margin (host module) both paths are compared
against the fp64 reference bn_pool_ref: the fused path's error (max-abs over max|ref|) may be at most twice the composed
path's error measured in the same test, with a floor of 2^-22 -- the two add the same terms in a different order.  Both
figures of every row go to the file RFN_STEPBN_POOL_ERRORS names, when set (profiles/stepbn_pool_errors.txt)."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_glow_shell import NAN
from tests.test_recurrent_shell import EW_BOUND, RED_BOUND, aligned_bits, nan_buf, put, relerr, scratch, tail_ok
from tests.test_recurrent_shell_host import ACTS, BN_EPS, BN_MOMENTUM, Bag, from_global, to_global
from tests.test_stepbn_pool_host import (POOL_SYNC, bn_pool_ref, case_id, pool_aligned, pool_cases, pool_id, pool_inputs,
                                         pool_label)

pytestmark = pytest.mark.gpu

_i, _f = ctypes.c_int, ctypes.c_float
FLOOR = 2.0 ** -22
KEYS = ("gx", "ggamma", "gbeta")


@pytest.fixture(scope="module")
def L():
    from rfn_hip import lib
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return lib


@pytest.fixture(scope="module")
def errors_file():
    lines = []
    yield lines
    path = os.environ.get("RFN_STEPBN_POOL_ERRORS")
    if path and lines:
        with open(path, "w") as f:
            f.write("# case | fused and composed error against fp64 (max-abs over max|ref|) of gx, ggamma, gbeta\n")
            f.write("\n".join(lines) + "\n")


def _running(I, dev):
    from Utils.modules import _ema_coef
    cf, cfu = _ema_coef(I.S, BN_MOMENTUM, I.B * I.HW, dev)
    return (I.rm.cuda(), I.rv.cuda(), cf, cfu, (1.0 - BN_MOMENTUM) ** I.S,
            torch.full((1,), I.nbt, device="cuda", dtype=torch.int64))


def fused(L, I, x, gp, affine, act, slope, mis):
    """forward + backward of the fused entry points into fresh NaN-filled outputs"""
    S, B, C, H, W = I.S, I.B, I.C, I.H, I.W
    op = 1 if mis == "p" else 0
    p, gx = nan_buf((S * B, C, H // 2, W // 2), op), nan_buf(tuple(x.shape), op)
    mean, var = nan_buf((S, C)), nan_buf((S, C))
    gamma, beta = (I.gamma.cuda(), I.beta.cuda()) if affine else (None, None)
    acc, n = scratch(L, S, B, C)
    rm, rv, cf, cfu, decay, nbt = _running(I, x.device)
    masks = (aligned_bits([x], [x, p]), aligned_bits([x, gp], [x, gp, gx]))
    L.call("rfn_stepbn_pool_fwd_f32", L.dev(x), L.dev(gamma), L.dev(beta), L.dev(p), L.dev(mean), L.dev(var), L.dev(acc),
           L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cfu), _f(decay), ctypes.c_void_p(nbt.data_ptr()), _i(S), _i(B), _i(C),
           _i(H), _i(W), _f(BN_EPS), _i(act), _f(slope))
    sums, _ = scratch(L, S, B, C)
    ggamma, gbeta = (nan_buf((C,)), nan_buf((C,))) if affine else (None, None)
    L.call("rfn_stepbn_pool_bwd_f32", L.dev(x), L.dev(gamma), L.dev(beta), L.dev(gp), L.dev(mean), L.dev(var),
           L.dev(sums), L.dev(gx), L.dev(ggamma), L.dev(gbeta), _i(S), _i(B), _i(C), _i(H), _i(W), _f(BN_EPS), _i(act),
           _f(slope), _i(0), _i(1))
    torch.cuda.synchronize()
    return Bag(p=p, gx=gx, mean=mean, var=var, ggamma=ggamma, gbeta=gbeta, rm=rm, rv=rv, nbt=nbt, masks=masks,
               scratch_ok=tail_ok(acc, n) and tail_ok(sums, n))


def composed(I, x, gp, affine, act, slope):
    """StepBatchNormActFn, then F.max_pool2d, gradients by autograd: the route the fused kernels replace"""
    from rfn_hip import ops as K
    xl = x.detach().requires_grad_(True)        # the same (perhaps misaligned) memory: the same statistics route
    gamma, beta = ((I.gamma.cuda().requires_grad_(True), I.beta.cuda().requires_grad_(True)) if affine else (None, None))
    running = _running(I, x.device)
    y, mean, var = K.StepBatchNormActFn.apply(xl, gamma, beta, I.S, BN_EPS, act, slope, running)
    p = F.max_pool2d(y, kernel_size=2, stride=2)
    gr = torch.autograd.grad(p, [xl] + ([gamma, beta] if affine else []), gp.contiguous())
    torch.cuda.synchronize()
    return Bag(p=p.detach(), gx=gr[0], mean=mean, var=var, ggamma=gr[1] if affine else None,
               gbeta=gr[2] if affine else None, rm=running[0], rv=running[1], nbt=running[5])


@pytest.fixture(scope="module")
def case_inputs():
    cache = {}

    def get(row, seed):
        k = (pool_id(row), seed)
        if k not in cache:
            cache.clear()
            I = pool_inputs(row, seed)
            cache[k] = (I, put(I.x, 1 if row["mis"] == "x" else 0), put(I.gp))
        return cache[k]
    return get


def _close_to_composed(got, comp, affine):
    """gx / ggamma / gbeta of the two GPU paths: the same terms, sums in another order"""
    for k in KEYS[:3 if affine else 1]:
        e = relerr(got[k], comp[k].double())
        assert e < (EW_BOUND if k == "gx" else RED_BOUND), (k, e)      # the unpooled kernels' bounds against fp64


@pytest.mark.parametrize("affine", (True, False), ids=("affine", "plain"))
@pytest.mark.parametrize("case", pool_cases(), ids=case_id)
def test_pool_vs_composed_and_fp64(L, case_inputs, errors_file, case, affine):
    row, a, seed = case
    act, slope = ACTS[a]
    has_ref = row["acts"][a] is not None
    I, x, gp = case_inputs(row, seed)
    got = fused(L, I, x, gp, affine, act, slope, row["mis"])
    comp = composed(I, x, gp, affine, act, slope)
    assert got.masks == (pool_aligned(row, 0), pool_aligned(row, 1)), got.masks       # the routes the labels were asked about
    assert got.scratch_ok, "a partial sum was left unwritten, or the scratch was overrun"
    # forward: not a bit moves
    for k in ("p", "mean", "var", "rm", "rv", "nbt"):
        assert torch.equal(got[k], comp[k]), (k, float((got[k].double() - comp[k].double()).abs().max()))
    assert int(got.nbt) == I.nbt + I.S
    # backward
    assert not bool(torch.isnan(got.gx).any()), "gx has unwritten elements"
    _close_to_composed(got, comp, affine)
    if not has_ref:
        return
    ga, be = (I.gamma, I.beta) if affine else (None, None)
    ref = bn_pool_ref(I.x, ga, be, I.gp, I.S, act, slope)
    assert relerr(got.p, ref.p) < 1e-5
    line = [case_id(case), "affine" if affine else "plain", pool_label(L, row, 1)]
    bad = []
    for k in KEYS[:3 if affine else 1]:
        r = getattr(ref, k)               # (bn_ref sets its gradients as attributes of the Bag)
        ef, ec = relerr(got[k], r), relerr(comp[k], r)
        line.append("%s fused %.3e composed %.3e" % (k, ef, ec))
        if not ef <= max(2.0 * ec, FLOOR):
            bad.append((k, ef, ec))
    print("\nPOOL " + " | ".join(line))
    errors_file.append(" | ".join(line))
    assert not bad, bad


def test_pool_is_deterministic_and_running_statistics_are_optional(L, case_inputs):
    row, a, seed = pool_cases()[3]                       # tanh on the vector route
    act, slope = ACTS[a]
    I, x, gp = case_inputs(row, seed)
    one, two = (fused(L, I, x, gp, True, act, slope, None) for _ in range(2))
    for k in ("p", "gx", "mean", "var", "ggamma", "gbeta", "rm", "rv"):
        assert torch.equal(one[k], two[k]), k
    S, B, C, H, W = row["shape"]
    p, mean, var = nan_buf((S * B, C, H // 2, W // 2)), nan_buf((S, C)), nan_buf((S, C))
    acc, n = scratch(L, S, B, C)
    gamma, beta = I.gamma.cuda(), I.beta.cuda()
    L.call("rfn_stepbn_pool_fwd_f32", L.dev(x), L.dev(gamma), L.dev(beta), L.dev(p), L.dev(mean), L.dev(var), L.dev(acc),
           None, None, None, None, _f(1.0), None, _i(S), _i(B), _i(C), _i(H), _i(W), _f(BN_EPS), _i(act), _f(slope))
    torch.cuda.synchronize()
    assert torch.equal(p, one.p) and torch.equal(mean, one.mean) and torch.equal(var, one.var) and tail_ok(acc, n)


def test_a_nan_input_behaves_as_in_the_composed_path(L):
    """a NaN in x poisons the statistics of its (step, channel) in both paths alike: that pair's pooled map is NaN, every
    other pair is untouched and bit-equal"""
    I = pool_inputs(dict(shape=(2, 3, 4, 4, 4)), 0)
    I.x[1, 2, 0, 1] = NAN
    x, gp = put(I.x), put(I.gp)
    got = fused(L, I, x, gp, True, 0, 0.0, None)
    comp = composed(I, x, gp, True, 0, 0.0)
    nan = torch.isnan(got.p)
    assert torch.equal(nan, torch.isnan(comp.p)) and bool(nan[:3, 2].all()) and int(nan.sum()) == 3 * 4
    assert torch.equal(torch.nan_to_num(got.p), torch.nan_to_num(comp.p))


@pytest.mark.parametrize("affine", (True, False), ids=("affine", "plain"))
def test_pool_backward_stages_over_two_ranks_vs_fp64_on_the_global_batch(L, affine):
    """stage 1 per rank, the sums added over the ranks, stage 2 with world = 2, on the GLOBAL statistics (combined from the
    ranks' moments as StepBatchNormActFn._forward_sync does) = bn_pool_ref on the global batch"""
    row = POOL_SYNC
    S, B, C, H, W = row["shape"]
    world = row["world"]
    act, slope = ACTS[row["act"]]
    ranks = [pool_inputs(row, row["seed"] + 100 * r) for r in range(world)]
    gamma, beta = ranks[0].gamma, ranks[0].beta
    ga, be = (gamma.cuda(), beta.cuda()) if affine else (None, None)
    xs, gps = [put(I.x) for I in ranks], [put(I.gp) for I in ranks]
    stats = []
    for x in xs:
        y, mean, var = nan_buf(tuple(x.shape)), nan_buf((S, C)), nan_buf((S, C))
        acc, n = scratch(L, S, B, C)
        L.call("rfn_stepbn_fwd_f32", L.dev(x), L.dev(ga), L.dev(be), L.dev(y), L.dev(mean), L.dev(var), L.dev(acc), None,
               None, None, None, _f(1.0), None, _i(S), _i(B), _i(C), _i(H * W), _f(BN_EPS), _i(act), _f(slope))
        stats.append(torch.stack((mean, var)))
    st = torch.stack(stats)
    mean = st[:, 0].mean(0).contiguous()
    var = (st[:, 1].mean(0) + (st[:, 0] - mean).pow(2).mean(0)).contiguous()
    sums = [scratch(L, S, B, C) for _ in xs]
    n = sums[0][1]
    out = [Bag(gx=nan_buf(tuple(x.shape)), ggamma=nan_buf((C,)) if affine else None,
               gbeta=nan_buf((C,)) if affine else None) for x in xs]
    args = lambda k: (L.dev(xs[k]), L.dev(ga), L.dev(be), L.dev(gps[k]), L.dev(mean), L.dev(var), L.dev(sums[k][0]),
                      L.dev(out[k].gx), L.dev(out[k].ggamma), L.dev(out[k].gbeta), _i(S), _i(B), _i(C), _i(H), _i(W),
                      _f(BN_EPS), _i(act), _f(slope))
    for k in range(world):
        L.call("rfn_stepbn_pool_bwd_f32", *args(k), _i(1), _i(world))
    torch.cuda.synchronize()
    assert all(tail_ok(sm, n) for sm, _ in sums) and all(bool(torch.isnan(o.gx).all()) for o in out)  # stage 1: no gx
    total = torch.stack([sm[:n] for sm, _ in sums]).sum(0)                         # the all-reduce
    for sm, _ in sums:
        sm[:n] = total
    for k in range(world):
        L.call("rfn_stepbn_pool_bwd_f32", *args(k), _i(2), _i(world))
    torch.cuda.synchronize()
    ref = bn_pool_ref(to_global([I.x for I in ranks], S), gamma if affine else None, beta if affine else None,
                      to_global([I.gp for I in ranks], S), S, act, slope)
    gx = from_global(ref.gx, S, world)
    e = Bag(gx=max(relerr(out[k].gx, gx[k]) for k in range(world)))
    if affine:
        e.update(ggamma=max(relerr(o.ggamma, ref.ggamma / world) for o in out),
                 gbeta=max(relerr(o.gbeta, ref.gbeta / world) for o in out))
    print("\nPOOL SYNC world=%d %s | %s" % (world, "affine" if affine else "plain", " ".join("%s %.1e" % kv for kv in e.items())))
    assert e.gx < 1e-5, e                           # the bounds of the unpooled kernels' rows (tests/test_recurrent_shell.py)
    if affine:
        assert e.ggamma < 1e-4 and e.gbeta < 1e-4, e


# ------------------------------------------------------------------------------------------------ autograd, module
def test_function_and_module_route_equal_the_unfused_route(L, monkeypatch):
    """Utils.modules.run_time_batched on BatchNorm -> act -> MaxPool2d(2, 2): the fused pattern against
    RFN_STEPBN_POOL=0 -- outputs and buffers bit-equal, gradients equal to the order of the backward sums; an odd map
    falls back by itself"""
    from Utils import modules as M
    torch.manual_seed(5)
    S, B = 3, 4
    for act, hw in ((M.ActFun("relu"), (8, 12)), (nn.Tanh(), (6, 10)), (M.ActFun("leakyrelu"), (7, 8))):
        seq = nn.Sequential(M.NormLayer(3, "batchnorm"), act, nn.MaxPool2d(kernel_size=2, stride=2)).cuda().train()
        with torch.no_grad():
            seq[0].norm.weight.uniform_(0.5, 1.5)
            seq[0].norm.bias.uniform_(-0.5, 0.5)
        x = torch.randn(S * B, 3, *hw, device="cuda")
        state = {k: v.clone() for k, v in seq.state_dict().items()}
        res = {}
        calls = {"n": 0}
        real = M.K.StepBatchNormActPoolFn.apply

        def counted(*a, **k):
            calls["n"] += 1
            return real(*a, **k)
        monkeypatch.setattr(M.K.StepBatchNormActPoolFn, "apply", counted)
        for mode in ("fused", "0"):
            seq.load_state_dict(state)
            seq.zero_grad(set_to_none=True)
            if mode == "0":
                monkeypatch.setenv("RFN_STEPBN_POOL", "0")
            else:
                monkeypatch.delenv("RFN_STEPBN_POOL", raising=False)
            xl = x.clone().requires_grad_(True)
            before = calls["n"]
            out = M.run_time_batched(seq, xl, S)
            (out * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum().backward()
            torch.cuda.synchronize()
            assert calls["n"] - before == (1 if mode == "fused" and hw[0] % 2 == 0 else 0)
            res[mode] = (out.detach(), {k: v.clone() for k, v in seq.state_dict().items()}, xl.grad,
                         [p.grad.clone() for p in seq.parameters()])
        monkeypatch.undo()
        assert torch.equal(res["fused"][0], res["0"][0])
        assert all(torch.equal(res["fused"][1][k], res["0"][1][k]) for k in state)
        assert relerr(res["fused"][2], res["0"][2].double()) < 1e-5
        for gf, g0 in zip(res["fused"][3], res["0"][3]):
            assert relerr(gf, g0.double()) < 1e-4
