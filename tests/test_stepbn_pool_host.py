"""Case table, launch routes and fp64 reference of the per-step BatchNorm + activation + 2x2 max-pool kernels
(rfn_stepbn_pool_{fwd,bwd}_f32), without a device.  tests/test_stepbn_pool.py runs the same rows on the GPU.

rfn_stepbn_pool_kernel_label prints the host struct the launchers read (choose_stepbn with its pool flag in csrc/stepbn.hip).  `aligned`
bit 0: x (statistics kernel) or, backward, x and gp (reduce kernel) are 16-byte aligned; bit 1: the apply kernel's
pointers (x, p; backward x, gp, gx).  The pooled kernels also need W % 4 == 0 for their 16-byte route; the statistics
kernel is the unpooled one and tests H*W % 4, which even sides always satisfy.

Winner margin: the kernels pick a window's winner among fp32 activated values, the reference among fp64 ones; the two can
differ where the two largest values of a window nearly tie.  Every row that is compared against fp64 carries the first
seed in 0..63 for which ALL windows have a gap of at least U_MARGIN between their two largest activated values, or have
both in the flat part of the activation (relu at 0: the gradient is zero whichever wins), and, for relu / leaky, for which
min|u| >= U_MARGIN as in tests/test_recurrent_shell_host.py.  Rows without such a seed (large, or built to tie) are
compared against the composed GPU path only (ref=False)."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_glow_shell_host import fields
from tests.test_recurrent_shell_host import ACTS, BN_EPS, U_MARGIN, bn_inputs, bn_ref, to_global

POOL_GRID_CAP = 8192
# (S, B, C, H, W); mis: None | "x" (x one float off 16 bytes) | "p" (p / gx one float off); acts -> seed (None: not compared
# against fp64); kind: bn_inputs' kinds and "saturate" (gamma x 30: tanhf reaches exactly 1 on most of the map)
POOL_ROWS = [
    dict(shape=(3, 4, 6, 8, 8), mis=None, ny=4, stats=("vec", "vec"), apply="vec4", sweeps=1,
         acts=dict(none=0, relu=0, leaky=0, tanh=0)),                                      # vector route
    dict(shape=(2, 3, 5, 6, 10), mis=None, ny=3, stats=("vec", "scalar"), apply="vec1", sweeps=1,
         acts=dict(none=1, relu=4, leaky=4, tanh=1)),                                      # pooled 3x5: W % 4 = 2
    dict(shape=(2, 3, 5, 2, 2), mis=None, ny=3, stats=("vec", "scalar"), apply="vec1", sweeps=1,
         acts=dict(none=0, relu=0, leaky=0, tanh=0)),                                      # pooled 1x1
    dict(shape=(5, 2, 16, 4, 4), mis=None, ny=2, stats=("vec", "vec"), apply="vec4", sweeps=1,
         acts=dict(none=0, relu=0, leaky=0, tanh=0)),                                      # the extractor's last pool
    dict(shape=(2, 37, 8, 4, 4), mis=None, ny=16, stats=("vec", "vec"), apply="vec4", sweeps=1,
         acts=dict(none=0, relu=4, leaky=4, tanh=0)),                                      # ny < B
    dict(shape=(9, 7, 64, 4, 4), mis=None, ny=3, stats=("vec", "vec"), apply="vec4", sweeps=1,
         acts=dict(none=1, tanh=None)),                                                    # S*C = 576; 16128 windows
    dict(shape=(3, 4, 6, 8, 8), mis="x", ny=4, stats=("scalar", "scalar"), apply="vec1", sweeps=1,
         acts=dict(tanh=0)),
    dict(shape=(3, 4, 6, 8, 8), mis="p", ny=4, stats=("vec", "vec"), apply="vec1", sweeps=1,
         acts=dict(leaky=0)),
    dict(shape=(2, 8, 66, 128, 128), mis=None, ny=8, stats=("vec", "vec"), apply="vec4", sweeps=2,
         acts=dict(relu=None), big=True),                                                  # 8448 > 8192 blocks
    dict(shape=(3, 4, 6, 8, 8), mis=None, ny=4, stats=("vec", "vec"), apply="vec4", sweeps=1,
         acts=dict(none=None), kind="dyadic", seed=12),                                    # exact ties
    dict(shape=(3, 4, 6, 8, 8), mis=None, ny=4, stats=("vec", "vec"), apply="vec4", sweeps=1,
         acts=dict(tanh=None), kind="saturate", seed=13),                                  # ties at exactly +-1
    dict(shape=(2, 3, 5, 6, 10), mis=None, ny=3, stats=("vec", "scalar"), apply="vec1", sweeps=1,
         acts=dict(relu=None), kind="dyadic", seed=14),                                    # ties at 0, scalar route
]
# stage 1 + 2 over two emulated ranks: (S, B per rank, C, H, W) -> activation, seed of rank 0 (rank r: seed + 100 r)
POOL_SYNC = dict(shape=(3, 2, 6, 4, 4), world=2, act="tanh", seed=0)


def pool_id(row):
    return "x".join(map(str, row["shape"])) + ("-" + row["kind"] if row.get("kind") else "") + \
        ("-mis" + row["mis"] if row["mis"] else "")


def pool_aligned(row, bwd):
    """the `aligned` argument for the pointers the GPU test passes: "p" moves p (forward) and gx (backward) only"""
    return {None: 3, "x": 0, "p": 1}[row["mis"]]


def pool_cases(rows=POOL_ROWS, ref=None):
    """[(row, activation name, seed)]; ref=True / False: only the cases compared / not compared against fp64"""
    out = []
    for r in rows:
        for a, seed in r["acts"].items():
            if ref is None or ref == (seed is not None):
                out.append((r, a, r.get("seed", 0) if seed is None else seed))
    return out


case_id = lambda c: "%s-%s" % (pool_id(c[0]), c[1])


# ------------------------------------------------------------------------------------------------ inputs, reference
def pool_inputs(row, seed):
    """bn_inputs of the row with this seed + a pooled incoming gradient gp; kind "saturate": gamma x 30"""
    kind = row.get("kind")
    I = bn_inputs(dict(shape=row["shape"], seed=seed, kind=None if kind == "saturate" else kind))
    gen = torch.Generator().manual_seed(seed + 4096)
    n = (I.S * I.B, I.C, I.H // 2, I.W // 2)
    I["gp"] = torch.randint(-8, 9, n, generator=gen).float() / 8 if kind == "dyadic" else torch.randn(n, generator=gen)
    if kind == "saturate":
        I["gamma"] = I.gamma * 30
    return I


def bn_pool_ref(x, gamma, beta, gp, S, act, slope, eps=BN_EPS):
    """bn_ref followed by F.max_pool2d(2, 2) in fp64; gradients of sum(p gp) by autograd: the pool's through a leaf copy of
    y, handed to bn_ref as its incoming gradient.  -> bn_ref's Bag + p, gy (the full-resolution gradient)"""
    fwd = bn_ref(x, gamma, beta, None, S, act, slope, eps)
    y = fwd.y.clone().requires_grad_(gp is not None)
    p = F.max_pool2d(y, 2, 2)
    if gp is None:
        fwd.update(p=p.detach(), gy=None)
        return fwd
    (gy,) = torch.autograd.grad((p * gp.double()).sum(), y)
    out = bn_ref(x, gamma, beta, gy, S, act, slope, eps)
    out.update(p=p.detach(), gy=gy)
    return out


def winner_margin(ref, act):
    """over all windows of a reference: (the smallest gap between the two largest activated values among the windows that
    are not flat, the number of flat windows).  Flat: relu with both of them 0 (every u of the window <= 0)."""
    y = ref.y
    N, C, H, W = y.shape
    win = y.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
    top = win.sort(1, descending=True).values
    gap = top[:, 0] - top[:, 1]
    flat = (top[:, 0] == 0) & (top[:, 1] == 0) if act == 1 else torch.zeros_like(gap, dtype=torch.bool)
    live = gap[~flat]
    return (float(live.min()) if live.numel() else math.inf), int(flat.sum())


def margins_hold(row, a, seed):
    """the docstring's two conditions, with and without affine parameters"""
    act, slope = ACTS[a]
    I = pool_inputs(row, seed)
    for ga, be in ((I.gamma, I.beta), (None, None)):
        ref = bn_ref(I.x, ga, be, None, I.S, act, slope)
        gap, _ = winner_margin(ref, act)
        if gap < U_MARGIN or (act in (1, 2) and float(ref.u.abs().min()) < U_MARGIN):
            return False
    return True


# ------------------------------------------------------------------------------------------------ routes
@pytest.fixture(scope="module")
def lib():
    from rfn_hip import lib as L_
    L_.load()
    return L_


def pool_label(lib, row, bwd=0):
    S, B, C, H, W = row["shape"]
    return lib.load().rfn_stepbn_pool_kernel_label(S, B, C, H, W, pool_aligned(row, bwd), bwd).decode()


@pytest.mark.parametrize("row", POOL_ROWS, ids=pool_id)
def test_pool_route_is_the_table_row(lib, row):
    S, B, C, H, W = row["shape"]
    for bwd in (0, 1):
        name, f = fields(pool_label(lib, row, bwd))
        assert name == "stepbn_pool"
        assert (f["ny"], f["stats"], f["apply"], f["sweeps"]) == (row["ny"], row["stats"][bwd], row["apply"], row["sweeps"]), f
        assert f["ny"] * 2 * S * C == lib.load().rfn_stepbn_scratch_floats(S, B, C)      # the unpooled kernels' scratch
        assert f["ny"] == max(1, min(2048 // (S * C), 16, B))
        units = S * B * C * H * W // (8 if f["apply"] == "vec4" else 4)
        blocks = -(-units // 256)
        assert f["grid"] == min(blocks, POOL_GRID_CAP) and f["sweeps"] == -(-blocks // f["grid"])
        assert (f["apply"] == "vec4") == (W % 4 == 0 and row["mis"] is None)
        assert (f["stats"] == "vec") == (row["mis"] != "x" and (W % 4 == 0 or not bwd))
    assert S * B * C * H * W < 2 ** 31 and H % 2 == 0 and W % 2 == 0


def test_pool_table_reaches_every_route(lib):
    rows = [(r, fields(pool_label(lib, r, 0))[1], fields(pool_label(lib, r, 1))[1]) for r in POOL_ROWS]
    assert {(b["stats"], b["apply"]) for _, _, b in rows} == {("vec", "vec4"), ("scalar", "vec1"), ("vec", "vec1")}
    assert {(f["stats"], f["apply"]) for _, f, _ in rows} == {("vec", "vec4"), ("scalar", "vec1"), ("vec", "vec1")}
    assert {f["sweeps"] for _, f, _ in rows} == {1, 2}
    assert any(f["ny"] < r["shape"][1] for r, f, _ in rows) and any(f["ny"] == r["shape"][1] for r, f, _ in rows)
    assert any(r["shape"][3:] == (2, 2) for r, _, _ in rows)                             # pooled 1x1
    assert any(r["shape"][0] * r["shape"][2] == 576 for r, _, _ in rows)                 # the training class
    assert {a for r, _, _ in rows for a in r["acts"]} == set(ACTS)
    assert {r["mis"] for r, _, _ in rows} == {None, "x", "p"}
    for a in ACTS:                                                                        # each against fp64 on both routes
        assert {r["apply"] for r, n, _ in pool_cases(ref=True) if n == a and r["mis"] is None} == {"vec4", "vec1"}


def test_pool_label_and_launchers_refuse_odd_sides(lib):
    L = lib.load()
    for H, W in ((3, 4), (4, 3), (1, 1)):
        assert L.rfn_stepbn_pool_kernel_label(2, 2, 2, H, W, 3, 0) == b"unsupported"
    assert L.rfn_stepbn_pool_kernel_label(0, 4, 4, 4, 4, 3, 0) == b"unsupported"
    assert L.rfn_stepbn_pool_kernel_label(2, 4, 4, 1 << 14, 1 << 13, 3, 1) == b"unsupported"          # 2^31 elements
    assert L.rfn_stepbn_pool_kernel_label(2, 2, 2, 4, 4, 3, 0).startswith(b"stepbn_pool ")
    # the argument checks return before anything is launched or dereferenced: placeholder addresses, no device
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for H, W in ((3, 4), (4, 3)):
        rc = L.rfn_stepbn_pool_fwd_f32(p, None, None, p, p, p, p, None, None, None, None, 1.0, None, 1, 1, 1, H, W, 1e-5, 0,
                                       0.0, None)
        assert rc == -5 and b"H % 2 == 0" in L.rfn_last_error()
        rc = L.rfn_stepbn_pool_bwd_f32(p, None, None, p, p, p, p, p, None, None, 1, 1, 1, H, W, 1e-5, 0, 0.0, 0, 1, None)
        assert rc == -5 and b"H % 2 == 0" in L.rfn_last_error()


# ------------------------------------------------------------------------------------------------ reference, margins
@pytest.mark.parametrize("a", list(ACTS))
def test_bn_pool_ref_equals_the_torch_modules(a):
    """nn.BatchNorm2d applied step by step + the activation + nn.MaxPool2d(2, 2) in fp64, gradients by autograd"""
    row = POOL_ROWS[1]
    act, slope = ACTS[a]
    I = pool_inputs(row, row["acts"][a])
    ref = bn_pool_ref(I.x, I.gamma, I.beta, I.gp, I.S, act, slope)
    bn = nn.BatchNorm2d(I.C, eps=BN_EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(I.gamma)
        bn.bias.copy_(I.beta)
    fn = {0: nn.Identity(), 1: nn.ReLU(), 2: nn.LeakyReLU(slope), 3: nn.Tanh()}[act]
    pool = nn.MaxPool2d(kernel_size=2, stride=2)
    x = I.x.double().requires_grad_(True)
    p = torch.cat([pool(fn(bn(xs))) for xs in x.view(I.S, I.B, I.C, I.H, I.W).unbind(0)])
    gx, gg, gb = torch.autograd.grad((p * I.gp.double()).sum(), [x, bn.weight, bn.bias])
    close = lambda u, v: float((u - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max()))
    assert torch.equal(p.detach(), ref.p) or close(p.detach(), ref.p)
    assert close(gx, ref.gx) and close(gg, ref.ggamma) and close(gb, ref.gbeta)
    assert int((ref.gy != 0).sum()) <= ref.p.numel()          # one position per window carries the gradient


@pytest.mark.parametrize("case", pool_cases(ref=True), ids=case_id)
def test_winner_margin_holds_for_the_recorded_seed(case):
    row, a, seed = case
    assert margins_hold(row, a, seed), "a window's two largest values nearly tie (or a kink is too near)"
    assert not any(margins_hold(row, a, s) for s in range(seed)), "the table records the FIRST seed that holds"


def test_sync_row_margin():
    row = POOL_SYNC
    act, slope = ACTS[row["act"]]
    ranks = [pool_inputs(row, row["seed"] + 100 * r) for r in range(row["world"])]
    for ga, be in ((ranks[0].gamma, ranks[0].beta), (None, None)):
        ref = bn_ref(to_global([I.x for I in ranks], ranks[0].S), ga, be, None, ranks[0].S, act, slope)
        assert winner_margin(ref, act)[0] >= U_MARGIN


def test_tie_rows_do_tie():
    """the rows built for ties have exact ones in a good share of their windows, in fp32 arithmetic as in fp64"""
    for row, a, seed in pool_cases(ref=False):
        if not row.get("kind"):
            continue
        act, slope = ACTS[a]
        I = pool_inputs(row, seed)
        ref = bn_ref(I.x, I.gamma, I.beta, None, I.S, act, slope)
        y = ref.y.float() if row["kind"] == "saturate" else ref.y    # tanhf reaches 1 where fp64 tanh does not
        win = y.view(I.S * I.B, I.C, I.H // 2, 2, I.W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        top = win.sort(1, descending=True).values
        ties = int((top[:, 0] == top[:, 1]).sum())
        assert ties * 10 >= win.shape[0], (pool_id(row), ties, win.shape[0])


# ------------------------------------------------------------------------------------------------ the module route
def _stack(pool, act=None):
    from Utils import modules as M
    return [nn.Conv2d(2, 4, 3, padding=1, bias=False), M.NormLayer(4, "batchnorm"), act or M.ActFun("relu"), pool,
            nn.Conv2d(4, 4, 3, padding=1, bias=False)]


def test_pool_pattern_conditions(monkeypatch):
    from Utils import modules as M
    from rfn_hip import dist as rdist
    monkeypatch.delenv("RFN_STEPBN_POOL", raising=False)
    x = torch.zeros(6, 4, 8, 6)
    good = _stack(nn.MaxPool2d(kernel_size=2, stride=2))
    assert M._pool_fusable(good, 1, x)
    assert M._pool_fusable(_stack(nn.MaxPool2d(2), nn.Tanh()), 1, x)                       # stride defaults to the kernel
    for bad in (nn.MaxPool2d(2, 2, padding=1), nn.MaxPool2d(2, 2, ceil_mode=True), nn.MaxPool2d(2, 2, return_indices=True),
                nn.MaxPool2d(2, 1), nn.MaxPool2d(3, 2), nn.MaxPool2d(2, 2, dilation=2), nn.AvgPool2d(2, 2)):
        assert not M._pool_fusable(_stack(bad), 1, x), bad
    assert not M._pool_fusable(_stack(nn.MaxPool2d(2, 2), M.tanh0_5()), 1, x)              # not an activation of the kernels
    assert not M._pool_fusable(good[:3], 1, x)                                             # nothing follows the activation
    assert not M._pool_fusable(good, 1, torch.zeros(6, 4, 7, 6)) and not M._pool_fusable(good, 1, torch.zeros(6, 4, 8, 5))
    monkeypatch.setattr(rdist, "sync_batchnorm_on", lambda: True)
    assert not M._pool_fusable(good, 1, x)
    monkeypatch.undo()
    monkeypatch.setenv("RFN_STEPBN_POOL", "0")
    assert not M._pool_fusable(good, 1, x)


def test_run_time_batched_on_cpu_takes_the_old_path(monkeypatch):
    """a CPU tensor: nothing of the fused kernels is called, and the result is the step-wise modules'"""
    from Utils import modules as M

    def never(*a, **k):
        raise AssertionError("the fused path was taken for a CPU tensor")
    monkeypatch.setattr(M.K.StepBatchNormActPoolFn, "apply", never)
    monkeypatch.setattr(M.K.StepBatchNormActFn, "apply", never)
    torch.manual_seed(3)
    seq = nn.Sequential(*_stack(nn.MaxPool2d(kernel_size=2, stride=2))).double().train()
    S, B = 3, 2
    x = torch.randn(S * B, 2, 8, 6, dtype=torch.float64)
    twin = nn.Sequential(*_stack(nn.MaxPool2d(kernel_size=2, stride=2))).double().train()
    twin.load_state_dict(seq.state_dict())
    got = M.run_time_batched(seq, x, S)
    want = torch.cat([twin(xs) for xs in x.view(S, B, 2, 8, 6).unbind(0)])
    assert got.shape == (S * B, 4, 4, 3) and float((got - want).detach().abs().max()) < 1e-12
    assert float((seq[1].norm.running_mean - twin[1].norm.running_mean).abs().max()) < 1e-12
    assert int(seq[1].norm.num_batches_tracked) == S
