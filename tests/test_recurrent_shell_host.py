"""Case tables, launch routes and fp64 references of the recurrent / likelihood shell kernels, without a device.

rfn_stepbn_kernel_label, rfn_convlstm_gates_kernel_label and rfn_latent_step_kernel_label print the host structs the
launchers themselves read (choose_stepbn in csrc/stepbn.hip, choose_stride_grid in csrc/recurrent_shell.hip).  The tables below say, from a reading of
the kernels, which branch each shape of tests/test_recurrent_shell.py is there for; this module holds the library to them
on any machine, and test_recurrent_shell.py runs the same rows on the GPU.

The fp64 references of that module live here too: plain torch written from the formulas of include/rfn_hip.h,
differentiated by autograd where a backward exists, and each checked here against an independent formulation
(nn.BatchNorm2d per step, the oracle's ConvLSTM cell with nonzero peepholes, torch.distributions, O.normal_log_prob), so
that the references are themselves tested.

Activation masks: the BatchNorm backward recomputes act'(u) from u = xhat * gamma + beta in fp32.  For the relu / leaky
rows the table fixes the first generator seed in 0..63 whose fp64 u has min|u| >= 1e-4 (fp32 errs by about 1e-6 there),
so the kernel cannot land on the other side of the kink and no element is excluded; the condition is asserted here.
"""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import rfn_oracle as O
from tests.test_glow_shell_host import fields

ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "leaky": (2, 0.2), "tanh": (3, 0.0)}
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
U_MARGIN = 1e-4

# ---- per-step BatchNorm: (S, B, C, H, W), mis = None | "y" (y / gx one float off 16 bytes) | "x" (x one float off)
#      -> ny, frames per stats block (most .. fewest), stats / apply route, apply sweeps, activations, seed, input kind
BN_ROWS = [
    dict(shape=(3, 4, 6, 8, 8), mis=None, ny=4, frames=(1,), stats="vec", apply="vec4", sweeps=1,
         acts=("none", "relu", "leaky", "tanh"), seed=0),                               # ny = B
    dict(shape=(2, 3, 5, 3, 5), mis=None, ny=3, frames=(1,), stats="scalar", apply="vec1", sweeps=1,
         acts=("none", "relu", "leaky", "tanh"), seed=0),                               # HW = 15
    dict(shape=(5, 2, 16, 2, 2), mis=None, ny=2, frames=(1,), stats="vec", apply="vec4", sweeps=1,
         acts=("none", "relu", "leaky", "tanh"), seed=2),                               # HW4 = 1
    dict(shape=(2, 37, 8, 4, 4), mis=None, ny=16, frames=(3, 2), stats="vec", apply="vec4", sweeps=1,
         acts=("none",), seed=3, kind="plane"),                                         # ny < B; one constant plane
    dict(shape=(9, 7, 64, 2, 2), mis=None, ny=3, frames=(3, 2), stats="vec", apply="vec4", sweeps=1,
         acts=("tanh",), seed=4),                                                       # S*C = 576: the training class
    dict(shape=(9, 7, 64, 2, 2), mis=None, ny=3, frames=(3, 2), stats="vec", apply="vec4", sweeps=1,
         acts=("none",), seed=5, kind="offset"),                                        # x = 1000 + randn
    dict(shape=(9, 5, 256, 2, 2), mis=None, ny=1, frames=(5,), stats="vec", apply="vec4", sweeps=1,
         acts=("tanh",), seed=6),
    dict(shape=(9, 5, 256, 1, 2), mis=None, ny=1, frames=(5,), stats="scalar", apply="vec1", sweeps=1,
         acts=("none",), seed=7),
    dict(shape=(3, 4, 6, 8, 8), mis="y", ny=4, frames=(1,), stats="vec", apply="vec1", sweeps=1,
         acts=("tanh",), seed=8),
    dict(shape=(3, 4, 6, 8, 8), mis="x", ny=4, frames=(1,), stats="scalar", apply="vec1", sweeps=1,
         acts=("none",), seed=9),
    dict(shape=(2, 8, 65, 128, 128), mis=None, ny=8, frames=(1,), stats="vec", apply="vec4", sweeps=2,
         acts=("tanh",), seed=10, big=True),                                            # 16640 > 16384 blocks
    dict(shape=(1, 4, 16, 257, 257), mis=None, ny=4, frames=(1,), stats="scalar", apply="vec1", sweeps=2,
         acts=("none",), seed=11, big=True),                                            # 16512 > 16384 blocks
]
BN_GRID_CAP = 16384
# ---- synchronised BatchNorm: (S, B per rank, C, H, W, world) -> activation, seed
SYNC_ROWS = [
    dict(shape=(3, 2, 6, 4, 4), world=2, act="tanh", seed=20),
    dict(shape=(2, 3, 5, 3, 5), world=3, act="none", seed=21),
    dict(shape=(9, 4, 64, 2, 2), world=2, act="tanh", seed=22),
]
# ---- ConvLSTM gates (N, Hc, HW) and latent step (B, ZHW) -> grid, sweeps
GATES_CASES = {(3, 5, 6): dict(grid=1, sweeps=1), (4, 60, 64): dict(grid=60, sweeps=1),
               (33, 64, 256): dict(grid=2048, sweeps=2)}                                # 540672 > 2048 * 256
LATENT_CASES = {(3, 28): dict(grid=1, sweeps=1), (5, 63): dict(grid=2, sweeps=1),
                (4, 66000): dict(grid=1024, sweeps=2)}                                  # 264000 > 1024 * 256
# ---- Gaussian (N, Cz, HW): e += 256 steps of a block; channel stats (N, C, HW): i += 256 steps
GAUSS_CASES = {(3, 5, 8): 1, (2, 4, 64): 1, (2, 257, 1): 2, (70, 2, 16): 1, (3, 3, 4096): 48}
STATS_CASES = {(7, 5, 18): 1, (5, 3, 100): 2, (2, 4, 4096): 32}


class Bag(dict):
    __getattr__ = dict.__getitem__


def bn_id(row):
    return "x".join(map(str, row["shape"])) + ("-" + row["kind"] if row.get("kind") else "") + \
        ("-mis" + row["mis"] if row["mis"] else "")


def bn_aligned_mask(row):
    """the `aligned` argument of rfn_stepbn_kernel_label for the pointers the GPU test passes (forward and backward)"""
    return {None: 3, "y": 1, "x": 0}[row["mis"]]


# ------------------------------------------------------------------------------------------------ inputs
def bn_inputs(row):
    """CPU fp32 inputs of a BatchNorm row: x [S*B, C, H, W] = 2 randn + 0.7, incoming gradient g, gamma in [0.5, 1.5],
    beta in [-0.5, 0.5], nonzero running statistics.  kind "plane": one (step, channel) plane is constant;
    "offset": x = 1000 + randn; "dyadic": x a multiple of 1/2 in [-2, 2], g of 1/8 in [-1, 1]."""
    S, B, C, H, W = row["shape"]
    kind = row.get("kind")
    gen = torch.Generator().manual_seed(row["seed"])
    gamma = 0.5 + torch.rand(C, generator=gen)
    beta = torch.rand(C, generator=gen) - 0.5
    rm, rv = torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
    n = (S * B, C, H, W)
    if kind == "dyadic":
        x = torch.randint(-4, 5, n, generator=gen).float() / 2
        g = torch.randint(-8, 9, n, generator=gen).float() / 8
    else:
        x = torch.randn(n, generator=gen)
        x = 1000 + x if kind == "offset" else 2 * x + 0.7
        g = torch.randn(n, generator=gen)
    if kind == "plane":
        x.view(S, B, C, H, W)[S - 1, :, C // 2] = 1.25
    return Bag(S=S, B=B, C=C, H=H, W=W, HW=H * W, x=x, g=g, gamma=gamma, beta=beta, rm=rm, rv=rv, nbt=5)


# ------------------------------------------------------------------------------------------------ fp64 references
def act64(u, act, slope):
    if act == 1:
        return torch.relu(u)
    if act == 2:
        return torch.where(u > 0, u, slope * u)
    if act == 3:
        return torch.tanh(u)
    return u


def bn_ref(x, gamma, beta, g, S, act, slope, eps=BN_EPS):
    """include/rfn_hip.h, per-step BatchNorm: statistics of each step's B samples per channel over (B, HW), biased
    variance, y = act(xhat gamma + beta); gradients of sum(y g) by autograd.  fp64 on the device of x.
    -> Bag(y, mean [S, C], var [S, C], u, gx, ggamma, gbeta) (ggamma / gbeta None without affine parameters)"""
    SB, C, H, W = x.shape
    B = SB // S
    xl = x.detach().double().clone().requires_grad_(g is not None)
    ga = None if gamma is None else gamma.detach().double().clone().requires_grad_(g is not None)
    be = None if beta is None else beta.detach().double().clone().requires_grad_(g is not None)
    xv = xl.view(S, B, C, H * W)
    mean = xv.mean((1, 3))
    var = ((xv - mean.view(S, 1, C, 1)) ** 2).mean((1, 3))
    u = (xv - mean.view(S, 1, C, 1)) / torch.sqrt(var.view(S, 1, C, 1) + eps)
    if ga is not None:
        u = u * ga.view(1, 1, C, 1) + be.view(1, 1, C, 1)
    y = act64(u, act, slope).reshape(SB, C, H, W)
    out = Bag(y=y.detach(), mean=mean.detach(), var=var.detach(), u=u.detach().reshape(SB, C, H, W),
              gx=None, ggamma=None, gbeta=None)
    if g is not None:
        wrt = [xl] + ([ga, be] if ga is not None else [])
        gr = torch.autograd.grad((y * g.double()).sum(), wrt)
        out.gx = gr[0]
        if ga is not None:
            out.ggamma, out.gbeta = gr[1], gr[2]
    return out


def ema_ref(mean, var, n, rm, rv, momentum=BN_MOMENTUM):
    """the S exponential-average updates of the step-wise calls, one after the other in fp64: the mean and the UNBIASED
    variance (var * n / (n - 1)) of each step"""
    rm, rv = rm.double().clone(), rv.double().clone()
    for s in range(mean.shape[0]):
        rm = (1 - momentum) * rm + momentum * mean[s]
        rv = (1 - momentum) * rv + momentum * var[s] * (n / max(n - 1, 1))
    return rm, rv


def to_global(ts, S):
    """per-rank step-major tensors [S*B, ...] -> the step-major global batch [S*world*B, ...]"""
    B = ts[0].shape[0] // S
    return torch.cat([t.view((S, B) + tuple(t.shape[1:])) for t in ts], 1).reshape((-1,) + tuple(ts[0].shape[1:]))


def from_global(t, S, world):
    B = t.shape[0] // (S * world)
    v = t.view((S, world, B) + tuple(t.shape[1:]))
    return [v[:, r].reshape((S * B,) + tuple(t.shape[1:])) for r in range(world)]


def bn_sync_ref(xs, gamma, beta, gs, S, act, slope):
    """synchronised BatchNorm over len(xs) ranks = bn_ref on the global batch: per-rank y / gx slices, the global
    statistics and the GLOBAL parameter gradients (a rank's are these divided by the number of ranks)"""
    world = len(xs)
    r = bn_ref(to_global(xs, S), gamma, beta, to_global(gs, S), S, act, slope)
    return Bag(y=from_global(r.y, S, world), gx=from_global(r.gx, S, world), mean=r.mean, var=r.var, ggamma=r.ggamma,
               gbeta=r.gbeta)


def gates_ref(cc, c_prev, wci, wcf, wco):
    """include/rfn_hip.h a9: cc [N, 4 Hc, HW] in gate order i, f, o, g; peepholes [Hc*HW] or None -> (h, c, gates)"""
    N, Hc, HW = c_prev.shape
    cci, ccf, cco, ccg = cc.view(N, 4, Hc, HW).unbind(1)
    z = lambda w: 0.0 if w is None else w.view(1, Hc, HW)
    i = torch.sigmoid(cci + z(wci) * c_prev)
    f = torch.sigmoid(ccf + z(wcf) * c_prev)
    g = torch.tanh(ccg)
    cn = f * c_prev + i * g
    o = torch.sigmoid(cco + z(wco) * cn)
    return o * torch.tanh(cn), cn, torch.stack((i, f, o, g), 1).reshape(N, 4 * Hc, HW)


def softplus64(raw):
    return F.softplus(raw, threshold=20.0)        # the kernels' (torch's) threshold: x itself above 20


def latent_ref(enc, pri, eps_p, eps_q, res_q):
    """include/rfn_hip.h a10: enc / pri [B, 2 ZHW] (loc | raw scale) -> zt, zxt, kl, em, es and A = the sum of the
    absolute values of the KL's four terms"""
    ZHW = enc.shape[1] // 2
    pm, ps = pri[:, :ZHW], softplus64(pri[:, ZHW:])
    em, es = enc[:, :ZHW] + (pm if res_q else 0.0), softplus64(enc[:, ZHW:])
    r2, d2 = (es / ps) ** 2, ((em - pm) / ps) ** 2
    kl = 0.5 * (r2 + d2 - 1.0 - torch.log(r2))
    return Bag(zt=pm + ps * eps_p, zxt=em + es * eps_q, kl=kl, em=em, es=es, A=0.5 * (r2 + d2 + 1.0 + torch.log(r2).abs()))


def gauss_params(o, layout, std_mode):
    """o [N, 2 Cz, HW] -> (mean, std, log std): layout 0 interleaved (2c, 2c+1), 1 halves (c, Cz+c)"""
    Cz = o.shape[1] // 2
    mean, raw = (o[:, 0::2], o[:, 1::2]) if layout == 0 else (o[:, :Cz], o[:, Cz:])
    if std_mode == 0:
        std = softplus64(raw) + 1e-8
        return mean, std, torch.log(std)
    return mean, torch.exp(raw), raw


def gauss_ref(z, o, layout, std_mode):
    """per-frame log N(z; mean, std) summed over (c, p) -> (logp [N], A [N] = the sum of the absolute terms)"""
    mean, std, logstd = gauss_params(o, layout, std_mode)
    q = (z - mean) ** 2 / (2 * std * std)
    half = 0.5 * math.log(2 * math.pi)
    return (-q - logstd - half).sum((1, 2)), (q + logstd.abs() + half).sum((1, 2))


def gauss_sample_ref(o, eps, temperature, layout, std_mode):
    mean, std, _ = gauss_params(o, layout, std_mode)
    return mean + std * temperature * eps


def channel_stats_ref(x):
    """x [N, C, HW] -> mean, unbiased variance per channel"""
    m = x.mean((0, 2))
    n = x.shape[0] * x.shape[2]
    return m, ((x - m.view(1, -1, 1)) ** 2).sum((0, 2)) / (n - 1)


# ------------------------------------------------------------------------------------------------ routes
@pytest.fixture(scope="module")
def lib():
    from rfn_hip import lib as L_
    L_.load()
    return L_


def bn_label(lib, row, bwd=0):
    S, B, C, H, W = row["shape"]
    return lib.load().rfn_stepbn_kernel_label(S, B, C, H * W, bn_aligned_mask(row), bwd).decode()


def gates_label(lib, N, Hc, HW):
    return lib.load().rfn_convlstm_gates_kernel_label(N, Hc, HW).decode()


def latent_label(lib, B, ZHW):
    return lib.load().rfn_latent_step_kernel_label(B, ZHW).decode()


@pytest.mark.parametrize("row", BN_ROWS, ids=bn_id)
def test_batchnorm_route_is_the_table_row(lib, row):
    S, B, C, H, W = row["shape"]
    HW = H * W
    for bwd in (0, 1):
        name, f = fields(bn_label(lib, row, bwd))
        assert name == "stepbn"
        assert (f["ny"], f["stats"], f["apply"], f["sweeps"]) == (row["ny"], row["stats"], row["apply"], row["sweeps"]), f
        assert f["ny"] * 2 * S * C == lib.load().rfn_stepbn_scratch_floats(S, B, C)
        assert f["ny"] == max(1, min(2048 // (S * C), 16, B))
        # the frames a stats / reduce block (sc, j) sees: j, j + ny, ...
        per_block = sorted({len(range(j, B, f["ny"])) for j in range(f["ny"])}, reverse=True)
        assert tuple(per_block) == row["frames"] and sum(len(range(j, B, f["ny"])) for j in range(f["ny"])) == B
        nthr = S * B * C * HW // (4 if f["apply"] == "vec4" else 1)
        blocks = -(-nthr // 256)
        assert f["grid"] == min(blocks, BN_GRID_CAP) and f["sweeps"] == -(-blocks // f["grid"])
        assert (f["stats"] == "vec") == (HW % 4 == 0 and row["mis"] != "x")
        assert (f["apply"] == "vec4") == (HW % 4 == 0 and row["mis"] is None)
    assert S * B * C * HW < 2 ** 31


def test_tables_reach_every_route(lib):
    bn = [(r, fields(bn_label(lib, r))[1]) for r in BN_ROWS]
    assert {(f["stats"], f["apply"]) for _, f in bn} == {("vec", "vec4"), ("scalar", "vec1"), ("vec", "vec1")}
    assert {(f["apply"], f["sweeps"]) for _, f in bn} >= {("vec4", 1), ("vec4", 2), ("vec1", 1), ("vec1", 2)}
    nys = {f["ny"] for _, f in bn}
    assert {1, 3, 16} <= nys and any(f["ny"] < r["shape"][1] for r, f in bn) and any(f["ny"] == r["shape"][1] for r, f in bn)
    assert any(len(r["frames"]) == 2 for r, _ in bn)                   # uneven frame counts over the blocks of a pair
    assert any(r["shape"][3] * r["shape"][4] == 4 and f["stats"] == "vec" for r, f in bn)      # HW4 = 1
    assert any(r["shape"][0] * r["shape"][2] in (576, 1152, 2304) for r, _ in bn)              # training S*C
    assert {a for r, _ in bn for a in r["acts"]} == set(ACTS)
    small = sorted(BN_ROWS, key=lambda r: math.prod(r["shape"]))[:3]
    for r in BN_ROWS:   # the kinked activations only on the three smallest shapes (the mask-margin seeds)
        assert set(r["acts"]) <= {"none", "tanh"} or r["shape"] in [s["shape"] for s in small]
    assert {fields(gates_label(lib, *c))[1]["sweeps"] for c in GATES_CASES} == {1, 2}
    assert {fields(latent_label(lib, *c))[1]["sweeps"] for c in LATENT_CASES} == {1, 2}
    assert {v > 1 for v in GAUSS_CASES.values()} == {False, True} == {v > 1 for v in STATS_CASES.values()}


def test_gates_latent_gauss_routes_are_the_table_rows(lib):
    for (N, Hc, HW), want in GATES_CASES.items():
        name, f = fields(gates_label(lib, N, Hc, HW))
        blocks = -(-N * Hc * HW // 256)
        assert name == "convlstm_gates" and f == want, (f, want)
        assert f["grid"] == min(blocks, 2048) and f["sweeps"] == -(-blocks // f["grid"])
    for (B, ZHW), want in LATENT_CASES.items():
        name, f = fields(latent_label(lib, B, ZHW))
        blocks = -(-B * ZHW // 256)
        assert name == "latent_step" and f == want, (f, want)
        assert f["grid"] == min(blocks, 1024) and f["sweeps"] == -(-blocks // f["grid"])
    for (N, Cz, HW), steps in GAUSS_CASES.items():       # one 256-thread block per frame, e += 256
        assert -(-Cz * HW // 256) == steps
    for (N, C, HW), steps in STATS_CASES.items():        # one 256-thread block per channel, i += 256
        assert -(-N * HW // 256) == steps
    L = lib.load()
    assert L.rfn_stepbn_kernel_label(0, 4, 4, 4, 3, 0) == b"unsupported"
    assert L.rfn_stepbn_kernel_label(2, 4, 4, 1 << 27, 3, 0) == b"unsupported"      # 2^31 elements: the launcher's -3
    assert L.rfn_convlstm_gates_kernel_label(0, 4, 4) == b"unsupported"
    assert L.rfn_latent_step_kernel_label(3, 0) == b"unsupported"


# ------------------------------------------------------------------------------------------------ mask margin
def _kinked(rows):
    return [r for r in rows if {"relu", "leaky"} & set(r["acts"])]


@pytest.mark.parametrize("row", _kinked(BN_ROWS), ids=bn_id)
def test_activation_mask_margin_holds_for_the_recorded_seed(row):
    """min|u| >= 1e-4 in fp64, with and without affine parameters, and the seed is the first of 0..63 that does"""
    def margin(seed):
        I = bn_inputs(dict(row, seed=seed))
        return min(float(bn_ref(I.x, ga, be, None, I.S, 0, 0.0).u.abs().min())
                   for ga, be in ((I.gamma, I.beta), (None, None)))
    assert margin(row["seed"]) >= U_MARGIN
    assert all(margin(s) < U_MARGIN for s in range(row["seed"]))


# ------------------------------------------------------------------------------------------------ the references
def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())


def _act_module(act, slope):
    return [nn.Identity(), nn.ReLU(), nn.LeakyReLU(slope), nn.Tanh()][act]


def _bn_module_per_step(x, gamma, beta, g, S, act, slope, rm, rv, nbt):
    """S calls of nn.BatchNorm2d (double, training mode) + the activation: what the model's step-wise calls compute"""
    C = x.shape[1]
    bn = nn.BatchNorm2d(C, eps=BN_EPS, momentum=BN_MOMENTUM, affine=gamma is not None).double().train()
    with torch.no_grad():
        if gamma is not None:
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
        bn.num_batches_tracked.fill_(nbt)
    xl = x.double().clone().requires_grad_()
    y = torch.cat([_act_module(act, slope)(bn(xs)) for xs in xl.view((S, -1) + tuple(x.shape[1:])).unbind(0)], 0)
    (y * g.double()).sum().backward()
    return y.detach(), xl.grad, bn


@pytest.mark.parametrize("affine", (True, False), ids=("affine", "plain"))
@pytest.mark.parametrize("row", [r for r in BN_ROWS if not r.get("big") and not r["mis"]], ids=bn_id)
def test_batchnorm_reference_is_batchnorm2d_per_step(row, affine):
    I = bn_inputs(row)
    ga, be = (I.gamma, I.beta) if affine else (None, None)
    for a in row["acts"]:
        act, slope = ACTS[a]
        r = bn_ref(I.x, ga, be, I.g, I.S, act, slope)
        y, gx, bn = _bn_module_per_step(I.x, ga, be, I.g, I.S, act, slope, I.rm, I.rv, I.nbt)
        assert _rel(r.y, y) < 1e-12 and _rel(r.gx, gx) < 1e-12
        if affine:
            assert _rel(r.ggamma, bn.weight.grad) < 1e-12 and _rel(r.gbeta, bn.bias.grad) < 1e-12
        rm, rv = ema_ref(r.mean, r.var, I.B * I.HW, I.rm, I.rv)
        assert _rel(rm, bn.running_mean) < 1e-12 and _rel(rv, bn.running_var) < 1e-12
        assert int(bn.num_batches_tracked) == I.nbt + I.S
        # the closed form the kernel is handed (Utils.modules._ema_coef) is the same recurrence
        from Utils.modules import _ema_coef
        coef, coef_u = _ema_coef(I.S, BN_MOMENTUM, I.B * I.HW, "cpu")
        decay = (1.0 - BN_MOMENTUM) ** I.S
        assert _rel(decay * I.rm.double() + (coef.double().view(-1, 1) * r.mean).sum(0), rm) < 1e-6      # (fp32 coef)
        assert _rel(decay * I.rv.double() + (coef_u.double().view(-1, 1) * r.var).sum(0), rv) < 1e-6
    if row.get("kind") == "plane":
        assert float(r.var[I.S - 1, I.C // 2]) == 0.0


def sync_inputs(row):
    """per-rank inputs of a synchronised row: every rank its own x and g, shared parameters"""
    S, B, C, H, W = row["shape"]
    ranks = [bn_inputs(dict(shape=row["shape"], seed=row["seed"] * 10 + r, mis=None)) for r in range(row["world"])]
    return ranks, ranks[0].gamma, ranks[0].beta


@pytest.mark.parametrize("row", SYNC_ROWS, ids=lambda r: "x".join(map(str, r["shape"])) + "-w%d" % r["world"])
def test_sync_reference_is_batchnorm2d_on_the_global_batch(row):
    ranks, gamma, beta = sync_inputs(row)
    S, B = row["shape"][:2]
    world = row["world"]
    act, slope = ACTS[row["act"]]
    r = bn_sync_ref([I.x for I in ranks], gamma, beta, [I.g for I in ranks], S, act, slope)
    C = row["shape"][2]
    bn = nn.BatchNorm2d(C, eps=BN_EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    leaves = [I.x.double().clone().requires_grad_() for I in ranks]
    loss = 0.0
    ys = [[None] * S for _ in range(world)]
    for s in range(S):      # step s of every rank, concatenated: the global batch of that step
        y = _act_module(act, slope)(bn(torch.cat([x[s * B:(s + 1) * B] for x in leaves], 0)))
        for k in range(world):
            ys[k][s] = y[k * B:(k + 1) * B]
            loss = loss + (ys[k][s] * ranks[k].g[s * B:(s + 1) * B].double()).sum()
    loss.backward()
    for k in range(world):
        assert _rel(torch.cat(ys[k], 0), r.y[k]) < 1e-12 and _rel(leaves[k].grad, r.gx[k]) < 1e-12
    assert _rel(bn.weight.grad, r.ggamma) < 1e-12 and _rel(bn.bias.grad, r.gbeta) < 1e-12


@pytest.mark.parametrize("pe", (False, True), ids=("nopeephole", "peephole"))
def test_gates_reference_is_the_oracle_cell(pe):
    """O.convlstm_cell with a 1x1 identity convolution (cc = x exactly) and nonzero Wci / Wcf / Wco"""
    N, Hc, H, W = 3, 5, 2, 3
    gen = torch.Generator().manual_seed(31)
    cc = 2 * torch.randn(N, 4 * Hc, H, W, generator=gen, dtype=torch.float64)
    c = torch.randn(N, Hc, H, W, generator=gen, dtype=torch.float64)
    h = torch.randn(N, Hc, H, W, generator=gen, dtype=torch.float64)
    w = torch.zeros(4 * Hc, 5 * Hc, 1, 1, dtype=torch.float64)
    w[:, :4 * Hc, 0, 0] = torch.eye(4 * Hc, dtype=torch.float64)
    sd = {"conv.0.weight": w}
    wc = [None, None, None]
    if pe:
        wc = [0.5 * torch.randn(1, Hc, H, W, generator=gen, dtype=torch.float64) for _ in range(3)]
        sd.update(Wci=wc[0], Wcf=wc[1], Wco=wc[2])
    h_o, c_o = O.convlstm_cell(sd, "", cc, h, c)
    h_r, c_r, gates = gates_ref(cc.view(N, 4 * Hc, H * W), c.view(N, Hc, H * W), *[None if t is None else t.reshape(-1) for t in wc])
    assert float((h_r.view_as(h_o) - h_o).abs().max()) < 1e-14 and float((c_r.view_as(c_o) - c_o).abs().max()) < 1e-14
    assert gates.shape == (N, 4 * Hc, H * W)
    if pe:      # the peepholes matter: the reference without them differs
        h_0, _, _ = gates_ref(cc.view(N, 4 * Hc, H * W), c.view(N, Hc, H * W), None, None, None)
        assert float((h_0.view_as(h_o) - h_o).abs().max()) > 1e-3


@pytest.mark.parametrize("res_q", (False, True))
def test_latent_reference_is_torch_distributions(res_q):
    import torch.distributions as td
    B, ZHW = 3, 28
    gen = torch.Generator().manual_seed(32)
    enc, pri = (1.5 * torch.randn(B, 2 * ZHW, generator=gen, dtype=torch.float64) for _ in range(2))
    enc[0, ZHW + 1], pri[1, ZHW + 2], enc[2, ZHW + 3] = 19.9, 20.1, 30.0
    ep, eq = (torch.randn(B, ZHW, generator=gen, dtype=torch.float64) for _ in range(2))
    r = latent_ref(enc, pri, ep, eq, res_q)
    pm, ps = pri[:, :ZHW], F.softplus(pri[:, ZHW:])
    em, es = enc[:, :ZHW] + (pm if res_q else 0), F.softplus(enc[:, ZHW:])
    kl = td.kl_divergence(td.Normal(em, es), td.Normal(pm, ps))
    assert float((r.kl - kl).abs().max()) < 1e-12 and bool((r.A >= r.kl.abs()).all())
    assert torch.equal(r.zt, pm + ps * ep) and torch.equal(r.zxt, em + es * eq) and torch.equal(r.em, em)


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("std_mode", (0, 1))
def test_gauss_reference_is_the_oracle_log_prob(layout, std_mode):
    N, Cz, HW = 3, 5, 8
    gen = torch.Generator().manual_seed(33)
    z = torch.randn(N, Cz, HW, generator=gen, dtype=torch.float64)
    o = torch.randn(N, 2 * Cz, HW, generator=gen, dtype=torch.float64)
    mean, raw = O.split_feature(o, "cross" if layout == 0 else "split")
    std = F.softplus(raw) + 1e-8 if std_mode == 0 else torch.exp(raw)
    want = O.normal_log_prob(z, mean, std).sum((1, 2))
    logp, A = gauss_ref(z, o, layout, std_mode)
    assert float((logp - want).abs().max()) < 1e-12 and bool((A >= logp.abs()).all())
    eps = torch.randn(N, Cz, HW, generator=gen, dtype=torch.float64)
    assert float((gauss_sample_ref(o, eps, 0.7, layout, std_mode) - (mean + std * 0.7 * eps)).abs().max()) < 1e-14
    m, v = channel_stats_ref(z)
    v2, m2 = torch.var_mean(z.permute(1, 0, 2).reshape(Cz, -1), 1, unbiased=True)
    assert float((m - m2).abs().max()) < 1e-14 and float((v - v2).abs().max()) < 1e-14
