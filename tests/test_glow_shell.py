"""The four shell entry points of a flow level, called directly, against fp64 on every launch route.

rfn_glow_shell_fwd_f32 (+ rfn_logdet_reduce_f32), rfn_glow_shell_bwd_f32 and rfn_actnorm_invconv_bwd_ld_f32 run between
and around the K Glow steps of a level; the per-frame log-det they produce is the loss.  The reference is one fp64 torch
function on the CPU written from the formulas of include/rfn_hip.h and oracle/rfn_oracle.py (clamp_log_scale,
affine_coupling, actnorm, invconv), differentiated by autograd:
    o = (tapgather(P) + b3) * exp(3 l3),  P[n, t*C + c, y + t//3 - 1, x + t%3 - 1]         (or o given)
    shift = o[:, 0::2], s = o[:, 1::2], ls = clamp(s);  z2' = (z2 + shift) * exp(ls);  ld[n] = sum ls
    head: znext = W ((v + bias) * exp(logs)),  ld[n] += H*W * sum_c logs[c] with ld_const
    backward: the conv3 output u (before bias and exp(3 l3)) and the previous step's post-InvConv tensor are leaves:
    gpre = dL/du, gz_prev[:, :C/2] is the pass-through part only.
The shapes are the rows of tests/test_glow_shell_host.py (FWD_CASES / BWD_CASES), which holds the library's route labels
to the branch each row is there for; the labels are printed here next to the measured errors.

Per forward case: head-only, tail-only and tail+head launches into three NaN-filled partial buffers, reduced together
(accumulate = 1) onto a nonzero log-det; z, znext and o_in are channel-slice views of sentinel-filled parents; every
launch runs twice and must repeat bit for bit.  Per backward case: both entry points, with and without glogdet, every
accumulated output pre-filled with nonzero values, every written output a NaN-filled view.

Bounds (not fitted to the kernels):
  elementwise outputs   max|d| / max|ref| < 1e-5      (the suite's bound for these kernels' unfused siblings)
  reduced gradients     max|d| / max|ref| < 1e-4      (same source)
  per-frame log-det     |d_n| <= 1e-5 * A_n,  A_n = fp64 sum of |ls| over the frame and the launches + H*W * sum|logs|
                        per ld_const launch: fp32 summation plus a few ulp per tanhf / log1pf / atanf is about 1e-6 A_n
  exact                 clamp none, s and logs multiples of 1/8: every fp32 sum is exact in any order, so the reduced
                        log-det is torch.equal to the integer-computed value (block / slot / frame indexing, bit for
                        bit); likewise o_out from dyadic P and b3 with l3 = 0

Measured on an MI355X (max over the cases of a route class):
  forward route (log-det class, PB, product)   elementwise  log-det/A_n   cases (/P: also with the P tail)
    frame          PB=256  global                1.5e-7       5.6e-8        64x4x32x32/P
    frame          PB=32   lds2                  1.6e-7       1.5e-8        5x16x8x8
    pow2x64        PB=128  lds4                  2.1e-7       5.1e-8        640x16x8x8
    pow2x64        PB=256  global                1.6e-7       5.0e-8        1024x4x8x8, 512x4x8x16
    pow2x32        PB=64   global                1.9e-7       6.3e-8        600x4x4x8/P
    pow2x16        PB=32   lds4                  3.1e-7       1.4e-8        4x32x4x4/P
    pow2x16        PB=32   global                2.6e-7       7.9e-9        3x24x4x4
    pow2x8         PB=32   global                9.7e-8       1.4e-8        9x8x2x4
    pow2x4         PB=32   lds4                  2.7e-7       9.7e-9        6x64x2x2
    pow2x4         PB=32   lds2                  5.3e-7       3.9e-8        3x48x2x2, 2x176x2x2 (146 KB of LDS)
    pow2x4         PB=32   global                4.6e-7       3.8e-8        2x186x2x2 (162 KB: the limit)
    frame+generic  PB=32   global                1.6e-7       1.3e-8        3x6x6x6/P, 3x12x12x12
    generic        PB=32   global                1.9e-7       2.1e-7        7x4x3x5/P, 70x2x1x1, 37x2x1x2
  backward route (both entry points, with and without glogdet)               elementwise  reduced
    small<4>  grid=256 sweeps=2                                 80x4x1024     2.4e-7       5.2e-7
    small<8>  grid=256 sweeps=2                                 300x8x225     1.6e-7       9.4e-7
    small<4>  grid=2   sweeps=1                                 3x4x100       1.3e-7       3.8e-7
    small<8>  grid=2   sweeps=1                                 5x8x64        2.3e-7       1.9e-7
    big PB=256 grid=512 ny=1 split sweeps=2                     160x12x1024   2.4e-7       2.9e-6
    big PB=256 grid=160 ny=2 split                              640x16x64     1.8e-7       9.2e-7
    big PB=128 grid=80  ny=4 owned                              640x32x16     2.9e-7       5.9e-7
    big PB=64  grid=40  ny=8 owned                              640x64x4      3.2e-7       4.9e-7
    big PB=256 grid=1   ny=3 split                              3x6x16        1.8e-7       2.2e-7
    big PB=256 grid=1   ny=5 split                              7x10x15       1.4e-7       1.2e-7
    big PB=64  grid=1   ny=8 owned (88 KB of LDS)               4x96x16       3.2e-7       2.6e-7
    big PB=64  grid=1   ny=8 owned (161 KB: the tail limit)     2x144x4       3.6e-7       3.2e-7
  The exact tests hold on all 18 forward rows (and the 5 P-tail rows); every repeated launch was bit-identical.
  Wall time of the module on the MI355X machine: 3 s for 60 tests, the slowest (64x4x32x32, with its fp64 tap gather) 0.4 s.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_glow_shell_host import BWD_CASES, FWD_CASES, bwd_label, fwd_label

pytestmark = pytest.mark.gpu

_i, _l = ctypes.c_int, ctypes.c_long
SENT = 777.0                      # fills the channels of a parent tensor that a kernel must not touch
NAN = float("nan")
EW_BOUND, RED_BOUND, LD_BOUND = 1e-5, 1e-4, 1e-5
CLAMPS = ("realnvp", "glow", "softclamp", "none")       # clamp_type 0 .. 3 (rfn_hip.ops.CLAMP)
P_TAIL = {(64, 4, 32, 32), (3, 6, 6, 6), (600, 4, 4, 8), (4, 32, 4, 4), (7, 4, 3, 5)}   # rows that also run the P tail
ids = lambda c: "x".join(map(str, c))


@pytest.fixture(scope="module")
def L():
    from rfn_hip import lib
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return lib


# ------------------------------------------------------------------------------------------------ helpers
def view_of(src):
    """a channel-slice view [:, 1:C+1] of a wider SENT-filled device tensor, holding `src` (a CPU tensor) or NaN (src =
    a shape: an output the kernel must write completely) -> (parent, view)"""
    shape = tuple(src.shape) if torch.is_tensor(src) else tuple(src)
    parent = torch.full((shape[0], shape[1] + 3) + shape[2:], SENT, device="cuda", dtype=torch.float32)
    v = parent[:, 1:shape[1] + 1]
    if torch.is_tensor(src):
        v.copy_(src)
    else:
        v.fill_(NAN)
    return parent, v


def untouched(parent):
    C = parent.shape[1] - 3
    return bool((parent[:, :1] == SENT).all()) and bool((parent[:, C + 1:] == SENT).all())


def relerr(got, ref):
    """max|got - ref| / max|ref| in fp64 (NaN if anything was left unwritten)"""
    d = (got.detach().double().cpu() - ref.detach().double()).abs().max()
    return float(d / ref.detach().abs().max().clamp_min(1e-300))


def clamp64(s, ct, scale, shift):
    """oracle.clamp_log_scale; scale / shift per coupling channel"""
    if ct == 0:
        shp = (1, -1) + (1,) * (s.dim() - 2)
        return scale.view(shp) * torch.tanh(s) + shift.view(shp)
    if ct == 1:
        return torch.log(torch.sigmoid(s + 2.0))
    if ct == 2:
        return 2.5 * 0.636 * torch.atan(s / 2.5)
    return s


def tapgather(P, C):
    """sum over the nine taps t of P[n, t*C + c, y + t//3 - 1, x + t%3 - 1], zero outside the map"""
    N, _, H, W = P.shape
    Pp = F.pad(P.reshape(N, 9, C, H, W), (1, 1, 1, 1))
    return sum(Pp[:, t, :, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9))


class Bag(dict):
    __getattr__ = dict.__getitem__


# ------------------------------------------------------------------------------------------------ forward
def fwd_inputs(case, dyadic, seed):
    N, C, H, W = case
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d8 = lambda *s: torch.randint(-8, 9, s, generator=g).float() / 8
    I = Bag(N=N, C=C, H=H, W=W)
    if dyadic:      # multiples of 1/8 in [-1, 1], drawn per element (so per frame): sums are exact in fp32
        I.update(z=d8(N, C, H, W), o=d8(N, C, H, W), b3=d8(C), l3=torch.zeros(C), bias=d8(C), logs=d8(C), Wm=d8(C, C),
                 scale=torch.ones(C // 2), shift=torch.zeros(C // 2), init=d8(N) * 4)
        I.P = d8(N, 9 * C, H, W) if case in P_TAIL else None
    else:
        o = r(N, C, H, W)
        o[:, 0::2] *= 0.5
        I.update(z=r(N, C, H, W), o=o, b3=0.1 * r(C), l3=0.1 * r(C), bias=0.5 * r(C), logs=0.3 * r(C),
                 Wm=r(C, C) / math.sqrt(C), scale=0.5 + torch.rand(C // 2, generator=g), shift=0.1 * r(C // 2),
                 init=r(N))
        I.P = r(N, 9 * C, H, W) / 3 if case in P_TAIL else None
    return I


def fwd_ref(I, tail, head, ct, ld_const):
    """fp64: (dict of z / o / znext, ld [N], A [N])"""
    Ch, HW = I.C // 2, I.H * I.W
    v = I.z.double()
    out, ld, A = {}, torch.zeros(I.N, dtype=torch.float64), torch.zeros(I.N, dtype=torch.float64)
    if tail:
        if tail == "P":
            o = (tapgather(I.P.double(), I.C) + I.b3.double().view(1, -1, 1, 1)) * torch.exp(3 * I.l3.double()).view(1, -1, 1, 1)
            out["o"] = o
        else:
            o = I.o.double()
        ls = clamp64(o[:, 1::2], ct, I.scale.double(), I.shift.double())
        v = torch.cat([v[:, :Ch], (v[:, Ch:] + o[:, 0::2]) * torch.exp(ls)], 1)
        out["z"] = v
        ld = ld + ls.sum((1, 2, 3))
        A = A + ls.abs().sum((1, 2, 3))
    if head:
        y = (v + I.bias.double().view(1, -1, 1, 1)) * torch.exp(I.logs.double()).view(1, -1, 1, 1)
        out["znext"] = torch.einsum("ij,njhw->nihw", I.Wm.double(), y)
        if ld_const:
            ld = ld + HW * I.logs.double().sum()
            A = A + HW * I.logs.double().abs().sum()
    return out, ld, A


def fwd_modes(tail, ld_const_th):
    """the three launches of a case: (name, tail kind, head, ld_const)"""
    return (("head", None, True, 1), ("tail", tail, False, 0), ("tail+head", tail, True, ld_const_th))


def fwd_run(L, I, tail, ct, ld_const_th):
    """the three launches into NaN-filled partials + one reduce onto I.init -> dict of CPU results"""
    N, C, H, W = I.N, I.C, I.H, I.W
    dev = lambda t: None if t is None else t.cuda()
    ldf = int(L.load().rfn_glow_shell_fwd_ld_floats(N, C, H, W))
    ldp = torch.full((3, ldf), NAN, device="cuda", dtype=torch.float32)
    b3, l3, bias, logs, Wm = dev(I.b3), dev(I.l3), dev(I.bias), dev(I.logs), dev(I.Wm).contiguous()
    scale, shift = (dev(I.scale), dev(I.shift)) if ct == 0 else (None, None)
    P = dev(I.P) if tail == "P" else None
    res = {}
    for k, (name, tk, head, ldc) in enumerate(fwd_modes(tail, ld_const_th)):
        zpar, z = view_of(I.z)
        zp, zns = L.frames(z, "z")
        keep = [zpar]
        o_out = None
        if tk == "P":
            o_out = torch.full((N, C, H, W), NAN, device="cuda", dtype=torch.float32)
            targs = (L.dev(P), None, _l(0), L.dev(b3), L.dev(l3), L.dev(o_out), L.dev(scale), L.dev(shift))
        elif tk == "o":
            opar, o = view_of(I.o)
            keep.append(opar)
            op, ons = L.frames(o, "o")
            targs = (None, op, _l(ons), None, None, None, L.dev(scale), L.dev(shift))
        else:
            targs = (None, None, _l(0), None, None, None, None, None)
        if head:
            npar, zn = view_of((N, C, H, W))
            znp, znns = L.frames(zn, "znext")
            hargs = (L.dev(bias), L.dev(logs), L.dev(Wm), znp, _l(znns))
        else:
            npar = zn = None
            hargs = (None, None, None, None, _l(0))
        L.call("rfn_glow_shell_fwd_f32", zp, _l(zns), *targs, L.dev(ldp[k]), _i(ct), *hargs, _i(ldc), _i(N), _i(C), _i(H),
               _i(W))
        torch.cuda.synchronize()
        ok = untouched(zpar) and (npar is None or untouched(npar)) and all(untouched(p_) for p_ in keep[1:])
        if tk == "o":
            ok = ok and torch.equal(keep[1][:, 1:C + 1].cpu(), I.o)         # o_in is read only
        res[name] = Bag(z=z.cpu(), znext=None if zn is None else zn.cpu(), o=None if o_out is None else o_out.cpu(),
                        parents_ok=ok)
    logdet = I.init.cuda()
    L.call("rfn_logdet_reduce_f32", L.dev(ldp), _i(3), L.dev(logdet), _i(1), _i(N), _i(C), _i(H), _i(W))
    torch.cuda.synchronize()
    res["ld"], res["ldp"] = logdet.cpu(), ldp.cpu()
    return res


def same_bits(a, b):
    for k in a:
        if k in ("ld", "ldp"):
            if not torch.equal(a[k], b[k]):
                return False
        else:
            for f in ("z", "znext", "o"):
                if (a[k][f] is None) != (b[k][f] is None) or (a[k][f] is not None and not torch.equal(a[k][f], b[k][f])):
                    return False
    return True


@pytest.mark.parametrize("case", list(FWD_CASES), ids=ids)
def test_forward_vs_fp64(L, case):
    idx = list(FWD_CASES).index(case)
    N, C, H, W = case
    Ch = C // 2
    I = fwd_inputs(case, False, 100 + idx)
    label = fwd_label(L, N, C, H, W)
    runs = [("o", idx % 4, idx % 2)] + ([("P", (idx + 1) % 4, 1)] if case in P_TAIL else [])
    for tail, ct, ldc_th in runs:
        got = fwd_run(L, I, tail, ct, ldc_th)
        again = fwd_run(L, I, tail, ct, ldc_th)
        ld_ref, A = I.init.double(), torch.zeros(N, dtype=torch.float64)
        worst = 0.0
        fails = []
        for name, tk, head, ldc in fwd_modes(tail, ldc_th):
            ref, ld, a = fwd_ref(I, tk, head, ct, ldc)
            ld_ref, A = ld_ref + ld, A + a
            g = got[name]
            if not g.parents_ok:
                fails.append("%s: a launch wrote outside its channel slice (or into o_in)" % name)
            if tk is None:
                if not torch.equal(g.z, I.z):
                    fails.append("head only: z was modified")
            else:
                if not torch.equal(g.z[:, :Ch], I.z[:, :Ch]):
                    fails.append("%s: the pass-through half of z was modified" % name)
                e = relerr(g.z, ref["z"])
                worst = max(worst, e) if e == e else NAN
            if tk == "P":
                e = relerr(g.o, ref["o"])
                worst = max(worst, e) if e == e else NAN
            if head:
                e = relerr(g.znext, ref["znext"])
                worst = max(worst, e) if e == e else NAN
        e_ld = float(((got["ld"].double() - ld_ref).abs() / A).max())
        print("\nFWD %s tail=%s clamp=%s %s | elementwise %.2e  log-det/A %.2e" %
              (ids(case), tail, CLAMPS[ct], label, worst, e_ld))
        assert not fails, fails
        assert not torch.isnan(got["ldp"]).any(), "a log-det partial slot was left unwritten"
        assert worst < EW_BOUND, (tail, worst)
        assert e_ld <= LD_BOUND, (tail, e_ld)
        assert same_bits(got, again), "two forward runs differ"


@pytest.mark.parametrize("case", list(FWD_CASES), ids=ids)
def test_forward_logdet_and_gather_are_exact_on_dyadic_inputs(L, case):
    """clamp none, everything a multiple of 1/8: the reduced log-det equals the integer-computed value bit for bit (every
    frame has its own s values: a wrong block, slot or frame index moves a sum), and so does o_out from P"""
    idx = list(FWD_CASES).index(case)
    N, C, H, W = case
    HW = H * W
    I = fwd_inputs(case, True, 200 + idx)
    ct = 3
    logs8 = int((I.logs * 8).long().sum())
    for tail in ["o"] + (["P"] if case in P_TAIL else []):
        got = fwd_run(L, I, tail, ct, 1)
        if tail == "P":
            o64 = tapgather(I.P.double(), C) + I.b3.double().view(1, -1, 1, 1)            # exp(3 * 0) = 1
            for name in ("tail", "tail+head"):
                assert torch.equal(got[name].o, o64.float()) and torch.equal(got[name].o.double(), o64), name
            s8 = (o64[:, 1::2] * 8).long()
        else:
            s8 = (I.o[:, 1::2] * 8).long()
        want8 = (I.init * 8).long() + 2 * s8.sum((1, 2, 3)) + 2 * HW * logs8       # two tails, two ld_const heads
        want = (want8.double() / 8).float()
        assert torch.equal(want.double() * 8, want8.double())                      # representable: the test's own premise
        assert torch.equal(got["ld"], want), (tail, (got["ld"] - want).abs().max(), int((got["ld"] != want).sum()))


# ------------------------------------------------------------------------------------------------ backward
def pre(n):
    """nonzero prefill of an accumulated output"""
    return ((torch.arange(n) % 5).float() - 2.0) * 0.25 + 0.125


def bwd_inputs(case, seed):
    N, C, HW = case
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    o = r(N, C, HW)
    o[:, 0::2] *= 0.5
    return Bag(N=N, C=C, HW=HW, x=r(N, C, HW), gz=r(N, C, HW), o=o, gld=0.5 * r(N), bias=0.5 * r(C), logs=0.3 * r(C),
               Wm=r(C, C) / math.sqrt(C), scale=0.5 + torch.rand(C // 2, generator=g), shift=0.1 * r(C // 2),
               l3=0.1 * r(C), b3=0.1 * r(C))


def leaf(t):
    return t.detach().double().clone().requires_grad_()


def ref_bwd_ld(I, use_gld):
    x, bias, logs, Wm = leaf(I.x), leaf(I.bias), leaf(I.logs), leaf(I.Wm)
    zn = torch.einsum("ij,njp->nip", Wm, (x + bias.view(1, -1, 1)) * torch.exp(logs).view(1, -1, 1))
    loss = (zn * I.gz.double()).sum()
    if use_gld:
        loss = loss + (I.gld.double() * (I.HW * logs.sum())).sum()
    gx, gbias, glogs, gW = torch.autograd.grad(loss, (x, bias, logs, Wm))
    return Bag(gx=gx, gbias=gbias, glogs=glogs, gW=gW)


def ref_shell_bwd(I, ct, use_gld):
    """step k's coupling tail + step k+1's ActNorm/InvConv head in fp64, differentiated.  The kernel is handed step k's
    OUTPUT x and coupling-net output o: the leaves (u, z_prev) are the fp64 values that reproduce exactly those."""
    Ch, HW = I.C // 2, I.HW
    bias, logs, Wm, l3, b3 = leaf(I.bias), leaf(I.logs), leaf(I.Wm), leaf(I.l3), leaf(I.b3)
    scale, shift = leaf(I.scale), leaf(I.shift)
    u = leaf(I.o.double() * torch.exp(-3 * I.l3.double()).view(1, -1, 1) - I.b3.double().view(1, -1, 1))
    o = (u + b3.view(1, -1, 1)) * torch.exp(3 * l3).view(1, -1, 1)
    sh, s = o[:, 0::2], o[:, 1::2]
    ls = clamp64(s, ct, scale, shift)
    zp1 = leaf(I.x[:, :Ch])
    zp2 = leaf(I.x[:, Ch:].double() * torch.exp(-ls.detach()) - sh.detach())
    x = torch.cat([zp1, (zp2 + sh) * torch.exp(ls)], 1)
    assert float((x.detach() - I.x.double()).abs().max()) < 1e-12
    zn = torch.einsum("ij,njp->nip", Wm, (x + bias.view(1, -1, 1)) * torch.exp(logs).view(1, -1, 1))
    loss = (zn * I.gz.double()).sum()
    if use_gld:
        loss = loss + (I.gld.double() * (ls.sum((1, 2)) + HW * logs.sum())).sum()
    wrt = [zp1, zp2, u, b3, l3, Wm, bias, logs] + ([scale, shift] if ct == 0 else [])
    gr = torch.autograd.grad(loss, wrt)
    out = Bag(gz_prev=torch.cat([gr[0], gr[1]], 1), gpre=gr[2], gb3=gr[3], gl3=gr[4], gW=gr[5], gbias=gr[6], glogs=gr[7])
    if ct == 0:
        out.update(gscale=gr[8], gshift=gr[9])
    return out


@pytest.fixture(scope="module")
def bwd_case_inputs():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = bwd_inputs(case, 300 + list(BWD_CASES).index(case))
        return cache[case]
    return get


@pytest.mark.parametrize("use_gld", (True, False), ids=("glogdet", "noglogdet"))
@pytest.mark.parametrize("case", list(BWD_CASES), ids=ids)
def test_backward_vs_fp64(L, bwd_case_inputs, case, use_gld):
    idx = list(BWD_CASES).index(case)
    N, C, HW = case
    Ch = C // 2
    I = bwd_case_inputs(case)
    ct = (idx + (0 if use_gld else 2)) % 4
    dev = lambda t: t.cuda()
    bias, logs, Wm, l3 = dev(I.bias), dev(I.logs), dev(I.Wm), dev(I.l3)
    gld = dev(I.gld) if use_gld else None
    xpar, x = view_of(I.x)
    gzpar, gz = view_of(I.gz)
    xp, xns = L.frames(x, "x")
    gzp, gzns = L.frames(gz, "gz")
    fails, ew, red = [], {}, {}

    # ---- rfn_actnorm_invconv_bwd_ld_f32
    ref = ref_bwd_ld(I, use_gld)
    gxpar, gx = view_of((N, C, HW))
    gxp, gxns = L.frames(gx, "gx")
    acc = Bag(gW=dev(pre(C * C)), gbias=dev(pre(C)), glogs=dev(pre(C)))
    L.call("rfn_actnorm_invconv_bwd_ld_f32", xp, _l(xns), L.dev(bias), L.dev(logs), L.dev(Wm), gzp, _l(gzns), gxp,
           _l(gxns), L.dev(acc.gW), L.dev(acc.gbias), L.dev(acc.glogs), L.dev(gld), _i(N), _i(C), _i(HW))
    torch.cuda.synchronize()
    if not (untouched(gxpar) and untouched(xpar) and untouched(gzpar)):
        fails.append("bwd_ld wrote outside a channel slice")
    ew["ld.gx"] = relerr(gx, ref.gx)
    for k in ("gW", "gbias", "glogs"):
        red["ld." + k] = relerr(acc[k].cpu().double() - pre(acc[k].numel()).double(), ref[k].reshape(-1))

    # ---- rfn_glow_shell_bwd_f32
    ref = ref_shell_bwd(I, ct, use_gld)
    opar, o = view_of(I.o)
    gppar, gz_prev = view_of((N, C, HW))
    gupar, gpre = view_of((N, C, HW))
    op, ons = L.frames(o, "o")
    gpp, gpns = L.frames(gz_prev, "gz_prev")
    gup, guns = L.frames(gpre, "gpre")
    acc = Bag(gW=dev(pre(C * C)), gbias=dev(pre(C)), glogs=dev(pre(C)), gb3=dev(pre(C)), gl3=dev(pre(C)))
    scale = shift = None
    if ct == 0:
        scale, shift = dev(I.scale), dev(I.shift)
        acc.update(gscale=dev(pre(Ch)), gshift=dev(pre(Ch)))
    L.call("rfn_glow_shell_bwd_f32", xp, _l(xns), L.dev(bias), L.dev(logs), L.dev(Wm), gzp, _l(gzns), L.dev(acc.gW),
           L.dev(acc.gbias), L.dev(acc.glogs), op, _l(ons), L.dev(gld), L.dev(scale), L.dev(shift), L.dev(l3), gpp,
           _l(gpns), gup, _l(guns), L.dev(acc.get("gscale")), L.dev(acc.get("gshift")), L.dev(acc.gb3), L.dev(acc.gl3),
           _i(ct), _i(1), _i(N), _i(C), _i(HW))
    torch.cuda.synchronize()
    if not all(untouched(p_) for p_ in (xpar, gzpar, opar, gppar, gupar)):
        fails.append("shell_bwd wrote outside a channel slice")
    if not (torch.equal(x.cpu(), I.x) and torch.equal(gz.cpu(), I.gz) and torch.equal(o.cpu(), I.o)):
        fails.append("an input was modified")
    ew["sh.gz_prev"] = relerr(gz_prev, ref.gz_prev)
    ew["sh.gpre"] = relerr(gpre, ref.gpre)
    for k in acc:
        red["sh." + k] = relerr(acc[k].cpu().double() - pre(acc[k].numel()).double(), ref[k].reshape(-1))

    fmt = lambda d: " ".join("%s %.1e" % kv for kv in d.items())
    print("\nBWD %s clamp=%s %s\n    %s\n    elementwise: %s\n    reduced: %s" %
          (ids(case), CLAMPS[ct], "glogdet" if use_gld else "no glogdet", bwd_label(L, N, C, HW, 1), fmt(ew), fmt(red)))
    assert not fails, fails
    for k, v in ew.items():
        assert v < EW_BOUND, (k, v)
    for k, v in red.items():
        assert v < RED_BOUND, (k, v)
