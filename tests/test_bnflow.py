"""rfn_bnflow_{fwd,bwd,apply}_f32 called directly (lib.call, ctypes arguments) against the float64 restatement of the
contract in tests/test_bnflow_host.py (bnflow_ref, bnflow_bwd_ref, running_ref, apply_ref; the backward formulas are
checked against autograd there).

Rows (S, B, C, H, W): E = C*H*W smaller than a wave; E = 90 (no multiple of 4, the 4-byte route) with an odd B; two
column blocks of the 16-byte route; level 0 of the canonical flow (E = 4096); B above half a wave; and the third row
again with x one float past a 16-byte boundary (the 4-byte route on an E that is a multiple of 4).  Momenta 0.0
("running = the last step") and 0.3.

Inputs: x = offset[e] + N(0, 1) with a per-element offset, every (step, row) with its own values, so a wrong step, row or
element index moves a result; gdl is non-zero; log_gamma has a non-zero mean, so the log-det is a sum that does not cancel.
Every output is a NaN-filled buffer, the scratch is NaN-filled with a sentinel tail, every launch runs twice and must
repeat bit for bit (no atomics).

Bounds: those the per-step BatchNorm2d kernels are held to (tests/test_recurrent_shell.py), max|d| / max|ref|:
  z, gx, the given-statistics map both ways      EW_BOUND   1e-5
  mean, var, dl, running mean / var              STAT_BOUND 1e-5
  g_log_gamma, g_beta                            RED_BOUND  1e-4
"""
import ctypes

import pytest
import torch

from tests.test_bnflow_host import EPS, apply_ref, bnflow_bwd_ref, bnflow_ref, running_ref
from tests.test_recurrent_shell import EW_BOUND, RED_BOUND, STAT_BOUND, NAN, SENT, nan_buf, put, relerr

pytestmark = pytest.mark.gpu

_i, _f = ctypes.c_int, ctypes.c_float
ROWS = [(1, 3, 4, 2, 2, 0), (3, 5, 6, 3, 5, 0), (2, 4, 12, 16, 16, 0), (4, 3, 4, 32, 32, 0), (1, 33, 8, 4, 4, 0),
        (2, 4, 12, 16, 16, 1)]          # (S, B, C, H, W, floats x starts past a 16-byte boundary)
MOMENTA = (0.0, 0.3)
row_id = lambda r: "x".join(map(str, r[:5])) + ("-xoff" if r[5] else "")


@pytest.fixture(scope="module")
def L():
    from rfn_hip import lib
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return lib


@pytest.fixture(scope="module")
def cases():
    """per row: CPU inputs (float32) and the float64 reference, computed once and left unchanged"""
    cache = {}

    def get(row):
        if row not in cache:
            S, B, C, H, W, _ = row
            E = C * H * W
            g = torch.Generator().manual_seed(1000 + S * 7 + B * 13 + E)
            I = {"S": S, "B": B, "E": E}
            I["x"] = torch.randn(E, generator=g) + torch.randn(S * B, E, generator=g)
            I["lg"] = 0.3 * torch.randn(E, generator=g) + 0.1
            I["beta"] = torch.randn(E, generator=g)
            I["gz"] = torch.randn(S * B, E, generator=g)
            I["gdl"] = torch.randn(S, generator=g) + 0.5
            I["rm"] = torch.randn(E, generator=g)
            I["rv"] = torch.rand(E, generator=g) + 0.5
            d = {k: v.double() for k, v in I.items() if torch.is_tensor(v)}
            R = {}
            R["z"], R["mean"], R["var"], R["dl"] = bnflow_ref(d["x"], d["lg"], d["beta"], S)
            R["gx"], R["glg"], R["gbeta"] = bnflow_bwd_ref(d["x"], d["lg"], S, d["gz"], d["gdl"])
            for m in MOMENTA:
                R["rm", m] = running_ref(d["rm"], R["mean"], m)
                R["rv", m] = running_ref(d["rv"], R["var"], m)
            R["y_fwd"], R["dl_fwd"] = apply_ref(d["x"], d["lg"], d["beta"], d["rm"], d["rv"], False)
            R["y_rev"], R["dl_rev"] = apply_ref(d["x"], d["lg"], d["beta"], d["rm"], d["rv"], True)
            cache[row] = (I, R)
        return cache[row]
    return get


def scratch(L, S, B, E, bwd):
    """NaN-filled scratch of exactly what the query asks for that direction + a sentinel tail -> (whole, n)"""
    n = int(L.load().rfn_bnflow_scratch_floats(S, B, E, bwd))
    buf = torch.full((n + 8,), NAN, device="cuda", dtype=torch.float32)
    buf[n:] = SENT
    return buf, n


def tail_ok(buf, n):
    return bool((buf[n:] == SENT).all())


def train_launch(L, I, off, m):
    """forward (with the running statistics when m is not None) + backward into NaN-filled outputs"""
    from rfn_hip.ops import bnflow_coef
    S, B, E = I["S"], I["B"], I["E"]
    x, gz = put(I["x"], off), put(I["gz"])
    lg, beta, gdl = I["lg"].cuda(), I["beta"].cuda(), I["gdl"].cuda()
    o = {k: nan_buf(s) for k, s in (("z", (S * B, E)), ("mean", (S, E)), ("var", (S, E)), ("dl", (S,)),
                                    ("gx", (S * B, E)), ("glg", (E,)), ("gbeta", (E,)))}
    rm = rv = cf = None
    decay = 1.0
    if m is not None:
        rm, rv = I["rm"].cuda(), I["rv"].cuda()
        cf, decay = bnflow_coef(S, m)
        cf = cf.float().cuda()
    s1, n1 = scratch(L, S, B, E, 0)
    L.call("rfn_bnflow_fwd_f32", L.dev(x), L.dev(lg), L.dev(beta), L.dev(o["z"]), L.dev(o["mean"]), L.dev(o["var"]),
           L.dev(o["dl"]), L.dev(s1), L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cf), _f(decay), _i(S), _i(B), _i(E), _f(EPS))
    s2, n2 = scratch(L, S, B, E, 1)
    L.call("rfn_bnflow_bwd_f32", L.dev(x), L.dev(lg), L.dev(gz), L.dev(gdl), L.dev(o["mean"]), L.dev(o["var"]),
           L.dev(o["gx"]), L.dev(o["glg"]), L.dev(o["gbeta"]), L.dev(s2), _i(S), _i(B), _i(E))
    torch.cuda.synchronize()
    o.update(rm=rm, rv=rv, scratch_ok=tail_ok(s1, n1) and tail_ok(s2, n2), x_aligned=x.data_ptr() % 16 == 0)
    return o


OUTS = ("z", "mean", "var", "dl", "gx", "glg", "gbeta", "rm", "rv")


@pytest.mark.parametrize("m", MOMENTA)
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_training_kernels_vs_fp64(L, cases, row, m):
    I, R = cases(row)
    got = train_launch(L, I, row[5], m)
    again = train_launch(L, I, row[5], m)
    e = {k: relerr(got[k], R[k]) for k in OUTS[:7]}
    e["rm"], e["rv"] = relerr(got["rm"], R["rm", m]), relerr(got["rv"], R["rv", m])
    print("\nbnflow %s m=%.1f | %s" % (row_id(row), m, " ".join("%s %.1e" % kv for kv in e.items())))
    assert got["x_aligned"] == (row[5] == 0)
    assert got["scratch_ok"], "the scratch was overrun"
    assert e["z"] < EW_BOUND and e["gx"] < EW_BOUND, e
    assert all(e[k] < STAT_BOUND for k in ("mean", "var", "dl", "rm", "rv")), e
    assert e["glg"] < RED_BOUND and e["gbeta"] < RED_BOUND, e
    for k in OUTS:
        assert torch.equal(got[k], again[k]), "two launches differ in " + k
    if m == 0.0:   # "running = the last step's statistics", bit for bit
        S = I["S"]
        assert torch.equal(got["rm"], got["mean"][S - 1]) and torch.equal(got["rv"], got["var"][S - 1])
    # without running statistics the same launches write the same outputs
    plain = train_launch(L, I, row[5], None)
    for k in OUTS[:7]:
        assert torch.equal(plain[k], got[k]), k


def apply_launch(L, I, x, reverse):
    N, E = x.shape
    y, dl = nan_buf((N, E)), nan_buf((1,))
    lg, beta, rm, rv = (I[k].cuda() for k in ("lg", "beta", "rm", "rv"))    # (held until the launch has run)
    L.call("rfn_bnflow_apply_f32", L.dev(x), L.dev(lg), L.dev(beta), L.dev(rm), L.dev(rv), L.dev(y), L.dev(dl), _i(N),
           _i(E), _i(1 if reverse else 0))
    torch.cuda.synchronize()
    return y, dl


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_given_statistics_map_vs_fp64_and_round_trip(L, cases, row):
    I, R = cases(row)
    x = put(I["x"], row[5])
    y, dl = apply_launch(L, I, x, False)
    y2, dl2 = apply_launch(L, I, x, False)
    xr, dlr = apply_launch(L, I, x, True)            # the reverse map on the same input, against its own reference
    back, dlb = apply_launch(L, I, y, True)          # forward then reverse
    e = dict(y=relerr(y, R["y_fwd"]), dl=relerr(dl, R["dl_fwd"].view(1)), rev=relerr(xr, R["y_rev"]),
             dl_rev=relerr(dlr, R["dl_rev"].view(1)), back=relerr(back, I["x"].double()))
    print("\nbnflow apply %s | %s" % (row_id(row), " ".join("%s %.1e" % kv for kv in e.items())))
    assert e["y"] < EW_BOUND and e["rev"] < EW_BOUND and e["back"] < EW_BOUND, e
    assert e["dl"] < STAT_BOUND and e["dl_rev"] < STAT_BOUND, e
    assert torch.equal(y, y2) and torch.equal(dl, dl2), "two launches differ"
    assert float(dl + dlb) == 0.0 and torch.equal(dlr, dlb)      # the two log-dets cancel exactly


def test_ops_node_equals_direct_launches(L, cases):
    """rfn_hip.ops.BatchNormFlowFn / bnflow_apply on [S*B, C, H, W] tensors: the same bits as the direct launches"""
    from rfn_hip import ops as K
    row = ROWS[1]
    S, B, C, H, W, _ = row
    I, R = cases(row)
    direct = train_launch(L, I, 0, 0.3)
    x = I["x"].view(S * B, C, H, W).cuda().requires_grad_(True)
    lg = I["lg"].view(1, C, H, W).cuda().requires_grad_(True)
    beta = I["beta"].view(1, C, H, W).cuda().requires_grad_(True)
    rm, rv = I["rm"].view(1, C, H, W).cuda(), I["rv"].view(1, C, H, W).cuda()
    cf, decay = K.bnflow_coef(S, 0.3)
    z, dl = K.BatchNormFlowFn.apply(x, lg, beta, S, EPS, (rm, rv, cf.float().cuda(), decay))
    ((z * I["gz"].view_as(z).cuda()).sum() + (dl * I["gdl"].cuda()).sum()).backward()
    for k, t in (("z", z), ("dl", dl), ("gx", x.grad), ("glg", lg.grad), ("gbeta", beta.grad), ("rm", rm), ("rv", rv)):
        assert torch.equal(t.detach().reshape(-1), direct[k].reshape(-1)), k
    y, d = K.bnflow_apply(x.detach(), lg, beta, rm, rv, False)
    xb, db = K.bnflow_apply(y, lg, beta, rm, rv, True)
    assert relerr(xb.view(S * B, -1), I["x"].double()) < EW_BOUND and float(d + db) == 0.0
