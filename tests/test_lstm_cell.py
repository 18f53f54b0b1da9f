"""rfn_lstm_cell_{fwd,bwd}_f32 (csrc/lstm_cell.hip) and rfn_hip.ops.lstm_cell on the KERNEL route against the float64
restatement of tests/lstm_ref.py (written from the definition in include/rfn_hip.h, held against nn.LSTMCell in float64 by
tests/test_lstm_cell_host.py).

Shapes (B, I, H): a single element; all three below a tile; exactly one tile; one row short of a tile with a k range of one
MFMA; four k chunks per product (one per wave); one past a tile in B with odd I and H (single-float loads for x, 16-byte
loads for h); three row tiles with H one past a tile; the model's width.  Inputs x, h, c ~ N(0, 1); weights and biases at
1/sqrt(H) and at 0.02 (the model's initial scale); one case with pre-activations of magnitude about 30 (saturated gates).

Forward bound of an element of h', c' and the saved activations, the larger of
  - four times the error of the float32 torch ops on the GPU (nn.LSTMCell for h' and c', the same formulas as torch ops
    for the activations) against float64: one figure per tensor;
  - 2^-20 (1 + |c|) A, A the largest of the element's four sum|x w| + sum|h w| + |b_ih| + |b_hh|: eight units of float32
    round-off; the MFMA chain has one to two of sum|a b| at K <= 1024, a handful of few-ulp transcendental calls come on
    top.
Backward bound of an element of D, g_c and the bias gradient (both upstreams, and each alone), the analogous one scaled
with the tensor's maximum, the larger of
  - four times the error of float32 autograd through the same torch ops against float64, one figure per tensor;
  - 2^-20 (1 + |c|) A of the element times the tensor's maximum (an element of the bias gradient takes the largest
    (1 + |c|) A of its column).
g_x, g_h, g_w_ih, g_w_hh of the full Function: the larger of four times the float32 torch chain's own error and 2^-20 of
sum |terms| of the element.

Bit for bit: two launches repeat; every row of the (33, 3, 17) and (17, 33, 40) launches equals the B = 1 launch on that
row (h', c', activations, D, g_c); a captured and replayed forward + backward equals the eager one.

The worst error / bound per case is printed; DESIGN.md section 22 holds the figures measured on an MI355X."""
import pytest
import torch

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (3, 5, 7), (4, 16, 16), (15, 4, 16), (16, 64, 64), (17, 33, 40), (33, 3, 17), (5, 256, 256)]
SCALES = ["rsqrt", "init"]
CASES = [(s, w) for s in SHAPES for w in SCALES] + [((4, 16, 16), "saturated")]
EPS20 = 2.0 ** -20
FWD = ("h_out", "c_out", "gates")
PW = ("D", "g_c", "g_bias")
MM = ("g_x", "g_h", "g_w_ih", "g_w_hh")
UPS = ("both", "gh", "gc")


def w_scale(shape, kind):
    B, I, H = shape
    return {"rsqrt": H ** -0.5, "init": 0.02, "saturated": 30.0 * (I + H) ** -0.5}[kind]


def torch_chain(v):
    """the cell as float32 / float64 torch ops with the pre-activations as a node: {h_out, c_out, gates, pre}"""
    H = v["h"].shape[1]
    pre = torch.addmm(v["b_ih"] + v["b_hh"], v["x"], v["w_ih"].t()) + torch.mm(v["h"], v["w_hh"].t())
    i, f, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
    g = torch.tanh(pre[:, 2 * H:3 * H])
    c_out = f * v["c"] + i * g
    return {"h_out": o * torch.tanh(c_out), "c_out": c_out, "gates": torch.cat([i, f, g, o], 1), "pre": pre}


def upstreams(shape):
    B, I, H = shape
    g = torch.Generator().manual_seed(99 + B + 7 * H)
    gh, gc = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    return {"both": (gh, gc), "gh": (gh, None), "gc": (None, gc)}


def chain32_grads(vd, gh, gc):
    """float32 autograd on the GPU through torch_chain: D (the gradient at the pre-activations), g_c, the bias gradient
    and the four matrix products"""
    leaves = {n: t.clone().requires_grad_(True) for n, t in vd.items()}
    out = torch_chain(leaves)
    total = sum((out[n] * u.to(DEV)).sum() for n, u in (("h_out", gh), ("c_out", gc)) if u is not None)
    names = ("pre", "c", "b_ih", "x", "h", "w_ih", "w_hh")
    gs = torch.autograd.grad(total, [out["pre"]] + [leaves[n] for n in names[1:]])
    return dict(zip(PW + MM, [g.detach().cpu().double() for g in gs]))


@pytest.fixture(scope="module")
def cases():
    """per case, computed once and left unchanged: inputs, the float64 forward and backward, the float32 torch errors"""
    cache = {}

    def get(shape, kind):
        key = (shape, kind)
        if key not in cache:
            assert torch.cuda.is_available(), "GPU tests need a device"
            B, I, H = shape
            v = R.make_inputs(B, I, H, w_scale(shape, kind), seed=SCALES.index(kind) if kind in SCALES else 2)
            vd = {n: t.to(DEV) for n, t in v.items()}
            fw = R.forward64(*[v[n] for n in R.NAMES])
            m = torch.nn.LSTMCell(I, H).to(DEV)
            with torch.no_grad():
                for n, k in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
                    getattr(m, n).copy_(vd[k])
                h32, c32 = m(vd["x"], (vd["h"], vd["c"]))
                g32 = torch_chain(vd)["gates"]
            err32 = {n: float((t.cpu().double() - fw[n]).abs().max())
                     for n, t in (("h_out", h32), ("c_out", c32), ("gates", g32))}
            amp = (1 + v["c"].double().abs()) * fw["A"]
            ups, bw, berr = upstreams(shape), {}, {}
            for u, (gh, gc) in ups.items():
                bw[u] = R.backward64(fw, gh, gc, v["x"], v["h"], v["c"], v["w_ih"], v["w_hh"])
                g32s = chain32_grads(vd, gh, gc)
                berr[u] = {n: float((g32s[n] - bw[u][n]).abs().max()) for n in PW + MM}
            cache[key] = {"v": v, "vd": vd, "fw": fw, "err32": err32, "amp": amp,
                          "ups": ups, "bw": bw, "berr": berr}
        return cache[key]
    return get


def fwd_entry(vd):
    from rfn_hip import lib as L
    B, I, H = vd["x"].shape[0], vd["x"].shape[1], vd["h"].shape[1]
    h_out, c_out = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV)
    gates = torch.empty(B, 4 * H, device=DEV)
    L.call("rfn_lstm_cell_fwd_f32", *[L.dev(vd[n]) for n in R.NAMES], L.dev(h_out), L.dev(c_out), L.dev(gates), B, I, H)
    return {"h_out": h_out, "c_out": c_out, "gates": gates}


def bwd_entry(gh, gc, gates, c, c_out):
    from rfn_hip import lib as L
    B, H = c.shape
    D, g_c, g_bias = torch.empty(B, 4 * H, device=DEV), torch.empty(B, H, device=DEV), torch.empty(4 * H, device=DEV)
    L.call("rfn_lstm_cell_bwd_f32", L.dev(gh), L.dev(gc), L.dev(gates), L.dev(c), L.dev(c_out), L.dev(D), L.dev(g_c),
           L.dev(g_bias), B, H)
    return {"D": D, "g_c": g_c, "g_bias": g_bias}


def pointwise_bound(c, ref, n, err32):
    """bound of D, g_c or the bias gradient: the larger of 4 x the float32 torch chain's error and the forward's term
    2^-20 (1 + |c|) A of the element times the tensor's maximum; an element of the bias gradient takes the largest
    (1 + |c|) A of its column"""
    amp = {"D": c["amp"].repeat(1, 4), "g_c": c["amp"], "g_bias": c["amp"].max(0).values.repeat(4)}[n]
    return torch.clamp(EPS20 * amp * ref[n].abs().max(), min=4 * err32)


def ratio_of(err, bound):
    return float((err / bound.clamp(min=1e-300)).max()) if float(err.max()) > 0 else 0.0


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape,kind", CASES)
def test_forward(cases, shape, kind):
    from rfn_hip import ops
    c = cases(shape, kind)
    B, I, H = shape
    got = fwd_entry(c["vd"])
    with torch.no_grad():
        h_out, c_out = ops.lstm_cell(*[c["vd"][n] for n in R.NAMES], route="kernel")
    assert torch.equal(h_out, got["h_out"]) and torch.equal(c_out, got["c_out"])
    worst = {}
    for n in FWD:
        ref = c["fw"][n]
        amp = c["amp"].repeat(1, 4) if n == "gates" else c["amp"]
        bound = torch.clamp(EPS20 * amp, min=4 * c["err32"][n])
        err = (got[n].cpu().double() - ref).abs()
        worst[n] = ratio_of(err, bound)
        print("forward %s %s %s: worst error %.3e, error / bound %.3f (float32 torch error %.1e)"
              % (shape, kind, n, float(err.max()), worst[n], c["err32"][n]))
    for n in FWD:
        assert worst[n] <= 1.0, (n, worst[n])
    if kind == "saturated":   # the case does reach saturation: some activation is within 1e-6 of its limit
        g = c["fw"]["gates"]
        assert float(g.abs().max()) > 1 - 1e-6 and float(g[:, :H].min()) < 1e-6


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("shape,kind", CASES)
def test_backward_kernel(cases, shape, kind):
    """D, g_c and the bias gradient of the entry point, fed the float32 forward of the kernel"""
    c = cases(shape, kind)
    fw = fwd_entry(c["vd"])
    for u in UPS:
        gh, gc = [None if t is None else t.to(DEV) for t in c["ups"][u]]
        got = bwd_entry(gh, gc, fw["gates"], c["vd"]["c"], fw["c_out"])
        ref = c["bw"][u]
        for n in PW:
            bound = pointwise_bound(c, ref, n, c["berr"][u][n])
            err = (got[n].cpu().double() - ref[n]).abs()
            r = ratio_of(err, bound)
            print("backward %s %s %s %s: worst error %.3e, error / bound %.3f (float32 torch error %.1e)"
                  % (shape, kind, u, n, float(err.max()), r, c["berr"][u][n]))
            assert r <= 1.0, (u, n, r)
    # a missing upstream is a zero one
    zero = torch.zeros_like(fw["c_out"])
    gh = c["ups"]["gh"][0].to(DEV)
    a, b = bwd_entry(gh, None, fw["gates"], c["vd"]["c"], fw["c_out"]), bwd_entry(gh, zero, fw["gates"], c["vd"]["c"],
                                                                                  fw["c_out"])
    for n in PW:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("shape,kind", CASES)
def test_function_gradients(cases, shape, kind):
    from rfn_hip import ops
    c = cases(shape, kind)
    for u in UPS:
        gh, gc = c["ups"][u]
        leaves = [c["vd"][n].clone().requires_grad_(True) for n in R.NAMES]
        h_out, c_out = ops.lstm_cell(*leaves, route="kernel")
        total = sum((o * g.to(DEV)).sum() for o, g in ((h_out, gh), (c_out, gc)) if g is not None)
        gs = dict(zip(("g_x", "g_h", "g_c", "g_w_ih", "g_w_hh", "g_bias", "g_b_hh"), torch.autograd.grad(total, leaves)))
        assert torch.equal(gs["g_bias"], gs["g_b_hh"])
        ref = c["bw"][u]
        for n in MM + ("g_c", "g_bias"):
            if n in MM:
                bound = torch.clamp(EPS20 * ref["abs_" + n], min=4 * c["berr"][u][n])
            else:
                bound = pointwise_bound(c, ref, n, c["berr"][u][n])
            err = (gs[n].cpu().double() - ref[n]).abs()
            r = ratio_of(err, bound)
            print("function %s %s %s %s: worst error %.3e, error / bound %.3f (float32 torch error %.1e)"
                  % (shape, kind, u, n, float(err.max()), r, c["berr"][u][n]))
            assert r <= 1.0, (u, n, r)


def test_route_follows_the_environment(cases, monkeypatch):
    from rfn_hip import ops
    c = cases((3, 5, 7), "rsqrt")
    args = [c["vd"][n] for n in R.NAMES]
    monkeypatch.setenv("RFN_LSTM_CELL", "1")
    assert ops.lstm_cell_route(args[0]) == "kernel"
    with torch.no_grad():
        k = ops.lstm_cell(*args)
    monkeypatch.setenv("RFN_LSTM_CELL", "0")
    assert ops.lstm_cell_route(args[0]) == "torch"
    with torch.no_grad():
        t = ops.lstm_cell(*args)
    monkeypatch.delenv("RFN_LSTM_CELL")
    assert ops.lstm_cell_route(args[0]) == ("kernel" if ops.LSTM_CELL_KERNEL_DEFAULT else "torch")
    assert torch.equal(k[0], fwd_entry(c["vd"])["h_out"])
    assert float((k[0] - t[0]).abs().max()) <= 1e-5 and float((k[1] - t[1]).abs().max()) <= 1e-5
    assert ops.lstm_cell_route(args[0].double()) == "torch"


# ------------------------------------------------------------------------------------------------ entry points
def test_entry_points_refuse_what_they_cannot_compute(cases):
    from rfn_hip import lib as L
    c = cases((3, 5, 7), "rsqrt")
    d = [L.dev(c["vd"][n]) for n in R.NAMES]
    outs = [torch.full(s, 7.0, device=DEV) for s in ((3, 7), (3, 7), (3, 28), (3, 28), (28,))]
    h_out, c_out, gates, D, g_bias = [L.dev(t) for t in outs]
    load = L.load()
    cur = torch.cuda.current_stream().cuda_stream

    def fwd(ins=d, o=(h_out, c_out, gates), B=3, I=5, H=7):
        return load.rfn_lstm_cell_fwd_f32(*ins, *o, B, I, H, cur)
    assert fwd(B=0) == -1 and fwd(I=0) == -1 and fwd(H=-2) == -1
    assert b"argument check failed" in load.rfn_last_error()
    for k in range(7):
        assert fwd(ins=d[:k] + [None] + d[k + 1:]) == -2, R.NAMES[k]
    assert fwd(o=(None, c_out, gates)) == -2 and fwd(o=(h_out, None, gates)) == -2 and fwd(o=(h_out, c_out, None)) == -2

    def bwd(gh=h_out, gc=c_out, g=gates, c_=d[2], co=c_out, D_=D, g_c=h_out, gb=g_bias, B=3, H=7):
        return load.rfn_lstm_cell_bwd_f32(gh, gc, g, c_, co, D_, g_c, gb, B, H, cur)
    assert bwd(B=0) == -1 and bwd(H=0) == -1
    for kw in ("g", "c_", "co", "D_", "g_c", "gb"):
        assert bwd(**{kw: None}) == -2, kw
    torch.cuda.synchronize()
    for t in outs:
        assert float(t.min()) == 7.0 and float(t.max()) == 7.0          # nothing was launched


# ------------------------------------------------------------------------------------------------ bit for bit
def test_two_launches_repeat_and_a_row_does_not_depend_on_the_batch(cases):
    for shape in ((33, 3, 17), (17, 33, 40)):
        c = cases(shape, "rsqrt")
        vd = c["vd"]
        gh, gc = [t.to(DEV) for t in c["ups"]["both"]]
        a, b = fwd_entry(vd), fwd_entry(vd)
        ga, gb = [bwd_entry(gh, gc, a["gates"], vd["c"], a["c_out"]) for _ in range(2)]
        for n in FWD:
            assert torch.equal(a[n], b[n]), n
        for n in PW:
            assert torch.equal(ga[n], gb[n]), n
        for r in range(shape[0]):
            row = dict(vd)
            for n in ("x", "h", "c"):
                row[n] = vd[n][r:r + 1].clone()     # (a fresh allocation: 16-byte aligned like the batch's)
            one = fwd_entry(row)
            for n in FWD:
                assert torch.equal(one[n][0], a[n][r]), (n, r)
            g1 = bwd_entry(gh[r:r + 1].clone(), gc[r:r + 1].clone(), one["gates"], row["c"], one["c_out"])
            for n in ("D", "g_c"):
                assert torch.equal(g1[n][0], ga[n][r]), (n, r)


def test_a_captured_forward_and_backward_equals_the_eager_one(cases):
    c = cases((17, 33, 40), "rsqrt")
    vd = c["vd"]
    gh, gc = [t.to(DEV) for t in c["ups"]["both"]]
    eager = fwd_entry(vd)
    eager_g = bwd_entry(gh, gc, eager["gates"], vd["c"], eager["c_out"])
    ins = {n: torch.zeros_like(t) for n, t in vd.items()}

    def body():
        fw = fwd_entry(ins)
        return fw, bwd_entry(gh, gc, fw["gates"], ins["c"], fw["c_out"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                           # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fw, bw = body()
    for n in R.NAMES:
        ins[n].copy_(vd[n])
    graph.replay()
    torch.cuda.synchronize()
    for n in FWD:
        assert torch.equal(fw[n], eager[n]), n
    for n in PW:
        assert torch.equal(bw[n], eager_g[n]), n
