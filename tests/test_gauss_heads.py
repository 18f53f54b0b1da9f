"""rfn_gauss_heads_{fwd,bwd}_f32 (csrc/gauss_heads.hip) and rfn_hip.ops.gauss_heads against a float64 restatement of the
DEFINITION in include/rfn_hip.h (written from that paragraph, not from the kernel), td.Normal / td.kl_divergence in
float64 included.

Shapes (B, Z): a single element, the default Z = 20 as a partial wave, exactly one wave, one element into the second
sweep of the lanes, and B no multiple of the four rows of a workgroup.  Inputs: loc ~ N(0,1), raw ~ U(-8, 8) with column
0 pinned at 25.0 (above softplus's threshold of 20) and, where Z > 1, column 1 at exactly 20.0 (the threshold itself,
which takes the log1p branch), eps ~ N(0,1).

Bound of an output: the larger of
  - four times the error of the SAME chain written as float32 torch ops (nn.Softplus, td.Normal(...).log_prob of the
    sample, td.kl_divergence, float32 autograd for the gradients) against float64: one figure per output tensor, its
    largest absolute error;
  - 2^-20 of the scale: |ref| of the element for elementwise outputs, sum_j |term_j| of the row for row sums, the
    tensor's maximum for gradients.  2^-20 is 16 units of float32 round-off: a handful of few-ulp transcendental calls
    (exp, log1p, log, a division) plus the ceil(Z/64) + 6 additions of the fixed-order sum.
torch.autograd.gradcheck is not the yardstick: the inputs are float32.

Measured on an MI355X, the largest error / bound of each test over its shapes, is printed per case; DESIGN.md section 21
holds the figures.

Bit for bit: two launches repeat; row b of a B = 5 launch equals the B = 1 launch on that row; a captured-and-replayed
launch equals the eager one; a request for fewer outputs gives the bits of the full request."""
import math

import pytest
import torch
import torch.distributions as td

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (4, 4), (3, 20), (5, 64), (2, 65), (7, 130)]
INS = ("q_loc", "q_raw", "p_loc", "p_raw", "eps_q", "eps_p")
OUTS = ("z_q", "z_p", "q_scale", "p_scale", "kl", "logq", "logp")
ROWS = ("kl", "logq", "logp")
UPS = ("z_q", "z_p", "kl", "logq", "logp")     # the outputs that carry an upstream gradient
EPS20 = 2.0 ** -20


def make_inputs(B, Z):
    g = torch.Generator().manual_seed(1000 * B + Z)
    x = {}
    for n in INS:
        if n.endswith("raw"):
            t = torch.rand(B, Z, generator=g) * 16.0 - 8.0
            t[:, 0] = 25.0
            if Z > 1:
                t[:, 1] = 20.0
        else:
            t = torch.randn(B, Z, generator=g)
        x[n] = t
    return x


def softplus_def(raw):
    """raw itself where raw > 20, otherwise log1p(exp(raw))"""
    return torch.where(raw > 20, raw, torch.log1p(torch.exp(torch.clamp(raw, max=20))))


def restate64(x):
    """(outputs, per-row scales of the row sums) in float64 from the header's formulas; differentiable in the inputs"""
    sq, sp = softplus_def(x["q_raw"]), softplus_def(x["p_raw"])
    a, d = sq / sp, (x["q_loc"] - x["p_loc"]) / sp
    t_kl = 0.5 * (a * a + d * d - 1) - (torch.log(sq) - torch.log(sp))
    t_lq = -0.5 * x["eps_q"] ** 2 - torch.log(sq) - 0.5 * math.log(2 * math.pi)
    t_lp = -0.5 * x["eps_p"] ** 2 - torch.log(sp) - 0.5 * math.log(2 * math.pi)
    out = {"z_q": x["q_loc"] + sq * x["eps_q"], "z_p": x["p_loc"] + sp * x["eps_p"], "q_scale": sq, "p_scale": sp,
           "kl": t_kl.sum(-1), "logq": t_lq.sum(-1), "logp": t_lp.sum(-1)}
    scale = {"kl": t_kl.abs().sum(-1), "logq": t_lq.abs().sum(-1), "logp": t_lp.abs().sum(-1)}
    return out, scale


def torch_chain(x):
    """the same step as the torch ops the kernel replaces (VRNN.py of the reference), in the dtype of x"""
    sq, sp = torch.nn.Softplus()(x["q_raw"]), torch.nn.Softplus()(x["p_raw"])
    qd, pd = td.Normal(x["q_loc"], sq), td.Normal(x["p_loc"], sp)
    z_q, z_p = x["q_loc"] + sq * x["eps_q"], x["p_loc"] + sp * x["eps_p"]
    return {"z_q": z_q, "z_p": z_p, "q_scale": sq, "p_scale": sp, "kl": td.kl_divergence(qd, pd).sum(-1),
            "logq": qd.log_prob(z_q).sum(-1), "logp": pd.log_prob(z_p).sum(-1)}


def upstreams(B, Z):
    g = torch.Generator().manual_seed(77 + 1000 * B + Z)
    return {n: torch.randn((B,) if n in ROWS else (B, Z), generator=g) for n in UPS}


def grads_of(fn, x, ups, dtype):
    """d sum_n <ups[n], out[n]> / d (q_loc, q_raw, p_loc, p_raw) of the chain `fn` in `dtype`"""
    leaves = {n: t.to(dtype).clone().requires_grad_(n in INS[:4]) for n, t in x.items()}
    out = fn(leaves)
    out = out[0] if isinstance(out, tuple) else out
    total = sum((out[n] * u.to(dtype)).sum() for n, u in ups.items())
    gs = torch.autograd.grad(total, [leaves[n] for n in INS[:4]], allow_unused=True)
    return {n: (torch.zeros_like(leaves[n]) if g is None else g).detach() for n, g in zip(INS[:4], gs)}


@pytest.fixture(scope="module")
def cases():
    """per shape, computed once and left unchanged: inputs, float64 outputs, scales, float32-chain errors, device inputs"""
    cache = {}

    def get(shape):
        if shape not in cache:
            assert torch.cuda.is_available(), "GPU tests need a device"
            B, Z = shape
            x = make_inputs(B, Z)
            x64 = {n: t.double() for n, t in x.items()}
            ref, scale = restate64(x64)
            lib64 = torch_chain(x64)   # td.Normal / kl_divergence in float64 say the same as the paragraph
            for n in OUTS:
                assert float((lib64[n] - ref[n]).abs().max()) <= 1e-12 * max(1.0, float(ref[n].abs().max())), n
            c32 = torch_chain(x)
            err32 = {n: float((c32[n].double() - ref[n]).abs().max()) for n in OUTS}
            cache[shape] = {"x": x, "ref": ref, "scale": scale, "err32": err32, "xd": {n: t.to(DEV) for n, t in x.items()}}
        return cache[shape]
    return get


def bound_of(c, name):
    scale = c["scale"][name] if name in ROWS else c["ref"][name].abs()
    return torch.clamp(EPS20 * scale, min=4 * c["err32"][name])


def check_outputs(c, got, tag):
    worst = 0.0
    for n, t in got.items():
        ref = c["ref"][n]
        assert t.shape == ref.shape and t.dtype == torch.float32, n
        err, bound = (t.detach().cpu().double() - ref).abs(), bound_of(c, n)
        ratio = float((err / bound.clamp(min=1e-300)).max()) if float(err.max()) > 0 else 0.0
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), "%s %s: error / bound %.3f" % (tag, n, ratio)
    return worst


def run(c, want, q=True):
    from rfn_hip import ops
    d = c["xd"]
    with torch.no_grad():
        if q:
            got = ops.gauss_heads(d["q_loc"], d["q_raw"], d["p_loc"], d["p_raw"], d["eps_q"], d["eps_p"], want=want)
        else:
            got = ops.gauss_heads(None, None, d["p_loc"], d["p_raw"], None, d["eps_p"], want=want)
    return dict(zip(want, got))


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_all_outputs(cases, shape):
    c = cases(shape)
    got = run(c, OUTS)
    worst = check_outputs(c, got, "all")
    print("forward %s: worst error / bound %.3f (float32 torch chain errors %s)" %
          (shape, worst, {n: "%.1e" % v for n, v in c["err32"].items()}))
    # above the threshold sigma is the raw input itself; at the threshold it is log1p(exp(20)) = 20 + 2.1e-9, which is
    # above 20 in float64 and rounds to 20 in float32 (the bound above has checked the value)
    assert torch.equal(got["q_scale"][:, 0].cpu(), c["x"]["q_raw"][:, 0])
    if shape[1] > 1:
        assert bool((c["ref"]["p_scale"][:, 1] > 20.0).all()) and bool((c["x"]["p_raw"][:, 1] == 20.0).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_prior_only_and_single_output_requests(cases, shape):
    c = cases(shape)
    full = run(c, OUTS)
    prior = run(c, ("z_p", "p_scale", "logp"), q=False)
    worst = check_outputs(c, prior, "prior-only")
    for n, t in prior.items():
        assert torch.equal(t, full[n]), n
    for n in OUTS:
        one = run(c, (n,))
        worst = max(worst, check_outputs(c, one, "single"))
        assert torch.equal(one[n], full[n]), n
    print("prior-only and single outputs %s: worst error / bound %.3f" % (shape, worst))


# ------------------------------------------------------------------------------------------------ backward
def kernel_grads(c, ups):
    from rfn_hip import ops
    d = c["xd"]
    leaves = {n: d[n].clone().requires_grad_(n in INS[:4]) for n in INS}
    out = dict(zip(OUTS, ops.gauss_heads(*[leaves[n] for n in INS], want=OUTS)))
    assert not out["q_scale"].requires_grad and not out["p_scale"].requires_grad
    total = sum((out[n] * u.to(DEV)).sum() for n, u in ups.items())
    gs = torch.autograd.grad(total, [leaves[n] for n in INS[:4]])
    return dict(zip(INS[:4], gs))


def check_grads(c, got, ups, tag):
    g64 = grads_of(restate64, c["x"], ups, torch.float64)
    g32 = grads_of(torch_chain, c["x"], ups, torch.float32)
    worst = 0.0
    for n in INS[:4]:
        err32 = float((g32[n].double() - g64[n]).abs().max())
        bound = max(4 * err32, EPS20 * float(g64[n].abs().max()))
        err = float((got[n].detach().cpu().double() - g64[n]).abs().max())
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
        assert err <= bound, "%s %s: error %.3e bound %.3e" % (tag, n, err, bound)
    return worst


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_all_upstreams_and_each_alone(cases, shape):
    c = cases(shape)
    ups = upstreams(*shape)
    worst = check_grads(c, kernel_grads(c, ups), ups, "all")
    for n in UPS:
        worst = max(worst, check_grads(c, kernel_grads(c, {n: ups[n]}), {n: ups[n]}, n + " alone"))
    print("backward %s: worst error / bound %.3f" % (shape, worst))
    # sigma'(raw) is exactly 1 above the threshold: d z_q / d q_raw[:, 0] = eps_q * g
    got = kernel_grads(c, {"z_q": ups["z_q"]})
    assert torch.equal(got["q_raw"][:, 0].cpu(), (c["x"]["eps_q"] * ups["z_q"])[:, 0])
    # nothing flows from logq into q_loc
    assert float(kernel_grads(c, {"logq": ups["logq"]})["q_loc"].abs().max()) == 0.0


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_reads_a_column_slice_in_place(cases, shape):
    """the entry point itself: g_zq as columns [3, 3 + Z) of a [B, Z + 5] tensor, row stride Z + 5"""
    from rfn_hip import lib as L
    c = cases(shape)
    B, Z = shape
    ups = upstreams(B, Z)
    d = c["xd"]
    wide = torch.full((B, Z + 5), float("nan"), device=DEV)
    wide[:, 3:3 + Z] = ups["z_q"].to(DEV)
    u = {n: t.to(DEV) for n, t in ups.items()}

    def call(g_zq_ptr, ns):
        outs = [torch.empty(B, Z, device=DEV) for _ in range(4)]
        L.call("rfn_gauss_heads_bwd_f32", *[L.dev(d[n]) for n in INS], g_zq_ptr, ns, L.dev(u["z_p"]), Z, L.dev(u["kl"]),
               L.dev(u["logq"]), L.dev(u["logp"]), *[L.dev(o) for o in outs], B, Z)
        return dict(zip(INS[:4], outs))
    dense = call(L.dev(u["z_q"]), Z)
    sliced = call(wide.data_ptr() + 3 * 4, Z + 5)
    for n in INS[:4]:
        assert torch.equal(dense[n], sliced[n]), n
    worst = check_grads(c, sliced, ups, "slice")
    print("backward from a column slice %s: worst error / bound %.3f" % (shape, worst))
    # and through autograd: torch.cat hands the Function a narrow view of the wider gradient
    from rfn_hip import ops
    leaves = {n: d[n].clone().requires_grad_(n in INS[:4]) for n in INS}
    z_q, = ops.gauss_heads(*[leaves[n] for n in INS], want=("z_q",))
    pad = torch.zeros(B, 3, device=DEV)
    w = torch.cat([pad, u["z_q"], pad[:, :2]], 1)
    gs = torch.autograd.grad((torch.cat([pad, z_q, pad[:, :2]], 1) * w).sum(), [leaves[n] for n in INS[:4]])
    check_grads(c, dict(zip(INS[:4], gs)), {"z_q": ups["z_q"]}, "cat")


def test_entry_point_refuses_what_it_cannot_compute(cases):
    from rfn_hip import lib as L
    c = cases((3, 20))
    d = {n: L.dev(t) for n, t in c["xd"].items()}
    out = torch.full((3, 20), 7.0, device=DEV)
    o = L.dev(out)
    load = L.load()
    cur = torch.cuda.current_stream().cuda_stream

    def fwd(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, outs, B=3, Z=20):
        return load.rfn_gauss_heads_fwd_f32(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, *outs, B, Z, cur)
    none7 = [None] * 7
    assert fwd(d["q_loc"], d["q_raw"], d["p_loc"], d["p_raw"], d["eps_q"], d["eps_p"], none7) == 0   # nothing asked
    assert fwd(d["q_loc"], d["q_raw"], d["p_loc"], d["p_raw"], None, d["eps_p"], [o] + [None] * 6) == -2     # z_q, no eps_q
    assert fwd(None, None, d["p_loc"], d["p_raw"], None, d["eps_p"], [None] * 4 + [o, None, None]) == -2     # kl, no q
    assert fwd(d["q_loc"], d["q_raw"], d["p_loc"], d["p_raw"], d["eps_q"], None, [None, o] + [None] * 5) == -2
    assert fwd(d["q_loc"], None, d["p_loc"], d["p_raw"], None, None, none7) == -1
    assert fwd(None, None, None, d["p_raw"], None, None, none7) == -1
    assert fwd(None, None, d["p_loc"], d["p_raw"], None, None, none7, B=0) == -1
    assert b"argument check failed" in load.rfn_last_error()
    rc = load.rfn_gauss_heads_bwd_f32(*[d[n] for n in INS], o, 19, None, 0, None, None, None, o, o, o, o, 3, 20, cur)
    assert rc == -3                                                       # a row stride below Z
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0          # nothing was launched


# ------------------------------------------------------------------------------------------------ bit for bit
def test_two_launches_repeat_and_a_row_does_not_depend_on_the_batch(cases):
    from rfn_hip import ops
    for shape in ((5, 64), (7, 130)):
        c = cases(shape)
        a, b = run(c, OUTS), run(c, OUTS)
        ups = upstreams(*shape)
        ga, gb = kernel_grads(c, ups), kernel_grads(c, ups)
        for n in OUTS:
            assert torch.equal(a[n], b[n]), n
        for n in INS[:4]:
            assert torch.equal(ga[n], gb[n]), n
        d = c["xd"]
        for r in range(shape[0]):
            row = [d[n][r:r + 1].contiguous() for n in INS]
            with torch.no_grad():
                one = dict(zip(OUTS, ops.gauss_heads(*row, want=OUTS)))
            for n in OUTS:
                assert torch.equal(one[n][0], a[n][r]), (n, r)
            leaves = [t.clone().requires_grad_(i < 4) for i, t in enumerate(row)]
            out = dict(zip(OUTS, ops.gauss_heads(*leaves, want=OUTS)))
            total = sum((out[n] * ups[n][r:r + 1].to(DEV)).sum() for n in UPS)
            for n, g in zip(INS[:4], torch.autograd.grad(total, leaves[:4])):
                assert torch.equal(g[0], ga[n][r]), (n, r)


def test_a_captured_launch_equals_the_eager_one(cases):
    from rfn_hip import lib as L
    from rfn_hip import ops
    c = cases((7, 130))
    B, Z = 7, 130
    d = c["xd"]
    ups = {n: t.to(DEV) for n, t in upstreams(B, Z).items()}
    eager = run(c, OUTS)
    eager_g = kernel_grads(c, {n: t.cpu() for n, t in ups.items()})
    ins = {n: torch.zeros_like(t) for n, t in d.items()}
    gouts = [torch.empty(B, Z, device=DEV) for _ in range(4)]

    def body():
        with torch.no_grad():
            out = ops.gauss_heads(*[ins[n] for n in INS], want=OUTS)
        L.call("rfn_gauss_heads_bwd_f32", *[L.dev(ins[n]) for n in INS], L.dev(ups["z_q"]), Z, L.dev(ups["z_p"]), Z,
               L.dev(ups["kl"]), L.dev(ups["logq"]), L.dev(ups["logp"]), *[L.dev(o) for o in gouts], B, Z)
        return out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    for n in INS:
        ins[n].copy_(d[n])
    graph.replay()
    torch.cuda.synchronize()
    for n, t in zip(OUTS, out):
        assert torch.equal(t, eager[n]), n
    for n, t in zip(INS[:4], gouts):
        assert torch.equal(t, eager_g[n]), n
