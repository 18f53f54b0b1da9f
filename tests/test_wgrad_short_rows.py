"""The 3x3 weight gradients of 4 x 4 and 2 x 2 maps with the taps shifted while staging (wgrad_plan forms "implicit_rows" and
"mirrored_rows", rfn_conv3x3_wgrad_rows[_mirrored][_grouped]_bf16x3): a staging unit of 8 pixels is two image rows of a
4-pixel-wide frame, or two whole 2 x 2 frames -- the last unit of an odd frame count holds one.

Exact cases: operands of small integers in [-2, 2], so every bf16 piece, product and partial sum is exactly representable
and the order of the float atomics cannot matter: the result must EQUAL the fp64 F.conv2d weight gradient.  A wrong tap,
a missing zero fill, a frame read past the end or a transposed output is a different integer.  The cases at the model's
channel counts hold the bound of the existing grouped weight-gradient tests for the same arithmetic (relerr < 2e-5)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = ("rfn_conv3x3_wgrad_rows_bf16x3", "rfn_conv3x3_wgrad_rows_grouped_bf16x3")
ROWS_MIRRORED = ("rfn_conv3x3_wgrad_rows_mirrored_bf16x3", "rfn_conv3x3_wgrad_rows_mirrored_grouped_bf16x3")
LABEL = {4: "gemm_wgrad_b3_kernel<2,2,2,2,64,2>", 2: "gemm_wgrad_b3_kernel<2,2,2,2,64,3>"}
EXPANSIONS = ("rfn_tap_scatter_f32", "rfn_im2col3x3_f32")


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert ops.bwd_b3(), "the short-row forms are the split-precision gradient path"
    return ops


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _profiled(fn):
    """fn() with the library's call profile on and torch.cat counted: (result, [(entry point, label)], cat calls)"""
    from rfn_hip import lib
    old, lib.PROFILE = lib.PROFILE, []
    cat, cats = torch.cat, []

    def counted(*a, **kw):
        cats.append(1)
        return cat(*a, **kw)
    torch.cat = counted
    try:
        out = fn()
        torch.cuda.synchronize()
        calls = [(name, meta[1]) for (name, meta, _, _) in lib.PROFILE if meta is not None]
    finally:
        lib.PROFILE, torch.cat = old, cat
    return out, calls, len(cats)


def _label(G, S):
    return LABEL[S].replace("<", "<grouped ") if G else LABEL[S]


def _data(form, S, N, chans, n, integers, seed):
    """operands of n gradients on the CPU and their fp64 references: implicit -- chans = (channels of the tensor in1 is the
    LAST C1 channels of, C1, C2, Cout); mirrored -- chans = (Cin, C)"""
    g = torch.Generator().manual_seed(seed)

    def draw(*shape):
        return torch.randint(-2, 3, shape, generator=g).float() if integers else torch.randn(*shape, generator=g)

    if form == "implicit":
        Ctot, C1, C2, Cout = chans
        wide = [draw(N, Ctot, S, S) for _ in range(n)]
        in2 = [draw(N, C2, S, S) for _ in range(n)]
        gy = draw(n, N, Cout, S, S)
        xs = [torch.cat((wide[i][:, Ctot - C1:], in2[i]), 1) for i in range(n)]
        ops_ = (wide, in2, gy)
    else:
        Cin, Cout = chans
        xs = [draw(N, Cin, S, S) for _ in range(n)]
        gy = draw(n, N, Cout, S, S)
        ops_ = (xs, None, gy)
    refs = []
    for i in range(n):
        w = torch.zeros(Cout, xs[i].shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(xs[i].double(), w, padding=1).backward(gy[i].double())
        refs.append(w.grad)
    return ops_, refs


def _run(K, form, G, S, chans, ops_, **kw):
    """the n gradients through the public functions (single: G = 0), with their launches and cat calls"""
    a, b, gy = ops_
    gyc = gy.cuda()
    gl = [gyc[i] for i in range(max(G, 1))]
    if form == "implicit":
        Ctot, C1, C2, Cout = chans
        in1 = [t.cuda()[:, Ctot - C1:] for t in a]
        in2 = [t.cuda() for t in b]
        if G:
            return _profiled(lambda: K.conv2d_wgrad_grouped(in1, in2, gl, Cout, 3, g_stacked=gyc, **kw))
        return _profiled(lambda: [K.conv2d_wgrad(in1[0], in2[0], gl[0], Cout, 3, **kw)])
    Cin, C = chans
    xs = [t.cuda() for t in a]
    if G:
        return _profiled(lambda: K.zeros_conv_wgrad_grouped(xs, gl, C, g_stacked=gyc, **kw))
    return _profiled(lambda: [K.zeros_conv_wgrad(xs[0], gl[0], C, 3, **kw)])


# form, map, N, channels: what it exercises
EXACT = {
    "implicit_4x4": ("implicit", 4, 5, (6, 3, 7, 40)),    # odd N, in1 a channel slice with its own frame stride, partial tile
    "implicit_2x2": ("implicit", 2, 7, (6, 6, 10, 24)),   # the last unit holds one frame
    "mirrored_4x4": ("mirrored", 4, 5, (40, 6)),          # 54 of 64 columns
    "mirrored_2x2": ("mirrored", 2, 9, (72, 16)),         # 144 columns: two column tiles
}
_exact_cache = {}


def _exact_data(name, n):
    if (name, n) not in _exact_cache:
        form, S, N, chans = EXACT[name]
        _exact_cache[name, n] = _data(form, S, N, chans, n, True, 4100 + 10 * sorted(EXACT).index(name) + n)
    return _exact_cache[name, n]


@pytest.mark.parametrize("G", [0, 3])
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_on_small_integers(K, name, G):
    form, S, N, chans = EXACT[name]
    ops_, refs = _exact_data(name, max(G, 1))
    for r in refs:   # the inputs make every tap's gradient non-trivial: a dropped or misplaced tap cannot hide
        assert all(bool(r[:, :, t // 3, t % 3].abs().max() > 0) for t in range(9)), name
        assert float(r.abs().max()) < 2 ** 20
    got, calls, cats = _run(K, form, G, S, chans, ops_, short_rows=True)
    entry = (ROWS if form == "implicit" else ROWS_MIRRORED)[1 if G else 0]
    assert calls == [(entry, _label(G, S))], calls
    assert cats == 0
    assert len(got) == len(refs)
    for i, (a, r) in enumerate(zip(got, refs)):
        assert tuple(a.shape) == tuple(r.shape)
        assert torch.equal(a.cpu().double(), r), (name, G, i, float((a.cpu().double() - r).abs().max()))


# form, G, N, channels, map at the model's channel counts (levels 3 and 4 of the flow)
MODEL = [
    ("implicit", 3, 33, (16, 16, 128, 256), 4),
    ("implicit", 2, 33, (32, 32, 256, 256), 2),
    ("mirrored", 3, 40, (256, 32), 4),       # 288 columns
    ("mirrored", 2, 40, (256, 64), 2),       # 576 columns
]


@pytest.mark.parametrize("form,G,N,chans,S", MODEL)
def test_model_channel_counts_against_fp64(K, form, G, N, chans, S):
    ops_, refs = _data(form, S, N, chans, G, False, 5200 + S + G)
    got, calls, cats = _run(K, form, G, S, chans, ops_, short_rows=True)
    assert calls == [((ROWS if form == "implicit" else ROWS_MIRRORED)[1], _label(G, S))] and cats == 0
    errs = [relerr(a, r) for a, r in zip(got, refs)]
    print("%s G%d N%d %s %dx%d: relerr %s" % (form, G, N, chans, S, S, ["%.3g" % e for e in errs]))
    assert max(errs) < 2e-5, errs


@pytest.mark.parametrize("name", sorted(EXACT))
@pytest.mark.parametrize("G", [0, 3])
def test_the_plan_is_what_runs(K, name, G):
    """with short_rows the launches are plan.launches -- one, no expansion pass, no cat; without it they are today's"""
    form, S, N, chans = EXACT[name]
    ops_, refs = _exact_data(name, max(G, 1))
    if form == "implicit":
        Ctot, C1, C2, Cout = chans
        args, kw = (G, N, C1, C2, Cout, S, S, 3), dict(g_ns=Cout * S * S, in1_ns=Ctot * S * S, stacked=bool(G))
    else:
        Cin, C = chans
        args, kw = (G, N, Cin, 0, C, S, S, 3), dict(few_out=True, stacked=bool(G))
    plan = K.wgrad_plan(*args, short_rows=True, **kw)
    got, calls, cats = _run(K, form, G, S, chans, ops_, short_rows=True)
    assert calls == plan.launches and len(calls) == 1 and cats == 0, (calls, plan)
    assert not any(e in EXPANSIONS for e, _ in calls)
    today = K.wgrad_plan(*args, **kw)
    old, calls_old, cats_old = _run(K, form, G, S, chans, ops_)
    assert calls_old == today.launches and today.form in ("im2col", "scatter"), (calls_old, today)
    assert any(e in EXPANSIONS for e, _ in calls_old)
    for a, b in zip(got, old):   # (integers: both routes are exact)
        assert torch.equal(a, b)


# ---- one level node end to end: the short-row launches against RFN_WGRAD_SHORT_ROWS=0 in a fresh child process
LEVEL = dict(N=48, C=8, Cc=12, S=4, Kn=2, Hd=256)


def _level_param_grads():
    """parameter gradients of one GlowLevelFn node (K = 2 steps, 4 x 4 maps, 48 frames) on seeded inputs, and the library
    launches of its backward pass"""
    from rfn_hip import ops as K
    N, C, Cc, S, Kn, Hd = (LEVEL[k] for k in ("N", "C", "Cc", "S", "Kn", "Hd"))
    Ch = C // 2
    g = torch.Generator().manual_seed(91)

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
    gout = torch.randn(N, C, S, S, generator=g).cuda()
    gdl = torch.randn(N, generator=g).cuda()
    out, dl = K.GlowLevelFn.apply(x, cond, Wst, K.ACT["leakyrelu"], K.CLAMP["realnvp"], None,
                                  *[t for st in steps for t in st])
    _, calls, _ = _profiled(lambda: ((out * gout).sum() + (dl * gdl).sum()).backward())
    return [t.grad.detach().cpu() for t in [Wst] + [t for st in steps for t in st]], [c[0] for c in calls]


def _child_main(path):
    grads, calls = _level_param_grads()
    torch.save({"grads": grads, "calls": calls}, path)


def test_level_node_equals_the_expanding_routes(K, tmp_path):
    """every parameter gradient of the node within 2e-5 relative of the same node with RFN_WGRAD_SHORT_ROWS=0 (im2col /
    tap scatter + GEMM): both sum the same products in fp32, in another order"""
    assert os.environ.get("RFN_WGRAD_SHORT_ROWS") != "0"
    grads, calls = _level_param_grads()
    assert sum(c in ROWS for c in calls) == 1 and sum(c in ROWS_MIRRORED for c in calls) == 1, calls
    assert not any(c in EXPANSIONS for c in calls), calls
    path = str(tmp_path / "expanded.pt")
    env = dict(os.environ, RFN_WGRAD_SHORT_ROWS="0")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import tests.conftest; "
                        "from tests.test_wgrad_short_rows import _child_main; _child_main(%r)" % (ROOT, path)],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    old = torch.load(path, weights_only=False)
    assert not any(c in ROWS + ROWS_MIRRORED for c in old["calls"]), old["calls"]
    assert any(c in EXPANSIONS for c in old["calls"]), old["calls"]
    assert len(old["grads"]) == len(grads)
    worst = 0.0
    for i, (a, b) in enumerate(zip(grads, old["grads"])):
        assert a.shape == b.shape
        e = relerr(a, b)
        worst = max(worst, e)
        assert e < 2e-5, (i, e)
    print("level node, short rows vs expanded: worst relerr %.3g over %d gradients" % (worst, len(grads)))
