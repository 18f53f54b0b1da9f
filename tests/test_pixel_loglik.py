"""ops.pixel_loglik and ops.normal_logvar_pair on the GPU against the float64 restatement of tests/pixel_loglik_ref.py
(DESIGN.md section 29).

pixel_loglik, per row:  |out - ref| <= (A(N) + 6) * 2^-24 * sum_n |l_n|,  A(N) = pixel_loglik_ref.longest_chain(N) the
additions on the longest path of the documented order.  The six per term are an allowance, not a measurement; what the
kernel spends of it, counted in units of 2^-24 relative to |l_n|:
  bernoulli  logf and log1pf at most 2 ulp each (4 units on the factor they multiply; x log(pc) and (1 - x) log1p(-pc)
             have the same sign for x in [0, 1], so each factor's error is relative to the term), the products, 1 - x and
             the sum are fp64 operations on fp32 values (below 2^-50), one rounding of the term to fp32: 5
  gaussian   x + u, the difference, the square, the product with 1 / (2 scale^2) and the sum with the constant are fp64
             (the constants are fp64 too), one rounding of the term: 1 (+ 2^-50s)
  mse        likewise: 1
normal_logvar_pair, per row:  (ceil(log2 Z) + 8) * 2^-24 * sum_j |term_j|; the kernel's terms are fp64 (fp64 exp) rounded
once, and for Z <= 128 the lane's chain plus the butterfly's additions of non-zero values are at most ceil(log2 Z)
(lane 0 adds at most two terms, one rounded addition, and the butterfly has six levels, of which those that add the
zeros of idle lanes are exact): Z = 1: 0, 10: 4, 64: 6, 65: 7.
Every test prints its worst error / bound before it asserts."""
import math

import pytest
import torch

from tests import pixel_loglik_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
EPS = 2.0 ** -23

# (K, B) at every N, and the 3x64x64 frame at R = 6, B = 3
SHAPES = [(K, B, N) for N in (1, 3, 35, 256, 64 * 64) for K in (1, 2) for B in (1, 2, 3)] + [(2, 3, 3 * 64 * 64)]
VARIANTS = ["bernoulli-binary", "bernoulli-uniform", "gaussian-0.01", "gaussian-0.01-noise", "gaussian-1", "gaussian-1-noise",
            "gaussian-30", "gaussian-30-noise", "mse"]
BERNOULLI_EDGES = [0.0, 1.0, EPS, 1.0 - EPS, 2.0 ** -21, 1.0 - 2.0 ** -21, 3 * 2.0 ** -22, 1.0 - 3 * 2.0 ** -22, 2.0 ** -20,
                   1.0 - 2.0 ** -20, 2.0 ** -30, 1.0 - 2.0 ** -24]


def _inputs(variant, K, B, N, seed):
    """(pred [K*B, N], target [B, N], mode, scale, noise) on the device"""
    g = torch.Generator().manual_seed(seed)
    Rr = K * B
    mode = variant.split("-")[0]
    scale = noise = None
    if mode == "bernoulli":
        pred = torch.rand(Rr, N, generator=g)
        flat = pred.view(-1)
        edges = torch.tensor(BERNOULLI_EDGES, dtype=torch.float32)
        n = min(flat.numel(), len(edges))
        shift = seed % len(edges)                                  # small shapes see different edges
        flat[:n] = torch.roll(edges, -shift)[:n]
        target = torch.rand(B, N, generator=g)
        if variant.endswith("binary"):
            target = target.round()
    elif mode == "gaussian":
        scale = float(variant.split("-")[1])
        pred = torch.rand(Rr, N, generator=g)
        target = torch.randint(0, 256, (B, N), generator=g).float() / 255.0
        if variant.endswith("noise"):
            noise = torch.rand(Rr, N, generator=g) / 256.0
    else:
        target = torch.rand(B, N, generator=g)
        pred = target.repeat(K, 1) + (torch.rand(Rr, N, generator=g) * 2.0 - 1.0) * 1e3
    dev = lambda t: None if t is None else t.to(DEV)
    return dev(pred), dev(target), mode, scale, dev(noise)


def _ratio(out, pred, target, mode, scale, noise):
    """worst |out - ref| / bound over the rows (the bound is positive: no row of these inputs is all zeros)"""
    ref, mag = R.pixel_loglik64(pred, target, mode, scale, noise)
    N = pred[0].numel()
    bound = (R.longest_chain(N) + 6) * U * mag
    assert bool(torch.isfinite(out).all()) and bool((bound > 0).all())
    return float(((out.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("variant", VARIANTS)
def test_pixel_loglik_against_fp64(variant):
    from rfn_hip import ops
    worst = 0.0
    for i, (K, B, N) in enumerate(SHAPES):
        pred, target, mode, scale, noise = _inputs(variant, K, B, N, 100 + i)
        out = ops.pixel_loglik(pred, target, mode, scale=scale, noise=noise)
        assert out.shape == (K * B,) and out.dtype == torch.float32 and out.is_cuda
        r = _ratio(out, pred, target, mode, scale, noise)
        worst = max(worst, r)
        assert r <= 1.0, (variant, K, B, N, r)
        if N == 35:    # the [R, C, H, W] form is the same call
            again = ops.pixel_loglik(pred.view(K * B, 1, 5, 7), target.view(B, 1, 5, 7), mode, scale=scale,
                                     noise=None if noise is None else noise.view(K * B, 1, 5, 7))
            assert torch.equal(again, out)
    print("%s: worst error / bound over %d shapes %.3e" % (variant, len(SHAPES), worst))


def test_bernoulli_edges():
    """every edge value of p against x = 0, 1, 1/4 and uniform: p exactly 0 and 1 are clamped to 2^-23 and 1 - 2^-23"""
    from rfn_hip import ops
    g = torch.Generator().manual_seed(7)
    edges = torch.tensor(BERNOULLI_EDGES, dtype=torch.float32)
    N = len(edges)
    target = torch.stack([torch.zeros(N), torch.ones(N), torch.full((N,), 0.25), torch.rand(N, generator=g)]).to(DEV)
    pred = edges.repeat(8, 1).to(DEV)                              # K = 2
    out = ops.pixel_loglik(pred, target, "bernoulli")
    r = _ratio(out, pred, target, "bernoulli", None, None)
    print("bernoulli edges: error / bound %.3e; rows %s" % (r, out.tolist()))
    assert r <= 1.0
    # one element each under x = 1: p = 0 is clamped to 2^-23, p = 1 to 1 - 2^-23
    one = ops.pixel_loglik(torch.tensor([[0.0], [1.0]], device=DEV), torch.ones(1, 1, device=DEV), "bernoulli")
    assert one.tolist() == pytest.approx([math.log(EPS), math.log1p(-EPS)], rel=3e-7)


@pytest.mark.parametrize("variant", ["bernoulli-binary", "gaussian-0.01-noise", "gaussian-1", "gaussian-30-noise", "mse"])
def test_pixel_loglik_against_the_torch_chain(variant):
    """the chain of VRNN._lpx / SVG._lpx on the repeated frames; relative difference of the row sums at most 1e-5"""
    import torch.distributions as td
    from rfn_hip import ops
    worst = 0.0
    for N in (35, 64 * 64):
        K, B = 2, 3
        pred, target, mode, scale, noise = _inputs(variant, K, B, N, 300 + N)
        if mode == "bernoulli":
            pred = torch.rand(K * B, N, generator=torch.Generator().manual_seed(N)).to(DEV)   # (no edge values here)
        x_rep = target.repeat(K, 1)
        if mode == "bernoulli":
            chain = td.Bernoulli(probs=pred).log_prob(x_rep).sum(1)
        elif mode == "gaussian":
            x = x_rep if noise is None else x_rep + noise
            chain = td.Normal(pred, scale * torch.ones_like(pred)).log_prob(x).sum(1)
        else:
            chain = -torch.nn.MSELoss(reduction="none")(pred, x_rep).sum(1)
        out = ops.pixel_loglik(pred, target, mode, scale=scale, noise=noise)
        rel = float(((out - chain).abs() / chain.abs()).max())
        worst = max(worst, rel)
        assert rel <= 1e-5, (variant, N, rel)
    print("%s: worst relative difference to the torch chain %.3e" % (variant, worst))


@pytest.mark.parametrize("N", [35, 256, 1027])
def test_rows_do_not_depend_on_the_call(N):
    """bit for bit: two launches; row k*B + b of the R-row call against row b of a B-row call on that slice of pred (at
    N = 35 and 1027 the slices' rows have other alignments than in the whole call: 16-byte path against single floats);
    a frame view of a [B, T, N] batch against its copy; a side stream"""
    from rfn_hip import ops
    K, B = 3, 3
    pred, target, mode, scale, noise = _inputs("gaussian-1-noise", K, B, N, 500 + N)
    out = ops.pixel_loglik(pred, target, mode, scale=scale, noise=noise)
    assert torch.equal(out, ops.pixel_loglik(pred, target, mode, scale=scale, noise=noise))
    for k in range(K):
        part = ops.pixel_loglik(pred[k * B:(k + 1) * B], target, mode, scale=scale, noise=noise[k * B:(k + 1) * B])
        assert torch.equal(part, out[k * B:(k + 1) * B]), k
    for b in range(B):   # and one row alone, K = 1, B = 1
        row = ops.pixel_loglik(pred[B + b:B + b + 1], target[b:b + 1], mode, scale=scale, noise=noise[B + b:B + b + 1])
        assert torch.equal(row, out[B + b:B + b + 1])
    batch = torch.rand(B, 4, N, device=DEV)
    batch[:, 2] = target
    assert not batch[:, 2].is_contiguous() or B == 1
    assert torch.equal(ops.pixel_loglik(pred, batch[:, 2], mode, scale=scale, noise=noise), out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.pixel_loglik(pred, target, mode, scale=scale, noise=noise)
    side.synchronize()
    assert torch.equal(other, out)
    for m in ("bernoulli", "mse"):
        a = ops.pixel_loglik(pred, target, m)
        assert torch.equal(a[B:2 * B], ops.pixel_loglik(pred[B:2 * B], target, m))


@pytest.mark.parametrize("N", [3, 35, 256])
def test_unaligned_bases(N):
    """pred, target and noise start one float past their allocations: the single-float path, same bits as aligned copies"""
    from rfn_hip import ops
    K, B = 2, 3
    pred, target, mode, scale, noise = _inputs("gaussian-1-noise", K, B, N, 700 + N)

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, device=DEV)
        buf[1:] = t.reshape(-1)
        v = buf[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    want = ops.pixel_loglik(pred, target, mode, scale=scale, noise=noise)
    got = ops.pixel_loglik(shifted(pred), shifted(target), mode, scale=scale, noise=shifted(noise))
    assert torch.equal(got, want)
    assert _ratio(got, pred, target, mode, scale, noise) <= 1.0
    for m in ("bernoulli", "mse"):
        assert torch.equal(ops.pixel_loglik(shifted(pred), target, m), ops.pixel_loglik(pred, shifted(target), m))


def test_canary_empty_and_many_rows():
    from rfn_hip import ops
    K, B, N = 2, 3, 35
    pred, target, mode, scale, noise = _inputs("mse", K, B, N, 900)
    # out is a view inside a larger buffer: the bytes around it are untouched
    buf = torch.full((K * B + 64,), float("nan"), device=DEV)
    buf.view(torch.int32)[:] = 0x7FC0BEEF
    before = buf.view(torch.int32).clone()
    out = ops.pixel_loglik(pred, target, mode, out=buf[32:32 + K * B])
    assert out.data_ptr() == buf[32:].data_ptr()
    after = buf.view(torch.int32)
    assert torch.equal(after[:32], before[:32]) and torch.equal(after[32 + K * B:], before[32 + K * B:])
    assert torch.equal(buf[32:32 + K * B], ops.pixel_loglik(pred, target, mode))
    with pytest.raises(ValueError, match="out must be"):
        ops.pixel_loglik(pred, target, mode, out=buf[:K * B + 1])
    # R = 0: an empty tensor, no launch
    empty = ops.pixel_loglik(pred[:0], target, mode)
    assert empty.shape == (0,) and empty.is_cuda
    # more rows than the grid has workgroups (65536): the grid-stride loop gives every row the bits of a small call
    Rr = 65536 + 3
    g = torch.Generator().manual_seed(5)
    many, tgt = torch.rand(Rr, 3, generator=g).to(DEV), torch.rand(1, 3, generator=g).to(DEV)
    out = ops.pixel_loglik(many, tgt, "bernoulli")
    assert _ratio(out, many, tgt, "bernoulli", None, None) <= 1.0
    assert torch.equal(out[-5:], ops.pixel_loglik(many[-5:], tgt, "bernoulli"))
    assert torch.equal(out[:5], ops.pixel_loglik(many[:5], tgt, "bernoulli"))


@pytest.mark.parametrize("Z", [1, 10, 64, 65])
def test_normal_logvar_pair_against_fp64(Z):
    from rfn_hip import ops
    worst = 0.0
    for B in (1, 3, 130):
        g = torch.Generator().manual_seed(40 * Z + B)
        mu_a, z_a, mu_b, z_b = (torch.randn(B, Z, generator=g).to(DEV) for _ in range(4))
        lv_a, lv_b = ((torch.rand(B, Z, generator=g) * 18.0 - 12.0).to(DEV) for _ in range(2))
        out_a, out_b = ops.normal_logvar_pair(mu_a, lv_a, z_a, mu_b, lv_b, z_b)
        assert out_a.shape == (B,) and out_b.shape == (B,) and out_a.dtype == torch.float32
        for out, (mu, lv, z) in ((out_a, (mu_a, lv_a, z_a)), (out_b, (mu_b, lv_b, z_b))):
            t = R.normal_logvar_terms64(mu, lv, z)
            bound = (math.ceil(math.log2(Z)) + 8) * U * t.abs().sum(1)
            assert bool(torch.isfinite(out).all())
            worst = max(worst, float(((out.double() - t.sum(1)).abs() / bound).max()))
        again = ops.normal_logvar_pair(mu_a, lv_a, z_a, mu_b, lv_b, z_b)
        assert torch.equal(again[0], out_a) and torch.equal(again[1], out_b)
        # the caller chooses which z goes with which distribution
        swapped = ops.normal_logvar_pair(mu_b, lv_b, z_b, mu_a, lv_a, z_a)
        assert torch.equal(swapped[0], out_b) and torch.equal(swapped[1], out_a)
        # against the chain it replaces
        import torch.distributions as td
        chain = td.Normal(mu_a, torch.exp(lv_a * 0.5)).log_prob(z_a).sum([-1])
        mag = R.normal_logvar_terms64(mu_a, lv_a, z_a).abs().sum(1)     # (a row's terms have both signs)
        assert float(((out_a - chain).abs() / mag).max()) <= 1e-5
    print("normal_logvar_pair Z = %d: worst error / bound %.3e" % (Z, worst))
    assert worst <= 1.0


def test_bound_with_kernels_on_and_off(monkeypatch):
    """SVG's bound (mse, the default loss) on recorded draws: RFN_PIXEL_LOGLIK=1 against the torch chain of =0, within the
    1e-5 relative that the deferred decoder is held to against per-k evaluation; and the kernels are what ran"""
    from argparse import Namespace
    import main_svg
    from rfn_hip import ops
    from SVG import SVG
    args = main_svg.build_parser().parse_args(
        "--batch_size 3 --x_dim 3 1 64 64 --condition_dim 3 1 64 64 --c_features 8 --h_dim 16 --z_dim 4".split())
    torch.manual_seed(11)
    m = SVG(Namespace(**vars(args))).to(DEV).eval()
    x = torch.rand(3, 3, 1, 64, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    calls = []
    plain_l, plain_n = ops.pixel_loglik, ops.normal_logvar_pair
    monkeypatch.setattr(ops, "pixel_loglik", lambda *a, **k: calls.append("l") or plain_l(*a, **k))
    monkeypatch.setattr(ops, "normal_logvar_pair", lambda *a, **k: calls.append("n") or plain_n(*a, **k))
    got = {}
    for env in ("1", "0"):
        monkeypatch.setenv("RFN_PIXEL_LOGLIK", env)
        torch.manual_seed(5)
        with torch.no_grad():
            got[env] = float(m.elbo_importance_weighting(x, 2))
        if env == "1":
            assert calls == ["n", "n", "l"] * 2
    assert calls == ["n", "n", "l"] * 2                       # =0: nothing more
    print("SVG bound: kernels %.6f torch chain %.6f" % (got["1"], got["0"]))
    assert abs(got["1"] - got["0"]) <= 1e-5 * abs(got["0"])
    monkeypatch.setenv("RFN_PIXEL_LOGLIK", "1")
    calls.clear()
    m.elbo_importance_weighting(x, 1)                          # grad mode on, parameters require grad: the torch chain
    assert calls == []
