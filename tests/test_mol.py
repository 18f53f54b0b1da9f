"""rfn_hip.ops.mol_nll / mol_sample (csrc/mol.hip) against the reference's float64 results of tests/golden/mol*.pt.

Bounds: for each tensor, 4x the largest error of the REFERENCE'S OWN float32 run against its float64 run on the same
inputs (both stored in the fixture), in max norm.  A pixel with an item whose float64 cdf_delta lies within 1 % of the
1e-5 threshold of the discontinuous select is left out (at most 2 % of the pixels); in the per-frame sums such a pixel
enters the yardstick with the kernel's own value.  The upstream gradients are non-uniform; a pixel's nll depends on that
pixel's parameters alone, so the weighted gradient is the stored d(sum nll_pix)/dl times the pixel's weight: exactly
for the float64 yardstick, rounded to float32 for the reference's float32 run (whose result is a float32 tensor).

Measured on an MI355X, kernel error / bound for nll_pix, frame nll, dl (per-pixel upstream), dl (per-frame upstream):
  rgb_m10   9.9e-6 / 2.2e-2   8.4e-5 / 2.5e-2   6.9e-4 / 5.1e-1   8.8e-4 / 7.5e-1
  gray_m10  1.6e-6 / 8.6e-4   4.7e-5 / 9.8e-4   2.5e-3 / 6.3e-2   1.5e-3 / 8.9e-2
  gray_m1   8.4e-6 / 3.4e-5   1.5e-5 / 5.9e-5   5.9e-5 / 2.4e-4   1.1e-5 / 4.6e-5
  rgb_m3    6.0e-5 / 3.0e-2   4.7e-4 / 7.6e-2   3.6e-3 / 7.4e-2   3.9e-3 / 5.5e-2
"""
import pytest
import torch

from tests import mol_ref as R
from tests.test_mol_host import CASES, load_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from rfn_hip import lib, ops as K
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return K


@pytest.fixture(scope="module")
def cases():
    """per case: the fixture, the kept-pixel mask and the upstream weights; computed once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            c = dict(load_case(name))
            N, _, H, W = c["x"].shape
            c["keep"] = ~R.near_threshold(c["x"].double(), c["l"].double())
            g = torch.Generator().manual_seed(31 + N * H * W)
            c["up_frame"] = torch.rand(N, generator=g) + 0.5
            c["up_pixel"] = torch.randn(N, H, W, generator=g)
            cache[name] = c
        return cache[name]
    return get


def _run(ops, c, reduce, up):
    x = c["x"].to(DEV)
    l = c["l"].to(DEV).requires_grad_(True)
    out = ops.mol_nll(x, l, reduce=reduce)
    (out * up.to(DEV)).sum().backward()
    return out.detach().cpu(), l.grad.cpu()


@pytest.mark.parametrize("name", CASES)
def test_nll_and_gradient_against_float64(ops, cases, name):
    c = cases(name)
    keep = c["keep"]
    left_out = 1.0 - float(keep.float().mean())
    print("%s: pixels left out %.4f" % (name, left_out))
    assert left_out <= 0.02
    N = c["x"].shape[0]
    pix, dl_p = _run(ops, c, "pixel", c["up_pixel"])
    frame, dl_f = _run(ops, c, "frame", c["up_frame"])
    n64, n32, g64, g32 = c["nll_pix64"], c["nll_pix32"], c["dl64"], c["dl32"]
    kd = keep.unsqueeze(1).expand_as(g64)
    checks = []
    # nll_pix
    checks.append(("nll_pix", float((pix.double() - n64)[keep].abs().max()), 4 * float((n32.double() - n64)[keep].abs().max())))
    # per-frame sums: the reference's float32 sum of its float32 pixels against the float64 sum, over the kept pixels
    zero32, zero64 = torch.zeros((), dtype=torch.float32), torch.zeros((), dtype=torch.float64)
    ref32 = torch.where(keep, n32, zero32).reshape(N, -1).sum(1)
    ref64 = torch.where(keep, n64, zero64).reshape(N, -1).sum(1)
    yard = torch.where(keep, n64, pix.double()).reshape(N, -1).sum(1)
    checks.append(("nll", float((frame.double() - yard).abs().max()), 4 * float((ref32.double() - ref64).abs().max())))
    # gradients under both upstream forms
    for tag, got, w in (("dl(pixel)", dl_p, c["up_pixel"].unsqueeze(1)), ("dl(frame)", dl_f, c["up_frame"].view(N, 1, 1, 1))):
        # (the float32 run's weighted gradient is a float32 number too: its product with the weight is rounded)
        ref32_w, w = (g32 * w).double(), w.double()
        checks.append((tag, float((got.double() - g64 * w)[kd].abs().max()),
                       4 * float((ref32_w - g64 * w)[kd].abs().max())))
    for tag, err, bound in checks:
        print("%s %-10s kernel error %.3e  bound %.3e" % (name, tag, err, bound))
    assert bool(torch.isfinite(dl_p).all()) and bool(torch.isfinite(dl_f).all())
    for tag, err, bound in checks:
        assert err <= bound, (name, tag, err, bound)
    # the pixel form and the frame form are the same per-pixel numbers
    pix2, _ = _run(ops, c, "pixel", c["up_pixel"])
    assert torch.equal(pix, pix2)


@pytest.mark.parametrize("name", CASES)
def test_repeats_bit_for_bit_and_frames_stand_alone(ops, cases, name):
    c = cases(name)
    N = c["x"].shape[0]
    a, ga = _run(ops, c, "frame", c["up_frame"])
    b, gb = _run(ops, c, "frame", c["up_frame"])
    assert torch.equal(a, b) and torch.equal(ga, gb)
    x, l = c["x"].to(DEV), c["l"].to(DEV)
    for i in range(N):
        alone = ops.mol_nll(x[i:i + 1], l[i:i + 1], reduce="frame").cpu()
        assert torch.equal(alone, a[i:i + 1]), (name, i)
    if N > 1:  # another neighbourhood: reversed frame order
        rev = ops.mol_nll(x.flip(0), l.flip(0), reduce="frame").cpu()
        assert torch.equal(rev.flip(0), a)


@pytest.mark.parametrize("name", CASES)
def test_sample_against_float64(ops, cases, name):
    c = cases(name)
    N, C, H, W = c["x"].shape
    M = c["M"]
    g = torch.Generator().manual_seed(5 + M + H)
    u_mix = torch.rand(N, H, W, M, generator=g) * (1 - 2e-5) + 1e-5
    u_x = torch.rand(N, H, W, C, generator=g) * (1 - 2e-5) + 1e-5
    ref, gap = R.sample(c["l"].double(), u_mix.double(), u_x.double())
    out = ops.mol_sample(c["l"].to(DEV), u_mix.to(DEV), u_x.to(DEV)).cpu()
    assert out.shape == (N, C, H, W)
    keep = (gap >= 1e-4).unsqueeze(1).expand_as(out)
    left_out = 1.0 - float(keep.float().mean())
    err = float((out.double() - ref)[keep].abs().max())
    print("%s: sample error %.3e, pixels left out %.4f" % (name, err, left_out))
    assert left_out <= 0.01
    assert err <= 1e-5
    assert float(out.abs().max()) <= 1.0
    # the recorded draws of the reference replay, and a call without uniforms draws its own in the reference's order
    again = ops.mol_sample(c["l"].to(DEV), c["u_mix"].to(DEV), c["u_x"].to(DEV)).cpu()
    r32, gap32 = R.sample(c["l"].double(), c["u_mix"].double(), c["u_x"].double())
    k32 = (gap32 >= 1e-4).unsqueeze(1).expand_as(again)
    assert float((again - c["sample32"])[k32].abs().max()) <= 1e-5
    gen = torch.Generator(device=DEV).manual_seed(9)
    own = ops.mol_sample(c["l"].to(DEV), generator=gen, channels=C)
    gen.manual_seed(9)
    um = torch.empty(N, H, W, M, device=DEV).uniform_(1e-5, 1 - 1e-5, generator=gen)
    ux = torch.empty(N, H, W, C, device=DEV).uniform_(1e-5, 1 - 1e-5, generator=gen)
    assert torch.equal(own, ops.mol_sample(c["l"].to(DEV), um, ux))


def test_error_paths(ops):
    x = torch.zeros(2, 3, 4, 4, device=DEV)
    l = torch.zeros(2, 30, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.mol_nll(x, torch.zeros(2, 31, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.mol_nll(x, torch.zeros(2, 30, 4, 5, device=DEV))
    with pytest.raises(RuntimeError, match="device"):
        ops.mol_nll(x.cpu(), l)
    with pytest.raises(RuntimeError, match="device"):
        ops.mol_nll(x, l.cpu())
    with pytest.raises(RuntimeError, match="no gradient flows into x"):
        ops.mol_nll(x.clone().requires_grad_(True), l)
    with pytest.raises(ValueError):
        ops.mol_nll(x, l, reduce="batch")
    with pytest.raises(RuntimeError, match="device"):
        ops.mol_sample(l.cpu(), channels=3)
    with pytest.raises(RuntimeError, match="uniforms"):
        ops.mol_sample(l, torch.rand(2, 4, 4, 4, device=DEV), torch.rand(2, 4, 4, 3, device=DEV))


def test_capturable_in_a_graph(ops, cases):
    """the launches go to the current stream and allocate nothing a capture cannot hold: likelihood and sampler captured
    once, replayed on new inputs"""
    c = cases("rgb_m3")
    x, l = c["x"].to(DEV), c["l"].to(DEV)
    u_mix, u_x = c["u_mix"].to(DEV), c["u_x"].to(DEV)
    eager, eager_s = ops.mol_nll(x, l), ops.mol_sample(l, u_mix, u_x)
    l_in = torch.zeros_like(l)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.mol_nll(x, l_in), ops.mol_sample(l_in, u_mix, u_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, out_s = ops.mol_nll(x, l_in), ops.mol_sample(l_in, u_mix, u_x)
    l_in.copy_(l)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out_s, eager_s)
