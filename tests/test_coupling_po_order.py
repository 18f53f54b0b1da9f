"""One-hot probes of the dense K order of the fused coupling kernels' first 3x3 product (csrc/coupling_po.hip).

Forward: conv1's weight w1[co] is one-hot at the co-th (tap, input channel) pair, no ActNorm, no activation, so h1[:, co]
must be the input channel of the pair shifted by its tap, zero outside the frame.  Backward: w3 is one-hot over the
9 C (output channel, tap) pairs along the hidden axis, so ga2[:, c2] must be go[:, co] shifted by the mirrored tap.
Every slot of the K order (full units, narrow leftover units, the padding unit), every frame edge, the halo rows
between the rounds of a frame and the round that holds two 8x8 frames are named by some output.

The comparison is torch.equal: each output has one nonzero product; integers of magnitude <= 1000 (< 2^11) and a
weight of 1 have an exact fp16 hi piece and a zero lo piece under the kernels' power-of-two scales (weights: 1 ->
2^14; image: the round maximum into [2^14, 2^15), a shift of at most 2^5 for a maximum of 1000, more for a smaller one,
the scaled integers always below 2^15 with at most 10 significant bits); exp(0) = 1.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LEVELS = [(4, 16, 32), (8, 32, 16), (16, 64, 8)]   # (C, Cc, S): the canonical flow levels 0, 1, 2
N = 2   # frames: rounds meet at a frame boundary; at 8x8 one round holds both


@pytest.fixture(autouse=True)
def mixed(monkeypatch):
    from rfn_hip import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", "mixed")


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    return ops


def integers(shape, seed):
    """integers in [-1000, 1000] that differ by channel, frame and pixel (a seeded draw, then made nonzero)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-1000, 1001, shape, generator=g)
    return torch.where(v == 0, torch.full_like(v, 7), v).float()


@pytest.mark.parametrize("C,Cc,S", LEVELS)
def test_forward_one_hot_conv1(K, C, Cc, S):
    Ch, Cin = C // 2, C // 2 + Cc
    z, cond = integers((N, C, S, S), 1), integers((N, Cc, S, S), 2)
    x = torch.cat((z[:, :Ch], cond), 1)
    pairs = [(tap, ci) for tap in range(9) for ci in range(Cin)]
    n_launch = (len(pairs) + 255) // 256
    assert n_launch == {18: 1, 36: 2, 72: 3}[Cin]
    w1s = []
    for li in range(n_launch):
        w1 = torch.zeros(256, Cin, 3, 3)
        for co, (tap, ci) in enumerate(pairs[256 * li:256 * (li + 1)]):
            w1[co, ci, tap // 3, tap % 3] = 1.0
        w1s.append(w1)
    zero = torch.zeros(256, device="cuda")
    w2 = torch.zeros(256, 256, 1, 1, device="cuda")
    w3 = torch.zeros(C, 256, 3, 3, device="cuda")
    nets = [(w1.cuda(), w2, w3) for w1 in w1s]
    plan = K.POPackPlan(nets)
    plan.run(bwd=False)
    zc, cc = z.cuda(), cond.cuda()
    for li, w1 in enumerate(w1s):
        h1, h2, P, _ = K.coupling_po_fwd(zc, cc, plan.bufs[li], zero, zero, zero, zero, C, 0)
        ref = F.conv2d(x.double(), w1.double(), padding=1).float()
        got = h1.cpu()
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()[0].tolist()
            co = bad[1]
            pytest.fail("launch %d: h1[%s] = %r, expected %r: (tap, channel) pair %r" % (
                li, bad, float(got[tuple(bad)]), float(ref[tuple(bad)]),
                pairs[256 * li + co] if 256 * li + co < len(pairs) else None))
        assert int(h2.count_nonzero()) == 0 and int(P.count_nonzero()) == 0


@pytest.mark.parametrize("C,Cc,S", LEVELS)
def test_backward_one_hot_conv3_transposed(K, C, Cc, S):
    Cin = C // 2 + Cc
    go = integers((N, C, S, S), 3)
    w3 = torch.zeros(C, 256, 3, 3)
    pairs = [(co, tap) for co in range(C) for tap in range(9)]
    for c2, (co, tap) in enumerate(pairs):
        w3[co, c2, tap // 3, tap % 3] = 1.0
    w1 = torch.zeros(256, Cin, 3, 3, device="cuda")
    w2 = torch.zeros(256, 256, 1, 1, device="cuda")
    plan = K.POPackPlan([(w1, w2, w3.cuda())])
    plan.run(bwd=True)
    zero = torch.zeros(256, device="cuda")
    ga2, ga1, _ = K.coupling_po_bwd(go.cuda(), plan.bwd_bufs[0], zero, zero, None, 0)
    # gradient of conv2d(h2, w3, padding=1) wrt h2: the transposed convolution (go[:, co] shifted by the mirrored tap)
    ref = F.conv_transpose2d(go.double(), w3.double(), padding=1).float()
    got = ga2.cpu()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()[0].tolist()
        pytest.fail("ga2[%s] = %r, expected %r: (co, tap) pair %r" % (
            bad, float(got[tuple(bad)]), float(ref[tuple(bad)]), pairs[bad[1]] if bad[1] < len(pairs) else None))
    assert int(ga1.count_nonzero()) == 0
