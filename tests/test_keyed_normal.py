"""GPU tests of the addressed normal noise (csrc/keyed_normal.hip through rfn_hip.ops.keyed_normal) against the float64
restatement of tests/test_keyed_normal_host.py, and of its addressing: a value depends on (seed, step, slot, sequence,
draw, position) alone, not on how the rows are spread over launches.

Tolerance 1e-5 absolute: the radius is at most 5.77, where one fp32 ulp is 4.8e-7; three correctly implemented fp32
functions (logf, sqrtf, cospif / sinpif) stay within a few ulp, 1e-5 leaves about 5x over that."""
import numpy as np
import pytest
import torch

from tests.test_keyed_normal_host import keyed_normal_ref

pytestmark = pytest.mark.gpu

TOL = 1e-5
SEED = 20261019
BIG = dict(step=70000, first_seq=(1 << 40) + 3, first_draw=1 << 33)   # every 64-bit word of the address is exercised
LENGTHS = (1, 7, 8, 15, 64, 4099)   # below one block, tail blocks, aligned, a long odd row


def _check(outs, numels, B, R, seed, **addr):
    refs = keyed_normal_ref(numels, B, R, seed, addr["step"], addr["first_seq"], addr["first_draw"])
    worst = 0.0
    for j, (o, r) in enumerate(zip(outs, refs)):
        if r is None:
            assert o is None
            continue
        assert o.dtype == torch.float32 and tuple(o.shape)[0] == B * R
        got = o.reshape(B * R, -1).cpu().double().numpy()
        assert got.shape == r.shape
        err = float(np.abs(got - r).max())
        worst = max(worst, err)
        assert err <= TOL, (j, numels[j], err)
    return worst


@pytest.mark.parametrize("B,R", [(1, 1), (3, 2), (2, 5)])
def test_kernel_matches_the_restatement(B, R):
    from rfn_hip import ops
    worst = 0.0
    for n in LENGTHS:                                     # one slot
        outs = ops.keyed_normal([(n,)], B, R, SEED, device="cuda", **BIG)
        worst = max(worst, _check(outs, [n], B, R, SEED, **BIG))
    outs = ops.keyed_normal([(15,), (2, 4, 8)], B, R, SEED, device="cuda", **BIG)    # two slots, mixed lengths
    assert tuple(outs[1].shape) == (B * R, 2, 4, 8)
    worst = max(worst, _check(outs, [15, 64], B, R, SEED, **BIG))
    shapes = [(1,), (7,), (8,), (15,), (64,), (4099,), (3, 3), (2, 2, 4)]               # eight slots
    outs = ops.keyed_normal(shapes, B, R, SEED, device="cuda", **BIG)
    worst = max(worst, _check(outs, [1, 7, 8, 15, 64, 4099, 9, 16], B, R, SEED, **BIG))
    outs = ops.keyed_normal([(8,), None, (24,)], B, R, 5, 3, device="cuda")            # a skipped slot, small address
    worst = max(worst, _check(outs, [8, None, 24], B, R, 5, step=3, first_seq=0, first_draw=0))
    print("B=%d R=%d max |kernel - float64 restatement| = %.3e" % (B, R, worst))


def test_unaligned_rows_take_the_scalar_path():
    """a view whose base is 4-byte but not 16-byte aligned, row length a multiple of 8: single stores, same values, and
    nothing outside the view is written"""
    from rfn_hip import ops
    B, R, n = 3, 2, 64
    buf = torch.full((B * R * n + 8,), 7.0, device="cuda")
    for off in (1, 2, 3):
        buf.fill_(7.0)
        view = buf[off:off + B * R * n].view(B * R, n)
        assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
        outs = ops.keyed_normal(None, B, R, SEED, out=[view], **BIG)
        assert outs[0] is view
        _check(outs, [n], B, R, SEED, **BIG)
        aligned = ops.keyed_normal([(n,)], B, R, SEED, device="cuda", **BIG)[0]
        assert torch.equal(view, aligned)
        assert bool((buf[:off] == 7.0).all()) and bool((buf[off + B * R * n:] == 7.0).all())


def test_addressing_is_independent_of_the_launch():
    """(B=3, R=2) in one launch == six launches of (B=1, R=1) at the matching first_seq / first_draw, bit for bit, ==
    a launch into out= views"""
    from rfn_hip import ops
    B, R = 3, 2
    shapes = [(4099,), (2, 4, 8), (7,)]
    kw = dict(BIG)
    whole = ops.keyed_normal(shapes, B, R, SEED, device="cuda", **kw)
    for r in range(R):
        for b in range(B):
            one = ops.keyed_normal(shapes, 1, 1, SEED, kw["step"], first_seq=kw["first_seq"] + b,
                                   first_draw=kw["first_draw"] + r, device="cuda")
            for w, o in zip(whole, one):
                assert torch.equal(w[r * B + b], o[0]), (r, b)
    # other batch splits: B=1 with all draws, and all sequences with one draw
    for b in range(B):
        part = ops.keyed_normal(shapes, 1, R, SEED, kw["step"], kw["first_seq"] + b, kw["first_draw"], device="cuda")
        for w, o in zip(whole, part):
            assert torch.equal(w[b::B], o)
    # out= views into one buffer (16-byte aligned here: the vector path where the length allows)
    sizes = [B * R * 4099, B * R * 64, B * R * 7]
    buf = torch.zeros(sum(sizes) + 64, device="cuda")
    views, at = [], 0
    for sh, sz in zip(shapes, sizes):
        views.append(buf[at:at + sz].view((B * R,) + sh))
        at += (sz + 3) // 4 * 4
    outs = ops.keyed_normal(shapes, B, R, SEED, out=views, **kw)
    for v, o, w in zip(views, outs, whole):
        assert o is v and torch.equal(v, w)
    # a different seed, step or slot gives different numbers
    other = ops.keyed_normal(shapes, B, R, SEED + 1, device="cuda", **kw)
    assert not torch.equal(other[0], whole[0])
    assert not torch.equal(whole[0][:, :7], whole[2])
