"""CPU tests of the addressed normal noise (csrc/keyed_normal.hip, rfn_hip.ops.keyed_normal) and of the Evaluator's
draws_per_pass setting.  The numpy restatement below (philox4x64_10_blocks, keyed_normal_ref) is the definition the GPU
kernel is compared with in tests/test_keyed_normal.py: Philox4x64-10 checked against numpy's np.random.Philox, and the
Box-Muller transformation in float64."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_moving_mnist_host import M64, PHILOX_M, PHILOX_W, _numpy_block

U64 = np.uint64
LO32 = U64(0xffffffff)
S32 = U64(32)


# ---------------------------------------------------------------------------------------------- the restatement
def _mulhilo(m, x):
    """(high, low) 64-bit words of the 128-bit product of the constant m and the uint64 array x"""
    m0, m1 = U64(m & 0xffffffff), U64(m >> 32)
    x0, x1 = x & LO32, x >> S32
    ll, lh, hl, hh = m0 * x0, m0 * x1, m1 * x0, m1 * x1
    mid = (ll >> S32) + (lh & LO32) + (hl & LO32)
    lo = (ll & LO32) | ((mid & LO32) << S32)
    hi = hh + (lh >> S32) + (hl >> S32) + (mid >> S32)
    return hi, lo


def philox4x64_10_blocks(c0, c1, c2, c3, key):
    """Philox4x64-10 of many counters at once: four uint64 arrays (words w0..w3) from four counter-word arrays (or
    scalars) under one 2-word key.  Its own copy of the rounds, vectorised; checked against np.random.Philox below."""
    c0, c1, c2, c3 = (np.asarray(np.broadcast_arrays(*[np.asarray(c, dtype=U64) for c in (c0, c1, c2, c3)])[i]).copy()
                      for i in range(4))
    k0, k1 = int(key[0]) & M64, int(key[1]) & M64
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(PHILOX_M[0], c0)
            hi1, lo1 = _mulhilo(PHILOX_M[1], c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ U64(k0), lo1, hi0 ^ c3 ^ U64(k1), lo0
            k0, k1 = (k0 + PHILOX_W[0]) & M64, (k1 + PHILOX_W[1]) & M64
    return c0, c1, c2, c3


def keyed_normal_row(numel, seed, step, slot, seq, draw):
    """one row of `numel` values in float64: block q = Philox(key = (seed, (step << 32) | slot), counter = (q, 0, seq,
    draw)); word w_i gives elements 8q + 2i, 8q + 2i + 1: a = w >> 32, b = w & 0xffffffff, u1 = ((a >> 8) + 1) 2^-24,
    u2 = (b >> 8) 2^-24, rad = sqrt(-2 ln u1), values rad cos(2 pi u2), rad sin(2 pi u2)"""
    nblk = (numel + 7) // 8
    q = np.arange(nblk, dtype=U64)
    words = philox4x64_10_blocks(q, 0, int(seq), int(draw), (int(seed), (int(step) << 32) | int(slot)))
    w = np.stack(words, axis=1)                                  # [nblk, 4]
    a, b = w >> S32, w & LO32
    u1 = ((a >> U64(8)) + U64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (b >> U64(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    out = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2)   # [nblk, 4, 2]
    return out.reshape(-1)[:numel]


def keyed_normal_ref(numels, B, n_draws, seed, step, first_seq=0, first_draw=0):
    """float64 arrays [n_draws*B, numel_j], slot j the list position (None skips a slot): row r*B + b is draw
    first_draw + r of sequence first_seq + b"""
    outs = []
    for j, n in enumerate(numels):
        if n is None:
            outs.append(None)
            continue
        rows = [keyed_normal_row(n, seed, step, j, first_seq + b, first_draw + r)
                for r in range(n_draws) for b in range(B)]
        outs.append(np.stack(rows) if rows else np.zeros((0, n)))
    return outs


# ---------------------------------------------------------------------------------------------- tests
def test_vectorised_philox_matches_numpy():
    g = np.random.RandomState(1)
    cases = [((0, 0, 0, 0), (0, 0)), ((M64, M64, M64, M64), (M64, M64)), ((5, 0, (1 << 40) + 3, 1 << 33), (20261019, (70000 << 32) | 7))]
    for _ in range(12):
        cases.append((tuple(int(v) for v in g.randint(0, 2 ** 63, size=4, dtype=np.int64)),
                      tuple(int(v) for v in g.randint(0, 2 ** 63, size=2, dtype=np.int64))))
    for ctr, key in cases:
        got = philox4x64_10_blocks(*ctr, key)
        assert tuple(int(np.asarray(w).reshape(-1)[0]) for w in got) == _numpy_block(ctr, key), (ctr, key)
    # a run of blocks: counter word 0 counts the blocks of a row
    key, seq, draw = (20261019, (3 << 32) | 2), 11, 4
    w = philox4x64_10_blocks(np.arange(40, dtype=U64), 0, seq, draw, key)
    for q in (0, 1, 39):
        assert tuple(int(x[q]) for x in w) == _numpy_block((q, 0, seq, draw), key)


def test_restatement_moments():
    """seed 20261019, one row of 2^20 values: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n), max |value| <= 5.77"""
    n = 1 << 20
    v = keyed_normal_row(n, 20261019, 0, 0, 0, 0)
    assert v.shape == (n,) and np.isfinite(v).all()
    mean, var, big = float(v.mean()), float(v.var()), float(np.abs(v).max())
    print("mean %.3e var-1 %.3e max %.3f" % (mean, var - 1.0, big))
    assert abs(mean) <= 5.0 / np.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert big <= 5.77


def test_restatement_addresses():
    """every coordinate of the address changes the values; a prefix of a longer row is the shorter row"""
    base = keyed_normal_row(24, 1, 2, 3, 4, 5)
    assert np.array_equal(base[:15], keyed_normal_row(15, 1, 2, 3, 4, 5))
    for other in ((2, 2, 3, 4, 5), (1, 3, 3, 4, 5), (1, 2, 4, 4, 5), (1, 2, 3, 5, 5), (1, 2, 3, 4, 6)):
        assert not np.array_equal(base, keyed_normal_row(24, *other))
    a, b = keyed_normal_ref([8, None, 5], 3, 2, 9, 1, first_seq=7, first_draw=2)[::2]
    assert a.shape == (6, 8) and b.shape == (6, 5)
    assert np.array_equal(a[1 * 3 + 2], keyed_normal_row(8, 9, 1, 0, 9, 3))
    assert np.array_equal(b[0 * 3 + 1], keyed_normal_row(5, 9, 1, 2, 8, 2))


def test_keyed_normal_refuses_bad_arguments():
    from rfn_hip import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.keyed_normal([(4,)], 1, 1, 0, 0, device="cpu")
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.keyed_normal(None, 1, 1, 0, 0, out=[torch.zeros(1, 4)])
    with pytest.raises(ValueError, match="rows"):
        ops.keyed_normal(None, 2, 1, 0, 0, out=[torch.zeros(1, 4)])
    with pytest.raises(ValueError, match="slots"):
        ops.keyed_normal(None, 1, 1, 0, 0, out=[torch.zeros(1, 4)] * 9)
    with pytest.raises(ValueError, match="seed"):
        ops.keyed_normal([(4,)], 1, 1, -1, 0, device="cuda")
    with pytest.raises(ValueError, match="step"):
        ops.keyed_normal([(4,)], 1, 1, 0, 1 << 31, device="cuda")
    with pytest.raises(TypeError, match="shapes or out"):
        ops.keyed_normal(None, 1, 1, 0, 0)


class _StubModel(object):
    """records the generation calls of the Evaluator; frames are zeros on the CPU"""

    class Stop(Exception):
        pass

    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def predict(self, image, n_predictions, n_conditions):
        self.calls.append(("predict", n_predictions, n_conditions))
        return image[:, :n_conditions].transpose(0, 1), torch.zeros((n_predictions, image.shape[0]) + tuple(image.shape[2:]))

    def loss(self, x, logdet=0):
        self.calls.append(("loss", tuple(x.shape)))
        return torch.tensor(0.0), torch.tensor(1.0), torch.tensor(2.0)

    def _predict_draws_device(self, image, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0):
        self.calls.append(("draws", n_predictions, n_conditions, n_draws, seed, first_seq, first_draw))
        raise self.Stop()   # what follows scores frames on the GPU


def _stub_evaluator(**settings):
    from evaluation_metrics import Evaluator
    model = _StubModel()
    solver = SimpleNamespace(model=model, args=SimpleNamespace(n_frames=4, n_conditions=2, batch_size=2),
                             device=torch.device("cpu"),
                             preprocess=lambda x, reverse=False: (x * 255).byte() if reverse else x)
    ev = Evaluator(solver, settings=SimpleNamespace(**settings))
    scores = lambda gt, pred: tuple(torch.zeros(gt.shape[:2]) for _ in range(3))
    ev.eval_seq = scores
    return ev, model


def test_draws_per_pass_unset_takes_the_sequential_path():
    batches = [torch.zeros(2, 6, 1, 16, 16) for _ in range(2)]
    ev, model = _stub_evaluator(n_frames=6, start_predictions=2, resample=3)
    assert ev.draws_per_pass is None and ev.seed == 0
    out = ev.get_eval_values("rfn.pt", loader=batches)
    assert [c[0] for c in model.calls] == ["predict", "loss"] * 6
    assert model.calls[0] == ("predict", 4, 2)
    assert tuple(out[0].shape) == (4, 4) and out[3] is None


def test_draws_per_pass_set_takes_the_batched_path():
    batches = [torch.zeros(2, 6, 1, 16, 16) for _ in range(2)]
    ev, model = _stub_evaluator(n_frames=6, start_predictions=2, resample=3, draws_per_pass=2, seed=17)
    assert ev.draws_per_pass == 2 and ev.seed == 17
    with pytest.raises(_StubModel.Stop):
        ev.get_eval_values("rfn.pt", loader=batches)
    assert model.calls == [("draws", 4, 2, 2, 17, 0, 0)]   # no predict, no loss before the passes
    ev, model = _stub_evaluator(n_frames=6, start_predictions=2, resample=3, draws_per_pass=0)
    with pytest.raises(ValueError, match="draws_per_pass"):
        ev.get_eval_values("rfn.pt", loader=batches)
