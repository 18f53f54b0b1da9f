"""The Python / numpy restatement of the synchronized Moving MNIST (MovingMNIST_synchronized of the reference,
data_generators/stochasticMovingMnist.py:131-248) on the addressed draws of tests/test_moving_mnist_host.py: the
definition rfn_moving_mnist_sync_render_f32 is compared with, bit for bit."""
import numpy as np

from tests.test_moving_mnist_host import D, M64, Draws, tensor_lut

SHARED_SEQ = M64   # counter word 2 of every draw the sequences share: 2^64 - 1, which no sequence id equals


def sync_walk(seed, split, seq, n, N, S, L, T, deterministic, addresses=None):
    """digit n of sequence `seq`: ([(digit index, y, x)] per frame, [clamped at a wall on frame t]).  idx is draw 0 at
    the plain address (0, retry, seq, n); sx, sy and the bounce redraws are draws 1, 2, 3, ... at (j, retry, 2^64 - 1,
    n); dx = dy = 3 whatever L is.  `addresses` (a list) receives (sequence word, draw number) of every draw made."""
    own, d = Draws(seed, split, seq, n), Draws(seed, split, SHARED_SEQ, n)
    d.j = 1

    def randint(src, lo, hi):
        if addresses is not None:
            addresses.append((src.seq, src.j))
        return src.randint(lo, hi)
    R = S - D
    idx = randint(own, 0, N)
    sx = randint(d, 0, R)
    sy = randint(d, 0, R)
    dx = dy = 3
    out, hits = [], []
    for t in range(T):
        hit = False
        if sy < 0:
            sy, hit = 0, True
            if deterministic:
                dy = -dy
            else:
                dy = randint(d, 1, L + 1)
                dx = randint(d, -L, L + 1)
        elif sy >= R:
            sy, hit = R - 1, True
            if deterministic:
                dy = -dy
            else:
                dy = randint(d, -L, 0)
                dx = randint(d, -L, L + 1)
        if sx < 0:
            sx, hit = 0, True
            if deterministic:
                dx = -dx
            else:
                dx = randint(d, 1, L + 1)
                dy = randint(d, -L, L + 1)
        elif sx >= R:
            sx, hit = R - 1, True
            if deterministic:
                dx = -dx
            else:
                dx = randint(d, -L, 0)
                dy = randint(d, -L, L + 1)
        out.append((idx, sy, sx))
        hits.append(hit)
        sy += dy
        sx += dx
    return out, hits


def sync_hit(seed, split, nd, S, L, T, deterministic):
    """hit_boundary as int64 [T]: the reference overwrites entry t with n + 1 in digit order, so the last clamped digit
    wins; 0 where no digit was clamped.  It does not depend on the sequence."""
    hit = np.zeros(T, dtype=np.int64)
    for n in range(nd):
        _, hits = sync_walk(seed, split, 0, n, 1, S, L, T, deterministic)
        for t, h in enumerate(hits):
            if h:
                hit[t] = n + 1
    return hit


def sync_render(digits, B, T, C, S, nd, L, deterministic, seed, split, first_id):
    """(frames float32 [B, T, C, S, S], trajectories int64 [B, nd, T, 3], hit int32 [B, T]): the float32 pixel pipeline
    of tests/test_moving_mnist_host.render on the synchronized walk"""
    digits = np.asarray(digits)
    lut = tensor_lut()
    N = digits.shape[0]
    x = np.zeros((B, T, S, S), dtype=np.float32)
    traj = np.zeros((B, nd, T, 3), dtype=np.int64)
    for b in range(B):
        for n in range(nd):
            w, _ = sync_walk(seed, split, first_id + b, n, N, S, L, T, deterministic)
            traj[b, n] = w
            glyph = lut[digits[w[0][0]]]
            for t, (_, sy, sx) in enumerate(w):
                x[b, t, sy:sy + D, sx:sx + D] += glyph
    x[x > 1] = 1.0
    hit = np.repeat(sync_hit(seed, split, nd, S, L, T, deterministic)[None], B, axis=0).astype(np.int32)
    return np.repeat(x[:, :, None], C, axis=2), traj, hit
