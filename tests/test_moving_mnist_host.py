"""CPU tests of Stochastic Moving MNIST (data_generators/moving_mnist.py, csrc/moving_mnist.hip): the MNIST readers on
files written in torchvision's layouts, the addressed random draws restated in Python against numpy's Philox, the walk
restatement's invariants, and the Solver's data-loader errors.  The restatement below (philox4x64_10, draw_below,
walk, render) is the definition the GPU kernel is compared with in tests/test_moving_mnist.py."""
import gzip
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

M64 = (1 << 64) - 1
PHILOX_M = (0xD2E7470EE14C6C93, 0xCA5A826395121157)
PHILOX_W = (0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B)
D = 28


# ---------------------------------------------------------------------------------------------- the restatement
def philox4x64_10(ctr, key):
    """the Philox4x64-10 block of a 4-word counter under a 2-word key (Salmon et al. 2011; numpy's np.random.Philox)"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M[0] * c0, PHILOX_M[1] * c2
        c0, c1, c2, c3 = ((p1 >> 64) ^ c1 ^ k0) & M64, p1 & M64, ((p0 >> 64) ^ c3 ^ k1) & M64, p0 & M64
        k0, k1 = (k0 + PHILOX_W[0]) & M64, (k1 + PHILOX_W[1]) & M64
    return c0, c1, c2, c3


def lemire(x, r):
    """Lemire's multiply-shift of a 64-bit word onto [0, r): the value, or None when the word is rejected"""
    m = x * r
    lo = m & M64
    if lo < r and lo < ((1 << 64) - r) % r:
        return None
    return m >> 64


class Draws:
    """the random draws of digit n of sequence `seq`: draw j uses word 0 of the block at counter (j, retry, seq, n) under
    key (seed, split); a rejected word advances retry"""

    def __init__(self, seed, split, seq, n):
        self.key, self.seq, self.n, self.j = (seed, split), seq, n, 0

    def below(self, r):
        retry = 0
        while True:
            v = lemire(philox4x64_10((self.j, retry, self.seq, self.n), self.key)[0], r)
            if v is not None:
                self.j += 1
                return v
            retry += 1

    def randint(self, lo, hi):   # numpy's randint(lo, hi): [lo, hi)
        return lo + self.below(hi - lo)


def walk(seed, split, seq, n, N, S, L, T, deterministic, events=None):
    """stochasticMovingMnist.py:73-111 for digit n: [(digit index, y, x)] per frame.  `events` (a list) receives
    (t, kind, sy, sx, dy, dx) after the bounce handling of every step, kind in {None, 'top', 'bottom', 'left', 'right'}
    (the last bounce of the step)."""
    d = Draws(seed, split, seq, n)
    R = S - D
    idx = d.randint(0, N)
    sx = d.randint(0, R)
    sy = d.randint(0, R)
    dx = d.randint(-L, L + 1)
    dy = d.randint(-L, L + 1)
    out = []
    for t in range(T):
        kind = None
        if sy < 0:
            sy, kind = 0, "top"
            if deterministic:
                dy = -dy
            else:
                dy = d.randint(1, L + 1)
                dx = d.randint(-L, L + 1)
        elif sy >= R:
            sy, kind = R - 1, "bottom"
            if deterministic:
                dy = -dy
            else:
                dy = d.randint(-L, 0)
                dx = d.randint(-L, L + 1)
        if sx < 0:
            sx, kind = 0, "left"
            if deterministic:
                dx = -dx
            else:
                dx = d.randint(1, L + 1)
                dy = d.randint(-L, L + 1)
        elif sx >= R:
            sx, kind = R - 1, "right"
            if deterministic:
                dx = -dx
            else:
                dx = d.randint(-L, 0)
                dy = d.randint(-L, L + 1)
        if events is not None:
            events.append((t, kind, sy, sx, dy, dx))
        out.append((idx, sy, sx))
        sy += dy
        sx += dx
    return out


def tensor_lut():
    """ToTensor's byte -> float32: k / 255 in float32"""
    return np.arange(256, dtype=np.float32) / np.float32(255)


def render(digits, B, T, C, S, nd, L, deterministic, seed, split, first_id):
    """the reference's MovingMNIST.__getitem__ (float32 sums in digit order, x[x > 1] = 1, channel copies) on the
    addressed walk: (frames float32 [B, T, C, S, S], trajectories int64 [B, nd, T, 3])"""
    digits = np.asarray(digits)
    lut = tensor_lut()
    N = digits.shape[0]
    x = np.zeros((B, T, S, S), dtype=np.float32)
    traj = np.zeros((B, nd, T, 3), dtype=np.int64)
    for b in range(B):
        for n in range(nd):
            w = walk(seed, split, first_id + b, n, N, S, L, T, deterministic)
            traj[b, n] = w
            glyph = lut[digits[w[0][0]]]
            for t, (_, sy, sx) in enumerate(w):
                x[b, t, sy:sy + D, sx:sx + D] += glyph
    x[x > 1] = 1.0
    return np.repeat(x[:, :, None], C, axis=2), traj


# ---------------------------------------------------------------------------------------------- fixtures on disk
def idx_bytes(images):
    images = np.asarray(images, dtype=np.uint8)
    n, h, w = images.shape
    return (2051).to_bytes(4, "big") + n.to_bytes(4, "big") + h.to_bytes(4, "big") + w.to_bytes(4, "big") + \
        images.tobytes()


def write_mnist(root, train_images, test_images, layout="raw"):
    """MNIST files as torchvision leaves them under `root`: layout 'raw' (idx), 'gz' (idx.gz) or 'processed' (.pt)"""
    for train, imgs in ((True, train_images), (False, test_images)):
        if layout == "processed":
            d = os.path.join(root, "MNIST", "processed")
            os.makedirs(d, exist_ok=True)
            data = torch.as_tensor(np.asarray(imgs, dtype=np.uint8))
            torch.save((data, torch.zeros(data.shape[0], dtype=torch.int64)),
                       os.path.join(d, "training.pt" if train else "test.pt"))
            continue
        d = os.path.join(root, "MNIST", "raw")
        os.makedirs(d, exist_ok=True)
        name = os.path.join(d, ("train" if train else "t10k") + "-images-idx3-ubyte")
        if layout == "gz":
            with gzip.open(name + ".gz", "wb") as f:
                f.write(idx_bytes(imgs))
        else:
            with open(name, "wb") as f:
                f.write(idx_bytes(imgs))


def fixture_digits(n, seed):
    """uint8 [n, 28, 28]: every byte value occurs, and half the digits are built from values whose pairwise float32 sums
    land just below, at and just above 1 (k1 + k2 = 254, 255, 256), so that overlaps exercise the rounding and the clip"""
    g = np.random.RandomState(seed)
    out = g.randint(0, 256, size=(n, D, D)).astype(np.uint8)
    out[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    edge = np.array([0, 1, 100, 127, 128, 154, 155, 156, 254, 255], dtype=np.uint8)
    out[1::2] = edge[g.randint(0, len(edge), size=out[1::2].shape)]
    return out


# ---------------------------------------------------------------------------------------------- readers
def test_readers_agree_across_layouts(tmp_path):
    from data_generators import load_mnist_digits
    tr, te = fixture_digits(9, 1), fixture_digits(4, 2)
    got = {}
    for layout in ("raw", "gz", "processed"):
        root = str(tmp_path / layout)
        write_mnist(root, tr, te, layout)
        got[layout] = (load_mnist_digits(root, True), load_mnist_digits(root, False))
    for a, b in got.values():
        assert a.dtype == torch.uint8 and tuple(a.shape) == (9, 28, 28) and tuple(b.shape) == (4, 28, 28)
        assert torch.equal(a, torch.from_numpy(tr)) and torch.equal(b, torch.from_numpy(te))


def test_reader_missing_files_names_paths(tmp_path):
    from data_generators import load_mnist_digits
    from data_generators.moving_mnist import mnist_candidate_paths
    with pytest.raises(FileNotFoundError) as e:
        load_mnist_digits(str(tmp_path), True)
    msg = str(e.value)
    assert "No download is attempted" in msg
    for p in mnist_candidate_paths(str(tmp_path), True):
        assert p in msg
    assert "t10k-images-idx3-ubyte" in " ".join(mnist_candidate_paths(str(tmp_path), False))


@pytest.mark.parametrize("gz", [False, True])
def test_reader_rejects_bad_files(tmp_path, gz):
    from data_generators import load_mnist_digits
    good = idx_bytes(fixture_digits(3, 4))
    d = tmp_path / "MNIST" / "raw"
    d.mkdir(parents=True)
    name = str(d / "train-images-idx3-ubyte") + (".gz" if gz else "")

    def put(raw):
        if gz:
            with gzip.open(name, "wb") as f:
                f.write(raw)
        else:
            with open(name, "wb") as f:
                f.write(raw)
    put(good[:-5])
    with pytest.raises(ValueError, match="truncated"):
        load_mnist_digits(str(tmp_path), True)
    put(good[:10])
    with pytest.raises(ValueError, match="truncated"):
        load_mnist_digits(str(tmp_path), True)
    put((2049).to_bytes(4, "big") + good[4:])
    with pytest.raises(ValueError, match="magic"):
        load_mnist_digits(str(tmp_path), True)
    put(good[:8] + (32).to_bytes(4, "big") + good[12:])
    with pytest.raises(ValueError):
        load_mnist_digits(str(tmp_path), True)
    put(good)
    assert tuple(load_mnist_digits(str(tmp_path), True).shape) == (3, 28, 28)


def test_reader_rejects_bad_processed_file(tmp_path):
    from data_generators import load_mnist_digits
    d = tmp_path / "MNIST" / "processed"
    d.mkdir(parents=True)
    torch.save((torch.zeros(2, 27, 28, dtype=torch.uint8), torch.zeros(2)), str(d / "test.pt"))
    with pytest.raises(ValueError, match="uint8"):
        load_mnist_digits(str(tmp_path), False)


# ---------------------------------------------------------------------------------------------- generator restatement
def _numpy_block(ctr, key):
    """numpy increments the 256-bit counter before it generates: the block of counter c is
    Philox(counter=c - 1, key=k).random_raw(4)"""
    c = sum(w << (64 * i) for i, w in enumerate(ctr))
    c = (c - 1) % (1 << 256)
    words = np.array([(c >> (64 * i)) & M64 for i in range(4)], dtype=np.uint64)
    bg = np.random.Philox(counter=words, key=np.array(key, dtype=np.uint64))
    return tuple(int(v) for v in bg.random_raw(4))


def test_philox_matches_numpy():
    g = np.random.RandomState(0)
    cases = [((0, 0, 0, 0), (0, 0)), ((1, 0, 0, 0), (0, 0)), ((0, 1, 0, 0), (0, 1)), ((M64, M64, M64, M64), (M64, M64)),
             ((0, 0, 12345, 2), (7, 1)), ((3, 1, 1 << 40, 7), (1 << 62, 0))]
    for _ in range(20):
        cases.append((tuple(int(v) for v in g.randint(0, 2 ** 63, size=4, dtype=np.int64)),
                      tuple(int(v) for v in g.randint(0, 2 ** 63, size=2, dtype=np.int64))))
    for ctr, key in cases:
        assert philox4x64_10(ctr, key) == _numpy_block(ctr, key), (ctr, key)


def test_bounded_draws():
    # draws are word 0 of the addressed block, mapped by the multiply-shift
    d = Draws(5, 1, 77, 2)
    for j, r in enumerate((60000, 36, 36, 9, 9, 4, 9, 1)):
        x = _numpy_block((j, 0, 77, 2), (5, 1))[0]
        assert d.below(r) == (x * r) >> 64 and d.j == j + 1
    # the rejection zone: low64(x * r) < 2^64 mod r
    assert lemire(0, 3) is None and lemire(1, 3) == 0 and lemire(M64, 3) == 2
    assert lemire(0, 1) == 0            # r = 1 never rejects
    r = 10
    zone = ((1 << 64) - r) % r          # = 6: words with low64(x * 10) < 6 are rejected
    assert zone == 6 and lemire(0, r) is None and lemire(1, r) == 0
    # a rejected word moves to retry + 1 of the same draw number
    calls = []
    real = philox4x64_10

    def fake(ctr, key):
        calls.append(ctr)
        return (0, 0, 0, 0) if ctr[1] == 0 else real(ctr, key)
    globals()["philox4x64_10"] = fake
    try:
        d = Draws(1, 0, 3, 0)
        v = d.below(3)
    finally:
        globals()["philox4x64_10"] = real
    assert calls == [(0, 0, 3, 0), (0, 1, 3, 0)] and d.j == 1
    assert v == (real((0, 1, 3, 0), (1, 0))[0] * 3) >> 64
    # uniform enough: every value of a small range occurs
    d = Draws(0, 0, 0, 0)
    seen = {d.randint(-4, 5) for _ in range(300)}
    assert seen == set(range(-4, 5))


# ---------------------------------------------------------------------------------------------- walk properties
@pytest.mark.parametrize("S,L", [(29, 1), (29, 4), (32, 4), (40, 8), (64, 4)])
def test_walk_stays_in_frame_and_velocities_in_range(S, L):
    R = S - D
    kinds = set()
    for seq in range(40):
        for n in range(2):
            ev = []
            traj = walk(11, 0, seq, n, 1000, S, L, 20, False, events=ev)
            assert 0 <= traj[0][0] < 1000 and len({t[0] for t in traj}) == 1
            for (t, kind, sy, sx, dy, dx), (_, ty, tx) in zip(ev, traj):
                assert (sy, sx) == (ty, tx)
                assert 0 <= sy <= R - 1 and 0 <= sx <= R - 1
                assert -L <= dy <= L and -L <= dx <= L
                kinds.add(kind)
                if kind == "top":
                    assert 1 <= dy <= L
                elif kind == "bottom":
                    assert -L <= dy <= -1
                elif kind == "left":
                    assert 1 <= dx <= L
                elif kind == "right":
                    assert -L <= dx <= -1
    assert kinds >= {None, "top", "bottom", "left", "right"} or S == 64


def test_walk_deterministic_reflects():
    for S, L in ((29, 3), (33, 4), (64, 4)):
        R = S - D
        for seq in range(30):
            ev = []
            walk(2, 1, seq, 0, 10, S, L, 30, True, events=ev)
            _, _, _, _, dy0, dx0 = ev[0]
            for (t, kind, sy, sx, dy, dx), prev in zip(ev[1:], ev[:-1]):
                assert 0 <= sy <= R - 1 and 0 <= sx <= R - 1
                # speeds never change; a wall flips the sign of the component that hit it
                assert abs(dy) == abs(dy0) and abs(dx) == abs(dx0)
                if dy != prev[4]:
                    assert prev[2] + prev[4] < 0 or prev[2] + prev[4] >= R
                if dx != prev[5]:
                    assert prev[3] + prev[5] < 0 or prev[3] + prev[5] >= R


def test_render_restatement_contract():
    digits = fixture_digits(6, 3)
    x, traj = render(digits, 2, 5, 3, 32, 2, 4, False, 0, 0, 0)
    assert x.dtype == np.float32 and x.shape == (2, 5, 3, 32, 32) and traj.shape == (2, 2, 5, 3)
    assert x.min() >= 0 and x.max() == 1.0
    assert (x[:, :, 0] == x[:, :, 1]).all() and (x[:, :, 0] == x[:, :, 2]).all()
    # float32 k / 255 is ToTensor's value
    assert torch.equal(torch.from_numpy(tensor_lut()), torch.arange(256, dtype=torch.uint8).float().div(255))


# ---------------------------------------------------------------------------------------------- Solver wiring
def _solver_argv(extra):
    return ("--extractor_structure 4-pool-8 8-pool-16 --upscaler_structure 16 upsample-8-8 --prior_structure 12 12 "
            "--encoder_structure 12 12 --z_dim 4 --h_dim 8 --n_units_affine 16 --n_units_prior 16 --K 2 --L 2 "
            "--n_frames 4 --image_size 32 --digit_size 28 --num_digits 2 --x_dim 2 1 32 32 --condition_dim 2 1 32 32 "
            "--batch_size 2 --num_workers 0 --skip_connection_flow without_skip --no-upscaler_tanh "
            "--no-downscaler_tanh " + extra).split()


def test_solver_mnist_without_files_raises_reader_error(tmp_path):
    import main_rfn
    from RFN.trainer import Solver
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv("--choose_data mnist --mnist_root %s --path %s" %
                                                           (tmp_path / "empty", rel)))
    assert args.data_seed == 0 and not args.synthetic_data
    with pytest.raises(FileNotFoundError, match="No download is attempted"):
        Solver(args).build()
    # the default root is the reference's `Mnist`, relative to the working directory
    assert main_rfn.build_parser().parse_args(_solver_argv("--choose_data mnist")).mnist_root == "Mnist"


def test_solver_bair_kth_without_synthetic_still_raise(tmp_path):
    import main_rfn
    from RFN.trainer import Solver
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    for data in ("bair", "kth"):
        args = main_rfn.build_parser().parse_args(_solver_argv("--choose_data %s --path %s" % (data, rel)))
        with pytest.raises(RuntimeError, match="--synthetic_data"):
            Solver(args).build()


def test_create_loaders_reads_old_args(tmp_path):
    """Namespaces saved before --mnist_root / --data_seed existed (and the reference's own) still build loaders"""
    from RFN.trainer import Solver
    import main_rfn
    write_mnist(str(tmp_path / "Mnist"), fixture_digits(10, 5), fixture_digits(6, 6))
    args = main_rfn.build_parser().parse_args(_solver_argv("--choose_data mnist"))
    del args.mnist_root, args.data_seed
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        s = Solver(args)
        tr, te = s.create_loaders()
    finally:
        os.chdir(cwd)
    assert len(tr) == 10 // 2 and len(te) == 6 // 2
    assert tr.dataset.seed == 0 and tr.dataset.split != te.dataset.split
    assert tr.dataset.channels == 1 and tr.dataset.image_size == 32 and not tr.dataset.deterministic
    args.use_validation_set = True
    s = Solver(Namespace(**vars(args)))
    s.args.mnist_root = str(tmp_path / "Mnist")
    tr, _ = s.create_loaders()
    assert len(tr.dataset) == 500 and len(tr) == 250


def test_generator_limits(tmp_path):
    from data_generators import MovingMNIST
    write_mnist(str(tmp_path), fixture_digits(4, 7), fixture_digits(4, 8))
    ok = dict(train=True, data_root=str(tmp_path), image_size=32)
    MovingMNIST(**ok)
    for bad, exc in ((dict(digit_size=32), ValueError), (dict(image_size=28), ValueError),
                     (dict(num_digits=0), ValueError), (dict(num_digits=9), ValueError),
                     (dict(step_length=0), ValueError), (dict(normalize=True), NotImplementedError),
                     (dict(make_target=True), NotImplementedError),
                     (dict(set_starting_position=True), NotImplementedError)):
        with pytest.raises(exc):
            MovingMNIST(**dict(ok, **bad))
