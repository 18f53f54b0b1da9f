"""CPU tests of the file-backed datasets (data_generators/clips.py, bair_push.py, kth.py): the Torch7 reader on byte
strings assembled here, BAIR and KTH trees written into tmp_path, the addressed clip draws against a restatement on
tests/test_moving_mnist_host.py's philox4x64_10 / lemire, the store cache, and the Solver's wiring.  The helpers
(t7_bytes, write_bair_tree, write_kth_tree, expected_*_table) also serve tests/test_clip_gather.py."""
import os
import re
import struct
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.test_moving_mnist_host import M64, _solver_argv, lemire, philox4x64_10

CLASSES = ['boxing', 'handclapping', 'handwaving', 'jogging', 'running', 'walking']


# ---------------------------------------------------------------------------------------------- the restatement
def randint_at(key, draw, seq, lo, hi):
    """numpy's randint(lo, hi) as an addressed draw: block (draw, retry, seq, 0) under `key`, word 0, Lemire"""
    retry = 0
    while True:
        v = lemire(philox4x64_10((draw, retry, seq, 0), key)[0], hi - lo)
        if v is not None:
            return lo + v
        retry += 1


def expected_permutation(seed, split, n, epoch):
    perm = list(range(n))
    for i in range(n - 1, 0, -1):
        j = randint_at((seed, 2 + split), i, epoch, 0, i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def expected_bair_table(offset, length, T, seed, train, epoch, n=None):
    """(examples, first frames) of an epoch of PushDataset"""
    n = len(offset) if n is None else n
    if not train:
        return list(range(n)), [int(offset[i]) for i in range(n)]
    perm = expected_permutation(seed, 0, n, epoch)
    return perm, [int(offset[ex]) + randint_at((seed, 0), 0, epoch * n + i, 0, int(length[ex]) - T)
                  for i, ex in enumerate(perm)]


def expected_kth_table(structure, offset, length, T, seed, train, epoch, n):
    """(sequences, starts) of an epoch of KTH; structure[c][v] = [store sequence numbers of the video's sequences]"""
    split = 0 if train else 1
    seqs, starts = [], []
    for i in range(n):
        sid = epoch * n + i if train else i
        a = 0
        while True:
            c = randint_at((seed, split), 3 * a, sid, 0, 6)
            v = randint_at((seed, split), 3 * a + 1, sid, 0, len(structure[c]))
            q = structure[c][v][randint_at((seed, split), 3 * a + 2, sid, 0, len(structure[c][v]))]
            if length[q] >= T:
                break
            a += 1
        seqs.append(q)
        starts.append(randint_at((seed, split), 3 * a + 3, sid, 0, int(length[q]) - T + 1))
    return seqs, starts


# ---------------------------------------------------------------------------------------------- fixtures on disk
def t7_bytes(obj, refs=None):
    """Torch7's binary serialisation of None, bool, numbers, bytes / str, lists (tables keyed 1..n) and dicts, as
    data_generators.kth.read_t7 describes it; a list or dict met twice (the same Python object) is written once and
    referred to by its index afterwards"""
    refs = {} if refs is None else refs
    if obj is None:
        return struct.pack("<i", 0)
    if isinstance(obj, bool):
        return struct.pack("<ii", 5, int(obj))
    if isinstance(obj, (int, float)):
        return struct.pack("<id", 1, float(obj))
    if isinstance(obj, (bytes, str)):
        b = obj.encode() if isinstance(obj, str) else obj
        return struct.pack("<ii", 2, len(b)) + b
    if isinstance(obj, (list, dict)):
        if id(obj) in refs:
            return struct.pack("<ii", 3, refs[id(obj)])
        refs[id(obj)] = len(refs) + 1
        items = list(enumerate(obj, 1)) if isinstance(obj, list) else list(obj.items())
        out = struct.pack("<iii", 3, refs[id(obj)], len(items))
        for k, v in items:
            out += t7_bytes(k, refs) + t7_bytes(v, refs)
        return out
    raise TypeError(type(obj))


def touch(path, nbytes):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\0" * nbytes)


def write_png(path, array):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(array).save(path)


BAIR_EXAMPLES = {"train": [("traj_10_to_11", 1, 10), ("traj_2_to_3", 1, 12), ("traj_2_to_3", 2, 9), ("traj_9_to_9", 1, 12)],
                 "test": [("traj_0_to_1", 2, 5), ("traj_0_to_1", 1, 4)]}


def bair_frames(split, side, seed=0):
    """{(trajectory dir, k): uint8 [n, side, side, 3]} of the fixture tree, and the examples in id order"""
    g = np.random.RandomState(seed + (split == "test"))
    frames = {(d, k): g.randint(0, 256, size=(n, side, side, 3)).astype(np.uint8) for d, k, n in BAIR_EXAMPLES[split]}
    order = sorted(frames, key=lambda e: int(e[0].split("_")[1]) + e[1] - 1)
    return frames, order


def write_bair_tree(root, side, write=write_png):
    """the fixture's BAIR tree under `root`; `write(path, frame)` puts one frame"""
    for split in ("train", "test"):
        frames, _ = bair_frames(split, side)
        for (d, k), arr in frames.items():
            for f in range(arr.shape[0]):
                write(os.path.join(root, split, d, str(k), "%d.png" % f), arr[f])


# KTH fixture: per class, videos of sequences of the given lengths (class 1's second video has a too-short sequence)
KTH_LENGTHS = {True: [[[7, 6]], [[8], [3, 6]], [[6]], [[9]], [[6], [7]], [[6, 6, 6]]],
               False: [[[6]], [[6]], [[7]], [[6]], [[6]], [[5]]]}
KTH_T = 5


def kth_layout(train):
    """(structure[c][v] = [sequence numbers], lengths, [[relative frame paths] per sequence], metas {class: object})"""
    structure, lengths, files, metas = [], [], [], {}
    for c, cls in enumerate(CLASSES):
        structure.append([])
        metas[cls] = []
        for v, seqs in enumerate(KTH_LENGTHS[train][c]):
            vid = "person%02d_%s_d%d" % (1 if train else 21, cls, v + 1)
            structure[c].append([])
            names = []
            for s, n in enumerate(seqs):
                structure[c][v].append(len(lengths))
                lengths.append(n)
                names.append([("image-%03d_%dx%d.png" % (100 * s + f, 8, 8)).encode() for f in range(n)])
                files.append(["processed/%s/%s/%s" % (cls, vid, nm.decode()) for nm in names[-1]])
            metas[cls].append({b"vid": vid.encode(), b"files": names, b"n": len(seqs)})
    return structure, lengths, files, metas


def kth_frames(train, side, seed=3):
    _, lengths, _, _ = kth_layout(train)
    g = np.random.RandomState(seed + int(train))
    return g.randint(0, 256, size=(sum(lengths), side, side, 3)).astype(np.uint8)   # channels differ: only 0 is kept


def write_kth_tree(root, side, write=write_png):
    for train in (True, False):
        _, _, files, metas = kth_layout(train)
        frames = kth_frames(train, side)
        for cls in CLASSES:
            p = os.path.join(root, "processed", cls, "%s_meta%dx%d.t7" % ("train" if train else "test", side, side))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(t7_bytes(metas[cls]))
        k = 0
        for seq in files:
            for rel in seq:
                write(os.path.join(root, rel), frames[k])
                k += 1


def array_store(lengths, side, channels, seed=0):
    from data_generators import FrameStore
    g = np.random.RandomState(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    frames = g.randint(0, 256, size=(int(lengths.sum()), side, side, channels)).astype(np.uint8)
    return FrameStore.from_arrays(frames, np.concatenate([[0], np.cumsum(lengths)[:-1]]), lengths)


# ---------------------------------------------------------------------------------------------- t7 reader
def test_t7_reader_on_hand_assembled_bytes():
    from data_generators import read_t7
    i32, f64 = lambda v: struct.pack("<i", v), lambda v: struct.pack("<d", v)
    string = lambda b: i32(2) + i32(len(b)) + b
    number = lambda v: i32(1) + f64(v)
    inner = i32(3) + i32(2) + i32(2) + number(1) + string(b"a.png") + number(2) + string(b"b.png")   # table 2: array
    raw = (i32(3) + i32(1) + i32(6) +                  # table 1: dict-like, 6 pairs
           string(b"vid") + string(b"person01") +
           string(b"files") + i32(3) + i32(3) + i32(2) + number(1) + inner + number(2) + i32(3) + i32(2) +   # table 3
           string(b"flag") + i32(5) + i32(1) +
           string(b"none") + i32(0) +
           string(b"half") + number(0.5) +
           number(7) + i32(3) + i32(4) + i32(0))       # numeric key 7 -> empty table 4
    got = read_t7(raw)
    assert got == {b"vid": b"person01", b"files": [[b"a.png", b"b.png"], [b"a.png", b"b.png"]], b"flag": True,
                   b"none": None, b"half": 0.5, 7: []}
    assert got[b"files"][0] is got[b"files"][1]            # the repeated reference is the same table
    assert type(got[7]) is list and type(got[b"flag"]) is bool
    assert read_t7(t7_bytes([{b"vid": b"x", b"files": [[b"f"]]}, 2.5, False])) == [{b"vid": b"x", b"files": [[b"f"]]},
                                                                                      2.5, False]
    assert read_t7(i32(3) + i32(1) + i32(2) + number(2) + string(b"b") + number(1) + string(b"a")) == [b"a", b"b"]
    assert read_t7(i32(3) + i32(1) + i32(2) + number(2) + string(b"b") + number(3) + string(b"c")) == {2: b"b", 3: b"c"}


def test_t7_reader_rejects_unknown_tags_and_truncation(tmp_path):
    from data_generators import read_t7
    i32 = lambda v: struct.pack("<i", v)
    good = t7_bytes([{b"vid": b"x", b"files": [[b"f"]]}])
    for tag in (4, 6, 7, 8, -1, 99):
        bad = i32(3) + i32(1) + i32(1) + i32(1) + struct.pack("<d", 1.0) + i32(tag) + i32(0)
        with pytest.raises(ValueError, match=r"tag %d at byte offset 24\b" % tag):
            read_t7(bad)
    with pytest.raises(ValueError, match=r"tag 4 at byte offset 0\b"):
        read_t7(i32(4) + i32(1))
    for cut in range(len(good)):
        with pytest.raises(ValueError, match="truncated") as e:
            read_t7(good[:cut])
        at, total = (int(v) for v in re.search(r"byte offset (\d+) of (\d+)", str(e.value)).groups())
        assert at <= cut == total and at > cut - 8      # the failed read starts inside the last 8 bytes that exist
    with pytest.raises(ValueError, match=r"byte offset 8 of 10"):
        read_t7(i32(2) + i32(5) + b"ab")
    p = tmp_path / "m.t7"
    p.write_bytes(good)
    assert read_t7(str(p)) == [{b"vid": b"x", b"files": [[b"f"]]}]


# ---------------------------------------------------------------------------------------------- the C entry point
def test_entry_point_argument_errors_launch_nothing():
    """every argument error of rfn_clip_gather_u8_f32 is a non-zero return before any launch (so it runs without a
    GPU); B == 0 returns 0 without one"""
    import ctypes
    from rfn_hip import lib
    L = lib.load()
    assert lib.SIGNATURES["rfn_clip_gather_u8_f32"] == [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p] + \
        [ctypes.c_int] * 6 + [ctypes.c_void_p]
    buf = ctypes.create_string_buffer(64)          # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda store, first, out, B, T, C, Cs, H, W, F=4: L.rfn_clip_gather_u8_f32(store, F, first, out, B, T, C, Cs,
                                                                                       H, W, None)
    assert call(None, None, None, 0, 2, 3, 3, 4, 4) == 0
    for C, Cs in ((2, 1), (1, 3), (2, 2), (3, 2), (0, 1), (4, 1), (3, 0), (1, 0)):
        assert call(p, p, p, 1, 2, C, Cs, 4, 4) != 0, (C, Cs)
        assert b"rfn_clip_gather_u8_f32" in L.rfn_last_error()
    for T, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4)):
        assert call(p, p, p, 1, T, 1, 1, H, W) != 0
    for ptrs in ((None, p, p), (p, None, p), (p, p, None)):
        assert call(*ptrs, 1, 2, 1, 1, 4, 4) != 0
    assert call(p, p, p, -1, 2, 1, 1, 4, 4) != 0 and call(p, p, p, 1, 2, 1, 1, 4, 4, F=-1) != 0
    assert call(p, p, p, 1 << 20, 1 << 20, 1, 1, 4, 4) != 0        # more workgroups than one launch holds
    assert L.rfn_abi_version() == 2


# ---------------------------------------------------------------------------------------------- the draws
def test_vectorised_philox_and_draws_match_the_restatement(monkeypatch):
    from data_generators import clips
    g = np.random.RandomState(0)
    ctrs = [(0, 0, 0, 0), (M64, M64, M64, 0), (1, 0, 5, 0)] + \
        [tuple(int(v) for v in g.randint(0, 2 ** 63, size=3, dtype=np.int64)) + (0,) for _ in range(20)]
    for key in ((0, 0), (M64, M64), (12345, 3)):
        cols = [np.array([c[k] for c in ctrs], dtype=np.uint64) for k in range(4)]
        got = clips.philox_word0(*cols, key)
        assert [int(v) for v in got] == [philox4x64_10(c, key)[0] for c in ctrs]
    a = np.array([0, 1, M64, 1 << 63, 0xDEADBEEFCAFEF00D, 3], dtype=np.uint64)
    b = np.array([M64, M64, M64, 2, 0x123456789ABCDEF1, 1 << 40], dtype=np.uint64)
    hi, lo = clips._mulhilo(a, b)
    assert [(int(h) << 64) | int(l) for h, l in zip(hi, lo)] == [int(x) * int(y) for x, y in zip(a, b)]
    draw = np.array([0, 1, 2, 3, 40], dtype=np.int64)
    seq = np.array([0, 7, 1 << 40, 9, 9], dtype=np.int64)
    r = np.array([1, 6, 70000, 3, (1 << 62) + 5], dtype=np.int64)
    got = clips.draw_below((5, 1), draw, seq, r)
    assert got.dtype == np.int64 and got.tolist() == [randint_at((5, 1), int(d), int(s), 0, int(x))
                                                      for d, s, x in zip(draw, seq, r)]
    assert clips.draw_below((5, 1), 3, seq, 4).tolist() == [randint_at((5, 1), 3, int(s), 0, 4) for s in seq]
    with pytest.raises(ValueError):
        clips.draw_below((0, 0), 0, 0, np.array([3, 0]))
    # a rejected word (low64(x * r) < 2^64 mod r) repeats the draw at retry + 1: word 0 is rejected for r = 3
    real = clips.philox_word0
    monkeypatch.setattr(clips, "philox_word0", lambda c0, c1, c2, c3, key: np.where(c1 == 0, np.uint64(0),
                                                                                    real(c0, c1, c2, c3, key)))
    assert lemire(0, 3) is None
    got = clips.draw_below((1, 0), np.array([0, 4]), np.array([3, 8]), np.array([3, 1]))
    assert got.tolist() == [lemire(philox4x64_10((0, 1, 3, 0), (1, 0))[0], 3), 0]   # (r = 1 never rejects)


def test_bair_epoch_tables_match_the_restatement():
    from data_generators import ClipLoader, PushDataset
    T = 4
    lengths = [12, 9, 12, 10, 5, 7, 30, 6, 12, 12, 8]
    store = array_store(lengths, 4, 3)
    tr = PushDataset("train", T, img_side=4, seed=6, store=store)
    te = PushDataset("test", T, img_side=4, seed=6, store=store)
    assert len(tr) == len(te) == len(lengths)
    starts = {n: set() for n in range(len(lengths))}
    perms = []
    for e in range(60):
        ex, first = expected_bair_table(store.offset, store.length, T, 6, True, e) if e < 3 else (None, None)
        got_ex, got = tr.epoch_examples(e), tr.epoch_table(e)
        if ex is not None:
            assert got_ex.tolist() == ex and got.tolist() == first
        assert got.dtype == np.int64 and sorted(got_ex.tolist()) == list(range(len(lengths)))
        perms.append(tuple(got_ex.tolist()))
        for x, f in zip(got_ex, got):
            starts[int(x)].add(int(f - store.offset[x]))
    assert len(set(perms)) > 50                                  # the permutations differ between epochs
    same = PushDataset("train", T, img_side=4, seed=6, store=store)
    assert same.epoch_examples(7).tolist() == list(perms[7]) and same.epoch_table(7).tolist() == tr.epoch_table(7).tolist()
    assert PushDataset("train", T, img_side=4, seed=7, store=store).epoch_examples(7).tolist() != list(perms[7])
    for n, L in enumerate(lengths):
        if L <= 12:   # randint(0, L - T): every start up to L - T - 1 occurs, L - T never
            assert starts[n] == set(range(L - T)), (n, L, starts[n])
        assert max(starts[n]) < L - T
    # the test split: example i from frame 0, whatever the epoch
    assert te.epoch_table(0).tolist() == store.offset.tolist() == te.epoch_table(9).tolist()
    assert te.epoch_examples(3).tolist() == list(range(len(lengths)))
    # the first `length` examples only (the reference's Subset)
    sub = PushDataset("train", T, img_side=4, seed=6, store=store, length=4)
    ex, first = expected_bair_table(store.offset, store.length, T, 6, True, 2, n=4)
    assert len(sub) == 4 and sub.epoch_examples(2).tolist() == ex and sub.epoch_table(2).tolist() == first
    # ranks: the union of the ranks' rows is the one-rank batch; incomplete global batches are dropped
    full = ClipLoader(tr, 4)
    assert len(full) == 2
    for g in range(len(full)):
        lo, hi = full.rows(g)
        rows = []
        for r in range(2):
            ld = ClipLoader(tr, 2, rank=r, world=2)
            assert len(ld) == 2
            a, b = ld.rows(g)
            rows += list(range(a, b))
        assert rows == list(range(lo, hi))
    with pytest.raises(ValueError):
        ClipLoader(tr, 2, rank=2, world=2)


def test_bair_limits():
    from data_generators import PushDataset
    store = array_store([6, 4, 6], 4, 3)
    PushDataset("test", 4, img_side=4, store=store)
    with pytest.raises(ValueError, match="more than 4"):
        PushDataset("train", 4, img_side=4, store=store)      # a train example needs n_frames > seq_len
    with pytest.raises(ValueError, match="at least 5"):
        PushDataset("test", 5, img_side=4, store=store)
    with pytest.raises(ValueError):
        PushDataset("test", 4, img_side=8, store=store)
    with pytest.raises(ValueError):
        PushDataset("test", 4, img_side=4, store=array_store([6], 4, 1))
    with pytest.raises(ValueError):
        PushDataset("valid", 4, img_side=4, store=store)


@pytest.fixture(scope="module")
def kth_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kth"))
    write_kth_tree(root, 8)
    return root


def test_kth_tree_store_and_epoch_tables(kth_root):
    from data_generators import KTH
    for train in (True, False):
        structure, lengths, _, _ = kth_layout(train)
        ds = KTH(train, kth_root, seq_len=KTH_T, image_size=8, seed=2)
        assert len(ds) == 6 * 36 * 5
        assert ds.store.Cs == 1 and ds.store.length.tolist() == lengths
        assert torch.equal(ds.store.frames, torch.from_numpy(kth_frames(train, 8)[:, :, :, :1].copy()))   # channel 0
        offset = ds.store.offset
        reached, chosen = set(), set()
        for e in range(2):
            seqs, starts = expected_kth_table(structure, offset, lengths, KTH_T, 2, train, e, len(ds))
            got_seq, got_start = ds.epoch_choices(e)
            assert got_seq.tolist() == seqs and got_start.tolist() == starts
            assert ds.epoch_table(e).tolist() == [int(offset[q]) + s for q, s in zip(seqs, starts)]
            chosen |= set(seqs)
            reached |= {lengths[q] - KTH_T - s for q, s in zip(seqs, starts)}
        short = {q for q, n in enumerate(lengths) if n < KTH_T}
        assert chosen == set(range(len(lengths))) - short          # the short sequence is never chosen
        assert bool(short) == train and 0 in reached               # the last start, length - T, is reached
        if train:
            assert ds.epoch_table(0).tolist() != ds.epoch_table(1).tolist()
        else:
            assert ds.epoch_table(0).tolist() == ds.epoch_table(1).tolist() == ds.epoch_table(5).tolist()
    assert len(KTH(True, kth_root, seq_len=KTH_T, image_size=8, length=500)) == 500
    with pytest.raises(ValueError, match="has 10 frames"):
        KTH(True, kth_root, seq_len=10, image_size=8)              # no sequence is that long
    with pytest.raises(ValueError):
        KTH(True, kth_root, seq_len=KTH_T, image_size=8, channels=2)
    with pytest.raises(ValueError):                                # not the sequences the meta files list
        KTH(True, kth_root, seq_len=KTH_T, image_size=8, store=array_store([5], 8, 1))
    with pytest.raises(FileNotFoundError):
        KTH(True, kth_root, seq_len=KTH_T, image_size=16)


# ---------------------------------------------------------------------------------------------- BAIR tree, cache
@pytest.fixture(scope="module")
def bair_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bair"))
    write_bair_tree(root, 8)
    return root


def test_bair_tree_is_packed_in_numeric_order(bair_root, tmp_path):
    from data_generators import PushDataset
    for split in ("train", "test"):
        frames, order = bair_frames(split, 8)
        ds = PushDataset(split, 3, img_side=8, dataset_dir=bair_root)
        assert [i for i, _ in ds.example_dirs] == sorted(int(d.split("_")[1]) + k - 1 for d, k in frames)
        assert [os.path.relpath(p, os.path.join(bair_root, split)) for _, p in ds.example_dirs] == \
            [os.path.join(d, str(k)) for d, k in order]
        assert ds.store.length.tolist() == [frames[e].shape[0] for e in order]
        # frame order is numeric too: 10.png follows 9.png
        assert torch.equal(ds.store.frames, torch.from_numpy(np.concatenate([frames[e] for e in order])))
        assert ds.store.offset.tolist() == np.concatenate([[0], np.cumsum(ds.store.length)[:-1]]).tolist()
    assert [i for i, _ in PushDataset("train", 3, img_side=8, dataset_dir=bair_root).example_dirs] == [2, 3, 9, 10]
    with pytest.raises(ValueError, match="traj_2_to_3"):            # 9 frames: too short for clips of 9
        PushDataset("train", 9, img_side=8, dataset_dir=bair_root)
    with pytest.raises(ValueError, match="not resized"):
        PushDataset("train", 3, img_side=16, dataset_dir=bair_root)
    os.makedirs(str(tmp_path / "train"))
    with pytest.raises(RuntimeError, match="No data files found"):
        PushDataset("train", 3, img_side=8, dataset_dir=str(tmp_path))
    write_png(str(tmp_path / "test" / "traj_1_to_2" / "1" / "0.png"), np.zeros((8, 8, 3), np.uint8))
    write_png(str(tmp_path / "test" / "traj_1_to_2" / "1" / "1.png"), np.zeros((7, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="1.png is 7x8"):
        PushDataset("test", 2, img_side=8, dataset_dir=str(tmp_path))


def test_store_cache_round_trip_and_invalidation(tmp_path, monkeypatch):
    from data_generators import FrameStore, PushDataset, bair_push
    store = array_store([3, 5], 6, 3, seed=4)
    store.paths, store.sizes = ["a/0.png", "b/1.png"], [10, 12]
    prefix = str(tmp_path / "cache" / "s")
    store.save(prefix)
    assert sorted(os.listdir(str(tmp_path / "cache"))) == ["s.frames.npy", "s.index.npz"]
    back = FrameStore.load(prefix)
    assert torch.equal(back.frames, store.frames) and back.frames.dtype == torch.uint8
    assert back.offset.tolist() == store.offset.tolist() and back.length.tolist() == store.length.tolist()
    assert (back.paths, back.sizes) == (store.paths, store.sizes)
    assert FrameStore.cached(prefix, store.paths, [10, 13]) is None and FrameStore.cached(prefix, store.paths, [10, 12])
    # a dataset: packed once, then loaded while the files match
    root = str(tmp_path / "bair")
    write_bair_tree(root, 8)
    prefix = str(tmp_path / "cache" / "bair_train")
    first = PushDataset("train", 3, img_side=8, dataset_dir=root, cache=prefix)
    assert first.store.paths[0] == "train/traj_10_to_11/1/0.png" and len(first.store.paths) == first.store.n_frames
    decoded = []
    real = bair_push._decode_rgb
    monkeypatch.setattr(bair_push, "_decode_rgb", lambda side: lambda p: (decoded.append(p), real(side)(p))[1])
    again = PushDataset("train", 3, img_side=8, dataset_dir=root, cache=prefix)
    assert not decoded and torch.equal(again.store.frames, first.store.frames)
    assert again.store.offset.tolist() == first.store.offset.tolist()
    # one file changes its size: packed again, and the cache is rewritten
    victim = os.path.join(root, "train", "traj_2_to_3", "1", "10.png")
    frames, _ = bair_frames("train", 8)
    write_png(victim, np.zeros((8, 8, 3), np.uint8))
    assert os.path.getsize(victim) != first.store.sizes[first.store.paths.index("train/traj_2_to_3/1/10.png")]
    third = PushDataset("train", 3, img_side=8, dataset_dir=root, cache=prefix)
    assert len(decoded) == first.store.n_frames
    k = int(third.store.offset[0]) + 10
    assert int(third.store.frames[k].max()) == 0 and torch.equal(third.store.frames[:k], first.store.frames[:k])
    assert FrameStore.load(prefix).sizes == third.store.sizes != first.store.sizes


# ---------------------------------------------------------------------------------------------- Solver wiring
def _args(extra):
    import main_rfn
    return main_rfn.build_parser().parse_args(_solver_argv("--n_frames 3 " + extra))


def test_solver_data_root_errors(tmp_path, monkeypatch):
    from RFN.trainer import Solver
    monkeypatch.chdir(tmp_path)
    assert _args("").data_root is None and _args("").data_cache is None
    for data, tried in (("bair", "bair_robot_data/processed_data"), ("kth", "kth_data")):
        with pytest.raises(RuntimeError) as e:
            Solver(_args("--choose_data %s" % data)).create_loaders()
        msg = str(e.value)
        assert os.path.join(str(tmp_path), tried) in msg and "--data_root" in msg and "--synthetic_data" in msg
        with pytest.raises(FileNotFoundError, match="nowhere"):
            Solver(_args("--choose_data %s --data_root %s" % (data, tmp_path / "nowhere"))).create_loaders()


def test_solver_builds_clip_loaders(bair_root, kth_root, tmp_path, monkeypatch):
    from RFN.trainer import Solver
    cache = tmp_path / "cache"
    s = Solver(_args("--choose_data bair --data_root %s --data_cache %s --x_dim 2 3 8 8 --data_seed 5" % (bair_root, cache)))
    tr, te = s.create_loaders()
    assert type(tr).__name__ == "ClipLoader" and (tr.rank, tr.world, tr.batch_size) == (0, 1, 2)
    assert len(tr) == 2 and len(te) == 1 and tr.dataset.seed == 5 and tr.dataset.train and not te.dataset.train
    assert tr.dataset.seq_len == 3 and tr.dataset.channels == 3
    assert sorted(os.listdir(str(cache))) == ["bair_test_8x8.frames.npy", "bair_test_8x8.index.npz",
                                              "bair_train_8x8.frames.npy", "bair_train_8x8.index.npz"]
    for bad in ("--x_dim 2 1 8 8", "--x_dim 2 3 16 16", "--x_dim 2 3 8 16"):
        with pytest.raises(ValueError):
            Solver(_args("--choose_data bair --data_root %s %s" % (bair_root, bad))).create_loaders()
    for c in (1, 3):
        s = Solver(_args("--choose_data kth --data_root %s --x_dim 2 %d 8 8 --image_size 8" % (kth_root, c)))
        tr, te = s.create_loaders()
        assert len(tr) == len(te) == 540 and tr.dataset.channels == c and tr.dataset.store.Cs == 1
    for bad in ("--x_dim 2 2 8 8 --image_size 8", "--x_dim 2 1 8 8 --image_size 16", "--x_dim 2 1 16 16 --image_size 8"):
        with pytest.raises(ValueError):
            Solver(_args("--choose_data kth --data_root %s %s" % (kth_root, bad))).create_loaders()
    s = Solver(_args("--choose_data kth --data_root %s --x_dim 2 1 8 8 --image_size 8 --use_validation_set" % kth_root))
    assert len(s.create_loaders()[0].dataset) == 500
    s = Solver(_args("--choose_data bair --data_root %s --x_dim 2 3 8 8 --use_validation_set" % bair_root))
    assert len(s.create_loaders()[0].dataset) == 4                # fewer than 500 examples: all of them


def test_create_loaders_reads_args_without_the_new_flags(tmp_path, monkeypatch):
    """Namespaces saved before --data_root / --data_cache existed (and the reference's own) still build loaders, from
    the reference's directories under the working directory"""
    from RFN.trainer import Solver
    write_bair_tree(str(tmp_path / "bair_robot_data" / "processed_data"), 8)
    write_kth_tree(str(tmp_path / "kth_data"), 8)
    monkeypatch.chdir(tmp_path)
    for extra, n in (("--choose_data bair --x_dim 2 3 8 8", 2), ("--choose_data kth --x_dim 2 1 8 8 --image_size 8", 540)):
        args = _args(extra)
        del args.data_root, args.data_cache, args.data_seed, args.mnist_root
        tr, te = Solver(Namespace(**vars(args))).create_loaders()
        assert len(tr) == n and tr.dataset.seed == 0
