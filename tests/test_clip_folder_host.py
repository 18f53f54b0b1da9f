"""Host tests of data_generators/clip_folder.py (no GPU): discovery and natural order, .npy sequences, refused size
changes, eligibility under the span, same-size ingest, the epoch tables restated from the address map of DESIGN.md
section 27, the cache, the new command-line flags and old Namespaces.  The tree builders also serve
tests/test_clip_folder.py."""
import os

import numpy as np
import pytest

from tests.clip_folder_ref import window_ref
from tests.test_clip_datasets_host import write_png
from tests.test_moving_mnist_host import _solver_argv, fixture_digits, write_mnist


def frames_of(T, H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, H, W, C), dtype=np.uint8)


def write_dir(path, frames, ext=".png", name="%d"):
    for k, a in enumerate(frames):
        write_png(os.path.join(path, (name % k) + ext), a[:, :, 0] if a.shape[2] == 1 else a)


def same_size_tree(root, H=6, W=8):
    """train: four sequences of 6x8 grey frames (a .npy among them), lengths 12, 3, 9, 7; test: lengths 5, 8, 2"""
    seqs = {"train": [("b/rec10", 12), ("b/rec2", 3), ("a.npy", 9), ("c/x/y", 7)],
            "test": [("t1", 5), ("t0.npy", 8), ("t2", 2)]}
    data = {}
    for split, items in seqs.items():
        for k, (rel, n) in enumerate(items):
            a = frames_of(n, H, W, 1, 10 * len(rel) + k)
            data[split, rel] = a
            if rel.endswith(".npy"):
                os.makedirs(os.path.join(root, split), exist_ok=True)
                np.save(os.path.join(root, split, rel), a[:, :, :, 0] if k % 2 == 0 else a)
            else:
                write_dir(os.path.join(root, split, rel), a)
    return data


def expected_tables(lengths, T, step, seed, train, epoch, n=None, flip=False, reverse=False):
    """(sequence, start, flags) restated: draw 0 the eligible sequence, 1 the start, 2 the mirror bit, 3 the reverse bit,
    all at the address e * len + i; test: the i-th eligible sequence from frame 0"""
    from data_generators.clips import draw_below
    span = (T - 1) * step + 1
    elig = [k for k, L in enumerate(lengths) if L >= span]
    if not train:
        return elig, [0] * len(elig), [0] * len(elig)
    n = len(elig) if n is None else n
    one = lambda draw, s, r: int(np.asarray(draw_below((seed, 0), draw, s, r)).reshape(-1)[0])
    out = ([], [], [])
    for i in range(n):
        s = epoch * n + i
        q = elig[one(0, s, len(elig))]
        out[0].append(q)
        out[1].append(one(1, s, lengths[q] - span + 1))
        out[2].append((one(2, s, 2) if flip else 0) | (2 * one(3, s, 2) if reverse else 0))
    return out


def test_discovery_and_natural_order(tmp_path):
    from data_generators.clip_folder import list_sequences, natural_key, read_sequence
    root = str(tmp_path)
    a = frames_of(12, 4, 5, 3, 1)
    write_dir(os.path.join(root, "train", "traj_10_to_11", "1"), a)
    write_dir(os.path.join(root, "train", "traj_2_to_3", "1"), a[:3], ext=".bmp")
    write_dir(os.path.join(root, "train", "walking", "person01_d1"), a[:2, :, :, :1], ext=".pgm", name="image-%03d")
    np.save(os.path.join(root, "train", "walking", "clip7.npy"), a[:4])
    with open(os.path.join(root, "train", "walking", "notes.txt"), "w") as f:
        f.write("not a frame")
    os.makedirs(os.path.join(root, "train", "empty"))
    seqs = list_sequences(root, "train")
    assert [r for r, _ in seqs] == ["traj_2_to_3/1", "traj_10_to_11/1", "walking/clip7.npy", "walking/person01_d1"]
    assert [os.path.basename(p) for p in seqs[1][1]] == ["%d.png" % k for k in range(12)]      # 2.png before 10.png
    assert sorted(["10.png", "9.png", "1.png"], key=natural_key) == ["1.png", "9.png", "10.png"]
    assert np.array_equal(read_sequence(seqs[1][1]), a) and np.array_equal(read_sequence(seqs[0][1]), a[:3])
    assert np.array_equal(read_sequence(seqs[2][1]), a[:4])
    assert np.array_equal(read_sequence(seqs[3][1]), a[:2, :, :, :1])                            # grey stays one channel
    with pytest.raises(FileNotFoundError):
        list_sequences(root, "test")


def test_npy_shapes_and_refusals(tmp_path):
    from data_generators.clip_folder import read_sequence
    a = frames_of(3, 4, 5, 1, 2)
    for k, arr in enumerate((a[..., 0], a, np.repeat(a, 3, axis=3))):
        p = str(tmp_path / ("s%d.npy" % k))
        np.save(p, arr)
        got = read_sequence([p])
        assert got.dtype == np.uint8 and got.shape == (3, 4, 5, 3 if k == 2 else 1) and np.array_equal(got[..., 0], a[..., 0])
    for k, arr in enumerate((a.astype(np.float32), a[0, :, :, 0], np.repeat(a, 2, axis=3))):
        p = str(tmp_path / ("bad%d.npy" % k))
        np.save(p, arr)
        with pytest.raises(ValueError, match="bad%d.npy" % k):
            read_sequence([p])


def test_size_change_inside_a_sequence_is_refused(tmp_path):
    from data_generators.clip_folder import list_sequences, read_sequence
    root = str(tmp_path)
    write_dir(os.path.join(root, "train", "s"), frames_of(3, 4, 5, 1, 3))
    write_png(os.path.join(root, "train", "s", "3.png"), frames_of(1, 5, 5, 1, 4)[0, :, :, 0])
    with pytest.raises(ValueError, match="3.png"):
        read_sequence(list_sequences(root, "train")[0][1])
    write_png(os.path.join(root, "train", "s", "3.png"), frames_of(1, 4, 5, 3, 4)[0])           # another channel count
    with pytest.raises(ValueError, match="3.png"):
        read_sequence(list_sequences(root, "train")[0][1])


def test_same_size_ingest_and_eligibility(tmp_path):
    from data_generators import ClipFolder
    root = str(tmp_path)
    data = same_size_tree(root)
    ds = ClipFolder(True, root, seq_len=4, channels=1, height=6, width=8, step=2, device="cpu")   # no GPU is touched
    order = ["a.npy", "b/rec2", "b/rec10", "c/x/y"]
    assert [r for r, _ in ds.sequences] == order
    assert ds.store.length.tolist() == [9, 3, 12, 7] and ds.store.offset.tolist() == [0, 9, 12, 24]
    assert np.array_equal(ds.store.frames.numpy(), np.concatenate([data["train", r] for r in order]))
    assert ds.span == 7 and ds.eligible.tolist() == [0, 2, 3] and len(ds) == 3
    assert len(ClipFolder(True, root, seq_len=4, height=6, width=8, step=2, device="cpu", length=50)) == 50
    assert ClipFolder(True, root, seq_len=4, height=6, width=8, step=3, device="cpu").eligible.tolist() == [2]
    with pytest.raises(ValueError, match="13 frames"):
        ClipFolder(True, root, seq_len=4, height=6, width=8, step=4, device="cpu")
    te = ClipFolder(False, root, seq_len=3, height=6, width=8, step=2, device="cpu", flip=True, reverse=True, length=50)
    assert [r for r, _ in te.sequences] == ["t0.npy", "t1", "t2"] and te.eligible.tolist() == [0, 1] and len(te) == 2
    for bad in (dict(step=0), dict(step=1.5), dict(channels=2), dict(height=0), dict(resize_mode="pad"),
                dict(seq_len=0)):
        with pytest.raises(ValueError):
            ClipFolder(True, root, **dict(dict(seq_len=4, height=6, width=8, device="cpu"), **bad))
    os.makedirs(os.path.join(root, "void", "train"))
    with pytest.raises(ValueError, match="no sequence"):
        ClipFolder(True, os.path.join(root, "void"), height=6, width=8, device="cpu")


def test_epoch_tables(tmp_path):
    from data_generators import ClipFolder, ClipLoader
    root = str(tmp_path)
    same_size_tree(root)
    lengths = [9, 3, 12, 7]
    kw = dict(seq_len=3, channels=1, height=6, width=8, step=2, device="cpu", seed=5)
    ds = ClipFolder(True, root, flip=True, reverse=True, length=24, **kw)
    tables = {}
    for e in (0, 1, 3):
        seq, start, flags = ds.epoch_choices(e)
        want = expected_tables(lengths, 3, 2, 5, True, e, 24, True, True)
        assert (seq.tolist(), start.tolist(), flags.tolist()) == tuple(want)
        assert flags.dtype == np.int32 and ds.epoch_flags(e).tolist() == want[2]
        assert ds.epoch_table(e).tolist() == [int(ds.store.offset[q]) + s for q, s in zip(want[0], want[1])]
        assert all(s + 5 <= lengths[q] for q, s in zip(want[0], want[1]))
        tables[e] = (ds.epoch_table(e).tolist(), want[2])
    again = ClipFolder(True, root, flip=True, reverse=True, length=24, **kw)
    assert (again.epoch_table(1).tolist(), again.epoch_flags(1).tolist()) == tables[1]     # one (seed, epoch), one table
    assert tables[0] != tables[1] and tables[1] != tables[3]
    assert set(tables[0][1]) == {0, 1, 2, 3}                                                # both bits are drawn
    other = ClipFolder(True, root, flip=True, reverse=True, length=24, **dict(kw, seed=6))
    assert other.epoch_table(0).tolist() != tables[0][0]
    # the rows a loader reads do not depend on the batch size or the rank split
    for B, world in ((4, 1), (2, 3), (3, 2), (1, 4)):
        rows = []
        for g in range(24 // (B * world)):
            for r in range(world):
                lo, hi = ClipLoader(ds, B, r, world).rows(g)
                rows += list(range(lo, hi))
        assert rows == list(range(24 // (B * world) * B * world))
    # bits are drawn only when enabled, and the clip choice does not depend on them
    for flip, reverse, allowed in ((False, False, {0}), (True, False, {0, 1}), (False, True, {0, 2})):
        d = ClipFolder(True, root, flip=flip, reverse=reverse, length=24, **kw)
        assert set(d.epoch_flags(0).tolist()) == allowed and d.epoch_table(0).tolist() == tables[0][0]
        assert d.epoch_flags(0).tolist() == [f & (1 * flip | 2 * reverse) for f in tables[0][1]]
    # the test split: every eligible sequence from its first frame, unflagged, whatever the epoch
    te = ClipFolder(False, root, flip=True, reverse=True, **dict(kw, seq_len=2))
    assert te.store.length.tolist() == [8, 5, 2] and te.eligible.tolist() == [0, 1]
    for e in (0, 7):
        assert te.epoch_table(e).tolist() == [0, 8] and te.epoch_flags(e).tolist() == [0, 0]


def test_cache_is_reused_and_repacked(tmp_path, monkeypatch):
    from data_generators import ClipFolder, clip_folder
    root, cache = str(tmp_path / "data"), str(tmp_path / "cache" / "folder_train_6x8x1_crop")
    same_size_tree(root)
    kw = dict(seq_len=3, channels=1, height=6, width=8, device="cpu")
    first = ClipFolder(True, root, cache=cache, **kw)
    assert os.path.isfile(cache + ".frames.npy") and os.path.isfile(cache + ".index.npz")
    reads = []
    real = clip_folder.read_sequence
    monkeypatch.setattr(clip_folder, "read_sequence", lambda files: (reads.append(files[0]), real(files))[1])
    again = ClipFolder(True, root, cache=cache, **kw)
    assert not reads and np.array_equal(again.store.frames.numpy(), first.store.frames.numpy())
    assert again.store.length.tolist() == first.store.length.tolist()
    # a changed file is packed again
    np.save(os.path.join(root, "train", "a.npy"), frames_of(10, 6, 8, 1, 77))
    changed = ClipFolder(True, root, cache=cache, **kw)
    assert len(reads) == 4 and changed.store.length.tolist() == [10, 3, 12, 7]
    # another geometry under the same prefix is not taken for this one (every sequence would need the GPU resize)
    del reads[:]
    from data_generators.clips import FrameStore
    stale = FrameStore(np.zeros((32, 3, 4, 1), dtype=np.uint8), changed.store.offset, changed.store.length,
                       changed.store.paths, changed.store.sizes)
    stale.save(cache)
    fresh = ClipFolder(True, root, cache=cache, **kw)
    assert len(reads) == 4 and (fresh.store.H, fresh.store.W) == (6, 8)


def test_resize_window_on_the_host():
    from rfn_hip import ops
    for Hs, Ws, H, W in ((120, 160, 64, 64), (160, 120, 64, 64), (12, 16, 8, 8), (10, 10, 8, 8), (7, 5, 3, 4),
                         (1, 500, 64, 1), (480, 640, 48, 64), (3, 1000, 9, 16)):
        for mode in ("crop", "stretch"):
            y0, x0, Hc, Wc = ops.resize_window(Hs, Ws, H, W, mode)
            assert (y0, x0, Hc, Wc) == window_ref(Hs, Ws, H, W, mode)
            assert Hc >= 1 and Wc >= 1 and 0 <= y0 <= Hs - Hc and 0 <= x0 <= Ws - Wc
    assert ops.resize_window(120, 160, 64, 64, "crop") == (0, 20, 120, 120)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """the new entry points' argument errors are returns before any launch"""
    from rfn_hip import lib
    L = lib.load()
    assert L.rfn_frames_resize_u8(None, 0, 0, 8, 8, 1, 4, 4, 1, 0, 0, 8, 8, None) == 0
    for code, args in ((-1, (1, 0, 8, 1, 4, 4, 1, 0, 0, 8, 8)), (-2, (1, 8, 8, 2, 4, 4, 1, 0, 0, 8, 8)),
                       (-3, (1, 8, 8, 1, 4, 4, 1, 0, 1, 8, 8)), (-5, (1, 8, 8, 1, 4, 4, 1, 0, 0, 8, 8))):
        assert L.rfn_frames_resize_u8(None, 0, *args, None) == code
        assert b"rfn_frames_resize_u8" in L.rfn_last_error()
    assert L.rfn_clip_gather_aug_u8_f32(None, 4, None, None, None, 0, 2, 1, 1, 4, 4, 1, None) == 0
    for code, args in ((-1, (1, 2, 1, 1, 4, 4, 0)), (-2, (1, 2, 1, 3, 4, 4, 1)), (-5, (1, 2, 1, 1, 4, 4, 1))):
        assert L.rfn_clip_gather_aug_u8_f32(None, 4, None, None, None, *args, None) == code
        assert b"rfn_clip_gather_aug_u8_f32" in L.rfn_last_error()


def test_parser_defaults_and_folder_flags(tmp_path):
    import main_rfn
    from RFN.trainer import Solver
    args = main_rfn.build_parser().parse_args([])
    assert (args.frame_step, args.augment, args.resize_mode, args.choose_data) == (1, [], "crop", "bair")
    args = main_rfn.build_parser().parse_args("--choose_data folder --frame_step 3 --augment flip reverse "
                                              "--resize_mode stretch".split())
    assert (args.choose_data, args.frame_step, args.augment, args.resize_mode) == ("folder", 3, ["flip", "reverse"],
                                                                                   "stretch")
    for bad in ("--augment rotate", "--resize_mode pad", "--choose_data video"):
        with pytest.raises(SystemExit):
            main_rfn.build_parser().parse_args(bad.split())
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv("--choose_data folder --path %s" % rel))
    with pytest.raises(ValueError, match="--data_root"):
        Solver(args).create_loaders()
    args.data_root = str(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError):
        Solver(args).create_loaders()


def test_solver_builds_folder_loaders_and_reads_old_args(tmp_path):
    """same-size frames: the loaders are built without a GPU; Namespaces saved before the new flags existed still work"""
    import main_rfn
    from RFN.trainer import Solver
    root = str(tmp_path / "data")
    same_size_tree(root)
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    argv = "--choose_data folder --data_root %s --data_cache %s --path %s --data_seed 5 --n_frames 3 --frame_step 2 " \
           "--augment flip reverse --x_dim 2 1 6 8 --condition_dim 2 1 6 8" % (root, tmp_path / "cache", rel)
    args = main_rfn.build_parser().parse_args(_solver_argv(argv))
    tr, te = Solver(args).create_loaders()
    assert type(tr).__name__ == "ClipLoader" and type(tr.dataset).__name__ == "ClipFolder"
    assert (tr.dataset.step, tr.dataset.flip, tr.dataset.reverse, tr.dataset.seed) == (2, True, True, 5)
    assert (te.dataset.step, te.dataset.flip, te.dataset.reverse) == (2, False, False)
    assert len(tr.dataset) == 3 and len(tr) == 1 and len(te.dataset) == 2
    want = expected_tables([9, 3, 12, 7], 3, 2, 5, True, 2, 3, True, True)
    assert tr.dataset.epoch_choices(2)[0].tolist() == want[0] and tr.dataset.epoch_flags(2).tolist() == want[2]
    assert os.path.isfile(str(tmp_path / "cache" / "folder_train_6x8x1_crop.frames.npy"))
    assert os.path.isfile(str(tmp_path / "cache" / "folder_test_6x8x1_crop.index.npz"))
    args.use_validation_set = True
    assert len(Solver(args).create_loaders()[0].dataset) == 500
    del args.frame_step, args.augment, args.resize_mode, args.data_cache, args.data_seed
    args.use_validation_set = False
    tr, _ = Solver(args).create_loaders()
    assert (tr.dataset.step, tr.dataset.flip, tr.dataset.reverse, tr.dataset.resize_mode) == (1, False, False, "crop")
    # ... and still build the mnist loaders
    write_mnist(str(tmp_path / "Mnist"), fixture_digits(10, 5), fixture_digits(6, 6))
    args = main_rfn.build_parser().parse_args(_solver_argv("--choose_data mnist --mnist_root %s" % (tmp_path / "Mnist")))
    del args.frame_step, args.augment, args.resize_mode
    tr, te = Solver(args).create_loaders()
    assert type(tr).__name__ == "MovingMNISTLoader" and len(tr) == 5 and len(te) == 3
