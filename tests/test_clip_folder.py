"""GPU tests of `--choose_data folder` end to end: a tree of RGB PNG directories and a grey .npy of other sizes is
resampled into the target geometry at ingest (the store equals the numpy restatement of rfn_frames_resize_u8), the
loader's batches equal the restated strided, mirrored, reversed gather of the restated epoch tables, and a Solver built
from the command line takes a training step on it."""
import math
import os

import numpy as np
import pytest
import torch

from tests.clip_folder_ref import gather_aug_ref, resize_ref, window_ref
from tests.test_clip_folder_host import expected_tables, frames_of, write_dir
from tests.test_moving_mnist_host import _solver_argv

pytestmark = pytest.mark.gpu


def mixed_tree(root, scale=1):
    """train: two RGB PNG directories of 12x16 (times `scale`) and a grey 10x10 .npy; test: one of each.  Returns the
    frames [(split, relative path)] as the reader should see them."""
    data = {}
    for split, items in (("train", [("push/rec2", 9, 3), ("push/rec10", 14, 3), ("grey.npy", 11, 1)]),
                         ("test", [("a", 8, 3), ("b.npy", 9, 1)])):
        for k, (rel, n, C) in enumerate(items):
            a = frames_of(n, (12 if C == 3 else 10) * scale, (16 if C == 3 else 10) * scale, C, 100 * len(split) + k)
            data[split, rel] = a
            if rel.endswith(".npy"):
                os.makedirs(os.path.join(root, split), exist_ok=True)
                np.save(os.path.join(root, split, rel), a[..., 0])
            else:
                write_dir(os.path.join(root, split, rel), a)
    return data


def restated_store(data, split, order, H, W, C, mode):
    return np.concatenate([resize_ref(data[split, r], H, W, C,
                                      window_ref(data[split, r].shape[1], data[split, r].shape[2], H, W, mode))
                           for r in order])


@pytest.mark.parametrize("mode", ["crop", "stretch"])
def test_ingest_and_batches_match_the_restatement(tmp_path, mode, monkeypatch):
    from data_generators import ClipFolder, ClipLoader, clips
    root = str(tmp_path / "data")
    data = mixed_tree(root)
    monkeypatch.setattr(clips, "RESIZE_CHUNK_BYTES", 5 * 12 * 16 * 3)          # several uploads per sequence
    T, step = 3, 2
    kw = dict(seq_len=T, channels=1, height=8, width=8, step=step, resize_mode=mode, seed=9)
    cache = str(tmp_path / "cache" / ("folder_train_8x8x1_" + mode))
    ds = ClipFolder(True, root, flip=True, reverse=True, length=12, cache=cache, **kw)
    order = ["grey.npy", "push/rec2", "push/rec10"]
    assert [r for r, _ in ds.sequences] == order and ds.store.length.tolist() == [11, 9, 14]
    want_store = restated_store(data, "train", order, 8, 8, 1, mode)
    assert np.array_equal(ds.store.frames.numpy(), want_store)
    assert np.array_equal(ClipFolder(True, root, cache=cache, **kw).store.frames.numpy(), want_store)   # from the cache
    for e in (0, 2):
        seq, start, flags = expected_tables([11, 9, 14], T, step, 9, True, e, 12, True, True)
        first = [int(ds.store.offset[q]) + s for q, s in zip(seq, start)]
        whole = gather_aug_ref(want_store, first, T, 1, step, flags)
        assert not np.isnan(whole).any()
        ld = ClipLoader(ds, 4)
        ld.set_epoch(e)
        got = list(ld)
        assert len(got) == 3
        for g, x in enumerate(got):
            assert tuple(x.shape) == (4, T, 1, 8, 8) and np.array_equal(x.cpu().numpy(), whole[4 * g:4 * g + 4])
        for r in range(2):                                         # rank r of 2 reads rows [2r, 2r + 2) of each batch
            lr = ClipLoader(ds, 2, rank=r, world=2)
            lr.set_epoch(e)
            assert all(torch.equal(x, full[2 * r:2 * r + 2]) for x, full in zip(lr, got))
        if e == 0:
            assert np.array_equal(ds[5].cpu().numpy(), whole[5])
    # three channels out of the same files: copies of the grey sequence, the RGB frames themselves
    rgb = ClipFolder(False, root, channels=3, height=8, width=8, seq_len=T, step=step, resize_mode=mode)
    want = restated_store(data, "test", ["a", "b.npy"], 8, 8, 3, mode)
    assert np.array_equal(rgb.store.frames.numpy(), want)
    x = next(iter(ClipLoader(rgb, 2)))
    assert np.array_equal(x.cpu().numpy(), gather_aug_ref(want, [0, 8], T, 3, step, [0, 0]))


def test_solver_trains_on_a_folder(tmp_path):
    import main_rfn
    from RFN.trainer import Solver
    root = str(tmp_path / "data")
    data = mixed_tree(root, scale=4)                                    # 48x64 RGB and 40x40 grey frames
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv(
        "--choose_data folder --data_root %s --data_cache %s --path %s --data_seed 4 --frame_step 2 "
        "--augment flip reverse" % (root, tmp_path / "cache", rel)))
    torch.manual_seed(0)
    s = Solver(args)
    s.build()
    tr = s.train_loader
    assert type(tr).__name__ == "ClipLoader" and type(tr.dataset).__name__ == "ClipFolder"
    order = ["grey.npy", "push/rec2", "push/rec10"]
    assert np.array_equal(tr.dataset.store.frames.numpy(), restated_store(data, "train", order, 32, 32, 1, "crop"))
    assert os.path.isfile(str(tmp_path / "cache" / "folder_train_32x32x1_crop.frames.npy"))
    x = next(iter(tr))
    assert x.is_cuda and tuple(x.shape) == (2, 4, 1, 32, 32) and 0.0 <= float(x.min()) and float(x.max()) <= 1.0
    loss = float(s.train_step(x).detach())
    torch.cuda.synchronize()
    assert math.isfinite(loss), loss
    te = next(iter(s.test_loader))
    assert tuple(te.shape) == (2, 4, 1, 32, 32) and not bool(torch.isnan(te).any())
