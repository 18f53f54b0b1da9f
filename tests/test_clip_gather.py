"""GPU tests of the file-backed datasets' device path: rfn_clip_gather_u8_f32 (through rfn_hip.ops.clip_gather) against
torch's own index / permute / float / divide, bit for bit; its guard, its argument errors and its stream; ClipLoader
batches against the host epoch tables restated in tests/test_clip_datasets_host.py; and the Solver / Evaluator end to
end on BAIR- and KTH-shaped stores loaded from a cache.  Everything is built from arrays: no image is decoded here."""
import itertools
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.test_clip_datasets_host import (CLASSES, array_store, bair_frames, expected_bair_table, expected_kth_table,
                                           kth_frames, kth_layout, touch, write_bair_tree, write_kth_tree)
from tests.test_moving_mnist_host import _solver_argv

pytestmark = pytest.mark.gpu

# (B, T, Cs, C, H, W): the issue's shapes -- the scalar path; a frame whose byte count is no multiple of 16; the BAIR
# frame (4 runs of 1024 pixels); KTH's three copies; a frame smaller than a run -- then a frame of 1296 pixels (a
# whole run and a tail of 272) and 12 pixels in 12 bytes (H*W a multiple of 4, the byte count not one of 16)
CASES = [(3, 2, 1, 1, 5, 7), (2, 3, 3, 3, 5, 7), (4, 5, 3, 3, 64, 64), (2, 4, 1, 3, 32, 32), (1, 1, 3, 3, 8, 8),
         (2, 2, 3, 3, 36, 36), (2, 2, 1, 3, 36, 36), (3, 2, 1, 1, 2, 6)]


def make_store(F, H, W, Cs, seed, slack=3):
    """uint8 [F, H, W, Cs] on the GPU holding every byte value: the leading F frames of a larger allocation, so that no
    read of a faulty kernel near the end leaves allocated memory"""
    g = torch.Generator().manual_seed(seed)
    big = torch.randint(0, 256, (F + slack, H, W, Cs), generator=g, dtype=torch.uint8)
    flat = big[:F].reshape(-1)
    n = min(256, flat.numel())
    flat[:n] = torch.arange(256, dtype=torch.uint8)[256 - n:]
    assert F * H * W * Cs < 256 or len(set(flat.tolist())) == 256
    big = big.cuda()
    return big[:F]


def torch_clips(store, first, T, C):
    """the same batch by torch: index, permute, float, divide.  Computed on the host, where torch divides: on the GPU
    its kernel for a Python-number divisor multiplies by float32(1 / 255) instead, another float for 126 of the bytes"""
    dev, store, first = store.device, store.cpu(), first.cpu()
    idx = first[:, None] + torch.arange(T)
    x = store[idx].permute(0, 1, 4, 2, 3)
    if x.shape[2] != C:
        x = x.expand(-1, -1, C, -1, -1)
    return (x.float() / 255).to(dev)


@pytest.mark.parametrize("B,T,Cs,C,H,W", CASES)
def test_kernel_matches_torch(B, T, Cs, C, H, W):
    from rfn_hip import ops
    F = T + 9
    store = make_store(F, H, W, Cs, B + T + H)
    # descending, with the last possible start, a repeated index and 0; taken B at a time
    firsts = [F - T, 5, 5, 3, 1, 0]
    firsts += firsts[:(-len(firsts)) % B]
    for k in range(0, len(firsts), B):
        first = torch.tensor(firsts[k:k + B], dtype=torch.int64, device="cuda")
        out = ops.clip_gather(store, first, T, C)
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, T, C, H, W) and out.is_contiguous()
        assert torch.equal(out, torch_clips(store, first, T, C))
    all_first = torch.tensor(firsts, dtype=torch.int64, device="cuda")
    assert torch.equal(ops.clip_gather(store, all_first, T, C), torch_clips(store, all_first, T, C))


def test_quotients_are_correctly_rounded():
    """all 256 bytes: float32(k) / float32(255), which is also float32(k / 255.) -- not k * (1 / 255.f)"""
    from rfn_hip import ops
    want = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(want, (np.arange(256) / 255.).astype(np.float32))
    assert int((want != np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))).sum()) == 126
    assert np.array_equal(want, (torch.arange(256, dtype=torch.uint8).float() / 255).numpy())   # torch_clips' rule
    for shape in ((1, 16, 16, 1), (1, 1, 256, 1), (1, 2, 128, 1)):
        store = torch.arange(256, dtype=torch.uint8).reshape(shape).cuda()
        out = ops.clip_gather(store, torch.zeros(1, dtype=torch.int64, device="cuda"), 1, 1)
        assert np.array_equal(out.cpu().numpy().reshape(-1), want)
    store = torch.arange(256, dtype=torch.uint8).repeat_interleave(3).reshape(1, 16, 16, 3).cuda()
    out = ops.clip_gather(store, torch.zeros(1, dtype=torch.int64, device="cuda"), 1, 3)
    assert all(np.array_equal(out[0, 0, c].cpu().numpy().reshape(-1), want) for c in range(3))


@pytest.mark.parametrize("Cs,C,H,W", [(3, 3, 8, 8), (1, 3, 36, 36), (3, 3, 5, 7), (1, 1, 2, 6)])
def test_guard_writes_nan_and_reads_nothing(Cs, C, H, W):
    from rfn_hip import ops
    T, F = 3, 8
    store = make_store(F, H, W, Cs, 11)
    first = torch.tensor([F - T, F - T + 1, 2, -1, 0, F + 100, -(1 << 62), (1 << 62)], dtype=torch.int64, device="cuda")
    out = ops.clip_gather(store, first, T, C)
    bad = [1, 3, 5, 6, 7]
    good = [0, 2, 4]
    assert bool(torch.isnan(out[bad]).all())                     # every frame of a clip that leaves the store
    assert torch.equal(out[good], torch_clips(store, first[good], T, C))   # its neighbours stay exact


def test_empty_batch_and_side_stream():
    from rfn_hip import ops
    store = make_store(9, 16, 16, 3, 2)
    out = ops.clip_gather(store, torch.zeros(0, dtype=torch.int64, device="cuda"), 4, 3)
    assert tuple(out.shape) == (0, 4, 3, 16, 16) and out.dtype == torch.float32 and out.is_cuda
    first = torch.tensor([5, 0, 2], dtype=torch.int64, device="cuda")
    want = torch_clips(store, first, 4, 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ops.clip_gather(store, first, 4, 3)
    side.synchronize()
    assert torch.equal(got, want)


def test_argument_errors():
    from rfn_hip import ops
    store = make_store(6, 4, 4, 3, 1)
    first = torch.zeros(2, dtype=torch.int64, device="cuda")
    ops.clip_gather(store, first, 2, 3)
    for bad_store, exc in ((store.float(), TypeError), ("frames", TypeError),
                           (store[0], ValueError), (store[..., :2], ValueError), (store[:, :0], ValueError),
                           (store.cpu(), ValueError), (store[:0], ValueError)):
        with pytest.raises(exc):
            ops.clip_gather(bad_store, first, 2, 3)
    for bad_first, exc in ((first.int(), TypeError), (first.float(), TypeError), ([0, 1], TypeError),
                           (first[:, None], ValueError), (first.cpu(), ValueError)):
        with pytest.raises(exc):
            ops.clip_gather(store, bad_first, 2, 3)
    for T, C in ((0, 3), (-1, 3), (2, 1), (2, 2), (2, 0)):        # three stored channels give three
        with pytest.raises(ValueError):
            ops.clip_gather(store, first, T, C)
    with pytest.raises(ValueError):
        ops.clip_gather(store[..., :1].contiguous(), first, 2, 2)  # one stored channel gives one or three


# ---------------------------------------------------------------------------------------------- the loader
def test_clip_loader_matches_host_tables(tmp_path):
    from data_generators import KTH, ClipLoader, PushDataset
    T = 4
    store = array_store([12, 9, 12, 10, 5, 7, 30, 6, 12], 8, 3, seed=5)
    dev = store.device_frames()
    assert store.device_frames() is dev                          # uploaded once
    for train in (True, False):
        ds = PushDataset("train" if train else "test", T, img_side=8, seed=3, store=store)
        ld = ClipLoader(ds, 4)
        assert len(ld) == 2
        for e in (0, 2):
            ld.set_epoch(e)
            _, first = expected_bair_table(store.offset, store.length, T, 3, train, e)
            got = list(ld)
            assert len(got) == 2 and got[0].data_ptr() != got[1].data_ptr()
            for g, x in enumerate(got):
                rows = torch.tensor(first[4 * g:4 * g + 4], device="cuda")
                assert tuple(x.shape) == (4, T, 3, 8, 8) and torch.equal(x, torch_clips(dev, rows, T, 3))
                assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
            for r in range(2):                                    # rank r of 2: rows [2r, 2r + 2) of each global batch
                lr = ClipLoader(ds, 2, rank=r, world=2)
                lr.set_epoch(e)
                assert all(torch.equal(x, full[2 * r:2 * r + 2]) for x, full in zip(lr, got))
        assert torch.equal(ds[1], torch_clips(dev, torch.tensor(expected_bair_table(
            store.offset, store.length, T, 3, train, 0)[1][1:2], device="cuda"), T, 3)[0])
    # KTH: the meta files alone describe the videos; the frames come from an array store
    root = str(tmp_path / "kth")
    write_kth_tree(root, 8, write=lambda p, a: touch(p, 1))
    for train in (True, False):
        structure, lengths, _, _ = kth_layout(train)
        store = array_store(lengths, 8, 1, seed=6)
        for C in (1, 3):
            ds = KTH(train, root, seq_len=T, image_size=8, seed=1, store=store, channels=C, length=24)
            ld = ClipLoader(ds, 8)
            ld.set_epoch(1)
            seqs, starts = expected_kth_table(structure, store.offset, lengths, T, 1, train, 1, 24)
            first = [int(store.offset[q]) + s for q, s in zip(seqs, starts)]
            got = list(ld)
            assert len(got) == 3
            for g, x in enumerate(got):
                rows = torch.tensor(first[8 * g:8 * g + 8], device="cuda")
                assert torch.equal(x, torch_clips(store.device_frames(), rows, T, C))


# ---------------------------------------------------------------------------------------------- end to end
def _cached_tree(tmp_path, data):
    """a tree of placeholder files (nothing in it can be decoded) and, under the cache directory, the packed stores
    with the tree's fingerprint: what a second run finds after a first one has decoded the dataset"""
    from data_generators import FrameStore, bair_push, clips
    root, cache = str(tmp_path / data), str(tmp_path / "cache")
    if data == "bair":
        write_bair_tree(root, 32, write=lambda p, a: touch(p, 5 + int(a[0, 0, 0])))
        for split in ("train", "test"):
            frames, order = bair_frames(split, 32)
            files = [f for _, _, f in bair_push.list_examples(root, split)]
            lengths = np.array([len(f) for f in files])
            assert lengths.tolist() == [frames[e].shape[0] for e in order]
            paths, sizes = clips.fingerprint(root, [p for f in files for p in f])
            FrameStore(np.concatenate([frames[e] for e in order]), np.concatenate([[0], np.cumsum(lengths)[:-1]]),
                       lengths, paths, sizes).save(os.path.join(cache, "bair_%s_32x32" % split))
    else:
        write_kth_tree(root, 32, write=lambda p, a: touch(p, 5 + int(a[0, 0, 0])))
        for train in (True, False):
            _, lengths, files, _ = kth_layout(train)
            name = "train" if train else "test"
            metas = [os.path.join(root, "processed", c, "%s_meta32x32.t7" % name) for c in CLASSES]
            paths, sizes = clips.fingerprint(root, [os.path.join(root, p) for f in files for p in f] + metas)
            lengths = np.array(lengths)
            FrameStore(kth_frames(train, 32)[:, :, :, :1].copy(), np.concatenate([[0], np.cumsum(lengths)[:-1]]),
                       lengths, paths, sizes).save(os.path.join(cache, "kth_%s_32x32" % name))
    return root, cache


@pytest.mark.parametrize("data,C", [("bair", 3), ("kth", 1)])
def test_solver_trains_and_evaluates_from_cached_store(tmp_path, data, C):
    import main_rfn
    from RFN.trainer import Solver
    from evaluation_metrics import Evaluator
    root, cache = _cached_tree(tmp_path, data)
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv(
        "--choose_data %s --data_root %s --data_cache %s --path %s --data_seed 4 --x_dim 2 %d 32 32 "
        "--condition_dim 2 %d 32 32" % (data, root, cache, rel, C, C)))
    torch.manual_seed(0)
    s = Solver(args)
    s.build()
    assert type(s.train_loader).__name__ == "ClipLoader" and type(s.test_loader).__name__ == "ClipLoader"
    want = torch.from_numpy(np.concatenate([bair_frames("train", 32)[0][e] for e in bair_frames("train", 32)[1]])
                            if data == "bair" else kth_frames(True, 32)[:, :, :, :1].copy())
    assert torch.equal(s.train_loader.dataset.store.frames, want)            # the cache, not the placeholders
    it = iter(s.train_loader)
    losses = []
    for _ in range(2):
        x = next(it)
        assert x.is_cuda and tuple(x.shape) == (2, 4, C, 32, 32)
        losses.append(float(s.train_step(x).detach()))
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in losses), losses
    ev = Evaluator(s, settings=Namespace(n_frames=4, start_predictions=2, resample=2, n_trained=4))
    seen = []
    watched = s.test_loader.dataset.gather
    s.test_loader.dataset.gather = lambda first: (seen.append(watched(first)), seen[-1])[1]
    mean, _ = ev.get_loss(max_batches=1)
    assert math.isfinite(float(mean))
    in_loss, seen = seen, []
    out = ev.get_eval_values(max_batches=1)
    mse, psnr, ssim, lpips, bpd, dkl, recon, ssim_std, psnr_std, lpips_std = out
    for t in (mse, psnr, ssim, ssim_std, psnr_std):
        assert tuple(t.shape) == (2, 2) and t.dtype == torch.float32
    assert lpips is None and tuple(bpd.shape) == (1,) and math.isfinite(float(bpd[0]))
    # two consecutive evaluations saw the same test batches: the test split is a fixed set
    assert in_loss and len(in_loss) == len(seen) and all(torch.equal(a, b) for a, b in zip(in_loss, seen))
    first = list(itertools.islice(iter(s.test_loader), 2))
    again = list(itertools.islice(iter(s.test_loader), 2))
    assert first and torch.equal(first[0], in_loss[0]) and all(torch.equal(a, b) for a, b in zip(first, again))
