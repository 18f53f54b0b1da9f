"""BAIR robot pushing from local PNG files, held on the device (the reference's data_generators/bair_push.py:20-109 as
RFN/trainer.py:132-140 drives it).

Examples are `<dataset_dir>/<split>/traj_<A>_to_<B>/<k>/<frame>.png`; example id = A + k - 1; examples and frames are
sorted numerically, as the reference sorts them.  All frames of the split are decoded once (PIL, RGB) into a FrameStore
(clips.py), or loaded from a cache whose fingerprint matches; a batch is then one launch of the clip-gather kernel.

Clip choice (clips.py states the draws): the train split visits a permutation of its examples per epoch (the
reference's shuffle=True) and starts each clip at randint(0, n_frames - seq_len) -- upper end exclusive, as numpy's, so
the last possible start is never taken, exactly as in the reference; the test split is example i from frame 0.

Deviations from the reference: frames that are not img_side x img_side raise (it would resize them with cv2); a train
example with n_frames <= seq_len raises at construction (its randint fails at fetch time); the loader yields the frames
alone, not the reference's (frames, index) tuple; the test loader is not shuffled."""
import os
import re

import numpy as np

from .clips import ClipDataset, draw_below, pack_or_load, permutation

_DIR = re.compile(r"^traj_(\d+)_to_(\d+)$")
_FRAME = re.compile(r"^(\d+)\.png$")


def list_examples(dataset_dir, split):
    """[(example id, directory, [frame paths in frame order])] of a split, sorted by id"""
    data_dir = os.path.join(dataset_dir, split)
    examples = []
    for traj in (sorted(os.listdir(data_dir)) if os.path.isdir(data_dir) else ()):
        tdir = os.path.join(data_dir, traj)
        if not os.path.isdir(tdir):
            continue
        m = _DIR.match(traj)
        for k in sorted(os.listdir(tdir)):
            ex_dir = os.path.join(tdir, k)
            if not os.path.isdir(ex_dir):
                continue
            if m is None or not k.isdigit():
                raise ValueError("PushDataset: %s is not traj_<A>_to_<B>/<k>" % ex_dir)
            frames = []
            for f in os.listdir(ex_dir):
                if f.endswith(".png"):
                    fm = _FRAME.match(f)
                    if fm is None:
                        raise ValueError("PushDataset: frame %s is not <number>.png" % os.path.join(ex_dir, f))
                    frames.append((int(fm.group(1)), os.path.join(ex_dir, f)))
            examples.append((int(m.group(1)) + int(k) - 1, ex_dir, [p for _, p in sorted(frames)]))
    if not examples:
        raise RuntimeError("No data files found at: %s" % data_dir)
    return sorted(examples, key=lambda e: (e[0], e[1]))


def _decode_rgb(side):
    def decode(path):
        from PIL import Image   # only needed when PNGs are decoded: a matching cache never gets here
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"))
        if a.shape != (side, side, 3):
            raise ValueError("PushDataset: %s is %dx%d, expected %dx%d (frames are not resized)" %
                             (path, a.shape[0], a.shape[1], side, side))
        return a
    return decode


class PushDataset(ClipDataset):
    """The reference's PushDataset with its constructor arguments (data_augmentation and normalize are as inert as
    there), plus `seed` (None = 0) keying the draws, `device` (where the frames live; default the current GPU),
    `cache` (a file prefix for the packed store), `length` (use only the first `length` examples: the reference's
    Subset) and `store` (a ready FrameStore: no file is read, its sequences are the examples in order)."""

    def __init__(self, split, seq_len, img_side=64, dataset_dir='', data_augmentation=True, normalize=True, seed=None,
                 device=None, cache=None, length=None, store=None):
        if split not in ("train", "test"):
            raise ValueError("PushDataset: split must be 'train' or 'test', got %r" % (split,))
        self.split, self.img_side = split, int(img_side)
        if store is None:
            examples = list_examples(dataset_dir, split)
            self.example_dirs = [[i, d] for i, d, _ in examples]
            store = pack_or_load(cache, dataset_dir, [f for _, _, f in examples], _decode_rgb(self.img_side),
                                 self.img_side, self.img_side, 3)
        else:
            self.example_dirs = [[n, None] for n in range(len(store))]
        if (store.H, store.W, store.Cs) != (self.img_side, self.img_side, 3):
            raise ValueError("PushDataset: the store holds %dx%dx%d frames, expected %dx%dx3" %
                             (store.H, store.W, store.Cs, self.img_side, self.img_side))
        if len(store) != len(self.example_dirs):
            raise ValueError("PushDataset: the store holds %d sequences for %d examples" %
                             (len(store), len(self.example_dirs)))
        self._setup(store, seq_len, 3, split == "train", seed, device)
        if length is not None:
            self.example_dirs = self.example_dirs[:int(length)]
        n = len(self.example_dirs)
        if n < 1:
            raise RuntimeError("PushDataset: no example in the %s split" % split)
        need = self.seq_len + 1 if self.train else self.seq_len
        short = np.nonzero(store.length[:n] < need)[0]
        if short.size:
            k = int(short[0])
            raise ValueError("PushDataset: example %s has %d frames; the %s split needs %s %d" %
                             (self.example_dirs[k][1] or k, int(store.length[k]), split,
                              "more than" if self.train else "at least", self.seq_len))

    def __len__(self):
        return len(self.example_dirs)

    def epoch_examples(self, epoch):
        """the example of every position of an epoch: a permutation for train, the identity for test"""
        n = len(self)
        return permutation((self.seed, 2 + self.split_id), n, int(epoch)) if self.train else np.arange(n, dtype=np.int64)

    def _epoch_first(self, epoch):
        ex = self.epoch_examples(epoch)
        first = self.store.offset[ex]
        if self.train:
            first = first + draw_below((self.seed, self.split_id), 0, self.sequence_ids(epoch),
                                       self.store.length[ex] - self.seq_len)
        return np.ascontiguousarray(first, dtype=np.int64)
