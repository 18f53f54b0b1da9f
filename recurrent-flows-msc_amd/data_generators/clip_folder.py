"""Clips from any folder of frames, held on the device: `<root>/{train,test}/...`, no dataset-specific layout.

Sequences.  Every directory under the split that directly holds image files (.png .jpg .jpeg .bmp .pgm .ppm, decoded
with PIL, 8 bits per channel: a grey image gives one channel, anything else is converted to RGB) is one recorded
sequence, its frames in natural order (digit runs compare as numbers: `2.png` before `10.png`).  Every `<name>.npy`
holding uint8 [T, H, W], [T, H, W, 1] or [T, H, W, 3] is one sequence too.  Sequences are ordered by their path
relative to the split, component by component, in natural order.  Sizes may differ between sequences; inside one
sequence a frame of another size or channel count is a ValueError naming the file.  So BAIR's `traj_*/k/*.png` trees and
raw `class/personNN_*/` frame folders both work; nothing here claims to reproduce the reference's KTH protocol.

Ingest (clips.pack_resized_or_load).  A sequence that already has the target H x W x C is copied on the host.  Any
other one is uploaded in chunks of at most clips.RESIZE_CHUNK_BYTES of source frames and resampled on the GPU by
rfn_frames_resize_u8 (csrc/frame_resize.hip: exact integer area mean over the window ops.resize_window chooses for
`resize_mode`); there is no host resize.  The result is an ordinary FrameStore, cached under a prefix that carries
H x W x C and the mode.

Clips.  With span = (T - 1) * step + 1, a sequence shorter than the span is not eligible.  Train, clip i of epoch e has
the address s = e * len + i and draws, all by clips.draw_below(key = (seed, split id), draw, s, r):
  draw 0  which of the eligible sequences (r = their number),
  draw 1  the start frame in [0, length - span]  (r = length - span + 1),
  draw 2  the mirror bit, only when `flip` is on (r = 2),
  draw 3  the time-reversal bit, only when `reverse` is on (r = 2).
len() is the number of eligible sequences, or `length`.  Test: clip i is the i-th eligible sequence from its frame 0,
unflagged, the same every epoch.  A clip depends on (seed, epoch, position) alone: not on the batch size, the rank or
the world size.  A batch is one launch of rfn_clip_gather_aug_u8_f32 reading its rows of the epoch's tables."""
import os
import re

import numpy as np
import torch

from .clips import ClipDataset, draw_below, pack_resized_or_load

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".pgm", ".ppm")


def natural_key(name):
    """sort key under which digit runs compare as numbers: 'f2' < 'f10'"""
    parts = re.split(r"(\d+)", name)
    return tuple(int(p) if k % 2 else p for k, p in enumerate(parts))


def _path_key(rel):
    return tuple(natural_key(c) for c in rel.split("/"))


def list_sequences(root, split):
    """[(relative path, [files])] of the sequences under <root>/<split>, in order: a directory of images with its frames
    in natural order, or one .npy file"""
    top = os.path.join(root, split)
    if not os.path.isdir(top):
        raise FileNotFoundError("ClipFolder: %s is not a directory (the layout is <root>/{train,test}/...)" % top)
    found = []
    for d, _, names in os.walk(top):
        rel = os.path.relpath(d, top).replace(os.sep, "/")
        images = sorted((n for n in names if n.lower().endswith(IMAGE_EXTENSIONS)), key=natural_key)
        if images:
            found.append((rel, [os.path.join(d, n) for n in images]))
        for n in names:
            if n.lower().endswith(".npy"):
                found.append((n if rel == "." else rel + "/" + n, [os.path.join(d, n)]))
    found.sort(key=lambda s: _path_key(s[0]))
    return found


def _decode(path):
    from PIL import Image   # only needed when frames are decoded: a matching cache never gets here
    with Image.open(path) as im:
        if im.mode == "L":
            return np.asarray(im)[:, :, None]
        return np.asarray(im.convert("RGB"))


def read_sequence(files):
    """uint8 [T, Hs, Ws, Cs] of one sequence of list_sequences"""
    if len(files) == 1 and files[0].lower().endswith(".npy"):
        a = np.load(files[0], allow_pickle=False)
        if a.ndim == 3:
            a = a[:, :, :, None]
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] not in (1, 3):
            raise ValueError("ClipFolder: %s holds %s %s, expected uint8 [T, H, W], [T, H, W, 1] or [T, H, W, 3]" %
                             (files[0], a.dtype, a.shape))
        return a
    first = _decode(files[0])
    out = np.empty((len(files),) + first.shape, dtype=np.uint8)
    out[0] = first
    for k in range(1, len(files)):
        a = _decode(files[k])
        if a.shape != first.shape:
            raise ValueError("ClipFolder: %s is %dx%dx%d, the sequence began with %dx%dx%d (%s)" %
                             ((files[k],) + a.shape + first.shape + (files[0],)))
        out[k] = a
    return out


class ClipFolder(ClipDataset):
    """Clips of `seq_len` frames, `step` apart, of the sequences under <data_root>/{train,test}, as [C, H, W] = `channels`
    x `height` x `width` frames.  `flip` / `reverse` switch the two augmentations on (train split only); `resize_mode`
    is ops.resize_window's; `seed` (None = 0) keys the draws; `device` is where the frames live (default the current
    GPU); `cache` a file prefix for the packed store; `length` overrides the number of train clips per epoch."""

    def __init__(self, train, data_root, seq_len=20, channels=1, height=64, width=64, step=1, flip=False, reverse=False,
                 resize_mode="crop", seed=None, device=None, cache=None, length=None):
        from rfn_hip import ops
        H, W, C = int(height), int(width), int(channels)
        if C not in (1, 3) or H < 1 or W < 1:
            raise ValueError("ClipFolder: frames are 1 or 3 channels of H, W >= 1; got %dx%dx%d" % (C, H, W))
        if isinstance(step, bool) or int(step) != step or step < 1:
            raise ValueError("ClipFolder: step must be an integer >= 1, got %r" % (step,))
        ops.resize_window(1, 1, H, W, resize_mode)   # (an unknown mode is refused here, not at the first odd sequence)
        self.data_root, self.split = str(data_root), "train" if train else "test"
        self.step, self.resize_mode = int(step), resize_mode
        self.sequences = list_sequences(self.data_root, self.split)
        if not self.sequences:
            raise ValueError("ClipFolder: no sequence (a directory of %s files, or a .npy) under %s" %
                             (" ".join(IMAGE_EXTENSIONS), os.path.join(self.data_root, self.split)))
        files = [f for _, f in self.sequences]
        store = pack_resized_or_load(cache, self.data_root, files, lambda n: read_sequence(files[n]), H, W, C,
                                     lambda Hs, Ws: ops.resize_window(Hs, Ws, H, W, resize_mode), device=device)
        self._setup(store, seq_len, C, train, seed, device)
        self.span = (self.seq_len - 1) * self.step + 1
        self.eligible = np.nonzero(store.length >= self.span)[0].astype(np.int64)
        if not self.eligible.size:
            raise ValueError("ClipFolder: no %s sequence under %s has the %d frames a clip spans (%d frames, %d apart)" %
                             (self.split, self.data_root, self.span, self.seq_len, self.step))
        self.flip, self.reverse = bool(flip) and self.train, bool(reverse) and self.train
        self.length = int(self.eligible.size) if length is None or not self.train else int(length)
        self._flags = (None, None, None)

    def __len__(self):
        return self.length

    def epoch_choices(self, epoch):
        """(sequence, start frame, flags) of every clip of an epoch: int64, int64, int32 [len(self)]"""
        n = len(self)
        if not self.train:
            return self.eligible.copy(), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        from rfn_hip import ops
        key, ids = (self.seed, self.split_id), self.sequence_ids(epoch)
        seq = self.eligible[draw_below(key, 0, ids, self.eligible.size)]
        start = draw_below(key, 1, ids, self.store.length[seq] - self.span + 1)
        flags = np.zeros(n, dtype=np.int32)
        if self.flip:
            flags |= (ops.CLIP_MIRROR * draw_below(key, 2, ids, 2)).astype(np.int32)
        if self.reverse:
            flags |= (ops.CLIP_REVERSE * draw_below(key, 3, ids, 2)).astype(np.int32)
        return seq, start, flags

    def _epoch_first(self, epoch):
        seq, start, _ = self.epoch_choices(epoch)
        return np.ascontiguousarray(self.store.offset[seq] + start, dtype=np.int64)

    def epoch_flags(self, epoch):
        """host int32 [len(self)]: the augmentation bits of clip i of `epoch` (all 0 on the test split)"""
        epoch = int(epoch) if self.train else 0
        if self._flags[0] != epoch:
            self._flags = (epoch, np.ascontiguousarray(self.epoch_choices(epoch)[2]), None)
        return self._flags[1]

    def device_flags(self, epoch):
        """epoch_flags(epoch) on the store's device: one upload per epoch (what ClipLoader hands to gather)"""
        host = self.epoch_flags(epoch)
        if self._flags[2] is None:
            self._flags = (self._flags[0], host, torch.from_numpy(host).to(self.store.device_frames(self._device).device))
        return self._flags[2]

    def gather(self, first, flags=None):
        """the clips starting at the store indices `first` (int64 device tensor [B]) with the bits `flags` (int32 [B] or
        None): fresh [B, T, C, H, W] float32"""
        from rfn_hip import ops
        return ops.clip_gather_aug(self.store.device_frames(self._device), first, self.seq_len, self.channels,
                                   step=self.step, flags=flags)

    def __getitem__(self, index):
        n = len(self)
        if not -n <= index < n:
            raise IndexError("ClipFolder index %d out of range for %d clips" % (index, n))
        index %= n
        return self.gather(self.device_table(0)[index:index + 1], self.device_flags(0)[index:index + 1])[0]
