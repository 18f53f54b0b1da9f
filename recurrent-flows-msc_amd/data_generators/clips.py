"""What the two file-backed datasets (bair_push.py, kth.py) share: the packed frame store, the addressed random draws
that choose the clips of an epoch, and the device loader.

- `FrameStore`: every frame of a split as one uint8 tensor [F, H, W, Cs] (channel-interleaved, the way an image decoder
  leaves it) plus int64 `offset[n]`, `length[n]` per recorded sequence.  `save` / `load` keep it as
  `<prefix>.frames.npy` and `<prefix>.index.npz`; the index carries a fingerprint of the source files (sorted relative
  paths and byte sizes), so that a changed dataset is packed again.  The frames are uploaded once per device; there
  is no host fallback.
- Draws: Philox4x64-10, word 0, bounded by Lemire's multiply-shift with rejection (retry starts at 0) -- the scheme
  of csrc/moving_mnist.hip, here vectorised in numpy on the host.  A dataset computes the first-frame index of every
  clip of an epoch at once (`epoch_table`); the table is uploaded as one int64 tensor and a batch is one launch of
  rfn_clip_gather_u8_f32 (csrc/clip_gather.hip) reading its B rows: no per-batch copy, no synchronisation.
- `ClipLoader`: MovingMNISTLoader's contract over such a dataset.  A dataset that has `device_flags(epoch)`
  (clip_folder.py: the augmentation bits of the epoch's clips) is handed its rows of them along with the first frames.
- `pack_resized_or_load`: pack_or_load for sequences of any frame size (clip_folder.py), resampled on the GPU."""
import os

import numpy as np
import torch

SPLIT_TRAIN, SPLIT_TEST = 0, 1

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_PHILOX_M = (np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157))
_PHILOX_W = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B))


# ------------------------------------------------------------------------------------------------- addressed draws
def _mulhilo(a, b):
    """(high, low) 64-bit halves of the 128-bit products of two uint64 arrays"""
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    return p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32), (p00 & _M32) | (mid << _S32)


def philox_word0(c0, c1, c2, c3, key):
    """word 0 of the Philox4x64-10 blocks at counters (c0, c1, c2, c3) (uint64 arrays of one shape) under `key`"""
    k0 = np.full(c0.shape, key[0], dtype=np.uint64)
    k1 = np.full(c0.shape, key[1], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(np.broadcast_to(_PHILOX_M[0], c0.shape), c0)
            hi1, lo1 = _mulhilo(np.broadcast_to(_PHILOX_M[1], c2.shape), c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0, k1 = k0 + _PHILOX_W[0], k1 + _PHILOX_W[1]
    return c0


def draw_below(key, draw, seq, r):
    """uniform integers in [0, r) (int64 array): block (draw, retry, seq, 0) under `key`, word 0, mapped by Lemire's
    multiply-shift; a rejected word repeats the draw with retry + 1.  `draw`, `seq`, `r` broadcast; every r >= 1."""
    draw, seq, r = (np.ascontiguousarray(v).astype(np.uint64) for v in np.broadcast_arrays(draw, seq, r))
    shape = r.shape
    draw, seq, r = draw.reshape(-1), seq.reshape(-1), r.reshape(-1)
    if r.size and int(r.min()) < 1:
        raise ValueError("draw_below: empty range")
    out = np.zeros(r.shape, dtype=np.int64)
    todo = np.arange(r.size)
    retry = 0
    with np.errstate(over="ignore"):
        while todo.size:
            d, s, rr = draw[todo], seq[todo], r[todo]
            x = philox_word0(d, np.full(d.shape, retry, dtype=np.uint64), s, np.zeros(d.shape, dtype=np.uint64), key)
            hi, lo = _mulhilo(x, rr)
            ok = ~((lo < rr) & (lo < (np.uint64(0) - rr) % rr))
            out[todo[ok]] = hi[ok].astype(np.int64)
            todo = todo[~ok]
            retry += 1
    return out.reshape(shape)


def permutation(key, n, epoch):
    """Fisher-Yates from the identity: for i = n-1 .. 1, j = randint(0, i + 1) at counter (i, retry, epoch, 0), swap"""
    perm = np.arange(n, dtype=np.int64)
    if n > 1:
        i = np.arange(1, n, dtype=np.int64)
        j = draw_below(key, i, epoch, i + 1)
        for a in range(n - 1, 0, -1):
            b = j[a - 1]
            perm[a], perm[b] = perm[b], perm[a]
    return perm


# ------------------------------------------------------------------------------------------------- the packed store
def fingerprint(root, paths):
    """(sorted relative paths, their byte sizes) of the source files of a store"""
    rel = sorted({os.path.relpath(p, root).replace(os.sep, "/") for p in paths})
    return rel, [os.path.getsize(os.path.join(root, p)) for p in rel]


class FrameStore(object):
    """uint8 frames [F, H, W, Cs] of `len(offset)` recorded sequences: sequence n is frames offset[n] ..
    offset[n] + length[n] - 1.  `paths`, `sizes`: the fingerprint of the files it was packed from (empty when built
    from arrays)."""

    def __init__(self, frames, offset, length, paths=(), sizes=()):
        frames = torch.as_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or int(frames.shape[3]) not in (1, 3):
            raise ValueError("FrameStore: frames must be uint8 [F, H, W, 1 or 3], got %s %s" %
                             (frames.dtype, tuple(frames.shape)))
        offset, length = np.asarray(offset, dtype=np.int64).reshape(-1), np.asarray(length, dtype=np.int64).reshape(-1)
        if offset.shape != length.shape:
            raise ValueError("FrameStore: %d offsets for %d lengths" % (offset.size, length.size))
        if offset.size and (int(offset.min()) < 0 or int(length.min()) < 0 or
                            int((offset + length).max()) > int(frames.shape[0])):
            raise ValueError("FrameStore: a sequence leaves the %d stored frames" % int(frames.shape[0]))
        self.frames, self.offset, self.length = frames.contiguous(), offset, length
        self.paths, self.sizes = [str(p) for p in paths], [int(s) for s in sizes]
        self._device = {}

    @classmethod
    def from_arrays(cls, frames, offset, length):
        return cls(frames, offset, length)

    n_frames = property(lambda self: int(self.frames.shape[0]))
    H = property(lambda self: int(self.frames.shape[1]))
    W = property(lambda self: int(self.frames.shape[2]))
    Cs = property(lambda self: int(self.frames.shape[3]))

    def __len__(self):
        return int(self.offset.size)

    def save(self, prefix):
        os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
        np.save(prefix + ".frames.npy", self.frames.numpy())
        np.savez(prefix + ".index.npz", offset=self.offset, length=self.length,
                 paths=np.array(self.paths, dtype=np.str_), sizes=np.array(self.sizes, dtype=np.int64))

    @classmethod
    def load(cls, prefix):
        with np.load(prefix + ".index.npz", allow_pickle=False) as idx:
            offset, length, paths, sizes = idx["offset"], idx["length"], idx["paths"].tolist(), idx["sizes"].tolist()
        return cls(np.load(prefix + ".frames.npy", allow_pickle=False), offset, length, paths, sizes)

    @staticmethod
    def cached(prefix, paths, sizes):
        """the store saved under `prefix` if there is one with this fingerprint, else None"""
        if prefix is None or not (os.path.isfile(prefix + ".index.npz") and os.path.isfile(prefix + ".frames.npy")):
            return None
        with np.load(prefix + ".index.npz", allow_pickle=False) as idx:
            same = idx["paths"].tolist() == list(paths) and idx["sizes"].tolist() == list(sizes)
        return FrameStore.load(prefix) if same else None

    def device_frames(self, device=None):
        """the frames on `device` (default: the current GPU), uploaded once per device"""
        dev = torch.device(device) if device is not None else torch.device("cuda")
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._device:
            self._device[dev] = self.frames.to(dev)
        return self._device[dev]


def pack_or_load(cache, root, files, decode, H, W, Cs, also=()):
    """the FrameStore of `files` ([[path, ...] per sequence], under `root`): the one saved under the prefix `cache` when
    its fingerprint (of `files` and the index files `also`) matches, else decoded frame by frame with
    `decode(path) -> uint8 [H, W, Cs]` and, with a prefix, saved there."""
    paths, sizes = fingerprint(root, [p for seq in files for p in seq] + list(also))
    store = FrameStore.cached(cache, paths, sizes)
    if store is not None:
        return store
    length = np.array([len(seq) for seq in files], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64) if len(files) else length
    frames = np.empty((int(length.sum()), H, W, Cs), dtype=np.uint8)
    k = 0
    for seq in files:
        for p in seq:
            frames[k] = decode(p)
            k += 1
    store = FrameStore(frames, offset, length, paths, sizes)
    if cache is not None:
        store.save(cache)
    return store


RESIZE_CHUNK_BYTES = 64 << 20   # most source bytes of one upload of pack_resized_or_load


def pack_resized_or_load(cache, root, files, read, H, W, C, window, device=None):
    """pack_or_load for sequences whose frames may have any size: the FrameStore [F, H, W, C] of `files` ([[path, ...]
    per sequence], under `root`), from the prefix `cache` when its fingerprint and geometry match, else built from
    `read(n) -> uint8 [T, Hs, Ws, Cs]` (sequence n, Cs in {1, 3}) and, with a prefix, saved there.  A sequence that
    already is H x W x C is copied on the host, with no kernel and no GPU.  Any other one is uploaded to `device`
    (default: the current GPU) at most RESIZE_CHUNK_BYTES of source frames at a time, at least one frame, and resampled
    there by rfn_hip.ops.frames_resize over `window(Hs, Ws) -> (y0, x0, Hc, Wc)`; there is no host resize."""
    paths, sizes = fingerprint(root, [p for seq in files for p in seq])
    store = FrameStore.cached(cache, paths, sizes)
    if store is not None and (store.H, store.W, store.Cs) == (H, W, C) and len(store) == len(files):
        return store
    parts = []
    for n in range(len(files)):
        a = np.asarray(read(n))
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] not in (1, 3):
            raise ValueError("sequence %s: frames must be uint8 [T, H, W, 1 or 3], got %s %s" %
                             (files[n][0] if files[n] else n, a.dtype, a.shape))
        if a.shape[1:] != (H, W, C) and a.shape[0]:
            from rfn_hip import ops
            dev = torch.device(device) if device is not None else torch.device("cuda")
            per = max(1, RESIZE_CHUNK_BYTES // int(np.prod(a.shape[1:])))
            win = window(a.shape[1], a.shape[2])
            a = np.concatenate([ops.frames_resize(torch.from_numpy(np.ascontiguousarray(a[k:k + per])).to(dev), H, W, C,
                                                  win).cpu().numpy() for k in range(0, a.shape[0], per)])
        parts.append(a.reshape(-1, H, W, C))
    length = np.array([p.shape[0] for p in parts], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64) if len(parts) else length
    frames = np.concatenate(parts) if parts else np.empty((0, H, W, C), dtype=np.uint8)
    store = FrameStore(frames, offset, length, paths, sizes)
    if cache is not None:
        store.save(cache)
    return store


# ------------------------------------------------------------------------------------------------- datasets, loader
class ClipDataset(object):
    """Base of PushDataset and KTH: a FrameStore, a clip length, a seed and a split.  A subclass supplies
    `_epoch_first(epoch)`: the store index of the first frame of every clip of an epoch, int64 [len(self)]."""

    def _setup(self, store, seq_len, channels, train, seed, device):
        if not seq_len >= 1:
            raise ValueError("%s: seq_len must be >= 1, got %r" % (type(self).__name__, seq_len))
        self.store, self.seq_len, self.channels, self.train = store, int(seq_len), int(channels), bool(train)
        self.seed = int(seed or 0)
        if not 0 <= self.seed < 1 << 63:
            raise ValueError("%s: seed must be in [0, 2^63), got %r" % (type(self).__name__, seed))
        self.split_id = SPLIT_TRAIN if self.train else SPLIT_TEST
        self._device = torch.device(device) if device is not None else None
        self._table = (None, None, None)

    def sequence_ids(self, epoch):
        """the addresses of the clips of an epoch: train e * len + i, test i"""
        n = len(self)
        return np.arange(n, dtype=np.int64) + (int(epoch) * n if self.train else 0)

    def epoch_table(self, epoch):
        """host int64 [len(self)]: the store index of the first frame of clip i of `epoch` (test: of any epoch)"""
        epoch = int(epoch) if self.train else 0
        if self._table[0] != epoch:
            self._table = (epoch, self._epoch_first(epoch), None)
        return self._table[1]

    def device_table(self, epoch):
        """epoch_table(epoch) on the store's device: one upload per epoch"""
        host = self.epoch_table(epoch)
        if self._table[2] is None:
            self._table = (self._table[0], host, torch.from_numpy(host).to(self.store.device_frames(self._device).device))
        return self._table[2]

    def gather(self, first):
        """the clips starting at the store indices `first` (int64 device tensor [B]): fresh [B, T, C, H, W] float32"""
        from rfn_hip import ops
        return ops.clip_gather(self.store.device_frames(self._device), first, self.seq_len, self.channels)

    def __getitem__(self, index):
        n = len(self)
        if not -n <= index < n:
            raise IndexError("%s index %d out of range for %d clips" % (type(self).__name__, index, n))
        index %= n
        return self.gather(self.device_table(0)[index:index + 1])[0]


class ClipLoader(object):
    """Device batches of a PushDataset or a KTH for the training / evaluation loops: iterating yields len(self) fresh
    [batch_size, T, C, H, W] float32 tensors in [0, 1] on the store's device, gathered on the current stream (global
    batches of world * batch_size clips, incomplete ones dropped; rank r takes rows [r * B, (r + 1) * B)).
    set_epoch(e) selects the train split's clips of epoch e; the test split is the same every epoch."""

    def __init__(self, dataset, batch_size, rank=0, world=1):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("ClipLoader: need batch_size >= 1 and 0 <= rank < world (got %r, %r, %r)" %
                             (batch_size, rank, world))
        self.dataset, self.batch_size, self.rank, self.world = dataset, int(batch_size), int(rank), int(world)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.dataset) // (self.batch_size * self.world)

    def rows(self, g):
        """the positions in the epoch of this rank's rows of global batch g"""
        lo = g * self.batch_size * self.world + self.rank * self.batch_size
        return lo, lo + self.batch_size

    def batch(self, g):
        lo, hi = self.rows(g)
        first = self.dataset.device_table(self.epoch)[lo:hi]
        flags = getattr(self.dataset, "device_flags", None)   # (ClipFolder: the augmentation bits of the epoch's clips)
        if flags is None:
            return self.dataset.gather(first)
        return self.dataset.gather(first, flags(self.epoch)[lo:hi])

    def __iter__(self):
        for g in range(len(self)):
            yield self.batch(g)
