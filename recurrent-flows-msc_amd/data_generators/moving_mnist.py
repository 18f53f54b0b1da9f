"""Stochastic Moving MNIST (SM-MNIST) rendered on the GPU: the dataset of the reference's canonical configuration
(data_generators/stochasticMovingMnist.py:9-127, driven by RFN/trainer.py:112-131 and :155-161).

- `load_mnist_digits(root, train)` reads the 28x28 uint8 MNIST digits from the files torchvision leaves under the
  reference's root (`Mnist/`): `MNIST/raw/{train,t10k}-images-idx3-ubyte[.gz]` or `MNIST/processed/{training,test}.pt`.
  It never downloads anything.
- `MovingMNIST` keeps the reference's constructor; the digit table lives on the device and a whole batch is one launch
  of rfn_moving_mnist_render_f32 (csrc/moving_mnist.hip).  Each sequence is the reference's walk draw for draw, with
  every random draw addressed by (seed, split, sequence id, digit, draw number) instead of numpy's global stream.
- `MovingMNIST_synchronized` is the reference's dataset for its parameter analysis: every sequence shares the digits'
  trajectories (rfn_moving_mnist_sync_render_f32) and `hit_boundary` records the wall contacts per frame.
- `MovingMNISTLoader` is what the Solver iterates in place of a DataLoader: device batches, no worker processes.
  Sequence ids: train split, sequence i of epoch e -> e * len + i (every epoch sees fresh sequences); test split -> i
  whatever the epoch (a fixed evaluation set).  Rank r of w renders rows [r * B, (r + 1) * B) of each global batch of
  w * B sequences, so the union over ranks is the one-rank batch."""
import gzip
import os

import numpy as np
import torch

SPLIT_TRAIN, SPLIT_TEST = 0, 1
DIGIT_SIZE = 28
MAX_DIGITS = 8


def _read_idx_images(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read()
    if len(raw) < 16:
        raise ValueError("%s: truncated idx header (%d bytes)" % (path, len(raw)))
    magic, n, h, w = (int.from_bytes(raw[i:i + 4], "big") for i in (0, 4, 8, 12))
    if magic != 2051:
        raise ValueError("%s: bad idx magic %d (expected 2051, unsigned byte images of rank 3)" % (path, magic))
    if (h, w) != (DIGIT_SIZE, DIGIT_SIZE):
        raise ValueError("%s: images are %dx%d, expected %dx%d" % (path, h, w, DIGIT_SIZE, DIGIT_SIZE))
    need = 16 + n * h * w
    if len(raw) != need:
        raise ValueError("%s: %d bytes, the header promises %d images (%d bytes)%s" %
                         (path, len(raw), n, need, " -- truncated" if len(raw) < need else ""))
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(n, h, w).copy())


def _read_processed(path):
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if not (isinstance(obj, (tuple, list)) and len(obj) == 2 and isinstance(obj[0], torch.Tensor)):
        raise ValueError("%s: expected torchvision's (data, targets) tuple" % path)
    data = obj[0]
    if data.dtype != torch.uint8 or data.dim() != 3 or tuple(data.shape[1:]) != (DIGIT_SIZE, DIGIT_SIZE):
        raise ValueError("%s: data must be uint8 [N, 28, 28], got %s %s" % (path, data.dtype, tuple(data.shape)))
    return data.contiguous()


def mnist_candidate_paths(root, train):
    """the files load_mnist_digits tries, in order"""
    raw = os.path.join(root, "MNIST", "raw", ("train" if train else "t10k") + "-images-idx3-ubyte")
    return [raw, raw + ".gz", os.path.join(root, "MNIST", "processed", "training.pt" if train else "test.pt")]


def load_mnist_digits(root, train):
    """uint8 [N, 28, 28] MNIST images of the train (60 000) or test (10 000) split from local files under `root`, in
    torchvision's layouts (see mnist_candidate_paths).  Labels are not read.  Nothing is downloaded: a missing dataset,
    a bad magic number, a truncated file or a wrong shape raises."""
    paths = mnist_candidate_paths(root, train)
    for p in paths:
        if os.path.isfile(p):
            data = _read_processed(p) if p.endswith(".pt") else _read_idx_images(p)
            if data.shape[0] < 1:
                raise ValueError("%s: holds no images" % p)
            return data
    raise FileNotFoundError("MNIST %s images not found; tried: %s. No download is attempted: place torchvision's MNIST "
                            "files there (or pass --mnist_root)." % ("train" if train else "test", ", ".join(paths)))


class MovingMNIST(object):
    """The reference's MovingMNIST (stochasticMovingMnist.py:9-127) rendered on the GPU.  Same constructor arguments,
    plus `device` (where the digit table lives; default the current GPU) and `length` (number of sequences per epoch;
    default the MNIST split size, as the reference's __len__).  `seed` (None = 0) keys the random draws; the train and
    the test split draw from different streams.  __getitem__(i) returns sequence i of epoch 0 as a device tensor
    [T, C, S, S] (C = 3 with three_channels); MovingMNISTLoader renders whole batches."""

    def __init__(self, train, data_root, seq_len=20, num_digits=2, image_size=32, digit_size=28, deterministic=True,
                 three_channels=True, step_length=4, normalize=False, make_target=False, set_starting_position=False,
                 seed=None, device=None, length=None):
        if digit_size != DIGIT_SIZE:
            raise ValueError("MovingMNIST: digit_size must be 28 (the reference's Resize(28) is then the identity; "
                             "other sizes would need its Lanczos resize), got %r" % (digit_size,))
        if not image_size > DIGIT_SIZE:
            raise ValueError("MovingMNIST: image_size must exceed the digit size 28, got %r" % (image_size,))
        if not 1 <= num_digits <= MAX_DIGITS:
            raise ValueError("MovingMNIST: num_digits must be in [1, %d], got %r" % (MAX_DIGITS, num_digits))
        if not step_length >= 1:
            raise ValueError("MovingMNIST: step_length must be >= 1, got %r" % (step_length,))
        if not seq_len >= 1:
            raise ValueError("MovingMNIST: seq_len must be >= 1, got %r" % (seq_len,))
        for flag, nm in ((normalize, "normalize"), (make_target, "make_target"),
                         (set_starting_position, "set_starting_position")):
            if flag:
                raise NotImplementedError("MovingMNIST: %s=True is not supported" % nm)
        self.train, self.seq_len, self.num_digits, self.image_size = bool(train), int(seq_len), int(num_digits), int(image_size)
        self.digit_size, self.deterministic, self.three_channels = DIGIT_SIZE, bool(deterministic), bool(three_channels)
        self.step_length, self.seed = int(step_length), int(seed or 0)
        if not 0 <= self.seed < 1 << 63:
            raise ValueError("MovingMNIST: seed must be in [0, 2^63), got %r" % (seed,))
        self.channels = 3 if self.three_channels else 1
        self.split = SPLIT_TRAIN if self.train else SPLIT_TEST
        self.digits = load_mnist_digits(data_root, self.train)
        self.N = int(self.digits.shape[0])
        self.length = self.N if length is None else int(length)
        self._device = torch.device(device) if device is not None else None
        self._tables = {}

    def __len__(self):
        return self.length

    def table(self):
        """the uint8 digit table on the constructor's device (default: the current GPU), uploaded once per device"""
        dev = self._device if self._device is not None else torch.device("cuda")
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._tables:
            self._tables[dev] = self.digits.to(dev)
        return self._tables[dev]

    def sequence_id(self, i, epoch=0):
        """the address of sequence i of an epoch: train e * len + i, test i"""
        return (int(epoch) * self.length + int(i)) if self.train else int(i)

    def render(self, first_id, count, trajectories=False):
        """`count` consecutive sequences from id `first_id` as one fresh [count, T, C, S, S] float32 device tensor"""
        from rfn_hip import ops
        return ops.moving_mnist_render(self.table(), count, self.seq_len, self.channels, self.image_size,
                                       self.num_digits, self.step_length, self.deterministic, self.seed, self.split,
                                       first_id, trajectories=trajectories)

    def __getitem__(self, index):
        if not -self.length <= index < self.length:
            raise IndexError("MovingMNIST index %d out of range for %d sequences" % (index, self.length))
        return self.render(self.sequence_id(index % self.length), 1)[0]


class MovingMNIST_synchronized(MovingMNIST):
    """The reference's MovingMNIST_synchronized (stochasticMovingMnist.py:131-248), "synchronized motion for parameter
    analysis", rendered on the GPU by rfn_moving_mnist_sync_render_f32: all sequences share one trajectory per digit
    (drawn start position, velocity (3, 3), the wall bounces of MovingMNIST with step_length / deterministic) and
    only the digit identities depend on the sequence id.  The constructor is the reference's plus `device` and
    `length`, with MovingMNIST's argument checks; render / sequence_id / __len__ / __getitem__ are MovingMNIST's, so
    MovingMNISTLoader takes it unchanged.  `hit_boundary` is the reference's float64 numpy array [seq_len]: entry t is
    n + 1 for the last digit n clamped at a wall on frame t, 0 if none; it is computed on first use from a
    one-sequence render (the reference fills it as a side effect of __getitem__)."""

    def __init__(self, train, data_root, seq_len=20, num_digits=2, image_size=32, digit_size=28, deterministic=True,
                 three_channels=True, step_length=4, normalize=False, make_target=False, seed=None, device=None,
                 length=None):
        super(MovingMNIST_synchronized, self).__init__(
            train, data_root, seq_len=seq_len, num_digits=num_digits, image_size=image_size, digit_size=digit_size,
            deterministic=deterministic, three_channels=three_channels, step_length=step_length, normalize=normalize,
            make_target=make_target, seed=seed, device=device, length=length)
        self._hit_boundary = None

    def render(self, first_id, count, trajectories=False, hits=False):
        """MovingMNIST.render of the synchronized walk; with hits=True also the int32 [count, T] hit table"""
        from rfn_hip import ops
        return ops.moving_mnist_sync_render(self.table(), count, self.seq_len, self.channels, self.image_size,
                                            self.num_digits, self.step_length, self.deterministic, self.seed,
                                            self.split, first_id, trajectories=trajectories, hits=hits)

    @property
    def hit_boundary(self):
        if self._hit_boundary is None:
            _, hit = self.render(0, 1, hits=True)
            self._hit_boundary = hit[0].cpu().numpy().astype(np.float64)
        return self._hit_boundary

    def __boundary__(self):
        return self.hit_boundary


class MovingMNISTLoader(object):
    """Device batches of a MovingMNIST for the training / evaluation loops: iterating yields len(self) fresh
    [batch_size, T, C, S, S] float32 tensors on the current device, rendered on the current stream (global batches of
    world * batch_size sequences, incomplete ones dropped; this rank's rows only).  set_epoch(e) selects the train
    split's sequences of epoch e; the test split is the same every epoch."""

    def __init__(self, dataset, batch_size, rank=0, world=1):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("MovingMNISTLoader: need batch_size >= 1 and 0 <= rank < world (got %r, %r, %r)" %
                             (batch_size, rank, world))
        self.dataset, self.batch_size, self.rank, self.world = dataset, int(batch_size), int(rank), int(world)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.dataset) // (self.batch_size * self.world)

    def batch(self, g):
        """this rank's rows of global batch g of the current epoch"""
        first = self.dataset.sequence_id(g * self.batch_size * self.world + self.rank * self.batch_size, self.epoch)
        return self.dataset.render(first, self.batch_size)

    def __iter__(self):
        for g in range(len(self)):
            yield self.batch(g)
