"""Frames made or moved on the GPU: the Moving MNIST renderers, the clip gathers and the resize at ingest; wrappers of
csrc/moving_mnist.hip, csrc/clip_gather.hip and csrc/frame_resize.hip.  rfn_hip.ops re-exports the public names."""
import torch

from . import lib as L
from .args import check_u63


def _moving_mnist_args(fn, digits, B, T, C, S, num_digits, step_length, seed, split, first_id):
    """the argument checks the two Moving MNIST renderers share; returns the contiguous digits and the integers"""
    if not isinstance(digits, torch.Tensor) or digits.dtype != torch.uint8:
        raise TypeError("%s: digits must be a uint8 tensor, got %s" %
                        (fn, digits.dtype if isinstance(digits, torch.Tensor) else type(digits).__name__))
    if digits.dim() != 3 or tuple(digits.shape[1:]) != (28, 28) or digits.shape[0] < 1:
        raise ValueError("%s: digits must be [N >= 1, 28, 28], got %s" % (fn, tuple(digits.shape),))
    if not digits.is_cuda:
        raise RuntimeError("rfn_hip kernels need device tensors; digits is on %s (no CPU fallback)" % digits.device)
    B, T, C, S, nd, L_, seed, split, first_id = (int(v) for v in (B, T, C, S, num_digits, step_length, seed, split,
                                                                  first_id))
    if B < 0 or T < 1 or C < 1:
        raise ValueError("%s: need B >= 0, T >= 1, C >= 1 (got %d, %d, %d)" % (fn, B, T, C))
    if not 28 < S <= 4096:
        raise ValueError("%s: image size %d must exceed the digit size 28 (and be <= 4096)" % (fn, S))
    if not 1 <= nd <= 8:
        raise ValueError("%s: num_digits %d not in [1, 8]" % (fn, nd))
    if not 1 <= L_ <= 1 << 20:
        raise ValueError("%s: step_length %d must be >= 1" % (fn, L_))
    check_u63(fn, seed=seed, split=split, first_id=first_id)
    if B * T > 0x7fffffff:
        raise ValueError("%s: B * T = %d frames exceed one launch" % (fn, B * T))
    return digits.contiguous(), B, T, C, S, nd, L_, seed, split, first_id


def _moving_mnist(sync, digits, B, T, C, S, num_digits, step_length, deterministic, seed, split, first_id, trajectories,
                  hits):
    """the body the two Moving MNIST renderers share: checks, fresh tensors, one launch, out or (out[, traj][, hit]).
    sync: the synchronized renderer, the only one with a hit table among its arguments."""
    fn, entry, label = (("moving_mnist_sync_render", "rfn_moving_mnist_sync_render_f32", "moving_mnist_sync") if sync else
                        ("moving_mnist_render", "rfn_moving_mnist_render_f32", "moving_mnist"))
    digits, B, T, C, S, nd, L_, seed, split, first_id = _moving_mnist_args(
        fn, digits, B, T, C, S, num_digits, step_length, seed, split, first_id)
    out = torch.empty((B, T, C, S, S), device=digits.device, dtype=torch.float32)
    traj = torch.empty((B, nd, T, 3), device=digits.device, dtype=torch.int64) if trajectories else None
    hit = torch.empty((B, T), device=digits.device, dtype=torch.int32) if hits else None
    if B:
        hit_arg = (hit.data_ptr() if hit is not None else 0,) if sync else ()
        with torch.cuda.device(digits.device):
            L.call(entry, digits.data_ptr(), int(digits.shape[0]), L.dev(out),
                   traj.data_ptr() if traj is not None else None, *hit_arg, B, T, C, S, nd, L_,
                   1 if deterministic else 0, seed, split, first_id,
                   meta=("shell", label, 0.0, "%dx%dx%dx%dx%d" % (B, T, C, S, S), 4.0 * out.numel()))
    extra = tuple(v for v in (traj, hit) if v is not None)
    return (out,) + extra if extra else out


def moving_mnist_render(digits, B, T, C, S, num_digits, step_length, deterministic, seed, split, first_id,
                        trajectories=False):
    """Stochastic Moving MNIST batch rendered on the GPU (rfn_moving_mnist_render_f32: the reference's
    MovingMNIST.__getitem__, stochasticMovingMnist.py:48-127, with addressed random draws): a fresh float32 tensor
    [B, T, C, S, S] in [0, 1] on the digits' device, sequence b having the id first_id + b; with trajectories=True also
    the int64 [B, num_digits, T, 3] (digit index, y, x) of every digit and frame.  `digits`: uint8 [N, 28, 28] device
    table.  One launch on the current stream; no CPU fallback."""
    return _moving_mnist(False, digits, B, T, C, S, num_digits, step_length, deterministic, seed, split, first_id,
                         trajectories, False)


def moving_mnist_sync_render(digits, B, T, C, S, num_digits, step_length, deterministic, seed, split, first_id,
                             trajectories=False, hits=False):
    """Synchronized Moving MNIST batch (rfn_moving_mnist_sync_render_f32: the reference's MovingMNIST_synchronized,
    stochasticMovingMnist.py:131-248): moving_mnist_render's arguments and outputs, but all sequences share one
    trajectory per digit (start position drawn, velocity (3, 3), the bounces with step_length / deterministic) and only
    the digit identities depend on the sequence id.  With hits=True also the int32 [B, T] hit table: the largest
    n + 1 over the digits clamped at a wall on frame t, 0 if none (every row the same).  Returns out, or the tuple
    (out[, traj][, hit]).  One launch on the current stream; no CPU fallback."""
    return _moving_mnist(True, digits, B, T, C, S, num_digits, step_length, deterministic, seed, split, first_id,
                         trajectories, hits)


def _clip_gather_args(fn, store, first, T, C):
    """the argument checks the two clip gathers share; returns the contiguous tensors and the integers"""
    for t, nm, dt in ((store, "store", torch.uint8), (first, "first", torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError("%s: %s must be a %s tensor, got %s" %
                            (fn, nm, str(dt).replace("torch.", ""),
                             t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
    if store.dim() != 4 or min(int(d) for d in store.shape[1:3]) < 1:
        raise ValueError("%s: store must be [F, H >= 1, W >= 1, Cs], got %s" % (fn, tuple(store.shape),))
    if first.dim() != 1:
        raise ValueError("%s: first must be [B], got %s" % (fn, tuple(first.shape),))
    F, H, W, Cs = (int(d) for d in store.shape)
    B, T, C = int(first.shape[0]), int(T), int(C)
    if T < 1:
        raise ValueError("%s: need T >= 1, got %d" % (fn, T))
    if (C, Cs) not in ((1, 1), (3, 1), (3, 3)):
        raise ValueError("%s: %d output channels from %d stored ones (C == Cs in {1, 3}, or 3 copies of 1)" %
                         (fn, C, Cs))
    for t, nm in ((store, "store"), (first, "first")):
        if not t.is_cuda:
            raise ValueError("%s: %s is on %s; the kernel needs device tensors (no CPU fallback)" % (fn, nm, t.device))
    if store.device != first.device:
        raise ValueError("%s: store is on %s, first on %s" % (fn, store.device, first.device))
    if B and F < 1:
        raise ValueError("%s: the store holds no frame" % fn)
    chunks = -(-H * W // 1024)
    if H * W > 0x7fffffff // 4 or B * T * chunks > 0x7fffffff:
        raise ValueError("%s: %d clips of %d frames of %dx%d exceed one launch" % (fn, B, T, H, W))
    return store.contiguous(), first.contiguous(), F, H, W, Cs, B, T, C


def _clip_gather_launch(store, first, F, H, W, Cs, B, T, C, aug=None):
    """the tail the two clip gathers share: the fresh [B, T, C, H, W] batch and the one launch that fills it.  aug: None
    for the plain kernel, (flags or None, step) for the augmenting one (2-6 % slower: DESIGN.md section 27)."""
    out = torch.empty((B, T, C, H, W), device=store.device, dtype=torch.float32)
    if B:
        shape, nbytes = "%dx%dx%dx%dx%d" % (B, T, C, H, W), 4.0 * out.numel() + float(B * T * H * W * Cs)
        with torch.cuda.device(store.device):
            if aug is None:
                L.call("rfn_clip_gather_u8_f32", store.data_ptr(), F, first.data_ptr(), L.dev(out), B, T, C, Cs, H, W,
                       meta=("shell", "clip_gather", 0.0, shape, nbytes))
            else:
                flags, step = aug
                L.call("rfn_clip_gather_aug_u8_f32", store.data_ptr(), F, first.data_ptr(),
                       flags.data_ptr() if flags is not None else None, L.dev(out), B, T, C, Cs, H, W, step,
                       meta=("shell", "clip_gather_aug", 0.0, shape, nbytes))
    return out


def clip_gather(store, first, T, C):
    """Clips of a device-resident frame store as one float32 batch (rfn_clip_gather_u8_f32: what the reference's
    PushDataset / KTH __getitem__ and the DataLoader's collation produce, bair_push.py:66-109, kth.py:34-65,
    trainer.py:132-161): a fresh [B, T, C, H, W] tensor on the store's device, clip b being frames first[b] ..
    first[b] + T - 1 as float32(byte) / 255.  `store`: uint8 [F, H, W, Cs] device tensor, Cs in {1, 3}; `first`: int64
    [B] on the same device; C == Cs, or C == 3 copies of a one-channel store.  A clip that would leave the store is
    NaN (nothing is read).  One launch on the current stream; no CPU fallback."""
    return _clip_gather_launch(*_clip_gather_args("clip_gather", store, first, T, C))


CLIP_MIRROR, CLIP_REVERSE = 1, 2   # the bits of clip_gather_aug's flags


def clip_gather_aug(store, first, T, C, step=1, flags=None):
    """clip_gather with a temporal stride and per-clip augmentations (rfn_clip_gather_aug_u8_f32): clip b is the T
    frames first[b], first[b] + step, ...; `flags`: None, or int32 [B] on the store's device, bit 0 (CLIP_MIRROR)
    mirrors the clip's frames in x, bit 1 (CLIP_REVERSE) reverses its frames in time, other bits are ignored.  A clip
    with first[b] < 0 or first[b] + (T - 1) * step + 1 > F is NaN (nothing is read).  With step 1 and no flags the
    result is clip_gather's bit for bit.  One launch on the current stream; no CPU fallback."""
    store, first, F, H, W, Cs, B, T, C = _clip_gather_args("clip_gather_aug", store, first, T, C)
    if isinstance(step, bool) or not isinstance(step, int) or not 1 <= step <= 0x7fffffff:
        raise ValueError("clip_gather_aug: step must be an int in [1, 2^31), got %r" % (step,))
    if flags is not None:
        if not isinstance(flags, torch.Tensor) or flags.dtype != torch.int32:
            raise TypeError("clip_gather_aug: flags must be an int32 tensor, got %s" %
                            (flags.dtype if isinstance(flags, torch.Tensor) else type(flags).__name__))
        if tuple(flags.shape) != (B,):
            raise ValueError("clip_gather_aug: flags must be [%d], got %s" % (B, tuple(flags.shape)))
        if flags.device != store.device:
            raise ValueError("clip_gather_aug: store is on %s, flags on %s (no CPU fallback)" %
                             (store.device, flags.device))
        flags = flags.contiguous()
    return _clip_gather_launch(store, first, F, H, W, Cs, B, T, C, aug=(flags, step))


RESIZE_MAX_SIDE = 32768   # rfn_frames_resize_u8's largest source or target side


def resize_window(Hs, Ws, H, W, mode="crop"):
    """the crop window (y0, x0, Hc, Wc) of an Hs x Ws frame for frames_resize to H x W: "stretch" is the whole frame,
    "crop" the largest centred window of the target's aspect ratio (the longer side is cut; integer floor)."""
    Hs, Ws, H, W = int(Hs), int(Ws), int(H), int(W)
    if min(Hs, Ws, H, W) < 1:
        raise ValueError("resize_window: sizes must be >= 1, got %dx%d -> %dx%d" % (Hs, Ws, H, W))
    if mode == "stretch":
        return 0, 0, Hs, Ws
    if mode != "crop":
        raise ValueError("resize_window: mode must be 'crop' or 'stretch', got %r" % (mode,))
    if Ws * H >= Hs * W:
        Hc, Wc = Hs, max(1, Hs * W // H)
    else:
        Hc, Wc = max(1, Ws * H // W), Ws
    return (Hs - Hc) // 2, (Ws - Wc) // 2, Hc, Wc


def frames_resize(src, H, W, Cd, window=None):
    """Frames resampled into another geometry on the GPU (rfn_frames_resize_u8; include/rfn_hip.h states the
    arithmetic): `src` uint8 [F, Hs, Ws, Cs] device tensor, Cs in {1, 3}; returns a fresh uint8 [F, H, W, Cd], Cd in
    {1, 3}, the exact integer area mean (rounded half up) of `window` = (y0, x0, Hc, Wc) of every frame (default: the
    whole frame), then 3 -> 1 channels by the integer luma weights or 1 -> 3 by copies.  One launch on the current
    stream; no CPU fallback."""
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8:
        raise TypeError("frames_resize: src must be a uint8 tensor, got %s" %
                        (src.dtype if isinstance(src, torch.Tensor) else type(src).__name__))
    if src.dim() != 4:
        raise ValueError("frames_resize: src must be [F, Hs, Ws, Cs], got %s" % (tuple(src.shape),))
    F, Hs, Ws, Cs = (int(d) for d in src.shape)
    H, W, Cd = int(H), int(W), int(Cd)
    if not (1 <= Hs <= RESIZE_MAX_SIDE and 1 <= Ws <= RESIZE_MAX_SIDE and 1 <= H <= RESIZE_MAX_SIDE and
            1 <= W <= RESIZE_MAX_SIDE):
        raise ValueError("frames_resize: sides must be in [1, %d], got %dx%d -> %dx%d" % (RESIZE_MAX_SIDE, Hs, Ws, H, W))
    if Cs not in (1, 3) or Cd not in (1, 3):
        raise ValueError("frames_resize: 1 or 3 channels on either side, got %d -> %d" % (Cs, Cd))
    y0, x0, Hc, Wc = (int(v) for v in (window if window is not None else (0, 0, Hs, Ws)))
    if Hc < 1 or Wc < 1 or y0 < 0 or x0 < 0 or y0 + Hc > Hs or x0 + Wc > Ws:
        raise ValueError("frames_resize: the window (y0 %d, x0 %d, %dx%d) is empty or leaves the %dx%d frame" %
                         (y0, x0, Hc, Wc, Hs, Ws))
    if not src.is_cuda:
        raise ValueError("frames_resize: src is on %s; the kernel needs device tensors (no CPU fallback)" % (src.device,))
    bands = -(-H // min(H, max(1, 256 // min(W, 256))))
    if F * bands > 0x7fffffff:
        raise ValueError("frames_resize: %d frames of %dx%d exceed one launch" % (F, H, W))
    src = src.contiguous()
    out = torch.empty((F, H, W, Cd), device=src.device, dtype=torch.uint8)
    if F:
        with torch.cuda.device(src.device):
            L.call("rfn_frames_resize_u8", src.data_ptr(), out.data_ptr(), F, Hs, Ws, Cs, H, W, Cd, y0, x0, Hc, Wc,
                   meta=("shell", "frames_resize", 0.0, "%dx%dx%dx%d>%dx%dx%d" % (F, Hs, Ws, Cs, H, W, Cd),
                         float(F * (Hc * Wc * Cs + H * W * Cd))))
    return out
