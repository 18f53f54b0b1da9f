"""Addressed (keyed) normal and uniform noise: wrappers of csrc/keyed_normal.hip and csrc/iw_bound.hip.  rfn_hip.ops
re-exports the public names."""
import ctypes

import torch

from . import lib as L
from .args import check_step, check_u63, fresh_device


KEYED_NORMAL_MAX_SLOTS = 8


def keyed_normal_tiled_row(k, r, b, n_draws, B):
    """the row of tile k, draw r (local to the call), sequence b (local to the batch) in a tensor of keyed_normal(...,
    tiles=K): tile-major, then draw-major.  It holds what row r*B + b holds with tiles = 1.  The batch of a
    temperature sweep (RFN.predict_draws(temperatures=...)) has the same layout, k being the temperature."""
    return (k * n_draws + r) * B + b


def keyed_normal(shapes, B, n_draws, seed, step, first_seq=0, first_draw=0, out=None, device=None, tiles=1):
    """Addressed N(0,1) noise (rfn_keyed_normal_f32; include/rfn_hip.h and DESIGN section 16 hold the definition): a list
    of float32 tensors [n_draws*B, *shape_j], slot j being the list position (at most 8).  Row r*B + b of every tensor
    stands for draw first_draw + r of sequence first_seq + b, and a value depends only on (seed, step, slot, sequence,
    draw, position in the row): the same on any grid, for any B, n_draws and split of the draws into calls.  An entry
    None of `shapes` skips that slot (None in the result).  out: tensors to fill in place instead of fresh ones (None
    where the slot is skipped), each contiguous float32 of n_draws*B rows on one device; with out, `shapes` may be None.
    device: where fresh tensors go (default: the current GPU).  One launch on the current stream; no CPU fallback.
    tiles = K > 1 (rfn_keyed_normal_tiled_f32): every tensor has K*n_draws*B rows and row (k*n_draws + r)*B + b holds
    exactly what row r*B + b holds with tiles = 1, for every k (the blocks of a temperature sweep share their noise);
    still one launch.  tiles = 1 is the untiled entry point."""
    B, n_draws, seed, step, first_seq, first_draw = (int(v) for v in (B, n_draws, seed, step, first_seq, first_draw))
    if isinstance(tiles, bool) or not isinstance(tiles, int):
        raise TypeError("keyed_normal: tiles must be an int, got %s" % type(tiles).__name__)
    if tiles < 1:
        raise ValueError("keyed_normal: tiles must be at least 1, got %d" % tiles)
    if B < 1 or n_draws < 0:
        raise ValueError("keyed_normal: need B >= 1 and n_draws >= 0 (got %d, %d)" % (B, n_draws))
    check_u63("keyed_normal", seed=seed, first_seq=first_seq, first_draw=first_draw)
    check_step("keyed_normal", step)
    tile_rows = n_draws * B          # the rows that are computed; every tensor holds them `tiles` times
    rows = tiles * tile_rows
    if rows > 0x7fffffff:
        raise ValueError("keyed_normal: %d rows exceed one launch" % rows)
    if out is None:
        if shapes is None:
            raise TypeError("keyed_normal: give shapes or out")
        device = fresh_device("keyed_normal", device)
        out = [None if sh is None else torch.empty((rows,) + tuple(int(d) for d in sh), device=device,
                                                   dtype=torch.float32) for sh in shapes]
    else:
        out = list(out)
        if shapes is not None and len(shapes) != len(out):
            raise ValueError("keyed_normal: %d shapes for %d out tensors" % (len(shapes), len(out)))
        for j, t in enumerate(out):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError("keyed_normal: out[%d] must be a tensor, got %s" % (j, type(t).__name__))
            if t.dim() < 1 or int(t.shape[0]) != rows:
                raise ValueError("keyed_normal: out[%d] must have %d rows, got shape %s" % (j, rows, tuple(t.shape)))
            if shapes is not None and shapes[j] is not None and tuple(t.shape[1:]) != tuple(int(d) for d in shapes[j]):
                raise ValueError("keyed_normal: out[%d] has rows %s, shapes[%d] is %s" %
                                 (j, tuple(t.shape[1:]), j, tuple(shapes[j])))
    if not 1 <= len(out) <= KEYED_NORMAL_MAX_SLOTS:
        raise ValueError("keyed_normal: %d slots, one launch fills 1 to %d" % (len(out), KEYED_NORMAL_MAX_SLOTS))
    live = [t for t in out if t is not None]
    for t in live:
        if t.device != live[0].device:
            raise ValueError("keyed_normal: the tensors are on %s and %s" % (live[0].device, t.device))
    ptrs = (ctypes.c_void_p * len(out))()
    numels = (ctypes.c_int * len(out))()
    total = 0
    for j, t in enumerate(out):
        if t is None or rows == 0:
            continue
        n = t.numel() // rows
        if n > 0x7fffffff:
            raise ValueError("keyed_normal: rows of %d values exceed one launch" % n)
        if n:
            ptrs[j] = L.dev(t, "out[%d]" % j).value
        numels[j] = n
        total += t.numel()
    if total:
        with torch.cuda.device(live[0].device):
            if tiles == 1:
                L.call("rfn_keyed_normal_f32", ptrs, numels, len(out), rows, B, seed, step, first_seq, first_draw,
                       meta=("shell", "keyed_normal", 0.0, "%dx%d" % (rows, total // rows), 4.0 * total))
            else:
                L.call("rfn_keyed_normal_tiled_f32", ptrs, numels, len(out), tile_rows, B, tiles, seed, step, first_seq,
                       first_draw,
                       meta=("shell", "keyed_normal", 0.0, "%dx%dx%d" % (tiles, tile_rows, total // rows), 4.0 * total))
    return out


KEYED_UNIFORM_SLOT_DEQUANT = 24   # the dequantisation noise of RFN.iw_log_weights (keyed_normal: 0 .. 7, mol: 16, 17)


def keyed_uniform(shape, B, n_draws, seed, first_step, n_steps=1, slot=KEYED_UNIFORM_SLOT_DEQUANT, scale=1.0, first_seq=0,
                  first_draw=0, device=None, out=None):
    """Addressed uniform noise in [0, scale) (rfn_keyed_uniform_f32; include/rfn_hip.h and DESIGN section 24 hold the
    definition): a float32 tensor [n_steps, n_draws*B, *shape].  Step-block s stands for step first_step + s, row r*B + b
    of every block for draw first_draw + r of sequence first_seq + b, and a value depends only on (seed, step, slot,
    sequence, draw, position in the row): the same on any grid, for any B, n_draws, n_steps and split into calls.  slot
    in [8, 2^31): keyed_normal owns the slots below.  out: a contiguous float32 tensor of that shape to fill in place
    instead of a fresh one (`shape` may then be None); device: where a fresh tensor goes (default: the current GPU).
    One launch on the current stream for all steps; torch's generators are not touched; no CPU fallback."""
    B, n_draws, seed, first_step, n_steps, first_seq, first_draw = (int(v) for v in (B, n_draws, seed, first_step, n_steps,
                                                                                  first_seq, first_draw))
    if isinstance(slot, bool) or not isinstance(slot, int):
        raise TypeError("keyed_uniform: slot must be an int, got %s" % type(slot).__name__)
    scale = float(scale)
    if B < 1 or n_draws < 0 or n_steps < 0:
        raise ValueError("keyed_uniform: need B >= 1, n_draws >= 0 and n_steps >= 0 (got %d, %d, %d)" %
                         (B, n_draws, n_steps))
    check_u63("keyed_uniform", seed=seed, first_seq=first_seq, first_draw=first_draw)
    if first_step < 0 or first_step + n_steps > 1 << 31:
        raise ValueError("keyed_uniform: steps %d .. %d not in [0, 2^31)" % (first_step, first_step + n_steps - 1))
    if not 8 <= slot < 1 << 31:
        raise ValueError("keyed_uniform: slot %d not in [8, 2^31) (keyed_normal owns slots 0 .. 7)" % slot)
    if not 0.0 < scale < float("inf"):
        raise ValueError("keyed_uniform: scale must be finite and positive, got %r" % scale)
    rows = n_draws * B
    if rows > 0x7fffffff:
        raise ValueError("keyed_uniform: %d rows exceed one launch" % rows)
    if out is None:
        if shape is None:
            raise TypeError("keyed_uniform: give shape or out")
        device = fresh_device("keyed_uniform", device)
        out = torch.empty((n_steps, rows) + tuple(int(d) for d in shape), device=device, dtype=torch.float32)
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError("keyed_uniform: out must be a tensor, got %s" % type(out).__name__)
        if out.dim() < 2 or tuple(out.shape[:2]) != (n_steps, rows):
            raise ValueError("keyed_uniform: out must be [%d, %d, ...], got shape %s" % (n_steps, rows, tuple(out.shape)))
        if shape is not None and tuple(out.shape[2:]) != tuple(int(d) for d in shape):
            raise ValueError("keyed_uniform: out has rows %s, shape is %s" % (tuple(out.shape[2:]), tuple(shape)))
    total = out.numel()
    if total:
        numel = total // (n_steps * rows)
        if numel > 0x7fffffff or -(-numel // 8) * rows * n_steps > 0x7fffffff * 256:
            raise ValueError("keyed_uniform: %d steps of %d rows of %d values exceed one launch" % (n_steps, rows, numel))
        ptr = L.dev(out, "out")
        with torch.cuda.device(out.device):
            L.call("rfn_keyed_uniform_f32", ptr, n_steps, rows, B, numel, scale, seed, first_step, slot,
                   first_seq, first_draw,
                   meta=("shell", "keyed_uniform", 0.0, "%dx%dx%d" % (n_steps, rows, numel), 4.0 * total))
    return out
