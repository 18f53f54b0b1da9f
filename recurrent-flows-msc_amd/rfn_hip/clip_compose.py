"""Animated prediction clips as 8-bit RGB pixels: the wrapper of csrc/clip_compose.hip (DESIGN.md section 28 is the
pixel contract).  rfn_hip.ops re-exports the public names; rfn_hip.pictures, the home of the still pictures, names
them too."""
import functools

import torch

from . import lib as L


CLIP_MODES = {"frame": 0, "mean": 1, "spread": 2}


@functools.lru_cache(maxsize=None)
def clip_limits():
    """(largest group G, largest gain) of a clip cell: the library's host-only queries (include/rfn_hip.h), read once;
    needs no device"""
    lib = L.load()
    return lib.rfn_clip_max_group(), lib.rfn_clip_max_gain()


class ClipCell(object):
    """One cell of compose_clip's grid: a sequence of frames that moves with the animation's t.  `frames`: a device
    tensor, fp32 in model space or uint8, [n, C, H, W] for mode "frame", [n, G, C, H, W] for "mean" / "spread" (the
    mean / gain times the population standard deviation over the G members, per byte); CHW dense, any strides along n
    and G (views such as predictions[:, :, b] of [n, D, B, C, H, W] are taken as they are).  Frame t shows
    frames[min(t, n - 1)].  The ring around the cell has colour `before` (r, g, b) for t < switch_at, else `after`."""

    def __init__(self, frames, mode="frame", gain=4, switch_at=0, before=(0, 160, 0), after=(208, 0, 0)):
        self.frames, self.mode, self.gain, self.switch_at = frames, mode, gain, switch_at
        self.before, self.after = before, after


def clip_shape(R, N, H, W, zoom, border, gutter):
    """(Hs, Ws) of a clip's frames: R x N cells of (zoom*H + 2*border) x (zoom*W + 2*border) pixels, `gutter` pixels
    between and around them"""
    Hc, Wc = zoom * H + 2 * border, zoom * W + 2 * border
    return R * Hc + (R + 1) * gutter, N * Wc + (N + 1) * gutter


def _rgb(c, what, where):
    try:
        c = tuple(int(v) for v in c)
    except TypeError:
        c = ()
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError("compose_clip: `%s` of cell %s must be three bytes (r, g, b)" % (what, where))
    return c[0] | c[1] << 8 | c[2] << 16


def compose_clip(cells, T, zoom=1, border=0, gutter=2, bg=255, n_bits=8, preprocess_range="0.5", scanlines=False,
                 out=None):
    """The T frames of an animation as 8-bit RGB pixels (rfn_clip_compose_u8, one launch for all of them).  `cells`: a
    list of R lists of N entries, each a ClipCell or None (an empty cell: all `bg`); all frames share one [C, H, W], C in
    {1, 3}, and one device.  Every cell is zoomed `zoom` times (nearest) and sits in a ring of `border` pixels in the
    cell's colour; cells are `gutter` pixels of `bg` apart.  fp32 frames become bytes exactly as
    Solver.preprocess(x, reverse=True) with this n_bits / preprocess_range makes them; uint8 frames are copied.  Returns
    uint8 [T, Hs, Ws, 3], or with scanlines=True [T, Hs, 1 + 3*Ws] whose lines start with the PNG filter byte 0
    (Utils.png.write_apng takes either); `out` (optional) is a contiguous uint8 tensor of that shape on the cells'
    device, at any byte address.  Argument errors are raised before anything touches the GPU.  No CPU fallback."""
    if not isinstance(cells, (list, tuple)) or not cells or not all(isinstance(r, (list, tuple)) for r in cells):
        raise TypeError("compose_clip: cells must be a non-empty list of lists of ClipCell / None")
    R, N = len(cells), len(cells[0])
    if N < 1 or any(len(r) != N for r in cells):
        raise ValueError("compose_clip: every row of the grid needs the same number (>= 1) of cells, got %s" %
                         ([len(r) for r in cells],))
    max_group, max_gain = clip_limits()
    T, zoom, border, gutter, bg, n_bits = int(T), int(zoom), int(border), int(gutter), int(bg), int(n_bits)
    records, first, tensors = [], None, []
    for r in range(R):
        for i in range(N):
            c, where = cells[r][i], "(%d, %d)" % (r, i)
            if c is None:
                records.append([0] * 8)
                continue
            if not isinstance(c, ClipCell):
                raise TypeError("compose_clip: cell %s must be a ClipCell or None, got %s" % (where, type(c).__name__))
            t = c.frames
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.uint8):
                raise TypeError("compose_clip: the frames of cell %s must be a float32 or uint8 tensor, got %s" %
                                (where, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
            if c.mode not in CLIP_MODES:
                raise ValueError("compose_clip: the mode of cell %s must be one of %s, got %r" %
                                 (where, sorted(CLIP_MODES), c.mode))
            grouped = c.mode != "frame"
            if t.dim() != (5 if grouped else 4):
                raise ValueError("compose_clip: the frames of cell %s (mode %r) must be %s, got %s" %
                                 (where, c.mode, "[n, G, C, H, W]" if grouped else "[n, C, H, W]", tuple(t.shape)))
            C, H, W = (int(d) for d in t.shape[-3:])
            if C not in (1, 3) or H < 1 or W < 1:
                raise ValueError("compose_clip: frames must be [C in {1, 3}, H >= 1, W >= 1], cell %s has %s" %
                                 (where, (C, H, W)))
            if first is None:
                first = (where, (C, H, W))
            elif first[1] != (C, H, W):
                raise ValueError("compose_clip: cell %s has frames %s, cell %s has %s" % (where, (C, H, W), first[0], first[1]))
            s = t.stride()
            if not ((W == 1 or s[-1] == 1) and (H == 1 or s[-2] == W) and (C == 1 or s[-3] == H * W)):
                raise ValueError("compose_clip: the frames of cell %s must be dense CHW, got shape %s stride %s" %
                                 (where, tuple(t.shape), tuple(s)))
            n, G = int(t.shape[0]), int(t.shape[1]) if grouped else 1
            if not 1 <= G <= max_group:
                raise ValueError("compose_clip: the group of cell %s has %d members, need 1..%d" % (where, G, max_group))
            gain = int(c.gain)
            if not 1 <= gain <= max_gain:
                raise ValueError("compose_clip: the gain of cell %s is %d, need 1..%d" % (where, gain, max_gain))
            switch_at = int(c.switch_at)
            if not -2 ** 31 <= switch_at < 2 ** 31:
                raise ValueError("compose_clip: switch_at of cell %s does not fit 32 bits: %d" % (where, switch_at))
            colours = _rgb(c.before, "before", where) | _rgb(c.after, "after", where) << 32
            if n == 0:   # no frame to show: an empty cell
                records.append([0] * 8)
                continue
            tensors.append((where, t))
            records.append([t, int(s[0]) if n > 1 else 0, int(s[1]) if grouped and G > 1 else 0, n, G,
                            (1 if t.dtype == torch.uint8 else 0) | CLIP_MODES[c.mode] << 8 | gain << 16, switch_at,
                            colours - (1 << 64) if colours >= 1 << 63 else colours])
    if first is None:
        raise ValueError("compose_clip: the grid needs at least one cell with frames")
    if (T < 1 or not 1 <= zoom <= 16 or not 0 <= border <= 64 or gutter < 0 or not 0 <= bg <= 255 or
            not 1 <= n_bits <= 8):
        raise ValueError("compose_clip: need T >= 1, zoom in [1, 16], border in [0, 64], gutter >= 0, bg in [0, 255], "
                         "n_bits in [1, 8] (got %d, %d, %d, %d, %d, %d)" % (T, zoom, border, gutter, bg, n_bits))
    C, H, W = first[1]
    Hs, Ws = clip_shape(R, N, H, W, zoom, border, gutter)
    if 3 * Ws + 1 > 0x7fffffff or T * Hs > 0x7fffffff:
        raise ValueError("compose_clip: %d frames of %dx%d pixels exceed one launch" % (T, Hs, Ws))
    for where, t in tensors:
        if not t.is_cuda:
            raise ValueError("compose_clip: cell %s is on %s; the kernel needs device tensors (no CPU fallback)" %
                             (where, t.device))
        if t.device != tensors[0][1].device:
            raise ValueError("compose_clip: cell %s is on %s, cell %s on %s" %
                             (tensors[0][0], tensors[0][1].device, where, t.device))
    dev = tensors[0][1].device
    shape = (T, Hs, 1 + 3 * Ws) if scanlines else (T, Hs, Ws, 3)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or
          not out.is_contiguous() or out.device != dev):
        raise ValueError("compose_clip: out must be a contiguous uint8 tensor %s on %s" % (shape, dev))
    table = torch.tensor([[rec[0].data_ptr() if isinstance(rec[0], torch.Tensor) else 0] + rec[1:] for rec in records],
                         dtype=torch.int64).to(dev)
    read = sum(float(min(T, rec[3]) * rec[4] * C * H * W * rec[0].element_size()) for rec in records
               if isinstance(rec[0], torch.Tensor))
    with torch.cuda.device(dev):
        L.call("rfn_clip_compose_u8", table.data_ptr(), R, N, T, C, H, W, zoom, border, gutter, bg, n_bits,
               1 if preprocess_range == "0.5" else 0, 1 if scanlines else 0, out.data_ptr(),
               meta=("shell", "clip_compose", 0.0, "%dx%dx%dx%dx%dx%d z%d" % (R, N, T, C, H, W, zoom),
                     float(out.numel()) + 64.0 * R * N + read))
    return out
