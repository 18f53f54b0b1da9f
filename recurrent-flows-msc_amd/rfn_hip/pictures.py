"""Pictures as 8-bit RGB pixels: the sample sheets and the chart rasteriser; wrappers of csrc/sheet.hip and
csrc/chart.hip (rfn_hip/chart.py builds the display lists).  rfn_hip.ops re-exports the public names.  The moving
pictures (csrc/clip_compose.hip) have their wrapper in rfn_hip/clip_compose.py, a module named after its csrc file like
every other family's; its names are reachable here as well."""
import ctypes

import torch

from . import lib as L
from .clip_compose import ClipCell, clip_limits, clip_shape, compose_clip  # noqa: F401


SHEET_MAX_ROWS = L.CONSTANTS["RFN_SHEET_MAX_ROWS"]   # the row descriptors travel in the launch's arguments


def sheet_shape(n_rows, n_cols, H, W, gutter):
    """(Hs, Ws) of a sheet of n_rows x n_cols cells of H x W pixels with `gutter` pixels between and around them"""
    return n_rows * H + (n_rows + 1) * gutter, n_cols * W + (n_cols + 1) * gutter


def compose_sheet(rows, n_cols, gutter=2, bg=255, n_bits=8, preprocess_range="0.5", scanlines=False, out=None):
    """A sheet of frames as 8-bit RGB pixels (rfn_sheet_compose_u8: the subplot grids of the reference's plotter and
    Evaluator.plot_samples, trainer.py:325-417, error_metrics.py:128-152, as pixels only).  `rows`: a list of device
    tensors [n, C, H, W], n <= n_cols, fp32 in model space or uint8, each with dense CHW frames and any stride along n
    (pass views such as image[0] of [B, T, C, H, W] or samples[:, 0] of [T, B, C, H, W]: nothing is copied).  Row r fills
    the first n cells of sheet row r, the rest is background `bg`; cells are `gutter` pixels apart.  fp32 frames become
    bytes exactly as Solver.preprocess(x, reverse=True) with this n_bits / preprocess_range makes them; uint8 frames are
    copied; C == 1 is written to R, G and B.  Returns uint8 [Hs, Ws, 3], or with scanlines=True [Hs, 1 + 3*Ws] whose
    lines start with the PNG filter byte 0 (Utils.png.write_png takes either); `out` (optional) is a contiguous uint8
    tensor of that shape on the rows' device to write into, at any byte address.  One launch on the current stream; no
    CPU fallback."""
    if not isinstance(rows, (list, tuple)) or not rows:
        raise TypeError("compose_sheet: rows must be a non-empty list of tensors, got %s" % type(rows).__name__)
    for r, t in enumerate(rows):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.uint8):
            raise TypeError("compose_sheet: row %d must be a float32 or uint8 tensor, got %s" %
                            (r, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.dim() != 4:
            raise ValueError("compose_sheet: row %d must be [n, C, H, W], got %s" % (r, tuple(t.shape)))
    n_cols, gutter, bg, n_bits = int(n_cols), int(gutter), int(bg), int(n_bits)
    C, H, W = (int(d) for d in rows[0].shape[1:])
    if C not in (1, 3) or H < 1 or W < 1:
        raise ValueError("compose_sheet: frames must be [C in {1, 3}, H >= 1, W >= 1], got %s" % ((C, H, W),))
    for r, t in enumerate(rows):
        if tuple(t.shape[1:]) != (C, H, W):
            raise ValueError("compose_sheet: row %d has frames %s, row 0 has %s" % (r, tuple(t.shape[1:]), (C, H, W)))
        s = t.stride()
        if not ((W == 1 or s[3] == 1) and (H == 1 or s[2] == W) and (C == 1 or s[1] == H * W)):
            raise ValueError("compose_sheet: the frames of row %d must be dense CHW, got shape %s stride %s" %
                             (r, tuple(t.shape), tuple(s)))
    if n_cols < 1 or gutter < 0 or not 0 <= bg <= 255 or not 1 <= n_bits <= 8:
        raise ValueError("compose_sheet: need n_cols >= 1, gutter >= 0, bg in [0, 255], n_bits in [1, 8] (got %d, %d, "
                         "%d, %d)" % (n_cols, gutter, bg, n_bits))
    if len(rows) > SHEET_MAX_ROWS:
        raise ValueError("compose_sheet: %d rows exceed the %d of one launch" % (len(rows), SHEET_MAX_ROWS))
    for r, t in enumerate(rows):
        if int(t.shape[0]) > n_cols:
            raise ValueError("compose_sheet: row %d holds %d frames for %d columns" % (r, int(t.shape[0]), n_cols))
    for r, t in enumerate(rows):
        if not t.is_cuda:
            raise ValueError("compose_sheet: row %d is on %s; the kernel needs device tensors (no CPU fallback)" %
                             (r, t.device))
        if t.device != rows[0].device:
            raise ValueError("compose_sheet: row 0 is on %s, row %d on %s" % (rows[0].device, r, t.device))
    Hs, Ws = sheet_shape(len(rows), n_cols, H, W, gutter)
    if Hs > 0x7fffffff or 3 * Ws + 1 > 0x7fffffff or C * H * W > 0x7fffffff:
        raise ValueError("compose_sheet: a %dx%d sheet of %dx%dx%d frames exceeds one launch" % (Hs, Ws, C, H, W))
    tab = (L.rfn_sheet_row * len(rows))()
    for r, t in enumerate(rows):
        n = int(t.shape[0])
        tab[r].ptr = t.data_ptr() if n else None
        tab[r].step = int(t.stride(0)) if n > 1 else 0
        tab[r].kind = 1 if t.dtype == torch.uint8 else 0
        tab[r].count = n
    dev = rows[0].device
    shape = (Hs, 1 + 3 * Ws) if scanlines else (Hs, Ws, 3)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or
          not out.is_contiguous() or out.device != dev):
        raise ValueError("compose_sheet: out must be a contiguous uint8 tensor %s on %s" % (shape, dev))
    with torch.cuda.device(dev):
        L.call("rfn_sheet_compose_u8", tab, len(rows), n_cols, C, H, W, gutter, bg, n_bits,
               1 if preprocess_range == "0.5" else 0, 1 if scanlines else 0, out.data_ptr(),
               meta=("shell", "sheet_compose", 0.0, "%dx%dx%dx%dx%d" % (len(rows), n_cols, C, H, W),
                     float(out.numel()) + sum(float(t.numel() * t.element_size()) for t in rows)))
    return out


def chart_chunk():
    """records one workgroup of the chart kernel culls at a time (rfn_chart_chunk); the picture does not depend on it"""
    return int(L.load().rfn_chart_chunk())


def chart_font():
    """the kernel's built-in 5x7 font (rfn_chart_font): int32 numpy [95, 5], row ch = character 32 + ch, one entry per
    column from the left, bit r = the dot in row r from the top"""
    import numpy as np
    buf = (ctypes.c_longlong * (95 * 5))()
    rc = L.load().rfn_chart_font(ctypes.cast(buf, ctypes.c_void_p))
    if rc != 0:
        raise RuntimeError("rfn_chart_font failed (code %d)" % rc)
    return np.frombuffer(buf, dtype=np.int64).astype(np.int32).reshape(95, 5)


def render_chart(chart, H=None, W=None, scanlines=False, out=None, bg=(255, 255, 255), device=None):
    """A line chart as 8-bit RGB pixels (rfn_chart_render_u8; the pixel contract is DESIGN.md section 25).  `chart`: a
    rfn_hip.chart.Figure or DisplayList (H, W and bg come from it; a given H / W must agree), or a display-list table
    int32 [n, 12] -- a numpy array or CPU tensor, checked against the contract's coordinate bounds and uploaded, or a
    contiguous device tensor, taken as it is -- painted on an H x W canvas of colour `bg` (r, g, b).  Returns uint8
    [H, W, 3], or with scanlines=True [H, 1 + 3*W] whose lines start with the PNG filter byte 0 (Utils.png.write_png
    takes either); `out` (optional) is a contiguous uint8 device tensor of that shape, at any byte address.  The device
    is that of `out`, of a device table, `device`, or the current one.  One launch on the current stream; no CPU
    fallback."""
    import numpy as np
    from . import chart as C
    if isinstance(chart, C.Figure):
        chart = C.build_display_list(chart)
    if isinstance(chart, C.DisplayList):
        if (H is not None and int(H) != chart.height) or (W is not None and int(W) != chart.width):
            raise ValueError("render_chart: the figure is %dx%d, H x W = %sx%s was asked for" %
                             (chart.height, chart.width, H, W))
        H, W, bg, table = chart.height, chart.width, chart.bg, chart.table
    else:
        table = chart
    if H is None or W is None:
        raise TypeError("render_chart: a table needs the canvas size H, W")
    H, W = int(H), int(W)
    if not (1 <= H <= C.MAX_SIDE and 1 <= W <= C.MAX_SIDE):
        raise ValueError("render_chart: the canvas is at most %d x %d pixels, got %d x %d" %
                         (C.MAX_SIDE, C.MAX_SIDE, H, W))
    bg = tuple(int(c) for c in bg)
    if len(bg) != 3 or not all(0 <= c <= 255 for c in bg):
        raise ValueError("render_chart: bg must be three bytes (r, g, b), got %s" % (bg,))
    on_device = isinstance(table, torch.Tensor) and table.is_cuda
    if on_device:
        if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != C.REC or not table.is_contiguous():
            raise ValueError("render_chart: a device table must be contiguous int32 [n, %d], got %s %s" %
                             (C.REC, table.dtype, tuple(table.shape)))
    elif isinstance(table, (torch.Tensor, np.ndarray)):
        table = C.check_table(table.numpy() if isinstance(table, torch.Tensor) else table)
    else:
        raise TypeError("render_chart: need a chart.Figure, a chart.DisplayList or an int32 [n, %d] table, got %s" %
                        (C.REC, type(chart).__name__))
    shape = (H, 1 + 3 * W) if scanlines else (H, W, 3)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or
                            tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda):
        raise ValueError("render_chart: out must be a contiguous uint8 device tensor %s" % (shape,))
    if out is not None:
        dev = out.device
    elif on_device:
        dev = table.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("render_chart: the chart kernel needs a GPU (no CPU fallback)")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("render_chart: the chart kernel needs a GPU, got device %s (no CPU fallback)" % dev)
    if on_device and table.device != dev:
        raise ValueError("render_chart: the table is on %s, out on %s" % (table.device, dev))
    if not on_device:
        table = torch.from_numpy(table).to(dev)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    n = int(table.shape[0])
    with torch.cuda.device(dev):
        L.call("rfn_chart_render_u8", table.data_ptr() if n else None, n, H, W, bg[0] | bg[1] << 8 | bg[2] << 16,
               1 if scanlines else 0, out.data_ptr(),
               meta=("shell", "chart_render", 0.0, "%dx%dx%d" % (n, H, W), float(out.numel()) + 48.0 * n))
    return out
