"""PNG files from pixel arrays with the standard library alone (zlib, struct): what the reference's figures end in
(`fig.savefig`, RFN/trainer.py:411 and evaluation_metrics/error_metrics.py:151) for sheets that are pixels only.
8-bit RGB (colour type 2), every line with filter type 0, one IDAT chunk, no interlace."""
import os
import struct
import zlib

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, data, level=6):
    """Write `data` to `path` as an 8-bit RGB PNG.  `data`: uint8, either pixels [H, W, 3] or scanlines [H, 1 + 3*W]
    whose byte 0 of every line is the filter type 0 (what rfn_hip.ops.compose_sheet(..., scanlines=True) returns: the
    PNG's raw stream as it stands); a numpy array or a tensor on any device.  The file appears under its name only when
    complete: it is written next to it under a temporary name and moved with os.replace."""
    if hasattr(data, "detach"):
        data = data.detach().cpu().numpy()
    data = np.asarray(data)
    if data.dtype != np.uint8:
        raise TypeError("write_png: data must be uint8, got %s" % data.dtype)
    if data.ndim == 3 and data.shape[2] == 3:
        h, w = int(data.shape[0]), int(data.shape[1])
        raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
        raw[:, 1:] = data.reshape(h, 3 * w)
    elif data.ndim == 2 and data.shape[1] % 3 == 1:
        h, w = int(data.shape[0]), int(data.shape[1]) // 3
        if data[:, 0].any():
            raise ValueError("write_png: scanlines must start with the filter type 0")
        raw = np.ascontiguousarray(data)
    else:
        raise ValueError("write_png: data must be [H, W, 3] pixels or [H, 1 + 3*W] scanlines, got %s" %
                         (tuple(data.shape),))
    if h < 1 or w < 1:
        raise ValueError("write_png: an image needs at least one pixel, got %dx%d" % (h, w))
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    blob = _SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b"")
    path = os.fspath(path)
    tmp = "%s.%d.tmp" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            f.write(blob)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return h, w
