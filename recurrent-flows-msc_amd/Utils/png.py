"""PNG files from pixel arrays with the standard library alone (zlib, struct): what the reference's figures end in
(`fig.savefig`, RFN/trainer.py:411 and evaluation_metrics/error_metrics.py:151) for sheets that are pixels only.
8-bit RGB (colour type 2), every line with filter type 0, one IDAT chunk, no interlace.  write_apng writes a sequence of
such pictures as one animated PNG."""
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


def write_apng(path, frames, delay_ms=100, loops=0, level=6):
    """Write `frames` to `path` as an animated PNG (APNG 1.0: PNG plus the chunks acTL, fcTL and fdAT; a viewer that does
    not know them shows frame 0).  `frames`: uint8, either pixels [T, H, W, 3] or scanlines [T, H, 1 + 3*W] whose byte 0 of
    every line is the filter type 0 (what rfn_hip.ops.compose_clip(..., scanlines=True) returns); a numpy array or a
    tensor on any device.  Every frame is shown for delay_ms milliseconds; the animation plays `loops` times (0: for
    ever).  Chunks: IHDR, acTL(T, loops), then fcTL + IDAT for frame 0 and fcTL + fdAT for every later one, IEND; every
    frame is a full one (offsets 0, dispose 0, blend 0: no delta frames) and the sequence numbers of the fcTL and fdAT
    chunks count up from 0.  The file appears under its name only when complete, as write_png's does."""
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise TypeError("write_apng: frames must be uint8, got %s" % frames.dtype)
    if frames.ndim == 4 and frames.shape[3] == 3:
        t, h, w = (int(d) for d in frames.shape[:3])
        raw = np.zeros((t, h, 1 + 3 * w), dtype=np.uint8)
        raw[:, :, 1:] = frames.reshape(t, h, 3 * w)
    elif frames.ndim == 3 and frames.shape[2] % 3 == 1:
        t, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2]) // 3
        if frames[:, :, 0].any():
            raise ValueError("write_apng: scanlines must start with the filter type 0")
        raw = np.ascontiguousarray(frames)
    else:
        raise ValueError("write_apng: frames must be [T, H, W, 3] pixels or [T, H, 1 + 3*W] scanlines, got %s" %
                         (tuple(frames.shape),))
    if t < 1 or h < 1 or w < 1:
        raise ValueError("write_apng: an animation needs at least one frame of one pixel, got %d frames of %dx%d" %
                         (t, h, w))
    delay_ms, loops = int(delay_ms), int(loops)
    if not 0 <= delay_ms <= 0xffff or not 0 <= loops <= 0x7fffffff:
        raise ValueError("write_apng: need 0 <= delay_ms <= 65535 and 0 <= loops < 2^31, got %d and %d" %
                         (delay_ms, loops))
    parts = [_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)),
             _chunk(b"acTL", struct.pack(">II", t, loops))]
    seq = 0
    for k in range(t):
        parts.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, delay_ms, 1000, 0, 0)))
        seq += 1
        data = zlib.compress(raw[k].tobytes(), level)
        if k == 0:
            parts.append(_chunk(b"IDAT", data))
        else:
            parts.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    parts.append(_chunk(b"IEND", b""))
    path = os.fspath(path)
    tmp = "%s.%d.tmp" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            f.write(b"".join(parts))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return t, h, w
