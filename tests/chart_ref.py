"""The chart kernel's pixel contract restated in int64 numpy, written from that text: records of
12 int32 {type, rgba, p0..p9}, 16 samples per pixel at {2, 6, 10, 14}/16, per-type integer inside-tests, and the blend
dst = (dst (4080 - w) + src w + 2040) / 4080 with w = alpha * coverage, record after record.  Meant for small canvases:
every record is evaluated on a window of whole pixels around its extreme coordinates."""
import numpy as np

OFFSETS = np.array([2, 6, 10, 14], dtype=np.int64)
BOX, CAPSULE, TRAPEZOID, TRIANGLE, GLYPH = range(5)


def inside(ty, p, sx, sy, font):
    """boolean array: which of the samples (sx, sy) (int64 arrays of one shape, 1/16 pixel) lie inside the record"""
    if ty == BOX:
        x0, y0, x1, y1, on, off = p[:6]
        ok = (x0 <= sx) & (sx < x1) & (y0 <= sy) & (sy < y1)
        if on + off > 0:
            t, t0 = (sx, x0) if x1 - x0 >= y1 - y0 else (sy, y0)
            ok &= np.where(ok, (t - t0) % (on + off), on) < on
        return ok
    if ty == CAPSULE:
        ax, ay, bx, by, hw = p[:5]
        dx, dy = bx - ax, by - ay
        px, py = sx - ax, sy - ay
        dot, dd, hh = px * dx + py * dy, dx * dx + dy * dy, hw * hw
        near_a = px * px + py * py <= hh
        near_b = (sx - bx) ** 2 + (sy - by) ** 2 <= hh
        cross = dx * py - dy * px
        return np.where(dot <= 0, near_a, np.where(dot >= dd, near_b, cross * cross <= hh * dd))
    if ty == TRAPEZOID:
        x0, x1, lo0, lo1, hi0, hi1 = p[:6]
        return ((x0 <= sx) & (sx < x1) & ((sy - lo0) * (x1 - x0) >= (lo1 - lo0) * (sx - x0)) &
                ((sy - hi0) * (x1 - x0) < (hi1 - hi0) * (sx - x0)))
    if ty == TRIANGLE:
        v = [(p[0], p[1]), (p[2], p[3]), (p[4], p[5])]
        if (v[1][0] - v[0][0]) * (v[2][1] - v[0][1]) == (v[1][1] - v[0][1]) * (v[2][0] - v[0][0]):   # zero area
            return np.zeros(sx.shape, dtype=bool)
        e = [(v[j][0] - v[i][0]) * (sy - v[i][1]) - (v[j][1] - v[i][1]) * (sx - v[i][0])
             for i, j in ((0, 1), (1, 2), (2, 0))]
        return ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
    if ty == GLYPH:
        x, y, code, k, rot = p[:5]
        if not (32 <= code <= 126 and 1 <= k <= 128):
            return np.zeros(sx.shape, dtype=bool)
        q, u, v = 16 * k, sx - x, sy - y
        nu, nv = (7 * q, 5 * q) if rot else (5 * q, 7 * q)
        ok = (0 <= u) & (u < nu) & (0 <= v) & (v < nv)
        a, b = np.where(ok, u // q, 0), np.where(ok, v // q, 0)
        col, row = (4 - b, a) if rot else (a, b)
        columns = np.asarray(font, dtype=np.int64)[code - 32]        # five column bytes, bit r = row r from the top
        return ok & (((columns[col] >> row) & 1) == 1)
    return np.zeros(sx.shape, dtype=bool)


def _window(ty, p, H, W):
    """pixel window [y0, y1) x [x0, x1) that holds every sample the record can cover (generous), clipped to the canvas"""
    if ty == BOX:
        xs, ys, m = (p[0], p[2]), (p[1], p[3]), 0
    elif ty == CAPSULE:
        xs, ys, m = (p[0], p[2]), (p[1], p[3]), abs(p[4])
    elif ty == TRAPEZOID:
        xs, ys, m = (p[0], p[1]), p[2:6], 0
    elif ty == TRIANGLE:
        xs, ys, m = p[0:6:2], p[1:6:2], 0
    elif ty == GLYPH:
        xs, ys, m = (p[0],), (p[1],), 7 * 16 * max(0, min(p[3], 128))
    else:
        return None
    x0, x1 = max(0, (min(xs) - m) // 16 - 1), min(W, (max(xs) + m) // 16 + 2)
    y0, y1 = max(0, (min(ys) - m) // 16 - 1), min(H, (max(ys) + m) // 16 + 2)
    return (y0, y1, x0, x1) if x0 < x1 and y0 < y1 else None


def coverage(ty, p, y0, y1, x0, x1, font):
    """c [y1 - y0, x1 - x0]: samples of each pixel of the window inside the record"""
    sx = (16 * np.arange(x0, x1, dtype=np.int64)[:, None] + OFFSETS[None, :]).reshape(-1)
    sy = (16 * np.arange(y0, y1, dtype=np.int64)[:, None] + OFFSETS[None, :]).reshape(-1)
    SX, SY = np.meshgrid(sx, sy)
    return inside(ty, p, SX, SY, font).reshape(y1 - y0, 4, x1 - x0, 4).sum(axis=(1, 3)).astype(np.int64)


def render(table, H, W, font, bg=(255, 255, 255), lead=0):
    """uint8 [H, W, 3] (lead = 0) or scanlines [H, 1 + 3 W] (lead = 1) of the display list"""
    img = np.empty((H, W, 3), dtype=np.int64)
    img[:] = np.asarray(bg, dtype=np.int64)
    for rec in np.asarray(table).reshape(-1, 12):
        ty, rgba = int(rec[0]), int(rec[1]) & 0xffffffff
        p = [int(v) for v in rec[2:]]
        alpha, src = rgba >> 24, (rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255)
        win = _window(ty, p, H, W)
        if win is None or alpha == 0:
            continue
        y0, y1, x0, x1 = win
        w = alpha * coverage(ty, p, y0, y1, x0, x1, font)
        for ch in range(3):
            dst = img[y0:y1, x0:x1, ch]
            img[y0:y1, x0:x1, ch] = (dst * (4080 - w) + src[ch] * w + 2040) // 4080
    assert img.min() >= 0 and img.max() <= 255
    out = img.astype(np.uint8)
    if lead:
        out = np.concatenate([np.zeros((H, 1), dtype=np.uint8), out.reshape(H, 3 * W)], axis=1)
    return out
