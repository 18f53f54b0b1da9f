"""The pixel contract of rfn_clip_compose_u8 restated on the CPU, written from that text: bytes by
Solver.preprocess(reverse=True), Python / numpy int64 sums with math.isqrt, and slice assignment into a bg-filled array.
`cells` is what rfn_hip.ops.compose_clip takes (tensors on any device)."""
import math

import numpy as np
import torch


def to_bytes(x, n_bits=8, preprocess_range="0.5"):
    """uint8 numpy of a frame tensor: uint8 as it is; fp32 as Solver.preprocess(x, reverse=True) (RFN/trainer.py), with
    the contract's NaN -> 0 made explicit (a NaN's cast to a byte is not defined on the CPU)"""
    x = x.detach().cpu()
    if x.dtype == torch.uint8:
        return x.numpy()
    n_bins = 2 ** n_bits
    if preprocess_range == "0.5":
        x = x + 0.5
    x = x * n_bins
    q = torch.clamp(torch.floor(x) * (256. / n_bins), 0, 255)
    return torch.nan_to_num(q, nan=0.0).byte().numpy()


def mean_rule(members):
    """members: integer array [G, ...] -> (sum + G/2) / G, floor division"""
    b = np.asarray(members).astype(np.int64)
    G = b.shape[0]
    return (b.sum(0) + G // 2) // G


def spread_rule(members, gain):
    """members: integer array [G, ...] -> min(255, isqrt(gain^2 (G sum b^2 - (sum b)^2)) / G), floor division"""
    b = np.asarray(members).astype(np.int64)
    G = b.shape[0]
    s1, s2 = b.sum(0), (b * b).sum(0)
    rad = gain * gain * (G * s2 - s1 * s1)
    root = np.array([math.isqrt(int(v)) for v in rad.reshape(-1)], dtype=np.int64).reshape(rad.shape)
    return np.minimum(255, root // G)


def clip_shape(R, N, H, W, zoom, border, gutter):
    Hc, Wc = zoom * H + 2 * border, zoom * W + 2 * border
    return R * Hc + (R + 1) * gutter, N * Wc + (N + 1) * gutter


def compose_clip_ref(cells, T, zoom=1, border=0, gutter=2, bg=255, n_bits=8, preprocess_range="0.5", scanlines=False):
    """uint8 numpy [T, Hs, Ws, 3], or [T, Hs, 1 + 3*Ws] with scanlines"""
    R, N = len(cells), len(cells[0])
    some = next(c for row in cells for c in row if c is not None)
    C, H, W = (int(d) for d in some.frames.shape[-3:])
    Hc, Wc = zoom * H + 2 * border, zoom * W + 2 * border
    Hs, Ws = clip_shape(R, N, H, W, zoom, border, gutter)
    out = np.full((T, Hs, Ws, 3), bg, dtype=np.uint8)
    for r in range(R):
        for i in range(N):
            c = cells[r][i]
            if c is None or int(c.frames.shape[0]) == 0:
                continue
            b = to_bytes(c.frames, n_bits, preprocess_range)
            y0, x0 = gutter + r * (Hc + gutter), gutter + i * (Wc + gutter)
            for t in range(T):
                f = b[min(t, b.shape[0] - 1)]
                if c.mode == "mean":
                    f = mean_rule(f)
                elif c.mode == "spread":
                    f = spread_rule(f, int(c.gain))
                f = np.asarray(f).astype(np.uint8)                     # [C, H, W]
                img = np.repeat(f, 3, axis=0) if C == 1 else f
                img = img.transpose(1, 2, 0).repeat(zoom, axis=0).repeat(zoom, axis=1)
                out[t, y0:y0 + Hc, x0:x0 + Wc] = np.array(c.before if t < c.switch_at else c.after, dtype=np.uint8)
                out[t, y0 + border:y0 + border + zoom * H, x0 + border:x0 + border + zoom * W] = img
    if not scanlines:
        return out
    lines = np.zeros((T, Hs, 1 + 3 * Ws), dtype=np.uint8)
    lines[:, :, 1:] = out.reshape(T, Hs, 3 * Ws)
    return lines
