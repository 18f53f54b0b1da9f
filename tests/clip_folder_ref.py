"""numpy restatements of the two contracts of DESIGN.md section 27, written from their definitions (not from the
kernels): the exact integer area-mean resize of rfn_frames_resize_u8 with its crop window, and the strided, mirrored,
time-reversed gather of rfn_clip_gather_aug_u8_f32.  tests/test_frame_resize.py, tests/test_clip_gather_aug.py,
tests/test_clip_folder.py and tests/test_clip_folder_host.py compare against them."""
import numpy as np


def window_ref(Hs, Ws, H, W, mode):
    """(y0, x0, Hc, Wc): "stretch" the whole frame, "crop" the largest centred window of the target's aspect ratio"""
    if mode == "stretch":
        return 0, 0, Hs, Ws
    assert mode == "crop"
    if Ws * H >= Hs * W:
        Hc, Wc = Hs, max(1, Hs * W // H)
    else:
        Wc, Hc = Ws, max(1, Ws * H // W)
    return (Hs - Hc) // 2, (Ws - Wc) // 2, Hc, Wc


def axis_weights(n_out, n_crop):
    """int64 [n_out, n_crop]: w[y, i] = the overlap of output cell [y * n_crop, (y + 1) * n_crop) and source cell
    [i * n_out, (i + 1) * n_out); 0 outside i = floor(y * n_crop / n_out) .. ceil((y + 1) * n_crop / n_out) - 1"""
    y = np.arange(n_out, dtype=np.int64)[:, None]
    i = np.arange(n_crop, dtype=np.int64)[None, :]
    w = np.minimum((y + 1) * n_crop, (i + 1) * n_out) - np.maximum(y * n_crop, i * n_out)
    w = np.maximum(w, 0)
    assert (w.sum(1) == n_crop).all()
    lo, hi = y[:, 0] * n_crop // n_out, -(-(y[:, 0] + 1) * n_crop // n_out) - 1
    inside = (i >= lo[:, None]) & (i <= hi[:, None])
    assert ((w > 0) == inside).all()          # every weight of the stated range is positive, every other one 0
    return w


def weighted_sums(src, H, W, window):
    """(int64 [F, H, W, Cs] of sum_i sum_j wy(i) wx(j) src[y0 + i, x0 + j, c], Hc * Wc)"""
    y0, x0, Hc, Wc = window
    crop = np.asarray(src)[:, y0:y0 + Hc, x0:x0 + Wc, :].astype(np.int64)
    assert crop.shape[1:3] == (Hc, Wc)
    wy, wx = axis_weights(H, Hc), axis_weights(W, Wc)
    rows = np.tensordot(wy, crop, axes=(1, 1))                  # [H, F, Wc, C]
    s = np.tensordot(wx, rows, axes=(1, 2))                     # [W, H, F, C]
    return np.ascontiguousarray(s.transpose(2, 1, 0, 3)), Hc * Wc


def resize_ref(src, H, W, Cd, window=None):
    """uint8 [F, H, W, Cd] of uint8 [F, Hs, Ws, Cs]: area mean rounded half up, then the channel rule on the bytes"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4
    if window is None:
        window = (0, 0, src.shape[1], src.shape[2])
    s, area = weighted_sums(src, H, W, window)
    v = (s + area // 2) // area
    Cs = src.shape[3]
    if Cs == 3 and Cd == 1:
        v = (19595 * v[..., 0:1] + 38470 * v[..., 1:2] + 7471 * v[..., 2:3] + 32768) >> 16
    elif Cs == 1 and Cd == 3:
        v = np.repeat(v, 3, axis=3)
    else:
        assert Cs == Cd
    assert v.min(initial=0) >= 0 and v.max(initial=0) <= 255
    return v.astype(np.uint8)


def gather_aug_ref(store, first, T, C, step=1, flags=None):
    """float32 [B, T, C, H, W] of the uint8 store [F, H, W, Cs]: out[b, t, c, y, x] = float32(byte) / float32(255) of
    store[first[b] + tt * step, y, xx, c'], tt = T - 1 - t under bit 1, xx = W - 1 - x under bit 0; a clip with
    first[b] < 0 or first[b] + (T - 1) * step + 1 > F is NaN"""
    store = np.asarray(store)
    F, H, W, Cs = store.shape
    first = [int(f) for f in np.asarray(first).reshape(-1)]
    flags = [0] * len(first) if flags is None else [int(f) for f in np.asarray(flags).reshape(-1)]
    out = np.full((len(first), T, C, H, W), np.nan, dtype=np.float32)
    for b, (f0, fl) in enumerate(zip(first, flags)):
        if f0 < 0 or f0 + (T - 1) * step + 1 > F:
            continue
        for t in range(T):
            tt = T - 1 - t if fl & 2 else t
            frame = store[f0 + tt * step]                         # [H, W, Cs]
            if fl & 1:
                frame = frame[:, ::-1, :]
            for c in range(C):
                out[b, t, c] = frame[:, :, c if Cs == C else 0].astype(np.float32) / np.float32(255)
    return out
