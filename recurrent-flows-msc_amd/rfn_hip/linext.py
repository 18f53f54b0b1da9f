"""Linear-extrapolation baseline (fused train and rollout) and its Gaussian-window SSIM: wrappers of
csrc/linear_extrap.hip.  rfn_hip.ops re-exports the public names."""
import functools

import torch

from . import lib as L
from .args import shape_label


@functools.lru_cache(maxsize=None)
def linext_limits():
    """(most conditioning frames, smallest and largest frame side of gauss_quality): the library's host-only queries
    (include/rfn_hip.h), read once; needs no device"""
    lib = L.load()
    return lib.rfn_linext_max_frames(), lib.rfn_gauss_quality_min_side(), lib.rfn_gauss_quality_max_side()


def linear_extrap_pairs(n):
    """the features of a window of n frames in the kernels' order (SimpleLinearModel.get_prediction): a list of
    (i, j or None), frame i itself or the difference frame i - frame j; n (n + 1) / 2 entries"""
    n = int(n)
    if n < 1:
        raise ValueError("linear_extrap_pairs: n must be >= 1, got %d" % n)
    pairs = [(f, None) for f in range(n)]
    for k in range(n - 1):
        pairs += [(j, j + k + 1) for j in range(n - k - 1)]
    return pairs


def linear_extrap_check(x, W, bias, n, start=0, P=None):
    """(B, T, CHW, F) of a linear_extrap_loss (P None) or linear_extrap_rollout call, or a ValueError naming what does
    not fit.  Needs no device."""
    who = "linear_extrap_loss" if P is None else "linear_extrap_rollout"
    for nm, v in (("n", n), ("start", start)) + ((("P", P),) if P is not None else ()):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s: %s must be an int, got %r" % (who, nm, v))
    if not 1 <= n <= linext_limits()[0]:
        raise ValueError("%s: n must be in 1..%d, got %d" % (who, linext_limits()[0], n))
    if start < 0:
        raise ValueError("%s: start must be >= 0, got %d" % (who, start))
    if P is not None and P < 1:
        raise ValueError("%s: P must be >= 1, got %d" % (who, P))
    for nm, t in (("x", x), ("W", W), ("bias", bias)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, nm, type(t).__name__))
        if t.dtype != torch.float32:
            raise ValueError("%s: %s must be float32, got %s" % (who, nm, t.dtype))
        if t.device != x.device:
            raise ValueError("%s: %s is on %s, x on %s" % (who, nm, t.device, x.device))
    if x.dim() != 5 or min(x.shape) < 1:
        raise ValueError("%s: x must be [B, T, C, H, W] with no empty dimension, got shape %s" % (who, tuple(x.shape)))
    B, T = int(x.shape[0]), int(x.shape[1])
    need = start + n + (1 if P is None else 0)
    if T < need:
        raise ValueError("%s: T = %d frames, start = %d and n = %d need T >= %d%s"
                         % (who, T, start, n, need, " (the window and its target)" if P is None else ""))
    F = n * (n + 1) // 2
    if W.numel() != F:
        raise ValueError("%s: W has %d elements (shape %s), n = %d needs F = n (n + 1) / 2 = %d"
                         % (who, W.numel(), tuple(W.shape), n, F))
    if bias.numel() != 1:
        raise ValueError("%s: bias has %d elements (shape %s), 1 is needed" % (who, bias.numel(), tuple(bias.shape)))
    CHW = int(x.shape[2]) * int(x.shape[3]) * int(x.shape[4])
    if B >= 2 ** 31 or (P is not None and P >= 2 ** 31):
        raise ValueError("%s: B and P must fit an int32" % who)
    return B, T, CHW, F


def _linext_frames(x):
    """(tensor, sequence stride, frame stride) of x [B, T, C, H, W] for the linear-extrapolation kernels: x itself when
    every frame is a dense block (a slice along B or T is read in place), a contiguous copy otherwise"""
    _, T, C, H, W = x.shape
    s = x.stride()
    dense = (W == 1 or s[4] == 1) and (H == 1 or s[3] == W) and (C == 1 or s[2] == H * W)
    if not dense or (T > 1 and s[1] < C * H * W) or (x.shape[0] > 1 and s[0] < (T - 1) * s[1] + C * H * W):
        x = x.contiguous()
        s = x.stride()
    fs = int(s[1]) if T > 1 else C * H * W
    ss = int(s[0]) if x.shape[0] > 1 else (T - 1) * fs + C * H * W
    return x, ss, fs


class LinearExtrapLossFn(torch.autograd.Function):
    """the MSE of the one-step prediction and the gradients of its 16-odd parameters in one pass over the frames
    (rfn_linext_train_f32, include/rfn_hip.h).  Saves the gradients; the backward scales them by the incoming scalar.
    There is no gradient to x."""

    @staticmethod
    def forward(ctx, x, W, bias, n, start):
        B, T, CHW, F = linear_extrap_check(x, W, bias, n, start)
        xv, ss, fs = _linext_frames(x.detach())
        w, b = W.detach().contiguous(), bias.detach().contiguous()
        ptrs = (L.dev(xv, "x", check_contiguous=False), L.dev(w, "W"), L.dev(b, "bias"))   # (device tensors or an error)
        partials = torch.empty(L.load().rfn_linext_max_blocks() * (F + 2), device=x.device, dtype=torch.float32)
        out = torch.empty(F + 2, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            L.call("rfn_linext_train_f32", ptrs[0], ss, fs, start, ptrs[1], ptrs[2], L.dev(partials), partials.numel(), L.dev(out), B, T, n, CHW,
                   meta=("shell", "linext_train", 0.0, shape_label(x), 4.0 * B * (n + 1) * CHW))
        ctx.save_for_backward(out)
        ctx.shapes = (tuple(W.shape), tuple(bias.shape), F)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        w_shape, b_shape, F = ctx.shapes
        need = ctx.needs_input_grad
        scaled = out[1:] * g    # one fp32 multiply per gradient
        return (None, scaled[:F].reshape(w_shape) if need[1] else None,
                scaled[F:].reshape(b_shape) if need[2] else None, None, None)


def linear_extrap_loss(x, W, bias, n, start=0):
    """MSE (mean over B*C*H*W) between the linear-extrapolation prediction from frames start .. start+n-1 of x
    [B, T, C, H, W] and frame start+n, differentiable in W [F] (any shape of F elements) and bias (one element).  Two
    launches on the current stream (the pass over the frames and the fixed-order sum of its partials); no CPU fallback."""
    linear_extrap_check(x, W, bias, n, start)
    return LinearExtrapLossFn.apply(x, W, bias, n, start)


def linear_extrap_rollout(x, W, bias, n, P, start=0):
    """[B, P, C, H, W]: P frames predicted autoregressively from the window x[:, start:start+n], each prediction
    replacing the window's oldest frame (SimpleLinearModel.sample; P = 1 is get_prediction).  No clamping, no gradient.
    One launch on the current stream; no CPU fallback."""
    B, T, CHW, _ = linear_extrap_check(x, W, bias, n, start, P)
    xv, ss, fs = _linext_frames(x.detach())
    w, b = W.detach().contiguous(), bias.detach().contiguous()
    ptrs = (L.dev(xv, "x", check_contiguous=False), L.dev(w, "W"), L.dev(b, "bias"))   # (device tensors or an error)
    out = torch.empty((B, P) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        L.call("rfn_linext_rollout_f32", ptrs[0], ss, fs, start, ptrs[1], ptrs[2], L.dev(out), B, T, n, P, CHW,
               meta=("shell", "linext_rollout", 0.0, shape_label(out), 4.0 * B * (n + P) * CHW))
    return out


def gauss_quality_check(pred, true, scale=255.0, lo=0.0, hi=255.0):
    """(N, C, H, W) of a gauss_quality call, or a ValueError naming what does not fit.  Needs no device."""
    for nm, t in (("pred", pred), ("true", true)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("gauss_quality: %s must be a tensor, got %s" % (nm, type(t).__name__))
        if t.dtype != torch.float32:
            raise ValueError("gauss_quality: %s must be float32, got %s" % (nm, t.dtype))
        if t.dim() != 4 or min(t.shape) < 1:
            raise ValueError("gauss_quality: %s must be [N, C, H, W] with no empty dimension, got shape %s"
                             % (nm, tuple(t.shape)))
    if tuple(pred.shape) != tuple(true.shape):
        raise ValueError("gauss_quality: shapes differ: pred %s, true %s" % (tuple(pred.shape), tuple(true.shape)))
    if pred.device != true.device:
        raise ValueError("gauss_quality: pred is on %s, true on %s" % (pred.device, true.device))
    N, C, H, W = (int(d) for d in pred.shape)
    _, side_min, side_max = linext_limits()
    for nm, v in (("H", H), ("W", W)):
        if not side_min <= v <= side_max:
            raise ValueError("gauss_quality: %s = %d, frames of %d..%d rows and columns are supported (the 11-tap window "
                             "needs 11; the kernel holds rows of at most 128)"
                             % (nm, v, side_min, side_max))
    scale, lo, hi = float(scale), float(lo), float(hi)
    if not (scale == scale and lo <= hi):
        raise ValueError("gauss_quality: scale must be a number and lo <= hi, got scale %r, lo %r, hi %r" % (scale, lo, hi))
    return N, C, H, W


def gauss_quality(pred, true, scale=255.0, lo=0.0, hi=255.0):
    """(ssim [N], psnr [N], mse [N]) of float32 frames [N, C, H, W], each read once as clamp(v * scale, lo, hi) (no
    scaled copy is written): ssim is pytorch_msssim.ssim(X, Y, data_range=255) per image (11-tap Gaussian window,
    sigma 1.5, no padding; DESIGN.md section 26 states it), mse the mean squared difference over C*H*W,
    psnr = 10 log10(255^2 / mse), +inf where mse == 0.  The data range of ssim and psnr is 255 whatever the scale.  One
    launch on the current stream; no CPU fallback."""
    N, C, H, W = gauss_quality_check(pred, true, scale, lo, hi)
    p, t = pred.detach().contiguous(), true.detach().contiguous()
    ptrs = (L.dev(p, "pred"), L.dev(t, "true"))   # (device tensors or an error)
    ssim = torch.empty(N, device=pred.device, dtype=torch.float32)
    mse = torch.empty_like(ssim)
    with torch.cuda.device(pred.device):
        L.call("rfn_gauss_quality_f32", ptrs[0], ptrs[1], L.dev(ssim), L.dev(mse), N, C, H, W,
               float(scale), float(lo), float(hi),
               meta=("shell", "gauss_quality", 0.0, shape_label(pred), 8.0 * pred.numel()))
    psnr = 10.0 * torch.log10(255.0 ** 2 / mse)   # (+inf at mse == 0: IEEE division)
    return ssim, psnr, mse
