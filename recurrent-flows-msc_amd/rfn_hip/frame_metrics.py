"""Per-frame MSE / PSNR / SSIM of uint8 videos: wrappers of csrc/frame_metrics.hip.  rfn_hip.ops re-exports the public
names."""
import torch

from . import lib as L
from .args import shape_label


def _u8_frames(t, C, H, W):
    """(tensor, pointer, frame stride) of a uint8 device tensor [..., C, H, W] seen as [N, C, H, W] frames (lib.dev stays
    fp32-only): no copy when the leading dims collapse to one frame stride and every frame is dense and disjoint (e.g.
    a channel slice), a contiguous copy otherwise (e.g. `x[:, start:]` of [B, T, C, H, W]).  Returns the tensor the
    pointer refers to as well: the caller keeps it alive over the launch."""
    v = t.reshape(-1, C, H, W)
    s = v.stride()
    dense = s[3] == 1 and s[2] == W and (s[1] == H * W or C == 1)
    if not dense or (v.shape[0] > 1 and s[0] < C * H * W):
        v = v.contiguous()
    ns = v.stride(0) if v.shape[0] > 1 else C * H * W
    return v, v.data_ptr(), int(ns)


def frame_quality(a, b):
    """Per-frame (mse, psnr, ssim) of two uint8 video tensors [..., C, H, W] on the GPU (rfn_frame_quality_u8: the
    reference's Evaluator.eval_seq, error_metrics.py:154-171, with skimage 0.17.2's SSIM / PSNR defaults): float32
    tensors over the leading shape.  mse = sum of squared differences / (C*H*W); psnr, ssim = means over channels of the
    single-channel figures (psnr is +inf on an identical channel).  No CPU fallback."""
    for t, nm in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("frame_quality: %s must be a tensor, got %s" % (nm, type(t).__name__))
        if t.dtype != torch.uint8:
            raise TypeError("frame_quality: %s must be uint8, got %s" % (nm, t.dtype))
        if t.dim() < 3:
            raise ValueError("frame_quality: %s must be [..., C, H, W], got shape %s" % (nm, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("frame_quality: shapes differ: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    C, H, W = (int(d) for d in a.shape[-3:])
    if H < 7 or W < 7:
        raise ValueError("frame_quality: the 7x7 SSIM window exceeds the %dx%d frame" % (H, W))
    if C < 1:
        raise ValueError("frame_quality: frames have no channel")
    for t, nm in ((a, "a"), (b, "b")):
        if not t.is_cuda:
            raise RuntimeError("rfn_hip kernels need device tensors; %s is on %s (no CPU fallback)" % (nm, t.device))
    if a.device != b.device:
        raise ValueError("frame_quality: a is on %s, b on %s" % (a.device, b.device))
    lead = tuple(a.shape[:-3])
    mse = torch.empty(lead, device=a.device, dtype=torch.float32)
    psnr = torch.empty_like(mse)
    ssim = torch.empty_like(mse)
    N = mse.numel()
    if N == 0:
        return mse, psnr, ssim
    av, ap, ans = _u8_frames(a, C, H, W)
    bv, bp, bns = _u8_frames(b, C, H, W)
    with torch.cuda.device(a.device):
        L.call("rfn_frame_quality_u8", ap, ans, bp, bns, L.dev(mse), L.dev(psnr), L.dev(ssim), N, C,
               H, W, meta=("shell", "frame_quality", 0.0, shape_label(a), 2.0 * a.numel()))
    return mse, psnr, ssim
