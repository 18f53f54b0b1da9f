"""The linear-extrapolation baseline (averagemodel/averagemodel.py:56-113 of the reference, its "simple linear model"):
every pixel of the next frame is a linear function of that pixel in the last `num_cond_frames` frames and in all their
lagged differences.  Same class name, parameters (`W [1, F]`, `bias [1, 1]`, zero-initialised; the reference's
state-dict keys) and methods.  `forward` and `sample` run on the fused kernels (rfn_hip.ops.linear_extrap_loss /
linear_extrap_rollout, csrc/linear_extrap.hip): no feature frames are materialised, the loss and all gradients come
from one pass over the frames, and the rollout keeps its window in registers.  `get_lagged_differences` stays the torch
expression: it is the documented feature order.

One deviation: the reference hard-codes `self.c = 3` for the reshape of its prediction; here the channel count comes
from the data.  DESIGN.md section 26."""
import torch
import torch.nn as nn

from rfn_hip import ops


class SimpleLinearModel(nn.Module):
    def __init__(self, num_cond_frames=9):
        super(SimpleLinearModel, self).__init__()
        num_cond_frames = int(num_cond_frames)
        if not 1 <= num_cond_frames <= ops.linext_limits()[0]:
            raise ValueError("SimpleLinearModel: num_cond_frames must be in 1..%d, got %d"
                             % (ops.linext_limits()[0], num_cond_frames))
        num_features = num_cond_frames * (num_cond_frames + 1) // 2
        self.W = nn.Parameter(torch.zeros(1, num_features))
        self.bias = nn.Parameter(torch.zeros(1, 1))
        self.num_cond_frames = num_cond_frames

    def get_lagged_differences(self, x):
        """:65-71: x [B, n, ...] -> [B, n (n - 1) / 2, ...], lag k + 1 for k = 0 .. n-2, inside that x_j - x_{j+k+1}"""
        laggeddif = []
        length = x.shape[1]
        for k in range(0, (x.shape[1] - 1)):
            laggeddif.append(x[:, 0:(length - k - 1)] - x[:, (k + 1):length])
        if not laggeddif:   # (one conditioning frame has no differences; the reference's torch.cat would raise)
            return x[:, 0:0]
        return torch.cat(laggeddif, dim=1)

    def get_prediction(self, x_use):
        """:72-81: the next frame [B, C, H, W] from the window x_use [B, n, C, H, W] (no gradient: the rollout kernel at
        P = 1)"""
        return ops.linear_extrap_rollout(x_use, self.W, self.bias, self.num_cond_frames, 1)[:, 0]

    def forward(self, x):
        """:82-90: MSE between the prediction from x[:, 0:n] and x[:, n], differentiable in W and bias"""
        return ops.linear_extrap_loss(x, self.W, self.bias, self.num_cond_frames)

    def sample(self, x, num_predictions):
        """:105-113: [B, num_predictions, C, H, W], rolled out from the window x[:, 0:n]; no clamping"""
        return ops.linear_extrap_rollout(x, self.W, self.bias, self.num_cond_frames, int(num_predictions))

    def ssim_val(self, X, Y, n_bits=8):
        """:91-96: pytorch_msssim.ssim(X, Y, data_range=2^n_bits - 1) of frames [N, C, H, W] already on the 0..255
        scale: the batch mean of rfn_hip.ops.gauss_quality.  Only n_bits = 8 is supported (the kernel's constants)."""
        if n_bits != 8:
            raise ValueError("SimpleLinearModel.ssim_val: only n_bits = 8 is supported, got %r" % (n_bits,))
        return ops.gauss_quality(X, Y, scale=1.0, lo=float("-inf"), hi=float("inf"))[0].mean()

    def PSNRbatch(self, X, Y, n_bits=8):
        """:97-104: the batch mean of the per-image 10 log10((2^n_bits - 1)^2 / mean((X - Y)^2))"""
        if n_bits != 8:
            raise ValueError("SimpleLinearModel.PSNRbatch: only n_bits = 8 is supported, got %r" % (n_bits,))
        return ops.gauss_quality(X, Y, scale=1.0, lo=float("-inf"), hi=float("inf"))[1].mean()
