"""Row-summed pixel log-likelihoods and SVG's pair of Normal densities for the baselines' importance-weighted bound:
wrappers of csrc/pixel_loglik.hip (forward only).  rfn_hip.ops re-exports the public names."""
import math
import os

import torch

from . import lib as L

PIXEL_LOGLIK_MODES = ("bernoulli", "gaussian", "mse")   # the header's RFN_PIXEL_LOGLIK_* in this order

# Route of the models' call sites for float32 device tensors without a gradient when RFN_PIXEL_LOGLIK is unset (DESIGN.md
# section 29 has the measurement it follows): True = the kernels, False = the torch chain.
PIXEL_LOGLIK_KERNEL_DEFAULT = True


def pixel_loglik_route(*tensors):
    """"kernel" or "torch" for a likelihood of the bound computed from `tensors` (None entries are skipped): the
    kernels have no backward pass, so "torch" whenever a gradient could be asked for (grad mode on and one of the tensors
    requires grad), for CPU or non-float32 tensors, and with RFN_PIXEL_LOGLIK=0 (read at every call, the counterpart of
    RFN_LSTM_CELL=0); RFN_PIXEL_LOGLIK=1 or unset: PIXEL_LOGLIK_KERNEL_DEFAULT decides when unset."""
    tensors = [t for t in tensors if t is not None]
    if not tensors or any(not t.is_cuda or t.dtype != torch.float32 for t in tensors):
        return "torch"
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return "torch"
    env = os.environ.get("RFN_PIXEL_LOGLIK")
    if env in ("0", "1"):
        return "kernel" if env == "1" else "torch"
    return "kernel" if PIXEL_LOGLIK_KERNEL_DEFAULT else "torch"


def _rows_dense(t):
    """every row of t (all dimensions after the first) is one dense block"""
    exp = 1
    for d in range(t.dim() - 1, 0, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            return False
        exp *= t.shape[d]
    return True


def pixel_loglik_check(pred, target, mode, scale=None, noise=None):
    """(R, B, N) of a pixel_loglik call, or a ValueError naming what does not fit.  Needs no device."""
    if mode not in PIXEL_LOGLIK_MODES:
        raise ValueError("pixel_loglik: mode is one of %s, got %r" % (PIXEL_LOGLIK_MODES, mode))
    if mode == "gaussian":
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not (0.0 < float(scale) < math.inf):
            raise ValueError("pixel_loglik: mode 'gaussian' needs scale, a positive finite Python float, got %r" % (scale,))
    elif scale is not None:
        raise ValueError("pixel_loglik: scale belongs to mode 'gaussian' only, got scale = %r with mode %r" % (scale, mode))
    given = {"pred": pred, "target": target}
    if noise is not None:
        given["noise"] = noise
    for n, t in given.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError("pixel_loglik: %s must be a tensor, got %s" % (n, type(t).__name__))
        if t.dtype != torch.float32:
            raise ValueError("pixel_loglik: tensors are float32; %s is %s" % (n, t.dtype))
        if t.device != pred.device:
            raise ValueError("pixel_loglik: %s is on %s, pred on %s" % (n, t.device, pred.device))
        if t.dim() < 2:
            raise ValueError("pixel_loglik: %s must be [rows, N] or [rows, C, H, W], got shape %s" % (n, tuple(t.shape)))
    R, B = int(pred.shape[0]), int(target.shape[0])
    N = 1
    for d in pred.shape[1:]:
        N *= int(d)
    n_target = 1
    for d in target.shape[1:]:
        n_target *= int(d)
    if N < 1 or n_target != N:
        raise ValueError("pixel_loglik: pred has N = %d values per row (shape %s), target %d (shape %s); N >= 1 and equal"
                         % (N, tuple(pred.shape), n_target, tuple(target.shape)))
    if B < 1 or R % B != 0:
        raise ValueError("pixel_loglik: pred has R = %d rows, target B = %d: R must be K * B (row k * B + b is scored "
                         "against target row b)" % (R, B))
    if R > 2 ** 31 - 1:
        raise ValueError("pixel_loglik: R = %d rows, at most 2^31 - 1" % R)
    if noise is not None and tuple(noise.shape) != tuple(pred.shape):
        raise ValueError("pixel_loglik: noise has shape %s, pred %s" % (tuple(noise.shape), tuple(pred.shape)))
    for n in ("pred", "noise"):
        if n in given and not given[n].is_contiguous():
            raise ValueError("pixel_loglik: %s must be contiguous, got shape %s stride %s"
                             % (n, tuple(given[n].shape), tuple(given[n].stride())))
    if not _rows_dense(target) or (B > 1 and target.stride(0) < N):
        raise ValueError("pixel_loglik: every row of target must be dense, got shape %s stride %s"
                         % (tuple(target.shape), tuple(target.stride())))
    return R, B, N


def pixel_loglik(pred, target, mode, scale=None, noise=None, out=None):
    """out [R] float32, out[r] = sum_n l(pred[r, n], x[r, n]): the row-summed log-likelihood of the R = K * B rows of
    pred ([R, N] or [R, C, H, W], row k * B + b) under the B rows of target ([B, N] or [B, C, H, W]; a view whose rows are
    dense is read in place, e.g. x[:, i] of a [B, T, C, H, W] batch), which is never repeated in memory.  noise [R, N]
    (optional) is added to the target of its row: x = target[r % B] + noise[r].
      "bernoulli"  l = x log(pc) + (1 - x) log1p(-pc), pc = clamp(p, 2^-23, 1 - 2^-23)   (td.Bernoulli(probs=p).log_prob(x))
      "gaussian"   l = -(x - p)^2 / (2 scale^2) - log(scale) - log(2 pi) / 2             (td.Normal(p, scale).log_prob(x))
      "mse"        l = -(p - x)^2
    scale: a positive finite Python float, for "gaussian" only.  One launch on the current stream, fixed summation order
    (include/rfn_hip.h): a row's bits depend on that row alone.  R = 0 returns an empty tensor without a launch.  out
    (optional): the contiguous float32 [R] tensor on pred's device to write to.  No backward pass and no CPU fallback."""
    R, B, N = pixel_loglik_check(pred, target, mode, scale, noise)
    p_pred = L.dev(pred.detach(), "pred")
    p_target = L.dev(target.detach(), "target", check_contiguous=False)
    p_noise = L.dev(None if noise is None else noise.detach(), "noise")
    if out is None:
        out = torch.empty((R,), device=pred.device, dtype=torch.float32)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != pred.device
          or tuple(out.shape) != (R,) or not out.is_contiguous()):
        raise ValueError("pixel_loglik: out must be a contiguous float32 [%d] tensor on %s" % (R, pred.device))
    if R == 0:
        return out
    stride = int(target.stride(0)) if B > 1 else N
    nbytes = 4.0 * (R * N * (2 if noise is not None else 1) + B * N + R)
    L.call("rfn_pixel_loglik_f32", p_pred, p_target, stride, p_noise, L.dev(out), R, B, N,
           PIXEL_LOGLIK_MODES.index(mode), float(scale) if mode == "gaussian" else 0.0,
           meta=("shell", "pixel_loglik_" + mode, 0.0, "%dx%d" % (R, N), nbytes))
    return out


def normal_logvar_pair_check(mu_a, logvar_a, z_a, mu_b, logvar_b, z_b):
    """(B, Z) of a normal_logvar_pair call, or a ValueError naming what does not fit.  Needs no device."""
    given = {"mu_a": mu_a, "logvar_a": logvar_a, "z_a": z_a, "mu_b": mu_b, "logvar_b": logvar_b, "z_b": z_b}
    for n, t in given.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError("normal_logvar_pair: %s must be a tensor, got %s" % (n, type(t).__name__))
        if t.dtype != torch.float32:
            raise ValueError("normal_logvar_pair: tensors are float32; %s is %s" % (n, t.dtype))
        if t.device != mu_a.device:
            raise ValueError("normal_logvar_pair: %s is on %s, mu_a on %s" % (n, t.device, mu_a.device))
    if mu_a.dim() != 2 or mu_a.shape[0] < 1 or mu_a.shape[1] < 1:
        raise ValueError("normal_logvar_pair: inputs are [B, Z] with B, Z >= 1, got mu_a %s" % (tuple(mu_a.shape),))
    for n, t in given.items():
        if tuple(t.shape) != tuple(mu_a.shape):
            raise ValueError("normal_logvar_pair: %s has shape %s, mu_a %s" % (n, tuple(t.shape), tuple(mu_a.shape)))
    return int(mu_a.shape[0]), int(mu_a.shape[1])


def normal_logvar_pair(mu_a, logvar_a, z_a, mu_b, logvar_b, z_b):
    """(out_a, out_b), float32 [B] each: out_a[b] = sum_j -logvar_a / 2 - (z_a - mu_a)^2 exp(-logvar_a) / 2 - log(2 pi) / 2,
    the row-summed density of N(mu_a, exp(logvar_a / 2)) at z_a, and the same of the b triple; the caller chooses which z
    goes with which distribution.  Six float32 [B, Z] device tensors, one launch on the current stream for both, fixed
    summation order.  No backward pass and no CPU fallback."""
    B, Z = normal_logvar_pair_check(mu_a, logvar_a, z_a, mu_b, logvar_b, z_b)
    ins = [t.detach().contiguous() for t in (mu_a, logvar_a, z_a, mu_b, logvar_b, z_b)]
    ptrs = [L.dev(t, n) for t, n in zip(ins, ("mu_a", "logvar_a", "z_a", "mu_b", "logvar_b", "z_b"))]
    out = torch.empty((2, B), device=mu_a.device, dtype=torch.float32)
    L.call("rfn_normal_logvar_pair_f32", *ptrs, L.dev(out[0]), L.dev(out[1]), B, Z,
           meta=("shell", "normal_logvar_pair", 0.0, "%dx%d" % (B, Z), 4.0 * (6 * B * Z + 2 * B)))
    return out[0], out[1]
