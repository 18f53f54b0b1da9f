"""float64 restatement of the two definitions of csrc/pixel_loglik.hip (include/rfn_hip.h), evaluated on the float32
inputs, and the length of the longest chain of additions of the kernel's documented summation order."""
import math

import torch

EPS = 2.0 ** -23
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def pixel_terms64(pred, target, mode, scale=None, noise=None):
    """float64 [R, N]: the terms l(pred[r, n], x[r, n]), x = target[r % B] (+ noise[r]); any device"""
    R, B = pred.shape[0], target.shape[0]
    p = pred.reshape(R, -1).double()
    x = target.reshape(B, -1).double().repeat(R // B, 1)
    if noise is not None:
        x = x + noise.reshape(R, -1).double()
    if mode == "bernoulli":
        pc = p.clamp(EPS, 1.0 - EPS)
        return x * torch.log(pc) + (1.0 - x) * torch.log1p(-pc)
    if mode == "gaussian":
        s = float(scale)
        return -(x - p) ** 2 / (2.0 * s * s) - math.log(s) - HALF_LOG_2PI
    if mode == "mse":
        return -(p - x) ** 2
    raise ValueError(mode)


def pixel_loglik64(pred, target, mode, scale=None, noise=None):
    """(row sums [R], sum of the terms' magnitudes [R]) in float64"""
    t = pixel_terms64(pred, target, mode, scale, noise)
    return t.sum(1), t.abs().sum(1)


def normal_logvar_terms64(mu, logvar, z):
    """float64 [B, Z]: -logvar / 2 - (z - mu)^2 exp(-logvar) / 2 - log(2 pi) / 2"""
    mu, logvar, z = mu.double(), logvar.double(), z.double()
    return -0.5 * logvar - (z - mu) ** 2 * torch.exp(-logvar) * 0.5 - HALF_LOG_2PI


LANES = 256   # one workgroup per row
GROUP = 4     # consecutive elements of one group


def lane_elements(N, lane):
    """how many of a row's N terms lane `lane` adds: its groups are lane, lane + 256, ... of the ceil(N / 4) groups of
    four consecutive elements, the last of which may be short"""
    groups = -(-N // GROUP)
    return sum(min(GROUP, N - GROUP * g) for g in range(lane, groups, LANES))


def longest_chain(N):
    """A(N): the additions on the longest path from a term to out[r].  A lane adds its L terms one after the other to a
    sum that starts at +0 (the first addition is exact: L - 1 rounded ones); lane 0 has the most.  Then six butterfly
    additions inside the wavefront and three to combine the four wavefront sums."""
    if N < 1:
        raise ValueError("N >= 1")
    return max(lane_elements(N, 0) - 1, 0) + 6 + 3
