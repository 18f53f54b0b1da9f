"""Seeded fill of an SRNN state_dict, shared by tests/golden/make_golden_srnn.py (which fills the reference's model) and
tests/test_srnn*.py (which fill the package's): the fixtures then need no stored parameters, only the key list, the
shapes and a checksum per tensor.  Entries are filled in sorted key order from one torch.Generator:
  integer entries (num_batches_tracked)   0
  *.running_var                           0.5 + |n|
  *.running_mean                          0.1 n
  tensors with two or more dimensions     n sqrt(2 / fan_in), fan_in = the elements of one slice along dimension 0
                                          (top-level initial states such as z_0, h_0 are batch-major: 0.5 n)
  one-dimensional *.weight (norm scales)  1 + 0.1 n
  everything else (biases, variance)      0.1 n
with n ~ N(0, 1): activations stay O(1) through the ReLU stacks."""
import math

import torch


def fill_state(sd, seed):
    """{key: float32 / integer CPU tensor} for the keys and shapes of `sd`"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in sorted(sd):
        v = sd[k]
        if not v.is_floating_point():
            out[k] = torch.zeros(v.shape, dtype=v.dtype)
            continue
        n = torch.randn(tuple(v.shape), generator=g, dtype=torch.float32)
        if k.endswith("running_var"):
            t = 0.5 + n.abs()
        elif k.endswith("running_mean"):
            t = 0.1 * n
        elif "." not in k and v.dim() >= 2:
            t = 0.5 * n
        elif v.dim() >= 2:
            t = n * math.sqrt(2.0 / v[0].numel())
        elif k.endswith(".weight"):
            t = 1.0 + 0.1 * n
        else:
            t = 0.1 * n
        out[k] = t
    return out


def checksum(t):
    """position-weighted float64 sum of a tensor (a plain float): tells two fills apart, permutations included"""
    f = t.detach().double().reshape(-1).cpu()
    w = (torch.arange(f.numel(), dtype=torch.float64) % 251.0) + 1.0
    return float((f * w).sum())


def describe(sd):
    """([keys], [shapes], [checksums]) in sorted key order"""
    keys = sorted(sd)
    return keys, [list(sd[k].shape) for k in keys], [checksum(sd[k]) for k in keys]
