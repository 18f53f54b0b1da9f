"""Float64 CPU restatement of RFN's importance-weighted bound, built from the oracle's pieces
(oracle/rfn_oracle.py: _rfn_states, _rfn_latent_step, _rfn_flow_conditions, listglow_log_prob, normal_log_prob), and a
host restatement of the addressed uniforms (csrc/iw_bound.hip) on the host Philox of tests/test_keyed_normal_host.py.
A helper, not a test: tests/test_iw_bound_host.py, tests/test_iw_kernels.py and tests/test_rfn_iw_bound.py use it.  The
noise is an input here; the chains run one at a time, one frame at a time."""
import math

import numpy as np
import torch

from oracle import rfn_oracle as O
from tests.test_keyed_normal_host import LO32, S32, U64, philox4x64_10_blocks


def state_dict64(model):
    """the model's state dict on the CPU, floating tensors as float64"""
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in model.state_dict().items()}


def iw_log_weights_ref(sd, cfg, x, eps, u):
    """log w [K, B] in float64.  sd: float64 state dict; cfg: vars(args); x [B, T, C, H, W] float64; eps[t - 1] [K, B, Z,
    h, w]: the posterior draws of step t; u[t - 1] [K, B, C, H, W]: the dequantisation noise of step t.  Per chain k and
    step t: encoder on (h_t, z^x_{t-1}, features of x_t) or (a_t, z^x_{t-1}); prior on (h_t, z^x_{t-1}), the chain's own
    sample whatever res_q is (zprev = zxprev in the oracle's latent step; its prior draw is unused: zeros); r_t = sum_j
    log N(z; pm, ps) - log N(z; em, es); l_t = -nll of the flow at x_t + u_t under cat(h_t, z^x_t)."""
    B, T = x.shape[0], x.shape[1]
    Kc = eps[0].shape[0]
    with torch.no_grad():
        feats, last, store_ht, store_at = O._rfn_states(sd, cfg, x, T, False)
        out = torch.zeros(Kc, B, dtype=torch.float64)
        for k in range(Kc):
            zx = sd["z_0x"]
            for i in range(1, T):
                pending = [torch.zeros_like(eps[i - 1][k]), eps[i - 1][k]]   # the oracle draws the prior's first
                _, zxt, pm, ps, em, es = O._rfn_latent_step(sd, cfg, i, feats, last, store_ht, store_at, zx, zx,
                                                            lambda shape=None: pending.pop(0), False)
                r = (O.normal_log_prob(zxt, pm, ps) - O.normal_log_prob(zxt, em, es)).sum(dim=(1, 2, 3))
                hz = torch.cat((store_ht[i - 1], zxt), 1)
                fc = O._rfn_flow_conditions(sd, cfg, hz, feats[i - 1], False)
                _, nll = O.listglow_log_prob(sd, "flow.", cfg, x[:, i], fc, hz, 0.0, u[i - 1][k], False)
                out[k] += r - nll
                zx = zxt
    return out


def iw_bound_ref(log_w):
    """bound[b] = logsumexp_k log w[k, b] - log K, float64"""
    log_w = log_w.double()
    return torch.logsumexp(log_w, 0) - math.log(log_w.shape[0])


def keyed_uniform_row(numel, seed, step, slot, seq, draw, scale=1.0):
    """one row of `numel` float32 values: block q = Philox(key = (seed, (step << 32) | slot), counter = (q, 0, seq,
    draw)); word w_i gives element 8q + 2i from its high half and 8q + 2i + 1 from its low half; value = (half >> 8) *
    2^-24 * scale, every product rounded to float32 (the first is exact)"""
    nblk = (numel + 7) // 8
    q = np.arange(nblk, dtype=U64)
    words = philox4x64_10_blocks(q, 0, int(seq), int(draw), (int(seed), (int(step) << 32) | int(slot)))
    w = np.stack(words, axis=1)                                      # [nblk, 4]
    halves = np.stack([w >> S32, w & LO32], axis=2).reshape(-1)      # high, low of w0, high, low of w1, ...
    v = (halves >> U64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (v * np.float32(scale))[:numel]


def keyed_uniform_ref(numel, B, n_draws, seed, first_step, n_steps=1, slot=24, scale=1.0, first_seq=0, first_draw=0):
    """float32 array [n_steps, n_draws*B, numel]: step-block s is step first_step + s, row r*B + b is draw first_draw + r
    of sequence first_seq + b"""
    out = np.zeros((n_steps, n_draws * B, numel), dtype=np.float32)
    for s in range(n_steps):
        for r in range(n_draws):
            for b in range(B):
                out[s, r * B + b] = keyed_uniform_row(numel, seed, first_step + s, slot, first_seq + b, first_draw + r,
                                                      scale)
    return out
