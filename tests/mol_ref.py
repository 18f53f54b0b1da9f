"""The mixture of discretized logistics written out from its definition in plain torch ops on
NCHW tensors, in whatever dtype and on whatever device the inputs have: the float64 yardstick of tests/test_mol*.py
and tests/test_srnn.py, and (in float32, on the GPU) the op chain tools/bench_mol.py times the kernels against.

  x [N,C,H,W] in [-1,1], C in {1,3};  l [N,Cl,H,W], Cl = M (1 + P C), P = 3 for C = 3 and 2 for C = 1
  channel m                     mixture logit of component m
  channel M + (c P + j) M + m   parameter j (0 mean, 1 log-scale, 2 coefficient) of colour channel c, component m
"""
import math

import torch
import torch.nn.functional as F

MIN_LOG_SCALE = -7.0
BIN = 1.0 / 255.0
THRESH = 1e-5


def split(l, C):
    """(logits [N,M,H,W], params [N,C,P,M,H,W]) views of l"""
    N, Cl, H, W = l.shape
    P = 3 if C == 3 else 2
    if C not in (1, 3) or Cl % (1 + P * C):
        raise ValueError("l has %d channels, which is no M*(1+%d*%d)" % (Cl, P, C))
    M = Cl // (1 + P * C)
    return l[:, :M], l[:, M:].reshape(N, C, P, M, H, W)


def means_of(x, par):
    """the component means [N,C,M,H,W] after the RGB conditioning on the observed x_0, x_1"""
    mu = par[:, :, 0]
    if x.shape[1] == 3:
        t = torch.tanh(par[:, :, 2])
        x0, x1 = x[:, 0:1], x[:, 1:2]
        mu = torch.stack([mu[:, 0], mu[:, 1] + t[:, 0] * x0, mu[:, 2] + t[:, 1] * x0 + t[:, 2] * x1], 1)
    return mu


def items(x, l):
    """log-probability of every (frame, colour channel, component, pixel) item [N,C,M,H,W], and its cdf_delta"""
    C = x.shape[1]
    logits, par = split(l, C)
    mu = means_of(x, par)
    ls = torch.clamp(par[:, :, 1], min=MIN_LOG_SCALE)
    xe = x.unsqueeze(2).expand_as(mu)
    cx = xe - mu
    inv = torch.exp(-ls)
    plus, minus, mid = inv * (cx + BIN), inv * (cx - BIN), inv * cx
    delta = torch.sigmoid(plus) - torch.sigmoid(minus)
    log_cdf_plus = plus - F.softplus(plus)
    log_one_minus_cdf_min = -F.softplus(minus)
    log_pdf_mid = mid - ls - 2.0 * F.softplus(mid)
    inner = torch.where(delta > THRESH, torch.log(torch.clamp(delta, min=1e-12)), log_pdf_mid - math.log(127.5))
    lp = torch.where(xe < -0.999, log_cdf_plus, torch.where(xe > 0.999, log_one_minus_cdf_min, inner))
    return lp, delta


def nll_pix(x, l):
    """negative log-likelihood per pixel [N,H,W]; differentiable in l"""
    logits, _ = split(l, x.shape[1])
    lp, _ = items(x, l)
    return -torch.logsumexp(lp.sum(1) + torch.log_softmax(logits, 1), 1)


def near_threshold(x, l, rel=0.01):
    """[N,H,W] bool: pixels with an item on the cdf_delta branches whose cdf_delta lies within `rel` of the threshold
    (the select is discontinuous there; an edge-branch item does not look at cdf_delta)"""
    _, delta = items(x, l)
    xe = x.unsqueeze(2).expand_as(delta)
    close = ((delta - THRESH).abs() <= rel * THRESH) & (xe >= -0.999) & (xe <= 0.999)
    return close.any(2).any(1)


def sample(l, u_mix, u_x):
    """(x [N,C,H,W], gap [N,H,W]) from uniforms u_mix [N,H,W,M], u_x [N,H,W,C]; gap = best minus second-best Gumbel
    score (inf for M = 1)"""
    C = u_x.shape[-1]
    logits, par = split(l, C)
    N, M, H, W = logits.shape
    score = logits - torch.log(-torch.log(u_mix.permute(0, 3, 1, 2)))
    best = score.argmax(1, keepdim=True)
    if M > 1:
        top = score.topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
    else:
        gap = torch.full((N, H, W), math.inf, dtype=l.dtype, device=l.device)
    idx = best.view(N, 1, 1, 1, H, W).expand(N, C, par.shape[2], 1, H, W)
    sel = par.gather(3, idx).squeeze(3)                       # [N,C,P,H,W]
    u = u_x.permute(0, 3, 1, 2)
    v = sel[:, :, 0] + torch.exp(torch.clamp(sel[:, :, 1], min=MIN_LOG_SCALE)) * (torch.log(u) - torch.log(1.0 - u))
    x0 = v[:, 0].clamp(-1.0, 1.0)
    if C == 1:
        return x0.unsqueeze(1), gap
    t = torch.tanh(sel[:, :, 2])
    x1 = (v[:, 1] + t[:, 0] * x0).clamp(-1.0, 1.0)
    x2 = (v[:, 2] + t[:, 1] * x0 + t[:, 2] * x1).clamp(-1.0, 1.0)
    return torch.stack([x0, x1, x2], 1), gap
