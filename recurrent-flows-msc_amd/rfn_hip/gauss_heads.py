"""The diagonal Gaussians of one VRNN step: wrappers of csrc/gauss_heads.hip.  rfn_hip.ops re-exports the public names."""
import torch

from . import lib as L
from .args import shell


GAUSS_HEADS_OUTPUTS = ("z_q", "z_p", "q_scale", "p_scale", "kl", "logq", "logp")
# what each output reads beside p_loc / p_raw, which every call needs
_GAUSS_HEADS_NEEDS = {"z_q": ("q_loc", "q_raw", "eps_q"), "z_p": ("eps_p",), "q_scale": ("q_loc", "q_raw"), "p_scale": (),
                      "kl": ("q_loc", "q_raw"), "logq": ("q_loc", "q_raw", "eps_q"), "logp": ("eps_p",)}


def gauss_heads_check(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want):
    """(B, Z) of a gauss_heads call, or a ValueError naming what does not fit.  Needs no device."""
    given = {"q_loc": q_loc, "q_raw": q_raw, "p_loc": p_loc, "p_raw": p_raw, "eps_q": eps_q, "eps_p": eps_p}
    want = tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in GAUSS_HEADS_OUTPUTS for w in want):
        raise ValueError("gauss_heads: want must name distinct outputs of %s, got %r" % (GAUSS_HEADS_OUTPUTS, want))
    if p_loc is None or p_raw is None:
        raise ValueError("gauss_heads: p_loc and p_raw are always needed")
    if (q_loc is None) != (q_raw is None):
        raise ValueError("gauss_heads: q_loc and q_raw come together (both None: the prior-only form)")
    if q_loc is None and eps_q is not None:
        raise ValueError("gauss_heads: eps_q without q_loc / q_raw")
    for w in want:
        missing = [n for n in _GAUSS_HEADS_NEEDS[w] if given[n] is None]
        if missing:
            raise ValueError("gauss_heads: output %r needs %s" % (w, ", ".join(missing)))
    if p_loc.dim() != 2 or p_loc.shape[0] < 1 or p_loc.shape[1] < 1:
        raise ValueError("gauss_heads: inputs are [B, Z] with B, Z >= 1, got p_loc %s" % (tuple(p_loc.shape),))
    for n, t in given.items():
        if t is not None and tuple(t.shape) != tuple(p_loc.shape):
            raise ValueError("gauss_heads: %s has shape %s, p_loc %s" % (n, tuple(t.shape), tuple(p_loc.shape)))
    return int(p_loc.shape[0]), int(p_loc.shape[1])


class GaussHeadsFn(torch.autograd.Function):
    """the diagonal Gaussians of one VRNN step in one kernel each way (rfn_gauss_heads_{fwd,bwd}_f32, include/rfn_hip.h):
    returns the seven GAUSS_HEADS_OUTPUTS in that order, None where `want` does not name one.  Saves the six inputs
    only; the backward recomputes sigma."""

    @staticmethod
    def forward(ctx, q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want):
        ctx.set_materialize_grads(False)  # unused outputs arrive as None
        B, Z = gauss_heads_check(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want)
        ins = [None if t is None else t.contiguous() for t in (q_loc, q_raw, p_loc, p_raw, eps_q, eps_p)]
        ptrs = [L.dev(t, n) for t, n in zip(ins, ("q_loc", "q_raw", "p_loc", "p_raw", "eps_q", "eps_p"))]
        outs = []
        for name in GAUSS_HEADS_OUTPUTS:
            shape = (B,) if name in ("kl", "logq", "logp") else (B, Z)
            outs.append(torch.empty(shape, device=p_loc.device, dtype=torch.float32) if name in want else None)
        L.call("rfn_gauss_heads_fwd_f32", *ptrs, *[L.dev(o) for o in outs], B, Z,
               meta=shell("gauss_heads_fwd", p_loc, sum(t is not None for t in ins + outs)))
        ctx.save_for_backward(*ins)
        ctx.cfg = (B, Z)
        # the ABI has no upstream gradient for the scales: they are values (the KL and the densities are outputs of their own)
        ctx.mark_non_differentiable(*[o for o in outs[2:4] if o is not None])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_zq, g_zp, g_qs, g_ps, g_kl, g_logq, g_logp):
        ins = ctx.saved_tensors
        q_loc, p_loc = ins[0], ins[2]
        B, Z = ctx.cfg
        # g_zq / g_zp may arrive as column slices of a wider gradient: read in place (row stride)
        strided, keep = [], []
        for g in (g_zq, g_zp):
            if g is None:
                strided += [None, 0]
                continue
            if (Z > 1 and g.stride(1) != 1) or (B > 1 and g.stride(0) < Z):
                g = g.contiguous()
            keep.append(g)
            strided += [L.dev(g, "g_z", check_contiguous=False), int(g.stride(0)) if B > 1 else Z]
        gs = [None if g is None else g.contiguous() for g in (g_kl, g_logq, g_logp)]
        g_q = [None, None] if q_loc is None else [torch.empty_like(q_loc), torch.empty_like(q_loc)]
        g_p = [torch.empty_like(p_loc), torch.empty_like(p_loc)]
        L.call("rfn_gauss_heads_bwd_f32", *[L.dev(t) for t in ins], *strided, *[L.dev(g) for g in gs],
               *[L.dev(g) for g in g_q + g_p], B, Z, meta=shell("gauss_heads_bwd", p_loc, 10))
        return g_q[0], g_q[1], g_p[0], g_p[1], None, None, None


def gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=None, eps_p=None, want=("z_q", "kl")):
    """The outputs named in `want`, in that order, of the [B, Z] Gaussians N(q_loc, softplus(q_raw)) and N(p_loc,
    softplus(p_raw)): "z_q" / "z_p" = loc + sigma * eps, "q_scale" / "p_scale" = sigma (no gradient is taken through
    them), "kl" [B] = KL(q || p) summed over the row, "logq" / "logp" [B] = the row-summed log-density of each
    distribution at its own sample.  q_loc = q_raw = eps_q = None is the prior-only form.  One launch each way on the
    current stream; no CPU fallback."""
    gauss_heads_check(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want)
    outs = GaussHeadsFn.apply(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, tuple(want))
    return tuple(outs[GAUSS_HEADS_OUTPUTS.index(w)] for w in want)
