"""Mixture of discretized logistics (likelihood, sampling, addressed uniforms): wrappers of csrc/mol.hip.  rfn_hip.ops
re-exports the public names."""
import torch

from . import lib as L
from .args import check_step, check_u63, fresh_device, shell


def mol_dims(x, l):
    """(N, C, M, HW) of a mixture-of-discretized-logistics call, or a RuntimeError naming what does not fit.  x [N,C,H,W]
    with C in {1, 3}; l [N,Cl,H,W] with Cl = 10 M (C = 3) or 3 M (C = 1).  Needs no device."""
    if x.dim() != 4 or l.dim() != 4:
        raise RuntimeError("mol: x and l must be [N,C,H,W], got %s and %s" % (tuple(x.shape), tuple(l.shape)))
    N, C, H, W = (int(d) for d in x.shape)
    if C not in (1, 3):
        raise RuntimeError("mol: x must have 1 or 3 channels, got %d" % C)
    per = 10 if C == 3 else 3
    Cl = int(l.shape[1])
    if (int(l.shape[0]), int(l.shape[2]), int(l.shape[3])) != (N, H, W) or Cl < per or Cl % per:
        raise RuntimeError("mol: logits %s do not fit x %s: need [%d, %d*M, %d, %d] with M >= 1" %
                           (tuple(l.shape), tuple(x.shape), N, per, H, W))
    return N, C, Cl // per, H * W


class MolNllFn(torch.autograd.Function):
    """nll_pix [N,H,W] (reduce = 0) or its per-frame sum nll [N] (reduce = 1) of x under the mixture of discretized
    logistics with parameters l (rfn_mol_nll_fwd / rfn_mol_nll_bwd).  Gradient into l only."""

    @staticmethod
    def forward(ctx, x, l, per_frame):
        N, C, M, HW = mol_dims(x, l)
        x, l = x.detach().contiguous(), l.contiguous()
        L.dev(x, "x"), L.dev(l, "l")  # (device fp32 tensors, before anything is allocated or loaded)
        nll_pix =torch.empty((N, x.shape[2], x.shape[3]), device=l.device, dtype=torch.float32)
        lse = torch.empty_like(nll_pix)
        nll = torch.empty((N,), device=l.device, dtype=torch.float32)
        part = torch.empty((int(L.load().rfn_mol_part_floats(N, HW)),), device=l.device, dtype=torch.float32)
        L.call("rfn_mol_nll_fwd", L.dev(x, "x"), L.dev(l, "l"), L.dev(nll_pix), L.dev(lse), L.dev(nll), L.dev(part), N, C,
               M, HW, meta=shell("mol_nll_fwd", l, 1))
        ctx.save_for_backward(x, l, lse)
        ctx.cfg = (N, C, M, HW, per_frame)
        return nll if per_frame else nll_pix

    @staticmethod
    def backward(ctx, g):
        x, l, lse = ctx.saved_tensors
        N, C, M, HW, per_frame = ctx.cfg
        g = g.contiguous()
        dl = torch.empty_like(l)
        L.call("rfn_mol_nll_bwd", L.dev(x), L.dev(l), L.dev(lse), L.dev(g, "grad"), 0 if per_frame else 1, L.dev(dl),
               N, C, M, HW, meta=shell("mol_nll_bwd", l, 2))
        return None, dl, None


def mol_nll(x, l, reduce="frame"):
    """Negative log-likelihood of x [N,C,H,W] in [-1,1] under the mixture of discretized logistics l [N,Cl,H,W]:
    reduce="pixel" -> [N,H,W], reduce="frame" -> [N], each frame's pixels summed in a fixed order (the bits of a frame do
    not depend on the other frames of the call).  Differentiable in l; x must not require a gradient."""
    if reduce not in ("frame", "pixel"):
        raise ValueError("mol_nll: reduce must be 'frame' or 'pixel', got %r" % (reduce,))
    if x.requires_grad:
        raise RuntimeError("mol_nll: no gradient flows into x; pass x.detach()")
    return MolNllFn.apply(x, l, reduce == "frame")


def _mol_channels(who, Cl, channels):
    """(C, M) of Cl logit channels: C is `channels`, else what Cl allows (10 M: RGB, 3 M: gray)"""
    C = channels
    if C is None:
        fits = [c for c, per in ((3, 10), (1, 3)) if Cl >= per and Cl % per == 0]
        if len(fits) != 1:
            raise RuntimeError("%s: %d logit channels %s; pass channels=1 or 3" %
                               (who, Cl, "fit both RGB and gray" if fits else "fit neither 10*M nor 3*M"))
        C = fits[0]
    per = 10 if C == 3 else 3
    if C not in (1, 3) or Cl < per or Cl % per:
        raise RuntimeError("%s: %d logit channels do not fit %d colour channels (need %d*M)" % (who, Cl, C, per))
    return C, Cl // per


def mol_sample(l, u_mix=None, u_x=None, generator=None, channels=None):
    """Draw x [N,C,H,W] from the mixture l [N,Cl,H,W] (rfn_mol_sample); no gradient.  u_mix [N,H,W,M] and u_x [N,H,W,C]
    are the reference's two uniform draws, in (1e-5, 1 - 1e-5); drawn here, in that order, from `generator` when not
    given.  C is `channels`, else the last extent of u_x, else what Cl allows (10 M: RGB, 3 M: gray); a Cl that allows
    both (30, 60, ...) needs one of the two."""
    if l.dim() != 4:
        raise RuntimeError("mol_sample: l must be [N,Cl,H,W], got %s" % (tuple(l.shape),))
    N, Cl, H, W = (int(d) for d in l.shape)
    if channels is None and u_x is not None:
        channels = int(u_x.shape[-1])
    C, M = _mol_channels("mol_sample", Cl, channels)
    l = l.detach().contiguous()
    L.dev(l, "l")
    if u_mix is None:
        u_mix = torch.empty((N, H, W, M), device=l.device, dtype=torch.float32).uniform_(1e-5, 1. - 1e-5, generator=generator)
    if u_x is None:
        u_x = torch.empty((N, H, W, C), device=l.device, dtype=torch.float32).uniform_(1e-5, 1. - 1e-5, generator=generator)
    if tuple(u_mix.shape) != (N, H, W, M) or tuple(u_x.shape) != (N, H, W, C):
        raise RuntimeError("mol_sample: uniforms must be [N,H,W,M] = %s and [N,H,W,C] = %s, got %s and %s" %
                           ((N, H, W, M), (N, H, W, C), tuple(u_mix.shape), tuple(u_x.shape)))
    u_mix, u_x = u_mix.contiguous(), u_x.contiguous()
    out = torch.empty((N, C, H, W), device=l.device, dtype=torch.float32)
    L.call("rfn_mol_sample", L.dev(l), L.dev(u_mix, "u_mix"), L.dev(u_x, "u_x"), L.dev(out), N, C, M,
           H * W, meta=shell("mol_sample", l, 1))
    return out


MOL_KEYED_SLOT_MIX, MOL_KEYED_SLOT_COLOUR = 16, 17   # the key's slot word (keyed_normal owns 0 .. 7)


def _mol_keyed_address(who, rows, B, seed, step, first_seq, first_draw):
    B, seed, step, first_seq, first_draw = (int(v) for v in (B, seed, step, first_seq, first_draw))
    if B < 1 or rows < 1 or rows % B:
        raise ValueError("%s: %d rows are no positive multiple of B = %d (row r*B + b is draw first_draw + r of sequence "
                         "first_seq + b)" % (who, rows, B))
    check_u63(who, seed=seed, first_seq=first_seq, first_draw=first_draw)
    check_step(who, step)
    return B, seed, step, first_seq, first_draw


def mol_sample_keyed(l, B, seed, step, first_seq=0, first_draw=0, channels=None):
    """mol_sample with addressed uniforms (rfn_mol_sample_keyed; include/rfn_hip.h and DESIGN section 20 hold the
    definition): x [rows,C,H,W] from the mixture l [rows,Cl,H,W], rows a multiple of B.  Row r*B + b is draw first_draw +
    r of sequence first_seq + b, and a pixel's uniforms depend only on (seed, step, sequence, draw, pixel, element): the
    same for any B, number of draws and split of the draws into calls.  No uniform tensor exists and torch's generator
    is not touched; mol_keyed_uniforms writes the numbers out.  One launch on the current stream; no CPU fallback."""
    if l.dim() != 4:
        raise RuntimeError("mol_sample_keyed: l must be [rows,Cl,H,W], got %s" % (tuple(l.shape),))
    rows, Cl, H, W = (int(d) for d in l.shape)
    C, M = _mol_channels("mol_sample_keyed", Cl, channels)
    B, seed, step, first_seq, first_draw = _mol_keyed_address("mol_sample_keyed", rows, B, seed, step, first_seq,
                                                              first_draw)
    l = l.detach().contiguous()
    L.dev(l, "l")
    out = torch.empty((rows, C, H, W), device=l.device, dtype=torch.float32)
    with torch.cuda.device(l.device):
        L.call("rfn_mol_sample_keyed", L.dev(l), L.dev(out), rows, B, C, M, H * W, seed, step, first_seq, first_draw,
               meta=shell("mol_sample_keyed", l, 1))
    return out


def mol_keyed_uniforms(shape_or_l, B, M, channels, seed, step, first_seq=0, first_draw=0, device=None):
    """(u_mix [rows,H,W,M], u_x [rows,H,W,C]): the uniforms mol_sample_keyed uses at that address
    (rfn_mol_keyed_uniforms), so that mol_sample(l, u_mix, u_x) replays it bit for bit.  shape_or_l: the logits (their
    rows, H, W and device are taken) or (rows, H, W); device: where the tensors go for a shape (default: the current
    GPU)."""
    if isinstance(shape_or_l, torch.Tensor):
        if shape_or_l.dim() != 4:
            raise RuntimeError("mol_keyed_uniforms: l must be [rows,Cl,H,W], got %s" % (tuple(shape_or_l.shape),))
        rows, _, H, W = (int(d) for d in shape_or_l.shape)
        device = shape_or_l.device
    else:
        if len(shape_or_l) != 3:
            raise ValueError("mol_keyed_uniforms: give the logits or (rows, H, W), got %s" % (tuple(shape_or_l),))
        rows, H, W = (int(d) for d in shape_or_l)
    M, C = int(M), int(channels)
    if M < 1 or C not in (1, 3) or H < 1 or W < 1:
        raise ValueError("mol_keyed_uniforms: need M >= 1, channels 1 or 3 and a non-empty frame (got M = %d, channels = "
                         "%d, %dx%d)" % (M, C, H, W))
    B, seed, step, first_seq, first_draw = _mol_keyed_address("mol_keyed_uniforms", rows, B, seed, step, first_seq,
                                                              first_draw)
    device = fresh_device("mol_keyed_uniforms", device)
    u_mix = torch.empty((rows, H, W, M), device=device, dtype=torch.float32)
    u_x = torch.empty((rows, H, W, C), device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        L.call("rfn_mol_keyed_uniforms", L.dev(u_mix), L.dev(u_x), rows, B, C, M, H * W, seed, step, first_seq,
               first_draw, meta=("shell", "mol_keyed_uniforms", 0.0, "%dx%dx%d" % (rows, H * W, M + C),
                                 4.0 * (u_mix.numel() + u_x.numel())))
    return u_mix, u_x
