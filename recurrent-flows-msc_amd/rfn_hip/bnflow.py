"""BatchNormFlow steps with per-timestep statistics: wrappers of csrc/bnflow.hip.  rfn_hip.ops re-exports the public
names."""
import torch

from . import lib as L
from .args import flat, shell


def bnflow_coef(steps, momentum):
    """(coef [steps] as float64, decay) of the closed form of `steps` running-statistics updates r <- m r + (1 - m) stat_s of
    BatchNormFlow (glow_modules.py:81-87; the momentum weights the OLD value): r <- decay r + sum_s coef[s] stat_s with
    decay = m^S, coef[s] = (1 - m) m^(S-1-s) and 0^0 = 1.  Needs no device."""
    m = float(momentum)
    coef = (1.0 - m) * torch.tensor([m ** (steps - 1 - s) for s in range(steps)], dtype=torch.float64)
    return coef, m ** steps


class BatchNormFlowFn(torch.autograd.Function):
    """BatchNormFlow in training mode, forward direction (glow_modules.py:76-98), on a step-major time-batched tensor
    x [steps*B, C, H, W] with the statistics of EACH step's B rows (rfn_bnflow_{fwd,bwd}_f32, two launches each way).
    log_gamma / beta: [1, C, H, W].  Returns (z, dl [steps]); dl[s] belongs to the log-det of every row of step s.
    running = (running_mean, running_var, coef [steps] device tensor, decay) or None: the `steps` updates of the
    step-wise calls, applied by the same launches in closed form (bnflow_coef)."""

    @staticmethod
    def forward(ctx, x, log_gamma, beta, steps, eps, running=None):
        x = x.contiguous()
        S, B = int(steps), int(x.shape[0]) // int(steps)
        E = x[0].numel()
        if S * B != x.shape[0] or log_gamma.numel() != E or beta.numel() != E:
            raise RuntimeError("BatchNormFlowFn: x %s is not %d steps of rows of %d elements" % (tuple(x.shape), S, log_gamma.numel()))
        lg, bt = flat(log_gamma), flat(beta)
        z = torch.empty_like(x)
        mean = torch.empty((S, E), device=x.device, dtype=torch.float32)
        var = torch.empty((S, E), device=x.device, dtype=torch.float32)
        dl = torch.empty((S,), device=x.device, dtype=torch.float32)
        scr = torch.empty((int(L.load().rfn_bnflow_scratch_floats(S, B, E, 0)),), device=x.device, dtype=torch.float32)
        rm = rv = cf = None
        decay = 1.0
        if running is not None:
            rm, rv, cf, decay = running
            if not (rm.is_contiguous() and rv.is_contiguous()) or rm.numel() != E or rv.numel() != E or cf.numel() != S:
                raise RuntimeError("BatchNormFlowFn: running statistics must be dense [%d] tensors, coef [%d]" % (E, S))
        L.call("rfn_bnflow_fwd_f32", L.dev(x), L.dev(lg), L.dev(bt), L.dev(z), L.dev(mean), L.dev(var), L.dev(dl),
               L.dev(scr), L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cf), decay, S, B, E,
               eps, meta=shell("bnflow_fwd", x, 2))
        ctx.save_for_backward(x, lg, mean, var)
        ctx.cfg = (S, B, E, log_gamma.shape)
        return z, dl

    @staticmethod
    def backward(ctx, gz, gdl):
        x, lg, mean, var = ctx.saved_tensors
        S, B, E, pshape = ctx.cfg
        gz = torch.zeros_like(x) if gz is None else gz.contiguous()
        gdl = None if gdl is None else gdl.contiguous()
        gx = torch.empty_like(x)
        glg = torch.empty(pshape, device=x.device, dtype=torch.float32)
        gbt = torch.empty(pshape, device=x.device, dtype=torch.float32)
        scr = torch.empty((int(L.load().rfn_bnflow_scratch_floats(S, B, E, 1)),), device=x.device, dtype=torch.float32)
        L.call("rfn_bnflow_bwd_f32", L.dev(x), L.dev(lg), L.dev(gz), L.dev(gdl), L.dev(mean), L.dev(var), L.dev(gx),
               L.dev(glg), L.dev(gbt), L.dev(scr), S, B, E, meta=shell("bnflow_bwd", x, 3))
        return gx, glg, gbt, None, None, None


def bnflow_apply(x, log_gamma, beta, running_mean, running_var, reverse):
    """BatchNormFlow with GIVEN statistics (glow_modules.py:90-103: eval mode, and the reverse direction in any mode), no
    gradient: (y, dl [1]) by rfn_bnflow_apply_f32; dl is to be ADDED to the log-det of every row (it carries the reverse
    direction's minus sign)."""
    x = x.detach().contiguous()
    N, E = int(x.shape[0]), x[0].numel()
    y = torch.empty_like(x)
    dl = torch.empty((1,), device=x.device, dtype=torch.float32)
    lg, bt, rm, rv = flat(log_gamma), flat(beta), flat(running_mean), flat(running_var)
    if not (lg.numel() == bt.numel() == rm.numel() == rv.numel() == E):
        raise RuntimeError("bnflow_apply: parameters do not match rows of %d elements" % E)
    L.call("rfn_bnflow_apply_f32", L.dev(x), L.dev(lg), L.dev(bt), L.dev(rm), L.dev(rv), L.dev(y), L.dev(dl), N, E,
           1 if reverse else 0, meta=shell("bnflow_apply", x, 2))
    return y, dl
