"""BatchNorm with per-timestep statistics (plain, synchronised, pooled) and the one-launch upsample + cat: wrappers of
csrc/stepbn.hip and csrc/up2x_cat.hip.  rfn_hip.ops re-exports the public names."""
import torch

from . import lib as L
from .args import shell


def _stepbn_fwd_buffers(x, gamma, beta, S, pooled=False):
    """What a per-step BatchNorm forward (plain, synchronised or pooled) allocates for x [S*B, C, H, W]: (B, mean [S, C],
    var [S, C], the output, the detached gamma and beta, the floats of scratch either direction needs, the scratch)."""
    SB, C, H, W = (int(v) for v in x.shape)
    B = SB // S
    mean = torch.empty((S, C), device=x.device, dtype=torch.float32)
    var = torch.empty((S, C), device=x.device, dtype=torch.float32)
    out = torch.empty((SB, C, H // 2, W // 2), device=x.device, dtype=torch.float32) if pooled else torch.empty_like(x)
    gm = None if gamma is None else gamma.detach().contiguous()
    bt = None if beta is None else beta.detach().contiguous()
    nscr = int(L.load().rfn_stepbn_scratch_floats(S, B, C))  # partial sums of the split reductions (either way)
    acc = torch.empty((nscr,), device=x.device, dtype=torch.float32)
    return B, mean, var, out, gm, bt, nscr, acc


def _stepbn_running_args(running):
    """the running-statistics arguments of rfn_stepbn_fwd_f32 / rfn_stepbn_pool_fwd_f32 from `running` (or None)"""
    if running is None:
        return None, None, None, None, 1.0, None
    rm, rv, cf, cfu, decay, nbt = running
    if nbt is not None and (nbt.dtype != torch.int64 or not nbt.is_cuda):
        raise RuntimeError("num_batches_tracked must be an int64 device tensor")
    return L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cfu), decay, None if nbt is None else nbt.data_ptr()


def _stepbn_bwd_buffers(x, C, affine, nscr):
    """what a per-step BatchNorm backward allocates: (sums, gx, ggamma, gbeta); the last two None without affine"""
    sums = torch.empty((nscr,), device=x.device, dtype=torch.float32)
    gx = torch.empty_like(x)
    ggamma = torch.empty((C,), device=x.device, dtype=torch.float32) if affine else None
    gbeta = torch.empty((C,), device=x.device, dtype=torch.float32) if affine else None
    return sums, gx, ggamma, gbeta


class StepBatchNormActFn(torch.autograd.Function):
    """Training-mode BatchNorm2d with per-timestep statistics on a step-major time-batched tensor [S*B, C, H, W],
    fused with the activation that follows it (rfn_stepbn_{fwd,bwd}_f32: two launches each way).  Returns (y, mean[S, C],
    biased var[S, C]).  act: 0 none, 1 relu, 2 leaky_relu(slope), 3 tanh.  running (optional) = (running_mean, running_var,
    coef[S], coef_u[S], decay, num_batches_tracked or None): the S exponential-average updates of the step-wise calls,
    applied by the same launch (r <- decay r + sum_s coef[s] stat[s]); without it the caller does them."""

    @staticmethod
    def forward(ctx, x, gamma, beta, S, eps, act, slope, running=None):
        ctx.set_materialize_grads(False)  # mean / var are not differentiable: no zero gradients built for them
        x = x.contiguous()
        from . import dist as rdist
        if rdist.sync_batchnorm_on():
            return StepBatchNormActFn._forward_sync(ctx, x, gamma, beta, S, eps, act, slope, running)
        ctx.world = 1
        C, HW = int(x.shape[1]), int(x.shape[2]) * int(x.shape[3])
        B, mean, var, y, gm, bt, nscr, acc = _stepbn_fwd_buffers(x, gamma, beta, S)
        L.call("rfn_stepbn_fwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(y), L.dev(mean), L.dev(var), L.dev(acc),
               *_stepbn_running_args(running), S, B, C, HW, eps, act, slope, meta=shell("stepbn_fwd", x, 3))
        ctx.save_for_backward(x, mean, var, gm, bt)
        ctx.cfg = (S, B, C, HW, eps, act, slope, gamma is not None, nscr)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def _forward_sync(ctx, x, gamma, beta, S, eps, act, slope, running):
        """synchronised BatchNorm (rfn_hip.dist.sync_batchnorm_on): the statistics of every step are those of the GLOBAL
        batch -- local moments, one all-gather of [2, S, C] floats, equal-count combination, apply with the given
        statistics; the running statistics follow the global moments (torch ops on [C] vectors)."""
        import torch.distributed as dist
        from . import dist as rdist
        C, HW = int(x.shape[1]), int(x.shape[2]) * int(x.shape[3])
        world = dist.get_world_size()
        B, mean, var, y, gm, bt, nscr, acc = _stepbn_fwd_buffers(x, gamma, beta, S)
        L.call("rfn_stepbn_fwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(y), L.dev(mean), L.dev(var), L.dev(acc),
               *_stepbn_running_args(None), S, B, C, HW, eps, act, slope)
        st = rdist.all_gather_cat(torch.stack((mean, var)).unsqueeze(0))          # [world, 2, S, C]
        mean = st[:, 0].mean(0).contiguous()
        var = (st[:, 1].mean(0) + (st[:, 0] - mean).pow(2).mean(0)).contiguous()  # equal counts per rank
        L.call("rfn_stepbn_apply_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(y), L.dev(mean), L.dev(var), S, B,
               C, HW, eps, act, slope)
        if running is not None:
            rm, rv, cf, cfu, decay, nbt = running
            n = B * HW * world
            cfu_g = cf * (n / max(n - 1, 1))          # unbiased variance of the global batch
            rm.mul_(decay).add_((cf.view(-1, 1) * mean).sum(0))
            rv.mul_(decay).add_((cfu_g.view(-1, 1) * var).sum(0))
            if nbt is not None:
                nbt.add_(S)
        ctx.save_for_backward(x, mean, var, gm, bt)
        ctx.cfg = (S, B, C, HW, eps, act, slope, gamma is not None, nscr)
        ctx.world = world
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, g, _gm, _gv):
        x, mean, var, gm, bt = ctx.saved_tensors
        S, B, C, HW, eps, act, slope, affine, nscr = ctx.cfg
        if g is None:
            return (None,) * 8
        g = g.contiguous()
        sums, gx, ggamma, gbeta = _stepbn_bwd_buffers(x, C, affine, nscr)
        args = (L.dev(x), L.dev(gm), L.dev(bt), L.dev(g), L.dev(mean), L.dev(var), L.dev(sums), L.dev(gx), L.dev(ggamma),
                L.dev(gbeta), S, B, C, HW, eps, act, slope)
        if ctx.world > 1:   # synchronised: partial sums, added over the ranks, apply
            from . import dist as rdist
            L.call("rfn_stepbn_bwd_f32", *args, 1, ctx.world)
            rdist.all_reduce_sum_(sums)
            L.call("rfn_stepbn_bwd_f32", *args, 2, ctx.world)
        else:
            L.call("rfn_stepbn_bwd_f32", *args, 0, 1)
        return gx, ggamma, gbeta, None, None, None, None, None


class StepBatchNormActPoolFn(torch.autograd.Function):
    """StepBatchNormActFn followed by MaxPool2d(2, 2) (rfn_stepbn_pool_{fwd,bwd}_f32: two launches each way).  Only the
    pooled map is written; the backward recomputes every window's winner from x, so no full-resolution activation, index
    map or full-resolution gradient exists.  Returns (p [S*B, C, H/2, W/2], mean[S, C], biased var[S, C]); arguments as
    StepBatchNormActFn.  H and W even; not for synchronised BatchNorm (the caller keeps the unfused route there)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, S, eps, act, slope, running=None):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        C, H, W = (int(v) for v in x.shape[1:])
        B, mean, var, p, gm, bt, nscr, acc = _stepbn_fwd_buffers(x, gamma, beta, S, pooled=True)
        # x read by the statistics and by the apply launch, a quarter of it written
        L.call("rfn_stepbn_pool_fwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(p), L.dev(mean), L.dev(var), L.dev(acc),
               *_stepbn_running_args(running), S, B, C, H, W, eps, act, slope, meta=shell("stepbn_pool_fwd", x, 2.25))
        ctx.save_for_backward(x, mean, var, gm, bt)
        ctx.cfg = (S, B, C, H, W, eps, act, slope, gamma is not None, nscr)
        ctx.mark_non_differentiable(mean, var)
        return p, mean, var

    @staticmethod
    def backward(ctx, gp, _gm, _gv):
        x, mean, var, gm, bt = ctx.saved_tensors
        S, B, C, H, W, eps, act, slope, affine, nscr = ctx.cfg
        if gp is None:
            return (None,) * 8
        gp = gp.contiguous()
        sums, gx, ggamma, gbeta = _stepbn_bwd_buffers(x, C, affine, nscr)
        # x and the pooled gradient read by the reduce and by the apply launch, gx written
        L.call("rfn_stepbn_pool_bwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(gp), L.dev(mean), L.dev(var), L.dev(sums),
               L.dev(gx), L.dev(ggamma), L.dev(gbeta), S, B, C, H, W, eps, act, slope, 0, 1,
               meta=shell("stepbn_pool_bwd", x, 3.5))
        return gx, ggamma, gbeta, None, None, None, None, None


class Up2xCatFn(torch.autograd.Function):
    """torch.cat((nearest_up2x(x), skip), 1) in one launch (rfn_up2x_cat_f32); backward: gx = the 2x2 block sums of
    g[:, :Cx] read in place (rfn_up2x_cat_bwd_f32), the skip's gradient is the view g[:, Cx:]."""

    @staticmethod
    def forward(ctx, x, skip):
        N, Cx, h, w = (int(v) for v in x.shape)
        Cs = int(skip.shape[1])
        if tuple(skip.shape) != (N, Cs, 2 * h, 2 * w):
            raise RuntimeError("Up2xCatFn: skip %s does not fit x %s" % (tuple(skip.shape), tuple(x.shape)))
        dense = lambda t: all(t.shape[d] == 1 or t.stride(d) == e for d, e in
                              ((3, 1), (2, t.shape[3]), (1, t.shape[2] * t.shape[3])))
        x, skip = (t if dense(t) else t.contiguous() for t in (x, skip))   # channel-slice views are read in place
        xp, xns = L.frames(x, "x")
        sp, sns = L.frames(skip, "skip")
        out = torch.empty((N, Cx + Cs, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
        L.call("rfn_up2x_cat_f32", xp, xns, sp, sns, L.dev(out), N, Cx, Cs, h, w,
               meta=shell("up2x_cat", out, 1.0 + (0.25 * Cx + Cs) / (Cx + Cs)))
        ctx.cfg = (N, Cx, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        N, Cx, h, w = ctx.cfg
        g = g.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gp, gns = L.frames(g, "g")
            gx = torch.empty((N, Cx, h, w), device=g.device, dtype=torch.float32)
            L.call("rfn_up2x_cat_bwd_f32", gp, gns, L.dev(gx), N, Cx, h, w, meta=shell("up2x_cat_bwd", gx, 5))
        return gx, (g[:, Cx:] if ctx.needs_input_grad[1] else None)
