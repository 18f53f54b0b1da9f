"""Adam for the training step (RFN/trainer.py:96 of the reference: torch.optim.Adam(model.parameters(), lr)) on the
one-launch HIP kernel rfn_adam_step_f32.  A subclass of torch.optim.Adam: constructor, param_groups, state layout
({"step", "exp_avg", "exp_avg_sq"} per parameter) and state_dict()/load_state_dict() are torch's, so checkpoints written
by either load into the other (the reference's rfn.pt holds `optimizer_state_dict`); only step() differs.

The kernel reads a device table of (p, g, m, v, numel, step offset) per tensor.  The table is rebuilt whenever a pointer
changed: never in hipGraph mode (the gradient tensors are the graph's static outputs), every step in eager mode (autograd
allocates fresh gradients), where the rebuild is one small host-to-device copy next to ~7000 eager launches.

The guard (`max_grad_norm` > 0 and / or `skip_nonfinite`; both off by default, and then step() is exactly the plain launch)
decides on the device: rfn_grad_sumsq_f32 -> rfn_grad_guard_f32 -> rfn_adam_step_guarded_f32 over the same table, clipping
to the global gradient norm (torch's clip_grad_norm_ formula) and leaving p, m, v untouched when the norm is not finite.
The host never learns of a skip on the step path: the kernels count skipped steps in a device counter and take it out of
the bias corrections; the host's step counts are settled against that counter where a read is allowed anyway (table
rebuild, state_dict(), guard_stats()).  Under data parallelism the squares of the rank-local gradients (`rank_local`, the
batch-sharded initial states; GradBucketReducer.finish() has divided them by the world size) are summed over ranks with
one scalar all-reduce, which gives every rank the norm of one process on the global batch, bit for bit, and hence the
same decision.

`ema_decay` d in (0, 1) keeps a Polyak average of every parameter in state[p]["ema"], updated inside the same launch
(rfn_adam_ema_step_f32 / rfn_adam_ema_step_guarded_f32): after a tensor's n-th APPLIED step, ema += w (p_new - ema) with
w = 1 - min(d, (1 + n) / (10 + n)).  The average starts as a copy of the parameter when its state is first built, a step
the guard skips leaves it alone, and swap_ema() exchanges parameters and averages in one launch.  With the default 0
nothing of this exists: the launches and the state are those of an optimizer without the keyword."""
import ctypes

import numpy as np
import torch

from . import lib as L


class HipAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0,
                 skip_nonfinite=False, rank_local=(), group=None, ema_decay=0.0):
        self.ema_decay = float(ema_decay)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError("HipAdam: ema_decay must be in [0, 1) (0 = no average), got %r" % (ema_decay,))
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False,
                         fused=False)
        self.max_grad_norm = float(max_grad_norm)
        if not self.max_grad_norm >= 0.0:
            raise ValueError("HipAdam: max_grad_norm must be >= 0 (0 = no clipping), got %r" % (max_grad_norm,))
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm > 0.0 or self.skip_nonfinite
        self._rank_local = {id(p) for p in rank_local}
        self._group = group
        self._gbuf = None     # guard on: 8 device floats = stats[0:3] | pad | sumsq[4:6] | skipped counter (int64) at [6:8]
        self._guard = None    # (partials, stats, sumsq, skipped, all-reduce sumsq[1]?) for the current table
        self._settled = 0     # skipped steps already taken out of _steps
        self._key = None
        self._ema = None      # ema on: (device array of the averages' pointers, the averages) for the current table
        self._swap = None     # swap_ema(): (key, table, chunks, n_chunks, pointers, parameters) over ALL averaged tensors
        self._keep = None
        self._t = 0           # kernel step counter; a tensor's own count is _t - its step_offset
        self._steps = {}      # id(p) -> step count as of the last step() (host ints; state["step"] is synced lazily)
        self._dirty = False

    # ---- torch-visible state -------------------------------------------------------------------------------------
    def _settle_skipped(self, gbuf_host=None):
        """take the steps the device skipped since the last look out of the host's counts (one device->host read).  The
        tensors of the current table are the ones that took part in every call since it was built."""
        if self._gbuf is None:
            return
        if gbuf_host is None:
            gbuf_host = self._gbuf.cpu()
        total = int(gbuf_host[6:8].view(torch.int64))
        delta = total - self._settled
        if delta and self._keep is not None:
            for p in self._keep[3]:
                if id(p) in self._steps:
                    self._steps[id(p)] -= delta
            self._dirty = True
        self._settled = total

    def guard_stats(self):
        """{"grad_norm", "scale", "skipped_steps"} of the last guarded step / of all steps since construction or
        load_state_dict: one device->host read, for the end of an epoch and for tests.  Also brings state["step"] up to
        date."""
        if self._gbuf is None:
            return {"grad_norm": 0.0, "scale": 1.0, "skipped_steps": 0}
        h = self._gbuf.cpu()
        self._settle_skipped(h)
        self._sync_step_tensors(settle=False)
        return {"grad_norm": float(h[0]), "scale": float(h[1]), "skipped_steps": self._settled}

    def _sync_step_tensors(self, settle=True):
        if settle:
            self._settle_skipped()
        if self._dirty:
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st is not None and id(p) in self._steps:
                        st["step"] = torch.tensor(float(self._steps[id(p)]))
            self._dirty = False

    def state_dict(self):
        self._sync_step_tensors()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if not self.ema_decay > 0.0:
            for st in self.state.values():   # nobody would update it: a stale average is worse than none
                st.pop("ema", None)
        self._key, self._steps, self._dirty = None, {}, False
        self._keep = self._gbuf = self._guard = None   # the skipped-step counter restarts with the loaded counts
        self._ema = self._swap = None                  # (a state without "ema" starts its average in _build)
        self._settled = 0

    # ---- the average ---------------------------------------------------------------------------------------------
    @staticmethod
    def _ema_of(p, st):
        """state[p]["ema"], created as a copy of the parameter where the state has none (first step, or a state loaded
        from a run without the average)"""
        if "ema" not in st:
            st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
        a = st["ema"]
        if a.dtype != torch.float32 or not a.is_cuda or not a.is_contiguous() or a.numel() != p.numel():
            raise RuntimeError("HipAdam: ema must be a dense fp32 device tensor of its parameter's %d elements (got %s %s, "
                               "%d elements, contiguous=%s)" % (p.numel(), a.dtype, a.device, a.numel(), a.is_contiguous()))
        return a

    @staticmethod
    def _ptr_array(tensors, dev):
        """device array of the tensors' addresses (float* const* of the entry points)"""
        host = (ctypes.c_void_p * max(1, len(tensors)))(*[t.data_ptr() for t in tensors])
        return torch.frombuffer(host, dtype=torch.uint8).to(dev)

    @torch.no_grad()
    def swap_ema(self):
        """exchange every averaged parameter with its average: one rfn_param_swap_f32 launch over all tensors whose state
        holds "ema" (whether or not the last step saw their gradient).  Calling it twice restores both, bit for bit.
        The parameters' version counters move, so reverse caches and generation graphs keyed on them rebuild."""
        if not self.ema_decay > 0.0:
            raise RuntimeError("HipAdam.swap_ema: this optimizer keeps no average (ema_decay = 0)")
        params = [p for group in self.param_groups for p in group["params"] if "ema" in self.state.get(p, ())]
        if not params:
            return
        emas = [self._ema_of(p, self.state[p]) for p in params]
        key = tuple((p.data_ptr(), a.data_ptr()) for p, a in zip(params, emas))
        if self._swap is None or self._swap[0] != key:
            for p in params:
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                    raise RuntimeError("HipAdam.swap_ema: parameters must be dense fp32 device tensors")
            dev = params[0].device
            chunk = int(L.load().rfn_adam_chunk_elems())
            ent = (L.rfn_adam_entry * len(params))()
            chunks = []
            for i, p in enumerate(params):
                ent[i] = L.rfn_adam_entry(p.data_ptr(), None, None, None, p.numel(), 0, 0)   # the kernel reads p and n
                nck = (p.numel() + chunk - 1) // chunk
                chunks.append(np.stack([np.full(nck, i, dtype=np.int32), np.arange(nck, dtype=np.int32)], 1))
            chunks = np.concatenate(chunks, 0)
            self._swap = (key, torch.frombuffer(ent, dtype=torch.uint8).to(dev),
                          torch.from_numpy(np.ascontiguousarray(chunks).reshape(-1)).to(dev), int(chunks.shape[0]),
                          self._ptr_array(emas, dev), params)
        _, tab_d, chk_d, nck, ptr_d, plist = self._swap
        L.call("rfn_param_swap_f32", tab_d.data_ptr(), chk_d.data_ptr(), nck, ptr_d.data_ptr(),
               meta=("shell", "param_swap", 0.0, "%d tensors" % len(plist), 16.0 * sum(p.numel() for p in plist)))
        torch.autograd.graph.increment_version(plist)

    # ---- the step ------------------------------------------------------------------------------------------------
    def _build(self, group, params, key):
        dev = params[0].device
        chunk = int(L.load().rfn_adam_chunk_elems())
        if self.guarded:
            if self._gbuf is None:
                self._gbuf = torch.zeros(8, dtype=torch.float32, device=dev)
            self._settle_skipped()   # (the previous table's tensors; a read is allowed here)
        ent = (L.rfn_adam_entry * len(params))()
        chunks = []
        emas = []
        for i, p in enumerate(params):
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if id(p) not in self._steps:
                self._steps[id(p)] = int(float(st["step"]))
            m, v, g = st["exp_avg"], st["exp_avg_sq"], p.grad
            for name, t in (("parameter", p), ("gradient", g), ("exp_avg", m), ("exp_avg_sq", v)):
                if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                    raise RuntimeError("HipAdam: %s must be a dense fp32 device tensor (got %s %s, contiguous=%s)" %
                                       (name, t.dtype, t.device, t.is_contiguous()))
            n = p.numel()
            for name, t in (("gradient", g), ("exp_avg", m), ("exp_avg_sq", v)):
                if t.numel() != n:   # e.g. moments of another batch size loaded from a checkpoint: the kernel indexes by n
                    raise RuntimeError("HipAdam: %s has %d elements, its parameter %d (shape %s)" %
                                       (name, t.numel(), n, tuple(p.shape)))
            if self.ema_decay > 0.0:
                emas.append(self._ema_of(p, st))
            # the guarded kernel subtracts the device's running count of skipped steps as well
            off = self._t - self._steps[id(p)] - self._settled
            flags = 1 if id(p) in self._rank_local else 0
            ent[i] = L.rfn_adam_entry(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, off, flags)
            nck = (n + chunk - 1) // chunk
            chunks.append(np.stack([np.full(nck, i, dtype=np.int32), np.arange(nck, dtype=np.int32)], 1))
        chunks = np.concatenate(chunks, 0) if chunks else np.zeros((0, 2), np.int32)
        tab_d = torch.frombuffer(ent, dtype=torch.uint8).to(dev)
        chk_d = torch.from_numpy(np.ascontiguousarray(chunks).reshape(-1)).to(dev)
        self._keep = (tab_d, chk_d, int(chunks.shape[0]), list(params), 28.0 * sum(p.numel() for p in params))
        self._key = key
        if self.ema_decay > 0.0:
            self._ema = (self._ptr_array(emas, dev), emas)
        if self.guarded:
            import torch.distributed as dist
            from . import dist as rdist
            partials = torch.empty(max(1, int(chunks.shape[0])), dtype=torch.float32, device=dev)
            reduce_local = bool(self._rank_local) and rdist.is_dist() and dist.get_world_size(self._group) > 1
            self._guard = (partials, self._gbuf[0:3], self._gbuf[4:6], self._gbuf[6:8], reduce_local)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise NotImplementedError("HipAdam: one parameter group (what the reference's trainer builds)")
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError("HipAdam: amsgrad / maximize are not implemented")
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return loss
        for p in params:
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
        key = tuple((p.data_ptr(), p.grad.data_ptr()) for p in params)
        if key != self._key or any(id(p) not in self._steps for p in params):
            # a parameter that skipped steps keeps its own count through its step_offset
            self._build(group, params, key)
        tab_d, chk_d, nck, plist, nbytes = self._keep
        # every listed tensor advances by one; the kernel computes bias corrections from t - step_offset
        self._t += 1
        for p in plist:
            self._steps[id(p)] += 1
        self._dirty = True
        beta1, beta2 = group["betas"]
        if self.guarded:
            self._guarded_launches(group, beta1, beta2)
            torch.autograd.graph.increment_version(plist)
            return loss
        if self.ema_decay > 0.0:
            L.call("rfn_adam_ema_step_f32", tab_d.data_ptr(), chk_d.data_ptr(), nck, float(group["lr"]), beta1, beta2,
                   group["eps"], group["weight_decay"], self._t, self.ema_decay, self._ema[0].data_ptr(),
                   meta=("shell", "adam_ema", 0.0, "%d tensors" % len(plist), nbytes * 36.0 / 28.0))
        else:
            L.call("rfn_adam_step_f32", tab_d.data_ptr(), chk_d.data_ptr(), nck, float(group["lr"]), beta1, beta2,
                   group["eps"], group["weight_decay"], self._t,
                   meta=("shell", "adam", 0.0, "%d tensors" % len(plist), nbytes))
        # the kernel wrote through raw pointers: tell autograd's version counters, which everything keyed on
        # `p._version` relies on (ListGlow._reverse_cache, RFN._gen_graph: cached inverse matrices / packs / hipGraph)
        torch.autograd.graph.increment_version(plist)
        return loss

    def _guarded_launches(self, group, beta1, beta2):
        """sumsq -> (rank-local part summed over ranks) -> guard -> guarded Adam; nothing here reads from the device"""
        from . import dist as rdist
        tab_d, chk_d, nck, plist, nbytes = self._keep
        partials, stats, sumsq, skipped, reduce_local = self._guard
        tab, chk = tab_d.data_ptr(), chk_d.data_ptr()
        L.call("rfn_grad_sumsq_f32", tab, chk, nck, partials.data_ptr(), sumsq.data_ptr(),
               meta=("shell", "grad_sumsq", 0.0, "%d tensors" % len(plist), nbytes / 7.0))
        if reduce_local:
            rdist.all_reduce_sum_(sumsq[1:2], group=self._group)
        L.call("rfn_grad_guard_f32", sumsq.data_ptr(), self.max_grad_norm, int(self.skip_nonfinite), stats.data_ptr(),
               skipped.data_ptr(), meta=("shell", "grad_guard", 0.0, "", 0.0))
        if self.ema_decay > 0.0:
            L.call("rfn_adam_ema_step_guarded_f32", tab, chk, nck, float(group["lr"]), beta1, beta2, group["eps"],
                   group["weight_decay"], self._t, stats.data_ptr(), skipped.data_ptr(), self.ema_decay,
                   self._ema[0].data_ptr(),
                   meta=("shell", "adam_ema_guarded", 0.0, "%d tensors" % len(plist), nbytes * 36.0 / 28.0))
            return
        L.call("rfn_adam_step_guarded_f32", tab, chk, nck, float(group["lr"]), beta1, beta2, group["eps"],
               group["weight_decay"], self._t, stats.data_ptr(), skipped.data_ptr(),
               meta=("shell", "adam_guarded", 0.0, "%d tensors" % len(plist), nbytes))
