"""RFN — recurrent flow network (SRNN latent dynamics + conditional Glow decoder) with the reference's surface:
`RFN(args)`, `.loss(x, logdet) -> (kl_free_bit, kl, nll)` (also exposed as `.forward`), `.predict`, `.reconstruct`,
`.sample`; same sub-module names, hence the same state_dict keys (RFN/RFN_new.py of the reference).

MI355X-first restructuring of `loss` (same mathematics, RFN/RFN_new.py:116-247):
  1. extractor over the T frames, ConvLSTM over t (HIP cell), optional backward smoothing LSTM;
  2. the latent recurrence (prior / encoder at the coarsest resolution) and the upscaler run per t — they are the only
     parts that are sequential through z_{t-1};
  3. the Glow decoder — ≈84 % of the reference's time — is evaluated ONCE on all B·(T−1) frames, t-major
     (`frame = (t-1)·B + b`), so every kernel launch carries the whole sequence batch.
Data dependent ActNorm initialisation uses the first B frames (t = 1) exactly like the reference's first call.
"""
import math
import os

import torch
import torch.nn as nn

from Flow import ListGlow
from Flow.glow_modules import ActNorm
from rfn_hip import ops as K
from rfn_hip import ops   # the same module, for the methods whose argument K is the number of chains
from rfn_hip import debug as DBG
from Utils import VGG_upscaler, VGG_downscaler, SimpleParamNet, ConvLSTM, free_bits_kl, batch_reduce
from Utils.modules import recurrent_pair, recurrent_pair_split


def kl_normal(q_mean, q_std, p_mean, p_std):
    """KL(N(q) || N(p)) element-wise — the closed form torch.distributions.kl_divergence evaluates for two Normals
    (RFN_new.py:206-207,236), written out so that no distribution object validates its arguments with a host sync
    (which would also make the step impossible to capture into a hipGraph)."""
    var_ratio = (q_std / p_std) ** 2
    t1 = ((q_mean - p_mean) / p_std) ** 2
    return 0.5 * (var_ratio + t1 - 1 - var_ratio.log())


def iw_bound(log_w):
    """bound[b] = logsumexp_k log_w[k, b] - log K of a table [K, B] of log importance weights, in
    the table's dtype and on its device; the largest entry of a column is taken out before the exponentials"""
    if log_w.dim() != 2 or log_w.shape[0] < 1:
        raise ValueError("iw_bound: log_w must be [K >= 1, B], got %s" % (tuple(log_w.shape),))
    top = log_w.max(dim=0).values
    return top + (log_w - top).exp().sum(0).log() - math.log(log_w.shape[0])


class RFN(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.params = args
        batch_size = args.batch_size
        self.u_dim = args.x_dim
        self.x_dim = args.condition_dim
        self.h_dim, self.z_dim = args.h_dim, args.z_dim
        self.beta = 1
        self.L, self.K = args.L, args.K
        self.temperature = args.temperature
        self.free_bits = args.free_bits
        self.skip_connection_flow = args.skip_connection_flow
        self.skip_connection_features = args.skip_connection_features
        self.kl_temperature = 1
        self.a_dim = args.a_dim
        self.enable_smoothing = args.enable_smoothing
        self.res_q = args.res_q
        self.D = args.D + 1
        self.overshot_w = args.overshot_w
        down_structure, up_structure = args.extractor_structure, args.upscaler_structure
        nf = args.norm_type_features

        self.single_feature = self.skip_connection_flow == "without_skip" and not self.skip_connection_features
        self.extractor = VGG_downscaler(down_structure, L=self.L, in_channels=self.x_dim[1], norm_type=nf,
                                        non_lin="relu", scale=args.structure_scaler,
                                        skip_con=not self.single_feature, tanh=args.downscaler_tanh)
        channel_dims = [i[-1] for i in up_structure][::-1]
        dims_skip = self.extractor.get_layer_size(down_structure, self.x_dim)
        hu, wu = self.u_dim[2], self.u_dim[3]
        condition_size_list = []
        for i in range(self.L):
            hu, wu = hu // 2, hu // 2
            if self.skip_connection_flow == "with_skip":
                cc = channel_dims[i] + dims_skip[i][1]
            elif self.skip_connection_flow == "without_skip":
                cc = channel_dims[i]
            elif self.skip_connection_flow == "only_skip":
                cc = dims_skip[i][1]
            else:
                raise ValueError("choose skip setting")
            condition_size_list.append([batch_size, cc, hu, wu])
        c_features = dims_skip[-1][1]

        # learnable initial states: batch-shaped, exactly as in the reference (RFN_new.py:69-76)
        self.z_0 = nn.Parameter(torch.zeros(batch_size, self.z_dim, hu, wu))
        self.z_0x = nn.Parameter(torch.zeros(batch_size, self.z_dim, hu, wu))
        self.h_0 = nn.Parameter(torch.zeros(batch_size, self.h_dim, hu, wu))
        self.c_0 = nn.Parameter(torch.zeros(batch_size, self.h_dim, hu, wu))
        self.a_0 = nn.Parameter(torch.zeros(batch_size, self.a_dim, hu, wu))
        self.ca_0 = nn.Parameter(torch.zeros(batch_size, self.a_dim, hu, wu))

        self.upscaler = VGG_upscaler(up_structure, L=self.L, in_channels=self.h_dim + self.z_dim, norm_type=nf,
                                     non_lin="leakyrelu", scale=args.structure_scaler,
                                     skips=self.skip_connection_features, size_skips=dims_skip, tanh=args.upscaler_tanh)
        self.lstm = ConvLSTM(in_channels=c_features, hidden_channels=self.h_dim, kernel_size=[3, 3], bias=True,
                             peephole=True)
        if self.enable_smoothing:
            self.a_lstm = ConvLSTM(in_channels=c_features + self.h_dim, hidden_channels=self.a_dim,
                                   kernel_size=[3, 3], bias=True, peephole=True)
        self.prior = SimpleParamNet(args.prior_structure, in_channels=self.h_dim + self.z_dim,
                                    out_channels=self.z_dim, norm_type=args.norm_type, non_lin="leakyrelu")
        base_dim = (batch_size, self.h_dim + self.z_dim, hu, wu)
        self.flow = ListGlow(self.x_dim, condition_size_list, base_dim, args=self.params)
        enc_in = (self.a_dim + self.z_dim) if self.enable_smoothing else (c_features + self.h_dim + self.z_dim)
        self.encoder = SimpleParamNet(args.encoder_structure, in_channels=enc_in, out_channels=self.z_dim,
                                      norm_type=args.norm_type, non_lin="leakyrelu")

    # ------------------------------------------------------------------------------------------------ helpers
    def get_inits(self):
        return self.h_0, self.c_0, self.a_0, self.ca_0, self.z_0, self.z_0x, 0, 0, 0

    def _last(self, feats):
        return feats if self.single_feature else feats[-1]

    def combineconditions(self, flow_conditions, skip_conditions):
        return [torch.cat((a, b), dim=1) for a, b in zip(flow_conditions, skip_conditions)]

    def _flow_conditions(self, hz, feats_prev):
        if self.skip_connection_features:
            fc = self.upscaler(hz, skip_list=feats_prev)
        else:
            fc = self.upscaler(hz)
        if self.skip_connection_flow == "with_skip":
            fc = self.combineconditions(fc, feats_prev)
        elif self.skip_connection_flow == "only_skip":
            fc = feats_prev
        return fc

    def _deterministic_states(self, feats, n_steps, hprev, cprev, aprev, caprev, x_all=None):
        """h_t for t = 1..n_steps-1 (RFN_new.py:131-139) and, with smoothing, the backward a_t (:142-153).
        x_all (optional): the deepest features of frames 0..n_steps-2 as one step-major [n_steps-1, B, ...] tensor."""
        if n_steps < 2:
            return [], [], hprev, cprev
        if x_all is None:
            x_all = torch.stack([self._last(feats[i - 1]) for i in range(1, n_steps)], 0)  # frames 0..n-2, step-major
        store_ht, hprev, cprev = self.lstm.forward_steps(x_all, hprev, cprev)
        store_at = [None] * (n_steps - 1)
        if self.enable_smoothing:  # runs backward in time over (h_t, features of frame t+1)
            inp = torch.stack([torch.cat([store_ht[n_steps - i - 1], self._last(feats[n_steps - i])], 1)
                               for i in range(1, n_steps)], 0)
            a_rev, aprev, caprev = self.a_lstm.forward_steps(inp, aprev, caprev)
            for i in range(1, n_steps):
                store_at[n_steps - i - 1] = a_rev[i - 1]
        return store_ht, store_at, hprev, cprev

    def _flow_needs_init(self):
        return any(m.needs_init() for m in self.flow.modules() if isinstance(m, ActNorm))

    # ------------------------------------------------------------------------------------------------ training
    def loss(self, x, logdet=0, draws=None):
        """RFN/RFN_new.py:116-247.  `draws` (optional) = list of noise tensors in the reference's draw order
        (per t: prior ε, encoder ε, dequantisation U; then the overshooting prior ε's) for parity runs."""
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        B, T = x.shape[0], x.shape[1]
        dev = x.device
        draws = list(draws) if draws is not None else None

        def eps_like(ref):
            return draws.pop(0).to(dev) if draws is not None else torch.randn(ref.shape, device=dev)

        hprev, cprev, aprev, caprev, zprev, zxprev, _, _, _ = self.get_inits()
        # extractor on all T frames at once (step-major), BatchNorm statistics per timestep as in the reference
        x_tm = x.transpose(0, 1).reshape(T * B, *x.shape[2:])
        feats_tb = self.extractor.forward_steps(x_tm, T)
        # the deepest features per step: a step-major view for the ConvLSTM and one unbind for the encoder inputs, so
        # that their gradients come back as one slice and one stack instead of T zero-fill + copy + add triples
        last_tb = feats_tb if self.single_feature else feats_tb[-1]
        last_steps = last_tb.view(T, B, *last_tb.shape[1:])
        last_t = last_steps.unbind(0)
        if self.single_feature:
            feats = list(last_t)
        else:
            feats = [[f[i * B:(i + 1) * B] for f in feats_tb[:-1]] + [last_t[i]] for i in range(T)]
        x_all = None if self.enable_smoothing else last_steps[:T - 1]
        store_ht, store_at, _, _ = self._deterministic_states(feats, T, hprev, cprev, aprev, caprev, x_all)
        for j, f in enumerate(feats_tb if not self.single_feature else [feats_tb]):
            DBG.check("feat%d" % j, f)
        DBG.check("ht_last", store_ht[T - 1] if len(store_ht) >= T else store_ht[-1])

        kl_loss, kl_terms = 0, []
        st_mean, st_std, st_zx = [], [], []
        base_t, noise_t = [], []
        # all 2(T-1) reparameterisation draws of the loop in one launch
        eps_all = None if draws is not None else torch.randn((T - 1, 2) + tuple(zprev.shape), device=dev)
        # The first conv of the encoder / prior sees cat(static, z) channels, and h_t, a_t and the frame features of every t
        # are known here: their share of that conv is one time-batched product per net, the per-step launches multiply
        # the z channels only (Utils.modules.recurrent_pair_split; None -> full inputs through recurrent_pair).
        h_all = torch.cat(store_ht[:T - 1], dim=0)
        Ch, Cz = int(h_all.shape[1]), int(zprev.shape[1])
        if self.enable_smoothing:
            s_enc = torch.cat(store_at[:T - 1], dim=0)
            rng_enc = (int(s_enc.shape[1]), int(s_enc.shape[1]) + Cz)
        else:
            s_enc = torch.cat((h_all, last_steps[1:T].reshape((T - 1) * B, *last_tb.shape[1:])), dim=1)
            rng_enc = (Ch, Ch + Cz)
        split_nets = recurrent_pair_split(self.encoder, s_enc, rng_enc, self.prior, h_all, (Ch, Ch + Cz), T - 1) \
            if x.is_cuda and torch.is_grad_enabled() else None
        both_nets = None if split_nets is not None else recurrent_pair(self.encoder, self.prior)
        for i in range(1, T):
            ht = store_ht[i - 1]
            if split_nets is not None:
                enc_raw, pri_raw = split_nets(i - 1, zxprev, zxprev if self.res_q else zprev)
            else:  # weight gradients time-batched, layer pairs co-launched
                if self.enable_smoothing:
                    enc_in = torch.cat((store_at[i - 1], zxprev), dim=1)
                else:
                    enc_in = torch.cat((ht, zxprev, self._last(feats[i])), dim=1)
                enc_raw, pri_raw = both_nets(enc_in, torch.cat((ht, zxprev if self.res_q else zprev), dim=1))
            # chunk + softplus, res_q shift, both reparameterised draws and the KL in one kernel (RNG order: prior first)
            eps_p = eps_like(zprev) if eps_all is None else eps_all[i - 1, 0]
            eps_q = eps_like(zprev) if eps_all is None else eps_all[i - 1, 1]
            zt, zxt, kl_t, enc_mean, enc_std = K.LatentStepFn.apply(enc_raw, pri_raw, eps_p, eps_q, self.res_q)
            DBG.check("enc_raw%d" % i, enc_raw); DBG.check("pri_raw%d" % i, pri_raw); DBG.check("zxt%d" % i, zxt)
            st_mean.append(enc_mean); st_std.append(enc_std); st_zx.append(zxprev)
            base_t.append(zxt)
            if draws is not None:
                noise_t.append(draws.pop(0).to(dev))
            if self.D == 1:
                kl_terms.append(kl_t)   # (summed after the loop: one stack + one reduction instead of T-1 adds each way)
            zprev, zxprev = zt, zxt

        # ---- the decoder: all B*(T-1) frames in one call, t-major
        xs = x_tm[B:]
        # base condition cat(h_t, z^x_t) of every step: two time-batched stacks and one channel cat
        base = torch.cat((h_all, torch.cat(base_t, dim=0)), dim=1)
        # upscaler for all T-1 steps at once; its skip maps are the extractor features of frames 0..T-2
        n1 = (T - 1) * B
        skips = None if self.single_feature else [f[:n1] for f in feats_tb]
        if self.skip_connection_features:
            conds = self.upscaler.forward_steps(base, T - 1, skip_list=skips)
        else:
            conds = self.upscaler.forward_steps(base, T - 1)
        if self.skip_connection_flow == "with_skip":
            conds = self.combineconditions(conds, skips)
        elif self.skip_connection_flow == "only_skip":
            conds = skips
        noise = torch.cat(noise_t, dim=0) if noise_t else None
        if self.training and self._flow_needs_init():
            with torch.no_grad():  # data dependent init on the t = 1 batch, as the reference's first call does
                # (batch-norm flow / prior: the reference updates the running statistics once per timestep, not once more
                # for this call)
                self.flow.log_prob(xs[:B], [c[:B] for c in conds], base[:B], 0,
                                   None if noise is None else noise[:B], update_running=False)
        for j, c in enumerate(conds):
            DBG.check("cond%d" % j, c)
        _, nll = self.flow.log_prob(xs, conds, base, logdet, noise, steps=T - 1)
        DBG.check("nll", nll)
        nll_loss = nll.view(T - 1, B).sum(0)
        if kl_terms:
            kl_loss = torch.stack(kl_terms).sum(0)

        if self.D > 1:  # overshooting (RFN_new.py:213-240)
            kl_loss = 0
            for i in range(1, T):
                overshot_loss, idt, zp = 0, i - 1, st_zx[i - 1]
                D = min(T - i, self.D)
                for d in range(D):
                    pm, ps = self.prior(torch.cat((store_ht[idt + d], zp), dim=1))
                    zp = pm + ps * eps_like(pm)
                    em, es = st_mean[idt + d], st_std[idt + d]
                    if d > 0:
                        em, es = em.detach().clone(), es.detach().clone()
                    overshot_loss = overshot_loss + self.overshot_w * kl_normal(em, es, pm, ps)
                kl_loss = kl_loss + 1 / D * overshot_loss

        kl_free_bit = free_bits_kl(kl_loss, free_bits=self.free_bits) if self.free_bits > 0 else kl_loss
        return batch_reduce(kl_free_bit).mean(), batch_reduce(kl_loss).mean(), nll_loss.mean()

    def forward(self, x, logdet=0):
        """Alias of `loss` so wrappers that hook `forward` (gradient all-reduce) see the training call."""
        return self.loss(x, logdet)

    # ------------------------------------------------------------------------------------------------ IWAE bound
    def _iw_arguments(self, who, K_, chains_per_pass):
        """(K, P) of an importance-weighted call; raises before anything runs"""
        if self.training:
            raise RuntimeError("RFN.%s needs eval mode: in training mode the batch statistics of the normalisation "
                               "layers would depend on K (call model.eval() first)" % who)
        for v, nm in ((K_, "K"), (chains_per_pass, "chains_per_pass")):
            if v is not None and (isinstance(v, bool) or int(v) != v):
                raise ValueError("RFN.%s: %s must be an integer, got %r" % (who, nm, v))
        K_ = int(K_)
        if K_ < 1:
            raise ValueError("RFN.%s: K must be at least 1, got %d" % (who, K_))
        P = K_ if chains_per_pass is None else int(chains_per_pass)
        if P < 1:
            raise ValueError("RFN.%s: chains_per_pass must be at least 1, got %d" % (who, P))
        return K_, min(P, K_)

    def iw_log_weights(self, x, K, seed, first_seq=0, first_chain=0, chains_per_pass=None):
        """The log importance weights of K posterior chains per sequence (DESIGN section 24 is the contract): a float64
        device tensor [K, B], entry [k, b] = sum_t (log p(x_t | h_t, z_t) + log p(z_t | h_t, z_{t-1}) - log q(z_t | ...))
        of chain first_chain + k of sequence first_seq + b, with z_t ~ q drawn along the chain and the flow's
        dequantisation noise u_t as part of the proposal; -ln(2^n_bits)*C*H*W per frame stays inside, as in
        flow.log_prob.  Eval mode only, run under torch.no_grad().
        The prior of step t is ALWAYS taken on the chain's own previous posterior sample z^x_{t-1}, also when res_q is
        False.  RFN.loss feeds the prior an ancestral prior sample in that case; importance weights with such a prior
        would not bound log p(x), so this method does not follow it there.  The scales are softplus(raw) as in
        rfn_latent_step; overshooting (D) and free_bits play no part.
        The extractor, the ConvLSTM and the smoothing LSTM run once per call, with the code `loss` uses.  The chains run
        in passes of P = chains_per_pass (default K) chains, P*B rows each, draw-major (row r*B + b): per step the encoder
        and prior convolutions on the replicated static inputs and one rfn_hip.ops.latent_iw launch, then ONE upscaler
        call and ONE flow.log_prob(..., steps=T-1) call for the pass's (T-1)*P*B frames, t-major as in `loss`.
        Noise: a chain is a "draw" of the addressing.  eps_t is rfn_hip.ops.keyed_normal slot 0 at step t, u_t is
        rfn_hip.ops.keyed_uniform slot 24 at step t with scale 2^-n_bits.  An entry therefore depends on (seed, sequence
        id, chain id) and the data alone -- not on K, P, B or torch's generators, which are left untouched -- up to the
        summation order of the batched kernels."""
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        Kc, P = self._iw_arguments("iw_log_weights", K, chains_per_pass)
        B, T = int(x.shape[0]), int(x.shape[1])
        if T < 2:
            raise ValueError("RFN.iw_log_weights: need at least 2 frames, got %d" % T)
        seed, first_seq, first_chain = int(seed), int(first_seq), int(first_chain)
        S = T - 1

        def rep_steps(t, p):   # [S, B, ...] -> [S*p*B, ...]: row (s*p + r)*B + b is sequence b at step s
            return t.unsqueeze(1).expand(S, p, *t.shape[1:]).reshape(S * p * B, *t.shape[2:])

        with torch.no_grad():
            # ---- the sample-independent front, as in `loss`: once for all chains
            hprev, cprev, aprev, caprev, _, z0x, _, _, _ = self.get_inits()
            x_tm = x.transpose(0, 1).reshape(T * B, *x.shape[2:])
            feats_tb = self.extractor.forward_steps(x_tm, T)
            last_tb = feats_tb if self.single_feature else feats_tb[-1]
            last_steps = last_tb.view(T, B, *last_tb.shape[1:])
            last_t = last_steps.unbind(0)
            if self.single_feature:
                feats = list(last_t)
            else:
                feats = [[f[i * B:(i + 1) * B] for f in feats_tb[:-1]] + [last_t[i]] for i in range(T)]
            x_all = None if self.enable_smoothing else last_steps[:S]
            store_ht, store_at, _, _ = self._deterministic_states(feats, T, hprev, cprev, aprev, caprev, x_all)
            h_sb = torch.stack(store_ht[:S], 0)
            # the encoder's static input channels: a_t, or (h_t, features of frame t) around the z channels
            enc_sb = torch.stack(store_at[:S], 0) if self.enable_smoothing else last_steps[1:T]
            skips_sb = None if self.single_feature else [f.view(T, B, *f.shape[1:])[:S] for f in feats_tb]
            xs_sb = x_tm.view(T, B, *x.shape[2:])[1:]
            zshape = tuple(z0x.shape[1:])
            both_nets = recurrent_pair(self.encoder, self.prior)
            scale = 1.0 / 2 ** self.flow.n_bits

            tables = []
            for c0 in range(0, Kc, P):
                p = min(P, Kc - c0)
                R = p * B
                h_rep = rep_steps(h_sb, p)
                h_steps, enc_steps = h_rep.view(S, R, *h_sb.shape[2:]), rep_steps(enc_sb, p).view(S, R, *enc_sb.shape[2:])
                zx = z0x.repeat(p, 1, 1, 1)
                base_t, logr_t = [], []
                for i in range(1, T):
                    ht = h_steps[i - 1]
                    if self.enable_smoothing:
                        enc_in = torch.cat((enc_steps[i - 1], zx), dim=1)
                    else:
                        enc_in = torch.cat((ht, zx, enc_steps[i - 1]), dim=1)
                    enc_raw, pri_raw = both_nets(enc_in, torch.cat((ht, zx), dim=1))
                    eps, = ops.keyed_normal([zshape], B, p, seed, i, first_seq, first_chain + c0, device=x.device)
                    zx, logr = ops.latent_iw(enc_raw, pri_raw, eps, self.res_q)
                    base_t.append(zx)
                    logr_t.append(logr)
                # ---- the decoder: all (T-1)*p*B frames of the pass in one call, t-major
                base = torch.cat((h_rep, torch.cat(base_t, dim=0)), dim=1)
                skips = None if skips_sb is None else [rep_steps(f, p) for f in skips_sb]
                if self.skip_connection_features:
                    conds = self.upscaler.forward_steps(base, S, skip_list=skips)
                else:
                    conds = self.upscaler.forward_steps(base, S)
                if self.skip_connection_flow == "with_skip":
                    conds = self.combineconditions(conds, skips)
                elif self.skip_connection_flow == "only_skip":
                    conds = skips
                u = ops.keyed_uniform(tuple(x.shape[2:]), B, p, seed, 1, n_steps=S, scale=scale, first_seq=first_seq,
                                    first_draw=first_chain + c0, device=x.device)
                _, nll = self.flow.log_prob(rep_steps(xs_sb, p), conds, base, 0, u.view(S * R, *x.shape[2:]), steps=S)
                tables.append((torch.cat(logr_t, dim=0).double() - nll.double()).view(S, p, B).sum(0))
            return torch.cat(tables, dim=0)

    def elbo_importance_weighting(self, x, K, seed=0, first_seq=0, chains_per_pass=None):
        """The importance-weighted bound of RFN in the sign and unit of the baselines' methods of this name (nats per
        sequence): -mean_b (logsumexp_k log w[k, b] - log K) over the K chains of `iw_log_weights` (chains 0 .. K-1 of
        sequences first_seq .. first_seq + B - 1 under `seed`), a float64 scalar on the device.  (u, z) is a joint
        proposal, so this is the standard sequence-level IWAE bound; K = 1 is a one-sample ELBO estimate.  The prior is
        always taken on the chain's own posterior sample, also when res_q is False, where RFN.loss does otherwise: see
        iw_log_weights.  Eval mode only."""
        self._iw_arguments("elbo_importance_weighting", K, chains_per_pass)
        return -iw_bound(self.iw_log_weights(x, K, seed, first_seq, 0, chains_per_pass)).mean()

    # ------------------------------------------------------------------------------------------------ generation
    # `draws` (optional, tests): the noise in the reference's draw order, see each method.
    def _gen_step(self, prediction, hprev, cprev, zprev, eps, kl_temp, temperature=None):
        """one autoregressive generation step (RFN_new.py:331-356 / :480-491): frame t-1 -> frame t.
        eps: [prior eps, flow base eps, Split2d eps (coarsest first) ...].  Returns (frame, ht, ct, zt).
        kl_temp: a number, or a [N, 1, 1, 1] tensor with one value per row; temperature: the flow's sampling
        temperature, None for self.temperature, or an N-element device tensor with one value per row."""
        eps = list(eps)
        take = lambda ref=None: eps.pop(0)
        condition_list = self.extractor(prediction)
        _, ht, ct = self.lstm(self._last(condition_list).unsqueeze(1), hprev, cprev)
        pm, ps = self.prior(torch.cat((ht, zprev), dim=1))
        zt = pm + ps * kl_temp * take(pm)
        hz = torch.cat((ht, zt), dim=1)
        fc = self._flow_conditions(hz, condition_list)
        frame = self._flow_sample(fc, hz, take, True, temperature=temperature)
        return frame, ht, ct, zt

    def _gen_eps_shapes(self, B):
        """shapes of the draws of one generation step: prior eps, base eps, Split2d eps list (coarsest first)"""
        hu, wu = self.z_0.shape[2], self.z_0.shape[3]
        shapes = [(B, self.z_dim, hu, wu)]
        c, h, w = self.x_dim[1], self.x_dim[2], self.x_dim[3]
        split = []
        for l in range(self.L):
            c, h, w = c * 4, h // 2, w // 2
            if l < self.L - 1:
                c = c // 2
                split.append((B, c, h, w))
        shapes.append((B, c, h, w))          # base distribution = what is left after the last level
        return shapes + split[::-1]

    _GEN_GRAPHS_KEPT = 4   # captured generation graphs kept per model, one per batch shape

    def _gen_step_graphed(self, prediction, hprev, cprev, zprev, kl_temp, eps_fill=None, temp_rows=None):
        """_gen_step with fresh N(0,1) draws, replayed from a hipGraph: generation is one frame at a time, a few hundred
        launches of a few microseconds each, i.e. bound by the host's launch rate when launched eagerly (38 ms per frame at
        B = 32 against ~6 ms of GPU work).  A graph is rebuilt whenever a parameter changed (the inverse matrices and
        weight packs of ListGlow._reverse_cache are baked into it); the draws are inputs of the graph.  One graph is kept
        per batch shape (`_gen_graphs`, the last few shapes used), so that predict at batch B and predict_draws at batch
        P*B alternate without a rebuild; `_gen_graph` is the one used last.
        eps_fill (optional): a callable that writes the draws into the list of eps tensors it is given, in place
        (predict_draws: addressed noise, written straight into the graph's inputs); without it the draws come from
        torch's generator, L + 1 launches.
        temp_rows (optional, predict_draws with per-row temperatures): (temperature [N], kl temperature [N]) device
        tensors; kl_temp is then ignored and self.temperature is not read.  The two vectors are static inputs of the
        graph, copied in before each replay like the state, and the graph's key holds the fact that the mode is
        per-row, not the values: another list of temperatures at the same shapes and weights replays the same graph."""
        import rfn_hip
        dev = prediction.device
        shapes = self._gen_eps_shapes(prediction.shape[0])
        ok = (dev.type == "cuda" and rfn_hip.graph_capture_safe() and not self.training
              and os.environ.get("RFN_GEN_GRAPH", "1") != "0")
        if eps_fill is None:
            eps = [torch.randn(sh, device=dev) for sh in shapes]
        elif not ok:
            eps = [torch.empty(sh, device=dev) for sh in shapes]
            eps_fill(eps)
        else:
            eps = None   # written into the graph's inputs below
        state = [prediction, hprev, cprev, zprev]
        n_eps = len(shapes)

        def step(ins):   # ins: the state, the draws [, temperature rows, kl temperature rows]
            if temp_rows is None:
                return self._gen_step(*ins[:4], ins[4:4 + n_eps], kl_temp)
            return self._gen_step(*ins[:4], ins[4:4 + n_eps], ins[5 + n_eps].view(-1, 1, 1, 1), ins[4 + n_eps])

        if not ok:
            return step(state + list(eps) + list(temp_rows or ()))
        shape_key = tuple(tuple(a.shape) for a in state) + tuple(shapes)
        if temp_rows is None:
            key = (tuple((p._version, p.data_ptr()) for p in self.parameters()), shape_key,
                   float(kl_temp), float(self.temperature))
        else:
            shape_key += ("rows",)   # its own entry: a scalar-mode graph of the same shapes is kept beside it
            key = (tuple((p._version, p.data_ptr()) for p in self.parameters()), shape_key, "rows")
        graphs = self.__dict__.setdefault("_gen_graphs", {})
        g = graphs.pop(shape_key, None)
        if g is None or g[0] != key:
            static_in = [a.clone() for a in state]
            if eps is not None:
                static_in += [a.clone() for a in eps]
            else:
                static_in += [torch.empty(sh, device=dev) for sh in shapes]
                eps_fill(static_in[4:])
            if temp_rows is not None:
                static_in += [a.clone() for a in temp_rows]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):  # warm-up on the capture path (lazy per-stream state, generation cache, MIOpen)
                    step(static_in)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = step(static_in)
            g = (key, graph, static_in, static_out)
            self._gen_graph_builds = getattr(self, "_gen_graph_builds", 0) + 1
        graphs[shape_key] = g          # most recently used last
        while len(graphs) > self._GEN_GRAPHS_KEPT:
            graphs.pop(next(iter(graphs)))
        self._gen_graph = g
        _, graph, static_in, static_out = g
        for s_, a in zip(static_in, state):
            s_.copy_(a)
        if eps is not None:
            for s_, a in zip(static_in[4:], eps):
                s_.copy_(a)
        else:
            eps_fill(static_in[4:4 + n_eps])
        if temp_rows is not None:
            for s_, a in zip(static_in[4 + n_eps:], temp_rows):
                s_.copy_(a)
        graph.replay()
        return tuple(o.clone() for o in static_out)

    def _flow_sample(self, fc, hz, take, pinned, z=None, temperature=None):
        """flow.sample with pinned draws: base eps (only when z is None), then the Split2d eps list, coarsest first.
        temperature: None for self.temperature, or a number, or one value per row as a device tensor"""
        eb = take() if (pinned and z is None) else None
        el = [take() for _ in range(self.L - 1)] if pinned else None
        return self.flow.sample(z, fc, hz, temperature=self.temperature if temperature is None else temperature,
                                eps_base=eb, eps_list=el)

    # predict / reconstruct / sample end in `.cpu()`, as the reference's do; the `_*_device` bodies return the same
    # tensors where they were computed (Solver.plotter composes its sheet from them without a host round trip).
    def predict(self, x, n_predictions, n_conditions, draws=None):
        """RFN/RFN_new.py:256-360 — condition on n_conditions frames, roll the prior forward n_predictions frames.
        draws: per warm-up step prior eps, encoder eps; per prediction prior eps, base eps, Split2d eps list."""
        true_x, predictions = self._predict_device(x, n_predictions, n_conditions, draws)
        return true_x.cpu(), predictions.cpu()

    def _predict_device(self, x, n_predictions, n_conditions, draws=None):
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        with torch.no_grad():
            take, dr = self._taker(draws, x.device)
            hprev, cprev, aprev, caprev, zprev, zxprev, _, _, _ = self.get_inits()
            feats = [self.extractor(x[:, i]) for i in range(n_conditions)]
            store_ht, store_at, hprev, cprev = self._deterministic_states(feats, n_conditions, hprev, cprev, aprev, caprev)
            for i in range(1, n_conditions):
                ht = store_ht[i - 1]
                if self.enable_smoothing:
                    enc_mean, enc_std = self.encoder(torch.cat((store_at[i - 1], zxprev), dim=1))
                else:
                    enc_mean, enc_std = self.encoder(torch.cat((ht, zxprev, self._last(feats[i])), dim=1))
                if self.res_q:
                    prior_mean, prior_std = self.prior(torch.cat((ht, zxprev), dim=1))
                    enc_mean = prior_mean + enc_mean
                else:
                    prior_mean, prior_std = self.prior(torch.cat((ht, zprev), dim=1))
                zprev = prior_mean + prior_std * self.kl_temperature * take(prior_mean)
                zxprev = enc_mean + enc_std * take(enc_mean)
            true_x = x[:, :n_conditions].transpose(0, 1).detach().clone()
            frames = []  # kept on the device: ONE device-to-host copy at the end instead of a sync per frame
            prediction = x[:, n_conditions - 1]
            for i in range(n_predictions):
                if dr is None:
                    prediction, ht, ct, zt = self._gen_step_graphed(prediction, hprev, cprev, zprev, self.kl_temperature)
                else:
                    eps = [take() for _ in range(self.L + 1)]
                    prediction, ht, ct, zt = self._gen_step(prediction, hprev, cprev, zprev, eps, self.kl_temperature)
                frames.append(prediction.detach())
                hprev, cprev, zprev = ht, ct, zt
            predictions = torch.stack(frames, 0) if frames else torch.zeros((0, *x[:, 0].shape), device=x.device)
        return true_x, predictions

    def predict_draws(self, x, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0,
                      temperatures=None, kl_temperatures=None):
        """`predict` for n_draws independent draws of every sequence in one pass, with addressed noise: returns
        (true_x, predictions), predictions [n_predictions, n_draws, B, C, H, W] on the CPU (`_predict_draws_device`: the
        same on the device).  The extractor and the ConvLSTM run once over the conditioning frames of the B sequences;
        from the first latent step on everything runs on n_draws*B rows, draw-major (row r*B + b: draw first_draw + r
        of sequence first_seq + b), the generation through _gen_step / its hipGraph at that batch.
        Noise: rfn_hip.ops.keyed_normal, one launch per step.  Conditioning step i (1 .. n_conditions-1) uses t = i:
        slot 0 the prior eps, slot 1 the encoder eps.  Generated frame i uses t = n_conditions + i: slot 0 the prior
        eps, slot 2 the flow's base eps, slots 3.. the Split2d eps list, coarsest first (the order of _gen_eps_shapes).
        A frame therefore depends on (seed, sequence id, draw id) and the data alone: not on B, on n_draws, on how the
        draws are split into calls, or on torch's generator, which is left untouched.  Eval mode only: batch statistics
        would couple the draws.
        temperatures / kl_temperatures (each a sequence of K numbers, or None): a sweep over K (temperature, kl
        temperature) pairs in the same pass; None stands for K copies of self.temperature / self.kl_temperature, and
        two lists have the same length.  With either given, predictions are [n_predictions, K, n_draws, B, C, H, W]:
        the batch is temperature-major, then draw-major (row (k*n_draws + r)*B + b), the conditioning frames are
        encoded once for all K*n_draws*B rows, and every place a temperature enters -- the prior samples of the
        warm-up steps and of generation, the flow's base and Split2d samples -- takes its row's value from a device
        vector.  The noise is tiled (keyed_normal(tiles=K)): block k uses exactly the numbers the call without
        temperatures uses, so a block does not depend on which other temperatures are swept with it.  In this mode
        the model's temperature / kl_temperature attributes are neither read (for the given lists) nor written."""
        true_x, predictions = self._predict_draws_device(x, n_predictions, n_conditions, n_draws, seed, first_seq,
                                                         first_draw, temperatures, kl_temperatures)
        return true_x.cpu(), predictions.cpu()

    def _temperature_lists(self, temperatures, kl_temperatures):
        """the two lists of K floats of a per-row call (None: K copies of the model's value, the only case in which an
        attribute is read)"""
        lists = []
        for v, nm in ((temperatures, "temperatures"), (kl_temperatures, "kl_temperatures")):
            if v is None:
                lists.append(None)
                continue
            if isinstance(v, (str, bytes, torch.Tensor)) or not hasattr(v, "__len__"):
                raise TypeError("RFN.predict_draws: %s must be a sequence of numbers, got %s" % (nm, type(v).__name__))
            v = [float(t) for t in v]
            if not v:
                raise ValueError("RFN.predict_draws: %s is empty" % nm)
            lists.append(v)
        t, kl = lists
        if t is not None and kl is not None and len(t) != len(kl):
            raise ValueError("RFN.predict_draws: %d temperatures and %d kl_temperatures" % (len(t), len(kl)))
        K_ = len(t if t is not None else kl)
        return (t if t is not None else [float(self.temperature)] * K_,
                kl if kl is not None else [float(self.kl_temperature)] * K_)

    @staticmethod
    def _temperature_rows(values, P, B, device):
        """float32 [K*P*B] on `device`: row rfn_hip.ops.keyed_normal_tiled_row(k, r, b, P, B) holds values[k]"""
        return torch.tensor(values, dtype=torch.float32).repeat_interleave(P * B).to(device)

    def _predict_draws_device(self, x, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0,
                              temperatures=None, kl_temperatures=None):
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        if self.training:
            raise RuntimeError("RFN.predict_draws needs eval mode: in training mode the batch statistics of the "
                               "normalisation layers would couple the draws (call model.eval() first)")
        P, B = int(n_draws), int(x.shape[0])
        if P < 1:
            raise ValueError("RFN.predict_draws: n_draws must be at least 1, got %d" % P)
        if self.L + 2 > K.KEYED_NORMAL_MAX_SLOTS:
            raise ValueError("RFN.predict_draws: L = %d needs %d noise slots, one launch fills %d" %
                             (self.L, self.L + 2, K.KEYED_NORMAL_MAX_SLOTS))

        per_row = temperatures is not None or kl_temperatures is not None
        Kt, temp_rows, kl_temp = 1, None, None
        if per_row:
            t_list, kl_list = self._temperature_lists(temperatures, kl_temperatures)
            Kt = len(t_list)
            # temperature-major: row (k*P + r)*B + b takes entry k
            temp_rows = tuple(self._temperature_rows(v, P, B, x.device) for v in (t_list, kl_list))
            kl_temp = temp_rows[1].view(-1, 1, 1, 1)
        else:
            kl_temp = self.kl_temperature

        def rep(t):   # (temperature-major, then) draw-major: row (k*P + r)*B + b is sequence b
            return t.repeat((Kt * P,) + (1,) * (t.dim() - 1))

        with torch.no_grad():
            hprev, cprev, aprev, caprev, zprev, zxprev, _, _, _ = self.get_inits()
            feats = [self.extractor(x[:, i]) for i in range(n_conditions)]
            store_ht, store_at, hprev, cprev = self._deterministic_states(feats, n_conditions, hprev, cprev, aprev, caprev)
            zprev, zxprev = rep(zprev), rep(zxprev)
            zshape = tuple(zprev.shape[1:])
            for i in range(1, n_conditions):
                eps_p, eps_q = K.keyed_normal([zshape, zshape], B, P, seed, i, first_seq, first_draw, device=x.device,
                                              tiles=Kt)
                ht = rep(store_ht[i - 1])
                if self.enable_smoothing:
                    enc_mean, enc_std = self.encoder(torch.cat((rep(store_at[i - 1]), zxprev), dim=1))
                else:
                    enc_mean, enc_std = self.encoder(torch.cat((ht, zxprev, rep(self._last(feats[i]))), dim=1))
                if self.res_q:
                    prior_mean, prior_std = self.prior(torch.cat((ht, zxprev), dim=1))
                    enc_mean = prior_mean + enc_mean
                else:
                    prior_mean, prior_std = self.prior(torch.cat((ht, zprev), dim=1))
                zprev = prior_mean + prior_std * kl_temp * eps_p
                zxprev = enc_mean + enc_std * eps_q
            true_x = x[:, :n_conditions].transpose(0, 1).detach().clone()
            frames = []
            prediction, hprev, cprev = rep(x[:, n_conditions - 1]), rep(hprev), rep(cprev)
            for i in range(n_predictions):
                def fill(eps, t=n_conditions + i):   # slot 1 (the encoder eps) is not drawn while generating
                    K.keyed_normal(None, B, P, seed, t, first_seq, first_draw, out=[eps[0], None] + list(eps[1:]),
                                   tiles=Kt)
                prediction, ht, ct, zt = self._gen_step_graphed(prediction, hprev, cprev, zprev,
                                                                None if per_row else kl_temp, eps_fill=fill,
                                                                temp_rows=temp_rows)
                frames.append(prediction.detach())
                hprev, cprev, zprev = ht, ct, zt
            lead = (Kt, P, B) if per_row else (P, B)
            if frames:
                predictions = torch.stack(frames, 0).view(n_predictions, *lead, *x.shape[2:])
            else:
                predictions = torch.zeros((0, *lead, *x.shape[2:]), device=x.device)
        return true_x, predictions

    def reconstruct(self, x, draws=None):
        """RFN/RFN_new.py:362-450 — posterior reconstructions and the flow bijection check g(f(x)).
        draws: per frame encoder eps, dequantisation noise, Split2d eps list of g(f(x)), base eps + Split2d eps list of
        the fresh sample."""
        recons, recons_flow = self._reconstruct_device(x, draws)
        return recons.cpu(), recons_flow.cpu()

    def _reconstruct_device(self, x, draws=None):
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        with torch.no_grad():
            take, dr = self._taker(draws, x.device)
            T = x.shape[1]
            hprev, cprev, aprev, caprev, _, zxprev, _, _, _ = self.get_inits()
            # results stay on the device until the end: a pageable device-to-host copy per frame stalls the launch stream
            recons = torch.zeros((T, *x[:, 0].shape), device=x.device)
            recons_flow = torch.zeros((T, *x[:, 0].shape), device=x.device)
            feats = [self.extractor(x[:, i]) for i in range(T)]
            store_ht, store_at, _, _ = self._deterministic_states(feats, T, hprev, cprev, aprev, caprev)
            for i in range(1, T):
                ht = store_ht[i - 1]
                if self.enable_smoothing:
                    enc_mean, enc_std = self.encoder(torch.cat((store_at[i - 1], zxprev), dim=1))
                else:
                    enc_mean, enc_std = self.encoder(torch.cat((ht, zxprev, self._last(feats[i])), dim=1))
                if self.res_q:
                    prior_mean, _ = self.prior(torch.cat((ht, zxprev), dim=1))
                    enc_mean = prior_mean + enc_mean
                zxt = enc_mean + enc_std * take(enc_mean)
                hz = torch.cat((ht, zxt), dim=1)
                fc = self._flow_conditions(hz, feats[i - 1])
                z, _ = self.flow.log_prob(x[:, i], fc, hz, 0.0, take() if dr is not None else None)
                recons_flow[i] = self._flow_sample(fc, hz, take, dr is not None, z=z)
                recons[i] = self._flow_sample(fc, hz, take, dr is not None)
                zxprev = zxt
        return recons, recons_flow

    def sample(self, x, n_samples, draws=None):
        """RFN/RFN_new.py:453-494 — unconditional roll-out from the first frame.
        draws: per sample prior eps, base eps, Split2d eps list."""
        return self._sample_device(x, n_samples, draws).cpu()

    def _sample_device(self, x, n_samples, draws=None):
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        with torch.no_grad():
            take, dr = self._taker(draws, x.device)
            hprev, cprev, _, _, zprev, _, _, _, _ = self.get_inits()
            frames = []
            sample = x[:, 0]
            for i in range(n_samples):
                if dr is None:
                    sample, ht, ct, zt = self._gen_step_graphed(sample, hprev, cprev, zprev, 1.0)
                else:
                    eps = [take() for _ in range(self.L + 1)]
                    sample, ht, ct, zt = self._gen_step(sample, hprev, cprev, zprev, eps, 1.0)
                frames.append(sample)
                zprev, hprev, cprev = zt, ht, ct
            samples = torch.stack(frames, 0) if frames else torch.zeros((0, *x[:, 0].shape), device=x.device)
        return samples

    # ------------------------------------------------------------------------------------------------ analyses
    # The evaluation-time methods of the reference (RFN/RFN_new.py:496-788), built on the same kernels.  They run under
    # torch.no_grad() like the reference's evaluator does; `draws` (optional) pins the noise in the reference's draw
    # order so that parity tests can feed the GPU path, the oracle and the reference the same numbers.
    def _post_prior_step(self, i, store_ht, store_at, feats, zprev, zxprev, take):
        """one latent step (RFN_new.py:548-566 and its copies): (zt, zxt, prior_mean, prior_std, enc_mean, enc_std)"""
        ht = store_ht[i - 1]
        if self.enable_smoothing:
            enc_mean, enc_std = self.encoder(torch.cat((store_at[i - 1], zxprev), dim=1))
        else:
            enc_mean, enc_std = self.encoder(torch.cat((ht, zxprev, self._last(feats[i])), dim=1))
        if self.res_q:
            prior_mean, prior_std = self.prior(torch.cat((ht, zxprev), dim=1))
            enc_mean = prior_mean + enc_mean
        else:
            prior_mean, prior_std = self.prior(torch.cat((ht, zprev), dim=1))
        zt = prior_mean + prior_std * take(prior_mean)        # draw order: prior first, then encoder
        zxt = enc_mean + enc_std * take(enc_mean)
        return zt, zxt, prior_mean, prior_std, enc_mean, enc_std

    @staticmethod
    def _taker(draws, dev):
        draws = list(draws) if draws is not None else None

        def take(ref=None, uniform=False):
            if draws is not None:
                return draws.pop(0).to(dev)
            if ref is None:
                return None
            return torch.randn(ref.shape, device=dev)
        return take, draws

    def reconstruct_elbo_gap(self, x, sample=True, draws=None):
        """RFN/RFN_new.py:687-788 -- per-frame KL and the flow NLL under z ~ prior (index 0) and z ~ posterior (index 1),
        plus (sample=True) reconstructions.  Returns (recons, recons_flow, averageKLDseq [T,B], averageNLLseq [2,T,B]).
        draws: per t: prior eps, encoder eps, then per z in (prior, posterior): dequantisation noise [, with sample:
        the Split2d eps list of g(f(x)), the base eps and the Split2d eps list of the fresh sample]."""
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        with torch.no_grad():
            B, T = x.shape[0], x.shape[1]
            take, dr = self._taker(draws, x.device)
            hprev, cprev, aprev, caprev, zprev, zxprev, _, _, _ = self.get_inits()
            feats = [self.extractor(x[:, i]) for i in range(T)]
            store_ht, store_at, _, _ = self._deterministic_states(feats, T, hprev, cprev, aprev, caprev)
            kld = torch.zeros((T, B), device=x.device)
            nlls = torch.zeros((2, T, B), device=x.device)
            recons = torch.zeros((2, T, *x[:, 0].shape), device=x.device) if sample else 0
            recons_flow = torch.zeros((2, T, *x[:, 0].shape), device=x.device) if sample else 0
            nsplit = self.L - 1
            for i in range(1, T):
                zt, zxt, pm, ps, em, es = self._post_prior_step(i, store_ht, store_at, feats, zprev, zxprev, take)
                ht = store_ht[i - 1]
                for count, zk in enumerate((zt, zxt)):
                    hz = torch.cat((ht, zk), dim=1)
                    fc = self._flow_conditions(hz, feats[i - 1])
                    b, nll = self.flow.log_prob(x[:, i], fc, hz, 0.0, take() if dr is not None else None)
                    nlls[count, i] = nll
                    if sample:
                        e1 = [take() for _ in range(nsplit)] if dr is not None else None
                        rf = self.flow.sample(b, fc, hz, temperature=self.temperature, eps_list=e1)
                        eb = take() if dr is not None else None
                        e2 = [take() for _ in range(nsplit)] if dr is not None else None
                        rs = self.flow.sample(None, fc, hz, temperature=self.temperature, eps_base=eb, eps_list=e2)
                        recons[count, i] = rs
                        recons_flow[count, i] = rf
                zprev, zxprev = zt, zxt
                kld[i] = kl_normal(em, es, pm, ps).sum([1, 2, 3])
        if sample:
            recons, recons_flow = recons.cpu(), recons_flow.cpu()
        return recons, recons_flow, kld.cpu(), nlls.cpu()

    def probability_future(self, x, n_conditions, draws=None):
        """RFN/RFN_new.py:590-685 -- NLL of the frames after n_conditions conditioning frames under the LAST conditioned
        state, with z ~ prior (index 0) and z ~ posterior (index 1).  The reference writes frame i's value to column
        i - n_conditions - 1 of a [B, 2, T - n_conditions - 1] tensor, i.e. frame n_conditions lands in the last column
        and is overwritten by the last frame; that indexing is kept.  draws: per warm-up step prior eps, encoder eps;
        then per frame and z the dequantisation noise."""
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        with torch.no_grad():
            B, T = x.shape[0], x.shape[1]
            take, dr = self._taker(draws, x.device)
            hprev, cprev, aprev, caprev, zprev, zxprev, _, _, _ = self.get_inits()
            out = torch.zeros((B, 2, T - n_conditions - 1), device=x.device)
            feats = [self.extractor(x[:, i]) for i in range(n_conditions)]
            store_ht, store_at, _, _ = self._deterministic_states(feats, n_conditions, hprev, cprev, aprev, caprev)
            zt = zxt = None
            for i in range(1, n_conditions):
                zt, zxt, _, _, _, _ = self._post_prior_step(i, store_ht, store_at, feats, zprev, zxprev, take)
                zprev, zxprev = zt, zxt
            ht = store_ht[n_conditions - 2]
            for i in range(n_conditions, T):
                for count, zk in enumerate((zt, zxt)):
                    hz = torch.cat((ht, zk), dim=1)
                    fc = self._flow_conditions(hz, feats[n_conditions - 2])
                    _, nll = self.flow.log_prob(x[:, i], fc, hz, 0.0, take() if dr is not None else None)
                    out[:, count, i - n_conditions - 1] = nll
        return out.cpu()

    def param_analysis(self, x, n_predictions, n_conditions, draws=None):
        """RFN/RFN_new.py:496-588 -- prior / posterior / flow-base parameters along the sequence and one flow sample per
        step.  (The reference passes 1.0 in the num_samples slot of flow.sample, so the sampling temperature is the
        default 0.8; frame 0 of `predictions` stays zero.)  draws: per step prior eps, encoder eps, base eps, the
        Split2d eps list."""
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        with torch.no_grad():
            B = x.shape[0]
            T = n_conditions + n_predictions
            take, dr = self._taker(draws, x.device)
            hprev, cprev, aprev, caprev, zprev, zxprev, _, _, _ = self.get_inits()
            feats = [self.extractor(x[:, i]) for i in range(T)]
            store_ht, store_at, _, _ = self._deterministic_states(feats, T, hprev, cprev, aprev, caprev)
            zs = tuple(zprev.shape[1:])
            dv = x.device
            mu_p, std_p = torch.zeros((T - 1, B) + zs, device=dv), torch.zeros((T - 1, B) + zs, device=dv)
            mu_q, std_q = torch.zeros((T - 1, B) + zs, device=dv), torch.zeros((T - 1, B) + zs, device=dv)
            mu_flow, std_flow = [], []
            predictions = torch.zeros((B, T, *x.shape[2:]), device=dv)
            nsplit = self.L - 1
            for i in range(1, T):
                zt, zxt, pm, ps, em, es = self._post_prior_step(i, store_ht, store_at, feats, zprev, zxprev, take)
                mu_p[i - 1], std_p[i - 1], mu_q[i - 1], std_q[i - 1] = pm, ps, em, es
                ht = store_ht[i - 1]
                fc = self._flow_conditions(torch.cat((ht, zxt), dim=1), feats[i - 1])
                base = torch.cat((ht, zt), dim=1)
                eb = take() if dr is not None else None
                el = [take() for _ in range(nsplit)] if dr is not None else None
                pred, params = self.flow.sample(None, fc, base, 1.0, eval_params=True, eps_base=eb, eps_list=el)
                mu_flow.append(params[0])
                std_flow.append(params[1])
                predictions[:, i] = pred
                zprev, zxprev = zt, zxt
        return (mu_p.cpu(), std_p.cpu(), mu_q.cpu(), std_q.cpu(), torch.stack(mu_flow).cpu(), torch.stack(std_flow).cpu(),
                predictions.cpu())
