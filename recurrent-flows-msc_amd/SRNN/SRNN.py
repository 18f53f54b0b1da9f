"""SRNN baseline — host mirror of the reference's SRNN/SRNN.py: same constructor arguments read from `args`, same
state_dict keys and shapes, same layer structure, and the reference's behaviour where it differs from its comments
(`store_ztx` holds zprevx; the non-smoothing encoder runs phi_x_t a second time per step).

On the package's kernels: the two ConvLSTMs (Utils.ConvLSTM) and, for `loss_type == "mol"`, the mixture of discretized
logistics: the logits of all T-1 frames are collected in the time loop and go through rfn_hip.ops.mol_nll in ONE launch
after it (the likelihood has no state across steps); the per-frame sums are added over time in step order.  Strided
convolutions, ConvTranspose2d, Linear and the norm layers are PyTorch modules.

Every method that draws takes `draws=None`: a list of tensors (or (kind, tensor) pairs, as the fixtures store them)
consumed in the order the reference draws — standard normals of each rsample, the uniforms of the dequantisation and of
the mixture sampler (u_mix [N,H,W,M], then u_x [N,H,W,C]).

`predict_draws` (several draws of every sequence in one pass, with addressed noise) and `elbo_importance_weighting` (the
bound the reference reports as the baselines' bits/dim) are what the Evaluator drives for srnn.pt; DESIGN.md section 20."""
import numpy as np
import torch
import torch.distributions as td
import torch.nn as nn

from Utils import ConvLSTM, NormLayer
from Utils import DiscretizedMixtureLogits, DiscretizedMixtureLogits_1d
from Utils import Flatten, UnFlatten, batch_reduce, get_layer_size


class _Draws:
    """the recorded draws in order, or fresh ones"""

    def __init__(self, draws, device):
        self.q = None if draws is None else [d[1] if isinstance(d, (tuple, list)) else d for d in draws]
        self.device = device

    def _next(self, shape):
        t = self.q.pop(0)
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("recorded draw has shape %s, the model asks for %s" % (tuple(t.shape), tuple(shape)))
        return t.to(self.device)

    def normal(self, shape):
        return torch.randn(tuple(shape), device=self.device) if self.q is None else self._next(shape)

    def uniform(self, shape, lo, hi):
        if self.q is None:
            return torch.empty(tuple(shape), device=self.device).uniform_(lo, hi)
        return self._next(shape)

    def rsample(self, dist):
        return dist.loc + dist.scale * self.normal(dist.loc.shape)

    def done(self):
        if self.q:
            raise RuntimeError("%d recorded draws left over" % len(self.q))


def _mlp(n_in, z_dim, softplus):
    layers = [nn.Linear(n_in, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, z_dim)]
    return nn.Sequential(*(layers + [nn.Softplus()] if softplus else layers))


class SRNN(nn.Module):
    def __init__(self, args):
        super().__init__()
        norm_type = args.norm_type
        self.batch_size = args.batch_size
        self.u_dim = args.condition_dim
        self.a_dim = args.a_dim
        self.x_dim = args.x_dim
        self.enable_smoothing = args.enable_smoothing
        self.h_dim, self.z_dim = h_dim, z_dim = args.h_dim, args.z_dim
        self.loss_type = args.loss_type
        self.beta = 1
        bu, cu, hu, wu = self.u_dim
        bx, cx, hx, wx = self.x_dim
        self.mse_criterion = nn.MSELoss(reduction="none")
        self.res_q = args.res_q
        self.bits = args.n_bits
        self.dequantize = args.dequantize
        self.preprocess_range = args.preprocess_range
        self.n_logistics = args.n_logistics

        def block(conv, c):
            return [conv, NormLayer(c, norm_type), nn.ReLU()]

        self.phi_x_t_channels = 256
        self.phi_x_t = nn.Sequential(
            *block(nn.Conv2d(cx, 64, kernel_size=3, stride=2, padding=1), 64),
            *block(nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1), 128),
            *block(nn.Conv2d(128, 256, kernel_size=3, stride=2, padding=1), 256),
            *block(nn.Conv2d(256, self.phi_x_t_channels, kernel_size=3, stride=1, padding=1), self.phi_x_t_channels))
        h, w = get_layer_size([hu, wu], kernels=[3, 3, 3], paddings=[1, 1, 1], strides=[2, 2, 2], dilations=[1, 1, 1])
        self.h, self.w = h, w

        phi_z_channels = 128
        self.phi_z = nn.Sequential(
            nn.Linear(z_dim, phi_z_channels * h * w), nn.ReLU(),
            nn.Linear(phi_z_channels * h * w, phi_z_channels * h * w), nn.ReLU(),
            UnFlatten(phi_z_channels, h, w),
            *block(nn.Conv2d(phi_z_channels, phi_z_channels, kernel_size=3, stride=1, padding=1), phi_z_channels))

        enc_in = phi_z_channels + (self.a_dim if self.enable_smoothing else self.h_dim + self.phi_x_t_channels)
        self.enc = nn.Sequential(*block(nn.Conv2d(enc_in, 256, kernel_size=3, stride=2, padding=1), 256), Flatten())
        n_flat = 256 * h // 2 * w // 2
        self.enc_mean = _mlp(n_flat, z_dim, False)
        self.enc_std = _mlp(n_flat, z_dim, True)

        self.prior = nn.Sequential(*block(nn.Conv2d(h_dim + phi_z_channels, 256, kernel_size=3, stride=2, padding=1), 256),
                                   Flatten())
        self.prior_mean = _mlp(n_flat, z_dim, False)
        self.prior_std = _mlp(n_flat, z_dim, True)

        def up(cin, cout):
            return nn.ConvTranspose2d(cin, cout, kernel_size=4, stride=2, padding=1, output_padding=0)

        self.dec = nn.Sequential(
            *block(up(h_dim + phi_z_channels, 512), 512),
            *block(nn.Conv2d(512, 256, kernel_size=3, stride=1, padding=1), 256),
            *block(up(256, 64), 64),
            *block(nn.Conv2d(64, 64, kernel_size=3, stride=1, padding=1), 64),
            *block(up(64, 32), 32))

        self.z_0 = nn.Parameter(torch.zeros(self.batch_size, z_dim))
        self.z_0x = nn.Parameter(torch.zeros(self.batch_size, z_dim))
        self.h_0 = nn.Parameter(torch.zeros(self.batch_size, self.h_dim, h, w))
        self.c_0 = nn.Parameter(torch.zeros(self.batch_size, self.h_dim, h, w))
        self.a_0 = nn.Parameter(torch.zeros(self.batch_size, self.a_dim, h, w))
        self.ca_0 = nn.Parameter(torch.zeros(self.batch_size, self.a_dim, h, w))

        self.lstm_h = ConvLSTM(in_channels=self.phi_x_t_channels, hidden_channels=self.h_dim, kernel_size=[3, 3],
                               bias=True, peephole=True)
        # (hidden_channels = h_dim, as the reference has it: smoothing needs a_dim == h_dim there too)
        self.lstm_a = ConvLSTM(in_channels=self.phi_x_t_channels + self.h_dim, hidden_channels=self.h_dim,
                               kernel_size=[3, 3], bias=True, peephole=True)
        if self.loss_type == "mol":
            per, lik = (10, DiscretizedMixtureLogits) if cx > 1 else (3, DiscretizedMixtureLogits_1d)
            self.dec_mean = nn.Sequential(nn.Conv2d(32, self.n_logistics * per, kernel_size=3, stride=1, padding=1))
            self.likelihood = lik(self.n_logistics)
        else:
            self.variance = nn.Parameter(torch.ones([1]))
            if self.preprocess_range == "0.5":
                self.dec_mean = nn.Sequential(nn.Conv2d(32, cx, kernel_size=3, stride=1, padding=1), nn.Tanh())
            elif self.preprocess_range == "1.0":
                self.dec_mean = nn.Sequential(nn.Conv2d(32, cx, kernel_size=3, stride=1, padding=1), nn.Sigmoid())
        if self.loss_type == "gaussian" and not self.dequantize:
            raise ValueError("loss_type 'gaussian' needs --dequantize: the reference's loss reads the dequantisation "
                             "term it only computes with it")
        self.D = args.num_shots + 1
        self.overshot_w = args.overshot_w

    # ------------------------------------------------------------------------------------------------ pieces
    def get_inits(self):
        return self.h_0, self.c_0, self.z_0, self.z_0x, self.a_0, self.ca_0, 0, 0, 0

    def _dequant_draw(self, x, d):
        """(u, objective) of uniform_binning_correction, whose x_noise is x + u"""
        b, c, h, w = x.size()
        n_bins = 2 ** self.bits
        u = d.uniform(x.shape, 0, 1.0 / n_bins)
        objective = -np.log(n_bins) * (c * h * w) * torch.ones(b, device=x.device)
        return u, objective

    def uniform_binning_correction(self, x, draws=None):
        d = draws if isinstance(draws, _Draws) else _Draws(draws, x.device)
        u, objective = self._dequant_draw(x, d)
        return x + u, objective

    def _prior_dist(self, ht, z):
        prior_t = self.prior(torch.cat([ht, self.phi_z(z)], 1))
        return td.Normal(self.prior_mean(prior_t), self.prior_std(prior_t))

    def _decode(self, ht, z):
        return self.dec_mean(self.dec(torch.cat([ht, self.phi_z(z)], 1)))

    def _generate(self, dec_mean_t, d):
        """the frame a decoder output stands for: a draw from the mixture, or the output itself"""
        if self.loss_type != "mol":
            return dec_mean_t
        lik = self.likelihood(logits=dec_mean_t)
        if d.q is None:
            return lik.sample()
        N, _, H, W = dec_mean_t.shape
        u_mix = d.uniform((N, H, W, self.n_logistics), 1e-5, 1. - 1e-5)
        return lik.sample(u_mix, d.uniform((N, H, W, lik.channels), 1e-5, 1. - 1e-5))

    def _smoothing_states(self, store_ht, feature_of, t, aprev, caprev):
        store_at = [None] * (t - 1)
        for i in range(1, t):
            lstm_a_input = torch.cat([store_ht[t - i - 1], feature_of(t - i)], 1)
            _, aprev, caprev = self.lstm_a(lstm_a_input.unsqueeze(1), aprev, caprev)
            store_at[t - i - 1] = aprev
        return store_at

    # ------------------------------------------------------------------------------------------------ loss
    def loss(self, xt, draws=None):
        b, t, c, h, w = xt.shape
        d = _Draws(draws, xt.device)
        hprev, cprev, zprev, zprevx, aprev, caprev, _, kl_loss, nll_loss = self.get_inits()
        feats = [self.phi_x_t(xt[:, i]) for i in range(t)]
        store_ht = []
        for i in range(1, t):
            _, hprev, cprev = self.lstm_h(feats[i - 1].unsqueeze(1), hprev, cprev)
            store_ht.append(hprev)
        if self.enable_smoothing:
            store_at = self._smoothing_states(store_ht, lambda i: feats[i], t, aprev, caprev)

        store_ztx_mean, store_ztx_std, store_ztx, logits = [], [], [], []
        for i in range(1, t):
            ht = store_ht[i - 1]
            if self.enable_smoothing:
                enc_t = self.enc(torch.cat([store_at[i - 1], self.phi_z(zprevx)], 1))
            else:
                enc_t = self.enc(torch.cat([ht, self.phi_z(zprevx), self.phi_x_t(xt[:, i])], 1))
            enc_std_t = self.enc_std(enc_t)
            # (res_q: the prior is conditioned on zprevx, as in the reference)
            prior_dist = self._prior_dist(ht, zprevx if self.res_q else zprev)
            enc_mean_t = self.enc_mean(enc_t)
            if self.res_q:
                enc_mean_t = prior_dist.loc + enc_mean_t
            enc_dist = td.Normal(enc_mean_t, enc_std_t)
            z_tx = d.rsample(enc_dist)
            z_t = d.rsample(prior_dist)
            store_ztx_mean.append(enc_mean_t)
            store_ztx_std.append(enc_std_t)
            store_ztx.append(zprevx)   # (the reference stores z_tx and overwrites it with zprevx)
            dec_mean_t = self._decode(ht, z_tx)
            zprevx, zprev = z_tx, z_t
            if self.D == 1:
                kl_loss = kl_loss + self.beta * td.kl_divergence(enc_dist, prior_dist)
            x_i = xt[:, i]
            if self.loss_type == "bernoulli":
                nll_loss = nll_loss - batch_reduce(td.Bernoulli(probs=dec_mean_t).log_prob(x_i))
            elif self.loss_type == "gaussian":
                x, nll_unif = self.uniform_binning_correction(x_i, d)
                scale = nn.functional.softplus(self.variance) * torch.ones_like(dec_mean_t)
                nll_loss = nll_loss - batch_reduce(td.Normal(dec_mean_t, scale).log_prob(x)) - nll_unif
            elif self.loss_type == "mse":
                nll_loss = nll_loss + batch_reduce(self.mse_criterion(dec_mean_t, x_i))
            elif self.loss_type == "mol":
                logits.append(dec_mean_t)
            else:
                raise ValueError("undefined loss %r" % (self.loss_type,))
        if self.loss_type == "mol":
            from rfn_hip import ops as K
            x_all = xt[:, 1:].transpose(0, 1).reshape((t - 1) * b, c, h, w)   # step-major, like the collected logits
            nll_steps = K.mol_nll(x_all.detach(), torch.cat(logits, 0), reduce="frame").view(t - 1, b)
            for s in range(t - 1):   # fixed order
                nll_loss = nll_loss + nll_steps[s]

        if self.D > 1:
            kl_loss = 0
            for i in range(1, t):
                overshot_loss = 0
                idt = i - 1
                zprev = store_ztx[idt]
                D = min(t - i, self.D)
                for k in range(D):
                    prior_dist = self._prior_dist(store_ht[idt + k], zprev)
                    zprev = d.rsample(prior_dist)
                    enc_mean, enc_std = store_ztx_mean[idt + k], store_ztx_std[idt + k]
                    if k > 0:   # the encoder is not to conform to the prior beyond the first shot
                        enc_mean, enc_std = enc_mean.detach(), enc_std.detach()
                    overshot_loss = overshot_loss + self.overshot_w * td.kl_divergence(td.Normal(enc_mean, enc_std),
                                                                                        prior_dist)
                kl_loss = kl_loss + 1 / D * overshot_loss * self.beta
        d.done()
        return batch_reduce(kl_loss).mean(), nll_loss.mean()

    # ------------------------------------------------------------------------------------------------ generation
    # predict ends in `.cpu()`, as the reference's does; `_predict_device` returns the same tensors where they were
    # computed (the Evaluator's FVD path embeds them without a host round trip).
    def predict(self, xt, n_predictions, n_conditions, draws=None):
        true_x, predictions = self._predict_device(xt, n_predictions, n_conditions, draws)
        return true_x.cpu(), predictions.cpu()

    def _predict_device(self, xt, n_predictions, n_conditions, draws=None):
        b, t, c, h, w = xt.shape
        assert n_conditions <= t, "n_conditions > t, number of conditioned frames is greater than number of frames"
        d = _Draws(draws, xt.device)
        hprev, cprev, zprev, zprevx, aprev, caprev, _, _, _ = self.get_inits()
        true_x = [xt[:, 0].detach()]
        store_ht = []
        for i in range(1, n_conditions):
            _, hprev, cprev = self.lstm_h(self.phi_x_t(xt[:, i - 1]).unsqueeze(1), hprev, cprev)
            store_ht.append(hprev)
        for i in range(1, n_conditions):
            zprev = d.rsample(self._prior_dist(store_ht[i - 1], zprev))
            true_x.append(xt[:, i].detach())
        prediction = xt[:, n_conditions - 1]
        predictions = []
        for i in range(n_predictions):
            _, ht, ct = self.lstm_h(self.phi_x_t(prediction).unsqueeze(1), hprev, cprev)
            z_t = d.rsample(self._prior_dist(ht, zprev))
            prediction = self._generate(self._decode(ht, z_t), d)
            zprev, hprev, cprev = z_t, ht, ct
            predictions.append(prediction.detach())
        d.done()
        return torch.stack(true_x, 0), torch.stack(predictions, 0)

    def predict_draws(self, xt, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0):
        """`predict` for n_draws independent draws of every sequence in one pass, with addressed noise (the counterpart
        of RFN.predict_draws, without temperatures): returns (true_x, predictions), predictions [n_predictions, n_draws,
        B, C, H, W] on the CPU (`_predict_draws_device`: the same on the device).  phi_x_t and lstm_h run once over the
        conditioning frames of the B sequences; from the first prior sample on everything runs on n_draws*B rows,
        draw-major (row r*B + b: draw first_draw + r of sequence first_seq + b); the [batch_size, ...] initial states
        are repeated.
        Noise: conditioning step i (1 .. n_conditions-1) uses t = i, rfn_hip.ops.keyed_normal slot 0 for the prior eps.
        Generated frame i uses t = n_conditions + i: slot 0 for the prior eps and, for loss_type "mol", the mixture
        sampler's addressed uniforms at that step (rfn_hip.ops.mol_sample_keyed).  The other loss
        types have no sampler noise.  A frame therefore depends on (seed, sequence id, draw id) and the data alone: not
        on B, on n_draws, on how the draws are split into calls, or on torch's generator, which is left untouched.
        Eval mode only: batch statistics would couple the draws."""
        true_x, predictions = self._predict_draws_device(xt, n_predictions, n_conditions, n_draws, seed, first_seq,
                                                         first_draw)
        return true_x.cpu(), predictions.cpu()

    def _predict_draws_device(self, xt, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0):
        from rfn_hip import ops as K
        assert len(xt.shape) == 5, "xt must be [bs, t, c, h, w]"
        if self.training:
            raise RuntimeError("SRNN.predict_draws needs eval mode: in training mode the batch statistics of the "
                               "normalisation layers would couple the draws (call model.eval() first)")
        b, t, c, h, w = xt.shape
        assert n_conditions <= t, "n_conditions > t, number of conditioned frames is greater than number of frames"
        P, B = int(n_draws), int(b)
        if P < 1:
            raise ValueError("SRNN.predict_draws: n_draws must be at least 1, got %d" % P)

        def rep(v):   # draw-major: row r*B + b is sequence b
            return v.repeat((P,) + (1,) * (v.dim() - 1))

        def prior_sample(ht, zprev, step):
            dist = self._prior_dist(ht, zprev)
            eps, = K.keyed_normal([tuple(dist.loc.shape[1:])], B, P, seed, step, first_seq, first_draw, device=xt.device)
            return dist.loc + dist.scale * eps

        with torch.no_grad():
            hprev, cprev, zprev, _, _, _, _, _, _ = self.get_inits()
            store_ht = []
            for i in range(1, n_conditions):
                _, hprev, cprev = self.lstm_h(self.phi_x_t(xt[:, i - 1]).unsqueeze(1), hprev, cprev)
                store_ht.append(hprev)
            zprev = rep(zprev)
            for i in range(1, n_conditions):
                zprev = prior_sample(rep(store_ht[i - 1]), zprev, i)
            true_x = xt[:, :n_conditions].transpose(0, 1).detach().clone()
            prediction, hprev, cprev = rep(xt[:, n_conditions - 1]), rep(hprev), rep(cprev)
            frames = []
            for i in range(n_predictions):
                step = n_conditions + i
                _, ht, ct = self.lstm_h(self.phi_x_t(prediction).unsqueeze(1), hprev, cprev)
                z_t = prior_sample(ht, zprev, step)
                prediction = self._decode(ht, z_t)
                if self.loss_type == "mol":
                    prediction = self.likelihood(logits=prediction).sample_keyed(B, seed, step, first_seq, first_draw)
                zprev, hprev, cprev = z_t, ht, ct
                frames.append(prediction.detach())
            if frames:
                predictions = torch.stack(frames, 0).view(n_predictions, P, B, c, h, w)
            else:
                predictions = torch.zeros((0, P, B, c, h, w), device=xt.device)
        return true_x, predictions

    # ------------------------------------------------------------------------------------------------ evaluation
    def _frame_nll(self, dec_mean_t, x_i, x_noise=None, nll_unif=None):
        """-log p(x_i | decoder output) per row, as `loss` computes it per step"""
        if self.loss_type == "bernoulli":
            return -batch_reduce(td.Bernoulli(probs=dec_mean_t).log_prob(x_i))
        if self.loss_type == "gaussian":
            scale = nn.functional.softplus(self.variance) * torch.ones_like(dec_mean_t)
            return -batch_reduce(td.Normal(dec_mean_t, scale).log_prob(x_noise)) - nll_unif
        if self.loss_type == "mse":
            return batch_reduce(self.mse_criterion(dec_mean_t, x_i))
        if self.loss_type == "mol":
            from rfn_hip import ops as K
            return K.mol_nll(x_i.detach(), dec_mean_t, reduce="frame")
        raise ValueError("undefined loss %r" % (self.loss_type,))

    def _frame_nll_rows(self, dec_mean_t, x_i, u=None, nll_unif=None, scale=None):
        """_frame_nll of the R = K*B rows (k*B + b) of a deferred decoder call under the B frames x_i; u [R, ...]: the
        dequantisation uniforms of "gaussian", one draw per row, nll_unif [R] their objective.  Without a gradient to
        keep, "bernoulli", "gaussian" and "mse" are one rfn_hip.ops.pixel_loglik launch that reads x_i in place (scale: a
        callable giving softplus(variance) as a Python float); otherwise, and with RFN_PIXEL_LOGLIK=0, the frames are
        repeated K times and the torch chain of _frame_nll runs ("mol" has its own kernel there)."""
        from rfn_hip import ops
        gauss = self.loss_type == "gaussian"
        if self.loss_type in ops.PIXEL_LOGLIK_MODES and ops.pixel_loglik_route(
                dec_mean_t, x_i, u, self.variance if gauss else None) == "kernel":
            if gauss:
                return -ops.pixel_loglik(dec_mean_t, x_i, "gaussian", scale=scale(), noise=u) - nll_unif
            return -ops.pixel_loglik(dec_mean_t, x_i, self.loss_type)
        x_rep = x_i.repeat(dec_mean_t.shape[0] // x_i.shape[0], 1, 1, 1)
        return self._frame_nll(dec_mean_t, x_rep, x_rep + u if gauss else None, nll_unif)

    def elbo_importance_weighting(self, xt, K, draws=None, defer_decoder=None):
        """The importance-weighted bound the reference reports as its baselines' bits/dim (SRNN/SRNN.py:482-579 of the
        reference), as that code behaves: zprevx and zprev chain through the K inner samples and on into the next time
        step; with res_q the prior is taken on zprevx; without smoothing phi_x_t(x_i) belongs to every inner sample; per
        inner sample the draws are the encoder eps, the prior eps and, for "gaussian", the dequantisation uniforms.
        Returns sum_t -mean_b(logsumexp_k(log p(x|z_k) + log p(z_k) - log q(z_k|x)) - log K).  The K x B tables stay on
        the device.
        The decoder does not feed the recurrence.  In eval mode (defer_decoder None) dec, dec_mean and the likelihood of
        a time step therefore run ONCE over the K*B rows collected in the k loop (one mol_nll launch per step in place
        of K), and the deterministic phi_x_t(x_i) is taken from the pass over the frames; in training mode every inner
        sample makes its own calls, because the batch statistics of the norm layers are per call in the reference.
        defer_decoder = False / True forces either form of the decoder.  The deferred likelihood is _frame_nll_rows:
        for the non-"mol" losses one pixel_loglik launch per time step when no gradient is kept, with softplus(variance)
        of "gaussian" read to the host once per call."""
        b, t, c, h, w = xt.shape
        K = int(K)
        if K < 1:
            raise ValueError("SRNN.elbo_importance_weighting: K must be at least 1, got %d" % K)
        defer = (not self.training) if defer_decoder is None else bool(defer_decoder)
        d = _Draws(draws, xt.device)
        hprev, cprev, zprev, zprevx, aprev, caprev, _, _, _ = self.get_inits()
        feats = [self.phi_x_t(xt[:, i]) for i in range(t)]
        store_ht = []
        for i in range(1, t):
            _, hprev, cprev = self.lstm_h(feats[i - 1].unsqueeze(1), hprev, cprev)
            store_ht.append(hprev)
        if self.enable_smoothing:
            store_at = self._smoothing_states(store_ht, lambda i: feats[i], t, aprev, caprev)
        log_k = float(np.log(K))
        host_scale = []

        def scale():   # one device-to-host read per call, and only when a kernel launch needs it
            if not host_scale:
                host_scale.append(float(nn.functional.softplus(self.variance.detach())))
            return host_scale[0]
        loss = 0
        for i in range(1, t):
            ht, x_i = store_ht[i - 1], xt[:, i]
            logpzs, logqzxs, nlls, ztxs, noisy, unifs = [], [], [], [], [], []
            for k in range(K):
                if self.enable_smoothing:
                    enc_t = self.enc(torch.cat([store_at[i - 1], self.phi_z(zprevx)], 1))
                else:
                    feat_i = self.phi_x_t(x_i) if self.training else feats[i]
                    enc_t = self.enc(torch.cat([ht, self.phi_z(zprevx), feat_i], 1))
                enc_std_t = self.enc_std(enc_t)
                prior_dist = self._prior_dist(ht, zprevx if self.res_q else zprev)
                enc_mean_t = self.enc_mean(enc_t)
                if self.res_q:
                    enc_mean_t = prior_dist.loc + enc_mean_t
                enc_dist = td.Normal(enc_mean_t, enc_std_t)
                z_tx = d.rsample(enc_dist)
                z_t = d.rsample(prior_dist)
                u = nll_unif = None
                if self.loss_type == "gaussian":
                    u, nll_unif = self._dequant_draw(x_i, d)
                if defer:
                    ztxs.append(z_tx)
                    noisy.append(u)
                    unifs.append(nll_unif)
                else:
                    nlls.append(self._frame_nll(self._decode(ht, z_tx), x_i, None if u is None else x_i + u, nll_unif))
                logpzs.append(prior_dist.log_prob(z_t).sum([-1]))
                logqzxs.append(enc_dist.log_prob(z_tx).sum([-1]))
                zprevx, zprev = z_tx, z_t
            if defer:   # rows k*B + b
                gauss = self.loss_type == "gaussian"
                nll = self._frame_nll_rows(self._decode(ht.repeat(K, 1, 1, 1), torch.cat(ztxs, 0)), x_i,
                                           torch.cat(noisy, 0) if gauss else None, torch.cat(unifs, 0) if gauss else None,
                                           scale)
                nll = nll.view(K, b)
            else:
                nll = torch.stack(nlls, 0)
            # (the reference adds its "lpx_Gz_obs", which is the NEGATIVE log-likelihood, as it stands: kept)
            table = nll + torch.stack(logpzs, 0) - torch.stack(logqzxs, 0)
            loss = loss - torch.mean(torch.logsumexp(table, 0) - log_k)
        d.done()
        return loss

    def reconstruct(self, xt, draws=None):
        b, t, c, h, w = xt.shape
        d = _Draws(draws, xt.device)
        hprev, cprev, zprev, zprevx, aprev, caprev, _, _, _ = self.get_inits()
        store_ht = []
        for i in range(1, t):
            _, hprev, cprev = self.lstm_h(self.phi_x_t(xt[:, i - 1]).unsqueeze(1), hprev, cprev)
            store_ht.append(hprev)
        if self.enable_smoothing:
            store_at = self._smoothing_states(store_ht, lambda i: self.phi_x_t(xt[:, i]), t, aprev, caprev)
        recons = [torch.zeros_like(xt[:, 0])]   # (frame 0 is never reconstructed)
        for i in range(1, t):
            ht = store_ht[i - 1]
            if self.enable_smoothing:
                enc_t = self.enc(torch.cat([store_at[i - 1], self.phi_z(zprevx)], 1))
            else:
                enc_t = self.enc(torch.cat([ht, self.phi_z(zprevx), self.phi_x_t(xt[:, i])], 1))
            enc_mean_t = self.enc_mean(enc_t)
            if self.res_q:
                enc_mean_t = self._prior_dist(ht, zprevx).loc + enc_mean_t
            z_tx = d.rsample(td.Normal(enc_mean_t, self.enc_std(enc_t)))
            recons.append(self._generate(self._decode(ht, z_tx), d).detach())
            zprevx = z_tx
        d.done()
        return torch.stack(recons, 0).cpu()

    def sample(self, xt, n_samples, draws=None):
        d = _Draws(draws, xt.device)
        hprev, cprev, zprev, zprevx, _, _, _, _, _ = self.get_inits()
        condition = xt[:, 0]
        samples = []
        for i in range(n_samples):
            _, ht, ct = self.lstm_h(self.phi_x_t(condition).unsqueeze(1), hprev, cprev)
            z_t = d.rsample(self._prior_dist(ht, zprev))
            condition = self._generate(self._decode(ht, z_t), d)
            zprev, hprev, cprev = z_t, ht, ct
            samples.append(condition.detach())
        d.done()
        return torch.stack(samples, 0).cpu()
