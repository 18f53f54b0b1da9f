"""VRNN baseline — host mirror of the reference's VRNN/VRNN.py: same constructor arguments read from `args`, same
state_dict keys and shapes, same layer structure, and the reference's behaviour where it differs from its comments:
phi_x_t runs twice per step of `loss` (on x_i and on x_{i-1}, as separate calls: batch statistics are per call and the
running buffers move twice), phi_z runs on zxprev for the LSTM and on zx_t for the decoder, z_0 is never used by `loss`,
and generation feeds phi_z of the PRIOR sample into the LSTM.

The time loop is strictly serial (h_t depends on z_{t-1}).  On the package's kernels: the ConvLSTM (Utils.ConvLSTM), the
mixture of discretized logistics (the logits of all T-1 frames go through rfn_hip.ops.mol_nll in ONE launch after the
loop, as in SRNN.loss) and, between the recurrent cell and the decoder, the step's diagonal Gaussians: the four MLP
outputs become samples, the KL row sums and the log-densities in one launch each way (rfn_hip.ops.gauss_heads, fed by
enc_std[:-1] and prior_std[:-1]: the Softplus modules stay in place so the state_dict keys do not move, the kernel
applies them).  Strided convolutions, ConvTranspose2d, Linear and the norm layers are PyTorch modules.

Every method that draws takes `draws=None`, as SRNN's do (SRNN/SRNN.py: the recorded draws in the reference's order).
`predict_draws`, `_predict_device` and `elbo_importance_weighting` are what an evaluation driver calls; DESIGN.md
section 21."""
import numpy as np
import torch
import torch.distributions as td
import torch.nn as nn

from SRNN.SRNN import _Draws, _mlp
from Utils import ConvLSTM, NormLayer
from Utils import DiscretizedMixtureLogits, DiscretizedMixtureLogits_1d
from Utils import Flatten, UnFlatten, batch_reduce, get_layer_size


class VRNN(nn.Module):
    def __init__(self, args):
        super().__init__()
        norm_type = args.norm_type
        self.batch_size = args.batch_size
        self.u_dim = args.condition_dim
        self.x_dim = args.x_dim
        self.h_dim, self.z_dim = h_dim, z_dim = args.h_dim, args.z_dim
        self.loss_type = args.loss_type
        self.beta = 1
        bu, cu, hu, wu = self.u_dim
        bx, cx, hx, wx = self.x_dim
        self.mse_criterion = nn.MSELoss(reduction="none")
        self.bits = args.n_bits
        self.dequantize = args.dequantize
        self.preprocess_range = args.preprocess_range
        self.n_logistics = args.n_logistics

        def block(conv, c):
            return [conv, NormLayer(c, norm_type), nn.ReLU()]

        phi_x_t_channels = 256
        self.phi_x_t = nn.Sequential(
            *block(nn.Conv2d(cx, 64, kernel_size=3, stride=2, padding=1), 64),
            *block(nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1), 128),
            *block(nn.Conv2d(128, 256, kernel_size=3, stride=2, padding=1), 256),
            *block(nn.Conv2d(256, phi_x_t_channels, kernel_size=3, stride=1, padding=1), phi_x_t_channels))
        h, w = get_layer_size([hu, wu], kernels=[3, 3, 3], paddings=[1, 1, 1], strides=[2, 2, 2], dilations=[1, 1, 1])
        self.h, self.w = h, w

        phi_z_channels = 128
        self.phi_z = nn.Sequential(
            nn.Linear(z_dim, phi_z_channels * h * w), nn.ReLU(),
            nn.Linear(phi_z_channels * h * w, phi_z_channels * h * w), nn.ReLU(),
            UnFlatten(phi_z_channels, h, w),
            *block(nn.Conv2d(phi_z_channels, phi_z_channels, kernel_size=3, stride=1, padding=1), phi_z_channels))

        self.enc = nn.Sequential(*block(nn.Conv2d(phi_x_t_channels + h_dim, 256, kernel_size=3, stride=2, padding=1), 256),
                                 Flatten())
        n_flat = 256 * h // 2 * w // 2
        self.enc_mean = _mlp(n_flat, z_dim, False)
        self.enc_std = _mlp(n_flat, z_dim, True)

        self.prior = nn.Sequential(*block(nn.Conv2d(h_dim, 256, kernel_size=3, stride=2, padding=1), 256), Flatten())
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

        self.z_0 = nn.Parameter(torch.zeros(self.batch_size, z_dim))
        self.z_0x = nn.Parameter(torch.zeros(self.batch_size, z_dim))
        self.h_0 = nn.Parameter(torch.zeros(self.batch_size, self.h_dim, h, w))
        self.c_0 = nn.Parameter(torch.zeros(self.batch_size, self.h_dim, h, w))

        self.lstm = ConvLSTM(in_channels=phi_x_t_channels + phi_z_channels, hidden_channels=self.h_dim,
                             kernel_size=[3, 3], bias=True, peephole=True)

    # ------------------------------------------------------------------------------------------------ pieces
    def get_inits(self):
        return self.h_0, self.c_0, self.z_0, self.z_0x, 0, 0, 0

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

    def _step(self, ut, z_in, hprev, cprev):
        """the recurrent cell on (phi_x_t of the previous frame, phi_z of the previous latent)"""
        _, ht, ct = self.lstm(torch.cat([ut, self.phi_z(z_in)], 1).unsqueeze(1), hprev, cprev)
        return ht, ct

    def _prior_heads(self, ht):
        prior_t = self.prior(ht)
        return self.prior_mean(prior_t), self.prior_std[:-1](prior_t)

    def _enc_heads(self, ht, xt_features):
        enc_t = self.enc(torch.cat([ht, xt_features], 1))
        return self.enc_mean(enc_t), self.enc_std[:-1](enc_t)

    @staticmethod
    def _sample_one(loc, raw, eps):
        """loc + softplus(raw) * eps of ONE Gaussian: the one-distribution form of the heads kernel"""
        from rfn_hip import ops as K
        return K.gauss_heads(None, None, loc, raw, None, eps, want=("z_p",))[0]

    def _prior_sample(self, ht, eps):
        return self._sample_one(*self._prior_heads(ht), eps)

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

    # ------------------------------------------------------------------------------------------------ loss
    def loss(self, xt, draws=None):
        from rfn_hip import ops as K
        b, t, c, h, w = xt.shape
        d = _Draws(draws, xt.device)
        hprev, cprev, _, zxprev, _, kl_loss, nll_loss = self.get_inits()
        logits = []
        for i in range(1, t):
            x_i = xt[:, i]
            xt_features = self.phi_x_t(x_i)          # (two separate calls, as in the reference: VRNN.py:197-198)
            ut = self.phi_x_t(xt[:, i - 1])
            ht, ct = self._step(ut, zxprev, hprev, cprev)
            p_loc, p_raw = self._prior_heads(ht)
            q_loc, q_raw = self._enc_heads(ht, xt_features)
            zx_t, kl_t = K.gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=d.normal(q_loc.shape), want=("z_q", "kl"))
            dec_mean_t = self._decode(ht, zx_t)
            zxprev, hprev, cprev = zx_t, ht, ct
            kl_loss = kl_loss + kl_t                  # row sums, added over time in step order
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
            x_all = xt[:, 1:].transpose(0, 1).reshape((t - 1) * b, c, h, w)   # step-major, like the collected logits
            nll_steps = K.mol_nll(x_all.detach(), torch.cat(logits, 0), reduce="frame").view(t - 1, b)
            for s in range(t - 1):   # fixed order
                nll_loss = nll_loss + nll_steps[s]
        d.done()
        return batch_reduce(kl_loss).mean(), nll_loss.mean()

    # ------------------------------------------------------------------------------------------------ generation
    # predict ends in `.cpu()`, as the reference's does; `_predict_device` returns the same tensors where they were
    # computed.
    def predict(self, xt, n_predictions, n_conditions, draws=None):
        true_x, predictions = self._predict_device(xt, n_predictions, n_conditions, draws)
        return true_x.cpu(), predictions.cpu()

    def _predict_device(self, xt, n_predictions, n_conditions, draws=None):
        from rfn_hip import ops as K
        b, t, c, h, w = xt.shape
        assert n_conditions <= t, "n_conditions > t, number of conditioned frames is greater than number of frames"
        d = _Draws(draws, xt.device)
        hprev, cprev, zprev, zxprev, _, _, _ = self.get_inits()
        true_x = [xt[:, 0].detach()]
        for i in range(1, n_conditions):
            xt_features = self.phi_x_t(xt[:, i])
            ut = self.phi_x_t(xt[:, i - 1])
            ht, ct = self._step(ut, zxprev, hprev, cprev)
            p_loc, p_raw = self._prior_heads(ht)
            eps_p = d.normal(p_loc.shape)            # (the prior is sampled first: VRNN.py:268, then :273)
            q_loc, q_raw = self._enc_heads(ht, xt_features)
            zx_t, z_t = K.gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=d.normal(q_loc.shape), eps_p=eps_p,
                                      want=("z_q", "z_p"))
            zprev, zxprev, hprev, cprev = z_t, zx_t, ht, ct
            true_x.append(xt[:, i].detach())
        prediction = xt[:, n_conditions - 1]
        predictions = []
        for i in range(n_predictions):
            ht, ct = self._step(self.phi_x_t(prediction), zprev, hprev, cprev)   # (phi_z of the PRIOR sample)
            z_t = self._prior_sample(ht, d.normal((ht.shape[0], self.z_dim)))
            prediction = self._generate(self._decode(ht, z_t), d)
            zprev, hprev, cprev = z_t, ht, ct
            predictions.append(prediction.detach())
        d.done()
        return torch.stack(true_x, 0), torch.stack(predictions, 0)

    def predict_draws(self, xt, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0):
        """`predict` for n_draws independent draws of every sequence in one pass, with addressed noise (the counterpart
        of SRNN.predict_draws): returns (true_x, predictions), predictions [n_predictions, n_draws, B, C, H, W] on the
        CPU (`_predict_draws_device`: the same on the device).  phi_x_t of the conditioning frames runs once on the B
        sequences; everything after it runs on n_draws*B rows, draw-major (row r*B + b: draw first_draw + r of sequence
        first_seq + b), because the recurrent state depends on the encoder sample; the [batch_size, ...] initial states
        are repeated.
        Noise: conditioning step i (1 .. n_conditions-1) uses t = i, rfn_hip.ops.keyed_normal slot 0 for the prior eps
        and slot 1 for the encoder eps.  Generated frame i uses t = n_conditions + i: slot 0 for the prior eps and, for
        loss_type "mol", the mixture sampler's addressed uniforms at that step (rfn_hip.ops.mol_sample_keyed).  A frame
        therefore depends on (seed, sequence id, draw id) and the data alone: not on B, on n_draws, on how the draws
        are split into calls, or on torch's generator, which is left untouched.
        Eval mode only: batch statistics would couple the draws."""
        true_x, predictions = self._predict_draws_device(xt, n_predictions, n_conditions, n_draws, seed, first_seq,
                                                         first_draw)
        return true_x.cpu(), predictions.cpu()

    def _predict_draws_device(self, xt, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0):
        from rfn_hip import ops as K
        assert len(xt.shape) == 5, "xt must be [bs, t, c, h, w]"
        if self.training:
            raise RuntimeError("VRNN.predict_draws needs eval mode: in training mode the batch statistics of the "
                               "normalisation layers would couple the draws (call model.eval() first)")
        b, t, c, h, w = xt.shape
        assert n_conditions <= t, "n_conditions > t, number of conditioned frames is greater than number of frames"
        P, B = int(n_draws), int(b)
        if P < 1:
            raise ValueError("VRNN.predict_draws: n_draws must be at least 1, got %d" % P)

        def rep(v):   # draw-major: row r*B + b is sequence b
            return v.repeat((P,) + (1,) * (v.dim() - 1))

        def eps(step, slots):
            return K.keyed_normal([(self.z_dim,)] * slots, B, P, seed, step, first_seq, first_draw, device=xt.device)

        with torch.no_grad():
            hprev, cprev, zprev, zxprev, _, _, _ = self.get_inits()
            feats = [rep(self.phi_x_t(xt[:, i])) for i in range(n_conditions)]   # (eval mode: one call per frame)
            hprev, cprev, zprev, zxprev = rep(hprev), rep(cprev), rep(zprev), rep(zxprev)
            for i in range(1, n_conditions):
                ht, ct = self._step(feats[i - 1], zxprev, hprev, cprev)
                p_loc, p_raw = self._prior_heads(ht)
                q_loc, q_raw = self._enc_heads(ht, feats[i])
                eps_p, eps_q = eps(i, 2)
                zx_t, z_t = K.gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=eps_q, eps_p=eps_p, want=("z_q", "z_p"))
                zprev, zxprev, hprev, cprev = z_t, zx_t, ht, ct
            true_x = xt[:, :n_conditions].transpose(0, 1).detach().clone()
            ut = feats[n_conditions - 1]
            frames = []
            for i in range(n_predictions):
                step = n_conditions + i
                ht, ct = self._step(ut, zprev, hprev, cprev)
                z_t = self._prior_sample(ht, eps(step, 1)[0])
                prediction = self._decode(ht, z_t)
                if self.loss_type == "mol":
                    prediction = self.likelihood(logits=prediction).sample_keyed(B, seed, step, first_seq, first_draw)
                zprev, hprev, cprev = z_t, ht, ct
                frames.append(prediction.detach())
                if i + 1 < n_predictions:
                    ut = self.phi_x_t(prediction)
            if frames:
                predictions = torch.stack(frames, 0).view(n_predictions, P, B, c, h, w)
            else:
                predictions = torch.zeros((0, P, B, c, h, w), device=xt.device)
        return true_x, predictions

    def reconstruct(self, xt, draws=None):
        b, t, c, h, w = xt.shape
        d = _Draws(draws, xt.device)
        hprev, cprev, _, zxprev, _, _, _ = self.get_inits()
        recons = [torch.zeros_like(xt[:, 0])]   # (frame 0 is never reconstructed)
        for i in range(1, t):
            ut = self.phi_x_t(xt[:, i - 1])
            xt_features = self.phi_x_t(xt[:, i])
            ht, ct = self._step(ut, zxprev, hprev, cprev)
            q_loc, q_raw = self._enc_heads(ht, xt_features)   # (no prior here, as in the reference)
            zx_t = self._sample_one(q_loc, q_raw, d.normal(q_loc.shape))
            recons.append(self._generate(self._decode(ht, zx_t), d).detach())
            zxprev, hprev, cprev = zx_t, ht, ct
        d.done()
        return torch.stack(recons, 0).cpu()

    def sample(self, xt, n_samples, draws=None):
        d = _Draws(draws, xt.device)
        ht, ct, zprev, _, _, _, _ = self.get_inits()
        ut = self.phi_x_t(xt[:, 0])
        samples = []
        for i in range(n_samples):
            ht, ct = self._step(ut, zprev, ht, ct)
            z_t = self._prior_sample(ht, d.normal((ht.shape[0], self.z_dim)))
            frame = self._generate(self._decode(ht, z_t), d)
            ut = self.phi_x_t(frame)
            zprev = z_t
            samples.append(frame.detach())
        d.done()
        return torch.stack(samples, 0).cpu()

    # ------------------------------------------------------------------------------------------------ evaluation
    def _lpx(self, dec_mean_t, x_i, x_noise=None, nll_unif=None):
        """the reference's `lpx_Gz_obs` per row (VRNN.py:400-415), with its sign per loss type AS IT STANDS there: the
        log-likelihood for "bernoulli", "gaussian" and "mse", the NEGATIVE log-likelihood for "mol" """
        if self.loss_type == "bernoulli":
            return batch_reduce(td.Bernoulli(probs=dec_mean_t).log_prob(x_i))
        if self.loss_type == "gaussian":
            scale = nn.functional.softplus(self.variance) * torch.ones_like(dec_mean_t)
            return batch_reduce(td.Normal(dec_mean_t, scale).log_prob(x_noise)) - nll_unif
        if self.loss_type == "mse":
            return -batch_reduce(self.mse_criterion(dec_mean_t, x_i))
        if self.loss_type == "mol":
            from rfn_hip import ops as K
            return K.mol_nll(x_i.detach(), dec_mean_t, reduce="frame")
        raise ValueError("undefined loss %r" % (self.loss_type,))

    def _lpx_rows(self, dec_mean_t, x_i, u=None, nll_unif=None, scale=None):
        """_lpx of the R = K*B rows (k*B + b) of a deferred decoder call under the B frames x_i; u [R, ...]: the
        dequantisation uniforms of "gaussian", one draw per row, nll_unif [R] their objective.  Without a gradient to
        keep, "bernoulli", "gaussian" and "mse" are one rfn_hip.ops.pixel_loglik launch that reads x_i in place (scale: a
        callable giving softplus(variance) as a Python float); otherwise, and with RFN_PIXEL_LOGLIK=0, the frames are
        repeated K times and the torch chain of _lpx runs."""
        from rfn_hip import ops
        gauss = self.loss_type == "gaussian"
        if self.loss_type in ops.PIXEL_LOGLIK_MODES and ops.pixel_loglik_route(
                dec_mean_t, x_i, u, self.variance if gauss else None) == "kernel":
            if gauss:
                return ops.pixel_loglik(dec_mean_t, x_i, "gaussian", scale=scale(), noise=u) - nll_unif
            return ops.pixel_loglik(dec_mean_t, x_i, self.loss_type)
        x_rep = x_i.repeat(dec_mean_t.shape[0] // x_i.shape[0], 1, 1, 1)
        return self._lpx(dec_mean_t, x_rep, x_rep + u if gauss else None, nll_unif)

    def elbo_importance_weighting(self, xt, K, draws=None, defer_decoder=None):
        """The importance-weighted bound the reference reports as its baselines' bits/dim (VRNN/VRNN.py:366-428 of the
        reference), as that code behaves: hprev, cprev and zxprev chain through the K inner samples and on into the next
        time step (the LSTM advances K times per frame); per inner sample the draws are the encoder eps, the prior eps
        and, for "gaussian", the dequantisation uniforms; log p(z) is the prior's density at its OWN sample z_t.
        Returns sum_t -mean_b(logsumexp_k(lpx + log p(z_k) - log q(zx_k|x)) - log K).  The K x B tables stay on the
        device; the step's Gaussians are one gauss_heads launch per inner sample.
        The decoder does not feed the recurrence.  In eval mode (defer_decoder None) dec, dec_mean and the likelihood of
        a time step therefore run ONCE over the K*B rows collected in the k loop, and phi_x_t of the two frames runs once
        per time step as in the reference; in training mode every inner sample makes its own decoder call, because the
        batch statistics of the norm layers are per call in the reference.  defer_decoder = False / True forces either
        form of the decoder.  The deferred likelihood is _lpx_rows: one pixel_loglik launch per time step when no
        gradient is kept, with softplus(variance) of "gaussian" read to the host once per call."""
        from rfn_hip import ops
        b, t, c, h, w = xt.shape
        K = int(K)
        if K < 1:
            raise ValueError("VRNN.elbo_importance_weighting: K must be at least 1, got %d" % K)
        defer = (not self.training) if defer_decoder is None else bool(defer_decoder)
        d = _Draws(draws, xt.device)
        hprev, cprev, _, zxprev, _, _, _ = self.get_inits()
        log_k = float(np.log(K))
        host_scale = []

        def scale():   # one device-to-host read per call, and only when a kernel launch needs it
            if not host_scale:
                host_scale.append(float(nn.functional.softplus(self.variance.detach())))
            return host_scale[0]
        loss = 0
        for i in range(1, t):
            x_i = xt[:, i]
            xt_features = self.phi_x_t(x_i)
            ut = self.phi_x_t(xt[:, i - 1])
            logpzs, logqzxs, lpxs, hts, zxs, noisy, unifs = [], [], [], [], [], [], []
            for k in range(K):
                ht, ct = self._step(ut, zxprev, hprev, cprev)
                p_loc, p_raw = self._prior_heads(ht)
                q_loc, q_raw = self._enc_heads(ht, xt_features)
                eps_q = d.normal(q_loc.shape)
                eps_p = d.normal(p_loc.shape)
                zx_t, logq, logp = ops.gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=eps_q, eps_p=eps_p,
                                                   want=("z_q", "logq", "logp"))
                u = nll_unif = None
                if self.loss_type == "gaussian":
                    u, nll_unif = self._dequant_draw(x_i, d)
                if defer:
                    hts.append(ht)
                    zxs.append(zx_t)
                    noisy.append(u)
                    unifs.append(nll_unif)
                else:
                    lpxs.append(self._lpx(self._decode(ht, zx_t), x_i, None if u is None else x_i + u, nll_unif))
                logpzs.append(logp)
                logqzxs.append(logq)
                zxprev, hprev, cprev = zx_t, ht, ct
            if defer:   # rows k*B + b
                gauss = self.loss_type == "gaussian"
                lpx = self._lpx_rows(self._decode(torch.cat(hts, 0), torch.cat(zxs, 0)), x_i,
                                     torch.cat(noisy, 0) if gauss else None, torch.cat(unifs, 0) if gauss else None, scale)
                lpx = lpx.view(K, b)
            else:
                lpx = torch.stack(lpxs, 0)
            table = lpx + torch.stack(logpzs, 0) - torch.stack(logqzxs, 0)
            loss = loss - torch.mean(torch.logsumexp(table, 0) - log_k)
        d.done()
        return loss
