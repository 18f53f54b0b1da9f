"""SVG baseline — host mirror of the reference's SVG/SVG.py (which follows github.com/edenton/svg): same constructor
arguments read from `args`, same classes, same state_dict keys and shapes, and the reference's behaviour where it differs
from what one would write: `loss` calls the encoder twice per step, on x_{i-1} and then on x_i, as separate calls (batch
statistics are per call, the encoder's running buffers move 2(T-1) times, the decoder's T-1 times) and takes the skip
tensors from the call on x_{i-1}; every gaussian_lstm call draws one [rows, z_dim] normal whether or not its sample is
used; what the reference calls `logvar` is the Softplus output of std_net, so sigma = exp(softplus(raw) / 2); the
importance-weighted bound takes log q at the PRIOR's sample.

The three LSTM nets (frame_predictor with its layers, posterior, prior: Linear -> nn.LSTMCell(h, h) per layer) run each
cell call through rfn_hip.ops.lstm_cell: one kernel each way on the device (csrc/lstm_cell.hip), the same formulas as
torch ops on the CPU or with RFN_LSTM_CELL=0.  The nn.LSTMCell modules stay in place as parameter holders, so the
state_dict keys (`frame_predictor.lstm.0.weight_ih`, ...) do not move.  Convolutions, BatchNorm, pooling, up-sampling and
the Linear layers are torch modules.  The hidden state is created on the parameters' device (no `.cuda()` anywhere).

One documented deviation: the reference's SVG.__init__ reads `args.variance`, which its own main_svg.py never defines;
main_svg.py of this package has `--variance` (default 1.0).

Every method that draws takes `draws=None`, as SRNN's do (SRNN/SRNN.py: the recorded draws in the reference's order).
`predict_draws`, `_predict_device` and `elbo_importance_weighting` are what an evaluation driver calls; DESIGN.md
section 22."""
import numpy as np
import torch
import torch.distributions as td
import torch.nn as nn

from SRNN.SRNN import _Draws
from Utils import batch_reduce


class vgg_layer(nn.Module):
    def __init__(self, nin, nout):
        super().__init__()
        self.main = nn.Sequential(nn.Conv2d(nin, nout, 3, 1, 1), nn.BatchNorm2d(nout), nn.LeakyReLU(0.2, inplace=True))

    def forward(self, input):
        return self.main(input)


class Encoder(nn.Module):
    def __init__(self, dim, nc=1):
        super().__init__()
        self.dim = dim
        self.c1 = nn.Sequential(vgg_layer(nc, 64), vgg_layer(64, 64))                                # 64 x 64
        self.c2 = nn.Sequential(vgg_layer(64, 128), vgg_layer(128, 128))                             # 32 x 32
        self.c3 = nn.Sequential(vgg_layer(128, 256), vgg_layer(256, 256), vgg_layer(256, 256))       # 16 x 16
        self.c4 = nn.Sequential(vgg_layer(256, 512), vgg_layer(512, 512), vgg_layer(512, 512))       # 8 x 8
        self.c5 = nn.Sequential(nn.Conv2d(512, dim, 4, 1, 0), nn.BatchNorm2d(dim), nn.Tanh())        # 4 x 4 -> 1 x 1
        self.mp = nn.MaxPool2d(kernel_size=2, stride=2, padding=0)

    def forward(self, input):
        h1 = self.c1(input)
        h2 = self.c2(self.mp(h1))
        h3 = self.c3(self.mp(h2))
        h4 = self.c4(self.mp(h3))
        h5 = self.c5(self.mp(h4))
        return h5.view(-1, self.dim), [h1, h2, h3, h4]


class Decoder(nn.Module):
    def __init__(self, dim, nc=1):
        super().__init__()
        self.dim = dim
        self.upc1 = nn.Sequential(nn.ConvTranspose2d(dim, 512, 4, 1, 0), nn.BatchNorm2d(512),
                                  nn.LeakyReLU(0.2, inplace=True))                                   # 1 x 1 -> 4 x 4
        self.upc2 = nn.Sequential(vgg_layer(512 * 2, 512), vgg_layer(512, 512), vgg_layer(512, 256))  # 8 x 8
        self.upc3 = nn.Sequential(vgg_layer(256 * 2, 256), vgg_layer(256, 256), vgg_layer(256, 128))  # 16 x 16
        self.upc4 = nn.Sequential(vgg_layer(128 * 2, 128), vgg_layer(128, 64))                        # 32 x 32
        self.out = nn.Sequential(vgg_layer(64 * 2, 64), nn.ConvTranspose2d(64, nc, 3, 1, 1), nn.Sigmoid())
        self.up = nn.UpsamplingNearest2d(scale_factor=2)

    def forward(self, input):
        vec, skip = input
        d1 = self.upc1(vec.view(-1, self.dim, 1, 1))
        d2 = self.upc2(torch.cat([self.up(d1), skip[3]], 1))
        d3 = self.upc3(torch.cat([self.up(d2), skip[2]], 1))
        d4 = self.upc4(torch.cat([self.up(d3), skip[1]], 1))
        return self.out(torch.cat([self.up(d4), skip[0]], 1))


class _lstm_stack(nn.Module):
    """what lstm_svg and gaussian_lstm share: embed -> the LSTM cells, with the hidden state kept on the module"""

    def __init__(self, input_size, output_size, hidden_size, n_layers, batch_size):
        super().__init__()
        self.input_size, self.output_size, self.hidden_size = input_size, output_size, hidden_size
        self.n_layers, self.batch_size = n_layers, batch_size
        self.embed = nn.Linear(input_size, hidden_size)
        self.lstm = nn.ModuleList([nn.LSTMCell(hidden_size, hidden_size) for i in range(self.n_layers)])

    def init_hidden(self, rows=None):
        rows = self.batch_size if rows is None else int(rows)
        p = self.embed.weight
        return [(torch.zeros(rows, self.hidden_size, device=p.device, dtype=p.dtype),
                 torch.zeros(rows, self.hidden_size, device=p.device, dtype=p.dtype)) for _ in range(self.n_layers)]

    def _cells(self, input):
        from rfn_hip import ops
        h_in = self.embed(input.view(-1, self.input_size))
        for i, cell in enumerate(self.lstm):   # (the modules hold the parameters; the cell itself is ops.lstm_cell)
            self.hidden[i] = ops.lstm_cell(h_in.contiguous(), self.hidden[i][0], self.hidden[i][1], cell.weight_ih,
                                           cell.weight_hh, cell.bias_ih, cell.bias_hh)
            h_in = self.hidden[i][0]
        return h_in


class lstm_svg(_lstm_stack):
    def __init__(self, input_size, output_size, hidden_size, n_layers, batch_size):
        super().__init__(input_size, output_size, hidden_size, n_layers, batch_size)
        self.output = nn.Sequential(nn.Linear(hidden_size, output_size), nn.Tanh())
        self.hidden = self.init_hidden()

    def forward(self, input):
        return self.output(self._cells(input))


class gaussian_lstm(_lstm_stack):
    def __init__(self, input_size, output_size, hidden_size, n_layers, batch_size):
        super().__init__(input_size, output_size, hidden_size, n_layers, batch_size)
        self.mu_net = nn.Linear(hidden_size, output_size)
        self.std_net = nn.Sequential(nn.Linear(hidden_size, output_size), nn.Softplus())
        self.hidden = self.init_hidden()

    def reparameterize(self, mu, logvar, eps):
        return eps.mul(logvar.mul(0.5).exp()).add(mu)

    def forward(self, input, draws=None, eps=None):
        """(z, mu, stdp).  One [rows, z_dim] normal per call, used or not: `eps`, or the next of `draws` (a _Draws)"""
        h_in = self._cells(input)
        mu = self.mu_net(h_in)
        stdp = self.std_net(h_in)
        if eps is None:
            eps = (draws if draws is not None else _Draws(None, mu.device)).normal(mu.shape)
        return self.reparameterize(mu, stdp, eps.to(mu.dtype)), mu, stdp


def init_weights(m):
    classname = m.__class__.__name__
    if classname.find('Conv') != -1 or classname.find('Linear') != -1:
        m.weight.data.normal_(0.0, 0.02)
        m.bias.data.fill_(0)
    elif classname.find('BatchNorm') != -1:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0)


LOSS_TYPES = ("bernoulli", "mse", "gaussian")


class SVG(nn.Module):
    def __init__(self, args):
        super().__init__()
        z_dim, c_features, h_dim = args.z_dim, args.c_features, args.h_dim
        self.loss_type = args.loss_type
        if self.loss_type not in LOSS_TYPES:   # (the reference prints "undefined loss" and fails later)
            raise ValueError("undefined loss %r: SVG has %s" % (self.loss_type, ", ".join(LOSS_TYPES)))
        self.batch_size, channels, hx, wx = args.x_dim
        self.z_dim = z_dim
        self.n_conditions = args.n_conditions
        self.n_predictions = args.n_predictions
        self.mse_criterion = nn.MSELoss(reduction="none")
        self.encoder = Encoder(c_features, channels)
        self.decoder = Decoder(c_features, channels)
        self.encoder.apply(init_weights)
        self.decoder.apply(init_weights)
        self.variance = args.variance
        self.frame_predictor = lstm_svg(c_features + z_dim, c_features, h_dim, args.predictor_rnn_layers, self.batch_size)
        self.posterior = gaussian_lstm(c_features, z_dim, h_dim, args.posterior_rnn_layers, self.batch_size)
        self.prior = gaussian_lstm(c_features, z_dim, h_dim, args.prior_rnn_layers, self.batch_size)
        self.frame_predictor.apply(init_weights)
        self.posterior.apply(init_weights)
        self.prior.apply(init_weights)

    # ------------------------------------------------------------------------------------------------ pieces
    def _init_hidden(self, rows):
        for net in (self.frame_predictor, self.posterior, self.prior):
            net.hidden = net.init_hidden(rows)

    def _nll_pixels(self, x_pred, x_i):
        """the step's negative log-likelihood per pixel (SVG.py:251-258)"""
        if self.loss_type == "bernoulli":
            return -td.Bernoulli(probs=x_pred).log_prob(x_i)
        if self.loss_type == "mse":
            return self.mse_criterion(x_pred, x_i)
        if self.loss_type == "gaussian":
            return -td.Normal(x_pred, self.variance * torch.ones_like(x_pred)).log_prob(x_i)
        raise ValueError("undefined loss %r" % (self.loss_type,))

    def kl_criterion(self, mu1, logvar1, mu2, logvar2):
        sigma1 = logvar1.mul(0.5).exp()
        sigma2 = logvar2.mul(0.5).exp()
        kld = torch.log(sigma2 / sigma1) + (torch.exp(logvar1) + (mu1 - mu2) ** 2) / (2 * torch.exp(logvar2)) - 1 / 2
        return kld.sum() / self.batch_size

    # ------------------------------------------------------------------------------------------------ loss
    def loss(self, x, draws=None):
        d = _Draws(draws, x.device)
        self._init_hidden(x.shape[0])
        t = x.shape[1]
        nll, kl = 0, 0
        for i in range(1, t):
            h, skip = self.encoder(x[:, i - 1])            # (two separate calls, as in the reference: SVG.py:242-243)
            h_target = self.encoder(x[:, i])[0]
            z_t, mu_q, logvar_q = self.posterior(h_target, d)
            _, mu_p, logvar_p = self.prior(h, d)           # (its sample is drawn and dropped)
            h_pred = self.frame_predictor(torch.cat([h, z_t], 1))
            x_pred = self.decoder([h_pred, skip])
            nll = nll + self._nll_pixels(x_pred, x[:, i])  # per pixel, added over time in step order
            kl = kl + self.kl_criterion(mu_q, logvar_q, mu_p, logvar_p)
        d.done()
        return kl, batch_reduce(nll).mean()

    # ------------------------------------------------------------------------------------------------ generation
    # reconstruct, sample and predict end on the CPU, as the reference's do (it fills CPU tensors); `_predict_device`
    # returns predict's tensors where they were computed.
    def reconstruct(self, x, draws=None):
        d = _Draws(draws, x.device)
        self._init_hidden(x.shape[0])
        t = x.shape[1]
        recons = [torch.zeros_like(x[:, 0])]                # (frame 0 is never reconstructed)
        for i in range(1, t):
            condition, skip = self.encoder(x[:, i - 1])
            target = self.encoder(x[:, i])[0].detach()
            z_t, _, _ = self.posterior(target, d)           # (no prior here, as in the reference)
            h_pred = self.frame_predictor(torch.cat([condition.detach(), z_t], 1))
            recons.append(self.decoder([h_pred, skip]).detach())
        d.done()
        return torch.stack(recons, 0).cpu()

    def sample(self, x, n_samples, draws=None):
        if n_samples < 1:
            return torch.zeros((0,) + tuple(x[:, 0].shape), dtype=x.dtype)
        d = _Draws(draws, x.device)
        self._init_hidden(x.shape[0])
        samples = [torch.zeros_like(x[:, 0])]               # (index 0 stays zero: the loop runs 1 .. n_samples - 1)
        condition_x = x[:, 0]
        for i in range(1, n_samples):
            condition, skip = self.encoder(condition_x)
            condition = condition.detach()
            z_t, _, _ = self.prior(condition, d)
            h_pred = self.frame_predictor(torch.cat([condition, z_t], 1))
            condition_x = self.decoder([h_pred, skip])
            samples.append(condition_x.detach())
        d.done()
        return torch.stack(samples, 0).cpu()

    def predict(self, x, n_predictions, n_conditions, draws=None):
        true_x, predictions = self._predict_device(x, n_predictions, n_conditions, draws)
        return true_x.cpu(), predictions.cpu()

    def _predict_device(self, x, n_predictions, n_conditions, draws=None):
        b, t, c, h, w = x.shape
        assert 1 <= n_conditions <= t, "n_conditions must be 1 .. t, the number of frames"
        d = _Draws(draws, x.device)
        self._init_hidden(b)
        x_in = x[:, 0]
        predictions = []
        for i in range(1, n_predictions + n_conditions):
            condition, skip = self.encoder(x_in)
            condition = condition.detach()
            if i < n_conditions:
                target = self.encoder(x[:, i])[0].detach()
                z_t, _, _ = self.posterior(target, d)
                self.prior(condition, d)                                  # (state and draw only)
                self.frame_predictor(torch.cat([condition, z_t], 1))      # (state only)
                x_in = x[:, i]
            else:
                z_t, _, _ = self.prior(condition, d)
                h_pred = self.frame_predictor(torch.cat([condition, z_t], 1))
                x_in = self.decoder([h_pred, skip])
                predictions.append(x_in.detach())
        d.done()
        true_x = x[:, :n_conditions].transpose(0, 1).detach().clone()
        if predictions:
            return true_x, torch.stack(predictions, 0)
        return true_x, torch.zeros((0, b, c, h, w), device=x.device, dtype=x.dtype)

    def predict_draws(self, x, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0):
        """`predict` for n_draws independent draws of every sequence in one pass, with addressed noise (the counterpart
        of VRNN.predict_draws): returns (true_x, predictions), predictions [n_predictions, n_draws, B, C, H, W] on the
        CPU (`_predict_draws_device`: the same on the device).  The encoder of the conditioning frames runs once on the
        B sequences; everything after it runs on n_draws*B rows, draw-major (row r*B + b: draw first_draw + r of
        sequence first_seq + b).
        Noise: conditioning step i (1 .. n_conditions-1) uses t = i, rfn_hip.ops.keyed_normal slot 0 for the posterior
        eps and slot 1 for the prior eps.  Generated frame i uses t = n_conditions + i, slot 0 for the prior eps.  A
        frame therefore depends on (seed, sequence id, draw id) and the data alone: not on B, on n_draws, on how the
        draws are split into calls, or on torch's generator, which is left untouched.
        Eval mode only: batch statistics would couple the draws."""
        true_x, predictions = self._predict_draws_device(x, n_predictions, n_conditions, n_draws, seed, first_seq,
                                                         first_draw)
        return true_x.cpu(), predictions.cpu()

    def _predict_draws_device(self, x, n_predictions, n_conditions, n_draws, seed, first_seq=0, first_draw=0):
        from rfn_hip import ops as K
        assert len(x.shape) == 5, "x must be [bs, t, c, h, w]"
        if self.training:
            raise RuntimeError("SVG.predict_draws needs eval mode: in training mode the batch statistics of the "
                               "normalisation layers would couple the draws (call model.eval() first)")
        b, t, c, h, w = x.shape
        assert 1 <= n_conditions <= t, "n_conditions must be 1 .. t, the number of frames"
        P, B = int(n_draws), int(b)
        if P < 1:
            raise ValueError("SVG.predict_draws: n_draws must be at least 1, got %d" % P)

        def rep(v):   # draw-major: row r*B + b is sequence b
            return v.repeat((P,) + (1,) * (v.dim() - 1))

        def eps(step, slots):
            return K.keyed_normal([(self.z_dim,)] * slots, B, P, seed, step, first_seq, first_draw, device=x.device)

        with torch.no_grad():
            self._init_hidden(P * B)
            feats = [self.encoder(x[:, i]) for i in range(n_conditions)]    # (eval mode: one call per frame, B rows)
            codes = [rep(f[0]) for f in feats]
            for i in range(1, n_conditions):
                eps_q, eps_p = eps(i, 2)
                z_t, _, _ = self.posterior(codes[i], eps=eps_q)
                self.prior(codes[i - 1], eps=eps_p)
                self.frame_predictor(torch.cat([codes[i - 1], z_t], 1))
            true_x = x[:, :n_conditions].transpose(0, 1).detach().clone()
            condition, skip = codes[n_conditions - 1], [rep(s) for s in feats[n_conditions - 1][1]]
            frames = []
            for i in range(n_predictions):
                z_t, _, _ = self.prior(condition, eps=eps(n_conditions + i, 1)[0])
                h_pred = self.frame_predictor(torch.cat([condition, z_t], 1))
                frame = self.decoder([h_pred, skip])
                frames.append(frame.detach())
                if i + 1 < n_predictions:
                    condition, skip = self.encoder(frame)
            if frames:
                predictions = torch.stack(frames, 0).view(n_predictions, P, B, c, h, w)
            else:
                predictions = torch.zeros((0, P, B, c, h, w), device=x.device, dtype=x.dtype)
        return true_x, predictions

    # ------------------------------------------------------------------------------------------------ evaluation
    def _lpx(self, x_pred, x_i):
        """the reference's `lpx_Gz_obs` per row (SVG.py:371-380), with its sign per loss type as it stands there: the
        log-likelihood for "bernoulli" and "gaussian", minus the squared error for "mse" """
        return -self._nll_pixels(x_pred, x_i).sum([-1, -2, -3])

    def _lpx_rows(self, x_pred, x_i):
        """_lpx of the R = K*B rows (k*B + b) of a deferred decoder call under the B frames x_i: without a gradient to
        keep one rfn_hip.ops.pixel_loglik launch that reads x_i in place; otherwise, and with RFN_PIXEL_LOGLIK=0, the
        frames are repeated K times and the torch chain of _lpx runs."""
        from rfn_hip import ops
        if self.loss_type in ops.PIXEL_LOGLIK_MODES and ops.pixel_loglik_route(x_pred, x_i) == "kernel":
            scale = float(self.variance) if self.loss_type == "gaussian" else None   # (a Python number here)
            return ops.pixel_loglik(x_pred, x_i, self.loss_type, scale=scale)
        return self._lpx(x_pred, x_i.repeat(x_pred.shape[0] // x_i.shape[0], 1, 1, 1))

    @staticmethod
    def _log_densities(mu_p, logvar_p, z_t, mu_q, logvar_q, z_tx):
        """(log p(z_t), log q(z_tx | x)) per row: the densities of N(mu_p, exp(logvar_p / 2)) at z_t and of N(mu_q,
        exp(logvar_q / 2)) at z_tx, summed over the latent; one rfn_hip.ops.normal_logvar_pair launch without a gradient
        to keep, the two torch.distributions chains otherwise and with RFN_PIXEL_LOGLIK=0"""
        from rfn_hip import ops
        if ops.pixel_loglik_route(mu_p, logvar_p, z_t, mu_q, logvar_q, z_tx) == "kernel":
            return ops.normal_logvar_pair(mu_p, logvar_p, z_t, mu_q, logvar_q, z_tx)
        return (td.Normal(mu_p, torch.exp(logvar_p * 0.5)).log_prob(z_t).sum([-1]),
                td.Normal(mu_q, torch.exp(logvar_q * 0.5)).log_prob(z_tx).sum([-1]))

    def elbo_importance_weighting(self, x, K, draws=None, defer_decoder=None):
        """The importance-weighted bound of the reference (SVG.py:344-385), as that code behaves: the hidden states of
        the three nets advance K times per frame and carry into the next frame; per inner sample the draws are the
        posterior eps, then the prior eps; log p(z) is the prior's density at the posterior sample z_t, log q(z|x) the
        posterior's density at the PRIOR's sample z_tx.  Returns sum_t -mean_b(logsumexp_k(lpx + log p - log q) - log K);
        the K x B tables stay on the device.
        The decoder does not feed the recurrence.  In eval mode (defer_decoder None) the decoder and the likelihood of a
        time step run ONCE over the K*B rows collected in the k loop, with the skip tensors repeated; in training mode
        every inner sample makes its own decoder call, because the batch statistics are per call in the reference.
        defer_decoder = False / True forces either form.  Without a gradient to keep, the two densities of an inner
        sample are one normal_logvar_pair launch and the deferred likelihood one pixel_loglik launch per time step
        (_log_densities, _lpx_rows)."""
        b, t = x.shape[0], x.shape[1]
        K = int(K)
        if K < 1:
            raise ValueError("SVG.elbo_importance_weighting: K must be at least 1, got %d" % K)
        defer = (not self.training) if defer_decoder is None else bool(defer_decoder)
        d = _Draws(draws, x.device)
        self._init_hidden(b)
        log_k = float(np.log(K))
        loss = 0
        for i in range(1, t):
            x_i = x[:, i]
            h, skip = self.encoder(x[:, i - 1])
            h_target = self.encoder(x_i)[0]
            logpzs, logqzxs, lpxs, h_preds = [], [], [], []
            for k in range(K):
                z_t, mu_q, logvar_q = self.posterior(h_target, d)
                z_tx, mu_p, logvar_p = self.prior(h, d)
                h_pred = self.frame_predictor(torch.cat([h, z_t], 1))
                logp, logq = self._log_densities(mu_p, logvar_p, z_t, mu_q, logvar_q, z_tx)
                logpzs.append(logp)
                logqzxs.append(logq)
                if defer:
                    h_preds.append(h_pred)
                else:
                    lpxs.append(self._lpx(self.decoder([h_pred, skip]), x_i))
            if defer:   # rows k*B + b
                x_pred = self.decoder([torch.cat(h_preds, 0), [s.repeat(K, 1, 1, 1) for s in skip]])
                lpx = self._lpx_rows(x_pred, x_i).view(K, b)
            else:
                lpx = torch.stack(lpxs, 0)
            table = lpx + torch.stack(logpzs, 0) - torch.stack(logqzxs, 0)
            loss = loss - torch.mean(torch.logsumexp(table, 0) - log_k)
        d.done()
        return loss
