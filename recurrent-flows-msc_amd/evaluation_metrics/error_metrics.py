"""Evaluator — the evaluation driver of the reference (evaluation_metrics/error_metrics.py): the `compute_loss`
bookkeeping (:358-368), the bits-per-dim test-set loop `get_loss` (:370-417) that re-uses `Solver.preprocess` and
`RFN.loss`, the per-frame image-quality scores `eval_seq` (:154-171: MSE, PSNR and SSIM with skimage 0.17.2's defaults,
computed on the GPU by one rfn_frame_quality_u8 launch per call instead of a per-channel CPU loop), the best-of-N
prediction evaluation `get_eval_values` (:419-598), plus thin wrappers over the model's analysis
methods (`RFN.reconstruct_elbo_gap`, `.probability_future`, `.param_analysis`, RFN/RFN_new.py:496-788).
`plot_samples` (:128-152) writes its ground-truth / prediction grid as a PNG of pixels (no titles, no PDF).
`get_lpips` (:173-187) scores frames with LPIPS on the AlexNet trunk (`lpips` 0.1.3, net='alex', version 0.1; the
definition is pinned in rfn_hip/lpips.py) on the GPU, one trunk pass per argument and one head launch instead of one
network call per frame, once `settings.lpips_weights` names the two upstream weight files (torchvision's AlexNet and
the lpips package's alex.pth; nothing is downloaded); without that setting LPIPS is not computed.
`get_fvd_values` (:1006-1063) is the Frechet Video Distance on the logits of the I3D network (Kinetics-400, RGB stream;
the definition is pinned in rfn_hip/i3d.py), the trunk on the GPU, once `settings.fvd_weights` names local files with
the I3D weights (a PyTorch state dict or an .npz of the TF variables; nothing is downloaded); without that setting it
raises.
`get_eval_values_temperatures` is the temperature study (eval_settings.py:110-126) as one pass: best-of-N at K sampling
temperatures from one RFN.predict_draws call per pass, the temperatures being per-row inputs of generation.
`plot_long_t`, `plot_diversity`, `plot_random_samples` and `plot_temp` (:1220-1415) are written as PNG sheets of pixels
like `plot_samples` (no titles, no coloured frames around the cells, no PDF).  `plot_clips` (ours) shows the draws of a
stochastic model as an animated PNG next to the ground truth, their mean and their spread, and it does draw the
coloured frames: green around given frames, red around generated ones.  The curve figures `plot_eval_values` /
`test_temp_values` (:600-1003) are drawn by the chart kernel (rfn_hip.ops.render_chart, one launch per figure) from the
statistics of evaluation_metrics/curves.py and written as PNG.  So are the analysis figures: `plot_elbo_gap` and
`plot_prob_of_t` (:189-270; get_eval_values("rfn.pt") draws them under settings.extra_plots) and `param_plots`
(:1069-1218) on the synchronized Moving MNIST (data_generators.MovingMNIST_synchronized)."""
import os
import warnings

import numpy as np
import torch


class _BestOfN(object):
    """The best-of-N bookkeeping of one block of draws (one temperature), shared by Evaluator._get_eval_values_draws
    and .get_eval_values_temperatures.  Per batch: start_batch(), add(scores, pred) once per draw in ascending draw id,
    end_batch().  The rules are the reference's (error_metrics.py:500-530): the time-means are compared strictly (ties
    keep the earlier draw), and draw 0's tensors ARE the best-so-far tensors (aliased), so that the "mean over draws"
    averages the final best values in place of draw 0.  The best prediction of every sequence by SSIM stays on the
    device."""
    LOWER_IS_BETTER = {"mse": True, "psnr": False, "ssim": False, "lpips": True}

    def __init__(self, names, device):
        self.names, self.device = tuple(names), device
        self.best_values = {k: [] for k in self.names}
        self.mean_values = {k: [] for k in self.names}
        self.best_preds, self.last_pred = [], None

    def start_batch(self):
        self.best, self.draws, self.best_pred = {}, {k: [] for k in self.names}, None

    def add(self, scores, pred):
        """scores: host tensor [metrics, B, n_pred] in the order of `names`; pred: uint8 [B, n_pred, C, H, W] on the
        device"""
        first = not self.draws[self.names[0]]
        for m, k in enumerate(self.names):
            v = scores[m].clone()
            if first:
                self.best[k] = v   # aliased with the first entry of draws[k], as in the reference
                better = None
            else:
                if self.LOWER_IS_BETTER[k]:
                    better = self.best[k].mean(-1) > v.mean(-1)
                else:
                    better = self.best[k].mean(-1) < v.mean(-1)
                self.best[k][better, :] = v[better, :]
            self.draws[k].append(v)
            if k == "ssim":
                if better is None:
                    self.best_pred = pred.clone()
                elif bool(better.any()):
                    sel = better.to(self.device)
                    self.best_pred[sel] = pred[sel]
        self.last_pred = pred

    def end_batch(self):
        for k in self.names:
            self.mean_values[k].append(torch.stack(self.draws[k]).mean(0))
            self.best_values[k].append(self.best[k])
        self.best_preds.append(self.best_pred)

    def result(self, bpd, dkl, recon):
        """the ten-element tuple of get_eval_values; bpd, dkl, recon: CPU tensors, one value per batch"""
        lp = "lpips" in self.names
        cat = lambda d, k: torch.cat(d[k])
        return (cat(self.best_values, "mse"), cat(self.best_values, "psnr"), cat(self.best_values, "ssim"),
                cat(self.best_values, "lpips") if lp else None, bpd, dkl, recon,
                cat(self.mean_values, "ssim"), cat(self.mean_values, "psnr"), cat(self.mean_values, "lpips") if lp else None)


class _ExtraPlots(object):
    """What get_eval_values("rfn.pt") adds under settings.extra_plots (error_metrics.py:468-476, :548-562, :585-587).
    add(image, imageloss, start), on the first draw of every batch: nll_prob = probability_future(image, start) /
    (ln 2 * prod(dims)) and, from reconstruct_elbo_gap(imageloss, sample=False), nllprior and nllposterior (frames
    1.. in bits per pixel) and their difference, the amortization gap.  finish(), after the loop: the reference's
    three printed lines, then plot_elbo_gap(the last batch) and plot_prob_of_t(all nll_prob).  The values are CPU
    tensors; `paths` holds the two files afterwards."""

    def __init__(self, evaluator):
        self.ev, self.prob, self.prior, self.posterior, self.gap, self.last, self.paths = evaluator, [], [], [], [], None, []

    def add(self, image, imageloss, start):
        model = self.ev.model
        scale = np.log(2.) * torch.prod(torch.tensor(imageloss.shape[2:]))
        self.prob.append(model.probability_future(image, start) / scale)
        _, _, _, nll = model.reconstruct_elbo_gap(imageloss, sample=False)
        self.prior.append(nll[0, 1:, :] / scale)
        self.posterior.append(nll[1, 1:, :] / scale)
        self.gap.append(self.prior[-1] - self.posterior[-1])
        self.last = image

    def finish(self):
        if self.last is None:
            return
        print("BPP Prior: ", torch.cat(self.prior, dim=1).mean())
        print("BPP Posterior: ", torch.cat(self.posterior, dim=1).mean())
        print("Amortization gap: " + str(torch.cat(self.gap, dim=1).mean()))
        self.paths = [self.ev.plot_elbo_gap(self.last), self.ev.plot_prob_of_t(torch.cat(self.prob, dim=0))]


MODEL_NAMES = ("rfn.pt", "srnn.pt")   # the checkpoints this package can evaluate


def check_model_name(model_name):
    """the reference's Evaluator branches on the checkpoint's name: "rfn.pt" takes its RFN branches, "srnn.pt" the other
    ones; its remaining baselines (svg.pt, vrnn.pt) are not part of this package"""
    if model_name not in MODEL_NAMES:
        raise ValueError("Evaluator: cannot evaluate %r: of the baseline models (svg.pt, vrnn.pt, srnn.pt) only srnn.pt "
                         "is part of this package, beside rfn.pt" % (model_name,))
    return model_name == "rfn.pt"


BASELINE_MODEL_NAMES = ("srnn.pt", "vrnn.pt", "svg.pt")   # what tools/eval_baselines.py asks an Evaluator to accept


class Evaluator(object):
    def __init__(self, solver, args=None, settings=None, model_names=None):
        """model_names: the checkpoint names this instance evaluates; None is MODEL_NAMES, what the reference-shaped
        driver (eval_settings.py) accepts.  tools/eval_baselines.py passes BASELINE_MODEL_NAMES: every name but "rfn.pt"
        takes the non-RFN branches (model.loss(image) -> (kl, nll) on the whole sequence,
        model.elbo_importance_weighting(imageloss, iw_samples), model._predict_device / _predict_draws_device)."""
        self.model_names = MODEL_NAMES if model_names is None else tuple(model_names)
        self.solver = solver
        self.model = solver.model
        self.args = args if args is not None else solver.args
        self.choose_data = getattr(self.args, "choose_data", "mnist")
        self.test_loader = getattr(solver, "test_loader", None)
        # the reference evaluates the loss on as many frames as the model was trained on (:387-388)
        self.n_trained = getattr(settings, "n_trained", None) or getattr(self.args, "n_frames", None)
        self.device = solver.device
        # get_eval_values (:419-598) reads the evaluation settings; unset ones default to the training arguments
        self.n_frames = getattr(settings, "n_frames", None) or getattr(self.args, "n_frames", None)
        self.start_predictions = (getattr(settings, "start_predictions", None) or
                                  getattr(self.args, "n_conditions", None))
        self.resample = getattr(settings, "resample", None) or 1
        # the curve figures (plot_eval_values / test_temp_values): the x axis starts at n_conditions
        self.n_conditions = getattr(settings, "n_conditions", None) or getattr(self.args, "n_conditions", None)
        self.temperatures = getattr(settings, "temperatures", None)
        self.extra_plots = bool(getattr(settings, "extra_plots", False))
        self.debug_plot = bool(getattr(settings, "debug_plot", False))
        self._warned_plots = False
        # optional: P draws of every sequence per generation pass, with addressed noise (get_eval_values); unset: one
        # RFN.predict call per draw, noise from torch's generator
        self.draws_per_pass = getattr(settings, "draws_per_pass", None)
        self.seed = int(getattr(settings, "seed", None) or 0)
        # the inner samples of SRNN.elbo_importance_weighting in get_loss("srnn.pt") (the reference's constant: 20)
        self.iw_samples = int(getattr(settings, "iw_samples", None) or 20)
        # optional: K chains per sequence of RFN.elbo_importance_weighting in get_loss("rfn.pt") (None or 0: off, the
        # single-sample ELBO of RFN.loss), run in passes of iw_chains_per_pass chains (None: all K in one pass)
        self.rfn_iw_samples = int(getattr(settings, "rfn_iw_samples", None) or 0)
        self.iw_chains_per_pass = getattr(settings, "iw_chains_per_pass", None)
        self.num_samples_to_plot = int(getattr(settings, "num_samples_to_plot", None) or 5)
        # optional: a directory or a list of files holding the LPIPS-alex weights (rfn_hip.ops.lpips_alex_load); loaded
        # on first use
        self.lpips_weights = getattr(settings, "lpips_weights", None)
        self._lpips = None
        # optional: a directory or a list of files holding the I3D weights (rfn_hip.ops.i3d_load); loaded on first use
        self.fvd_weights = getattr(settings, "fvd_weights", None)
        self._i3d = None

    def check_model_name(self, model_name):
        """True for "rfn.pt", False for another checkpoint name this instance accepts, else a ValueError: with the default
        names that of the module's check_model_name"""
        if self.model_names == MODEL_NAMES:
            return check_model_name(model_name)
        if model_name not in self.model_names:
            raise ValueError("Evaluator: cannot evaluate %r: this Evaluator accepts %s" %
                             (model_name, ", ".join(self.model_names)))
        return model_name == "rfn.pt"

    def compute_loss(self, nll, kl, dims, t=10):
        """error_metrics.py:358-368 -> (bits/dim, kl / t, nll / t)"""
        kl_store, nll_store = kl.detach(), nll.detach()
        elbo = -(kl_store + nll_store)
        bits_per_dim_loss = float(-elbo / (np.log(2.) * torch.prod(torch.tensor(dims)) * t))
        return bits_per_dim_loss, float(kl_store / t), float(nll_store / t)

    def get_loss(self, model_name="rfn.pt", loss_resamples=1, loader=None, max_batches=None):
        """error_metrics.py:370-417: mean (and, with resampling, standard deviation) of the per-batch bits/dim over the
        test set, model in eval mode.  "rfn.pt": RFN.loss through compute_loss.  "srnn.pt" (the reference's other
        branch, :396-399): the importance-weighted bound SRNN.elbo_importance_weighting(imageloss, K) / (ln 2 * prod(dims)
        * t) with K = settings.iw_samples (default 20, the reference's constant).
        With settings.rfn_iw_samples = K > 0, "rfn.pt" reports the same kind of figure as the baselines: batch i of
        resample r is RFN.elbo_importance_weighting(imageloss, K, seed=settings.seed + r, first_seq=i * B,
        chains_per_pass=settings.iw_chains_per_pass) / (ln 2 * prod(dims) * t), B being the first batch's size; the
        noise is addressed, so the figure is reproducible and torch's generators are not touched.  Unset, "rfn.pt" is
        the path above, unchanged."""
        rfn = self.check_model_name(model_name)
        loader = loader if loader is not None else self.test_loader
        with torch.no_grad():
            self.model.eval()
            means = []
            for r in range(loss_resamples):
                bpd = []
                batch_size = None
                for batch_i, true_image in enumerate(loader):
                    if max_batches is not None and batch_i >= max_batches:
                        break
                    image = true_image[0] if self.choose_data == "bair" and isinstance(true_image, (list, tuple)) else true_image
                    image = self.solver.preprocess(image.to(self.device))
                    imageloss = image[:, :self.n_trained] if self.n_trained else image
                    batch_size = batch_size or int(image.shape[0])
                    if rfn and self.rfn_iw_samples:
                        loss = self.model.elbo_importance_weighting(imageloss, self.rfn_iw_samples, seed=self.seed + r,
                                                                    first_seq=batch_i * batch_size,
                                                                    chains_per_pass=self.iw_chains_per_pass)
                        b = float(loss / (np.log(2.) * torch.prod(torch.tensor(imageloss.shape[2:])) *
                                          (imageloss.shape[1] - 1)))
                    elif rfn:
                        _, kl, nll = self.model.loss(imageloss, 0)
                        b, _, _ = self.compute_loss(nll=nll, kl=kl, dims=imageloss.shape[2:], t=imageloss.shape[1] - 1)
                    else:
                        loss = self.model.elbo_importance_weighting(imageloss, self.iw_samples)
                        b = float(loss / (np.log(2.) * torch.prod(torch.tensor(imageloss.shape[2:])) *
                                          (imageloss.shape[1] - 1)))
                    bpd.append(b)
                means.append(torch.FloatTensor(bpd))
            means = torch.stack(means)
            mean = means.mean()
            std = means.std() if loss_resamples > 1 else -1
        return mean, std

    @staticmethod
    def _as_u8(x, name):
        """uint8 view of a frame tensor: uint8 as is, a float tensor only when it holds integers in [0, 255] (what the
        reference passes after `preprocess(reverse=True)` and its FloatTensor cast)"""
        if not isinstance(x, torch.Tensor):
            raise ValueError("eval_seq: %s must be a tensor, got %s" % (name, type(x).__name__))
        if x.dtype == torch.uint8:
            return x
        if not x.is_floating_point():
            raise ValueError("eval_seq: %s must be uint8 or a float tensor of integers in [0, 255], got %s" %
                             (name, x.dtype))
        if x.numel() and not bool(((x >= 0) & (x <= 255) & (x == torch.floor(x))).all()):
            raise ValueError("eval_seq: %s holds values that are not integers in [0, 255]" % name)
        return x.to(torch.uint8)

    def eval_seq(self, gt, pred):
        """error_metrics.py:154-171: per-frame (mse, ssim, psnr) of ground truth and prediction [bs, T, C, H, W]
        (uint8, or float tensors of integers in [0, 255], on the GPU) as CPU float32 [bs, T]: ssim / psnr are the means
        over channels of skimage 0.17.2's single-channel SSIM / PSNR (+inf on an identical channel), mse the mean of the
        squared difference over (C, H, W).  One kernel launch; no CPU fallback."""
        from rfn_hip import ops
        if not (isinstance(gt, torch.Tensor) and isinstance(pred, torch.Tensor)):
            raise ValueError("eval_seq: gt and pred must be tensors")
        if gt.dim() != 5 or tuple(gt.shape) != tuple(pred.shape):
            raise ValueError("eval_seq: gt and pred must both be [bs, T, C, H, W], got %s and %s" %
                             (tuple(gt.shape), tuple(pred.shape)))
        mse, psnr, ssim = ops.frame_quality(self._as_u8(gt, "gt"), self._as_u8(pred, "pred"))
        return mse.cpu(), ssim.cpu(), psnr.cpu()

    def _lpips_loaded(self):
        """the packed LPIPS-alex weights on the solver's device, loaded once"""
        if self.lpips_weights is None:
            raise RuntimeError("Evaluator: LPIPS needs pretrained weights: set settings.lpips_weights to a directory or "
                               "a list of files holding torchvision's AlexNet state dict and the lpips package's "
                               "alex.pth (nothing is downloaded)")
        if self._lpips is None:
            from rfn_hip import ops
            self._lpips = ops.lpips_alex_load(self.lpips_weights, self.device)
        return self._lpips

    def _lpips_frames(self, x, name):
        if not isinstance(x, torch.Tensor) or x.dim() != 5:
            raise ValueError("get_lpips: %s must be a tensor [bs, T, C, H, W]" % name)
        return self._as_u8(x, name).to(self.device)

    def get_lpips(self, X, Y):
        """error_metrics.py:173-187: per-frame LPIPS (AlexNet trunk; rfn_hip/lpips.py pins the definition) of two video
        tensors [bs, T, C, H, W] (uint8, or float tensors of integers in [0, 255]; C in {1, 3}, one channel standing
        for three) as CPU float32 [bs, T].  One trunk pass per argument and one head launch; no CPU fallback.  Needs
        settings.lpips_weights."""
        from rfn_hip import ops
        w = self._lpips_loaded()
        X, Y = self._lpips_frames(X, "X"), self._lpips_frames(Y, "Y")
        if tuple(X.shape) != tuple(Y.shape):
            raise ValueError("get_lpips: X and Y must both be [bs, T, C, H, W], got %s and %s" %
                             (tuple(X.shape), tuple(Y.shape)))
        return ops.lpips_alex_distance(w, ops.lpips_alex_features(w, X), ops.lpips_alex_features(w, Y)).cpu()

    def _i3d_loaded(self):
        """the packed I3D weights on the solver's device, loaded once"""
        if self.fvd_weights is None:
            raise RuntimeError("Evaluator: FVD needs pretrained weights: set settings.fvd_weights to a directory or a "
                               "list of files holding the I3D (Kinetics-400, RGB) weights, as the PyTorch port's state "
                               "dict or as an .npz of the TF variables (nothing is downloaded)")
        if self._i3d is None:
            from rfn_hip import ops
            self._i3d = ops.i3d_load(self.fvd_weights, self.device)
        return self._i3d

    def get_fvd_values(self, model_name="rfn.pt", n_predicts=None, loader=None, max_batches=None):
        """error_metrics.py:1006-1063: (mean, std) of two Frechet Video Distances between the test set's ground truth,
        frames start_predictions : start_predictions + n_predicts of every sequence, and the model's predictions of
        those frames, each of the two passes over the test data with fresh draws (np.std: the population figure, as
        the reference).  A short last batch is padded with zeros up to the first batch's size for `predict` and cut
        again.  The videos are embedded by the I3D trunk on the GPU (rfn_hip.ops.i3d_embed; embeddings stay on the
        device) and compared by rfn_hip.ops.frechet_distance.  The ground truth's embeddings do not depend on the draw:
        they are computed in the first pass only.  n_predicts defaults to n_frames - start_predictions and must be at
        least 9; fewer than 16 sequences is a ValueError.  Needs settings.fvd_weights."""
        from rfn_hip import ops
        rfn = self.check_model_name(model_name)
        w = self._i3d_loaded()
        # (srnn.pt: the frames stay where they were computed; the embeddings are computed there)
        predict = self.model.predict if rfn else self.model._predict_device
        loader = loader if loader is not None else self.test_loader
        start = self.start_predictions
        n_predicts = int(n_predicts) if n_predicts is not None else self.n_frames - start
        values, gt_emb, batch_size = [], None, getattr(self.args, "batch_size", None)
        with torch.no_grad():
            self.model.eval()
            for _ in range(2):
                preds, gts = [], []
                for batch_i, true_image in enumerate(loader):
                    if max_batches is not None and batch_i >= max_batches:
                        break
                    image = true_image[0] if self.choose_data == "bair" and isinstance(true_image, (list, tuple)) else true_image
                    image = self.solver.preprocess(image.to(self.device))
                    cur_bs = int(image.shape[0])
                    batch_size = batch_size or cur_bs
                    if cur_bs < batch_size:
                        pad = torch.zeros((batch_size - cur_bs,) + tuple(image.shape[1:]), device=image.device,
                                          dtype=image.dtype)
                        _, predictions = predict(torch.cat((image, pad), 0), n_predicts, start)
                        predictions = predictions[:, :cur_bs]
                    else:
                        _, predictions = predict(image, n_predicts, start)
                    pred_u8 = self.solver.preprocess(predictions, reverse=True).permute(1, 0, 2, 3, 4).to(self.device)
                    preds.append(ops.i3d_embed(w, self._as_u8(pred_u8, "pred")))
                    if gt_emb is None:
                        gt_u8 = self.solver.preprocess(image, reverse=True)[:, start:start + n_predicts]
                        gts.append(ops.i3d_embed(w, self._as_u8(gt_u8, "gt").to(self.device)))
                if gt_emb is None:
                    gt_emb = torch.cat(gts)
                values.append(ops.frechet_distance(gt_emb, torch.cat(preds)))
        return float(np.mean(values)), float(np.std(values))

    def plot_samples(self, predictions, true_image, name="samples", n=None):
        """error_metrics.py:128-152 as pixels: a sheet of 2*n rows x T columns, row 2k the ground truth of sequence k
        and row 2k+1 its prediction, written to `<path>eval_folder/<name>.png` (the reference writes a PDF whose cells
        carry score titles; no text is rendered here).  predictions, true_image: uint8 [bs, T, C, H, W] on either
        device (moved to the solver's); n (default: all bs sequences) is how many sequences to show.  One compose
        launch; returns the file's path."""
        from rfn_hip import ops
        from Utils.png import write_png
        for t, nm in ((predictions, "predictions"), (true_image, "true_image")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 5:
                raise ValueError("plot_samples: %s must be a uint8 tensor [bs, T, C, H, W], got %s" %
                                 (nm, (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        if tuple(predictions.shape) != tuple(true_image.shape):
            raise ValueError("plot_samples: predictions %s and true_image %s differ in shape" %
                             (tuple(predictions.shape), tuple(true_image.shape)))
        bs, T = int(predictions.shape[0]), int(predictions.shape[1])
        n = bs if n is None else int(n)
        if not 1 <= n <= bs or T < 1:
            raise ValueError("plot_samples: n = %d sequences of %d, %d frames each" % (n, bs, T))
        predictions, true_image = predictions.to(self.device), true_image.to(self.device)
        rows = []
        for k in range(n):
            rows += [true_image[k], predictions[k]]
        sheet = ops.compose_sheet(rows, T, scanlines=True)
        folder = self.solver.path + "eval_folder"
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, name + ".png")
        write_png(path, sheet)
        return path

    @staticmethod
    def clip_cells(predictions, true_image, n, n_conditions, gain, show=None):
        """the grid of plot_clips: row k = sequence k; columns: the ground truth, the first `show` (default: all) of
        the D draws, the MEAN and the SPREAD of all D.  predictions uint8 [D, bs, T, C, H, W], true_image uint8
        [bs, T, C, H, W], on one device; nothing is copied."""
        from rfn_hip import ops
        D = int(predictions.shape[0])
        cell = lambda frames, mode="frame": ops.ClipCell(frames, mode, gain=gain, switch_at=n_conditions)
        return [[cell(true_image[k])] + [cell(predictions[d, k]) for d in range(D if show is None else show)] +
                [cell(predictions[:, k].transpose(0, 1), "mean"), cell(predictions[:, k].transpose(0, 1), "spread")]
                for k in range(n)]

    def plot_clips(self, predictions, true_image, name="clips", n=None, n_conditions=None, zoom=2, border=2, gain=4,
                   delay_ms=100):
        """The draws of a stochastic model as an animation, `<path>eval_folder/<name>.png` (an animated PNG: viewers that
        do not know the format show frame 0): one row per sequence for the first n (default: all bs) sequences, columns
        ground truth | the D draws | their per-pixel MEAN | their SPREAD (gain x the population standard deviation of
        the bytes), every cell zoomed `zoom` times inside a ring of `border` pixels that is green while the frames are
        given (t < n_conditions, default: the evaluator's) and red once they are generated.  predictions: uint8
        [D, bs, T, C, H, W] or [bs, T, C, H, W] (one draw); true_image: uint8 [bs, T, C, H, W]; on either device (moved
        to the solver's).  One compose launch for all T frames (rfn_hip.ops.compose_clip); returns the file's path."""
        from rfn_hip import ops
        from Utils.png import write_apng
        for t, nm, dims in ((predictions, "predictions", (5, 6)), (true_image, "true_image", (5,))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in dims:
                raise ValueError("plot_clips: %s must be a uint8 tensor [%sbs, T, C, H, W], got %s" %
                                 (nm, "D, " if len(dims) > 1 else "",
                                  (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        if predictions.dim() == 5:
            predictions = predictions.unsqueeze(0)
        if tuple(predictions.shape[1:]) != tuple(true_image.shape):
            raise ValueError("plot_clips: predictions %s and true_image %s differ in shape" %
                             (tuple(predictions.shape), tuple(true_image.shape)))
        D, bs, T = (int(d) for d in predictions.shape[:3])
        n = bs if n is None else int(n)
        if not 1 <= n <= bs or T < 1 or D < 1:
            raise ValueError("plot_clips: n = %d sequences of %d, %d draws of %d frames each" % (n, bs, D, T))
        n_conditions = int(n_conditions if n_conditions is not None else (self.n_conditions or 0))
        predictions, true_image = predictions.to(self.device), true_image.to(self.device)
        clip = ops.compose_clip(self.clip_cells(predictions, true_image, n, n_conditions, int(gain)), T, zoom=int(zoom),
                                border=int(border), scanlines=True)
        folder = self.solver.path + "eval_folder"
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, name + ".png")
        write_apng(path, clip, delay_ms=delay_ms)
        return path

    def get_eval_values(self, model_name="rfn.pt", loader=None, max_batches=None):
        """error_metrics.py:419-598 (its debug_plot sheets only on the draws_per_pass path): per test batch,
        `resample` rounds of RFN.predict (conditioned on start_predictions frames, n_frames - start_predictions
        predicted), the loss on the first n_trained frames and
        eval_seq of the predictions against the ground truth; per sequence the best of the draws is kept (strictly
        higher time-mean PSNR / SSIM, strictly lower MSE; ties keep the earlier draw).  Returns the reference's tuple
        (MSE, PSNR, SSIM, LPIPS, BPD, DKL, RECON, SSIM_std, PSNR_std, LPIPS_std): MSE / PSNR / SSIM [n_seq, n_pred] of the
        best draws; BPD / DKL / RECON one value per batch, from its last resample; SSIM_std / PSNR_std [n_seq, n_pred], the
        mean over the draws.  LPIPS and LPIPS_std are None unless settings.lpips_weights is set; with weights they are
        CPU float32 [n_seq, n_pred] like SSIM and SSIM_std (best draw: strictly lower time-mean LPIPS, :511-512), the
        ground truth's AlexNet features computed once per batch and reused for every draw (resample + 1 trunk passes per
        batch).

        Reference quirk kept on purpose, so that the figures stay comparable with published ones: the first draw's
        SSIM / PSNR / LPIPS tensors ARE the best-so-far tensors (the reference aliases them) and the best-of-N updates write into
        them in place, so the "mean over draws" averages the final best values in place of draw 0.

        With settings.draws_per_pass = P the draws of a batch are generated P at a time with addressed noise
        (settings.seed) and the figures are reproducible: see _get_eval_values_draws.

        With settings.extra_plots and "rfn.pt" (:468-476, :548-562, :585-587): on the first draw of every batch the
        analyses of _ExtraPlots.add, after the loop its three printed lines and the figures KLDdiagnostic.png
        (plot_elbo_gap of the last batch) and bpp_sequence.png (plot_prob_of_t); the returned tuple is the same.  Other
        checkpoints skip the figures.  settings.debug_plot draws nothing on this path (a warning says so).

        "srnn.pt" takes the reference's other branch (:478-483): `kl, nll = model.loss(image)` on the WHOLE sequence,
        with the dims and t of `image`; everything else is the same code."""
        rfn = self.check_model_name(model_name)
        if self.draws_per_pass is not None:
            return self._get_eval_values_draws(loader, max_batches, rfn)
        if self.debug_plot and not self._warned_plots:
            warnings.warn("Evaluator.get_eval_values: debug_plot only draws figures; skipped (the draws_per_pass path "
                          "writes its sheets)")
            self._warned_plots = True
        loader = loader if loader is not None else self.test_loader
        start, n_frames = self.start_predictions, self.n_frames
        extra = _ExtraPlots(self) if rfn and self.extra_plots else None
        lpips_w = self._lpips_loaded() if self.lpips_weights is not None else None
        lpips_values, lpips_std_values = [], []
        if lpips_w is not None:
            from rfn_hip import ops
        mse_values, psnr_values, ssim_values, ssim_std_values, psnr_std_values = [], [], [], [], []
        bpd_list, dkl_list, recon_list = [], [], []
        with torch.no_grad():
            self.model.eval()
            for batch_i, true_image in enumerate(loader):
                if max_batches is not None and batch_i >= max_batches:
                    break
                image = true_image[0] if self.choose_data == "bair" and isinstance(true_image, (list, tuple)) else true_image
                image = self.solver.preprocess(image.to(self.device))
                imageloss = image[:, :self.n_trained] if self.n_trained else image
                image_u8 = self.solver.preprocess(image, reverse=True)
                ssim_draws, psnr_draws, lpips_draws = [], [], []
                gt_feats = None
                for r in range(self.resample):
                    _, predictions = self.model.predict(image, n_frames - start, start)
                    bpd, kl_loss, recon_loss = self._batch_loss(imageloss if rfn else image, rfn)
                    if r == 0 and extra is not None:
                        extra.add(image, imageloss, start)
                    pred_u8 = self.solver.preprocess(predictions, reverse=True).permute(1, 0, 2, 3, 4)
                    pred_u8 = pred_u8.to(self.device)
                    gt_u8 = image_u8[:, start:start + pred_u8.shape[1]]
                    mse, ssim, psnr = self.eval_seq(gt_u8, pred_u8)
                    if lpips_w is not None:
                        if gt_feats is None:
                            gt_feats = ops.lpips_alex_features(lpips_w, self._as_u8(gt_u8, "gt"))
                        lpips = ops.lpips_alex_distance(lpips_w, ops.lpips_alex_features(
                            lpips_w, self._as_u8(pred_u8, "pred")), gt_feats).cpu()
                        if r == 0:
                            lpips_best = lpips   # aliased, as in the reference
                        else:
                            better = lpips_best.mean(-1) > lpips.mean(-1)
                            lpips_best[better, :] = lpips[better, :]
                        lpips_draws.append(lpips)
                    if r == 0:
                        mse_best, ssim_best, psnr_best = mse, ssim, psnr   # aliased, as in the reference
                    else:
                        better = psnr_best.mean(-1) < psnr.mean(-1)
                        psnr_best[better, :] = psnr[better, :]
                        better = ssim_best.mean(-1) < ssim.mean(-1)
                        ssim_best[better, :] = ssim[better, :]
                        better = mse_best.mean(-1) > mse.mean(-1)
                        mse_best[better, :] = mse[better, :]
                    ssim_draws.append(ssim)
                    psnr_draws.append(psnr)
                ssim_std_values.append(torch.stack(ssim_draws).mean(0))
                psnr_std_values.append(torch.stack(psnr_draws).mean(0))
                if lpips_w is not None:
                    lpips_std_values.append(torch.stack(lpips_draws).mean(0))
                    lpips_values.append(lpips_best)
                mse_values.append(mse_best)
                psnr_values.append(psnr_best)
                ssim_values.append(ssim_best)
                bpd_list.append(bpd)
                dkl_list.append(kl_loss)
                recon_list.append(recon_loss)
            if extra is not None:
                extra.finish()
        return (torch.cat(mse_values), torch.cat(psnr_values), torch.cat(ssim_values),
                torch.cat(lpips_values) if lpips_w is not None else None,
                torch.FloatTensor(bpd_list), torch.FloatTensor(dkl_list), torch.FloatTensor(recon_list),
                torch.cat(ssim_std_values), torch.cat(psnr_std_values),
                torch.cat(lpips_std_values) if lpips_w is not None else None)

    def _get_eval_values_draws(self, loader=None, max_batches=None, rfn=True):
        """get_eval_values with settings.draws_per_pass = P: per batch ceil(resample / P) calls of
        RFN._predict_draws_device (SRNN._predict_draws_device for srnn.pt), each generating P draws of the B sequences as P*B rows of one batch (the extractor
        and the ConvLSTM over the conditioning frames run once per call, every generated frame is one hipGraph replay
        for all P*B rows).  The noise is addressed (rfn_hip.ops.keyed_normal): draw r of sequence batch_i * B + b under
        settings.seed is the same numbers whatever P, the batch size or anything drawn before, so the result for a
        given (seed, resample) does not depend on P; a last pass still runs P draws and ignores draws >= resample.
        Per pass one frame_quality launch scores the P*B sequences (with lpips_weights: one trunk pass over the P*B*T
        predicted frames; the ground truth's features are computed once per batch), the scores come to the host in
        one copy and the predictions stay on the device.  The best-of-N rules are those of get_eval_values, applied to
        the draws in ascending draw id: strict comparisons of time-means, ties keep the earlier draw, and the
        reference's aliasing of draw 0 in the "mean over draws".  Same tuple, dtypes, shapes and devices.
        model.loss runs once per batch, after the passes, not once per draw: BPD / DKL / RECON are one stochastic
        evaluation per batch either way (get_eval_values reports that of the last draw).
        The best prediction of every sequence by SSIM is kept on the device; with settings.debug_plot three sheets are
        written through plot_samples after the loop (error_metrics.py:590-597, pixels only): random_samples_ssim.png
        (the last batch's last draw), best_samples.png and worst_samples.png (the first and last of the sequences
        ordered by time-mean SSIM of their best draw, descending), settings.num_samples_to_plot sequences each
        (default 5, capped at the sequences there are), the first six predicted frames.  With settings.extra_plots the
        analyses of _ExtraPlots run once per batch, after the passes, and its figures are drawn after the loop."""
        P = int(self.draws_per_pass)
        if P < 1:
            raise ValueError("Evaluator: settings.draws_per_pass must be at least 1, got %d" % P)
        loader = loader if loader is not None else self.test_loader
        start, n_frames, R = self.start_predictions, self.n_frames, self.resample
        n_pass = -(-R // P)
        lpips_w = self._lpips_loaded() if self.lpips_weights is not None else None
        names = ("mse", "psnr", "ssim") + (("lpips",) if lpips_w is not None else ())
        book = _BestOfN(names, self.device)
        extra = _ExtraPlots(self) if rfn and self.extra_plots else None
        bpd_list, dkl_list, recon_list = [], [], []
        gts = []
        batch_size = None
        with torch.no_grad():
            self.model.eval()
            for batch_i, true_image in enumerate(loader):
                if max_batches is not None and batch_i >= max_batches:
                    break
                image = true_image[0] if self.choose_data == "bair" and isinstance(true_image, (list, tuple)) else true_image
                image = self.solver.preprocess(image.to(self.device))
                imageloss = image[:, :self.n_trained] if self.n_trained else image
                B = int(image.shape[0])
                batch_size = batch_size or B
                gt_u8 = self.solver.preprocess(image, reverse=True)[:, start:n_frames].contiguous()
                gt_feats = None
                book.start_batch()
                for ps in range(n_pass):
                    _, predictions = self.model._predict_draws_device(image, n_frames - start, start, P, self.seed,
                                                                      first_seq=batch_i * batch_size, first_draw=ps * P)
                    # [n_pred, P, B, C, H, W] -> [P, B, n_pred, C, H, W]
                    pred_u8 = self.solver.preprocess(predictions, reverse=True).permute(1, 2, 0, 3, 4, 5).contiguous()
                    host, gt_feats = self._score_pass(gt_u8, pred_u8, names, lpips_w, gt_feats)
                    for d in range(min(P, R - ps * P)):
                        book.add(host[:, d], pred_u8[d])
                bpd, kl_loss, recon_loss = self._batch_loss(imageloss if rfn else image, rfn)
                if extra is not None:
                    extra.add(image, imageloss, start)
                book.end_batch()
                bpd_list.append(bpd)
                dkl_list.append(kl_loss)
                recon_list.append(recon_loss)
                gts.append(gt_u8)
                last_gt = gt_u8
            if extra is not None:
                extra.finish()
        out = book.result(torch.FloatTensor(bpd_list), torch.FloatTensor(dkl_list), torch.FloatTensor(recon_list))
        ssim_all, last_pred = out[2], book.last_pred
        # best_preds_ssim of the reference: every sequence's best draw by SSIM, on the device
        self.best_preds_ssim = torch.cat(book.best_preds)
        if self.debug_plot:
            ns, nf = self.num_samples_to_plot, 6
            ordered = torch.argsort(ssim_all.mean(-1), descending=True).to(self.device)
            preds, gt = self.best_preds_ssim[ordered], torch.cat(gts)[ordered]
            n = min(ns, int(last_pred.shape[0]))
            self.plot_samples(last_pred[:n, :nf], last_gt[:n, :nf], name="random_samples_ssim")
            n = min(ns, int(preds.shape[0]))
            self.plot_samples(preds[:n, :nf], gt[:n, :nf], name="best_samples")
            self.plot_samples(preds[-n:, :nf], gt[-n:, :nf], name="worst_samples")
        return out

    def _score_pass(self, gt_u8, pred_u8, names, lpips_w, gt_feats):
        """the scores of one generation pass: gt_u8 uint8 [B, n_pred, C, H, W], pred_u8 uint8 [M, B, n_pred, C, H, W]
        (M draws, or temperatures x draws) -> (host tensor [metrics, M, B, n_pred] in the order of `names`, the ground
        truth's LPIPS features repeated M times, for the batch's next pass).  One frame_quality launch, with lpips_w
        one trunk pass over the predicted frames, one device-to-host copy."""
        from rfn_hip import ops
        M = int(pred_u8.shape[0])
        gt_rep = gt_u8.unsqueeze(0).expand(M, *gt_u8.shape)
        scores = dict(zip(("mse", "psnr", "ssim"), ops.frame_quality(gt_rep, pred_u8)))
        if lpips_w is not None:
            if gt_feats is None:
                f = ops.lpips_alex_features(lpips_w, gt_u8)
                gt_feats = ops.LpipsFeatures(f.data.repeat(M, 1), (M,) + f.lead, f.H, f.W)
            scores["lpips"] = ops.lpips_alex_distance(lpips_w, ops.lpips_alex_features(lpips_w, pred_u8), gt_feats)
        return torch.stack([scores[k] for k in names]).cpu(), gt_feats   # the pass's one copy

    def _batch_loss(self, imageloss, rfn=True):
        """(bits/dim, kl / t, nll / t) of one model.loss evaluation of a batch: RFN.loss(x, logdet) -> (kl with free
        bits, kl, nll), SRNN.loss(x) -> (kl, nll)"""
        if rfn:
            _, kl, nll = self.model.loss(imageloss, 0)
        else:
            kl, nll = self.model.loss(imageloss)
        return self.compute_loss(nll=nll, kl=kl, dims=imageloss.shape[2:], t=imageloss.shape[1] - 1)

    def get_eval_values_temperatures(self, temperatures, model_name="rfn.pt", loader=None, max_batches=None):
        """The temperature study (eval_settings.py:110-126: get_eval_values once per value of --temperatures) as one
        pass over the test set: returns {T: tuple}, each tuple the ten-element tuple of get_eval_values computed for
        that sampling temperature (the kl temperature is the model's, as in the reference's loop).  Needs
        settings.draws_per_pass; with K temperatures a pass generates P = max(1, draws_per_pass // K) draws of the B
        sequences at all K temperatures as K*P*B rows of one RFN._predict_draws_device call (about draws_per_pass * B
        rows, the memory of that setting), ceil(resample / P) passes per batch.  The conditioning frames are encoded
        once per pass, the temperatures are per-row inputs of generation (one hipGraph whatever the values) and all K
        blocks use the same addressed noise, draw r of sequence batch_i * B + b under settings.seed: the figures for
        one temperature do not depend on which other temperatures are swept with it, nor on P.  Per pass one
        frame_quality launch scores the K*P*B sequences (with lpips_weights: one trunk pass) and the scores come to
        the host in one copy.  Per temperature the rules are those of _get_eval_values_draws (the same bookkeeping
        code): ascending draw id, strict comparisons of time-means, the draw-0 aliasing, draws >= resample of a padded
        last pass ignored.  model.loss runs once per batch: BPD / DKL / RECON do not depend on the sampling temperature
        and the K tuples share them.  self.best_preds_ssim becomes a dict {T: uint8 tensor on the device} in this call
        only.  The debug_plot sheets are not written here (they would overwrite one another per temperature).
        RFN only: SRNN has no sampling temperature, "srnn.pt" is a ValueError."""
        if not self.check_model_name(model_name):
            raise ValueError("Evaluator.get_eval_values_temperatures: %s has no sampling temperature; the temperature "
                             "study is for rfn.pt" % model_name)
        temps = [float(t) for t in temperatures]
        if not temps or len(set(temps)) != len(temps):
            raise ValueError("Evaluator.get_eval_values_temperatures: need at least one temperature and no duplicates, "
                             "got %s" % (temps,))
        if self.draws_per_pass is None:
            raise ValueError("Evaluator.get_eval_values_temperatures needs settings.draws_per_pass (without it, call "
                             "get_eval_values once per temperature)")
        K = len(temps)
        P = self.draws_per_temperature(self.draws_per_pass, K)
        if self.extra_plots and not self._warned_plots:
            warnings.warn("Evaluator.get_eval_values: extra_plots only draws figures; skipped")
            self._warned_plots = True
        loader = loader if loader is not None else self.test_loader
        start, n_frames, R = self.start_predictions, self.n_frames, self.resample
        n_pass = -(-R // P)
        lpips_w = self._lpips_loaded() if self.lpips_weights is not None else None
        names = ("mse", "psnr", "ssim") + (("lpips",) if lpips_w is not None else ())
        books = [_BestOfN(names, self.device) for _ in temps]
        bpd_list, dkl_list, recon_list = [], [], []
        batch_size = None
        with torch.no_grad():
            self.model.eval()
            for batch_i, true_image in enumerate(loader):
                if max_batches is not None and batch_i >= max_batches:
                    break
                image = true_image[0] if self.choose_data == "bair" and isinstance(true_image, (list, tuple)) else true_image
                image = self.solver.preprocess(image.to(self.device))
                imageloss = image[:, :self.n_trained] if self.n_trained else image
                B = int(image.shape[0])
                batch_size = batch_size or B
                gt_u8 = self.solver.preprocess(image, reverse=True)[:, start:n_frames].contiguous()
                gt_feats = None
                for book in books:
                    book.start_batch()
                for ps in range(n_pass):
                    _, predictions = self.model._predict_draws_device(image, n_frames - start, start, P, self.seed,
                                                                      first_seq=batch_i * batch_size, first_draw=ps * P,
                                                                      temperatures=temps)
                    # [n_pred, K, P, B, C, H, W] -> [K*P, B, n_pred, C, H, W]
                    pred_u8 = self.solver.preprocess(predictions, reverse=True)
                    pred_u8 = pred_u8.reshape(pred_u8.shape[0], K * P, *pred_u8.shape[3:]).permute(1, 2, 0, 3, 4, 5)
                    pred_u8 = pred_u8.contiguous()
                    host, gt_feats = self._score_pass(gt_u8, pred_u8, names, lpips_w, gt_feats)
                    for k, book in enumerate(books):
                        for d in range(min(P, R - ps * P)):
                            book.add(host[:, k * P + d], pred_u8[k * P + d])
                bpd, kl_loss, recon_loss = self._batch_loss(imageloss)
                for book in books:
                    book.end_batch()
                bpd_list.append(bpd)
                dkl_list.append(kl_loss)
                recon_list.append(recon_loss)
        shared = (torch.FloatTensor(bpd_list), torch.FloatTensor(dkl_list), torch.FloatTensor(recon_list))
        self.best_preds_ssim = {t: torch.cat(book.best_preds) for t, book in zip(temps, books)}
        return {t: book.result(*shared) for t, book in zip(temps, books)}

    @staticmethod
    def draws_per_temperature(draws_per_pass, n_temperatures):
        """P = max(1, draws_per_pass // K): the draws per pass of a sweep over K temperatures, so that a pass holds about
        draws_per_pass * B rows"""
        draws_per_pass, n_temperatures = int(draws_per_pass), int(n_temperatures)
        if draws_per_pass < 1 or n_temperatures < 1:
            raise ValueError("Evaluator: need draws_per_pass >= 1 and at least one temperature (got %d, %d)" %
                             (draws_per_pass, n_temperatures))
        return max(1, draws_per_pass // n_temperatures)

    # ---- the four RFN-only figures of eval_settings.py (error_metrics.py:1220-1415) as sheets of pixels
    def _sheet_batch(self):
        """the first test batch in model space on the device; torch's generators are restored by the caller"""
        image = next(iter(self.test_loader))
        image = image[0] if self.choose_data == "bair" and isinstance(image, (list, tuple)) else image
        return self.solver.preprocess(image.to(self.device))

    def _write_sheet(self, rows, n_cols, name):
        from rfn_hip import ops
        from Utils.png import write_png
        sheet = ops.compose_sheet(rows, n_cols, n_bits=int(getattr(self.solver, "n_bits", 8)),
                                  preprocess_range=getattr(self.solver, "preprocess_range", "0.5"), scanlines=True)
        folder = self.solver.path + "eval_folder"
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, name + ".png")
        write_png(path, sheet)
        return path

    def _sheet(self, model_name, draw):
        """run `draw(image)` -> [(rows, n_cols, name), ...] on the first test batch in eval mode and write the sheets;
        torch's CPU and GPU generator states and model.training are what they were afterwards (the loader may shuffle
        with torch's generator; the frames themselves are drawn with addressed noise under settings.seed)"""
        if model_name != "rfn.pt":
            raise ValueError("Evaluator: the sheets need an RFN model (rfn.pt), got %s" % model_name)
        was_training = self.model.training
        on_gpu = self.device.type == "cuda"
        cpu_rng = torch.get_rng_state()
        gpu_rng = torch.cuda.get_rng_state(self.device) if on_gpu else None
        try:
            with torch.no_grad():
                self.model.eval()
                paths = [self._write_sheet(*sheet) for sheet in draw(self._sheet_batch())]
        finally:
            self.model.train(was_training)
            torch.set_rng_state(cpu_rng)
            if on_gpu:
                torch.cuda.set_rng_state(gpu_rng, self.device)
        return paths

    def _rollout_sheet(self, model_name, name, n_predictions, n_conditions, t_list, n_sequences):
        t_list = [int(t) for t in t_list]
        if not t_list or min(t_list) < 0 or max(t_list) >= n_conditions + n_predictions:
            raise ValueError("Evaluator.%s: t_list %s outside the %d frames of cat(conditions, predictions)" %
                             (name, t_list, n_conditions + n_predictions))

        def draw(image):
            conditions, predictions = self.model._predict_draws_device(image, n_predictions, n_conditions, 1, self.seed)
            t_seq = torch.cat((conditions, predictions[:, 0]), 0)           # [T, B, C, H, W]
            n = min(int(n_sequences), int(image.shape[0]))
            return [([t_seq[t_list, k] for k in range(n)], len(t_list), name)]
        return self._sheet(model_name, draw)[0]

    def plot_long_t(self, model_name="rfn.pt", n_predictions=80, n_conditions=5, t_list=(3, 4, 9, 19, 39, 59, 69),
                    n_sequences=4):
        """error_metrics.py:1220-1258 as pixels: `eval_folder/plot_long_t.png`, one row per sequence (the first
        n_sequences of the first test batch, capped at the batch), the columns being frames t_list of
        cat(conditions, predictions) of one rollout of n_predictions frames after n_conditions given ones, at the
        model's temperatures.  No titles and no red / green cell borders.  The noise is addressed noise under
        settings.seed (draw 0); torch's generators and the model's attributes are left as they were.  Returns the
        path."""
        return self._rollout_sheet(model_name, "plot_long_t", n_predictions, n_conditions, t_list, n_sequences)

    def plot_random_samples(self, model_name="rfn.pt", n_predictions=10, n_conditions=3, t_list=(1, 2, 3, 4, 5, 6, 7),
                            n_sequences=5):
        """error_metrics.py:1378-1415 as pixels: `eval_folder/plot_rollouts.png`, the layout of plot_long_t.  Returns
        the path."""
        return self._rollout_sheet(model_name, "plot_rollouts", n_predictions, n_conditions, t_list, n_sequences)

    def plot_diversity(self, model_name="rfn.pt", n_resamples=3, n_predictions=25, n_conditions=5, t_list=(3, 7, 12, 20)):
        """error_metrics.py:1328-1376 as pixels: `eval_folder/plot_diversity_1.png` (sequence 1 of the first test batch)
        and `plot_diversity_2.png` (sequence 0), one row per draw, the columns being predicted frames t_list.  All
        n_resamples draws come from one RFN.predict_draws call (addressed noise under settings.seed, draws
        0 .. n_resamples - 1).  Returns the two paths."""
        t_list = [int(t) for t in t_list]
        if not t_list or min(t_list) < 0 or max(t_list) >= n_predictions:
            raise ValueError("Evaluator.plot_diversity: t_list %s outside the %d predicted frames" % (t_list, n_predictions))

        def draw(image):
            if int(image.shape[0]) < 2:
                raise ValueError("Evaluator.plot_diversity shows sequences 0 and 1; the batch holds %d" % image.shape[0])
            _, predictions = self.model._predict_draws_device(image, n_predictions, n_conditions, int(n_resamples),
                                                              self.seed)                 # [n_pred, R, B, C, H, W]
            return [([predictions[t_list, r, seq] for r in range(int(n_resamples))], len(t_list), name)
                    for name, seq in (("plot_diversity_1", 1), ("plot_diversity_2", 0))]
        return tuple(self._sheet(model_name, draw))

    def plot_temp(self, model_name="rfn.pt", orig_temps=None, kl_analysis=False, duplicate_samples=False,
                  t_list=(0, 1, 2, 9, 19, 39), temperatures=(0.001, 0.3, 0.5, 0.7, 1, 2), n_conditions=5):
        """error_metrics.py:1260-1325 as pixels: one row per temperature, showing sequence 0 of the first test batch,
        written to `eval_folder/plot_temp_samples.png`, `plot_temp_samples_kl.png` (kl_analysis),
        `plot_temp_samples_dup.png` (duplicate_samples) or `plot_temp_dup_kl.png` (both).  The swept temperature is the
        flow's sampling temperature, with kl_analysis the prior's (kl) temperature; the other one is 1e-9 in every row.
        Without duplicate_samples the rows are one rollout of max(t_list) + 1 predicted frames (the reference always
        rolls 50) and column i shows frame t_list[i]; with it, column i shows frame t_list[i] of draw i of a 5-frame
        rollout, so t_list = [0] * 8 is eight independent first frames.  Either way all rows come from ONE
        RFN.predict_draws call with len(temperatures) per-row temperatures, and all rows share their noise (addressed
        noise under settings.seed): a row is the same draw as the row above it at another temperature, which is the
        comparison the figure is for (the reference draws every row afresh).  orig_temps (the reference restores the
        model's attributes from it) is accepted and ignored: the attributes are never changed.  Returns the path."""
        t_list = [int(t) for t in t_list]
        swept = [float(t) for t in temperatures]
        if not swept:
            raise ValueError("Evaluator.plot_temp: no temperatures")
        n_pred = 5 if duplicate_samples else (max(t_list) + 1 if t_list else 0)
        if not t_list or min(t_list) < 0 or max(t_list) >= n_pred:
            raise ValueError("Evaluator.plot_temp: t_list %s outside the %d predicted frames" % (t_list, n_pred))
        name = {(False, False): "plot_temp_samples", (True, False): "plot_temp_samples_kl",
                (False, True): "plot_temp_samples_dup", (True, True): "plot_temp_dup_kl"}[(bool(kl_analysis),
                                                                                          bool(duplicate_samples))]
        other = [1e-9] * len(swept)
        kw = dict(temperatures=other, kl_temperatures=swept) if kl_analysis else dict(temperatures=swept,
                                                                                      kl_temperatures=other)

        def draw(image):
            n_draws = len(t_list) if duplicate_samples else 1
            _, preds = self.model._predict_draws_device(image, n_pred, n_conditions, n_draws, self.seed, **kw)
            # [n_pred, K, n_draws, B, C, H, W]
            if duplicate_samples:
                rows = [torch.stack([preds[t, k, i, 0] for i, t in enumerate(t_list)]) for k in range(len(swept))]
            else:
                rows = [preds[t_list, k, 0, 0] for k in range(len(swept))]
            return [(rows, len(t_list), name)]
        return self._sheet(model_name, draw)[0]

    # ---- the curve figures (error_metrics.py:600-1003), drawn by the chart kernel (rfn_hip.ops.render_chart)
    def _curve_figures(self, entries, folder, suffix):
        """the three figures of evaluation_metrics.curves.build_figures for `entries`, each rendered in one launch and
        written to folder/<name><suffix>.png; returns the paths"""
        from evaluation_metrics.curves import FIGURE_NAMES, build_figures
        from rfn_hip import ops
        from Utils.png import write_png
        if self.n_conditions is None or self.n_trained is None:
            raise ValueError("Evaluator: the curve figures need settings.n_conditions and the trained sequence length")
        figures = build_figures(entries, int(self.n_conditions), int(self.n_trained))
        os.makedirs(folder, exist_ok=True)
        paths = []
        for name in FIGURE_NAMES:
            paths.append(os.path.join(folder, name + suffix + ".png"))
            write_png(paths[-1], ops.render_chart(figures[name], scanlines=True))
        return paths

    def plot_eval_values(self, path, label_names, experiment_names):
        """error_metrics.py:812-1003: best-of-N SSIM / PSNR / LPIPS against the frame index for several experiments,
        read from `path + experiment + "/eval_folder/evaluations.pt"`: eval_plots_max (means with 95 % confidence
        bands), eval_plots_max_median (medians with 2.5 % / 97.5 % quantile bands) and eval_plots_mean_mean (the mean
        over draws with error bars), three panels each, x = n_conditions + arange(T), a dashed line at n_trained, a
        grid, the legend under the panels; written into the LAST experiment's eval_folder, as the reference does.
        1900 x 500 pixels (its 19 x 5 inches at 100 dpi).  Deviations: PNG instead of PDF, drawn by the chart kernel
        with a 5x7 dot-matrix font; the median-LPIPS panel uses the x axis of the others (the reference's arange(0, T)
        there is a slip); when an experiment's LPIPS entries are None (no weights were given) the LPIPS panels show
        their title and "no LPIPS weights".  Touches neither the model nor torch's generators nor the loaders.  Returns
        the three paths."""
        if len(label_names) < len(experiment_names):
            raise ValueError("Evaluator.plot_eval_values: %d labels for %d experiments" %
                             (len(label_names), len(experiment_names)))
        entries = []
        for label, name in zip(label_names, experiment_names):
            d = torch.load(path + name + "/eval_folder/evaluations.pt", map_location="cpu", weights_only=True)
            print("Temperature is set to " + str(d["temperature"]) + " for experiment " + label)
            entries.append((label, d))
        return self._curve_figures(entries, path + experiment_names[-1] + "/eval_folder", "")

    def test_temp_values(self, path, label_names, experiment_names):
        """error_metrics.py:600-809: the three figures of plot_eval_values over the temperatures of ONE experiment:
        curve k is `path + experiment_names[0] + "/eval_folder/t<T>evaluations.pt"` of settings.temperatures[k],
        labelled "T= <T>"; written as eval_plots_max_temp, eval_plots_max_median_temp and eval_plots_mean_mean_temp
        into experiment 0's eval_folder.  The same deviations and no side effects; label_names is unused, as in the
        reference."""
        if not self.temperatures:
            raise ValueError("Evaluator.test_temp_values needs settings.temperatures")
        folder = path + experiment_names[0] + "/eval_folder"
        entries = []
        for T in self.temperatures:
            label = "T= " + str(T)
            d = torch.load(folder + "/t" + str(T).replace(".", "") + "evaluations.pt", map_location="cpu",
                           weights_only=True)
            print("Temperature is set to " + str(d["temperature"]) + " for experiment " + label)
            entries.append((label, d))
        return self._curve_figures(entries, folder, "_temp")

    # ---- the analyses the reference's evaluator drives (error_metrics.py: plot_elbo_gap, plot_prob_of_t, param_plots)
    def elbo_gap(self, image, sample=False):
        self.model.eval()
        return self.model.reconstruct_elbo_gap(self.solver.preprocess(image.to(self.device)), sample=sample)

    def probability_future(self, image, n_conditions):
        self.model.eval()
        return self.model.probability_future(self.solver.preprocess(image.to(self.device)), n_conditions)

    def param_analysis(self, image, n_predictions, n_conditions):
        self.model.eval()
        return self.model.param_analysis(self.solver.preprocess(image.to(self.device)), n_predictions, n_conditions)

    def _chart_png(self, figure, path):
        from rfn_hip import ops
        from Utils.png import write_png
        os.makedirs(os.path.dirname(path), exist_ok=True)
        write_png(path, ops.render_chart(figure, scanlines=True))
        return path

    def elbo_gap_rows(self, image, recons):
        """the three rows of plot_elbo_gap's sheet as uint8 device tensors [t, C, H, W]: sequence 0 of `image` (model
        space, [B, t, C, H, W]) and of recons[0] / recons[1] ([2, t, B, C, H, W]: prior, posterior) as
        Solver.preprocess(x, reverse=True) makes them; column 0 of the two reconstruction rows is empty (white, the
        sheet's background)"""
        to_u8 = lambda x: self.solver.preprocess(x.to(self.device), reverse=True).contiguous()
        rows = [to_u8(image[0]), to_u8(recons[0, :, 0]), to_u8(recons[1, :, 0])]
        for r in rows[1:]:
            r[0] = 255
        return rows

    def plot_elbo_gap(self, image):
        """error_metrics.py:189-247: `eval_folder/KLDdiagnostic.png` from the first 10 frames of `image` (model space,
        [B, T, C, H, W]) through RFN.reconstruct_elbo_gap (sample=True).  Sequence 0 is shown as three rows of t cells
        -- ground truth, the reconstruction under z ~ prior, under z ~ posterior -- labelled "GT:", "Prior:" and
        "Posterior:"; below them two stacked panels over x = 0 .. t - 1: "Avg. KLD", bars of averageKLDseq[:, 0], and
        "BPP", paired bars "Prior" / "Posterior" of averageNLLseq[z, :, 0] / (ln 2 * prod(dims)), with the reference's
        y range (evaluation_metrics.curves.elbo_gap_figure).  200 t x 972 pixels (figsize (2 t, 1.62 * 6) at 100
        dpi).  The chart kernel paints the figure, one compose_sheet launch the rows, and the sheet is copied on the
        device into the figure's reserved top band.  Deviations: PNG instead of PDF; the frames are shown pixel for
        pixel, not scaled to the reference's 2-inch cells; both panels carry a legend and x tick labels (the reference
        hides the upper panel's); a 5x7 dot-matrix font.  Returns the path."""
        from evaluation_metrics.curves import elbo_gap_band, elbo_gap_figure
        from rfn_hip import ops
        from Utils.png import write_png
        image = image[:, :10].to(self.device)
        with torch.no_grad():
            self.model.eval()
            recons, _, kld, nll = self.model.reconstruct_elbo_gap(image)
        t, (H, W) = int(image.shape[1]), (int(d) for d in image.shape[3:])
        bpp = nll[:, :, 0].double().numpy() / (np.log(2.) * float(np.prod(tuple(image.shape[2:]))))
        figure = elbo_gap_figure(kld[:, 0].double().numpy(), bpp, H, W)
        canvas = ops.render_chart(figure, scanlines=False, device=self.device)
        sheet = ops.compose_sheet(self.elbo_gap_rows(image, recons), t, scanlines=False)
        _, x, y, _ = elbo_gap_band(t, H, W)
        canvas[y:y + sheet.shape[0], x:x + sheet.shape[1]] = sheet
        folder = self.solver.path + "eval_folder"
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, "KLDdiagnostic.png")
        write_png(path, canvas)
        return path

    def plot_prob_of_t(self, probT):
        """error_metrics.py:250-270: `eval_folder/bpp_sequence.png`, the mean over sequences of probT[:, 0, :] ([N, 2,
        T'], bits per pixel under z ~ prior) against x = n_conditions + arange(T') with the band -+ 1.96 std / sqrt(N)
        (numpy's population std), a grid, a title and the axis labels "Bits per pixel" / "Frame number"
        (evaluation_metrics.curves.prob_of_t_figure).  640 x 480 pixels (matplotlib's default figsize at 100 dpi).
        Deviations: PNG instead of PDF; the statistics are float64; the band's alpha is the other curve figures' 0.2
        (the reference: 0.1); plain-text title.  Returns the path."""
        from evaluation_metrics.curves import prob_of_t_figure
        if self.n_conditions is None:
            raise ValueError("Evaluator.plot_prob_of_t needs settings.n_conditions")
        return self._chart_png(prob_of_t_figure(probT, int(self.n_conditions)),
                               os.path.join(self.solver.path + "eval_folder", "bpp_sequence.png"))

    def param_plots(self, path, n_conditions, n_sequences=400):
        """error_metrics.py:1069-1218, the parameter analysis on synchronized motion.  The first n_sequences (the
        reference's 400) test sequences of MovingMNIST_synchronized(False, --mnist_root, seq_len=30, num_digits=2,
        deterministic=False, three_channels=False, image_size / digit_size / step_length of the run), ids 0 .. in
        order, in batches of the run's batch size (an incomplete last batch is dropped), go through
        model.param_analysis(x, 30 - n_conditions, n_conditions); the six parameter tensors are summed over (C, H, W),
        averaged over batches and sequences and min-max scaled (evaluation_metrics.curves.parameter_curves).  Written
        into `path`:
          parameter_analysis2.png   two stacked panels "Average" against t = 1 .. 29, x range [1, 29]: the prior's,
                                    posterior's and base distribution's mean above, their sigmas below, a red dashed
                                    line at every k + 1 with hit_boundary[k] == 1, a blue one where it is 2
                                    (curves.param_figure; 1000 x 800 pixels)
          parameter_analysis_mnist_plots_true.png / _pred.png   sequence 0 of the last batch (the frames, the
                                    predictions) as three strips of frames 1:11, 11:21 and 21:29, one compose_sheet
                                    launch each (rows of 10, 10 and 8 cells, no gutter) -- what the reference's permute /
                                    reshape / transpose chain lays out.
        Deviations: the reference takes a random 400 of the test split and shuffles them; only the digit identities
        depend on the sequence id and the curves are means over the sequences, so the first 400 in order are used.  PNG
        charts by the chart kernel, plain-text labels; the strips are pixels, stacked in one sheet each.  Needs an
        SM-MNIST run (choose_data == "mnist") and the MNIST files: otherwise a ValueError names the reason.  Returns
        the three paths."""
        from data_generators import MovingMNIST_synchronized, MovingMNISTLoader
        from data_generators.moving_mnist import mnist_candidate_paths
        from evaluation_metrics.curves import param_figure, parameter_curves
        from rfn_hip import ops
        from Utils.png import write_png
        if self.choose_data != "mnist":
            raise ValueError("Evaluator.param_plots runs on synchronized Moving MNIST: it needs an SM-MNIST run "
                             "(choose_data == 'mnist'), this one is %r" % (self.choose_data,))
        root = getattr(self.args, "mnist_root", "Mnist")
        candidates = mnist_candidate_paths(root, False)
        if not any(os.path.isfile(p) for p in candidates):
            raise ValueError("Evaluator.param_plots needs the MNIST test images; none of %s exists (nothing is "
                             "downloaded)" % ", ".join(candidates))
        seq_len, n_conditions, batch_size = 30, int(n_conditions), int(self.args.batch_size)
        if not 1 <= n_conditions < seq_len or int(n_sequences) < batch_size:
            raise ValueError("Evaluator.param_plots: need 1 <= n_conditions < %d and at least one batch of %d sequences "
                             "(got %d, %d)" % (seq_len, batch_size, n_conditions, int(n_sequences)))
        dataset = MovingMNIST_synchronized(False, root, seq_len=seq_len, num_digits=2,
                                           image_size=int(self.args.image_size), digit_size=int(self.args.digit_size),
                                           deterministic=False, three_channels=False,
                                           step_length=int(self.args.step_length), normalize=False, make_target=False,
                                           seed=getattr(self.args, "data_seed", 0), device=self.device,
                                           length=int(n_sequences))
        print("Init parameter analysis")
        sums = []
        with torch.no_grad():
            self.model.eval()
            for true_image in MovingMNISTLoader(dataset, batch_size):
                image = self.solver.preprocess(true_image.to(self.device))
                out = self.model.param_analysis(image, seq_len - n_conditions, n_conditions)
                sums.append([p.sum([2, 3, 4]) for p in out[:6]])
                prediction = out[6]
        figure = param_figure(parameter_curves(sums), dataset.hit_boundary)
        os.makedirs(path, exist_ok=True)
        paths = [self._chart_png(figure, os.path.join(path, "parameter_analysis2.png"))]
        bits, rng = int(getattr(self.solver, "n_bits", 8)), getattr(self.solver, "preprocess_range", "0.5")
        for name, frames in (("true", image), ("pred", prediction.to(self.device))):
            strips = [frames[0, 1:11], frames[0, 11:21], frames[0, 21:29]]
            paths.append(os.path.join(path, "parameter_analysis_mnist_plots_%s.png" % name))
            write_png(paths[-1], ops.compose_sheet(strips, 10, gutter=0, n_bits=bits, preprocess_range=rng,
                                                   scanlines=True))
        print("Parameter analysis has finished")
        return paths
