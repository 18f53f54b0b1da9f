"""Evaluator — the evaluation driver of the reference (evaluation_metrics/error_metrics.py): the `compute_loss`
bookkeeping (:358-368), the bits-per-dim test-set loop `get_loss` (:370-417) that re-uses `Solver.preprocess` and
`RFN.loss`, the per-frame image-quality scores `eval_seq` (:154-171: MSE, PSNR and SSIM with skimage 0.17.2's defaults,
computed on the GPU by one rfn_frame_quality_u8 launch per call instead of a per-channel CPU loop), the best-of-N
prediction evaluation `get_eval_values` (:419-598, without its plots), plus thin wrappers over the model's analysis
methods (`RFN.reconstruct_elbo_gap`, `.probability_future`, `.param_analysis`, RFN/RFN_new.py:496-788).
`plot_samples` (:128-152) writes its ground-truth / prediction grid as a PNG of pixels (no titles, no PDF).
`get_lpips` (:173-187) scores frames with LPIPS on the AlexNet trunk (`lpips` 0.1.3, net='alex', version 0.1; the
definition is pinned in rfn_hip/lpips.py) on the GPU, one trunk pass per argument and one head launch instead of one
network call per frame, once `settings.lpips_weights` names the two upstream weight files (torchvision's AlexNet and
the lpips package's alex.pth; nothing is downloaded); without that setting LPIPS is not computed.
`get_fvd_values` (:1006-1063) is the Frechet Video Distance on the logits of the I3D network (Kinetics-400, RGB stream;
the definition is pinned in rfn_hip/i3d.py), the trunk on the GPU, once `settings.fvd_weights` names local files with
the I3D weights (a PyTorch state dict or an .npz of the TF variables; nothing is downloaded); without that setting it
raises.  The other plots are not drawn."""
import os
import warnings

import numpy as np
import torch


class Evaluator(object):
    def __init__(self, solver, args=None, settings=None):
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
        self.extra_plots = bool(getattr(settings, "extra_plots", False))
        self.debug_plot = bool(getattr(settings, "debug_plot", False))
        self._warned_plots = False
        # optional: P draws of every sequence per generation pass, with addressed noise (get_eval_values); unset: one
        # RFN.predict call per draw, noise from torch's generator
        self.draws_per_pass = getattr(settings, "draws_per_pass", None)
        self.seed = int(getattr(settings, "seed", None) or 0)
        self.num_samples_to_plot = int(getattr(settings, "num_samples_to_plot", None) or 5)
        # optional: a directory or a list of files holding the LPIPS-alex weights (rfn_hip.ops.lpips_alex_load); loaded
        # on first use
        self.lpips_weights = getattr(settings, "lpips_weights", None)
        self._lpips = None
        # optional: a directory or a list of files holding the I3D weights (rfn_hip.ops.i3d_load); loaded on first use
        self.fvd_weights = getattr(settings, "fvd_weights", None)
        self._i3d = None

    def compute_loss(self, nll, kl, dims, t=10):
        """error_metrics.py:358-368 -> (bits/dim, kl / t, nll / t)"""
        kl_store, nll_store = kl.detach(), nll.detach()
        elbo = -(kl_store + nll_store)
        bits_per_dim_loss = float(-elbo / (np.log(2.) * torch.prod(torch.tensor(dims)) * t))
        return bits_per_dim_loss, float(kl_store / t), float(nll_store / t)

    def get_loss(self, model_name="rfn.pt", loss_resamples=1, loader=None, max_batches=None):
        """error_metrics.py:370-417: mean (and, with resampling, standard deviation) of the per-batch bits/dim over the
        test set, model in eval mode.  Only the RFN branch exists here (the reference's other branch is the
        importance-weighted bound of its VRNN / SRNN baselines)."""
        assert model_name == "rfn.pt", "only the RFN loss is on the hot path"
        loader = loader if loader is not None else self.test_loader
        with torch.no_grad():
            self.model.eval()
            means = []
            for _ in range(loss_resamples):
                bpd = []
                for batch_i, true_image in enumerate(loader):
                    if max_batches is not None and batch_i >= max_batches:
                        break
                    image = true_image[0] if self.choose_data == "bair" and isinstance(true_image, (list, tuple)) else true_image
                    image = self.solver.preprocess(image.to(self.device))
                    imageloss = image[:, :self.n_trained] if self.n_trained else image
                    _, kl, nll = self.model.loss(imageloss, 0)
                    b, _, _ = self.compute_loss(nll=nll, kl=kl, dims=imageloss.shape[2:], t=imageloss.shape[1] - 1)
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
        assert model_name == "rfn.pt", "only the RFN evaluation is on the hot path"
        w = self._i3d_loaded()
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
                        _, predictions = self.model.predict(torch.cat((image, pad), 0), n_predicts, start)
                        predictions = predictions[:, :cur_bs]
                    else:
                        _, predictions = self.model.predict(image, n_predicts, start)
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

    def get_eval_values(self, model_name="rfn.pt", loader=None, max_batches=None):
        """error_metrics.py:419-598 without the plots: per test batch, `resample` rounds of RFN.predict (conditioned on
        start_predictions frames, n_frames - start_predictions predicted), the loss on the first n_trained frames and
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
        (settings.seed) and the figures are reproducible: see _get_eval_values_draws."""
        assert model_name == "rfn.pt", "only the RFN evaluation is on the hot path"
        if self.draws_per_pass is not None:
            return self._get_eval_values_draws(loader, max_batches)
        if (self.extra_plots or self.debug_plot) and not self._warned_plots:
            warnings.warn("Evaluator.get_eval_values: extra_plots / debug_plot only draw figures; skipped")
            self._warned_plots = True
        loader = loader if loader is not None else self.test_loader
        start, n_frames = self.start_predictions, self.n_frames
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
                    _, kl, nll = self.model.loss(imageloss, 0)
                    bpd, kl_loss, recon_loss = self.compute_loss(nll=nll, kl=kl, dims=imageloss.shape[2:],
                                                                 t=imageloss.shape[1] - 1)
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
        return (torch.cat(mse_values), torch.cat(psnr_values), torch.cat(ssim_values),
                torch.cat(lpips_values) if lpips_w is not None else None,
                torch.FloatTensor(bpd_list), torch.FloatTensor(dkl_list), torch.FloatTensor(recon_list),
                torch.cat(ssim_std_values), torch.cat(psnr_std_values),
                torch.cat(lpips_std_values) if lpips_w is not None else None)

    def _get_eval_values_draws(self, loader=None, max_batches=None):
        """get_eval_values with settings.draws_per_pass = P: per batch ceil(resample / P) calls of
        RFN._predict_draws_device, each generating P draws of the B sequences as P*B rows of one batch (the extractor
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
        (default 5, capped at the sequences there are), the first six predicted frames."""
        from rfn_hip import ops
        P = int(self.draws_per_pass)
        if P < 1:
            raise ValueError("Evaluator: settings.draws_per_pass must be at least 1, got %d" % P)
        if self.extra_plots and not self._warned_plots:
            warnings.warn("Evaluator.get_eval_values: extra_plots only draws figures; skipped")
            self._warned_plots = True
        loader = loader if loader is not None else self.test_loader
        start, n_frames, R = self.start_predictions, self.n_frames, self.resample
        n_pass = -(-R // P)
        lpips_w = self._lpips_loaded() if self.lpips_weights is not None else None
        names = ("mse", "psnr", "ssim") + (("lpips",) if lpips_w is not None else ())
        lower_is_better = {"mse": True, "psnr": False, "ssim": False, "lpips": True}
        best_values = {k: [] for k in names}
        mean_values = {k: [] for k in names}
        bpd_list, dkl_list, recon_list = [], [], []
        best_preds, gts = [], []
        batch_size, last_pred = None, None
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
                gt_rep = gt_u8.unsqueeze(0).expand(P, *gt_u8.shape)
                gt_feats = None
                best, draws, best_pred = {}, {k: [] for k in names}, None
                for ps in range(n_pass):
                    _, predictions = self.model._predict_draws_device(image, n_frames - start, start, P, self.seed,
                                                                      first_seq=batch_i * batch_size, first_draw=ps * P)
                    # [n_pred, P, B, C, H, W] -> [P, B, n_pred, C, H, W]
                    pred_u8 = self.solver.preprocess(predictions, reverse=True).permute(1, 2, 0, 3, 4, 5).contiguous()
                    scores = dict(zip(("mse", "psnr", "ssim"), ops.frame_quality(gt_rep, pred_u8)))
                    if lpips_w is not None:
                        if gt_feats is None:
                            f = ops.lpips_alex_features(lpips_w, gt_u8)
                            gt_feats = ops.LpipsFeatures(f.data.repeat(P, 1), (P,) + f.lead, f.H, f.W)
                        scores["lpips"] = ops.lpips_alex_distance(lpips_w, ops.lpips_alex_features(lpips_w, pred_u8),
                                                                  gt_feats)
                    host = torch.stack([scores[k] for k in names]).cpu()   # [metrics, P, B, n_pred]: the pass's one copy
                    for d in range(min(P, R - ps * P)):
                        for m, k in enumerate(names):
                            v = host[m, d].clone()
                            if ps == 0 and d == 0:
                                best[k] = v   # aliased with the first entry of draws[k], as in the reference
                                better = None
                            else:
                                if lower_is_better[k]:
                                    better = best[k].mean(-1) > v.mean(-1)
                                else:
                                    better = best[k].mean(-1) < v.mean(-1)
                                best[k][better, :] = v[better, :]
                            draws[k].append(v)
                            if k == "ssim":
                                if better is None:
                                    best_pred = pred_u8[d].clone()
                                elif bool(better.any()):
                                    sel = better.to(self.device)
                                    best_pred[sel] = pred_u8[d][sel]
                        last_pred = pred_u8[d]
                _, kl, nll = self.model.loss(imageloss, 0)
                bpd, kl_loss, recon_loss = self.compute_loss(nll=nll, kl=kl, dims=imageloss.shape[2:],
                                                             t=imageloss.shape[1] - 1)
                for k in names:
                    mean_values[k].append(torch.stack(draws[k]).mean(0))
                    best_values[k].append(best[k])
                bpd_list.append(bpd)
                dkl_list.append(kl_loss)
                recon_list.append(recon_loss)
                best_preds.append(best_pred)
                gts.append(gt_u8)
                last_gt = gt_u8
        ssim_all = torch.cat(best_values["ssim"])
        # best_preds_ssim of the reference: every sequence's best draw by SSIM, on the device
        self.best_preds_ssim = torch.cat(best_preds)
        if self.debug_plot:
            ns, nf = self.num_samples_to_plot, 6
            ordered = torch.argsort(ssim_all.mean(-1), descending=True).to(self.device)
            preds, gt = self.best_preds_ssim[ordered], torch.cat(gts)[ordered]
            n = min(ns, int(last_pred.shape[0]))
            self.plot_samples(last_pred[:n, :nf], last_gt[:n, :nf], name="random_samples_ssim")
            n = min(ns, int(preds.shape[0]))
            self.plot_samples(preds[:n, :nf], gt[:n, :nf], name="best_samples")
            self.plot_samples(preds[-n:, :nf], gt[-n:, :nf], name="worst_samples")
        return (torch.cat(best_values["mse"]), torch.cat(best_values["psnr"]), ssim_all,
                torch.cat(best_values["lpips"]) if lpips_w is not None else None,
                torch.FloatTensor(bpd_list), torch.FloatTensor(dkl_list), torch.FloatTensor(recon_list),
                torch.cat(mean_values["ssim"]), torch.cat(mean_values["psnr"]),
                torch.cat(mean_values["lpips"]) if lpips_w is not None else None)

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
