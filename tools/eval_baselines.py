#!/usr/bin/env python3
"""Evaluate the learned baselines (SRNN, VRNN, SVG) with the Evaluator, and draw them in one panel with RFN runs:

    python tools/eval_baselines.py --folder_path ./runs/ --experiment_names my_vrnn my_svg --model_path vrnn.pt svg.pt \
        --n_frames 30 --start_predictions 5 --resample 30 --draws_per_pass 8 --seed 1 [--eval_loss] [--calc_fvd] \
        [--lpips_weights ...] [--fvd_weights ...] [--max_batches N] [--plot_with my_rfn my_average --label_names ...]

The reference-shaped driver (evaluation_metrics/eval_settings.py) takes rfn.pt and srnn.pt and refuses every other name;
that stays.  This tool keeps its own table, srnn.pt / vrnn.pt / svg.pt -> Solver, and refuses rfn.pt with a line that
points at the driver.  For every experiment it loads `<folder_path><experiment>/model_folder/<model_path[i]>` and
rebuilds the Solver from the stored arguments with eval_settings.build_evaluator (nothing from the file is executed),
asking for an Evaluator that accepts the three baseline names: they take its non-RFN branches (model.loss(image) on the
whole sequence, elbo_importance_weighting(imageloss, 20) as bits/dim under --eval_loss, _predict_device /
_predict_draws_device).  It writes `<folder_path><experiment>/eval_folder/evaluations.pt` with eval_settings.FULL_KEYS
and `eval_avg_losses.txt` (eval_settings.write_avg_losses): `temperature` is None (the baselines have none), FVD_* and
bits_* are -1 unless --calc_fvd / --eval_loss are given, LPIPS entries are None without --lpips_weights.  The RFN-only
sheets and analyses are skipped with one printed line.  torch's generator is seeded with --seed per experiment and the
convolutions run their deterministic algorithms, so with --draws_per_pass the same --seed gives the same file.

With --plot_with the last step calls Evaluator.plot_eval_values over `plot_with + experiment_names` (labels:
--label_names when there are enough, else the experiment names): eval_plots_max.png, eval_plots_max_median.png and
eval_plots_mean_mean.png, all models in one panel, in the last experiment's eval_folder.  Every evaluations.pt named must
exist (an RFN run's from eval_settings.py, the linear baseline's from main_average.py); otherwise one line says which
is missing and nothing is drawn.  Returns (and prints) the paths written."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))

SOLVERS = {"srnn.pt": "SRNN.trainer", "vrnn.pt": "VRNN.trainer", "svg.pt": "SVG.trainer"}


def solver_class(model_name):
    """the Solver of a baseline's checkpoint name"""
    if model_name == "rfn.pt":
        raise ValueError("eval_baselines: rfn.pt is evaluated by evaluation_metrics/eval_settings.py (its sheets, "
                         "temperatures and analyses live there); this tool takes %s" % ", ".join(sorted(SOLVERS)))
    if model_name not in SOLVERS:
        raise ValueError("eval_baselines: cannot evaluate %r: the checkpoints are %s" %
                         (model_name, ", ".join(sorted(SOLVERS))))
    import importlib
    return importlib.import_module(SOLVERS[model_name]).Solver


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--folder_path", help="Path to folder that contains the experiments", default="./runs/", type=str)
    p.add_argument("--experiment_names", nargs="+", help="Name of the experiments to eval", required=True, type=str)
    p.add_argument("--model_path", nargs="+", help="Name of each experiment's checkpoint: " + ", ".join(sorted(SOLVERS)),
                   required=True, type=str)
    p.add_argument("--n_frames", help="Specify the sequence length of the test data", default=30, type=int)
    p.add_argument("--start_predictions", help="Specify when model starts predicting", default=5, type=int)
    p.add_argument("--n_conditions", help="Number of conditions used for plotting eval_values", default=5, type=int)
    p.add_argument("--resample", help="Draws per sequence of the best-of-N metrics", default=30, type=int)
    p.add_argument("--draws_per_pass", help="Generate this many draws of every sequence per pass, with addressed noise "
                   "(reproducible figures)", default=None, type=int)
    p.add_argument("--seed", help="Seed of the addressed noise of --draws_per_pass", default=0, type=int)
    p.add_argument("--iw_samples", help="Inner samples of the importance-weighted bound of --eval_loss", default=20,
                   type=int)
    p.add_argument("--eval_loss", action="store_true", help="bits/dim as the importance-weighted bound (bits_mean, bits_std)")
    p.add_argument("--calc_fvd", action="store_true", help="Frechet Video Distance (needs --fvd_weights)")
    p.add_argument("--fvd_predicts", help="How far into the future to predict for FVD", default=13, type=int)
    p.add_argument("--lpips_weights", nargs="+", help="Directory or files holding the LPIPS-alex weights (nothing is "
                   "downloaded); without it LPIPS entries are None", default=None, type=str)
    p.add_argument("--fvd_weights", nargs="+", help="Directory or files holding the I3D weights for --calc_fvd (nothing "
                   "is downloaded)", default=None, type=str)
    p.add_argument("--max_batches", help="Evaluate at most this many test batches", default=None, type=int)
    p.add_argument("--plot_with", nargs="*", help="Experiments whose evaluations.pt already exist (RFN runs, the linear "
                   "baseline), drawn in one panel with the ones evaluated here", default=None, type=str)
    p.add_argument("--label_names", nargs="+", help="Labels of the curves: of --plot_with, then of --experiment_names",
                   default=[], type=str)
    return p


def parse_args(argv=None):
    p = build_parser()
    s = p.parse_args(argv)
    if len(s.model_path) < len(s.experiment_names):
        p.error("%d experiments but %d --model_path entries" % (len(s.experiment_names), len(s.model_path)))
    if not 1 <= s.start_predictions < s.n_frames:
        p.error("need 1 <= --start_predictions < --n_frames")
    if s.resample < 1 or s.iw_samples < 1:
        p.error("need --resample >= 1 and --iw_samples >= 1")
    for k in ("lpips_weights", "fvd_weights"):   # one entry: a directory or a file, as the Evaluator takes it
        v = getattr(s, k)
        if v is not None and len(v) == 1:
            setattr(s, k, v[0])
    # what eval_settings.build_evaluator reads beside the flags above
    s.use_validation_set, s.debug_mnist = False, False
    s.extra_plots, s.debug_plot, s.temperatures = False, False, None
    return s


def draw_curves(settings, evaluator):
    """the tool's last step: Evaluator.plot_eval_values over plot_with + experiment_names, or one line naming the first
    evaluations.pt that does not exist.  Returns the paths written."""
    experiments = list(settings.plot_with) + list(settings.experiment_names)
    labels = settings.label_names if len(settings.label_names) >= len(experiments) else experiments
    needed = [settings.folder_path + e + "/eval_folder/evaluations.pt" for e in experiments]
    missing = [p for p in needed if not os.path.exists(p)]
    if missing:
        print("eval_baselines: the curve figures are not drawn: %s does not exist" % missing[0])
        return []
    return evaluator.plot_eval_values(settings.folder_path, labels, experiments)


def main(settings):
    import torch
    from evaluation_metrics import eval_settings as E
    from evaluation_metrics.error_metrics import BASELINE_MODEL_NAMES
    experiments = settings.experiment_names
    for name in settings.model_path[:len(experiments)]:   # before any file is read
        solver_class(name)
    evaluator = None
    for i in range(len(experiments)):
        model_name = settings.model_path[i]
        torch.manual_seed(settings.seed)   # a loader that shuffles, model.loss and the bound draw from torch's generator
        evaluator, args, folder, max_batches = E.build_evaluator(settings, i, solver_for=solver_class,
                                                                 model_names=BASELINE_MODEL_NAMES)
        print("eval_baselines: %s: the RFN-only figures and analyses are skipped (%s)" %
              (model_name, ", ".join(E.RFN_ONLY_SHEETS)))
        # the baselines' strided (de)convolutions are torch modules whose default algorithms add split-K slices with
        # float atomics: the same seed is to give the same file
        deterministic, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
        try:
            if settings.calc_fvd:
                fvd_mean, fvd_std = evaluator.get_fvd_values(model_name, settings.fvd_predicts, max_batches=max_batches)
            else:
                fvd_mean, fvd_std = -1, -1
            if settings.eval_loss:
                bits_mean, bits_std = evaluator.get_loss(model_name, loss_resamples=2, max_batches=max_batches)
            else:
                bits_mean, bits_std = -1, -1
            values = evaluator.get_eval_values(model_name, max_batches=max_batches)
        finally:
            torch.backends.cudnn.deterministic = deterministic
        d = E.eval_dict(values, None)
        d.update({"FVD_mean": fvd_mean, "FVD_std": fvd_std, "bits_mean": bits_mean, "bits_std": bits_std})
        torch.save(d, folder + "/evaluations.pt")
        E.write_avg_losses(folder + "/eval_avg_losses.txt", d)
        print(folder + "/evaluations.pt")
    paths = []
    if settings.plot_with is not None and evaluator is not None:
        paths = draw_curves(settings, evaluator)
        for p in paths:
            print(p)
    return paths


if __name__ == "__main__":
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # hipGraph replay (rfn_hip.graph_capture_safe)
    if "torch" not in sys.modules:
        os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
    main(parse_args())
