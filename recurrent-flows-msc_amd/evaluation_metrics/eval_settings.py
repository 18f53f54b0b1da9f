"""Evaluation driver -- the reference's evaluation entry point (evaluation_metrics/eval_settings.py) for RFN runs:

    python evaluation_metrics/eval_settings.py --folder_path ./runs/ --experiment_names my_run --temperatures 0.7 \
        --n_frames 30 --start_predictions 5 --resample 30 --draws_per_pass 8 --seed 1

For every experiment it loads `<folder_path><experiment>/model_folder/<model_path[i]>` (nothing from the file is
executed), rebuilds the Solver from the stored arguments with test sequences of --n_frames frames, and runs the selected
evaluations with the Evaluator (error_metrics.py):

  without --test_temperature   the four RFN sheets (plot_long_t, plot_diversity, plot_random_samples and plot_temp in
                               the reference's four flag combinations), get_fvd_values under --calc_fvd,
                               get_loss(loss_resamples=2) under --eval_loss and get_eval_values under --calc_eval, at
                               model.temperature = temperatures[i], kl_temperature = 1; written to
                               `<folder_path><experiment>/eval_folder/evaluations.pt` and `eval_avg_losses.txt` with the
                               reference's keys and line order.
  with --test_temperature      best-of-N metrics at every value of --temperatures, one
                               `eval_folder/t<T without the dot>evaluations.pt` each, with the reference's eleven keys.
                               With --draws_per_pass the whole sweep is ONE pass over the test set
                               (Evaluator.get_eval_values_temperatures: the temperatures are per-row inputs of
                               generation); without it, one get_eval_values pass per temperature as in the reference.

Flags, defaults and meanings are the reference's; --draws_per_pass, --seed, --lpips_weights, --fvd_weights and
--max_batches are ours.  `--model_path srnn.pt` evaluates the SRNN baseline through the reference's
non-RFN branches: get_eval_values with SRNN.loss on the whole sequence, get_loss as the
importance-weighted bound (settings.iw_samples inner samples when a caller sets it on the settings object; the parser
has no flag for it and the default is the reference's 20), get_fvd_values; the RFN-only sheets and analyses are skipped
with one printed line, and --test_temperature is refused (SRNN has no temperature).  Deviations: the SVG / VRNN
baselines are not part of this package (any other model name is a ValueError); LPIPS entries are None when --lpips_weights is not given (the reference
would need the lpips package's download); --debug_mnist / --use_validation_set evaluate the FIRST 1000 test sequences
(the reference: a random 1000 for --debug_mnist); the curve figures of plot_eval_values / test_temp_values, the last
step of a run, are PNG files drawn by the chart kernel (skipped with one line when the evaluations.pt files they read
do not exist); --eval_parameters saves the tensors of Evaluator.param_analysis on the first test batch to
`eval_folder/param_analysis.pt` and then, on an SM-MNIST run, draws the figures of Evaluator.param_plots into the
experiment's eval_folder (on other data one line says that they need SM-MNIST); --extra_plots makes get_eval_values
draw KLDdiagnostic.png and bpp_sequence.png (Evaluator.plot_elbo_gap / plot_prob_of_t).  The sheets are written to
the solver's own `eval_folder` (the run's --path under the working directory), which is the same directory when the
driver is started where the training was."""
import argparse
import copy
import os
import sys

if __name__ == "__main__":   # started as a script: the package root is the parent of this directory
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # hipGraph replay (rfn_hip.graph_capture_safe)
    if "torch" not in sys.modules:
        os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")

import torch

EVAL_KEYS = ("SSIM_values", "PSNR_values", "MSE_values", "LPIPS_values", "temperature", "BPD", "DKL", "RECON",
             "SSIM_std_mean", "PSNR_std_mean", "LPIPS_std_mean")                      # the --test_temperature files
FULL_KEYS = EVAL_KEYS + ("FVD_mean", "FVD_std", "bits_mean", "bits_std")              # evaluations.pt
PARAM_KEYS = ("mu_p", "std_p", "mu_q", "std_q", "mu_flow", "std_flow", "predictions")  # param_analysis.pt


def temperature_file_name(temperature):
    """eval_settings.py:126: "t" + str(T) without the dot + "evaluations.pt" (0.7 -> t07evaluations.pt)"""
    return "t" + str(temperature).replace(".", "") + "evaluations.pt"


RFN_ONLY_SHEETS = ("plot_long_t", "plot_diversity", "plot_random_samples", "plot_temp", "param_analysis", "extra_plots")


def solver_class(model_name):
    """eval_settings.py:18-27: the Solver for a checkpoint name; the RFN and the SRNN baseline are part of this package"""
    if model_name == "rfn.pt":
        from RFN.trainer import Solver
    elif model_name == "srnn.pt":
        from SRNN.trainer import Solver
    else:
        raise ValueError("eval_settings: cannot evaluate %r: of the baseline models (svg.pt, vrnn.pt, srnn.pt) only "
                         "srnn.pt is part of this package, beside rfn.pt" % (model_name,))
    return Solver


def eval_dict(values, temperature):
    """the reference's eleven keys from the ten-element tuple of Evaluator.get_eval_values (LPIPS entries stay None
    without weights)"""
    mse, psnr, ssim, lpips, bpd, dkl, recon, ssim_std, psnr_std, lpips_std = values
    cpu = lambda t: None if t is None else t.cpu()
    return {"SSIM_values": cpu(ssim), "PSNR_values": cpu(psnr), "MSE_values": cpu(mse), "LPIPS_values": cpu(lpips),
            "temperature": temperature, "BPD": cpu(bpd), "DKL": cpu(dkl), "RECON": cpu(recon),
            "SSIM_std_mean": ssim_std, "PSNR_std_mean": psnr_std, "LPIPS_std_mean": lpips_std}


def write_avg_losses(path, d):
    """eval_settings.py:94-108, the same lines in the same order"""
    mean0 = lambda t: None if t is None else t.mean(0)
    with open(path, "w") as f:
        print("SSIM:", mean0(d["SSIM_values"]), file=f)
        print("PSNR:", mean0(d["PSNR_values"]), file=f)
        print("MSE:", mean0(d["MSE_values"]), file=f)
        print("LPIPS:", mean0(d["LPIPS_values"]), file=f)
        print("BPD:", d["BPD"].mean(), file=f)
        print("DKL:", d["DKL"].mean(), file=f)
        print("RECON:", d["RECON"].mean(), file=f)
        for k in ("SSIM_std_mean", "PSNR_std_mean", "LPIPS_std_mean", "FVD_mean", "FVD_std", "bits_mean", "bits_std"):
            print(k + ":", d[k], file=f)


def build_evaluator(settings, i, solver_for=None, model_names=None):
    """Solver and Evaluator of experiment i: the stored arguments on one rank, test sequences of settings.n_frames frames
    (the loss is still evaluated on as many frames as the run was trained on).  solver_for / model_names: another table
    of checkpoint names (tools/eval_baselines.py); None is this driver's solver_class and the Evaluator's default."""
    from evaluation_metrics.error_metrics import Evaluator
    model_name = settings.model_path[i]
    Solver = (solver_for or solver_class)(model_name)
    exp = settings.folder_path + settings.experiment_names[i]
    ckpt = Solver.read_checkpoint(exp + "/model_folder/" + model_name)
    args = Solver.args_for_world(ckpt, 1)
    n_trained = args.n_frames
    args.n_frames = settings.n_frames
    solver = Solver(args)
    solver.build()
    solver.load(ckpt)
    ev_settings = copy.copy(settings)
    ev_settings.n_trained = n_trained
    evaluator = Evaluator(solver, args, ev_settings, model_names=model_names)
    os.makedirs(exp + "/eval_folder", exist_ok=True)
    os.makedirs(solver.path + "eval_folder", exist_ok=True)
    evaluator.model.eval()
    max_batches = settings.max_batches
    small = settings.use_validation_set or (settings.debug_mnist and args.choose_data == "mnist")
    if max_batches is None and small:
        max_batches = max(1, 1000 // int(args.batch_size))
    return evaluator, args, exp + "/eval_folder", max_batches


def draw_curve_figures(settings, evaluator):
    """eval_settings.py:128-141, the driver's last step: Evaluator.test_temp_values under --test_temperature, else
    Evaluator.plot_eval_values over all experiments, with --label_names (the experiment names when there are fewer
    labels than experiments).  If a file the figures are read from does not exist (--no-calc_eval), or none of the
    experiments is an RFN run, one line says so and nothing is drawn.  Returns the paths written."""
    experiments = settings.experiment_names
    labels = settings.label_names if len(settings.label_names) >= len(experiments) else experiments
    if settings.test_temperature:
        name = "test_temp_values"
        needed = [settings.folder_path + experiments[0] + "/eval_folder/" + temperature_file_name(T)
                  for T in settings.temperatures]
    else:
        name = "plot_eval_values"
        needed = [settings.folder_path + e + "/eval_folder/evaluations.pt" for e in experiments]
    if "rfn.pt" not in settings.model_path[:len(experiments)]:
        # a run over baselines alone leaves nothing but its values in eval_folder (pinned by tests/test_srnn_eval.py);
        # their curves are drawn when they are compared with an RFN run
        print("eval_settings: the curve figures of %s are not drawn: none of the experiments is an RFN run (rfn.pt)" % name)
        return []
    missing = [p for p in needed if not os.path.exists(p)]
    if missing:
        print("eval_settings: the curve figures of %s are not drawn: %s does not exist" % (name, missing[0]))
        return []
    return getattr(evaluator, name)(settings.folder_path, labels, experiments)


def main(settings):
    experiments = settings.experiment_names
    if len(settings.model_path) < len(experiments):
        raise ValueError("eval_settings: %d experiments but %d --model_path entries" %
                         (len(experiments), len(settings.model_path)))
    if not settings.test_temperature and len(settings.temperatures) < len(experiments):
        raise ValueError("eval_settings: %d experiments but %d --temperatures" %
                         (len(experiments), len(settings.temperatures)))
    for name in settings.model_path[:len(experiments)]:   # before any file is read
        solver_class(name)
        if settings.test_temperature and name != "rfn.pt":
            raise ValueError("eval_settings: --test_temperature with %s: only rfn.pt has a sampling temperature" % name)
    for i in range(len(experiments)):
        model_name = settings.model_path[i]
        rfn = model_name == "rfn.pt"
        evaluator, args, folder, max_batches = build_evaluator(settings, i)
        if not settings.test_temperature:
            T = settings.temperatures[i]
            evaluator.model.temperature = T
            evaluator.model.kl_temperature = 1
            if not rfn:
                print("eval_settings: %s: the RFN-only figures and analyses are skipped (%s)" %
                      (model_name, ", ".join(RFN_ONLY_SHEETS)))
                evaluator.extra_plots = False
            if settings.eval_parameters and rfn:
                image = next(iter(evaluator.test_loader))
                image = image[0] if args.choose_data == "bair" and isinstance(image, (list, tuple)) else image
                out = evaluator.param_analysis(image, settings.n_frames - settings.n_conditions, settings.n_conditions)
                torch.save(dict(zip(PARAM_KEYS, out)), folder + "/param_analysis.pt")
                if args.choose_data == "mnist":
                    evaluator.param_plots(folder, settings.n_conditions)
                else:
                    print("eval_settings: the figures of param_plots need an SM-MNIST run (synchronized Moving MNIST); "
                          "the tensors are in %s/param_analysis.pt" % folder)
            if settings.calc_fvd:
                print("Computing FVD")
                fvd_mean, fvd_std = evaluator.get_fvd_values(model_name, settings.fvd_predicts, max_batches=max_batches)
                print("Done - FVD")
            else:
                fvd_mean, fvd_std = -1, -1
            if rfn:
                evaluator.plot_long_t(model_name)
                evaluator.plot_diversity(model_name)
                evaluator.plot_random_samples(model_name)
                evaluator.plot_temp(model_name, orig_temps=[T, 1], kl_analysis=False)
                evaluator.plot_temp(model_name, orig_temps=[T, 1], kl_analysis=True, duplicate_samples=False)
                evaluator.plot_temp(model_name, orig_temps=[T, 1], kl_analysis=False, duplicate_samples=True,
                                    t_list=[0] * 8)
                evaluator.plot_temp(model_name, orig_temps=[T, 1], kl_analysis=True, duplicate_samples=True,
                                    t_list=[0] * 8)
            if settings.eval_loss:
                bits_mean, bits_std = evaluator.get_loss(model_name, loss_resamples=2, max_batches=max_batches)
            else:
                bits_mean, bits_std = -1, -1
            if settings.calc_eval:
                d = eval_dict(evaluator.get_eval_values(model_name, max_batches=max_batches), T)
                d.update({"FVD_mean": fvd_mean, "FVD_std": fvd_std, "bits_mean": bits_mean, "bits_std": bits_std})
                torch.save(d, folder + "/evaluations.pt")
                write_avg_losses(folder + "/eval_avg_losses.txt", d)
        elif settings.draws_per_pass is not None:
            swept = evaluator.get_eval_values_temperatures(settings.temperatures, model_name, max_batches=max_batches)
            for T in settings.temperatures:
                torch.save(eval_dict(swept[float(T)], T), folder + "/" + temperature_file_name(T))
        else:
            for T in settings.temperatures:
                evaluator.model.temperature = T
                torch.save(eval_dict(evaluator.get_eval_values(model_name, max_batches=max_batches), T),
                           folder + "/" + temperature_file_name(T))
    draw_curve_figures(settings, evaluator)


def add_bool_arg(parser, name, help, default=False):
    group = parser.add_mutually_exclusive_group(required=False)
    group.add_argument("--" + name, dest=name, action="store_true", help=help)
    group.add_argument("--no-" + name, dest=name, action="store_false", help=help)
    parser.set_defaults(**{name: default})


def build_parser():
    p = argparse.ArgumentParser()
    # PATH SETTINGS
    p.add_argument("--folder_path", help="Path to folder that contains the experiments", default="./work1/s146996/",
                   type=str)
    p.add_argument("--experiment_names", nargs="+", help="Name of the experiments to eval", default=["rfn_bair_final"],
                   type=str)
    p.add_argument("--label_names", nargs="+", help="Name of the labels for the eval plots", default=["RFN-BAIR"],
                   type=str)
    p.add_argument("--model_path", nargs="+", help="Name of model.pt file", default=["rfn.pt"], type=str)
    # CALCULATE VALUES SETTINGS
    add_bool_arg(p, "use_validation_set", default=False,
                 help="If true then a validation set (the first 1000 test sequences) is used to tune parameters")
    p.add_argument("--num_samples_to_plot", help="This will create a plot of N sequences", default=3, type=int)
    p.add_argument("--n_frames", help="Specify the sequence length of the test data", default=30, type=int)
    p.add_argument("--start_predictions", help="Specify when model starts predicting", default=5, type=int)
    p.add_argument("--temperatures", nargs="+", help="Specify temperature for the model", default=[0.7], type=float)
    p.add_argument("--resample", help="Loops over the test set more than once to get better measures. WARNING: can be "
                   "slow", default=30, type=int)
    add_bool_arg(p, "extra_plots", default=False, help="Plots the elbo gap of the RFN model and the bits per pixel of "
                 "future frames (KLDdiagnostic.png, bpp_sequence.png) while the eval values are computed")
    # TEST TEMPERATURE
    add_bool_arg(p, "test_temperature", default=False,
                 help="Allows one to test temperature. If enabled different temperatures (from --temperatures) are "
                      "tested for each specified model")
    # DEBUG SETTINGS
    add_bool_arg(p, "debug_mnist", default=True,
                 help="Uses a small test set (1000 sequences) to speed up iterations for debugging. Only works for "
                      "SM-MNIST")
    # EVAL VALUES PLOTTER SETTINGS
    add_bool_arg(p, "calc_eval", default=True, help="Set to false if we do not want to calculate eval values")
    add_bool_arg(p, "debug_plot", default=True,
                 help="Plots num_samples_to_plot samples to make sure the loader and eval works")
    p.add_argument("--n_conditions", help="Number of conditions used for plotting eval_values", default=5, type=int)
    add_bool_arg(p, "eval_parameters", default=False,
                 help="If true then the parameter analysis is run, its tensors are saved and, on SM-MNIST, its "
                      "figures are drawn")
    # FVD settings
    add_bool_arg(p, "calc_fvd", default=False, help="Enabling this allows us to compute FVD (needs --fvd_weights)")
    p.add_argument("--fvd_predicts", help="How far into the future to predict", default=13, type=int)
    # ELBO
    add_bool_arg(p, "eval_loss", default=False, help="Enabling this allows us to evaluate the BPP of the models")
    # additions of this implementation
    p.add_argument("--draws_per_pass", help="Generate this many draws of every sequence per pass, with addressed noise "
                   "(reproducible figures); with --test_temperature the temperatures share the pass", default=None,
                   type=int)
    p.add_argument("--seed", help="Seed of the addressed noise of --draws_per_pass and of the sheets", default=0, type=int)
    p.add_argument("--lpips_weights", nargs="+", help="Directory or files holding the LPIPS-alex weights (nothing is "
                   "downloaded); without it LPIPS entries are None", default=None, type=str)
    p.add_argument("--fvd_weights", nargs="+", help="Directory or files holding the I3D weights for --calc_fvd (nothing "
                   "is downloaded)", default=None, type=str)
    p.add_argument("--max_batches", help="Evaluate at most this many test batches", default=None, type=int)
    return p


def parse_args(argv=None):
    settings = build_parser().parse_args(argv)
    for k in ("lpips_weights", "fvd_weights"):   # one entry: a directory or a file, as the Evaluator takes it
        v = getattr(settings, k)
        if v is not None and len(v) == 1:
            setattr(settings, k, v[0])
    return settings


if __name__ == "__main__":
    main(parse_args())
