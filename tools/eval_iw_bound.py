#!/usr/bin/env python3
"""RFN bits/dim under the importance-weighted bound, beside the single-sample ELBO:

    python tools/eval_iw_bound.py --iw_samples 20 --chains_per_pass 20 \
        --folder_path ./runs/ --experiment_names my_run --n_frames 30 --seed 1 --max_batches 10

--iw_samples K and --chains_per_pass P are this tool's own flags; every other argument goes to
evaluation_metrics/eval_settings.py's parser unchanged (its parser has no flag for the two settings).  Each experiment
is loaded as eval_settings.main loads it (build_evaluator: nothing from the checkpoint is executed), and two figures are
computed on the frames the run was trained on: Evaluator.get_loss as it stands (RFN.loss, one ELBO sample per batch from
torch's generator) and Evaluator.get_loss with settings.rfn_iw_samples = K (RFN.elbo_importance_weighting: K chains per
sequence with addressed noise under --seed, P chains per pass).  The lines are printed and written
to `<folder_path><experiment>/eval_folder/iw_bits_per_dim.txt`.  RFN checkpoints only: the baselines' get_loss is the
importance-weighted bound already."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))


def split_args(argv=None):
    """(K, P, the remaining arguments): this tool's flags taken out, the driver's left in their order"""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--iw_samples", type=int, default=20, help="K: chains per sequence of the importance-weighted bound")
    p.add_argument("--chains_per_pass", type=int, default=None, help="P: chains per pass (default: all K)")
    own, rest = p.parse_known_args(argv)
    if own.iw_samples < 1:
        p.error("--iw_samples must be at least 1")
    if own.chains_per_pass is not None and own.chains_per_pass < 1:
        p.error("--chains_per_pass must be at least 1")
    return own.iw_samples, own.chains_per_pass, rest


def parse_args(argv=None):
    """the driver's settings object with rfn_iw_samples and iw_chains_per_pass set on it"""
    from evaluation_metrics import eval_settings
    K, P, rest = split_args(argv)
    settings = eval_settings.parse_args(rest)
    settings.rfn_iw_samples, settings.iw_chains_per_pass = K, P
    return settings


def report_lines(experiment, elbo, iw, K, P, seed):
    return ["experiment: %s" % experiment,
            "ELBO bits/dim (RFN.loss, one sample): %.6f" % elbo,
            "IW bits/dim (K = %d): %.6f" % (K, iw),
            "K: %d  chains_per_pass: %s  seed: %d" % (K, "K" if P is None else P, seed)]


def main(settings):
    from evaluation_metrics import eval_settings
    if len(settings.model_path) < len(settings.experiment_names):
        raise ValueError("eval_iw_bound: %d experiments but %d --model_path entries" %
                         (len(settings.experiment_names), len(settings.model_path)))
    for i, experiment in enumerate(settings.experiment_names):
        if settings.model_path[i] != "rfn.pt":
            raise ValueError("eval_iw_bound: %s: the K-chain bound of this tool is RFN's (rfn.pt)" % settings.model_path[i])
        evaluator, args, folder, max_batches = eval_settings.build_evaluator(settings, i)
        K, evaluator.rfn_iw_samples = evaluator.rfn_iw_samples, 0
        elbo, _ = evaluator.get_loss("rfn.pt", max_batches=max_batches)
        evaluator.rfn_iw_samples = K
        iw, _ = evaluator.get_loss("rfn.pt", max_batches=max_batches)
        lines = report_lines(experiment, float(elbo), float(iw), K, evaluator.iw_chains_per_pass, evaluator.seed)
        print("\n".join(lines))
        with open(os.path.join(folder, "iw_bits_per_dim.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
    main(parse_args())
