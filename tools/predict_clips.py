#!/usr/bin/env python3
"""The draws of a trained model as an animated PNG, next to the ground truth, their mean and their spread:

    python tools/predict_clips.py --folder_path ./runs/ --experiment_names my_run --model_path rfn.pt \
        --n_frames 30 --start_predictions 5 --draws 8 --show_draws 6 --sequences 4 --temperature 0.7 --seed 0

For every experiment it loads `<folder_path><experiment>/model_folder/<model_path[i]>` through the checkpoint's own
Solver (rfn.pt, srnn.pt, vrnn.pt or svg.pt: this tool keeps its own table, so the two baselines the evaluation driver
does not take get a visual output here) as eval_settings.build_evaluator does -- nothing from the file is executed --
takes the first test batch of --n_frames frames and generates --draws draws of every sequence with addressed noise
(`_predict_draws_device` under --seed: the clip is reproducible byte for byte; --temperature is set on RFN only, the
baselines have none).  Frames become bytes by the Solver's own preprocess(reverse=True).  The clip has one row for each
of the first --sequences sequences and the columns ground truth | the first --show_draws draws | MEAN | SPREAD of all
--draws (--gain times the standard deviation of the bytes), composed in one launch (rfn_hip.ops.compose_clip, DESIGN.md
section 28).  The --start_predictions given frames are shown in every draw column inside a green ring, so the spread is
black until the ring turns red and generation starts.  Written to `<folder_path><experiment>/eval_folder/clips.png`
(APNG: a viewer that does not know it shows frame 0); the path is printed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))

SOLVERS = {"rfn.pt": "RFN.trainer", "srnn.pt": "SRNN.trainer", "vrnn.pt": "VRNN.trainer", "svg.pt": "SVG.trainer"}


def solver_class(model_name):
    """the Solver of a checkpoint name: all four models of the package"""
    if model_name not in SOLVERS:
        raise ValueError("predict_clips: cannot load %r: the checkpoints are %s" % (model_name, ", ".join(sorted(SOLVERS))))
    import importlib
    return importlib.import_module(SOLVERS[model_name]).Solver


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--folder_path", help="Path to folder that contains the experiments", default="./runs/", type=str)
    p.add_argument("--experiment_names", nargs="+", help="Name of the experiments", default=["rfn_bair_final"], type=str)
    p.add_argument("--model_path", nargs="+", help="Name of each experiment's checkpoint: " + ", ".join(sorted(SOLVERS)),
                   default=["rfn.pt"], type=str)
    p.add_argument("--n_frames", help="Frames of the clip: given and generated together", default=30, type=int)
    p.add_argument("--start_predictions", help="Number of given frames", default=5, type=int)
    p.add_argument("--draws", help="Draws of every sequence (MEAN and SPREAD run over all of them)", default=8, type=int)
    p.add_argument("--show_draws", help="How many of the draws get a column", default=6, type=int)
    p.add_argument("--sequences", help="Rows: the first sequences of the first test batch", default=4, type=int)
    p.add_argument("--temperature", help="Sampling temperature (RFN only)", default=0.7, type=float)
    p.add_argument("--seed", help="Seed of the addressed noise", default=0, type=int)
    p.add_argument("--zoom", help="Pixels per source pixel", default=2, type=int)
    p.add_argument("--delay_ms", help="Milliseconds per frame", default=100, type=int)
    p.add_argument("--gain", help="SPREAD shows this many times the standard deviation", default=4, type=int)
    return p


def parse_args(argv=None):
    p = build_parser()
    s = p.parse_args(argv)
    if len(s.model_path) < len(s.experiment_names):
        p.error("%d experiments but %d --model_path entries" % (len(s.experiment_names), len(s.model_path)))
    if not 1 <= s.start_predictions < s.n_frames:
        p.error("need 1 <= --start_predictions < --n_frames")
    if s.draws < 1 or not 0 <= s.show_draws <= s.draws or s.sequences < 1:
        p.error("need --draws >= 1, 0 <= --show_draws <= --draws and --sequences >= 1")
    return s


def load_solver(settings, i):
    """the Solver of experiment i, rebuilt from the stored arguments on one rank with test sequences of
    settings.n_frames frames, weights loaded, model in eval mode (the steps of eval_settings.build_evaluator)"""
    Solver = solver_class(settings.model_path[i])
    exp = settings.folder_path + settings.experiment_names[i]
    ckpt = Solver.read_checkpoint(exp + "/model_folder/" + settings.model_path[i])
    args = Solver.args_for_world(ckpt, 1)
    args.n_frames = settings.n_frames
    solver = Solver(args)
    solver.build()
    solver.load(ckpt)
    solver.model.eval()
    return solver, args, exp + "/eval_folder"


def clip_frames(solver, image, start, n_frames, draws, seed):
    """(truth uint8 [B, T, C, H, W], draws uint8 [D, B, T, C, H, W]) on the device, T = n_frames: every draw holds the
    `start` given frames followed by its generated ones; `image` is a preprocessed batch [B, >= T, C, H, W]"""
    import torch
    _, pred = solver.model._predict_draws_device(image, n_frames - start, start, draws, seed)
    truth = solver.preprocess(image[:, :n_frames], reverse=True)
    pred = solver.preprocess(pred, reverse=True).permute(1, 2, 0, 3, 4, 5)   # [n, D, B, ...] -> [D, B, n, ...]
    given = truth[:, :start].unsqueeze(0).expand((draws,) + tuple(truth[:, :start].shape))
    return truth, torch.cat((given, pred), dim=2).contiguous()


def main(settings):
    import torch
    from evaluation_metrics.error_metrics import Evaluator
    from rfn_hip import ops
    from Utils.png import write_apng
    paths = []
    for i, experiment in enumerate(settings.experiment_names):
        torch.manual_seed(settings.seed)   # a loader that shuffles does so with torch's generator
        solver, args, folder = load_solver(settings, i)
        if settings.model_path[i] == "rfn.pt":
            solver.model.temperature = settings.temperature
        image = next(iter(solver.test_loader))
        image = image[0] if getattr(args, "choose_data", "mnist") == "bair" and isinstance(image, (list, tuple)) else image
        # the baselines' strided (de)convolutions are torch modules whose default algorithms add split-K slices with
        # float atomics: the same seed is to give the same file
        deterministic, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
        try:
            with torch.no_grad():
                image = solver.preprocess(image.to(solver.device))
                truth, full = clip_frames(solver, image, settings.start_predictions, settings.n_frames, settings.draws,
                                          settings.seed)
        finally:
            torch.backends.cudnn.deterministic = deterministic
        rows = min(settings.sequences, int(truth.shape[0]))
        # the layout of Evaluator.plot_clips, with a column for the first --show_draws draws only
        cells = Evaluator.clip_cells(full, truth, rows, settings.start_predictions, settings.gain, show=settings.show_draws)
        clip = ops.compose_clip(cells, settings.n_frames, zoom=settings.zoom, border=2, scanlines=True)
        os.makedirs(folder, exist_ok=True)
        paths.append(os.path.join(folder, "clips.png"))
        write_apng(paths[-1], clip, delay_ms=settings.delay_ms)
        print(paths[-1])
    return paths


if __name__ == "__main__":
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
    main(parse_args())
