"""Solver of the SVG baseline (SVG/trainer.py of the reference) as a subclass of the SRNN Solver, as VRNN's is: the
reference's trainers share `compute_loss`, the checkpoint dict and the plateau scheduler stepped after every epoch
(tests/golden/svg.pt records the SVG trainer's own arithmetic).  Overridden here: the model class, the checkpoint names
(`svg.pt`, `svg_best_model.pt`) and `preprocess`, which in the SVG trainer has its own "1.0" range (x scale / 2^bits, not
SRNN's 2x - 1) and a fourth range, "none", the parser's default.

Eager steps only: a captured-graph step and data parallelism are refused with a message, not half supported."""
import os

import torch

from SRNN.trainer import Solver as SRNNSolver
from .SVG import SVG


class Solver(SRNNSolver):
    checkpoint_names = ("svg.pt", "svg_best_model.pt")

    def __init__(self, args):
        if getattr(args, "multigpu", False) or int(os.environ.get("WORLD_SIZE", 1)) > 1:
            raise NotImplementedError("the SVG baseline trains on one GPU: --multigpu / several ranks are not supported")
        super().__init__(args)

    def make_model(self):
        return SVG(self.args)

    def preprocess(self, x, reverse=False):
        """SVG/trainer.py:160-198."""
        n_bins = 2 ** self.n_bits
        rng = self.preprocess_range
        if rng in ("0.5", "1.0"):
            if not reverse:
                x = x * self.preprocess_scale
                if self.n_bits < 8:
                    x = torch.floor(x / 2 ** (8 - self.n_bits))
                x = x / n_bins
                return x - 0.5 if rng == "0.5" else x
            if rng == "0.5":
                x = x + 0.5
            return torch.clamp(torch.floor(x * n_bins) * (256. / n_bins), 0, 255).byte()
        if rng == "minmax":
            if not reverse:
                return (x - x.min()) / (x.max() - x.min())
            x = x * (x.max() - x.min()) + x.min()
            return torch.clamp(x * 255, 0, 255).byte()
        if rng == "none":
            return x if not reverse else torch.clamp(x * 255, 0, 255).byte()
        raise ValueError("Invalid preprocess choice %r" % (rng,))

    def capture_graph(self, example_image, static_draws=None):
        raise NotImplementedError("the SVG baseline has no captured-graph step: eager steps only")

    def plotter(self):
        raise NotImplementedError("sample sheets of the SVG baseline are not implemented")
