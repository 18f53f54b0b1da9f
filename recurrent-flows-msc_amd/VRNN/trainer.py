"""Solver of the VRNN baseline (VRNN/trainer.py of the reference) as a subclass of the SRNN Solver: the reference's two
trainers share `preprocess`, `compute_loss`, the checkpoint dict and the plateau scheduler stepped after every epoch
(tests/golden/vrnn.pt records the VRNN trainer's own arithmetic), so only the model class and the checkpoint names
(`vrnn.pt`, `vrnn_best_model.pt`) are overridden here.

Eager steps only: a captured-graph step and data parallelism are refused with a message, not half supported."""
import os

from SRNN.trainer import Solver as SRNNSolver
from .VRNN import VRNN


class Solver(SRNNSolver):
    checkpoint_names = ("vrnn.pt", "vrnn_best_model.pt")

    def __init__(self, args):
        if getattr(args, "multigpu", False) or int(os.environ.get("WORLD_SIZE", 1)) > 1:
            raise NotImplementedError("the VRNN baseline trains on one GPU: --multigpu / several ranks are not supported")
        super().__init__(args)

    def make_model(self):
        return VRNN(self.args)

    def capture_graph(self, example_image, static_draws=None):
        raise NotImplementedError("the VRNN baseline has no captured-graph step: eager steps only")

    def plotter(self):
        raise NotImplementedError("sample sheets of the VRNN baseline are not implemented")
