"""Solver of the SRNN baseline (SRNN/trainer.py of the reference) as a subclass of the package's RFN Solver: the two
trainers of the reference differ in a few places only, and only those are overridden here — the model class, a loss of
two values, `compute_loss(nll, kl, dims, t)`, SRNN's `preprocess` with its own "1.0" and "minmax" ranges, the checkpoint
names and keys (`srnn.pt`, `srnn_best_model.pt`), and the plateau scheduler stepped after every epoch.  Loaders, the
device datasets, the optimizer (HipAdam) and the epoch loop are the base class's.

Eager steps only: a captured-graph step and data parallelism are refused with a message, not half supported."""
import copy
import os

import numpy as np
import torch

from RFN.trainer import Solver as RFNSolver
from .SRNN import SRNN


class Solver(RFNSolver):
    checkpoint_names = ("srnn.pt", "srnn_best_model.pt")

    def __init__(self, args):
        if getattr(args, "multigpu", False) or int(os.environ.get("WORLD_SIZE", 1)) > 1:
            raise NotImplementedError("the SRNN baseline trains on one GPU: --multigpu / several ranks are not supported")
        base = copy.copy(args)
        base.scheduler_type = "plateau"   # (SRNN/trainer.py:252: the plateau scheduler steps after every epoch)
        super().__init__(base)
        self.args = args                  # what the checkpoint stores: the reference's own Namespace

    def make_model(self):
        return SRNN(self.args)

    # ---------------------------------------------------------------------------------------------- arithmetic
    def preprocess(self, x, reverse=False):
        """SRNN/trainer.py:160-191."""
        n_bins = 2 ** self.n_bits
        rng = self.preprocess_range
        if rng == "0.5":
            if not reverse:
                x = x * self.preprocess_scale
                if self.n_bits < 8:
                    x = torch.floor(x / 2 ** (8 - self.n_bits))
                return x / n_bins - 0.5
            x = (x + 0.5) * n_bins
            return torch.clamp(torch.floor(x) * (256. / n_bins), 0, 255).byte()
        if rng == "1.0":
            if not reverse:
                return x * 2 - 1
            x = (x + 1) / 2 * n_bins
            return torch.clamp(torch.floor(x) * (256. / n_bins), 0, 255).byte()
        if rng == "minmax":
            if not reverse:
                return (x - x.min()) / (x.max() - x.min())
            x = x * (x.max() - x.min()) + x.min()
            return torch.clamp(x * 255, 0, 255).byte()
        raise ValueError("Invalid preprocess choice %r" % (rng,))

    def compute_loss(self, nll, kl, dims, t=1):
        """SRNN/trainer.py:193-206 — loss = nll + β·kl ; bits/dim = (kl+nll)/(ln2 · C·H·W · t)."""
        loss = nll + self.beta * kl
        kl_store, nll_store = kl.detach(), nll.detach()
        bits = (kl_store + nll_store) / (np.log(2.) * float(np.prod(list(dims))) * t)
        self._log_step(float(bits), float(loss.detach()) / t, float(kl_store) / t, float(nll_store) / t)
        return loss

    # ---------------------------------------------------------------------------------------------- loop
    def train_step(self, image):
        """one eager optimizer step on a resident [B,T,C,H,W] batch in [0,1] (SRNN/trainer.py:223-236)."""
        self.beta = min(self.beta_max, self.beta_min + self.counter * (self.beta_max - self.beta_min) / self.beta_steps)
        image = self.preprocess(image)
        kl, nll = self.model.loss(image)
        loss = self.compute_loss(nll, kl, image.shape[2:], t=image.shape[1] - 1)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer_step()
        self.counter += 1
        return loss

    def capture_graph(self, example_image, static_draws=None):
        raise NotImplementedError("the SRNN baseline has no captured-graph step: eager steps only")

    def plotter(self):
        raise NotImplementedError("sample sheets of the SRNN baseline are not implemented")

    # ---------------------------------------------------------------------------------------------- state
    def checkpoint(self, model_name, epoch, loss):
        """the reference's dict (SRNN/trainer.py:259-272)"""
        torch.save({"epoch": epoch, "model_state_dict": self.model.state_dict(),
                    "optimizer_state_dict": self.optimizer.state_dict(), "loss": loss, "kl_loss": self.kl_loss,
                    "recon_loss": self.recon_loss, "losses": self.losses, "bits": self.bits,
                    "plot_counter": self.plot_counter, "annealing_counter": self.counter, "args": self.args},
                   self.path + "model_folder/" + model_name)

    def load(self, load_model):
        self.model.load_state_dict(load_model["model_state_dict"])
        self.optimizer.load_state_dict(load_model["optimizer_state_dict"])
        self.epoch_i += load_model["epoch"]
        loss = load_model["loss"]
        self.kl_loss, self.recon_loss = load_model["kl_loss"], load_model["recon_loss"]
        self.losses, self.bits = load_model["losses"], load_model["bits"]
        self.plot_counter, self.counter = load_model["plot_counter"], load_model["annealing_counter"]
        self.best_loss = loss
        self.model.to(self.device)
        return self.epoch_i, loss
