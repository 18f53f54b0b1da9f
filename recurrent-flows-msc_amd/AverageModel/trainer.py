"""Solver of the linear-extrapolation baseline: the training loop of averagemodel/averagemodel.py:115-133 of the
reference on the package's loaders (a subclass of the RFN Solver for `create_loaders`, `make_optimizer` and
`read_checkpoint`; the synthetic generator, Stochastic Moving MNIST, BAIR push and KTH with the data flags of
main_svg.py).  The train loader yields sequences of n_conditions + 1 frames, the test loader sequences of --n_frames;
frames reach the model as the loaders deliver them, float32 in [0, 1].  Adam at --learning_rate (1e-3) for --n_epochs (3)
epochs of batches of --batch_size (256); `--max_steps` stops early.  The reference creates a plateau scheduler and never
steps it: there is none here.  Its matplotlib figures of the loop are not drawn.  `<path>model_folder/average.pt`
holds `model_state_dict` and `args`.

One GPU, eager steps."""
import copy
import os

import torch

from RFN.trainer import Solver as RFNSolver
from .averagemodel import SimpleLinearModel

# what the base Solver reads and this driver's parser does not define
_BASE_DEFAULTS = dict(n_bits=8, verbose=False, patience_lr=10, factor_lr=0.2, min_lr=1e-6, patience_es=50, beta_max=0.0,
                      beta_min=0.0, beta_steps=1, preprocess_range="none", preprocess_scale=255, multigpu=False,
                      scheduler_type="none", use_validation_set=False, num_workers=4, image_size=64, digit_size=28,
                      step_length=4, num_digits=2)


class Solver(RFNSolver):
    checkpoint_names = ("average.pt",)

    def __init__(self, args):
        if getattr(args, "multigpu", False) or int(os.environ.get("WORLD_SIZE", 1)) > 1:
            raise NotImplementedError("the linear-extrapolation baseline trains on one GPU")
        base = copy.copy(args)
        for k, v in _BASE_DEFAULTS.items():
            if not hasattr(base, k):
                setattr(base, k, v)
        super().__init__(base)
        self.base_args = base
        self.args = args          # what the checkpoint stores
        self.n_frames_test = int(args.n_frames)

    def build(self):
        # the same datasets at two sequence lengths: n_conditions + 1 frames to train on, --n_frames to evaluate on
        self.args, own = self.base_args, self.args    # (create_loaders reads self.args: the one with every data flag)
        try:
            self.n_frames = self.n_conditions + 1
            self.train_loader, _ = self.create_loaders()
            self.n_frames = self.n_frames_test
            _, self.test_loader = self.create_loaders()
        finally:
            self.args = own
        os.makedirs(self.path + "model_folder", exist_ok=True)
        os.makedirs(self.path + "eval_folder", exist_ok=True)
        self.model = self.make_model().to(self.device)
        self.optimizer = self.make_optimizer(self.model.parameters(), self.learning_rate)
        self.counter, self.stop = 0, False

    def make_model(self):
        return SimpleLinearModel(num_cond_frames=self.n_conditions)

    def batch(self, image):
        """a loader's item as a device tensor [B, T, C, H, W] (the file-backed BAIR loader of the reference yields a list)"""
        image = image[0] if isinstance(image, (list, tuple)) else image
        return image.to(self.device, non_blocking=True)

    def train_step(self, image):
        """averagemodel.py:129-133: one Adam step on a resident batch; the loss stays on the device"""
        loss = self.model(image)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        self.counter += 1
        return loss.detach()

    def train(self):
        max_steps = getattr(self.args, "max_steps", 0)
        for _ in range(self.n_epochs):
            self.model.train()
            if hasattr(self.train_loader, "set_epoch"):
                self.train_loader.set_epoch(self.epoch_i)
            self.epoch_i += 1
            epoch = []
            for image in self.train_loader:
                epoch.append(self.train_step(self.batch(image)))
                if max_steps and self.counter >= max_steps:
                    self.stop = True
                    break
            if epoch:   # one device->host read per epoch
                self.losses += torch.stack(epoch).tolist()
            self.checkpoint(self.checkpoint_names[0])
            if self.stop:
                break

    def checkpoint(self, model_name="average.pt"):
        torch.save({"model_state_dict": self.model.state_dict(), "args": self.args, "losses": self.losses,
                    "epoch": self.epoch_i}, self.path + "model_folder/" + model_name)

    def load(self, load_model):
        self.model.load_state_dict(load_model["model_state_dict"])
        self.losses = list(load_model.get("losses", []))
        self.epoch_i = int(load_model.get("epoch", 0))
        self.model.to(self.device)
        return self.epoch_i

    def capture_graph(self, example_image, static_draws=None):
        raise NotImplementedError("the linear-extrapolation baseline has no captured-graph step: eager steps only")

    def plotter(self):
        raise NotImplementedError("sample sheets of the linear-extrapolation baseline are not implemented")

