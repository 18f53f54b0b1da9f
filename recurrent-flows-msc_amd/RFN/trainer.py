"""Solver — training driver with the reference's surface (RFN/trainer.py of the reference): `Solver(args).build();
.train(); .load(ckpt)`, `preprocess`, `compute_loss` (bits/dim bookkeeping), β annealing, linear LR decay, checkpoint
dict layout.  `plotter` writes the reference's sheet of frames (ground truth, samples, predictions, reconstructions,
bijection check of one test sequence) as `png_folder/samples<k>.png`, composed on the GPU in one launch and encoded
with zlib: pixels only, no matplotlib, no titles, no loss-curve panel; `--plot_every N` calls it after every N-th
epoch (default: never).  A synthetic SM-MNIST-shaped loader is built in (`--synthetic_data`); otherwise the dataset lives on the GPU: Stochastic Moving MNIST is rendered from local
MNIST files (`--choose_data mnist`, data_generators/moving_mnist.py), BAIR push and KTH clips are gathered from their
packed frames (`bair`, `kth`; data_generators/clips.py).  Multi-GPU = one process per GPU (rfn_hip/dist.py)."""
import contextlib
import math
import os

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader

from data_generators import SyntheticMovingMNIST
from rfn_hip import dist as rdist
from Utils import set_gpu
from .RFN_new import RFN


class EarlyStopping:
    """RFN/trainer.py:18-44."""

    def __init__(self, min_delta=0, patience=50, verbose=True):
        self.min_delta, self.patience, self.verbose = min_delta, patience, verbose
        self.wait, self.best_loss, self.stop_training = 0, 1e15, False

    def step(self, epoch, loss):
        if loss is None:
            return False
        if (loss - self.best_loss) < -self.min_delta:
            self.best_loss, self.wait = loss, 1
            return False
        if self.wait >= self.patience:
            self.stop_training = True
            if self.verbose:
                print("STOP! Criterion met at epoch %d" % epoch)
            return True
        self.wait += 1
        return False


class Solver(object):
    # what a sibling trainer (SRNN/trainer.py) replaces: the checkpoint files of train() and the model of build()
    checkpoint_names = ("rfn.pt", "rfn_best_model.pt")

    def __init__(self, args):
        self.args = args
        for k in ("n_bits", "n_epochs", "learning_rate", "verbose", "batch_size", "patience_lr", "factor_lr", "min_lr",
                  "patience_es", "beta_max", "beta_min", "beta_steps", "choose_data", "n_frames", "digit_size",
                  "step_length", "num_digits", "image_size", "preprocess_range", "preprocess_scale", "num_workers",
                  "multigpu", "n_predictions", "n_conditions", "scheduler_type", "use_validation_set"):
            setattr(self, k, getattr(args, k))
        self.path = str(os.path.abspath(os.getcwd())) + args.path
        self.plot_counter, self.epoch_i, self.counter = 0, 0, 0
        self.losses, self.kl_loss, self.recon_loss, self.bits = [], [], [], []
        self.best_loss, self.beta, self.stop = 1e15, args.beta_min, False
        # the guard of the optimizer step (Namespaces saved before these flags existed do not have them: all off)
        self.grad_clip_norm = float(getattr(args, "grad_clip_norm", 0.0) or 0.0)
        self.skip_nonfinite_steps = bool(getattr(args, "skip_nonfinite_steps", False))
        self.max_skipped_steps = int(getattr(args, "max_skipped_steps", 100))
        self.guard_on = self.grad_clip_norm > 0.0 or self.skip_nonfinite_steps
        self._host_guard = {"grad_norm": 0.0, "scale": 1.0, "skipped_steps": 0}   # CPU parameters only
        self._guard_last, self._skipped_before_epoch = None, 0
        # Polyak average of the weights (0 = off; Namespaces saved before the flag existed do not have it)
        self.ema_decay = float(getattr(args, "ema_decay", 0.0) or 0.0)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError("--ema_decay must be in [0, 1) (0 = no average), got %r" % (self.ema_decay,))
        self.rank = int(os.environ.get("RANK", 0))
        self.world = int(os.environ.get("WORLD_SIZE", 1))
        self.device = set_gpu(True)

    # ---------------------------------------------------------------------------------------------- setup
    def build(self):
        if self.multigpu and self.world > 1 and not dist.is_initialized():
            local = int(os.environ.get("LOCAL_RANK", 0))
            if torch.cuda.is_available():
                if os.environ.get("RFN_SINGLE_GPU"):
                    local = 0
                torch.cuda.set_device(local)
                self.device = torch.device("cuda", local)
            # (RFN_DIST_BACKEND=gloo: rehearsal with several ranks on one GPU, as in bench.py and the tests)
            dist.init_process_group(os.environ.get("RFN_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo"))
        self.train_loader, self.test_loader = self.create_loaders()
        if self.rank == 0:
            os.makedirs(self.path + "png_folder", exist_ok=True)
            os.makedirs(self.path + "model_folder", exist_ok=True)
        self.model = self.make_model().to(self.device)
        rdist.broadcast_module_state(self.model)
        self.reducer = rdist.GradBucketReducer(list(self.model.named_parameters()))
        self.optimizer = self.make_optimizer(self.model.parameters(), self.learning_rate, **self.guard_kwargs(),
                                             ema_decay=self.ema_decay)
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, "min", patience=self.patience_lr,
                                                                    factor=self.factor_lr, min_lr=self.min_lr)
        self.earlystopping = EarlyStopping(min_delta=0, patience=self.patience_es, verbose=self.verbose)
        self.counter, self.stop = 0, False

    def make_model(self):
        return RFN(self.args)

    def guard_kwargs(self):
        """the guard's keywords for `make_optimizer`, from --grad_clip_norm / --skip_nonfinite_steps; the batch-sharded
        initial states are the tensors whose gradients are rank-local"""
        return dict(max_grad_norm=self.grad_clip_norm, skip_nonfinite=self.skip_nonfinite_steps,
                    rank_local=tuple(self.reducer.sharded))

    @staticmethod
    def make_optimizer(params, lr, max_grad_norm=0.0, skip_nonfinite=False, rank_local=(), group=None, ema_decay=0.0):
        """RFN/trainer.py:96: Adam with torch's defaults.  On the GPU the whole update is one launch of the HIP kernel
        (rfn_hip.optim.HipAdam, same state layout as torch.optim.Adam) and the guard, when asked for, runs in front of it
        on the device; CPU parameters only occur in host-logic tests, where torch.optim.Adam steps and
        `Solver.optimizer_step` guards it with a few torch ops.  `ema_decay` > 0 keeps the Polyak average of the weights
        in state[p]["ema"]: inside HipAdam's launch, or (CPU parameters) by `Solver.optimizer_step`."""
        ema_decay = float(ema_decay)
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError("ema_decay must be in [0, 1) (0 = no average), got %r" % (ema_decay,))
        params = list(params)
        if params and params[0].is_cuda:
            from rfn_hip.optim import HipAdam
            return HipAdam(params, lr=lr, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                           rank_local=rank_local, group=group, ema_decay=ema_decay)
        opt = torch.optim.Adam(params, lr=lr)
        if ema_decay > 0.0:
            opt.ema_decay = ema_decay   # (what rfn_hip.dist reads to treat "ema" like the moments)
        return opt

    @staticmethod
    def ema_step_decay(decay, n):
        """d_n of a tensor's n-th applied step: the warm-up min(d, (1 + n) / (10 + n)) keeps the first averages from
        being dominated by the initial weights"""
        return min(float(decay), (1.0 + n) / (10.0 + n))

    def create_loaders(self):
        if not getattr(self.args, "synthetic_data", False):
            if self.choose_data == "mnist":
                return self.create_mnist_loaders()
            if self.choose_data == "folder":
                return self.create_folder_loaders()
            return self.create_clip_loaders()
        c = self.args.x_dim[1]
        mk = lambda seed: SyntheticMovingMNIST(seq_len=self.n_frames, image_size=self.image_size,
                                               digit_size=self.digit_size, num_digits=self.num_digits,
                                               step_length=self.step_length, channels=c,
                                               seed=seed * self.world + self.rank)
        kw = dict(batch_size=self.batch_size, num_workers=self.num_workers, shuffle=True, drop_last=True)
        return DataLoader(mk(0), **kw), DataLoader(mk(1), **kw)

    def create_mnist_loaders(self):
        """RFN/trainer.py:112-131, :155-161: Stochastic Moving MNIST (deterministic=False, normalize=False) rendered on
        the GPU from the MNIST files under --mnist_root (default "Mnist", relative to the working directory, like the
        reference).  One channel, or three copies when x_dim asks for 3.  With --use_validation_set the train split
        is its first 500 sequences per epoch.  Every rank renders its own rows of each global batch; the test split is
        the same set of sequences on every evaluation."""
        from data_generators import MovingMNIST, MovingMNISTLoader
        c = self.args.x_dim[1]
        if c not in (1, 3):
            raise ValueError("Stochastic Moving MNIST has 1 or 3 (replicated) channels; x_dim asks for %d" % c)
        root = getattr(self.args, "mnist_root", "Mnist")   # (Namespaces saved before these flags existed)
        seed = getattr(self.args, "data_seed", 0)
        mk = lambda train, length=None: MovingMNIST(train, root, seq_len=self.n_frames, num_digits=self.num_digits,
                                                    image_size=self.image_size, digit_size=self.digit_size,
                                                    deterministic=False, three_channels=c == 3,
                                                    step_length=self.step_length, normalize=False, seed=seed,
                                                    device=self.device, length=length)
        trainset = mk(True, 500 if self.use_validation_set else None)
        testset = mk(False)
        return (MovingMNISTLoader(trainset, self.batch_size, self.rank, self.world),
                MovingMNISTLoader(testset, self.batch_size, self.rank, self.world))

    def create_clip_loaders(self):
        """RFN/trainer.py:132-161: BAIR push (`<root>/{train,test}/traj_*/*/*.png`) or KTH (`<root>/processed/...`) from
        --data_root (default, as the reference: bair_robot_data/processed_data/ or kth_data under the working
        directory).  The frames of each split are packed once into a device-resident store (kept under --data_cache
        while the files match) and every batch is one launch of the clip-gather kernel.  x_dim must agree with the
        frames: 3 channels for BAIR, 1 or 3 (copies) for KTH, H = W = the stored side.  With --use_validation_set
        the train split is its first 500 sequences, as the reference's Subset."""
        from data_generators import KTH, ClipLoader, PushDataset
        bair = self.choose_data == "bair"
        root = getattr(self.args, "data_root", None)   # (Namespaces saved before these flags existed)
        cache_dir = getattr(self.args, "data_cache", None)
        seed = getattr(self.args, "data_seed", 0)
        if root is None:
            root = os.path.join(os.path.abspath(os.getcwd()), "bair_robot_data/processed_data/" if bair else "kth_data")
            if not os.path.isdir(root):
                raise RuntimeError("%s data not found at %s (nothing is downloaded): pass --data_root, or "
                                   "--synthetic_data for SM-MNIST-shaped synthetic video" %
                                   ("BAIR" if bair else "KTH", root))
        elif not os.path.isdir(root):
            raise FileNotFoundError("--data_root %s is not a directory" % root)
        _, c, h, w = self.args.x_dim
        if h != w or c not in ((3,) if bair else (1, 3)):
            raise ValueError("%s frames are square with %s channels; x_dim asks for %dx%dx%d" %
                             ("BAIR" if bair else "KTH", "3" if bair else "1 (or 3 copies)", c, h, w))
        if not bair and h != self.image_size:
            raise ValueError("KTH frames are image_size = %d wide; x_dim asks for %d" % (self.image_size, h))
        length = 500 if self.use_validation_set else None
        cache = lambda name: None if cache_dir is None else os.path.join(cache_dir, "%s_%dx%d" % (name, h, w))
        if bair:
            mk = lambda split, length=None: PushDataset(split=split, dataset_dir=root, seq_len=self.n_frames, img_side=h,
                                                        seed=seed, device=self.device, cache=cache("bair_" + split),
                                                        length=length)
            trainset, testset = mk("train", length), mk("test")
        else:
            mk = lambda train, length=None: KTH(train=train, data_root=root, seq_len=self.n_frames, image_size=h,
                                                seed=seed, device=self.device, channels=c, length=length,
                                                cache=cache("kth_" + ("train" if train else "test")))
            trainset, testset = mk(True, length), mk(False)
        return (ClipLoader(trainset, self.batch_size, self.rank, self.world),
                ClipLoader(testset, self.batch_size, self.rank, self.world))

    def create_folder_loaders(self):
        """`--choose_data folder`: any tree of frame directories and .npy sequences under
        --data_root/{train,test} (data_generators/clip_folder.py).  x_dim's C, H, W is the target geometry (1 or 3
        channels, non-square allowed): frames of another size are resampled on the GPU once, over the window of
        --resize_mode, and the packed store is kept under --data_cache while the files match.  --frame_step is the
        distance between two frames of a clip; --augment flip / reverse switch the mirror and time-reversal bits of
        the train split on.  With --use_validation_set the train split has 500 clips per epoch."""
        from data_generators import ClipFolder, ClipLoader
        root = getattr(self.args, "data_root", None)
        if root is None:
            raise ValueError("--choose_data folder needs --data_root: the directory holding train/ and test/ (nothing is "
                             "searched for or downloaded)")
        if not os.path.isdir(root):
            raise FileNotFoundError("--data_root %s is not a directory" % root)
        cache_dir = getattr(self.args, "data_cache", None)
        step = getattr(self.args, "frame_step", 1)   # (Namespaces saved before these flags existed)
        augment = list(getattr(self.args, "augment", None) or [])
        mode = getattr(self.args, "resize_mode", "crop")
        _, c, h, w = self.args.x_dim
        cache = lambda split: None if cache_dir is None else os.path.join(
            cache_dir, "folder_%s_%dx%dx%d_%s" % (split, h, w, c, mode))
        mk = lambda train, length=None: ClipFolder(
            train, root, seq_len=self.n_frames, channels=c, height=h, width=w, step=step, flip="flip" in augment,
            reverse="reverse" in augment, resize_mode=mode, seed=getattr(self.args, "data_seed", 0), device=self.device,
            cache=cache("train" if train else "test"), length=length)
        trainset, testset = mk(True, 500 if self.use_validation_set else None), mk(False)
        return (ClipLoader(trainset, self.batch_size, self.rank, self.world),
                ClipLoader(testset, self.batch_size, self.rank, self.world))

    # ---------------------------------------------------------------------------------------------- arithmetic
    def preprocess(self, x, reverse=False):
        """RFN/trainer.py:165-188."""
        n_bins = 2 ** self.n_bits
        if not reverse:
            x = x * self.preprocess_scale
            if self.n_bits < 8:
                x = torch.floor(x / 2 ** (8 - self.n_bits))
            x = x / n_bins
            return x - 0.5 if self.preprocess_range == "0.5" else x
        if self.preprocess_range == "0.5":
            x = x + 0.5
        x = x * n_bins
        return torch.clamp(torch.floor(x) * (256. / n_bins), 0, 255).byte()

    def adjust_learning_rate(self, batch):
        """RFN/trainer.py:190-204 — linear decay to zero over 150k steps after step 100k."""
        startbatch, num_steps = 100000, 150000
        if batch > startbatch:
            lr = self.learning_rate - (batch - startbatch) * self.learning_rate / num_steps
            for g in self.optimizer.param_groups:
                g["lr"] = lr
        if batch == (startbatch + num_steps - 5):
            self.stop = True

    def compute_loss(self, nll, kl_free_bit, kl, dims, t=10):
        """RFN/trainer.py:206-219 — loss = nll + β·kl_fb ; bits/dim = (kl+nll)/(ln2 · C·H·W · t)."""
        loss = nll + self.beta * kl_free_bit
        kl_store, nll_store = kl.detach(), nll.detach()
        bits = (kl_store + nll_store) / (np.log(2.) * float(np.prod(list(dims))) * t)
        self._log_step(float(bits), float(loss.detach()) / t, float(kl_store) / t, float(nll_store) / t)
        return loss

    def _log_step(self, bits, loss, kl, nll):
        """one step's scalars into the histories.  With --skip_nonfinite_steps a step whose scalars are not finite (the
        optimizer skips it) leaves no trace, so the epoch mean that drives early stopping and the plateau scheduler
        survives it."""
        if self.skip_nonfinite_steps and not all(math.isfinite(v) for v in (bits, loss, kl, nll)):
            return
        self.bits.append(bits)
        self.losses.append(loss)
        self.kl_loss.append(kl)
        self.recon_loss.append(nll)

    def optimizer_step(self):
        """optimizer.step() behind the guard.  HipAdam carries the guard itself (on the device, no host read).  For CPU
        parameters the same semantics in torch ops: global norm with the rank-local part summed over ranks, skip when
        it is not finite (an fp32 overflow of the sum of squares counts), scale by min(1, max / (norm + 1e-6))."""
        opt = self.optimizer
        if hasattr(opt, "guard_stats"):
            return opt.step()
        if not self.guard_on:
            return self._host_adam_step()
        grads = [p.grad for g in opt.param_groups for p in g["params"] if p.grad is not None]
        local = {id(p.grad) for p in self.reducer.sharded if p.grad is not None}
        sq = torch.zeros(2, dtype=torch.float64)
        for g in grads:
            sq[int(id(g) in local)] += g.detach().double().pow(2).sum().cpu()
        if rdist.is_dist() and self.reducer.sharded:
            rdist.all_reduce_sum_(sq[1:2])
        total = float(sq.sum())
        norm = math.sqrt(total) if total >= 0.0 else math.nan
        scale = min(1.0, self.grad_clip_norm / (norm + 1e-6)) if self.grad_clip_norm > 0.0 else 1.0
        self._host_guard.update(grad_norm=norm, scale=scale)
        if self.skip_nonfinite_steps and not (total <= float(torch.finfo(torch.float32).max)):
            self._host_guard["skipped_steps"] += 1
            return None
        if scale != 1.0:
            torch._foreach_mul_(grads, scale)
        return self._host_adam_step()

    def _host_adam_step(self):
        """an applied step of torch.optim.Adam on CPU parameters and, with --ema_decay, HipAdam's average in torch ops:
        state[p]["ema"] starts as the parameter before its first update, then ema += w (p_new - ema) with
        w = float32(1 - d_n), n the tensor's own step count"""
        opt = self.optimizer
        if not self.ema_decay > 0.0:
            return opt.step()
        with torch.no_grad():
            stepped = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
            # (torch's Adam creates its state where the state is empty: the first copies wait until it has)
            fresh = {p: p.detach().clone() for p in stepped if "ema" not in opt.state.get(p, ())}
            out = opt.step()
            for p in stepped:
                st = opt.state[p]
                ema = st.setdefault("ema", fresh.get(p))
                w = float(np.float32(1.0 - self.ema_step_decay(self.ema_decay, int(float(st["step"])))))
                ema.add_(p.detach() - ema, alpha=w)
        return out

    # ---------------------------------------------------------------------------------------------- average
    def swap_ema(self):
        """exchange parameters and averages (HipAdam: one launch; CPU parameters: torch copies)"""
        opt = self.optimizer
        if not self.ema_decay > 0.0:
            raise RuntimeError("swap_ema: this run keeps no average (--ema_decay 0)")
        if hasattr(opt, "swap_ema"):
            return opt.swap_ema()
        with torch.no_grad():
            for g in opt.param_groups:
                for p in g["params"]:
                    ema = opt.state.get(p, {}).get("ema")
                    if ema is not None:
                        tmp = p.detach().clone()
                        p.copy_(ema)
                        ema.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """context manager: the model holds the averaged weights inside, the raw ones again outside (also when the body
        raises).  Buffers are not averaged.  Nothing may step the optimizer inside."""
        self.swap_ema()
        try:
            yield self.model
        finally:
            self.swap_ema()

    def guard_stats(self):
        """{"grad_norm", "scale", "skipped_steps"}: one device->host read with HipAdam"""
        if hasattr(self.optimizer, "guard_stats"):
            return self.optimizer.guard_stats()
        return dict(self._host_guard)

    # ---------------------------------------------------------------------------------------------- loop
    def train_step(self, image):
        """one optimizer step on an already-resident [B,T,C,H,W] batch in [0,1] (RFN/trainer.py:237-250)."""
        self.beta = min(self.beta_max, self.beta_min + self.counter * (self.beta_max - self.beta_min) / self.beta_steps)
        if self._graph is not None:
            return self._graphed_step(image)
        image = self.preprocess(image)
        first = self.counter == 0 and self.world > 1
        kl_free_bit, kl, nll = self.model.loss(image, 0)
        if first:  # replicas must share rank 0's data dependent ActNorm init: broadcast, then redo the step's forward
            rdist.broadcast_module_state(self.model)
            kl_free_bit, kl, nll = self.model.loss(image, 0)
        loss = self.compute_loss(nll, kl_free_bit, kl, image.shape[2:], t=image.shape[1] - 1)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.reducer.finish()
        self.optimizer_step()
        if self.scheduler_type == "linear":
            self.adjust_learning_rate(self.counter)
        self.counter += 1
        return loss

    # ---- hipGraph mode: preprocess + loss forward + backward of one step are captured once and replayed, which removes
    # the ~7000 per-step launches' host cost (the step is launch-bound once the batch is sharded over several GPUs).
    # Gradient all-reduce, Adam, the beta/LR schedules and the loss bookkeeping stay outside the graph.
    _graph = None

    def capture_graph(self, example_image, static_draws=None):
        """Call after a few eager steps (ActNorm initialised, MIOpen solvers chosen).  Returns True on success; on
        any capture failure the solver silently stays in eager mode.  `static_draws` (tests only) pins the noise.
        The caller must not hold tensors of an earlier eager step's autograd graph (e.g. a returned loss): their
        AccumulateGrad nodes are bound to the default stream and would pull it into the capture."""
        if not torch.cuda.is_available():
            return False
        import rfn_hip
        if rdist.sync_batchnorm_on():
            self._graph_error = "synchronised BatchNorm issues a collective per layer: eager launches only"
            return False
        if not rfn_hip.graph_capture_safe():
            # see rfn_hip/__init__.py: replays are not trustworthy with packet capture on (memset nodes race), and the
            # flag only counts when it was in the environment before the HIP runtime initialised
            self._graph_error = "DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 must be exported before the HIP runtime starts"
            return False
        try:
            self._g_draws = static_draws
            self._g_in = example_image.clone()
            self._g_beta = torch.zeros((), device=example_image.device)
            self.reducer.remove_hooks()           # reductions run after the replay, on the static gradient tensors
            self.optimizer.zero_grad(set_to_none=True)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                # three warm-ups of exactly the captured callable on a side stream: MIOpen / the autograd engine still
                # initialise lazily on the 2nd-3rd execution of a backward, and doing that under capture crashes
                for _ in range(int(os.environ.get("RFN_CAPTURE_WARMUPS", "3"))):  # (developer knob: DESIGN.md §3)
                    self._graph_body()
                    self.optimizer.zero_grad(set_to_none=True)
            torch.cuda.current_stream().wait_stream(side)
            self.optimizer.zero_grad(set_to_none=True)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._graph_body()
            self._graph = g
            return True
        except Exception as e:  # noqa: BLE001 - any failure means "no graph", never a dead trainer
            import traceback
            self._graph = None
            self._graph_error = repr(e)[:200] + " | " + " <- ".join(
                "%s:%d %s" % (f.filename.split("/")[-1], f.lineno, f.name) for f in traceback.extract_tb(e.__traceback__)[-6:])
            torch.cuda.synchronize()
            self.reducer.add_hooks()
            self.optimizer.zero_grad(set_to_none=True)
            return False

    def _graph_body(self):
        from rfn_hip import debug as D
        D.begin()
        image = self.preprocess(self._g_in)
        D.check("image", image)
        kl_free_bit, kl, nll = self.model.loss(image, 0, draws=getattr(self, "_g_draws", None))
        loss = nll + self._g_beta * kl_free_bit
        loss.backward()
        self._g_out = torch.stack([loss.detach(), kl_free_bit.detach(), kl.detach(), nll.detach()])

    def _graphed_step(self, image):
        if os.environ.get("RFN_STEP_TRACE") == "1":  # developer aid: wall time of the phases of a replayed step
            import time
            ts = []
            def mark():
                torch.cuda.synchronize()
                ts.append(time.perf_counter())
            mark(); self._g_in.copy_(image, non_blocking=True); self._g_beta.fill_(self.beta)
            mark(); self._graph.replay()
            mark(); self.reducer.finish()
            mark(); self.optimizer_step()
            mark()
            print("[step %d rank %d] copy %.3f replay %.3f reduce %.3f adam %.3f s" % (
                self.counter, self.rank, ts[1] - ts[0], ts[2] - ts[1], ts[3] - ts[2], ts[4] - ts[3]), flush=True)
        else:
            self._g_in.copy_(image, non_blocking=True)
            self._g_beta.fill_(self.beta)
            self._graph.replay()
            self.reducer.finish()
            self.optimizer_step()
        if self.scheduler_type == "linear":
            self.adjust_learning_rate(self.counter)
        self.counter += 1
        self._pending_log = (self._g_out, tuple(image.shape))
        return self._g_out[0]

    def flush_log(self):
        """bits/dim bookkeeping of the last graphed step (one device->host read, kept off the per-step path)."""
        if getattr(self, "_pending_log", None) is None:
            return
        out, shape = self._pending_log
        loss, _, kl, nll = [float(v) for v in out.tolist()]
        t = shape[1] - 1
        self._log_step((kl + nll) / (np.log(2.) * float(np.prod(shape[2:])) * t), loss / t, kl / t, nll / t)
        self._pending_log = None

    def train(self):
        max_steps = getattr(self.args, "max_steps", 0)
        for _ in range(self.n_epochs):
            self.model.train()
            if hasattr(self.train_loader, "set_epoch"):   # the device loader: epoch e renders its own sequences
                self.train_loader.set_epoch(self.epoch_i)
            self.epoch_i += 1
            for image in self.train_loader:
                image = image[0] if self.choose_data == "bair" and isinstance(image, (list, tuple)) else image
                self.train_step(image.to(self.device, non_blocking=True))
                if max_steps and self.counter >= max_steps:
                    self.stop = True
                    break
            self.flush_log()   # graph mode keeps the last step's scalars on the device until asked
            if self.guard_on:
                self._end_of_epoch_guard()   # (may set self.stop: before the consensus below)
            plot_every = getattr(self.args, "plot_every", 0)   # (Namespaces saved before the flag existed)
            if plot_every > 0 and self.epoch_i % plot_every == 0:
                self.plotter()   # (rank 0 only, no collective, leaves model, RNG states and counters as they were)
            epoch_loss = float(np.mean(self.losses)) if self.losses else math.nan
            # every rank must take the same decisions (checkpoint value, early stop, plateau scheduler): rank-local
            # losses would let learning rates diverge or leave one rank waiting in an all-reduce the others never enter
            # (host scalars: all_reduce_mean_scalars moves them to the GPU when the group is RCCL-only)
            epoch_loss, stop_flag = rdist.all_reduce_mean_scalars(torch.tensor(epoch_loss), torch.tensor(float(self.stop)))
            self.stop = stop_flag > 0.0
            self.checkpoint(self.checkpoint_names[0], self.epoch_i, epoch_loss)   # (collective: gathers the sharded initial states)
            stop = self.earlystopping.step(self.epoch_i, epoch_loss)
            if stop or self.stop:
                break
            if self.earlystopping.best_loss < self.best_loss and self.epoch_i > 50:
                self.best_loss = self.earlystopping.best_loss
                self.checkpoint(self.checkpoint_names[1], self.epoch_i, epoch_loss)
            if self.scheduler_type == "plateau":
                self.scheduler.step(epoch_loss)
            if self.verbose:
                print("Epoch {} Loss: {:.2f}".format(self.epoch_i, epoch_loss))
            elif self.rank == 0:
                self.status()

    def _end_of_epoch_guard(self):
        """read the guard once per epoch; more than --max_skipped_steps skipped steps in one epoch end the training after
        this epoch's checkpoint (whose weights are finite: a skipped step writes nothing)"""
        gs = self._guard_last = self.guard_stats()
        skipped = gs["skipped_steps"] - self._skipped_before_epoch
        self._skipped_before_epoch = gs["skipped_steps"]
        if skipped > self.max_skipped_steps:
            self.stop = True
            why = "STOP: %d steps of epoch %d were skipped for non-finite gradients (--max_skipped_steps %d)" % (
                skipped, self.epoch_i, self.max_skipped_steps)
            if self.rank == 0:
                with open(self.path + "model_folder/status.txt", "a") as f:
                    print(why, file=f)
            if self.verbose:
                print(why)

    # ---------------------------------------------------------------------------------------------- sheets
    def _plot_rows(self, image):
        """the five rows of the plotter's sheet for a preprocessed batch [B, T, C, H, W]: views of device tensors, one
        [n, C, H, W] each (sequence 0 of the batch), in model space"""
        x_conditions, predictions = self.model._predict_device(image, self.n_predictions, self.n_conditions)
        recons, recons_flow = self.model._reconstruct_device(image)
        samples = self.model._sample_device(image, self.n_frames)
        plot_preds = torch.cat((x_conditions, predictions), 0)
        n = self.n_frames
        return [image[0, :n], samples[:n, 0], plot_preds[:n, 0], recons[:n, 0], recons_flow[:n, 0]]

    def plotter(self):
        """RFN/trainer.py:325-417, the frames only: for sequence 0 of the first test batch, a sheet of 5 rows x n_frames
        columns -- ground truth, samples from the first frame, n_conditions given frames followed by n_predictions
        predicted ones, posterior reconstructions, and the flow bijection check g(f(x)) -- written to
        `png_folder/samples<plot_counter>.png`; plot_counter is then incremented.  One compose launch on the GPU
        (rfn_hip.ops.compose_sheet), zlib on the host; no text is drawn and there is no loss-curve panel.
        Two deviations from the reference: its fifth row shows `recons` a second time under the title
        "Recon-Bijection", ours shows `recons_flow`, which is what the title says; and where n_conditions +
        n_predictions < n_frames the missing cells of the prediction row are background (the reference raises).
        Only rank 0 plots and nothing here is a collective.  On return model.training, every parameter and buffer and
        torch's CPU and GPU generator states are what they were (the device datasets draw by address and keep no
        counter), so a run with sheets takes the same training steps as a run without.  Returns the file's path
        (None on other ranks)."""
        if self.rank != 0:
            return None
        from rfn_hip import ops
        from Utils.png import write_png
        if self.model._flow_needs_init():
            # generation marks untouched ActNorm layers initialised (as the reference does), which would change
            # buffers and cancel the data dependent initialisation of the first training step
            raise RuntimeError("plotter: the flow's ActNorm layers are not initialised yet; train a step or load a "
                               "checkpoint first")
        was_training = self.model.training
        on_gpu = self.device.type == "cuda"
        cpu_rng = torch.get_rng_state()
        gpu_rng = torch.cuda.get_rng_state(self.device) if on_gpu else None
        try:
            with torch.no_grad():
                self.model.eval()
                image = next(iter(self.test_loader))
                image = image[0] if self.choose_data == "bair" and isinstance(image, (list, tuple)) else image
                image = self.preprocess(image.to(self.device))
                # with --ema_decay the sheet shows the averaged weights (swapped in and out again: bit-exact moves)
                with self.ema_weights() if self.ema_decay > 0.0 else contextlib.nullcontext():
                    sheet = ops.compose_sheet(self._plot_rows(image), self.n_frames, n_bits=self.n_bits,
                                              preprocess_range=self.preprocess_range, scanlines=True)
            path = self.path + "png_folder/samples%d.png" % self.plot_counter
            write_png(path, sheet)
        finally:
            self.model.train(was_training)
            torch.set_rng_state(cpu_rng)
            if on_gpu:
                torch.cuda.set_rng_state(gpu_rng, self.device)
        self.plot_counter += 1
        return path

    # ---------------------------------------------------------------------------------------------- state
    def checkpoint(self, model_name, epoch, loss):
        """same dict layout as RFN/trainer.py:277-300 (model/optimizer state, histories, counters, args); `args_dict` is
        the same Namespace as a plain dict.  Collective under data parallelism: the batch-sharded initial states are
        gathered so that the file holds the GLOBAL batch rows (a single process can resume it); rank 0 writes.  With
        --ema_decay the averaged weights travel inside `optimizer_state_dict` (state[i]["ema"]); the top-level keys are
        the same with and without."""
        state = rdist.gather_sharded_state(self.model)
        opt_state = rdist.gather_sharded_optimizer_state(self.optimizer, self.model)   # (moments of the sharded rows too)
        if self.rank != 0:
            return
        # `args.batch_size` is the per-rank batch; the file describes the GLOBAL batch (rows in rank order)
        common = {"epoch": epoch, "loss": loss, "kl_loss": self.kl_loss, "recon_loss": self.recon_loss,
                  "losses": self.losses, "bits_per_dim": self.bits, "annealing_counter": self.counter,
                  "args": self.args, "args_dict": dict(vars(self.args)), "world_size": self.world,
                  "global_batch_size": int(self.batch_size) * self.world}
        full = dict(common)
        full.update({"model_state_dict": state, "optimizer_state_dict": opt_state,
                     "plot_counter": self.plot_counter})
        torch.save(full, self.path + "model_folder/" + model_name)
        torch.save(common, self.path + "model_folder/eval_dict.pt")

    @staticmethod
    def args_for_world(ckpt, world):
        """the Namespace to rebuild a Solver from `ckpt` on `world` ranks: the stored `batch_size` is per rank of the
        run that wrote the file; the global batch is what is kept (files without `global_batch_size` -- the reference's
        own -- are single-process: global = stored)."""
        import copy
        args = copy.copy(ckpt["args"])
        gb = int(ckpt.get("global_batch_size", args.batch_size))
        if gb % world:
            raise ValueError("checkpoint global batch %d does not divide over %d ranks" % (gb, world))
        args.batch_size = gb // world
        for k in ("x_dim", "condition_dim"):   # [B, C, H, W] lists carry the batch too
            v = getattr(args, k, None)
            if isinstance(v, (list, tuple)) and len(v) == 4:
                setattr(args, k, [gb // world] + list(v[1:]))
        return args

    @staticmethod
    def read_checkpoint(path):
        """load an rfn.pt written by this Solver or by the reference WITHOUT executing anything from the file: tensors,
        containers and numbers plus the one class the layout needs (argparse.Namespace)."""
        import argparse
        with torch.serialization.safe_globals([argparse.Namespace]):
            return torch.load(path, map_location="cpu", weights_only=True)

    def load(self, load_model):
        rdist.load_sharded_state(self.model, load_model["model_state_dict"])
        # the file holds the moments of the GLOBAL rows of the batch-sharded initial states: every rank takes its own
        # (torch's load_state_dict does not compare shapes, and HipAdam indexes the moments by the parameter's numel)
        opt_state = rdist.shard_optimizer_state(load_model["optimizer_state_dict"], self.model)
        if not self.ema_decay > 0.0:   # a run without --ema_decay would carry the file's average along, never updated
            opt_state = dict(opt_state, state={i: {k: v for k, v in st.items() if k != "ema"}
                                               for i, st in opt_state["state"].items()})
        self.optimizer.load_state_dict(opt_state)
        # (the count of skipped steps restarts with the loaded state, in HipAdam and for CPU parameters)
        self._skipped_before_epoch = self._host_guard["skipped_steps"] = 0
        self.epoch_i += load_model["epoch"]
        loss = load_model["loss"]
        self.kl_loss, self.recon_loss = load_model["kl_loss"], load_model["recon_loss"]
        self.losses, self.plot_counter = load_model["losses"], load_model["plot_counter"]
        self.counter, self.bits = load_model["annealing_counter"], load_model["bits_per_dim"]
        self.best_loss = loss
        self.model.to(self.device)
        return self.epoch_i, loss

    @staticmethod
    def ema_tensors(ckpt):
        """{parameter index: average} of a checkpoint written with --ema_decay: `optimizer_state_dict["state"][i]["ema"]`,
        i counting model.parameters() (global rows for the batch-sharded initial states).  ValueError when the file
        holds none."""
        state = (ckpt.get("optimizer_state_dict") or {}).get("state") or {}
        out = {int(i): st["ema"] for i, st in state.items() if isinstance(st, dict) and "ema" in st}
        if not out:
            raise ValueError("the checkpoint holds no averaged weights (it was not written with --ema_decay)")
        return out

    def load_ema_weights(self, load_model):
        """copy the averages saved in a checkpoint into the model's parameters (by index in model.parameters() order;
        a batch-sharded initial state takes this rank's rows of the global ones, as `load` does).  Parameters without a
        saved average (they never saw a gradient) and all buffers keep their values: call after `load`.  Returns the
        number of parameters written."""
        emas = self.ema_tensors(load_model)
        params = list(self.model.parameters())
        world = dist.get_world_size() if rdist.is_dist() else 1
        sharded = set(rdist._sharded_param_indices(self.model))
        todo = []
        for i, ema in sorted(emas.items()):
            if i >= len(params):
                raise ValueError("the checkpoint averages parameter %d, the model has %d" % (i, len(params)))
            p = params[i]
            if i in sharded and world > 1 and ema.shape[0] == p.shape[0] * world and \
                    tuple(ema.shape[1:]) == tuple(p.shape[1:]):
                ema = ema[self.rank * p.shape[0]:(self.rank + 1) * p.shape[0]]
            if tuple(ema.shape) != tuple(p.shape):
                raise ValueError("averaged parameter %d has shape %s, the model's %s" %
                                 (i, tuple(ema.shape), tuple(p.shape)))
            todo.append((p, ema))
        with torch.no_grad():
            for p, ema in todo:
                p.copy_(ema.to(p.device))
        return len(todo)

    def status(self):
        lr = self.optimizer.param_groups[0]["lr"]
        with open(self.path + "model_folder/status.txt", "a") as f:
            print("STATUS:", file=f)
            if self.kl_loss:
                print("\tKL and Reconstruction loss: {:.4f}, {:.4f}".format(self.kl_loss[-1], self.recon_loss[-1]),
                      file=f)
            print(f"\tEpoch {self.epoch_i}, Beta value {self.beta:.4f}, Learning rate {lr}", file=f)
            if self.guard_on and self._guard_last is not None:
                print("\tGradient norm {:.4g}, skipped steps {}".format(self._guard_last["grad_norm"],
                                                                        self._guard_last["skipped_steps"]), file=f)
