"""GPU tests of Stochastic Moving MNIST: rfn_moving_mnist_render_f32 (through rfn_hip.ops.moving_mnist_render) against the
Python / numpy restatement of tests/test_moving_mnist_host.py, bit for bit on frames and trajectories; the addressing of
sequences (epochs, splits, ranks); and the Solver / Evaluator on the device loaders, end to end.  The digits are
generated here (tests/test_moving_mnist_host.fixture_digits)."""
import itertools
import math
import os
from argparse import Namespace

import pytest
import torch

from tests.test_moving_mnist_host import _solver_argv, fixture_digits, render, write_mnist

pytestmark = pytest.mark.gpu


# (B, T, S, num_digits, L, deterministic, C): every value of every axis occurs
CASES = [(1, 1, 29, 1, 1, False, 1), (7, 20, 32, 2, 4, True, 3), (32, 20, 64, 3, 4, False, 1),
         (7, 20, 29, 3, 1, False, 3), (32, 1, 32, 2, 1, True, 1), (1, 20, 64, 1, 4, True, 3),
         (32, 20, 29, 2, 4, False, 3), (7, 20, 64, 3, 1, True, 1), (32, 20, 32, 3, 4, False, 1)]


@pytest.mark.parametrize("B,T,S,nd,L,det,C", CASES)
def test_kernel_matches_restatement(B, T, S, nd, L, det, C):
    from rfn_hip import ops
    digits = fixture_digits(64, B + T + S)
    seed, split, first = 3 + S, int(det), (1 << 40) + 17 * B
    out, traj = ops.moving_mnist_render(torch.from_numpy(digits).cuda(), B, T, C, S, nd, L, det, seed, split, first,
                                        trajectories=True)
    torch.cuda.synchronize()
    want_x, want_traj = render(digits, B, T, C, S, nd, L, det, seed, split, first)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, T, C, S, S) and out.is_contiguous()
    assert torch.equal(traj.cpu(), torch.from_numpy(want_traj))
    assert torch.equal(out.cpu(), torch.from_numpy(want_x))


def test_kernel_rounding_and_clip_exercised():
    """the fixture really reaches the float32 rounding / clip cases: overlapping sums at, below and above 1"""
    from rfn_hip import ops
    digits = fixture_digits(64, 5)
    out = ops.moving_mnist_render(torch.from_numpy(digits).cuda(), 32, 20, 1, 29, 3, 4, False, 1, 0, 0).cpu()
    want, _ = render(digits, 32, 20, 1, 29, 3, 4, False, 1, 0, 0)
    assert torch.equal(out, torch.from_numpy(want))
    assert bool((out == 1.0).any()) and bool(((out > 0.99) & (out < 1.0)).any())


def _dataset(root, train, **kw):
    from data_generators import MovingMNIST
    base = dict(seq_len=6, num_digits=2, image_size=32, deterministic=False, three_channels=False, step_length=4, seed=9)
    base.update(kw)
    return MovingMNIST(train, root, **base)


@pytest.fixture(scope="module")
def mnist_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("mnist"))
    write_mnist(root, fixture_digits(48, 21), fixture_digits(24, 22), layout="gz")
    return root


def test_addressing(mnist_root):
    from data_generators import MovingMNISTLoader
    tr, te = _dataset(mnist_root, True), _dataset(mnist_root, False)
    assert len(tr) == 48 and len(te) == 24
    a = tr.render(100, 8)
    assert torch.equal(a, tr.render(100, 8))                         # same address, same bytes
    assert torch.equal(a[3:5], tr.render(103, 2))                    # batch composition does not matter
    assert torch.equal(tr[5].unsqueeze(0), tr.render(5, 1))
    assert not torch.equal(a, te.render(100, 8))                     # the splits are different streams
    assert not torch.equal(a, _dataset(mnist_root, True, seed=10).render(100, 8))
    ld = MovingMNISTLoader(tr, 4)
    assert len(ld) == 12
    e0 = list(ld)
    ld.set_epoch(1)
    e1 = list(ld)
    assert all(not torch.equal(x, y) for x, y in zip(e0, e1))       # every epoch sees fresh sequences
    assert torch.equal(e1[2], tr.render(48 + 8, 4))
    lt = MovingMNISTLoader(te, 4)
    t0 = list(lt)
    lt.set_epoch(7)
    assert all(torch.equal(x, y) for x, y in zip(t0, lt))            # the test split ignores the epoch
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(t0, list(lt)))   # fresh tensors
    # ranks: rank r of w renders rows [r*B, (r+1)*B) of each world-1 global batch
    for world in (2, 4):
        B = 8 // world
        for ep in (0, 3):
            full = MovingMNISTLoader(tr, 8)
            full.set_epoch(ep)
            ref = list(full)
            for r in range(world):
                ldr = MovingMNISTLoader(tr, B, rank=r, world=world)
                ldr.set_epoch(ep)
                got = list(ldr)
                assert len(got) == len(ref) == 6
                for g, x in zip(got, ref):
                    assert torch.equal(g, x[r * B:(r + 1) * B])
    # three channels are copies; values in [0, 1]
    c3 = _dataset(mnist_root, True, three_channels=True).render(100, 8)
    assert tuple(c3.shape) == (8, 6, 3, 32, 32) and torch.equal(c3[:, :, 1], a[:, :, 0]) and torch.equal(c3[:, :, 2], a[:, :, 0])
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0


def test_solver_trains_and_evaluates_on_moving_mnist(mnist_root, tmp_path):
    import main_rfn
    from RFN.trainer import Solver
    from evaluation_metrics import Evaluator
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv("--choose_data mnist --mnist_root %s --path %s --data_seed 4"
                                                           % (mnist_root, rel)))
    torch.manual_seed(0)
    s = Solver(args)
    s.build()
    assert type(s.train_loader).__name__ == "MovingMNISTLoader" and len(s.train_loader) == 24
    it = iter(s.train_loader)
    losses = []
    for _ in range(2):
        x = next(it)
        assert x.is_cuda and tuple(x.shape) == (2, 4, 1, 32, 32)
        losses.append(float(s.train_step(x).detach()))
    assert s.capture_graph(next(it)), getattr(s, "_graph_error", "")
    for _ in range(2):
        losses.append(float(s.train_step(next(it)).detach()))
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in losses), losses
    # the test loader is a fixed set
    first = list(itertools.islice(iter(s.test_loader), 3))
    again = list(itertools.islice(iter(s.test_loader), 3))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    ev = Evaluator(s, settings=Namespace(n_frames=4, start_predictions=2, resample=2, n_trained=4))
    mean, _ = ev.get_loss(max_batches=2)
    assert math.isfinite(float(mean))
    out = ev.get_eval_values(max_batches=1)
    mse, psnr, ssim, lpips, bpd, dkl, recon, ssim_std, psnr_std, lpips_std = out
    for t in (mse, psnr, ssim, ssim_std, psnr_std):
        assert tuple(t.shape) == (2, 2) and t.dtype == torch.float32
    assert lpips is None and lpips_std is None and tuple(bpd.shape) == (1,) and math.isfinite(float(bpd[0]))


def test_solver_train_sets_the_epoch(mnist_root, tmp_path):
    """Solver.train hands the epoch to the loader before each epoch (a resumed run continues the stream)"""
    import main_rfn
    from RFN.trainer import Solver
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv("--choose_data mnist --mnist_root %s --path %s --n_epochs 1 "
                                                           "--max_steps 1" % (mnist_root, rel)))
    s = Solver(args)
    s.build()
    seen = []
    plain = s.train_step
    s.train_step = lambda x: (seen.append(x.clone()), plain(x))[1]
    s.epoch_i = 5                      # as after load() of a file written at the end of epoch 5
    s.train()
    assert s.train_loader.epoch == 5 and s.epoch_i == 6
    assert torch.equal(seen[0], s.train_loader.dataset.render(5 * 48, 2))
