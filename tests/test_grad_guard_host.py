"""CPU-only tests of the optimizer-step guard (global gradient-norm clip, non-finite skip): the command line flags, the
Solver's handling of CPU parameters (torch.optim.Adam guarded by a few torch ops, the semantics of the device guard of
rfn_hip.optim.HipAdam), the loss histories, Namespaces from before the flags, and the three C symbols."""
import math
import os
from argparse import Namespace

import torch

from tests.test_host_logic import _parse_header
from tests.test_moving_mnist_host import _solver_argv


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.h_0 = torch.nn.Parameter(torch.randn(2, 3, generator=g))      # batch-shaped: its gradient is rank-local
        self.w = torch.nn.Parameter(torch.randn(7, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(11, generator=g))


def _solver(extra=""):
    import main_rfn
    from RFN.trainer import Solver
    from rfn_hip import dist as rdist
    s = Solver(main_rfn.build_parser().parse_args(_solver_argv("--synthetic_data --choose_data mnist " + extra)))
    s.model = Toy()
    s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
    s.optimizer = s.make_optimizer(s.model.parameters(), 1e-2, **s.guard_kwargs())
    return s


def _set_grads(model, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g) * scale


def test_parser_accepts_the_guard_flags():
    import main_rfn
    p = main_rfn.build_parser()
    d = p.parse_args([])
    assert d.grad_clip_norm == 0 and d.skip_nonfinite_steps is False and d.max_skipped_steps == 100
    a = p.parse_args("--grad_clip_norm 2.5 --skip_nonfinite_steps --max_skipped_steps 7".split())
    assert a.grad_clip_norm == 2.5 and a.skip_nonfinite_steps is True and a.max_skipped_steps == 7
    assert p.parse_args(["--no-skip_nonfinite_steps"]).skip_nonfinite_steps is False


def test_cpu_solver_skips_a_step_with_non_finite_gradients():
    s = _solver("--skip_nonfinite_steps --grad_clip_norm 1e30")
    assert s.guard_on and type(s.optimizer) is torch.optim.Adam
    assert [id(p) for p in s.guard_kwargs()["rank_local"]] == [id(s.model.h_0)]
    _set_grads(s.model, 2)
    s.optimizer_step()                                   # a clean step first: the moments exist
    for poison, where in ((math.nan, "w"), (math.inf, "h_0"), (-math.inf, "b"), (3e19, "w")):
        before = [p.detach().clone() for p in s.model.parameters()]
        moments = [s.optimizer.state[p]["exp_avg"].clone() for p in s.model.parameters()]
        skipped = s.guard_stats()["skipped_steps"]
        _set_grads(s.model, 3)
        getattr(s.model, where).grad.view(-1)[:2] = poison   # (two elements of 3e19: the sum of squares leaves fp32)
        s.optimizer_step()
        assert s.guard_stats()["skipped_steps"] == skipped + 1
        for p, q, m in zip(s.model.parameters(), before, moments):
            assert torch.equal(p.detach(), q) and torch.equal(s.optimizer.state[p]["exp_avg"], m)
            assert float(s.optimizer.state[p]["step"]) == 1.0
    _set_grads(s.model, 4)
    s.optimizer_step()
    assert float(s.optimizer.state[s.model.w]["step"]) == 2.0
    assert all(bool(torch.isfinite(p).all()) for p in s.model.parameters())


def test_cpu_solver_clips_to_the_requested_norm():
    s = _solver("--grad_clip_norm 0.75")
    ref = Toy()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    for i in range(3):
        _set_grads(s.model, 10 + i, scale=3.0)
        _set_grads(ref, 10 + i, scale=3.0)
        norm = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ref.parameters()))
        assert norm > 0.75
        s.optimizer_step()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.75)
        opt.step()
        gs = s.guard_stats()
        assert abs(gs["grad_norm"] - norm) <= 1e-12 * norm and abs(gs["scale"] - 0.75 / (norm + 1e-6)) <= 1e-12
        assert gs["skipped_steps"] == 0
    for p, q in zip(s.model.parameters(), ref.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7)
    # a gradient inside the ball is left alone
    _set_grads(s.model, 20, scale=1e-3)
    _set_grads(ref, 20, scale=1e-3)
    s.optimizer_step()
    assert s.guard_stats()["scale"] == 1.0
    for p, q in zip(s.model.parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_non_finite_scalars_stay_out_of_the_histories():
    dims = torch.Size([1, 8, 8])
    for flag, kept in (("--skip_nonfinite_steps", 1), ("", 2)):
        s = _solver(flag)
        s.beta = 0.5
        s.compute_loss(torch.tensor(3.0), torch.tensor(1.0), torch.tensor(1.5), dims, t=3)
        s.compute_loss(torch.tensor(math.nan), torch.tensor(1.0), torch.tensor(1.5), dims, t=3)
        for h in (s.losses, s.kl_loss, s.recon_loss, s.bits):
            assert len(h) == kept
        # the same rule for the scalars a replayed graph leaves on the device until flush_log()
        s._pending_log = (torch.tensor([math.inf, 1.0, 1.5, 3.0]), (2, 4, 1, 8, 8))
        s.flush_log()
        assert s._pending_log is None and len(s.losses) == (kept if flag else kept + 1)
        s._pending_log = (torch.tensor([3.5, 1.0, 1.5, 3.0]), (2, 4, 1, 8, 8))
        s.flush_log()
        assert len(s.losses) == len(s.bits) == (kept + 1 if flag else kept + 2)
        assert math.isfinite(sum(s.losses) + sum(s.bits)) == bool(flag)


def test_too_many_skipped_steps_end_the_training(tmp_path):
    """end of an epoch with the guard on: the stats are read once, status() reports them, and more skipped steps in one
    epoch than --max_skipped_steps set the stop flag and write the reason to status.txt"""
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    s = _solver("--skip_nonfinite_steps --max_skipped_steps 3 --path %s" % rel)
    os.makedirs(s.path + "model_folder")
    s.epoch_i = 1
    s._host_guard.update(grad_norm=12.5, skipped_steps=3)
    s._end_of_epoch_guard()
    assert not s.stop                                   # 3 is not more than 3
    s.status()
    s.epoch_i = 2
    s._host_guard.update(skipped_steps=7)               # four more in this epoch
    s._end_of_epoch_guard()
    assert s.stop
    txt = open(s.path + "model_folder/status.txt").read()
    assert "Gradient norm 12.5, skipped steps 3" in txt
    assert "STOP: 4 steps of epoch 2 were skipped" in txt and "--max_skipped_steps 3" in txt
    # guard off: status() writes what it wrote before
    q = _solver("--path %s" % ("/" + os.path.relpath(str(tmp_path / "off"), os.getcwd()) + "/"))
    os.makedirs(q.path + "model_folder")
    q.status()
    assert "Gradient norm" not in open(q.path + "model_folder/status.txt").read()


def test_namespace_without_the_guard_flags_builds_and_steps_as_before(tmp_path, monkeypatch):
    import main_rfn
    from RFN.trainer import Solver
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv("--synthetic_data --choose_data mnist --path %s" % rel))
    new = ("grad_clip_norm", "skip_nonfinite_steps", "max_skipped_steps")
    old = Namespace(**{k: v for k, v in vars(args).items() if k not in new})
    assert not any(hasattr(old, k) for k in new)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # host logic only: build on the CPU
    torch.manual_seed(0)
    s = Solver(old)
    s.build()
    assert not s.guard_on and s.max_skipped_steps == 100 and type(s.optimizer) is torch.optim.Adam
    twin = [torch.nn.Parameter(p.detach().clone()) for p in s.model.parameters()]
    opt = torch.optim.Adam(twin, lr=s.learning_rate)
    g = torch.Generator().manual_seed(5)
    for p, q in zip(s.model.parameters(), twin):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    s.optimizer_step()
    opt.step()
    for p, q in zip(s.model.parameters(), twin):
        assert torch.equal(p.detach(), q.detach())
    s.compute_loss(torch.tensor(math.nan), torch.tensor(1.0), torch.tensor(1.5), torch.Size([1, 8, 8]), t=3)
    assert len(s.losses) == 1                        # guard off: the histories take what comes, as before


def test_header_and_binding_declare_the_guard_symbols():
    from rfn_hip import lib
    protos, _ = _parse_header()
    for name in ("rfn_grad_sumsq_f32", "rfn_grad_guard_f32", "rfn_adam_step_guarded_f32"):
        assert name in protos and name in lib.SIGNATURES
        assert len(protos[name]) == len(lib.SIGNATURES[name])
    plain, guarded = protos["rfn_adam_step_f32"], protos["rfn_adam_step_guarded_f32"]
    assert guarded[:len(plain) - 1] == plain[:-1] and guarded[-1] == plain[-1]   # the plain arguments, then stats, skipped
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rfn_hip.h")).read()
    assert "int flags;" in hdr and "int reserved;" not in hdr
