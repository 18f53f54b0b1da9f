"""CPU-only tests of the Polyak average of the weights (--ema_decay): the decay rule with its warm-up, the flag, the
Solver's torch-op version for CPU parameters (the semantics of the average rfn_hip.optim.HipAdam keeps inside its launch)
against a float64 restatement of the definition, skipped steps, the sharded rows of the batch-shaped initial states, and
tools/export_ema.py / Solver.load_ema_weights on a hand-built checkpoint."""
import importlib.util
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.test_grad_guard_host import Toy, _set_grads
from tests.test_moving_mnist_host import _solver_argv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_export_ema():
    spec = importlib.util.spec_from_file_location("export_ema", os.path.join(ROOT, "tools", "export_ema.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the definition, restated in float64: d in (0, 1); n = 1, 2, ... counts the tensor's applied Adam steps; after the
# update of step n has produced p_new:  d_n = min(d, (1 + n) / (10 + n)) in double, w = (float)(1 - d_n),
# ema <- ema + w (p_new - ema).  The tests feed it the float32 parameters the code under test produced.
def decay_at(d, n):
    return min(d, (1.0 + n) / (10.0 + n))


def restate(ema64, p_new, d, n):
    w = float(np.float32(1.0 - decay_at(d, n)))
    return ema64 + w * (p_new.double() - ema64)


def _solver(extra="", model=None):
    import main_rfn
    from RFN.trainer import Solver
    from rfn_hip import dist as rdist
    s = Solver(main_rfn.build_parser().parse_args(_solver_argv("--synthetic_data --choose_data mnist " + extra)))
    s.model = model if model is not None else Toy()
    s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
    s.optimizer = s.make_optimizer(s.model.parameters(), 1e-2, **s.guard_kwargs(), ema_decay=s.ema_decay)
    return s


def test_decay_rule_and_its_warm_up():
    from RFN.trainer import Solver
    d = 0.999
    assert Solver.ema_step_decay(d, 1) == 2.0 / 11.0
    assert Solver.ema_step_decay(d, 2) == 3.0 / 12.0
    assert Solver.ema_step_decay(d, 90) == 91.0 / 100.0
    assert Solver.ema_step_decay(d, 10 ** 6) == d
    # (1 + n) / (10 + n) >= 0.999  <=>  n >= 8990
    assert Solver.ema_step_decay(d, 8989) == 8990.0 / 8999.0 < d
    assert Solver.ema_step_decay(d, 8990) == d and Solver.ema_step_decay(d, 8991) == d
    for n in (1, 2, 90, 8989, 8990, 10 ** 6):
        assert Solver.ema_step_decay(d, n) == decay_at(d, n)


def test_flag_default_range_and_old_namespaces():
    import main_rfn
    from RFN.trainer import Solver
    p = main_rfn.build_parser()
    assert p.parse_args([]).ema_decay == 0.0
    assert p.parse_args(["--ema_decay", "0.999"]).ema_decay == 0.999
    for bad in ("1.0", "-0.1", "1.5", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["--ema_decay", bad])
    args = p.parse_args(_solver_argv("--synthetic_data --choose_data mnist"))
    assert Solver(args).ema_decay == 0.0
    old = Namespace(**{k: v for k, v in vars(args).items() if k != "ema_decay"})
    assert not hasattr(old, "ema_decay") and Solver(old).ema_decay == 0.0
    for bad in (1.0, -0.25, math.nan):
        with pytest.raises(ValueError):
            Solver(Namespace(**dict(vars(args), ema_decay=bad)))
        with pytest.raises(ValueError):
            Solver.make_optimizer(Toy().parameters(), 1e-2, ema_decay=bad)


def test_cpu_solver_applied_steps_match_the_restatement():
    d = 0.9
    s = _solver("--ema_decay %s" % d)
    assert s.ema_decay == d and type(s.optimizer) is torch.optim.Adam
    params = list(s.model.parameters())
    ema64 = [p.detach().double().clone() for p in params]       # the copy taken before the first update
    for n in (1, 2, 3):
        _set_grads(s.model, 30 + n)
        before = [p.detach().clone() for p in params]
        s.optimizer_step()
        assert all(not torch.equal(p.detach(), q) for p, q in zip(params, before))
        for j, p in enumerate(params):
            ema64[j] = restate(ema64[j], p.detach(), d, n)
            got = s.optimizer.state[p]["ema"]
            assert got.dtype == torch.float32 and got.shape == p.shape
            err = float((got.double() - ema64[j]).abs().max())
            bound = 3 * 2.0 ** -23 * float(p.detach().abs().max())
            print("step", n, "tensor", j, "err", err, "bound", bound)
            assert err <= bound
            assert float(s.optimizer.state[p]["step"]) == n
    # the average is not the parameter: it lags behind
    assert all(not torch.equal(s.optimizer.state[p]["ema"], p.detach()) for p in params)


def test_cpu_solver_skipped_step_leaves_the_average_and_its_count():
    d = 0.999
    s = _solver("--ema_decay %s --skip_nonfinite_steps" % d)
    params = list(s.model.parameters())
    ema64 = [p.detach().double().clone() for p in params]
    _set_grads(s.model, 41)
    s.optimizer_step()
    ema64 = [restate(e, p.detach(), d, 1) for e, p in zip(ema64, params)]
    kept = [s.optimizer.state[p]["ema"].clone() for p in params]
    _set_grads(s.model, 42)
    s.model.w.grad.view(-1)[3] = math.nan
    s.optimizer_step()
    assert s.guard_stats()["skipped_steps"] == 1
    for p, k in zip(params, kept):
        assert torch.equal(s.optimizer.state[p]["ema"], k)      # bit-unchanged
        assert float(s.optimizer.state[p]["step"]) == 1.0
    _set_grads(s.model, 43)
    s.optimizer_step()
    for j, p in enumerate(params):
        bound = 3 * 2.0 ** -23 * float(p.detach().abs().max())
        want = restate(ema64[j], p.detach(), d, 2)              # n = 2: the skipped step is not counted
        wrong = restate(ema64[j], p.detach(), d, 3)
        got = s.optimizer.state[p]["ema"].double()
        assert float((got - want).abs().max()) <= bound
        assert float((got - wrong).abs().max()) > bound         # d_2 = 1/4 against d_3 = 4/13: the count is visible


def test_flag_off_keeps_no_average():
    s = _solver("")
    assert s.ema_decay == 0.0 and not hasattr(s.optimizer, "ema_decay")
    _set_grads(s.model, 5)
    s.optimizer_step()
    for p in s.model.parameters():
        assert sorted(s.optimizer.state[p]) == ["exp_avg", "exp_avg_sq", "step"]
    assert all("ema" not in st for st in s.optimizer.state_dict()["state"].values())
    with pytest.raises(RuntimeError):
        s.swap_ema()


def test_cpu_solver_swaps_the_average_in_and_out():
    s = _solver("--ema_decay 0.9")
    for n in range(2):
        _set_grads(s.model, 50 + n)
        s.optimizer_step()
    params = list(s.model.parameters())
    raw = [p.detach().clone() for p in params]
    avg = [s.optimizer.state[p]["ema"].clone() for p in params]
    with s.ema_weights() as model:
        assert model is s.model
        assert all(torch.equal(p.detach(), a) for p, a in zip(params, avg))
        assert all(torch.equal(s.optimizer.state[p]["ema"], r) for p, r in zip(params, raw))
    assert all(torch.equal(p.detach(), r) for p, r in zip(params, raw))
    assert all(torch.equal(s.optimizer.state[p]["ema"], a) for p, a in zip(params, avg))
    with pytest.raises(KeyError):                               # swapped out again when the body raises
        with s.ema_weights():
            raise KeyError("body")
    assert all(torch.equal(p.detach(), r) for p, r in zip(params, raw))


def test_shard_optimizer_state_cuts_the_average_like_the_moments(monkeypatch):
    """one process standing in for rank 1 of 2: the file's global rows of the batch-shaped h_0 become this rank's"""
    from rfn_hip import dist as rdist
    m = Toy()
    names = [n for n, _ in m.named_parameters()]
    i_h, i_w = names.index("h_0"), names.index("w")
    g = torch.Generator().manual_seed(9)
    glob = {k: torch.randn(4, 3, generator=g) for k in ("exp_avg", "exp_avg_sq", "ema")}
    rep = {k: torch.randn(7, 5, generator=g) for k in ("exp_avg", "exp_avg_sq", "ema")}
    sd = {"state": {i_h: dict(glob, step=torch.tensor(2.0)), i_w: dict(rep, step=torch.tensor(2.0))},
          "param_groups": [{"params": list(range(len(names)))}]}
    monkeypatch.setattr(rdist, "is_dist", lambda: True)
    monkeypatch.setattr(rdist.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(rdist.dist, "get_rank", lambda group=None: 1)
    out = rdist.shard_optimizer_state(sd, m)
    for k in ("exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(out["state"][i_h][k], glob[k][2:4])
        assert torch.equal(out["state"][i_w][k], rep[k])        # replicated: untouched
    assert tuple(sd["state"][i_h]["ema"].shape) == (4, 3)       # the input is not modified
    # local rows already (a single-process file): kept
    local = {"state": {i_h: {k: v[:2] for k, v in glob.items()}}, "param_groups": sd["param_groups"]}
    assert torch.equal(rdist.shard_optimizer_state(local, m)["state"][i_h]["ema"], glob["ema"][:2])
    # an average that fits neither the local nor the global batch drops the entry, as a moment of that shape does
    bad = {"state": {i_h: dict(glob, ema=torch.zeros(7, 3))}, "param_groups": sd["param_groups"]}
    assert i_h not in rdist.shard_optimizer_state(bad, m)["state"]


class ToyWithBuffers(Toy):
    def __init__(self):
        super().__init__()
        self.register_buffer("running_mean", torch.arange(5.0))
        self.register_buffer("num_batches_tracked", torch.tensor(7))


def _hand_built_checkpoint(with_ema=True):
    m = ToyWithBuffers()
    names = [n for n, _ in m.named_parameters()]
    g = torch.Generator().manual_seed(21)
    state = {}
    for i, (n, p) in enumerate(m.named_parameters()):
        state[i] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(p.shape, generator=g),
                    "exp_avg_sq": torch.rand(p.shape, generator=g)}
        if with_ema and n != "b":                               # b never saw a gradient: no average
            state[i]["ema"] = torch.randn(p.shape, generator=g)
    ckpt = {"epoch": 4, "loss": 1.5, "model_state_dict": {k: v.clone() for k, v in m.state_dict().items()},
            "optimizer_state_dict": {"state": state, "param_groups": [{"lr": 1e-2, "params": list(range(len(names)))}]},
            "plot_counter": 0, "losses": [2.0, 1.5]}
    return m, names, ckpt


def test_export_ema_on_a_hand_built_checkpoint():
    X = load_export_ema()
    m, names, ckpt = _hand_built_checkpoint()
    before = {k: v.clone() for k, v in ckpt["model_state_dict"].items()}
    out = X.export_ema(ckpt, names)
    assert list(out) == list(ckpt)                              # the same top-level keys, in order
    sd = out["model_state_dict"]
    assert list(sd) == list(before)
    for i, n in enumerate(names):
        if n == "b":
            assert torch.equal(sd[n], before[n])
        else:
            assert torch.equal(sd[n], ckpt["optimizer_state_dict"]["state"][i]["ema"])
            assert not torch.equal(sd[n], before[n])
    for n in ("running_mean", "num_batches_tracked"):           # buffers are not averaged
        assert torch.equal(sd[n], before[n]) and sd[n].dtype == before[n].dtype
    assert out["optimizer_state_dict"] is ckpt["optimizer_state_dict"] and out["losses"] == ckpt["losses"]
    assert all(torch.equal(ckpt["model_state_dict"][k], v) for k, v in before.items())   # input untouched
    m.load_state_dict(sd)                                       # and it is a state_dict of the model
    # an average of the wrong shape is refused, and so is a file without averages
    ckpt["optimizer_state_dict"]["state"][1]["ema"] = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="shape"):
        X.export_ema(ckpt, names)
    with pytest.raises(ValueError, match="no averaged weights"):
        X.export_ema(_hand_built_checkpoint(with_ema=False)[2], names)


def test_export_writes_a_shared_parameter_under_each_of_its_names():
    """the extractor's layers are registered twice (l_nets and net): parameters() lists such a tensor once, state_dict()
    saves it under both names and load_state_dict copies them in turn, so the last name would win"""
    X = load_export_ema()
    m = torch.nn.Module()
    m.a, m.b, m.c = (torch.nn.Linear(3, 3, bias=False) for _ in range(3))
    m.b.weight = m.a.weight
    assert X.param_keys_of(m) == [("a.weight", "b.weight"), ("c.weight",)]
    ema = {0: {"ema": torch.full((3, 3), 5.0)}, 1: {"ema": torch.full((3, 3), 7.0)}}
    ckpt = {"model_state_dict": {k: v.clone() for k, v in m.state_dict().items()},
            "optimizer_state_dict": {"state": ema, "param_groups": [{"params": [0, 1]}]}}
    sd = X.export_ema(ckpt, X.param_keys_of(m))["model_state_dict"]
    assert all(bool((sd[k] == 5.0).all()) for k in ("a.weight", "b.weight")) and bool((sd["c.weight"] == 7.0).all())
    m.load_state_dict(sd)
    assert bool((m.a.weight == 5.0).all()) and m.b.weight is m.a.weight and bool((m.c.weight == 7.0).all())


def test_load_ema_weights():
    m, names, ckpt = _hand_built_checkpoint()
    s = _solver("", model=ToyWithBuffers())
    with torch.no_grad():
        for p in s.model.parameters():
            p.add_(1.0)
    kept_b, kept_buf = s.model.b.detach().clone(), s.model.running_mean.clone()
    assert s.load_ema_weights(ckpt) == 2
    for i, (n, p) in enumerate(s.model.named_parameters()):
        if n == "b":
            assert torch.equal(p.detach(), kept_b)
        else:
            assert torch.equal(p.detach(), ckpt["optimizer_state_dict"]["state"][i]["ema"])
    assert torch.equal(s.model.running_mean, kept_buf)
    with pytest.raises(ValueError, match="no averaged weights"):
        s.load_ema_weights(_hand_built_checkpoint(with_ema=False)[2])
    with pytest.raises(ValueError, match="no averaged weights"):
        s.load_ema_weights({"model_state_dict": {}})
    ckpt["optimizer_state_dict"]["state"][1]["ema"] = torch.zeros(3, 3)
    before = [p.detach().clone() for p in s.model.parameters()]
    with pytest.raises(ValueError, match="shape"):
        s.load_ema_weights(ckpt)
    assert all(torch.equal(p.detach(), q) for p, q in zip(s.model.parameters(), before))   # nothing half-written


def test_header_declares_the_ema_entry_points():
    from rfn_hip import lib
    from tests.test_host_logic import _parse_header
    protos, _ = _parse_header()
    plain, guarded = protos["rfn_adam_step_f32"], protos["rfn_adam_step_guarded_f32"]
    tail = ["double ema_decay", "float* const* ema"]
    assert protos["rfn_adam_ema_step_f32"] == plain[:-1] + tail + plain[-1:]
    assert protos["rfn_adam_ema_step_guarded_f32"] == guarded[:-1] + tail + guarded[-1:]
    assert protos["rfn_param_swap_f32"] == plain[:3] + tail[1:] + plain[-1:]
    for name in ("rfn_adam_ema_step_f32", "rfn_adam_ema_step_guarded_f32", "rfn_param_swap_f32"):
        assert len(lib.SIGNATURES[name]) == len(protos[name])
