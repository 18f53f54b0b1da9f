"""CPU tests of RFN's importance-weighted bound: the rule that combines a table of log weights,
the argument errors of RFN.iw_log_weights / RFN.elbo_importance_weighting (raised before any kernel is touched), the
Evaluator's route (settings.rfn_iw_samples), tools/eval_iw_bound.py's parser, and the host restatement of the addressed
uniforms that tests/test_iw_kernels.py compares the kernel with."""
import importlib.util
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import iw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the combine rule
@pytest.mark.parametrize("K,B", [(1, 1), (1, 5), (2, 3), (20, 7)])
def test_combine_rule(K, B):
    from RFN.RFN_new import iw_bound
    g = torch.Generator().manual_seed(100 * K + B)
    # log weights of the size the model gives (thousands of nats) with a spread that underflows a naive exp
    table = -3000.0 + 400.0 * torch.randn(K, B, generator=g, dtype=torch.float64)
    got = iw_bound(table)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B,)
    want = torch.logsumexp(table, 0) - math.log(K)
    assert torch.allclose(got, want, rtol=1e-14, atol=0.0), (got, want)
    assert torch.equal(iw_ref.iw_bound_ref(table), want)
    if K == 1:
        assert torch.equal(got, table[0])
    # adding c to every entry shifts the bound by c
    for c in (-123.5, 1e4):
        assert torch.allclose(iw_bound(table + c), want + c, rtol=1e-13, atol=0.0)
    # never below the mean of the log weights (Jensen), up to rounding
    assert bool((got >= table.mean(0) - 1e-9 * table.abs().max()).all())
    if K > 1:
        assert bool((got > table.mean(0)).any())
    with pytest.raises(ValueError, match="log_w"):
        iw_bound(table[0])


# ---------------------------------------------------------------------------------------------- argument errors
@pytest.fixture(scope="module")
def cpu_model():
    import __graft_entry__ as ge
    from RFN import RFN
    torch.manual_seed(0)
    return RFN(ge._tiny_args()).eval()


def test_argument_errors_before_any_kernel(cpu_model):
    m = cpu_model
    x = torch.zeros(2, 4, 1, 16, 16)   # on the CPU: a launch would raise "no CPU fallback", not these
    for call in (lambda **k: m.iw_log_weights(x, seed=1, **k), lambda **k: m.elbo_importance_weighting(x, **k)):
        for bad in (0, -3):
            with pytest.raises(ValueError, match="K must be at least 1"):
                call(K=bad)
        with pytest.raises(ValueError, match="K must be an integer"):
            call(K=2.5)
        for bad in (0, -1):
            with pytest.raises(ValueError, match="chains_per_pass must be at least 1"):
                call(K=4, chains_per_pass=bad)
        with pytest.raises(ValueError, match="chains_per_pass must be an integer"):
            call(K=4, chains_per_pass=1.5)
        m.train()
        try:
            with pytest.raises(RuntimeError, match="eval mode"):
                call(K=4)
        finally:
            m.eval()
    with pytest.raises(ValueError, match="2 frames"):
        m.iw_log_weights(x[:, :1], 2, 1)


def test_ops_refuse_bad_arguments():
    from rfn_hip import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.keyed_uniform((4,), 1, 1, 0, 0, device="cpu")
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.keyed_uniform(None, 1, 1, 0, 0, out=torch.zeros(1, 1, 4))
    with pytest.raises(ValueError, match="slot"):
        ops.keyed_uniform((4,), 1, 1, 0, 0, slot=7, device="cuda")
    with pytest.raises(ValueError, match="slot"):
        ops.keyed_uniform((4,), 1, 1, 0, 0, slot=1 << 31, device="cuda")
    with pytest.raises(TypeError, match="slot"):
        ops.keyed_uniform((4,), 1, 1, 0, 0, slot=24.0, device="cuda")
    with pytest.raises(ValueError, match="seed"):
        ops.keyed_uniform((4,), 1, 1, -1, 0, device="cuda")
    with pytest.raises(ValueError, match="steps"):
        ops.keyed_uniform((4,), 1, 1, 0, (1 << 31) - 1, n_steps=2, device="cuda")
    with pytest.raises(ValueError, match="scale"):
        ops.keyed_uniform((4,), 1, 1, 0, 0, scale=0.0, device="cuda")
    with pytest.raises(ValueError, match="scale"):
        ops.keyed_uniform((4,), 1, 1, 0, 0, scale=float("inf"), device="cuda")
    with pytest.raises(ValueError, match="out must be"):
        ops.keyed_uniform(None, 2, 1, 0, 0, out=torch.zeros(1, 1, 4))
    with pytest.raises(TypeError, match="shape or out"):
        ops.keyed_uniform(None, 1, 1, 0, 0)
    enc = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.latent_iw(enc.clone().requires_grad_(True), enc, torch.zeros(2, 4), False)
    with pytest.raises(ValueError, match="eps_q"):
        ops.latent_iw(enc, enc, torch.zeros(2, 3), False)
    with pytest.raises(ValueError, match="enc_raw and pri_raw"):
        ops.latent_iw(enc, torch.zeros(2, 6), torch.zeros(2, 4), False)
    with pytest.raises(ValueError, match="rows >= 1"):
        ops.latent_iw(enc[:0], enc[:0], torch.zeros(0, 4), False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.latent_iw(enc, enc, torch.zeros(2, 4), False)


# ---------------------------------------------------------------------------------------------- the uniform's addresses
def test_uniform_restatement():
    """every coordinate of the address changes the values; a prefix of a longer row is the shorter row; the values lie
    in [0, scale), also at the largest half-word; slot 0 of the normal noise shares no Philox block with slot 24"""
    base = iw_ref.keyed_uniform_row(24, 1, 2, 24, 4, 5)
    assert base.dtype == np.float32 and base.shape == (24,)
    assert np.array_equal(base[:15], iw_ref.keyed_uniform_row(15, 1, 2, 24, 4, 5))
    for other in ((2, 2, 24, 4, 5), (1, 3, 24, 4, 5), (1, 2, 25, 4, 5), (1, 2, 24, 5, 5), (1, 2, 24, 4, 6)):
        assert not np.array_equal(base, iw_ref.keyed_uniform_row(24, *other))
    for scale in (1.0, 2.0 ** -8, 0.3, 3.0):
        v = iw_ref.keyed_uniform_row(1 << 14, 7, 1, 24, 0, 0, scale)
        assert float(v.min()) >= 0.0 and float(v.max()) < np.float32(scale)
        top = np.float32((1 << 24) - 1) * np.float32(2.0 ** -24) * np.float32(scale)
        assert top < np.float32(scale)
    v = iw_ref.keyed_uniform_row(1 << 16, 20261019, 3, 24, 0, 0)
    assert abs(float(v.mean()) - 0.5) <= 5.0 / math.sqrt(12 * v.size)
    whole = iw_ref.keyed_uniform_ref(5, 3, 2, 9, 4, n_steps=2, first_seq=7, first_draw=2)
    assert whole.shape == (2, 6, 5)
    assert np.array_equal(whole[1, 1 * 3 + 2], iw_ref.keyed_uniform_row(5, 9, 5, 24, 9, 3))


# ---------------------------------------------------------------------------------------------- the Evaluator's route
class _SpyModel(object):
    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def loss(self, x, logdet=0):
        self.calls.append(("loss", tuple(x.shape)))
        return torch.tensor(0.0), torch.tensor(1.0), torch.tensor(2.0)

    def elbo_importance_weighting(self, x, K, seed=0, first_seq=0, chains_per_pass=None):
        self.calls.append(("iw", tuple(x.shape), K, seed, first_seq, chains_per_pass))
        return torch.tensor(100.0 + first_seq + 10 * seed, dtype=torch.float64)


def _spy_evaluator(**settings):
    from evaluation_metrics import Evaluator
    model = _SpyModel()
    solver = SimpleNamespace(model=model, args=SimpleNamespace(n_frames=4, n_conditions=2, batch_size=2),
                             device=torch.device("cpu"), preprocess=lambda x, reverse=False: x)
    return Evaluator(solver, settings=SimpleNamespace(**settings)), model


def test_get_loss_route():
    batches = [torch.zeros(2, 6, 1, 16, 16) for _ in range(3)]
    for off in ({}, {"rfn_iw_samples": None}, {"rfn_iw_samples": 0}):
        ev, model = _spy_evaluator(seed=5, **off)
        assert ev.rfn_iw_samples == 0
        mean, std = ev.get_loss("rfn.pt", loader=batches)
        assert model.calls == [("loss", (2, 4, 1, 16, 16))] * 3
        assert float(mean) == pytest.approx(3.0 / (math.log(2.0) * 256 * 3)) and std == -1
    ev, model = _spy_evaluator(seed=5, rfn_iw_samples=7, iw_chains_per_pass=3)
    assert ev.rfn_iw_samples == 7 and ev.iw_chains_per_pass == 3
    mean, std = ev.get_loss("rfn.pt", loss_resamples=2, loader=batches, max_batches=2)
    shape = (2, 4, 1, 16, 16)
    assert model.calls == [("iw", shape, 7, 5, 0, 3), ("iw", shape, 7, 5, 2, 3),
                           ("iw", shape, 7, 6, 0, 3), ("iw", shape, 7, 6, 2, 3)]
    per = [[(100.0 + fs + 10 * s) / (math.log(2.0) * 256 * 3) for fs in (0, 2)] for s in (5, 6)]
    want = torch.FloatTensor(per)
    assert float(mean) == pytest.approx(float(want.mean()), rel=1e-6)
    assert float(std) == pytest.approx(float(want.std()), rel=1e-4)   # over all entries, as get_loss always did
    # the baselines' branch and the refusals are what they were
    ev, model = _spy_evaluator(rfn_iw_samples=7, iw_samples=4)
    model.elbo_importance_weighting = lambda x, K: model.calls.append(("srnn", K)) or torch.tensor(1.0)
    ev.get_loss("srnn.pt", loader=batches[:1])
    assert model.calls == [("srnn", 4)]
    for name in ("svg.pt", "vrnn.pt"):
        with pytest.raises(ValueError, match="only srnn.pt"):
            ev.get_loss(name, loader=batches)


# ---------------------------------------------------------------------------------------------- the tool's parser
def _tool():
    spec = importlib.util.spec_from_file_location("eval_iw_bound", os.path.join(ROOT, "tools", "eval_iw_bound.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parser_splits_its_flags_from_the_drivers(capsys):
    from evaluation_metrics import eval_settings
    tool = _tool()
    argv = ["--folder_path", "runs/", "--iw_samples", "7", "--experiment_names", "a", "b", "--chains_per_pass", "3",
            "--seed", "4", "--max_batches", "2"]
    K, P, rest = tool.split_args(argv)
    assert (K, P) == (7, 3)
    assert rest == ["--folder_path", "runs/", "--experiment_names", "a", "b", "--seed", "4", "--max_batches", "2"]
    s = tool.parse_args(argv)
    assert (s.rfn_iw_samples, s.iw_chains_per_pass, s.seed, s.max_batches) == (7, 3, 4, 2)
    assert s.folder_path == "runs/" and s.experiment_names == ["a", "b"]
    plain = eval_settings.parse_args(rest)
    for k, v in vars(plain).items():   # everything else is what the driver's parser gives
        assert getattr(s, k) == v, k
    assert not hasattr(plain, "rfn_iw_samples") and not hasattr(plain, "iw_chains_per_pass")
    d = tool.parse_args([])
    assert (d.rfn_iw_samples, d.iw_chains_per_pass) == (20, None)
    for bad in (["--iw_samples", "0"], ["--chains_per_pass", "0"], ["--no_such_flag", "1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    with pytest.raises(SystemExit):       # the driver's own parser has no such flag
        eval_settings.parse_args(["--iw_samples", "7"])
    capsys.readouterr()
    lines = tool.report_lines("a", 1.25, 1.125, 7, 3, 4)
    assert "1.250000" in lines[1] and "1.125000" in lines[2] and "K: 7" in lines[3] and "seed: 4" in lines[3]
