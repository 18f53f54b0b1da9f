"""The SRNN baseline on the GPU against the reference's CPU run of tests/golden/srnn*.pt (make_golden_srnn.py): tiny
configurations (B = 4, T = 4, 32x32, h_dim = a_dim = 8, z_dim = 4, n_logistics = 3) — gray mol; RGB mol with res_q and
smoothing; gray mol with two over-shots; bernoulli without norm layers.  Parameters are not stored: both sides fill the
state_dict from tests/srnn_state.fill_state, and the fixture's checksums tell that they did.

The yardstick of the gradients is the reference's training call replayed in float64 (same state, same draws).  The four
gradient configurations run without norm layers, and "gray_mol_batchnorm" adds the default norm for the losses and the
generation paths only: through batch norms over B = 4 samples the reference's own float32 call misses its float64
replay by 1 to 60 times the gradient bound below (make_golden_srnn.py), which no float32
implementation can be held to.

Bounds (tests/test_hip_modules.py): losses 1e-4 relative (nll_rel), gradients grads_close (rtol 2e-3 + 2e-4 of the
tensor's maximum), generated frames 1e-4 absolute.  A generated pixel whose two best Gumbel scores differ by less than
1e-4 is left out (at most 1 %); predict() feeds its frames back, so frames after one with such a pixel are not compared.
One eager Solver step on synthetic data writes srnn.pt with the reference's checkpoint keys."""
import os
from argparse import Namespace

import pytest
import torch

from tests import mol_ref as R
from tests.srnn_state import describe, fill_state
from tests.test_hip_modules import grads_close, nll_rel
from tests.test_srnn_host import CONFIGS, FX, GOLD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def models():
    """per configuration: (model on the GPU in the filled state, the filled state, loss part, generation part)"""
    cache = {}

    def get(name):
        if name not in cache:
            from SRNN import SRNN
            assert torch.cuda.is_available(), "GPU tests need a device"
            c = FX["configs"][name]
            m = SRNN(Namespace(**c["args"]))
            state = fill_state(m.state_dict(), c["seed"])
            assert describe(state)[2] == pytest.approx(c["checksums"], rel=1e-12, abs=1e-12)
            m.load_state_dict(state)
            parts = [torch.load(os.path.join(GOLD, p), weights_only=True) for p in c["parts"]]
            cache[name] = (m.to(DEV), state, parts[0], parts[1])
        return cache[name]
    return get


@pytest.mark.parametrize("name", CONFIGS)
def test_loss_and_gradients(models, name):
    m, state, f, _ = models(name)
    m.load_state_dict(state)
    m.train()
    m.zero_grad(set_to_none=True)
    kl, nll = m.loss(f["x"].to(DEV), draws=f["draws"])
    (nll + 0.3 * kl).backward()
    print("%s: kl %.6f (ref %.6f)  nll %.6f (ref %.6f)" % (name, float(kl), f["out"][0], float(nll), f["out"][1]))
    nll_rel(kl, torch.tensor(f["out"][0]))
    nll_rel(nll, torch.tensor(f["out"][1]))
    assert len(f["grads"]) >= 10 or name == "gray_mol_batchnorm"   # (that one: losses only, see the module docstring)
    grads_close(m, f["grads"])


def _record_samples(monkeypatch):
    """every mol_sample call of the code under test: (logits, u_mix) on the CPU"""
    from rfn_hip import ops
    calls, orig = [], ops.mol_sample

    def rec(l, u_mix=None, u_x=None, **kw):
        calls.append((l.detach().cpu(), u_mix.detach().cpu(), u_x.detach().cpu()))
        return orig(l, u_mix, u_x, **kw)
    monkeypatch.setattr(ops, "mol_sample", rec)
    return calls


def _keep_masks(calls, shape):
    """[frames] of [B,C,H,W] bool: pixels whose component choice is no near tie; all True without a mixture"""
    out = []
    for l, u_mix, u_x in calls:
        _, gap = R.sample(l.double(), u_mix.double(), u_x.double())
        out.append((gap >= 1e-4).unsqueeze(1).expand(shape))
    return out


@pytest.mark.parametrize("name", CONFIGS)
def test_predict_and_reconstruct(models, name, monkeypatch):
    m, state, _, gen = models(name)
    f = FX["configs"][name]
    x = torch.load(os.path.join(GOLD, f["parts"][0]), weights_only=True)["x"]
    mol = f["args"]["loss_type"] == "mol"
    m.load_state_dict(state)
    m.eval()
    calls = _record_samples(monkeypatch)
    with torch.no_grad():
        p = gen["predict"]
        tx, pr = m.predict(x.to(DEV), p["n_predictions"], p["n_conditions"], draws=p["draws"])
        keep_p = _keep_masks(calls, pr[0].shape) if mol else [torch.ones_like(pr[0], dtype=torch.bool)] * len(pr)
        del calls[:]
        r = gen["reconstruct"]
        rc = m.reconstruct(x.to(DEV), draws=r["draws"])
        keep_r = _keep_masks(calls, rc[0].shape) if mol else [torch.ones_like(rc[0], dtype=torch.bool)] * (len(rc) - 1)
    assert torch.equal(tx, p["true_x"])
    assert pr.shape == p["predictions"].shape and rc.shape == r["recons"].shape
    assert len(keep_p) == len(pr) and len(keep_r) == len(rc) - 1
    compared = 0
    for k, keep in enumerate(keep_p):
        left_out = 1.0 - float(keep.float().mean())
        err = float((pr[k] - p["predictions"][k])[keep].abs().max())
        print("%s predict frame %d: error %.3e, left out %.4f" % (name, k, err, left_out))
        assert left_out <= 0.01 and err <= 1e-4
        compared += 1
        if left_out > 0.0:
            break   # the next frame is conditioned on this one, near ties included
    assert compared >= 1
    assert float(rc[0].abs().max()) == 0.0 and float(r["recons"][0].abs().max()) == 0.0
    for k, keep in enumerate(keep_r, start=1):
        left_out = 1.0 - float(keep.float().mean())
        err = float((rc[k] - r["recons"][k])[keep].abs().max())
        print("%s reconstruct frame %d: error %.3e, left out %.4f" % (name, k, err, left_out))
        assert left_out <= 0.01 and err <= 1e-4


def test_sample_runs_and_draws_its_own_noise(models):
    m, state, f, _ = models("gray_mol")
    m.load_state_dict(state)
    m.eval()
    with torch.no_grad():
        s = m.sample(f["x"].to(DEV), 2)
    assert s.shape == (2, 4, 1, 32, 32) and bool(torch.isfinite(s).all()) and float(s.abs().max()) <= 1.0


def test_one_eager_solver_step(tmp_path, monkeypatch):
    import main_srnn
    from SRNN.trainer import Solver
    monkeypatch.chdir(tmp_path)
    args = main_srnn.build_parser().parse_args(
        "--synthetic_data --max_steps 1 --n_epochs 1 --batch_size 2 --n_frames 3 --image_size 32 --digit_size 12 "
        "--x_dim 2 1 32 32 --condition_dim 2 1 32 32 --h_dim 8 --a_dim 8 --z_dim 4 --n_logistics 3 --num_workers 0 "
        "--path /run/".split())
    torch.manual_seed(3)
    s = Solver(args)
    s.build()
    before = {k: v.detach().clone() for k, v in s.model.state_dict().items()}
    s.train()
    assert s.counter == 1 and len(s.losses) == 1
    for v in (s.losses[0], s.kl_loss[0], s.recon_loss[0], s.bits[0]):
        assert v == v and abs(v) != float("inf")
    after = s.model.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point())
    assert any(not torch.equal(before[k], after[k]) for k in ("dec_mean.0.weight", "lstm_h.LSTMlayer.conv.0.weight"))
    path = tmp_path / "run" / "model_folder" / "srnn.pt"
    ckpt = Solver.read_checkpoint(str(path))
    assert sorted(ckpt) == FX["checkpoint_keys"]
    assert sorted(ckpt["model_state_dict"]) == sorted(before)
