"""The VRNN baseline on the GPU against the reference's CPU run of tests/golden/vrnn*.pt (make_golden_vrnn.py): tiny
configurations (B = 4, T = 4, 32x32, h_dim = 8, z_dim = 4, n_logistics = 3, range "1.0") — gray mol, RGB mol, bernoulli
on binary frames, all without norm layers, and gray mol with the default batch norm for the losses, the generation paths
and the bound only (a bias in front of a batch norm has a zero true gradient: no relative gradient comparison there).
Parameters are not stored: both sides fill the state_dict from tests/srnn_state.fill_state, and the fixture's checksums
tell that they did.

Bounds, those of tests/test_srnn.py and tests/test_srnn_eval.py: losses 1e-4 relative (nll_rel), gradients grads_close
(rtol 2e-3 + 2e-4 of the tensor's maximum) against the reference's training call replayed in float64, generated frames
1e-4 absolute.  A generated pixel whose two best Gumbel scores differ by less than 1e-4 is left out (at most 1 %; the
generator accepted its inputs at 0.25 % on the reference's own logits); predict() feeds its frames back, so frames
after one with such a pixel are not compared.  The importance-weighted bound (K = 2, eval mode) lies within
max(4 |ref32 - ref64|, 1e-4 |ref64|) of the reference's float64 replay, and the deferred decoder within 1e-5 relative of
per-k evaluation.  predict_draws at one draw is predict fed keyed_normal / mol_keyed_uniforms at the documented
addresses: first generated frame bit for bit, later frames within 1e-5, under deterministic convolutions (DESIGN.md
section 20 explains why).  One eager Solver step on synthetic data writes vrnn.pt with the reference's checkpoint
keys.

Measured on an MI355X: gradients, worst error / bound over the thirteen tensors: gray_mol 0.013,
rgb_mol 0.014, bernoulli 0.010; generated frames within 1.4e-6; the bound, error / bound: 3.0e-4, 2.8e-4, 7.9e-4, 1.2e-4;
deferred decoder against per-k evaluation 0; predict_draws: later frames differ by 0.
The gradient comparison is sensitive to the last bits of torch's convolutions, which differ run to run on the GPU: the
inputs are chosen so that the reference's own float32 call stays within a quarter of the bound under four CPU
arithmetics and 16 calls with one unit of round-off of noise on every layer output (asserted below from the fixture),
yet one of five runs of this build missed (gray_mol, one element of h_0 at 1.28 of its bound).  Deterministic
convolutions are no remedy: under them bernoulli's c_0 misses the bound 4 times in every run."""
import os
from argparse import Namespace

import pytest
import torch

from tests import mol_ref as R
from tests.srnn_state import describe, fill_state
from tests.test_hip_modules import grads_close, nll_rel
from tests.test_vrnn_host import CONFIGS, FX, GOLD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 20261020
GRAD_CONFIGS = [n for n in CONFIGS if n != "gray_mol_batchnorm"]


@pytest.fixture(scope="module")
def models():
    """per configuration: (model on the GPU in the filled state, the filled state, loss part, generation part)"""
    cache = {}

    def get(name):
        if name not in cache:
            from VRNN import VRNN
            assert torch.cuda.is_available(), "GPU tests need a device"
            c = FX["configs"][name]
            m = VRNN(Namespace(**c["args"]))
            state = fill_state(m.state_dict(), c["seed"])
            assert describe(state)[2] == pytest.approx(c["checksums"], rel=1e-12, abs=1e-12)
            m.load_state_dict(state)
            parts = [torch.load(os.path.join(GOLD, p), weights_only=True) for p in c["parts"]]
            cache[name] = (m.to(DEV), state, parts[0], parts[1])
        return cache[name]
    return get


@pytest.fixture
def deterministic_convolutions():
    """for the bit-for-bit comparison: the strided convolutions and deconvolutions are torch modules whose default
    algorithms add split-K slices with float atomics (tests/test_srnn_eval.py)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("name", CONFIGS)
def test_loss_and_gradients(models, name):
    m, state, f, _ = models(name)
    m.load_state_dict(state)
    m.train()
    m.zero_grad(set_to_none=True)
    kl, nll = m.loss(f["x"].to(DEV), draws=f["draws"])
    (nll + 0.3 * kl).backward()
    print("%s: kl %.6f (ref %.6f, float64 %.6f)  nll %.6f (ref %.6f, float64 %.6f)" %
          (name, float(kl.detach()), f["out"][0], f["out64"][0], float(nll.detach()), f["out"][1], f["out64"][1]))
    nll_rel(kl, torch.tensor(f["out"][0]))
    nll_rel(nll, torch.tensor(f["out"][1]))
    if name in GRAD_CONFIGS:
        assert len(f["grads"]) == 13 and max(v.numel() for v in f["grads"].values()) <= 120000
        assert m.z_0.grad is None                     # z_0 is never used by the loss
        # the yardstick was checked: the reference's own float32 call, under each float32 arithmetic of the generator,
        # stays within a quarter of the bound of its float64 replay on this input
        assert len(f["grads32_ratio_variants"]) == 4
        assert max([f["grads32_ratio"]] + list(f["grads32_ratio_variants"].values())) <= 0.25
        assert len(f["grads32_ratio_noise"]) == 16 and max(f["grads32_ratio_noise"]) <= 0.25
        grads_close(m, f["grads"])
    else:
        assert f["grads"] == {}
        # the running statistics of phi_x_t moved twice per step: 2 (T - 1) calls
        tracked = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
        assert len(tracked) == 12
        T = f["x"].shape[1]
        for k, v in tracked.items():   # phi_z: once for the LSTM, once for the decoder; the others once per step
            assert v == (2 * (T - 1) if k.startswith(("phi_x_t.", "phi_z.")) else T - 1), (k, v)


def _record_samples(monkeypatch):
    """every mol_sample call of the code under test: (logits, u_mix, u_x) on the CPU"""
    from rfn_hip import ops
    calls, orig = [], ops.mol_sample

    def rec(l, u_mix=None, u_x=None, **kw):
        calls.append((l.detach().cpu(), u_mix.detach().cpu(), u_x.detach().cpu()))
        return orig(l, u_mix, u_x, **kw)
    monkeypatch.setattr(ops, "mol_sample", rec)
    return calls


def _keep_masks(calls, shape):
    """[frames] of [B,C,H,W] bool: pixels whose component choice is no near tie"""
    out = []
    for l, u_mix, u_x in calls:
        _, gap = R.sample(l.double(), u_mix.double(), u_x.double())
        out.append((gap >= 1e-4).unsqueeze(1).expand(shape))
    return out


@pytest.mark.parametrize("name", CONFIGS)
def test_predict_and_reconstruct(models, name, monkeypatch):
    m, state, f, gen = models(name)
    x = f["x"]
    mol = FX["configs"][name]["args"]["loss_type"] == "mol"
    assert gen["near_ties"] <= 0.0025
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
    assert not tx.is_cuda and not pr.is_cuda and not rc.is_cuda
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
        s2 = m.sample(f["x"].to(DEV), 2)
    assert s.shape == (2, 4, 1, 32, 32) and bool(torch.isfinite(s).all()) and float(s.abs().max()) <= 1.0
    assert not s.is_cuda and not torch.equal(s, s2)


# ------------------------------------------------------------------------------------- the importance-weighted bound
@pytest.mark.parametrize("name", CONFIGS)
def test_importance_weighted_bound_against_the_reference(models, name):
    m, state, _, _ = models(name)
    m.load_state_dict(state)
    m.eval()
    f = torch.load(os.path.join(GOLD, "vrnn_iw.%s.pt" % name), weights_only=True)
    assert f["K"] == 2 and f["mode"] == "eval"
    assert abs(f["ref32"] - f["ref64"]) <= 1e-4 * abs(f["ref64"])       # what the generator accepted the input by
    x = f["x"].to(DEV)
    with torch.no_grad():
        ours = float(m.elbo_importance_weighting(x, f["K"], draws=f["draws"]))
        per_k = float(m.elbo_importance_weighting(x, f["K"], draws=f["draws"], defer_decoder=False))
    bound = max(4 * abs(f["ref32"] - f["ref64"]), 1e-4 * abs(f["ref64"]))
    err = abs(ours - f["ref64"])
    print("%s: ours %.6f ref32 %.6f ref64 %.6f  error / bound %.3e (bound %.3e)  deferred against per-k %.2e relative" %
          (name, ours, f["ref32"], f["ref64"], err / bound, bound, abs(ours - per_k) / abs(per_k)))
    assert err <= bound
    assert abs(ours - per_k) <= 1e-5 * abs(per_k)


def test_importance_weighting_draws_its_own_noise_and_checks_K(models):
    m, state, f, _ = models("gray_mol")
    m.load_state_dict(state)
    m.eval()
    x = f["x"].to(DEV)
    with torch.no_grad():
        a = float(m.elbo_importance_weighting(x, 2))
        b = float(m.elbo_importance_weighting(x, 2))
    assert a == a and abs(a) != float("inf") and a != b
    with pytest.raises(ValueError, match="K must be"):
        m.elbo_importance_weighting(x, 0)
    with pytest.raises(RuntimeError, match="left over"):
        g = torch.load(os.path.join(GOLD, "vrnn_iw.gray_mol.pt"), weights_only=True)
        with torch.no_grad():
            m.elbo_importance_weighting(g["x"].to(DEV)[:, :3], 2, draws=g["draws"])     # recorded for T = 4


# ------------------------------------------------------------------------------------- predict_draws
def _draw_list(m, B, C, H, W, n_pred, n_cond, seed, first_seq, first_draw):
    """the `draws` list of VRNN.predict for one draw id, from the documented addresses: conditioning step i: t = i,
    keyed_normal slot 0 = prior eps, slot 1 = encoder eps (predict draws the prior first); generated frame i: t = n_cond +
    i, slot 0, then the sampler's u_mix, u_x at that step"""
    from rfn_hip import ops
    out = []
    for i in range(1, n_cond):
        out += ops.keyed_normal([(m.z_dim,), (m.z_dim,)], B, 1, seed, i, first_seq, first_draw, device=DEV)
    for i in range(n_pred):
        t = n_cond + i
        out += ops.keyed_normal([(m.z_dim,)], B, 1, seed, t, first_seq, first_draw, device=DEV)
        if m.loss_type == "mol":
            out += list(ops.mol_keyed_uniforms((B, H, W), B, m.n_logistics, C, seed, t, first_seq, first_draw, device=DEV))
    return out


@pytest.mark.parametrize("name", ["gray_mol", "rgb_mol", "bernoulli"])
def test_predict_draws_is_predict_fed_the_same_noise(models, name, deterministic_convolutions):
    m, state, f, _ = models(name)
    m.load_state_dict(state)
    m.eval()
    x = f["x"].to(DEV)
    B, _, C, H, W = x.shape
    n_cond, n_pred = 3, 3
    for first_seq, first_draw in ((0, 0), (8, 5)):
        tx, pr = m.predict_draws(x, n_pred, n_cond, 1, SEED, first_seq, first_draw)
        assert pr.shape == (n_pred, 1, B) + tuple(x.shape[2:]) and not pr.is_cuda
        with torch.no_grad():
            tx2, ref = m.predict(x, n_pred, n_cond, draws=_draw_list(m, B, C, H, W, n_pred, n_cond, SEED, first_seq,
                                                                     first_draw))
        assert torch.equal(tx, tx2) and torch.equal(tx, x[:, :n_cond].transpose(0, 1).cpu())
        assert torch.equal(pr[0, 0], ref[0])                                   # the first generated frame: bit for bit
        later = float((pr[1:, 0] - ref[1:]).abs().max())
        print("%s seq %d draw %d: later frames differ by %.3e" % (name, first_seq, first_draw, later))
        assert later <= 1e-5
    dev_tx, dev_pr = m._predict_draws_device(x, n_pred, n_cond, 1, SEED, 8, 5)
    assert dev_pr.is_cuda and torch.equal(dev_pr.cpu(), pr)
    dev_tx, dev_pr = m._predict_device(x, 1, n_cond)
    assert dev_pr.is_cuda and dev_tx.is_cuda and dev_pr.shape == (1, B) + tuple(x.shape[2:])
    # several draws: draw-major rows, each draw its own noise
    _, three = m.predict_draws(x, 1, n_cond, 3, SEED, 8, 4)
    assert three.shape == (1, 3, B) + tuple(x.shape[2:])
    assert not torch.equal(three[:, 0], three[:, 1])


def test_predict_draws_refuses_training_mode_and_leaves_the_generator(models):
    m, state, f, _ = models("gray_mol")
    m.load_state_dict(state)
    x = f["x"].to(DEV)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            m.predict_draws(x, 1, 2, 2, SEED)
    finally:
        m.eval()
    with pytest.raises(ValueError, match="n_draws"):
        m.predict_draws(x, 1, 2, 0, SEED)
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    m.predict_draws(x, 2, 2, 2, SEED)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(DEV), gpu_state)


# ------------------------------------------------------------------------------------- the Solver
def test_one_eager_solver_step(tmp_path, monkeypatch):
    import main_vrnn
    from VRNN.trainer import Solver
    monkeypatch.chdir(tmp_path)
    args = main_vrnn.build_parser().parse_args(
        "--synthetic_data --max_steps 1 --n_epochs 1 --batch_size 2 --n_frames 3 --image_size 32 --digit_size 12 "
        "--x_dim 2 1 32 32 --condition_dim 2 1 32 32 --h_dim 8 --z_dim 4 --n_logistics 3 --num_workers 0 "
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
    assert not torch.equal(before["dec_mean.0.weight"], after["dec_mean.0.weight"])
    path = tmp_path / "run" / "model_folder" / "vrnn.pt"
    ckpt = Solver.read_checkpoint(str(path))
    assert sorted(ckpt) == FX["checkpoint_keys"]
    assert sorted(ckpt["model_state_dict"]) == sorted(before)
    assert len(ckpt["model_state_dict"]) == 120
