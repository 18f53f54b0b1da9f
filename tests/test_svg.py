"""The SVG baseline on the GPU, the LSTM cells on the KERNEL route (RFN_LSTM_CELL=1 for every test here), against the
reference's CPU run of tests/golden/svg*.pt (make_golden_svg.py): B = 4, T = 3, 64x64, c_features 8, h_dim 16, z_dim 4,
posterior / predictor / prior layers 1 / 2 / 1, range "none" — gray mse, RGB mse, bernoulli on binary frames, gaussian.
Parameters are not stored: both sides fill the state_dict from tests/srnn_state.fill_state, and the fixture's checksums
tell that they did.

Bounds: losses 1e-4 relative (nll_rel).  There is NO gradient comparison against the reference: the generator's criterion
(per tensor in the L2 norm, the reference's own 21 float32 calls within 5e-4 of its float64 replay) is met by no seed of
twelve in any configuration (the default call alone misses by 2e-3 to 2e-2, for bernoulli 0.2 to 0.4: batch statistics
over four rows), so the fixtures hold no gradients, which is asserted together with the stored figures; the comparison of
the two routes below stands in for it.  Generated frames 1e-4 absolute (the reference's float32 frames lie within 2.5e-5 of its float64 replay, asserted from the fixture).  The importance-weighted
bound (K = 2, eval mode) lies within max(4 |ref32 - ref64|, 1e-4 |ref64|) of the float64 replay, and the deferred decoder
within 1e-5 relative of per-k evaluation.  predict_draws at one draw is predict fed keyed_normal at the documented
addresses: first generated frame bit for bit, later frames within 1e-5, under deterministic convolutions.  One eager Solver
step on synthetic data writes svg.pt with the reference's checkpoint keys.

DESIGN.md section 22 holds the figures measured on an MI355X."""
import os
from argparse import Namespace

import pytest
import torch

from tests.srnn_state import describe, fill_state
from tests.test_hip_modules import nll_rel
from tests.test_svg_host import CONFIGS, FX, GOLD, frames

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 20261020


@pytest.fixture(autouse=True)
def kernel_route(monkeypatch):
    monkeypatch.setenv("RFN_LSTM_CELL", "1")


@pytest.fixture(scope="module")
def models():
    """per configuration: (model on the GPU in the filled state, the filled state, loss part, generation part, x)"""
    cache = {}

    def get(name):
        if name not in cache:
            from SVG import SVG
            assert torch.cuda.is_available(), "GPU tests need a device"
            c = FX["configs"][name]
            m = SVG(Namespace(**c["args"]))
            state = fill_state(m.state_dict(), c["seed"])
            assert describe(state)[2] == pytest.approx(c["checksums"], rel=1e-12, abs=1e-12)
            m.load_state_dict(state)
            parts = [torch.load(os.path.join(GOLD, p), weights_only=True) for p in c["parts"]]
            x = frames(parts[0]["k"], m.loss_type).to(DEV)
            cache[name] = (m.to(DEV), state, parts[0], parts[1], x)
        return cache[name]
    return get


@pytest.fixture
def deterministic_convolutions():
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture
def cell_calls(monkeypatch):
    """counts the launches of the two entry points"""
    from rfn_hip import lib as L
    seen, orig = {"rfn_lstm_cell_fwd_f32": 0, "rfn_lstm_cell_bwd_f32": 0}, L.call

    def call(name, *a, **k):
        if name in seen:
            seen[name] += 1
        return orig(name, *a, **k)
    monkeypatch.setattr(L, "call", call)
    return seen


@pytest.mark.parametrize("name", CONFIGS)
def test_loss_and_gradients(models, name, cell_calls):
    m, state, f, _, x = models(name)
    m.load_state_dict(state)
    m.train()
    m.zero_grad(set_to_none=True)
    T = x.shape[1]
    kl, nll = m.loss(x, draws=f["draws"])
    (nll + 0.3 * kl).backward()
    print("%s: kl %.6f (ref %.6f, float64 %.6f)  nll %.6f (ref %.6f, float64 %.6f)" %
          (name, float(kl.detach()), f["out"][0], f["out64"][0], float(nll.detach()), f["out"][1], f["out64"][1]))
    # four cells per step (predictor 2, posterior 1, prior 1), each one launch each way
    assert cell_calls == {"rfn_lstm_cell_fwd_f32": 4 * (T - 1), "rfn_lstm_cell_bwd_f32": 4 * (T - 1)}
    nll_rel(kl, torch.tensor(f["out"][0]))
    nll_rel(nll, torch.tensor(f["out"][1]))
    # the encoder's running statistics moved twice per step, the decoder's once
    tracked = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
    assert len(tracked) == 21
    for k, v in tracked.items():
        assert v == (2 * (T - 1) if k.startswith("encoder.") else T - 1), (k, v)
    # no seed of twelve met the generator's gradient criterion in any configuration: there is no
    # gradient fixture, and the figures that refused the seeds are stored
    assert f["grads"] == {} and f["n_float32_calls"] == 21
    assert max(f["grads_rel_l2_default"].values()) > 5e-4 and sorted(f["grads_rel_l2_ref"]) == sorted(FX["grad_names"])


def test_the_torch_route_computes_the_same_loss(models, monkeypatch, cell_calls):
    m, state, f, _, x = models("gray_mse")
    m.load_state_dict(state)
    m.train()
    kl, nll = m.loss(x, draws=f["draws"])
    n_kernel = cell_calls["rfn_lstm_cell_fwd_f32"]
    monkeypatch.setenv("RFN_LSTM_CELL", "0")
    m.load_state_dict(state)
    kl0, nll0 = m.loss(x, draws=f["draws"])
    assert n_kernel == 8 and cell_calls["rfn_lstm_cell_fwd_f32"] == n_kernel       # RFN_LSTM_CELL=0 launched none
    assert float(kl0.detach()) == pytest.approx(float(kl.detach()), rel=1e-5)
    assert float(nll0.detach()) == pytest.approx(float(nll.detach()), rel=1e-5)


def test_gradients_of_the_two_routes_agree_with_running_statistics(models, monkeypatch):
    """No configuration has a gradient fixture (the reference's own float32 gradients miss its float64 replay by 3e-3 to
    1e-2 in the L2 norm on every seed: batch statistics over four rows), and the cell's gradients
    are held against float64 in tests/test_lstm_cell.py.  What is left to check is that the model feeds them through:
    with the batch norms on their running statistics (eval mode: the network is then a plain stack of convolutions) the
    gradients of loss = nll + 0.3 kl on the kernel route and on the torch route, both float32 on the same device, agree
    per named tensor to 2e-4 in the L2 norm, the absolute term of the gradient criterion."""
    m, state, f, _, x = models("gray_mse")
    grads = {}
    for route in ("1", "0"):
        monkeypatch.setenv("RFN_LSTM_CELL", route)
        m.load_state_dict(state)
        m.eval()
        m.zero_grad(set_to_none=True)
        kl, nll = m.loss(x, draws=f["draws"])
        (nll + 0.3 * kl).backward()
        named = dict(m.named_parameters())
        grads[route] = {n: named[n].grad.detach().double().clone() for n in FX["grad_names"]}
    report = {n: float((grads["1"][n] - grads["0"][n]).norm() / grads["0"][n].norm()) for n in FX["grad_names"]}
    print("kernel route against torch route, ||g1 - g0|| / ||g0||: %s" % {n: "%.1e" % r for n, r in report.items()})
    for n, r in report.items():
        assert float(grads["0"][n].norm()) > 0 and r <= 2e-4, (n, r)


@pytest.mark.parametrize("name", CONFIGS)
def test_predict_and_reconstruct(models, name):
    m, state, f, gen, x = models(name)
    assert gen["gen_err64"] <= 2.5e-5            # what the generator accepted the input by
    m.load_state_dict(state)
    m.eval()
    p, r = gen["predict"], gen["reconstruct"]
    with torch.no_grad():
        tx, pr = m.predict(x, p["n_predictions"], p["n_conditions"], draws=p["draws"])
        rc = m.reconstruct(x, draws=r["draws"])
    assert not tx.is_cuda and not pr.is_cuda and not rc.is_cuda
    assert torch.equal(tx, x[:, :1].transpose(0, 1).cpu())
    assert pr.shape == p["predictions"].shape and rc.shape[1:] == r["recons_from_1"].shape[1:]
    assert rc.shape[0] == x.shape[1] and float(rc[0].abs().max()) == 0.0
    err_p = [float((pr[k] - p["predictions"][k]).abs().max()) for k in range(len(pr))]
    err_r = [float((rc[k + 1] - r["recons_from_1"][k]).abs().max()) for k in range(len(rc) - 1)]
    print("%s: predicted frames differ by %s, reconstructed by %s" %
          (name, ["%.2e" % e for e in err_p], ["%.2e" % e for e in err_r]))
    assert max(err_p) <= 1e-4 and max(err_r) <= 1e-4


def test_sample_runs_and_draws_its_own_noise(models):
    m, state, f, _, x = models("gray_mse")
    m.load_state_dict(state)
    m.eval()
    with torch.no_grad():
        s, s2 = m.sample(x, 3), m.sample(x, 3)
    assert s.shape == (3, 4, 1, 64, 64) and bool(torch.isfinite(s).all()) and not s.is_cuda
    assert float(s[0].abs().max()) == 0.0 and 0.0 < float(s[1:].max()) <= 1.0 and not torch.equal(s, s2)


# ------------------------------------------------------------------------------------- the importance-weighted bound
@pytest.mark.parametrize("name", CONFIGS)
def test_importance_weighted_bound_against_the_reference(models, name):
    m, state, _, _, _ = models(name)
    m.load_state_dict(state)
    m.eval()
    f = torch.load(os.path.join(GOLD, "svg_iw.%s.pt" % name), weights_only=True)
    assert f["K"] == 2 and f["mode"] == "eval"
    assert abs(f["ref32"] - f["ref64"]) <= 1e-4 * abs(f["ref64"])       # what the generator accepted the input by
    x = frames(f["k"], m.loss_type).to(DEV)
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
    m, state, f, _, x = models("gray_mse")
    m.load_state_dict(state)
    m.eval()
    with torch.no_grad():
        a = float(m.elbo_importance_weighting(x, 2))
        b = float(m.elbo_importance_weighting(x, 2))
    assert a == a and abs(a) != float("inf") and a != b
    with pytest.raises(ValueError, match="K must be"):
        m.elbo_importance_weighting(x, 0)
    with pytest.raises(RuntimeError, match="left over"):
        g = torch.load(os.path.join(GOLD, "svg_iw.gray_mse.pt"), weights_only=True)
        with torch.no_grad():
            m.elbo_importance_weighting(x[:, :2], 2, draws=g["draws"])     # recorded for T = 3


# ------------------------------------------------------------------------------------- predict_draws
def _draw_list(m, B, n_pred, n_cond, seed, first_seq, first_draw):
    """the `draws` list of SVG.predict for one draw id, from the documented addresses: conditioning step i: t = i,
    keyed_normal slot 0 = posterior eps, slot 1 = prior eps; generated frame i: t = n_cond + i, slot 0 = prior eps"""
    from rfn_hip import ops
    out = []
    for i in range(1, n_cond):
        out += ops.keyed_normal([(m.z_dim,), (m.z_dim,)], B, 1, seed, i, first_seq, first_draw, device=DEV)
    for i in range(n_pred):
        out += ops.keyed_normal([(m.z_dim,)], B, 1, seed, n_cond + i, first_seq, first_draw, device=DEV)
    return out


@pytest.mark.parametrize("name", ["gray_mse", "rgb_mse"])
def test_predict_draws_is_predict_fed_the_same_noise(models, name, deterministic_convolutions):
    m, state, f, _, x = models(name)
    m.load_state_dict(state)
    m.eval()
    B = x.shape[0]
    n_cond, n_pred = 2, 3
    for first_seq, first_draw in ((0, 0), (8, 5)):
        tx, pr = m.predict_draws(x, n_pred, n_cond, 1, SEED, first_seq, first_draw)
        assert pr.shape == (n_pred, 1, B) + tuple(x.shape[2:]) and not pr.is_cuda
        with torch.no_grad():
            tx2, ref = m.predict(x, n_pred, n_cond, draws=_draw_list(m, B, n_pred, n_cond, SEED, first_seq, first_draw))
        assert torch.equal(tx, tx2) and torch.equal(tx, x[:, :n_cond].transpose(0, 1).cpu())
        assert torch.equal(pr[0, 0], ref[0])                                   # the first generated frame: bit for bit
        later = float((pr[1:, 0] - ref[1:]).abs().max())
        print("%s seq %d draw %d: later frames differ by %.3e" % (name, first_seq, first_draw, later))
        assert later <= 1e-5
    dev_tx, dev_pr = m._predict_draws_device(x, n_pred, n_cond, 1, SEED, 8, 5)
    assert dev_pr.is_cuda and torch.equal(dev_pr.cpu(), pr)
    dev_tx, dev_pr = m._predict_device(x, 1, n_cond)
    assert dev_pr.is_cuda and dev_tx.is_cuda and dev_pr.shape == (1, B) + tuple(x.shape[2:])
    # several draws: draw-major rows, each draw its own noise; a draw does not depend on how the draws are split
    _, three = m.predict_draws(x, 1, n_cond, 3, SEED, 8, 4)
    assert three.shape == (1, 3, B) + tuple(x.shape[2:])
    assert not torch.equal(three[:, 0], three[:, 1])
    assert float((three[0, 1] - pr[0, 0]).abs().max()) <= 1e-5              # draw 5 of sequences 8 .. 8 + B - 1


def test_predict_draws_refuses_training_mode_and_leaves_the_generator(models):
    m, state, f, _, x = models("gray_mse")
    m.load_state_dict(state)
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
def test_one_eager_solver_step(tmp_path, monkeypatch, cell_calls):
    import main_svg
    from SVG.trainer import Solver
    monkeypatch.chdir(tmp_path)
    args = main_svg.build_parser().parse_args(
        "--synthetic_data --max_steps 1 --n_epochs 1 --batch_size 2 --n_frames 3 --image_size 64 --digit_size 12 "
        "--x_dim 2 1 64 64 --condition_dim 2 1 64 64 --c_features 8 --h_dim 16 --z_dim 4 --num_workers 0 "
        "--path /run/".split())
    torch.manual_seed(3)
    s = Solver(args)
    s.build()
    before = {k: v.detach().clone() for k, v in s.model.state_dict().items()}
    s.train()
    assert s.counter == 1 and len(s.losses) == 1
    assert cell_calls == {"rfn_lstm_cell_fwd_f32": 8, "rfn_lstm_cell_bwd_f32": 8}
    for v in (s.losses[0], s.kl_loss[0], s.recon_loss[0], s.bits[0]):
        assert v == v and abs(v) != float("inf")
    after = s.model.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values() if v.is_floating_point())
    for k in ("decoder.out.1.weight", "frame_predictor.lstm.1.weight_hh", "posterior.lstm.0.bias_ih"):
        assert not torch.equal(before[k], after[k]), k
    path = tmp_path / "run" / "model_folder" / "svg.pt"
    ckpt = Solver.read_checkpoint(str(path))
    assert sorted(ckpt) == FX["checkpoint_keys"]
    assert sorted(ckpt["model_state_dict"]) == sorted(before)
    assert ckpt["args"].variance == 1.0
