"""Evaluating the SRNN baseline on the GPU: SRNN.elbo_importance_weighting against the reference's
CPU run of tests/golden/srnn_iw.*.pt (make_golden_srnn_iw.py), SRNN.predict_draws against SRNN.predict fed the same
noise and against itself at other batchings, and the Evaluator / eval_settings paths for srnn.pt.  The tiny
configurations of tests/golden/make_golden_srnn.py (B = 4, T = 4, 32x32, h_dim = a_dim = 8, z_dim = 4, M = 3), state
from tests/srnn_state.fill_state.

The importance-weighted bound replays the reference's recorded draws and must lie within
max(4 |ref32 - ref64|, 1e-4 |ref64|) of the reference's float64 replay: four times the reference's own float32 error
(section 19's yardstick), or the 1e-4 relative that tests/test_srnn.py holds losses to.

Measured on an MI355X, |ours - ref64| / bound (bound; deferred decoder against per-k evaluation, relative):
  gray_mol K=3              9.3e-4 (1.99; 9.8e-8)
  rgb_mol_resq_smooth K=2   5.1e-4 (5.84; 0)
  bernoulli_nonorm K=2      3.3e-4 (0.214; 0)
  gray_mol_batchnorm K=2    8.2e-5 (1.91; 0)
Independence of batching: bernoulli_nonorm P = 3 against P = 1, 2 + 3 frames: 8.1e-7 of the maximum; gray_mol first
generated frame: share of pixels off by more than 1e-4: 0 of 12288 (cap 0.005).
"""
import os
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

from tests.srnn_state import describe, fill_state
from tests.test_srnn_host import FX, GOLD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IW_CONFIGS = {"gray_mol": 3, "rgb_mol_resq_smooth": 2, "bernoulli_nonorm": 2, "gray_mol_batchnorm": 2}
SEED = 20261020


@pytest.fixture(scope="module")
def models():
    """per configuration: (model on the GPU in eval mode in the filled state, the input x of the loss fixture)"""
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
            x = torch.load(os.path.join(GOLD, c["parts"][0]), weights_only=True)["x"]
            cache[name] = (m.to(DEV).eval(), x.to(DEV))
        return cache[name]
    return get


@pytest.fixture
def deterministic_convolutions():
    """for the bit-for-bit comparisons.  The strided convolutions and deconvolutions of SRNN are torch modules, and
    the algorithms MIOpen picks by default for these few-pixel problems add their split-K slices with float
    atomics: SRNN.predict called twice with the SAME recorded draws differs from itself (measured on an MI355X: 2.4e-7
    in the first generated frame of bernoulli_nonorm, 1.1e-6 of gray_mol; SRNN.loss twice: kl differs by 7.6e-6), so no
    two passes can be compared bitwise.  With torch.backends.cudnn.deterministic every one of those pairs is equal bit for
    bit (same measurement)."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


# ------------------------------------------------------------------------------------- the importance-weighted bound
@pytest.mark.parametrize("name", list(IW_CONFIGS))
def test_importance_weighted_bound_against_the_reference(models, name):
    m, _ = models(name)
    f = torch.load(os.path.join(GOLD, "srnn_iw.%s.pt" % name), weights_only=True)
    assert f["K"] == IW_CONFIGS[name] and f["mode"] == "eval" and not m.training
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
    m, x = models("gray_mol")
    with torch.no_grad():
        a = float(m.elbo_importance_weighting(x, 2))
        b = float(m.elbo_importance_weighting(x, 2))
    assert a == a and abs(a) != float("inf") and a != b
    with pytest.raises(ValueError, match="K must be"):
        m.elbo_importance_weighting(x, 0)
    with pytest.raises(RuntimeError, match="left over"):
        f = torch.load(os.path.join(GOLD, "srnn_iw.gray_mol.pt"), weights_only=True)
        with torch.no_grad():
            m.elbo_importance_weighting(f["x"].to(DEV), 2, draws=f["draws"])     # recorded for K = 3


# ------------------------------------------------------------------------------------- predict_draws
def _draw_list(m, B, C, H, W, n_pred, n_cond, seed, first_seq, first_draw):
    """the `draws` list of SRNN.predict for one draw id, from the documented addresses: conditioning step i: t = i,
    keyed_normal slot 0; generated frame i: t = n_cond + i, slot 0, then the sampler's u_mix, u_x at that step"""
    from rfn_hip import ops
    out = []
    for i in range(1, n_cond):
        out += ops.keyed_normal([(m.z_dim,)], B, 1, seed, i, first_seq, first_draw, device=DEV)
    for i in range(n_pred):
        t = n_cond + i
        out += ops.keyed_normal([(m.z_dim,)], B, 1, seed, t, first_seq, first_draw, device=DEV)
        if m.loss_type == "mol":
            out += list(ops.mol_keyed_uniforms((B, H, W), B, m.n_logistics, C, seed, t, first_seq, first_draw, device=DEV))
    return out


@pytest.mark.parametrize("name", ["gray_mol", "rgb_mol_resq_smooth", "bernoulli_nonorm"])
def test_predict_draws_is_predict_fed_the_same_noise(models, name, deterministic_convolutions):
    m, x = models(name)
    B, _, C, H, W = x.shape
    n_cond, n_pred = 2, 3
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


def test_batching_does_not_change_the_draws_without_a_sampler(models):
    """bernoulli_nonorm: no discrete choice anywhere.  torch's convolutions and GEMMs may pick other algorithms at 12 rows
    than at 4, so not bit for bit: within 1e-4 of the tensor's maximum over 2 + 3 frames"""
    m, x = models("bernoulli_nonorm")
    _, all3 = m.predict_draws(x, 3, 2, 3, SEED, first_seq=4)
    worst = 0.0
    for r in range(3):
        _, one = m.predict_draws(x, 3, 2, 1, SEED, first_seq=4, first_draw=r)
        worst = max(worst, float((all3[:, r] - one[:, 0]).abs().max() / one.abs().max()))
    print("bernoulli_nonorm P = 3 against P = 1: %.3e of the maximum" % worst)
    assert worst <= 1e-4
    assert not torch.equal(all3[:, 0], all3[:, 1])
    # a second batch of sequences: other noise
    _, other = m.predict_draws(x, 3, 2, 1, SEED, first_seq=8, first_draw=0)
    assert not torch.equal(other[:, 0], all3[:, 0])


def test_batching_changes_few_mixture_pixels(models):
    """gray_mol, the FIRST generated frame (later ones are conditioned on it): its pixels agree within 1e-4 but for
    component flips, where two Gumbel scores are closer than the logits' rounding between batch sizes: at most 0.5 %"""
    m, x = models("gray_mol")
    _, all3 = m.predict_draws(x, 1, 2, 3, SEED)
    off, n = 0, 0
    for r in range(3):
        _, one = m.predict_draws(x, 1, 2, 1, SEED, first_draw=r)
        bad = (all3[0, r] - one[0, 0]).abs() > 1e-4
        off, n = off + int(bad.sum()), n + bad.numel()
    print("gray_mol first frame: %d of %d pixels differ by more than 1e-4 (share %.5f)" % (off, n, off / n))
    assert off / n <= 0.005


def test_predict_draws_refuses_training_mode_and_leaves_the_generator(models):
    m, x = models("gray_mol")
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


# ------------------------------------------------------------------------------------- the Evaluator
class _Solver(object):
    """what the Evaluator reads of a Solver, with SRNN's preprocess"""
    n_bits, preprocess_range, preprocess_scale = 8, "1.0", 255

    def __init__(self, model, path):
        from SRNN.trainer import Solver
        self.model, self.device, self.path = model, torch.device(DEV), path
        self.args = SimpleNamespace(n_frames=4, n_conditions=2, batch_size=4, choose_data="mnist")
        self.preprocess = lambda x, reverse=False: Solver.preprocess(self, x, reverse)


@pytest.fixture(scope="module")
def loader():
    g = torch.Generator().manual_seed(12)
    return [torch.randint(0, 256, (4, 5, 1, 32, 32), generator=g).float() / 255.0 for _ in range(2)]


@pytest.fixture(scope="module")
def short_loader():
    """two batches of 2 + 1 frames for the comparison of draws_per_pass 1 and 3, whose precondition is that the two runs
    generate the same uint8 frames.  SRNN's strided convolutions and deconvolutions are torch modules: at 12 rows they
    run other algorithms than at 4 (measured per module: phi_x_t, prior and dec differ by 2e-6, 4e-6 and 7e-7 between
    the row counts; Linear, ConvLSTM, dec_mean and the sampler do not), and a float that moves by 1e-7 across a
    quantisation boundary changes its uint8 level.  Counted over ten loader seeds (12 .. 21), values differing by one
    level, never by more: 1, 3, 0, 3, 0, 5, 0, 0, 2, 1 of 73728 at three predicted frames and 0, 0, 0, 1, 0, 0, 1, 1, 0, 1
    of 24576 at one.  So the comparison runs at the smallest exposure, one predicted frame, on a seed (16) on which no
    value moved at either length; with deterministic convolutions each pass repeats bit for bit."""
    g = torch.Generator().manual_seed(16)
    return [torch.randint(0, 256, (4, 3, 1, 32, 32), generator=g).float() / 255.0 for _ in range(2)]


def _evaluator(m, tmp_path, n_frames=5, **settings):
    from evaluation_metrics import Evaluator
    return Evaluator(_Solver(m, str(tmp_path) + "/"),
                     settings=SimpleNamespace(n_frames=n_frames, start_predictions=2, **settings))


def test_evaluator_best_of_n_does_not_depend_on_draws_per_pass(models, short_loader, tmp_path,
                                                               deterministic_convolutions):
    m, _ = models("gray_mol")
    loader, n_pred = short_loader, 1
    outs, preds = {}, {}
    plain = m._predict_draws_device
    for P in (1, 3):
        seen = []

        def spy(*a, _seen=seen, **k):
            tx, pr = plain(*a, **k)
            _seen.append(pr)
            return tx, pr
        m._predict_draws_device = spy
        try:
            ev = _evaluator(m, tmp_path, n_frames=3, resample=3, draws_per_pass=P, seed=SEED)
            torch.manual_seed(5)
            outs[P] = ev.get_eval_values("srnn.pt", loader=loader)
        finally:
            del m._predict_draws_device
        assert len(seen) == 2 * (3 // P)
        # uint8 [batch, draw, n_pred, B, C, H, W]
        u8 = [ev.solver.preprocess(p, reverse=True) for p in seen]
        preds[P] = torch.stack([torch.cat(u8[b * (3 // P):(b + 1) * (3 // P)], 1).transpose(0, 1) for b in range(2)])
    for P, out in outs.items():       # the reference's ten-element tuple, with the shapes of the RFN path
        assert len(out) == 10 and out[3] is None and out[9] is None
        for i in (0, 1, 2, 7, 8):
            assert tuple(out[i].shape) == (8, n_pred) and out[i].dtype == torch.float32 and not out[i].is_cuda
        for i in (4, 5, 6):
            assert tuple(out[i].shape) == (2,) and bool(torch.isfinite(out[i]).all())
    # BPD / DKL / RECON: compute_loss of model.loss(image) on the WHOLE sequence, replayed with the same generator state
    torch.manual_seed(5)
    ev = _evaluator(m, tmp_path, n_frames=3)
    with torch.no_grad():
        for b, batch in enumerate(loader):
            image = ev.solver.preprocess(batch.to(DEV))
            kl, nll = m.loss(image)
            want = ev.compute_loss(nll=nll, kl=kl, dims=image.shape[2:], t=image.shape[1] - 1)
            for P in (1, 3):
                assert tuple(float(outs[P][i][b]) for i in (4, 5, 6)) == tuple(float(torch.tensor(v, dtype=torch.float32))
                                                                               for v in want)
    # the precondition of the comparison: the two runs generated the same uint8 frames
    differing = int((preds[1] != preds[3]).sum())
    print("uint8 predictions differing between draws_per_pass 1 and 3: %d of %d" % (differing, preds[1].numel()))
    assert differing == 0, "the uint8 predictions of the two runs differ in %d of %d values" % (differing, preds[1].numel())
    for i in (0, 1, 2, 7, 8):
        assert torch.equal(outs[1][i], outs[3][i]), i


def test_evaluator_sequential_path_and_loss(models, loader, tmp_path):
    m, _ = models("gray_mol")
    ev = _evaluator(m, tmp_path, resample=2, iw_samples=2)
    out = ev.get_eval_values("srnn.pt", loader=loader)
    assert len(out) == 10 and tuple(out[0].shape) == (8, 3) and tuple(out[4].shape) == (2,)
    mean, std = ev.get_loss("srnn.pt", loss_resamples=1, loader=loader)
    assert bool(torch.isfinite(mean)) and std == -1
    # bits/dim = loss / (ln 2 * prod(dims) * t) of the bound on the trained frames
    with torch.no_grad():
        torch.manual_seed(3)
        mean, _ = ev.get_loss("srnn.pt", loader=loader[:1])
        torch.manual_seed(3)
        image = ev.solver.preprocess(loader[0].to(DEV))[:, :4]
        want = float(m.elbo_importance_weighting(image, 2)) / (0.6931471805599453 * 32 * 32 * 3)
    assert float(mean) == pytest.approx(want, rel=1e-6)
    with pytest.raises(ValueError, match="srnn.pt"):
        ev.plot_long_t("srnn.pt")


def test_driver_writes_evaluations_for_srnn(tmp_path, capsys):
    """a checkpoint written by one SRNN Solver step on synthetic data; eval_settings.main writes evaluations.pt and
    eval_avg_losses.txt with the reference's keys, skips the RFN-only sheets with one line"""
    import main_srnn
    from SRNN.trainer import Solver
    from evaluation_metrics import eval_settings as E
    exp = tmp_path / "run"
    exp.mkdir()
    rel = "/" + os.path.relpath(str(exp), os.getcwd()) + "/"
    args = main_srnn.build_parser().parse_args(
        ("--synthetic_data --max_steps 1 --n_epochs 1 --batch_size 2 --n_frames 3 --image_size 32 --digit_size 12 "
         "--x_dim 2 1 32 32 --condition_dim 2 1 32 32 --h_dim 8 --a_dim 8 --z_dim 4 --n_logistics 3 --num_workers 0 "
         "--path " + rel).split())
    torch.manual_seed(3)
    s = Solver(args)
    s.build()
    s.train()
    assert os.path.isfile(str(exp / "model_folder" / "srnn.pt"))
    del s
    settings = E.parse_args(("--folder_path %s/ --experiment_names run --model_path srnn.pt --temperatures 1.0 "
                             "--max_batches 1 --draws_per_pass 2 --n_frames 5 --start_predictions 2 --resample 2 --seed 4 "
                             "--eval_loss --no-debug_plot" % tmp_path).split())
    settings.iw_samples = 2
    capsys.readouterr()
    E.main(settings)
    printed = capsys.readouterr().out
    assert printed.count("RFN-only") == 1 and "plot_long_t" in printed
    folder = str(exp) + "/eval_folder/"
    saved = torch.load(folder + "evaluations.pt", weights_only=True)
    assert tuple(saved) == E.FULL_KEYS
    assert tuple(saved["SSIM_values"].shape) == (2, 3) and tuple(saved["BPD"].shape) == (1,)
    assert saved["LPIPS_values"] is None and (saved["FVD_mean"], saved["FVD_std"]) == (-1, -1)
    assert bool(torch.isfinite(saved["bits_mean"])) and bool(torch.isfinite(saved["bits_std"]))
    lines = open(folder + "eval_avg_losses.txt").read().splitlines()
    assert [l.split(":")[0] for l in lines if not l.startswith(" ")] == [
        "SSIM", "PSNR", "MSE", "LPIPS", "BPD", "DKL", "RECON", "SSIM_std_mean", "PSNR_std_mean", "LPIPS_std_mean",
        "FVD_mean", "FVD_std", "bits_mean", "bits_std"]
    assert not [f for f in os.listdir(folder) if f.endswith(".png")]
