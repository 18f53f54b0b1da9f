"""GPU tests of the temperature sweep: RFN.predict_draws with per-row temperatures (blocks against scalar runs, the
one-temperature identity, the graph that takes the temperatures as inputs, independence of a block from the other
temperatures of the sweep), Evaluator.get_eval_values_temperatures against the float64 restatement of
tests/test_predict_draws.py, the four RFN sheets, and the evaluation driver end to end on a tiny synthetic-data run.
The tiny model, its solver and the helpers are those of tests/test_predict_draws.py."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.test_moving_mnist_host import _solver_argv
from tests.test_predict_draws import (B_, R_, START, T_, _close64, _expected, _graph_mode, close, solver,  # noqa: F401
                                      tiny)
from tests.test_sheet_host import decode_png

pytestmark = pytest.mark.gpu

TEMPS = [0.5, 1.0]


def _builds(m):
    return getattr(m, "_gen_graph_builds", 0)


# ------------------------------------------------------------------------------------------------ RFN.predict_draws
@pytest.fixture(scope="module")
def live(tiny):
    """The tiny model by the recipe of tests/test_predict_draws.py (`tiny`), with every parameter that is still all
    zero after the data dependent init -- the Conv2dZeros layers at the end of the coupling nets, of Split2d and of the
    learned base distribution -- set to 0.1 * N(0, 1).  In a model fresh from its init those zeros cut the flow off
    from its conditions, so the latent z, and with it the kl temperature, has no effect on a frame at all: blocks at kl
    temperatures 0.5 and 1.0 came out bit-identical on the untouched `tiny` model (measured; the flow's own temperature
    is not affected and differed there).  A trained model has no such zeros; this stands in for one."""
    import __graft_entry__ as ge
    from RFN import RFN
    _, x = tiny
    torch.manual_seed(5)
    m = RFN(ge._tiny_args()).cuda().train()
    m.loss(x, 0)
    m.eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in m.parameters():
            if not bool(p.any()):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return m, x


@pytest.mark.parametrize("which", ["temperatures", "kl_temperatures"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_blocks_equal_scalar_runs(live, monkeypatch, graph, which):
    _graph_mode(monkeypatch, graph)
    m, x = live
    B = x.shape[0]
    attr = "temperature" if which == "temperatures" else "kl_temperature"
    before = (m.temperature, m.kl_temperature)
    true_x, sweep = m.predict_draws(x, 3, 2, n_draws=2, seed=9, **{which: TEMPS})
    assert (m.temperature, m.kl_temperature) == before
    assert sweep.device.type == "cpu" and tuple(sweep.shape) == (3, 2, 2, B) + tuple(x.shape[2:])
    assert tuple(true_x.shape) == (2, B) + tuple(x.shape[2:])
    dev = m._predict_draws_device(x, 3, 2, 2, 9, **{which: TEMPS})[1]
    assert dev.is_cuda and torch.equal(dev.cpu(), sweep)
    for k, T in enumerate(TEMPS):
        setattr(m, attr, T)
        try:
            _, ref = m.predict_draws(x, 3, 2, n_draws=2, seed=9)
        finally:
            m.temperature, m.kl_temperature = before
        close(sweep[:, k], ref)
    assert float((sweep[:, 0] - sweep[:, 1]).abs().max()) > 1e-3
    # both lists at once: the same length, each row its own pair
    _, both = m.predict_draws(x, 3, 2, n_draws=2, seed=9, temperatures=[before[0], 0.5], kl_temperatures=[before[1], 0.5])
    _, plain = m.predict_draws(x, 3, 2, n_draws=2, seed=9)
    close(both[:, 0], plain)
    with pytest.raises(ValueError, match="kl_temperatures"):
        m.predict_draws(x, 3, 2, n_draws=2, seed=9, temperatures=[0.5, 1.0], kl_temperatures=[1.0])
    assert (m.temperature, m.kl_temperature) == before


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_one_temperature_is_the_plain_call(live, monkeypatch, graph):
    """K = 1 at the model's own temperature: the same batch, the same kernels, the same noise -- the same bits"""
    _graph_mode(monkeypatch, graph)
    m, x = live
    _, plain = m.predict_draws(x, 3, 2, n_draws=2, seed=9)
    _, one = m.predict_draws(x, 3, 2, n_draws=2, seed=9, temperatures=[m.temperature])
    assert tuple(one.shape) == (3, 1, 2) + tuple(plain.shape[2:])
    assert torch.equal(one.reshape(plain.shape), plain)
    _, one_kl = m.predict_draws(x, 3, 2, n_draws=2, seed=9, kl_temperatures=[m.kl_temperature])
    assert torch.equal(one_kl.reshape(plain.shape), plain)


def test_temperatures_are_inputs_of_the_graph(live, monkeypatch):
    monkeypatch.setenv("RFN_GEN_GRAPH", "1")
    m, x = live
    before = _builds(m)
    _, a = m.predict_draws(x, 2, 2, n_draws=2, seed=4, temperatures=[0.5, 1.0])
    _, b = m.predict_draws(x, 2, 2, n_draws=2, seed=4, temperatures=[0.3, 2.0])
    assert _builds(m) - before <= 1
    m.predict_draws(x, 2, 2, n_draws=2, seed=4)
    assert _builds(m) - before <= 2
    _, c = m.predict_draws(x, 2, 2, n_draws=2, seed=4, temperatures=[0.5, 1.0])
    assert _builds(m) - before <= 2
    # the replays took the values they were given
    assert torch.equal(a, c) and float((a - b).abs().max()) > 1e-3


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_block_does_not_depend_on_the_sweep(live, monkeypatch, graph):
    _graph_mode(monkeypatch, graph)
    m, x = live
    _, two = m.predict_draws(x, 3, 2, n_draws=2, seed=9, temperatures=[0.5, 1.0])
    _, three = m.predict_draws(x, 3, 2, n_draws=2, seed=9, temperatures=[0.3, 0.5, 2.0])
    close(two[:, 0], three[:, 1])


# ------------------------------------------------------------------------------------------------ the Evaluator
def _run_sweep(s, args, batches, temps, **extra):
    """get_eval_values_temperatures with draws_per_pass = 4 (P = 2 at two temperatures) and the spies of
    tests/test_predict_draws.py: the draws of the padded last pass beyond `resample` are replaced by the ground truth
    (a perfect score) in every temperature's block before the Evaluator sees them -- they must not count"""
    from evaluation_metrics import Evaluator
    settings = Namespace(n_frames=T_, start_predictions=START, resample=R_, n_trained=args.n_frames, draws_per_pass=4,
                         seed=21, **extra)
    ev = Evaluator(s, settings=settings)
    seen, losses = [], []
    plain_draws, plain_loss = s.model._predict_draws_device, s.model.loss

    def draws_spy(image, n_pred, n_cond, P, seed, first_seq=0, first_draw=0, temperatures=None, kl_temperatures=None):
        tx, pr = plain_draws(image, n_pred, n_cond, P, seed, first_seq=first_seq, first_draw=first_draw,
                             temperatures=temperatures, kl_temperatures=kl_temperatures)
        assert kl_temperatures is None and list(temperatures) == list(temps)
        assert pr.is_cuda and tuple(pr.shape) == (n_pred, len(temps), P, image.shape[0]) + tuple(image.shape[2:])
        pr = pr.clone()
        for d in range(P):
            if first_draw + d >= R_:
                pr[:, :, d] = image[:, n_cond:n_cond + n_pred].transpose(0, 1).unsqueeze(1)
        seen.append((P, seed, first_seq, first_draw, pr.clone()))
        return tx, pr

    def loss_spy(*a, **k):
        out = plain_loss(*a, **k)
        losses.append((out[1].detach().clone(), out[2].detach().clone(), tuple(a[0].shape)))
        return out

    s.model._predict_draws_device, s.model.loss = draws_spy, loss_spy
    try:
        out = ev.get_eval_values_temperatures(temps, "rfn.pt", loader=batches, max_batches=2)
    finally:
        del s.model._predict_draws_device, s.model.loss
    return ev, out, seen, losses


def test_evaluator_sweep_against_the_restatement(solver):
    """per temperature, the tuple is what the float64 restatement of tests/test_predict_draws.py (_expected: best-of-N
    in ascending draw id, strict comparisons, the draw-0 aliasing, its near-tie assertion at 1e-4) gives for that
    temperature's block of the predictions the model returned"""
    s, args, batches = solver
    before = (s.model.temperature, s.model.kl_temperature)
    ev, out, seen, losses = _run_sweep(s, args, batches, TEMPS)
    assert (s.model.temperature, s.model.kl_temperature) == before
    assert list(out) == TEMPS
    assert len(seen) == 2 * 2          # two batches, ceil(3 / 2) passes each, all temperatures in every pass
    assert len(losses) == 2            # model.loss once per batch
    assert all(e[0] == 2 for e in seen)   # P = max(1, 4 // 2)
    n_pred = T_ - START
    assert isinstance(ev.best_preds_ssim, dict) and list(ev.best_preds_ssim) == TEMPS
    want = []
    for kl, nll, shp in losses:
        assert shp == (B_, args.n_frames, 1, 16, 16)
        want.append(ev.compute_loss(nll=nll, kl=kl, dims=shp[2:], t=shp[1] - 1))
    for k, T in enumerate(TEMPS):
        mse_v, psnr_v, ssim_v, lpips_v, bpd, dkl, recon, ssim_std, psnr_std, lpips_std = out[T]
        assert lpips_v is None and lpips_std is None
        for t in (mse_v, psnr_v, ssim_v, ssim_std, psnr_std):
            assert tuple(t.shape) == (2 * B_, n_pred) and t.dtype == torch.float32 and t.device.type == "cpu"
        block = [(P, seed, fs, fd, pr[:, k]) for P, seed, fs, fd, pr in seen]
        exp, _ = _expected(s, batches, block)
        _close64(mse_v, exp["mse"])
        _close64(psnr_v, exp["psnr"])
        _close64(ssim_v, exp["ssim"], rtol=0.0, atol=1e-6)
        _close64(psnr_std, exp["psnr_std"])
        _close64(ssim_std, exp["ssim_std"], rtol=0.0, atol=1e-6)
        # the padded draw (ground truth, a perfect score) did not count
        assert bool(torch.isfinite(psnr_v).all()) and float(ssim_v.max()) < 1.0
        # BPD / DKL / RECON: one evaluation per batch, shared by the temperatures
        for j, got in enumerate((bpd, dkl, recon)):
            assert torch.equal(got, torch.FloatTensor([w[j] for w in want]))
            assert got is out[TEMPS[0]][4 + j]
        bp = ev.best_preds_ssim[T]
        assert bp.is_cuda and bp.dtype == torch.uint8 and tuple(bp.shape) == (2 * B_, n_pred, 1, 16, 16)
        for i in range(2 * B_):
            bi, b = divmod(i, B_)
            r = int(exp["best_draw"][i])
            pr = [e for e in block if e[2] == bi * B_][r // 2][4][:, r % 2, b]
            assert torch.equal(bp[i], s.preprocess(pr, reverse=True))
    assert float((out[TEMPS[0]][2] - out[TEMPS[1]][2]).abs().max()) > 0   # the temperatures score differently


# ------------------------------------------------------------------------------------------------ the four sheets
def _cell(px, r, i, S=16, gutter=2):
    y0, x0 = gutter + r * (S + gutter), gutter + i * (S + gutter)
    return np.asarray(px)[y0:y0 + S, x0:x0 + S]


def _grey(s, frame):
    """a model-space frame [1, S, S] as the sheet shows it: the solver's bytes in R, G and B"""
    return s.preprocess(frame, reverse=True)[0].cpu().numpy()[:, :, None].repeat(3, 2)


def test_the_four_sheets(solver):
    from evaluation_metrics import Evaluator
    from rfn_hip import ops
    s, args, batches = solver
    ev = Evaluator(s, settings=Namespace(n_frames=T_, start_predictions=START, seed=21))
    ev.test_loader = batches
    folder = s.path + "eval_folder/"
    calls = []
    plain = s.model._predict_draws_device

    def spy(image, *a, **k):
        out = plain(image, *a, **k)
        calls.append((a, k, out[0].clone(), out[1].clone()))
        return out

    def read(path, n_rows, n_cols):
        assert os.path.isfile(path)
        (w, h), px = decode_png(open(path, "rb").read())
        assert (h, w) == ops.sheet_shape(n_rows, n_cols, 16, 16, 2), path
        return px

    torch.manual_seed(99)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    attrs = (s.model.temperature, s.model.kl_temperature, s.model.training)
    s.model._predict_draws_device = spy
    try:
        # plot_long_t / plot_random_samples: one row per sequence, columns t_list of cat(conditions, predictions)
        for method, name in ((ev.plot_long_t, "plot_long_t"), (ev.plot_random_samples, "plot_rollouts")):
            del calls[:]
            path = method("rfn.pt", n_predictions=3, n_conditions=2, t_list=(1, 3), n_sequences=2)
            assert path == folder + name + ".png" and len(calls) == 1
            a, k, tx, pr = calls[0]
            assert a[:4] == (3, 2, 1, 21) and not k
            t_seq = torch.cat((tx, pr[:, 0]), 0)
            px = read(path, 2, 2)
            for row in range(2):
                for i, t in enumerate((1, 3)):
                    assert np.array_equal(_cell(px, row, i), _grey(s, t_seq[t, row])), (name, row, i)
        # plot_diversity: one call for all draws; sheet 1 shows sequence 1, sheet 2 sequence 0
        del calls[:]
        paths = ev.plot_diversity("rfn.pt", n_resamples=2, n_predictions=3, n_conditions=2, t_list=(0, 2))
        assert paths == (folder + "plot_diversity_1.png", folder + "plot_diversity_2.png") and len(calls) == 1
        a, k, tx, pr = calls[0]
        assert a[:4] == (3, 2, 2, 21) and not k
        for path, seq in zip(paths, (1, 0)):
            px = read(path, 2, 2)
            for r in range(2):
                for i, t in enumerate((0, 2)):
                    assert np.array_equal(_cell(px, r, i), _grey(s, pr[t, r, seq])), (path, r, i)
        # plot_temp: one row per temperature, one call per sheet with per-row temperatures
        names = {(False, False): "plot_temp_samples", (True, False): "plot_temp_samples_kl",
                 (False, True): "plot_temp_samples_dup", (True, True): "plot_temp_dup_kl"}
        for (kl, dup), name in names.items():
            del calls[:]
            path = ev.plot_temp("rfn.pt", orig_temps=[0.7, 1], kl_analysis=kl, duplicate_samples=dup, t_list=(0, 1),
                                temperatures=(0.5, 1.0), n_conditions=2)
            assert path == folder + name + ".png" and len(calls) == 1
            a, k, tx, pr = calls[0]
            assert a[:4] == ((5, 2, 2, 21) if dup else (2, 2, 1, 21))
            swept, other = ("kl_temperatures", "temperatures") if kl else ("temperatures", "kl_temperatures")
            assert k[swept] == [0.5, 1.0] and k[other] == [1e-9, 1e-9]
            px = read(path, 2, 2)
            for row in range(2):
                for i, t in enumerate((0, 1)):
                    frame = pr[t, row, i if dup else 0, 0]
                    assert np.array_equal(_cell(px, row, i), _grey(s, frame)), (name, row, i)
    finally:
        del s.model._predict_draws_device
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    assert (s.model.temperature, s.model.kl_temperature, s.model.training) == attrs
    with pytest.raises(ValueError, match="rfn.pt"):
        ev.plot_long_t("vrnn.pt")


# ------------------------------------------------------------------------------------------------ the driver
def _same(a, b):
    return (a is None and b is None) or (torch.is_tensor(a) and torch.equal(a, b)) or (not torch.is_tensor(a) and a == b)


def test_driver_end_to_end(tmp_path):
    """a checkpoint of a tiny synthetic-data run; eval_settings.main plainly and with --test_temperature: every file, the
    keys of the saved dicts, and the saved values against direct Evaluator calls on the same settings (torch's generator
    is seeded alike in front of both: the synthetic loader shuffles with it and model.loss draws from it)"""
    import main_rfn
    from RFN.trainer import Solver
    from evaluation_metrics import eval_settings as E
    exp = tmp_path / "exp"
    exp.mkdir()
    rel = "/" + os.path.relpath(str(exp), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv("--synthetic_data --choose_data mnist --path %s" % rel))
    torch.manual_seed(0)
    s = Solver(args)
    s.build()
    s.model.train()
    s.train_step(next(iter(s.train_loader)).to(s.device))
    s.checkpoint("rfn.pt", 1, 0.0)
    del s
    base = ("--folder_path %s/ --experiment_names exp --temperatures 0.5 1.0 --max_batches 1 --draws_per_pass 4 "
            "--n_frames 6 --start_predictions 2 --resample 3 --seed 21" % tmp_path).split()
    folder = str(exp) + "/eval_folder/"

    # plainly: the sheets, evaluations.pt and eval_avg_losses.txt at temperatures[0]
    torch.manual_seed(11)
    E.main(E.parse_args(base))
    for name in ("plot_long_t", "plot_diversity_1", "plot_diversity_2", "plot_rollouts", "plot_temp_samples",
                 "plot_temp_samples_kl", "plot_temp_samples_dup", "plot_temp_dup_kl"):
        assert os.path.isfile(folder + name + ".png"), name
    saved = torch.load(folder + "evaluations.pt", weights_only=True)
    assert tuple(saved) == E.FULL_KEYS
    assert saved["temperature"] == 0.5 and saved["LPIPS_values"] is None and saved["LPIPS_std_mean"] is None
    assert (saved["FVD_mean"], saved["FVD_std"], saved["bits_mean"], saved["bits_std"]) == (-1, -1, -1, -1)
    assert tuple(saved["SSIM_values"].shape) == (2, 4) and tuple(saved["BPD"].shape) == (1,)
    lines = open(folder + "eval_avg_losses.txt").read().splitlines()
    assert [l.split(":")[0] for l in lines if not l.startswith(" ")] == [
        "SSIM", "PSNR", "MSE", "LPIPS", "BPD", "DKL", "RECON", "SSIM_std_mean", "PSNR_std_mean", "LPIPS_std_mean",
        "FVD_mean", "FVD_std", "bits_mean", "bits_std"]
    torch.manual_seed(11)
    ev, _, _, max_batches = E.build_evaluator(E.parse_args(base), 0)
    assert max_batches == 1 and ev.n_trained == 4 and ev.n_frames == 6
    ev.model.temperature, ev.model.kl_temperature = 0.5, 1
    direct = E.eval_dict(ev.get_eval_values("rfn.pt", max_batches=1), 0.5)
    for k in E.EVAL_KEYS:
        assert _same(saved[k], direct[k]), k

    # the temperature study: one file per temperature from one pass
    torch.manual_seed(12)
    E.main(E.parse_args(base + ["--test_temperature"]))
    torch.manual_seed(12)
    ev, _, _, _ = E.build_evaluator(E.parse_args(base), 0)
    swept = ev.get_eval_values_temperatures([0.5, 1.0], "rfn.pt", max_batches=1)
    for T, name in ((0.5, "t05evaluations.pt"), (1.0, "t10evaluations.pt")):
        saved = torch.load(folder + name, weights_only=True)
        assert tuple(saved) == E.EVAL_KEYS and saved["temperature"] == T
        direct = E.eval_dict(swept[T], T)
        for k in E.EVAL_KEYS:
            assert _same(saved[k], direct[k]), (T, k)
    assert not os.path.exists(folder + "t07evaluations.pt")
