"""tools/eval_baselines.py on the GPU: one-step synthetic runs of main_vrnn.py (gray, bernoulli,
32x32) and main_svg.py (gray, mse, 64x64) are evaluated through the Evaluator's non-RFN branches; evaluations.pt has
eval_settings.FULL_KEYS with the shapes of the RFN path, the same --seed gives the same tensors, --draws_per_pass 1 and 2
agree as tests/test_srnn_eval.py holds SRNN to (the same uint8 frames, then equal metrics), and --plot_with draws the
all-models curve figures."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("SSIM_values", "PSNR_values", "MSE_values", "SSIM_std_mean", "PSNR_std_mean")


def _tool():
    spec = importlib.util.spec_from_file_location("eval_baselines", os.path.join(ROOT, "tools", "eval_baselines.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module", autouse=True)
def grey_frames_under_a_bernoulli():
    """The synthetic frames are grey.  VRNN.loss with --loss_type bernoulli is td.Bernoulli(probs=).log_prob(x), and
    torch.distributions refuses an x off {0, 1} while its argument validation is on, although the formula
    x log p + (1 - x) log(1 - p) it computes is defined there (ops.pixel_loglik takes any x).  The one-step run and
    Evaluator's model.loss(image) go through that chain, so validation is off while this module runs."""
    import torch.distributions as td
    td.Distribution.set_default_validate_args(False)
    yield
    td.Distribution.set_default_validate_args(True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """folder with the two experiments `vrnn` and `svg`, each one optimizer step on synthetic data.  Three sequences per
    batch: the tool generates under deterministic convolution algorithms, and at the row counts of tests/test_vrnn.py
    and tests/test_svg.py (B = 4 with the same layer sizes) the algorithm chosen here would be reused by their gradient
    comparisons later in the same process, which are sensitive to it (tests/test_vrnn.py's docstring)."""
    import main_svg
    import main_vrnn
    from SVG.trainer import Solver as SVGSolver
    from VRNN.trainer import Solver as VRNNSolver
    folder = tmp_path_factory.mktemp("baselines")
    common = "--synthetic_data --max_steps 1 --n_epochs 1 --batch_size 3 --n_frames 3 --digit_size 12 --num_workers 0 "
    for name, main, Solver, flags in (
            ("vrnn", main_vrnn, VRNNSolver, "--image_size 32 --x_dim 3 1 32 32 --condition_dim 3 1 32 32 --h_dim 8 --z_dim 4 "
                                            "--loss_type bernoulli"),
            ("svg", main_svg, SVGSolver, "--image_size 64 --x_dim 3 1 64 64 --condition_dim 3 1 64 64 --c_features 8 "
                                         "--h_dim 16 --z_dim 4 --loss_type mse")):
        exp = folder / name
        exp.mkdir()
        rel = "/" + os.path.relpath(str(exp), os.getcwd()) + "/"
        torch.manual_seed(3)
        s = Solver(main.build_parser().parse_args((common + flags + " --path " + rel).split()))
        s.build()
        s.train()
        assert os.path.isfile(str(exp / "model_folder" / (name + ".pt")))
        del s
    return folder


def _argv(folder, extra):
    return ("--folder_path %s/ --experiment_names vrnn svg --model_path vrnn.pt svg.pt --n_frames 3 --start_predictions 2 "
            "--max_batches 1 --resample 2 --seed 4 --iw_samples 2 --eval_loss %s" % (folder, extra)).split()


def _saved(folder):
    return {e: torch.load(str(folder / e / "eval_folder" / "evaluations.pt"), weights_only=True) for e in ("vrnn", "svg")}


def test_tool_writes_evaluations_for_vrnn_and_svg(runs, capsys, monkeypatch):
    from evaluation_metrics import eval_settings as E
    from SVG.SVG import SVG
    from VRNN.VRNN import VRNN
    T = _tool()
    # the uint8 frames every pass generated, per model: the precondition of the draws_per_pass comparison
    seen = {}
    for cls, key in ((VRNN, "vrnn"), (SVG, "svg")):
        plain = cls._predict_draws_device

        def spy(self, *a, _plain=plain, _key=key, **k):
            tx, pr = _plain(self, *a, **k)
            seen.setdefault(_key, []).append(pr)
            return tx, pr
        monkeypatch.setattr(cls, "_predict_draws_device", spy)
    capsys.readouterr()
    assert T.main(T.parse_args(_argv(runs, "--draws_per_pass 2"))) == []
    printed = capsys.readouterr().out
    assert printed.count("RFN-only") == 2 and "plot_long_t" in printed
    first = _saved(runs)
    frames2 = {k: torch.cat(v, 1) for k, v in seen.items()}               # [n_pred, draws, B, C, H, W]
    for e, side in (("vrnn", 32), ("svg", 64)):
        d = first[e]
        assert tuple(d) == E.FULL_KEYS
        for k in METRICS:                                                 # [n_seq, n_pred]
            assert tuple(d[k].shape) == (3, 1) and d[k].dtype == torch.float32, (e, k)
        for k in ("BPD", "DKL", "RECON"):                                 # one value per batch
            assert tuple(d[k].shape) == (1,) and bool(torch.isfinite(d[k]).all()), (e, k)
        assert d["temperature"] is None and d["LPIPS_values"] is None and d["LPIPS_std_mean"] is None
        assert (d["FVD_mean"], d["FVD_std"]) == (-1, -1)
        assert bool(torch.isfinite(d["bits_mean"])) and bool(torch.isfinite(d["bits_std"]))
        assert tuple(frames2[e].shape) == (1, 2, 3, 1, side, side)
        folder = str(runs / e / "eval_folder") + "/"
        lines = open(folder + "eval_avg_losses.txt").read().splitlines()
        assert [l.split(":")[0] for l in lines if not l.startswith(" ")] == [
            "SSIM", "PSNR", "MSE", "LPIPS", "BPD", "DKL", "RECON", "SSIM_std_mean", "PSNR_std_mean", "LPIPS_std_mean",
            "FVD_mean", "FVD_std", "bits_mean", "bits_std"]
        assert not [f for f in os.listdir(folder) if f.endswith(".png")]
    # the same --seed: the same tensors, the stochastic loss figures included
    seen.clear()
    T.main(T.parse_args(_argv(runs, "--draws_per_pass 2")))
    again = _saved(runs)
    for e in ("vrnn", "svg"):
        for k in METRICS + ("BPD", "DKL", "RECON", "bits_mean", "bits_std"):
            assert torch.equal(torch.as_tensor(first[e][k]), torch.as_tensor(again[e][k])), (e, k)
    # draws_per_pass 1: the same uint8 frames (the precondition), then the same metrics
    seen.clear()
    T.main(T.parse_args(_argv(runs, "--draws_per_pass 1")))
    one = _saved(runs)
    from SVG.trainer import Solver as SVGSolver
    from VRNN.trainer import Solver as VRNNSolver
    for e, Solver in (("vrnn", VRNNSolver), ("svg", SVGSolver)):
        frames1 = torch.cat(seen[e], 1)
        ckpt = Solver.read_checkpoint(str(runs / e / "model_folder" / (e + ".pt")))
        solver = Solver(Solver.args_for_world(ckpt, 1))
        u8 = [solver.preprocess(f, reverse=True) for f in (frames1, frames2[e])]
        differing = int((u8[0] != u8[1]).sum())
        print("%s: uint8 predictions differing between draws_per_pass 1 and 2: %d of %d" % (e, differing, u8[0].numel()))
        assert differing == 0, "the uint8 predictions of the two runs differ in %d of %d values" % (differing, u8[0].numel())
        for k in METRICS:
            assert torch.equal(one[e][k], first[e][k]), (e, k)


def test_tool_draws_all_models_in_one_panel(runs, capsys):
    """the sequential path (no --draws_per_pass) for the values, then --plot_with over the two runs and a third
    experiment whose evaluations.pt is a stand-in with the right keys"""
    from evaluation_metrics import eval_settings as E
    T = _tool()
    other = runs / "other" / "eval_folder"
    os.makedirs(str(other))
    g = torch.Generator().manual_seed(1)
    fake = {k: None for k in E.FULL_KEYS}
    for k in METRICS:
        fake[k] = torch.rand(5, 1, generator=g)
    fake.update(temperature=0.7, BPD=torch.rand(1), DKL=torch.rand(1), RECON=torch.rand(1), FVD_mean=-1, FVD_std=-1,
                bits_mean=-1, bits_std=-1)
    argv = _argv(runs, "--plot_with other --label_names RFN VRNN SVG")
    torch.save(fake, str(other / "evaluations.pt"))
    paths = T.main(T.parse_args(argv))
    folder = str(runs / "svg" / "eval_folder")                           # the last experiment's, as the reference does
    assert paths == [os.path.join(folder, n + ".png") for n in ("eval_plots_max", "eval_plots_max_median",
                                                               "eval_plots_mean_mean")]
    for p in paths:
        blob = open(p, "rb").read()
        assert blob[:8] == b"\x89PNG\r\n\x1a\n" and len(blob) > 1000
    saved = _saved(runs)
    for e in ("vrnn", "svg"):
        assert tuple(saved[e]) == E.FULL_KEYS and tuple(saved[e]["SSIM_values"].shape) == (3, 1)
