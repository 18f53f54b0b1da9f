"""Host side of the linear-extrapolation baseline (no device): the feature order of rfn_hip.ops.linear_extrap_pairs
against the torch expression SimpleLinearModel.get_lagged_differences, the refusals of the *_check functions, the
parser's defaults against the constants of the reference's script, the header's entry points and their binding, and an
evaluations.pt of the driver's layout through evaluation_metrics.curves.build_figures."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 2, 5, 10])
def test_pairs_reproduce_the_torch_feature_order(n):
    from AverageModel import SimpleLinearModel
    from rfn_hip import ops
    g = torch.Generator().manual_seed(n)
    x = torch.rand(2, n, 1, 3, 4, generator=g, dtype=torch.float64)
    model = SimpleLinearModel(num_cond_frames=n)
    feats = torch.cat((x, model.get_lagged_differences(x)), dim=1)
    pairs = ops.linear_extrap_pairs(n)
    F = n * (n + 1) // 2
    assert len(pairs) == F == feats.shape[1] == model.W.shape[1]
    assert tuple(model.W.shape) == (1, F) and tuple(model.bias.shape) == (1, 1)
    assert not model.W.any() and not model.bias.any()
    for f, (i, j) in enumerate(pairs):
        want = x[:, i] if j is None else x[:, i] - x[:, j]
        assert torch.equal(feats[:, f], want), (n, f, i, j)
    assert list(model.state_dict()) == ["W", "bias"]


def test_pairs_refuse_an_empty_window():
    from rfn_hip import ops
    with pytest.raises(ValueError, match="n must be >= 1"):
        ops.linear_extrap_pairs(0)


def _lx(n=2, T=4, shape=(1, 5, 7), B=3):
    F = n * (n + 1) // 2
    return [torch.zeros((B, T) + shape), torch.zeros(1, F), torch.zeros(1, 1), n]


def test_linear_extrap_check_names_what_does_not_fit():
    from rfn_hip import ops
    assert ops.linear_extrap_check(*_lx(), start=1) == (3, 4, 35, 3)
    assert ops.linear_extrap_check(*_lx(), start=2, P=7) == (3, 4, 35, 3)
    assert ops.linext_limits() == (10, 11, 128)

    def bad(match, args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.linear_extrap_check(*args, **kw)

    for P in (None, 2):
        kw = {} if P is None else {"P": P}
        a = _lx()
        bad("n must be in 1..10, got 0", a[:3] + [0], **kw)
        bad("n must be in 1..10, got 11", a[:3] + [11], **kw)
        bad("n must be an int", a[:3] + [2.0], **kw)
        bad("start must be >= 0", a, start=-1, **kw)
        bad(r"W has 4 elements .* F = n \(n \+ 1\) / 2 = 3", [a[0], torch.zeros(1, 4), a[2], 2], **kw)
        bad("bias has 2 elements", [a[0], a[1], torch.zeros(2), 2], **kw)
        bad("x must be float32, got torch.float64", [a[0].double(), a[1], a[2], 2], **kw)
        bad("W must be float32, got torch.float16", [a[0], a[1].half(), a[2], 2], **kw)
        bad("bias must be float32", [a[0], a[1], a[2].double(), 2], **kw)
        bad("x must be a tensor", [None, a[1], a[2], 2], **kw)
        bad(r"x must be \[B, T, C, H, W\]", [a[0][0], a[1], a[2], 2], **kw)
    # the loss needs the window and its target, the rollout the window alone
    bad("T = 4 frames, start = 2 and n = 2 need T >= 5", _lx(), start=2)
    ops.linear_extrap_check(*_lx(), start=2, P=1)
    bad("T = 4 frames, start = 3 and n = 2 need T >= 5", _lx(), start=3, P=1)
    bad("P must be >= 1, got 0", _lx(), P=0)
    bad("P must be an int", _lx(), P=1.5)
    # the ops refuse the same inputs before anything is launched, and have no CPU path behind them
    with pytest.raises(ValueError, match="n must be in 1..10"):
        ops.linear_extrap_loss(*_lx()[:3], 11)
    with pytest.raises(ValueError, match="P must be >= 1"):
        ops.linear_extrap_rollout(*_lx(), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_extrap_rollout(*_lx(), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_extrap_loss(*_lx())


def test_gauss_quality_check_names_what_does_not_fit():
    from rfn_hip import ops
    ok = torch.zeros(2, 3, 11, 128)
    assert ops.gauss_quality_check(ok, ok) == (2, 3, 11, 128)

    def bad(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.gauss_quality_check(*args, **kw)

    for side in (10, 129):
        t = torch.zeros(1, 1, side, 16)
        bad("H = %d" % side, t, t)
        t = torch.zeros(1, 1, 16, side)
        bad("W = %d" % side, t, t)
    bad(r"shapes differ: pred \(2, 3, 11, 128\), true \(2, 3, 12, 128\)", ok, torch.zeros(2, 3, 12, 128))
    bad("pred must be float32, got torch.uint8", ok.byte(), ok)
    bad("true must be float32, got torch.float64", ok, ok.double())
    bad(r"pred must be \[N, C, H, W\]", ok[0], ok[0])
    bad("true must be a tensor", ok, None)
    bad("lo <= hi", ok, ok, lo=2.0, hi=1.0)
    with pytest.raises(ValueError, match="H = 10"):
        ops.gauss_quality(torch.zeros(1, 1, 10, 16), torch.zeros(1, 1, 10, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gauss_quality(ok, ok)


def test_parser_defaults_are_the_reference_scripts_constants():
    import main_average
    import main_svg
    a = main_average.build_parser().parse_args([])
    # averagemodel.py: seq_len_train - 1 = 5, seq_len_test = 20, num_predictions = 10, batch 128 * 2, range(3), lr 0.001,
    # trainset_str = 'bair', num_workers = 10, MovingMNIST(image_size=64, digit_size=28, num_digits=2, step_length=4)
    assert (a.n_conditions, a.n_frames, a.n_predictions, a.batch_size, a.n_epochs, a.learning_rate) == (5, 20, 10, 256, 3, 1e-3)
    assert (a.choose_data, a.num_workers, a.image_size, a.digit_size, a.num_digits, a.step_length) == ("bair", 10, 64, 28, 2, 4)
    assert a.load_model is False and a.max_batches is None and a.lpips_weights is None and a.max_steps == 0
    # the data additions of main_svg.py, with its defaults
    s = main_svg.build_parser().parse_args([])
    for k in ("synthetic_data", "max_steps", "mnist_root", "data_seed", "data_root", "data_cache", "use_validation_set"):
        assert getattr(a, k) == getattr(s, k), k
    assert main_average.reference_file_name("bair", 5) == "SSIM_PSNR_bair_averagemodel_trained_on_6_frames.pt"


def test_model_refuses_a_window_the_kernels_do_not_hold():
    from AverageModel import SimpleLinearModel
    for n in (0, 11):
        with pytest.raises(ValueError, match="num_cond_frames must be in 1..10"):
            SimpleLinearModel(num_cond_frames=n)


def test_header_declares_the_entry_points_and_the_binding_derives_them():
    from rfn_hip import lib
    with open(os.path.join(ROOT, "include", "rfn_hip.h")) as f:
        text = f.read()
    sigs, res, consts = lib.parse_header(text)
    P, I, Lg, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert sigs["rfn_linext_train_f32"] == [P, Lg, Lg, I, P, P, P, Lg, P, I, I, I, Lg, P]
    assert sigs["rfn_linext_rollout_f32"] == [P, Lg, Lg, I, P, P, P, I, I, I, I, Lg, P]
    assert sigs["rfn_gauss_quality_f32"] == [P, P, P, P, I, I, I, I, Fl, Fl, Fl, P]
    queries = ("rfn_linext_max_frames", "rfn_linext_max_blocks", "rfn_gauss_quality_min_side", "rfn_gauss_quality_max_side")
    for name in ("rfn_linext_train_f32", "rfn_linext_rollout_f32", "rfn_gauss_quality_f32") + queries:
        assert res[name] is I
    assert all(sigs[q] == [] for q in queries)
    assert "#define RFN_LINEXT_MAX_FRAMES (10)" in text
    assert lib.ABI_VERSION == 2
    with open(os.path.join(ROOT, "recurrent-flows-msc_amd", "csrc", "Makefile")) as f:
        assert "linear_extrap.hip" in f.read()
    if os.path.exists(lib.HEADER_PATH):      # a built tree: the copy the loader reads says the same
        for name in ("rfn_linext_train_f32", "rfn_linext_rollout_f32", "rfn_gauss_quality_f32"):
            assert lib.SIGNATURES[name] == sigs[name]
    if os.path.exists(lib.LIB_PATH):
        assert lib.load().rfn_abi_version() == 2
        assert lib.load().rfn_linext_max_blocks() >= 1 and lib.load().rfn_linext_max_frames() == 10


def test_an_evaluations_file_of_the_drivers_layout_passes_through_build_figures(tmp_path):
    from evaluation_metrics.curves import FIGURE_NAMES, build_figures
    from evaluation_metrics.eval_settings import eval_dict
    g = torch.Generator().manual_seed(3)
    N, P = 8, 3
    ssim, psnr, mse = torch.rand(N, P, generator=g), 10 + 20 * torch.rand(N, P, generator=g), torch.rand(N, P, generator=g)
    d = {"SSIM_values": ssim, "PSNR_values": psnr, "MSE_values": mse, "LPIPS_values": None, "temperature": None,
         "BPD": None, "DKL": None, "RECON": None, "SSIM_std_mean": ssim, "PSNR_std_mean": psnr, "LPIPS_std_mean": None}
    assert set(d) == set(eval_dict((None,) * 10, None))       # the Evaluator's eleven keys
    path = str(tmp_path / "evaluations.pt")
    torch.save(d, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    figures = build_figures([("RFN", back), ("linear", back)], 2, 3)
    assert list(figures) == list(FIGURE_NAMES)
    for fig in figures.values():
        assert [len(p.series) for p in fig.panels[:2]] == [2, 2]
        assert fig.panels[0].series[1].label == "linear"
        assert len(fig.panels[0].series[1].y) == P
