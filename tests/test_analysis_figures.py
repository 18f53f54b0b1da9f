"""GPU tests of the analysis figures: rfn_moving_mnist_sync_render_f32 (through rfn_hip.ops.moving_mnist_sync_render)
bit for bit against the restatement of tests/sync_mnist_ref.py on frames, trajectories and hits; the
MovingMNIST_synchronized dataset and its loader; Evaluator.plot_elbo_gap / plot_prob_of_t pixel for pixel against the CPU
rasteriser (tests/chart_ref.py) and compose_sheet; get_eval_values with extra_plots; and Evaluator.param_plots on a small
RFN, with model.param_analysis also replaced by a stub whose sums are exact."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import chart_ref as R
from tests.sync_mnist_ref import sync_hit, sync_render
from tests.test_analysis_figures_host import SYNC_CASES, sync_case_key
from tests.test_moving_mnist_host import fixture_digits, write_mnist
from tests.test_sheet_host import decode_png

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def font():
    from rfn_hip import ops
    return ops.chart_font()


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("B,T,S,nd,L,det,C", SYNC_CASES)
def test_sync_kernel_matches_restatement(B, T, S, nd, L, det, C):
    from rfn_hip import ops
    digits = fixture_digits(64, B + T + S)
    table = torch.from_numpy(digits).cuda()
    seed, split, first = sync_case_key(B, T, S, nd, L, det, C)
    out, traj, hit = ops.moving_mnist_sync_render(table, B, T, C, S, nd, L, det, seed, split, first,
                                                  trajectories=True, hits=True)
    torch.cuda.synchronize()
    want_x, want_traj, want_hit = sync_render(digits, B, T, C, S, nd, L, det, seed, split, first)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, T, C, S, S) and out.is_contiguous()
    assert hit.dtype == torch.int32 and tuple(hit.shape) == (B, T) and traj.dtype == torch.int64
    assert torch.equal(traj.cpu(), torch.from_numpy(want_traj))
    assert torch.equal(hit.cpu(), torch.from_numpy(want_hit))
    assert torch.equal(out.cpu(), torch.from_numpy(want_x))
    if S in (29, 32) and T >= 9:
        assert bool((hit == 0).any()) and bool((hit != 0).any())
    # every sequence shares the positions; hit = None and traj = None leave the frames alone
    assert torch.equal(traj[:, :, :, 1:], traj[:1, :, :, 1:].expand(B, -1, -1, -1))
    assert torch.equal(ops.moving_mnist_sync_render(table, B, T, C, S, nd, L, det, seed, split, first), out)
    only_hit = ops.moving_mnist_sync_render(table, B, T, C, S, nd, L, det, seed, split, first, hits=True)
    only_traj = ops.moving_mnist_sync_render(table, B, T, C, S, nd, L, det, seed, split, first, trajectories=True)
    assert len(only_hit) == 2 and torch.equal(only_hit[0], out) and torch.equal(only_hit[1], hit)
    assert len(only_traj) == 2 and torch.equal(only_traj[0], out) and torch.equal(only_traj[1], traj)


def test_sync_kernel_large_first_id_and_plain_entry_untouched():
    from rfn_hip import ops
    from tests.test_moving_mnist_host import render
    digits = fixture_digits(64, 9)
    table = torch.from_numpy(digits).cuda()
    first = (1 << 40) + 5
    out, traj, hit = ops.moving_mnist_sync_render(table, 3, 12, 1, 32, 2, 4, False, 8, 1, first, trajectories=True,
                                                  hits=True)
    want_x, want_traj, want_hit = sync_render(digits, 3, 12, 1, 32, 2, 4, False, 8, 1, first)
    assert torch.equal(out.cpu(), torch.from_numpy(want_x)) and torch.equal(traj.cpu(), torch.from_numpy(want_traj))
    assert torch.equal(hit.cpu(), torch.from_numpy(want_hit))
    # a batch is its sequences: rows 1.. of a launch are the launch that starts one id later
    assert torch.equal(out[1:], ops.moving_mnist_sync_render(table, 2, 12, 1, 32, 2, 4, False, 8, 1, first + 1))
    # the plain renderer still draws its own walk from the same key
    plain = ops.moving_mnist_render(table, 3, 12, 1, 32, 2, 4, False, 8, 1, first)
    assert torch.equal(plain.cpu(), torch.from_numpy(render(digits, 3, 12, 1, 32, 2, 4, False, 8, 1, first)[0]))
    assert not torch.equal(plain, out)


# ---------------------------------------------------------------------------------------------- the dataset
@pytest.fixture(scope="module")
def mnist_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("mnist_sync"))
    write_mnist(root, fixture_digits(48, 21), fixture_digits(24, 22), layout="gz")
    return root


def test_sync_dataset_and_loader(mnist_root):
    from data_generators import MovingMNIST_synchronized, MovingMNISTLoader
    ds = MovingMNIST_synchronized(False, mnist_root, seq_len=30, num_digits=2, image_size=32, deterministic=False,
                                  three_channels=False, step_length=4, seed=9, length=10)
    _, hit = ds.render(0, 3, hits=True)
    hb = ds.hit_boundary
    assert hb.dtype == np.float64 and hb.shape == (30,) and np.array_equal(hb, hit[0].cpu().numpy())
    assert np.array_equal(hb, sync_hit(9, 1, 2, 32, 4, 30, False)) and ds.__boundary__() is hb
    assert set(np.unique(hb)) <= {0.0, 1.0, 2.0} and (hb == 0).any() and (hb != 0).any()
    ld = MovingMNISTLoader(ds, 4)
    batches = list(ld)
    assert len(ld) == len(batches) == 2
    for g, x in enumerate(batches):
        assert x.is_cuda and tuple(x.shape) == (4, 30, 1, 32, 32) and torch.equal(x, ds.render(4 * g, 4))
    assert torch.equal(ds[5], batches[1][1]) and len(ds) == 10
    want, _, _ = sync_render(fixture_digits(24, 22), 4, 30, 1, 32, 2, 4, False, 9, 1, 4)
    assert torch.equal(batches[1].cpu(), torch.from_numpy(want))


# ---------------------------------------------------------------------------------------------- Evaluator figures
def _solver(tmp_path, **extra):
    from RFN.trainer import Solver
    from tests.test_hip_modules import _tiny_solver_args
    args = _tiny_solver_args("/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/")
    for k, v in extra.items():
        setattr(args, k, v)
    s = Solver(args)
    s.device = torch.device("cuda")
    return s, args


def _plain_evaluator(golden, tmp_path, **settings):
    from RFN import RFN
    from evaluation_metrics import Evaluator
    from tests.test_hip_modules import load_sd
    f = golden("rfn_analysis.pt")["plain"]
    s, args = _solver(tmp_path)
    s.model = load_sd(RFN(Namespace(**f["args"])), f["sd"]).eval()
    return Evaluator(s, settings=Namespace(n_conditions=2, **settings)), f


def test_plot_elbo_gap_pixels(golden, tmp_path, font):
    from evaluation_metrics.curves import elbo_gap_band, elbo_gap_figure
    from rfn_hip import chart, ops
    ev, f = _plain_evaluator(golden, tmp_path)
    x = f["x"].cuda()
    T = int(x.shape[1])
    seen = {}
    plain = ev.model.reconstruct_elbo_gap

    def spy(image, sample=True):
        seen["sample"], seen["out"] = sample, plain(image, sample=sample)
        return seen["out"]
    ev.model.reconstruct_elbo_gap = spy
    try:
        path = ev.plot_elbo_gap(x)
    finally:
        del ev.model.reconstruct_elbo_gap
    assert path == ev.solver.path + "eval_folder/KLDdiagnostic.png" and seen["sample"] is True
    (w, h), px = decode_png(open(path, "rb").read())
    assert (w, h) == (200 * T, 972)
    recons, _, kld, nll = seen["out"]
    bpp = nll[:, :, 0].double().numpy() / (np.log(2.) * 16 * 16)
    fig = elbo_gap_figure(kld[:, 0].double().numpy(), bpp, 16, 16)
    top, sx, sy, _ = elbo_gap_band(T, 16, 16)
    dl = chart.build_display_list(fig)
    want = R.render(dl.table, dl.height, dl.width, font, dl.bg)
    assert np.array_equal(px[top:], want[top:])                      # below the band: the chart
    # inside the band: the sheet of the three rows, the labels left of it, background elsewhere
    rows = [ev.solver.preprocess(x[0], reverse=True), ev.solver.preprocess(recons[0, :, 0].cuda(), reverse=True),
            ev.solver.preprocess(recons[1, :, 0].cuda(), reverse=True)]
    rows[1][0], rows[2][0] = 255, 255
    sheet = ops.compose_sheet(rows, T, scanlines=False).cpu().numpy()
    assert sheet.shape == (3 * 16 + 4 * 2, T * 16 + (T + 1) * 2, 3) and sy + sheet.shape[0] <= top
    assert np.array_equal(px[sy:sy + sheet.shape[0], sx:sx + sheet.shape[1]], sheet)
    want[sy:sy + sheet.shape[0], sx:sx + sheet.shape[1]] = sheet
    assert np.array_equal(px[:top], want[:top])
    assert (px[:top, :sx] != 255).any() and (sheet[2 + 16 + 2:2 + 16 + 2 + 16, 2:2 + 16] == 255).all()   # labels; empty cell
    assert (px[top:] != 255).any()


def test_plot_prob_of_t_pixels(golden, tmp_path, font):
    from evaluation_metrics.curves import prob_of_t_figure
    from rfn_hip import chart
    ev, _ = _plain_evaluator(golden, tmp_path)
    rng = np.random.RandomState(8)
    probT = torch.from_numpy((1.0 + rng.rand(6, 2, 9)).astype(np.float32))
    path = ev.plot_prob_of_t(probT)
    assert path == ev.solver.path + "eval_folder/bpp_sequence.png"
    (w, h), px = decode_png(open(path, "rb").read())
    dl = chart.build_display_list(prob_of_t_figure(probT, 2))
    assert (w, h) == (640, 480) and np.array_equal(px, R.render(dl.table, 480, 640, font, dl.bg))
    assert (px != 255).any()


@pytest.mark.parametrize("draws_per_pass", [None, 2])
def test_get_eval_values_with_extra_plots(golden, tmp_path, capsys, draws_per_pass):
    import warnings
    common = dict(n_frames=5, start_predictions=2, resample=2, n_trained=4, draws_per_pass=draws_per_pass)
    ev, f = _plain_evaluator(golden, tmp_path, extra_plots=True, **common)
    g = torch.Generator().manual_seed(3)
    loader = [torch.rand(2, 5, 1, 16, 16, generator=g) for _ in range(2)]
    folder = ev.solver.path + "eval_folder/"
    capsys.readouterr()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = ev.get_eval_values("rfn.pt", loader=loader)
    printed = capsys.readouterr().out.splitlines()
    assert not any("skipped" in str(w.message) for w in caught)
    lines = [l for l in printed if l.startswith(("BPP Prior:", "BPP Posterior:", "Amortization gap:"))]
    assert [l.split(":")[0] for l in lines] == ["BPP Prior", "BPP Posterior", "Amortization gap"]
    (w, h), _ = decode_png(open(folder + "KLDdiagnostic.png", "rb").read())
    assert (w, h) == (200 * 5, 972)                         # the last batch's five frames
    (w, h), _ = decode_png(open(folder + "bpp_sequence.png", "rb").read())
    assert (w, h) == (640, 480)
    ev2, _ = _plain_evaluator(golden, tmp_path / "plain", **common)
    ref = ev2.get_eval_values("rfn.pt", loader=loader)
    assert not os.path.exists(ev2.solver.path + "eval_folder/KLDdiagnostic.png")
    for a, b in zip(out, ref):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype


# ---------------------------------------------------------------------------------------------- param_plots
@pytest.fixture(scope="module")
def param_run(tmp_path_factory, mnist_root):
    """a small RFN at [2, 1, 32, 32] with random weights, ActNorm initialised by one forward, and its Evaluator"""
    from RFN import RFN
    from evaluation_metrics import Evaluator
    tmp = tmp_path_factory.mktemp("param_plots")
    s, args = _solver(tmp, x_dim=[2, 1, 32, 32], condition_dim=[2, 1, 32, 32], image_size=32, mnist_root=mnist_root,
                      data_seed=3)
    torch.manual_seed(11)
    s.model = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        s.model.loss(s.preprocess(torch.rand(2, 4, 1, 32, 32, generator=g).cuda()), 0)
    s.model.eval()
    return Evaluator(s, args), args, str(tmp)


def _strips(ev, frames):
    from rfn_hip import ops
    frames = frames.cuda()
    return ops.compose_sheet([frames[0, 1:11], frames[0, 11:21], frames[0, 21:29]], 10, gutter=0).cpu().numpy()


def test_param_plots_on_a_small_rfn(param_run, mnist_root, font):
    from data_generators import MovingMNIST_synchronized
    from evaluation_metrics.curves import BLUE, RED
    from rfn_hip import chart, ops
    ev, args, tmp = param_run
    seen = []
    plain = ev.model.param_analysis

    def spy(x, n_pred, n_cond):
        seen.append((x.clone(), n_pred, n_cond, plain(x, n_pred, n_cond)))
        return seen[-1][3]
    ev.model.param_analysis = spy
    figures = []
    render = ops.render_chart
    ops.render_chart = lambda fig, **kw: figures.append(fig) or render(fig, **kw)
    try:
        paths = ev.param_plots(tmp + "/out", 3, n_sequences=4)
    finally:
        del ev.model.param_analysis
        ops.render_chart = render
    assert paths == [tmp + "/out/" + n for n in ("parameter_analysis2.png", "parameter_analysis_mnist_plots_true.png",
                                                  "parameter_analysis_mnist_plots_pred.png")]
    ds = MovingMNIST_synchronized(False, mnist_root, seq_len=30, num_digits=2, image_size=32, deterministic=False,
                                  three_channels=False, step_length=4, seed=3)
    assert len(seen) == 2 and all(s[1:3] == (27, 3) for s in seen)              # 2 batches of 2, ids 0 .. 3 in order
    for g, (x, _, _, _) in enumerate(seen):
        assert torch.equal(x, ev.solver.preprocess(ds.render(2 * g, 2)))
    # the chart: 1000 x 800, the kernel's picture of the figure, dashed lines at the columns of hit_boundary
    (w, h), px = decode_png(open(paths[0], "rb").read())
    dl = chart.build_display_list(figures[0])
    assert (w, h) == (1000, 800) and len(figures) == 1
    assert np.array_equal(px, R.render(dl.table, 800, 1000, font, dl.bg))
    hb = ds.hit_boundary
    want = [(float(k + 1), RED) for k in np.where(hb == 1)[0]] + [(float(k + 1), BLUE) for k in np.where(hb == 2)[0]]
    assert (hb[:29] == 1).any() and (hb[:29] == 2).any()
    lines = dl.table[(dl.table[:, 0] == chart.BOX) & (dl.table[:, 6] > 0)]
    drawn = [v for v in want if v[0] <= 29]                  # k + 1 = 30 lies outside the axes
    assert len(lines) == 2 * len(drawn)
    for i, ax in enumerate(chart.layout(figures[0])):
        assert figures[0].panels[i].vlines == want and ax.xlim == (1.0, 29.0)
        for rec, (v, colour) in zip(lines[i * len(drawn):], drawn):
            assert (rec[2] + rec[4]) // 2 == ax.subpixel(v, 0)[0] and rec[1] == chart.rgba(colour)
            # the picture carries the colour on the line's columns (a 2-pixel line covers one column whole); at
            # x = 1 and x = 29 the axes' frame, drawn later, lies over the line
            if 1 < v < 29:
                cols = px[ax.y0 + 2:ax.y1 - 1, rec[2] // 16:rec[4] // 16 + 1].reshape(-1, 3)
                assert (cols == np.array(colour, dtype=np.uint8)).all(1).any(), (v, colour)
    # the strips: sequence 0 of the last batch, frames 1:11, 11:21, 21:29
    x_last, _, _, out = seen[-1]
    for path, frames in ((paths[1], x_last), (paths[2], out[6])):
        (w, h), px = decode_png(open(path, "rb").read())
        assert (w, h) == (10 * 32, 3 * 32) and np.array_equal(px, _strips(ev, frames))
        assert (px[64:, 8 * 32:] == 255).all()                                  # the third strip has 8 cells
    # the curves are those of the numpy restatement on the tensors the model returned
    for first, panel in enumerate(figures[0].panels):
        for s, k in zip(panel.series, (first, first + 2, first + 4)):
            sums = np.stack([o[3][k].sum([2, 3, 4]).double().numpy() for o in seen])
            m = sums.mean(axis=(0, 2))
            with np.errstate(invalid="ignore"):   # a zero-initialised head gives a constant curve: 0 / 0, not drawn
                assert np.array_equal(s.y, (m - m.min()) / (m.max() - m.min()), equal_nan=True)
    assert sum(bool(np.isfinite(s.y).all()) for panel in figures[0].panels for s in panel.series) >= 4


def test_param_plots_curves_are_exact_with_integer_parameters(param_run):
    from rfn_hip import ops
    ev, args, tmp = param_run
    rng = np.random.RandomState(13)
    outs = []

    def stub(x, n_pred, n_cond):
        z = [torch.from_numpy(rng.randint(-9, 10, size=(29, 2, 4, 8, 8)).astype(np.float32)) for _ in range(4)]
        fl = [torch.from_numpy(rng.randint(-9, 10, size=(29, 2, 2, 16, 16)).astype(np.float32)) for _ in range(2)]
        outs.append(tuple(z + fl) + (torch.zeros(2, 30, 1, 32, 32),))
        return outs[-1]
    figures = []
    render = ops.render_chart
    ev.model.param_analysis = stub
    ops.render_chart = lambda fig, **kw: figures.append(fig) or render(fig, **kw)
    try:
        ev.param_plots(tmp + "/exact", 5, n_sequences=5)         # 5 sequences: 2 batches of 2, the fifth is dropped
    finally:
        del ev.model.param_analysis
        ops.render_chart = render
    assert len(outs) == 2
    for first, panel in enumerate(figures[0].panels):
        for s, k in zip(panel.series, (first, first + 2, first + 4)):
            # integer sums below 2^24: exact in float32, so the float64 restatement from the raw tensors is THE value
            sums = np.stack([o[k].double().numpy().sum(axis=(2, 3, 4)) for o in outs])
            m = sums.mean(axis=(0, 2))
            assert np.array_equal(s.y, (m - m.min()) / (m.max() - m.min())) and s.y.min() == 0.0 and s.y.max() == 1.0


def test_param_plots_refusals(param_run, tmp_path):
    ev, args, tmp = param_run
    ev.choose_data = "bair"
    try:
        with pytest.raises(ValueError, match="SM-MNIST"):
            ev.param_plots(str(tmp_path), 3)
    finally:
        ev.choose_data = "mnist"
    root = args.mnist_root
    args.mnist_root = str(tmp_path / "nowhere")
    try:
        with pytest.raises(ValueError, match="MNIST test images"):
            ev.param_plots(str(tmp_path), 3)
    finally:
        args.mnist_root = root
