"""CPU tests of the analysis figures' host side: the synchronized Moving MNIST walk restated on the addressed draws
(tests/sync_mnist_ref.py), the argument checks of MovingMNIST_synchronized, the chart capabilities the figures need
(bars, coloured vertical lines, fixed limits and ticks, stacked panels, the reserved band, free text) read from the
display lists of plot_elbo_gap / plot_prob_of_t / param_plots on synthetic inputs, their statistics against float64
numpy, and the driver's --eval_parameters / --extra_plots wiring with stub evaluators."""
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.sync_mnist_ref import SHARED_SEQ, sync_hit, sync_render, sync_walk
from tests.test_moving_mnist_host import D, fixture_digits, write_mnist

# (B, T, S, digits, L, deterministic, C) of the GPU comparison (tests/test_analysis_figures.py) and the key of each
SYNC_CASES = [(1, 1, 29, 1, 1, False, 1), (3, 12, 32, 2, 4, False, 1), (7, 30, 32, 3, 1, True, 3),
              (5, 30, 64, 2, 4, False, 1), (2, 9, 29, 8, 4, False, 3)]


def sync_case_key(B, T, S, nd, L, det, C):
    """(seed, split, first_id) of a case"""
    return 5 + S + T, int(det), 17 * B


# ---------------------------------------------------------------------------------------------- the walk
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("det", [False, True])
def test_sync_walk_shares_positions_and_addresses(L, det):
    N, S, T = 1000, 32, 25
    R = S - D
    idx = set()
    for n in range(3):
        adr_a, adr_b = [], []
        a, hits_a = sync_walk(7, 1, 3, n, N, S, L, T, det, addresses=adr_a)
        b, hits_b = sync_walk(7, 1, (1 << 40) + 9, n, N, S, L, T, det, addresses=adr_b)
        assert [p[1:] for p in a] == [p[1:] for p in b] and hits_a == hits_b          # every (y, x) is shared
        assert len({p[0] for p in a}) == 1 and 0 <= a[0][0] < N
        idx.add((a[0][0], b[0][0]))
        # idx: draw 0 at the sequence's own address; everything else at the shared address, draws 1, 2, 3, ... in order
        assert adr_a[0] == (3, 0) and adr_b[0] == ((1 << 40) + 9, 0)
        assert adr_a[1:] == adr_b[1:] == [(SHARED_SEQ, j) for j in range(1, len(adr_a))]
        assert (len(adr_a) == 3) == (det or not any(hits_a))
        assert all(0 <= y <= R - 1 and 0 <= x <= R - 1 for _, y, x in a)               # positions stay in the frame
        # dx = dy = 3 whatever L is: until the first clamp the walk moves by (3, 3)
        first = hits_a.index(True) if any(hits_a) else T
        assert first >= 1 and not hits_a[0]
        for t in range(1, first):
            assert (a[t][1] - a[t - 1][1], a[t][2] - a[t - 1][2]) == (3, 3)
        if first < T:   # the clamped frame follows a step of 3 that left [0, R - 1]
            y, x = a[first - 1][1] + 3, a[first - 1][2] + 3
            assert y >= R or x >= R
    assert any(i != j for i, j in idx)                                                 # the identities differ


def test_sync_hit_is_the_last_clamped_digit():
    for S, L, det, nd in ((32, 4, False, 3), (29, 1, True, 2), (40, 4, False, 8)):
        T = 30
        hit = sync_hit(11, 1, nd, S, L, T, det)
        per_digit = [sync_walk(11, 1, 5, n, 10, S, L, T, det)[1] for n in range(nd)]
        for t in range(T):
            clamped = [n for n in range(nd) if per_digit[n][t]]
            assert hit[t] == (clamped[-1] + 1 if clamped else 0)
        assert (hit == 0).any() and (hit != 0).any()
    _, _, h = sync_render(fixture_digits(4, 0), 3, 12, 1, 32, 2, 4, False, 2, 1, 40)
    assert h.dtype == np.int32 and h.shape == (3, 12) and (h == h[0]).all()


@pytest.mark.parametrize("case", SYNC_CASES)
def test_gpu_cases_reach_both_hit_values(case):
    """the seeds of the GPU comparison give a zero and a non-zero hit wherever the issue asks for both"""
    B, T, S, nd, L, det, C = case
    seed, split, _ = sync_case_key(*case)
    hit = sync_hit(seed, split, nd, S, L, T, det)
    if S in (29, 32) and T >= 9:
        assert (hit == 0).any() and (hit != 0).any(), hit


def test_sync_dataset_argument_checks(tmp_path):
    from data_generators import MovingMNIST_synchronized
    write_mnist(str(tmp_path), fixture_digits(4, 7), fixture_digits(5, 8))
    ok = dict(train=False, data_root=str(tmp_path), image_size=32)
    ds = MovingMNIST_synchronized(**ok)
    assert len(ds) == 5 and ds.sequence_id(3, epoch=9) == 3 and ds.channels == 3 and ds.seq_len == 20
    assert len(MovingMNIST_synchronized(length=2, three_channels=False, **ok)) == 2
    assert MovingMNIST_synchronized(True, str(tmp_path)).sequence_id(1, epoch=2) == 9
    for bad, exc in ((dict(digit_size=32), ValueError), (dict(image_size=28), ValueError),
                     (dict(num_digits=0), ValueError), (dict(num_digits=9), ValueError),
                     (dict(normalize=True), NotImplementedError), (dict(make_target=True), NotImplementedError)):
        with pytest.raises(exc):
            MovingMNIST_synchronized(**dict(ok, **bad))
    with pytest.raises(TypeError):     # the reference's class has no set_starting_position
        MovingMNIST_synchronized(set_starting_position=False, **ok)


# ---------------------------------------------------------------------------------------------- chart capabilities
def _boxes(dl, layer):
    from rfn_hip import chart
    t = dl.table[np.array(dl.layers) == layer]
    return t[t[:, 0] == chart.BOX]


def _inside(rec, ax):
    return 16 * ax.x0 <= rec[2] <= rec[4] <= 16 * ax.x1 and 16 * ax.y0 <= rec[3] <= rec[5] <= 16 * ax.y1


def test_defaults_leave_existing_display_lists_alone():
    """rows = 1, top = 0, no bars / vlines / limits / texts: the layout and the table of the merged figures"""
    from rfn_hip import chart
    from tests import chart_cases as K
    fig = K.small_figure()
    assert (fig.rows, fig.top, fig.texts) == (1, 0, [])
    assert all(p.vlines == [] and p.xlim is None and p.ylim is None and p.xticks is None for p in fig.panels)
    assert all(s.bar is None for p in fig.panels for s in p.series)
    u = fig.text_scale
    t, pad, tick = u + u // 2, 4 * u, 3 * u
    for ax in chart.layout(fig):
        assert ax.top == 0 and ax.y0 == pad + 7 * t + pad
        assert ax.y1 == fig.height - (tick + pad + 7 * u + pad + 7 * t + pad) - (7 * u + 2 * pad)


def test_bars_are_boxes_at_the_mapped_coordinates_clipped_to_the_axes():
    from rfn_hip import chart
    x = np.arange(4)
    y = np.array([2.0, -1.0, float("nan"), 9.0])
    mk = lambda **kw: chart.Figure([chart.Panel(series=[chart.Series(x, y, (9, 8, 7), line=False, bar=(0.5, 0.25),
                                                                     label="b")], **kw)], width=400, height=300)
    fig = mk()
    ax = chart.layout(fig)[0]
    # autoscale takes the bars' x extents and the baseline
    assert ax.xlim == chart.autoscale([0.25 - 0.25, 3.25 + 0.25]) and ax.ylim == chart.autoscale([-1.0, 9.0, 0.0])
    dl = chart.build_display_list(fig)
    bars = _boxes(dl, "bands")
    assert len(bars) == 3 + 1                                  # the finite points, and the legend's sample box
    for rec, i in zip(bars, (0, 1, 3)):
        x0, y_val = ax.subpixel(x[i] + 0.25 - 0.25, y[i])
        x1, base = ax.subpixel(x[i] + 0.25 + 0.25, 0.0)
        assert tuple(rec[2:6]) == (x0, min(base, y_val), x1, max(base, y_val)) and rec[1] == chart.rgba((9, 8, 7))
        assert (rec[6], rec[7]) == (0, 0) and _inside(rec, ax)
    assert not _inside(bars[3], ax) and bars[3][3] > 16 * ax.y1     # the sample lies in the legend row
    assert not (np.array(dl.layers) == "lines").any()          # line=False: bars only
    # fixed limits clip: the bar of 9 is cut at ylim's top, the bar of -1 lies wholly below ylim and is left out,
    # the bar at x = 0 is cut at xlim's left end
    fig = mk(xlim=(0.1, 3.2), ylim=(0.5, 4.0))
    ax = chart.layout(fig)[0]
    assert (ax.xlim, ax.ylim) == ((0.1, 3.2), (0.5, 4.0))
    bars = _boxes(chart.build_display_list(fig), "bands")[:-1]
    assert len(bars) == 2 and all(_inside(r, ax) for r in bars)
    assert bars[0][2] == 16 * ax.x0 and bars[0][5] == 16 * ax.y1 and bars[0][3] == ax.subpixel(0.0, 2.0)[1]
    assert bars[1][3] == 16 * ax.y0 and bars[1][5] == 16 * ax.y1 and bars[1][4] == 16 * ax.x1
    with pytest.raises(ValueError, match="bar"):
        chart.Series(x, y, (0, 0, 0), bar=(0.0, 0.0))
    with pytest.raises(ValueError, match="ylim"):
        chart.Panel(ylim=(1.0, 1.0))


def test_coloured_vlines_ticks_rows_band_and_text():
    from rfn_hip import chart
    x = np.arange(1, 11)
    s = lambda: [chart.Series(x, x * 0.5, chart.TAB10[0], label="a")]
    red, blue = (255, 0, 0), (0, 0, 255)
    panels = [chart.Panel(series=s(), vlines=[(3, red), (7, blue), (40, red)], xlim=(1, 10), xticks=[1, 5.5, 10, 11]),
              chart.Panel(series=s(), vline=4, vlines=[(2, blue)])]
    fig = chart.Figure(panels, width=500, height=700, rows=2, top=100, texts=[(8, 20, "GT:"), (8, 60, "Prior:")])
    axes = chart.layout(fig)
    rh = (700 - 100) // 2
    assert [a.top for a in axes] == [100, 100 + rh] and axes[0].x0 == axes[1].x0 and axes[0].x1 == axes[1].x1
    assert axes[0].top < axes[0].y0 < axes[0].y1 < axes[1].top < axes[1].y0 < axes[1].y1 <= 700   # no overlap
    assert axes[0].y1 - axes[0].y0 == axes[1].y1 - axes[1].y0
    dl = chart.build_display_list(fig)
    assert np.array_equal(dl.table, chart.build_display_list(fig).table)
    chart.check_table(dl.table)
    lines = _boxes(dl, "lines")
    dashed = lines[lines[:, 6] > 0]
    # panel 0: red at 3, blue at 7 (40 is outside xlim); panel 1: the black vline, then blue at 2
    want = [(axes[0], 3, red), (axes[0], 7, blue), (axes[1], 4, chart.BLACK), (axes[1], 2, blue)]
    assert len(dashed) == len(want)
    for rec, (ax, v, colour) in zip(dashed, want):
        assert (rec[2] + rec[4]) // 2 == ax.subpixel(v, 0)[0] and (rec[3], rec[5]) == (16 * ax.y0, 16 * ax.y1)
        assert rec[1] == chart.rgba(colour)
    # explicit ticks: 1, 5.5 and 10 (11 is outside), one decimal
    glyphs = dl.table[dl.table[:, 0] == chart.GLYPH]
    row = glyphs[glyphs[:, 3] == 16 * (axes[0].y1 + 3 * 2 + 4 * 2)]
    assert "".join(chr(c) for c in row[:, 4]) == "1.05.510.0"
    # the reserved band holds the free text and nothing else
    ys = {chart.BOX: (3, 5), chart.CAPSULE: (3, 5), chart.TRAPEZOID: (4, 5, 6, 7), chart.TRIANGLE: (3, 5, 7),
          chart.GLYPH: (3,)}
    in_band = [rec for rec in dl.table if min(rec[k] for k in ys[rec[0]]) < 16 * 100]
    assert "".join(chr(r[4]) for r in in_band) == "GT:Prior:" and all(r[0] == chart.GLYPH for r in in_band)
    assert [tuple(r[2:4]) for r in in_band[:2]] == [(16 * 8, 16 * 20), (16 * (8 + 12), 16 * 20)]
    # a legend row per grid row, under its own panel
    legend = [r for r in dl.table if r[0] == chart.CAPSULE and r[3] == r[5] and
              r[3] in (16 * (100 + rh - 8 - 14) + 16 * 7, 16 * (100 + 2 * rh - 8 - 14) + 16 * 7)]
    assert len(legend) == 2
    with pytest.raises(ValueError, match="rows"):
        chart.Figure(panels + [chart.Panel()], rows=2)
    with pytest.raises(ValueError, match="reserved"):
        chart.Figure(panels, height=90, top=90)


# ---------------------------------------------------------------------------------------------- the three figures
def _elbo_inputs(T=10):
    rng = np.random.RandomState(4)
    kld = rng.rand(T) * 30
    kld[0] = 0.0
    bpp = 1.0 + rng.rand(2, T)
    bpp[:, 0] = 0.0
    return kld, bpp


def test_elbo_gap_figure_display_list():
    from evaluation_metrics.curves import ROW_LABELS, bpp_ylim, elbo_gap_band, elbo_gap_figure
    from rfn_hip import chart
    kld, bpp = _elbo_inputs()
    H = W = 32
    fig = elbo_gap_figure(kld, bpp, H, W)
    top, sx, sy, label_y = elbo_gap_band(10, H, W)
    assert (fig.width, fig.height, fig.rows, fig.top) == (2000, 972, 2, top)
    assert top == 3 * H + 4 * 2 + 2 * 8 and sy == 8 and sx == 8 + chart.text_width("Posterior:", 2) + 8
    assert sx + 10 * W + 11 * 2 <= fig.width
    a0, a1 = chart.layout(fig)
    assert top <= a0.top < a0.y0 < a0.y1 < a1.top < a1.y0 < a1.y1 <= 972
    assert a0.xlim == a1.xlim == (-0.5, 9.5) and a1.ylim == bpp_ylim(bpp)
    dl = chart.build_display_list(fig)
    assert np.array_equal(dl.table, chart.build_display_list(elbo_gap_figure(kld, bpp, H, W)).table)
    chart.check_table(dl.table)
    bars = _boxes(dl, "bands")
    in0, in1 = [r for r in bars if _inside(r, a0)], [r for r in bars if _inside(r, a1)]
    # KLD: one bar per frame with kld > 0 (a bar of height zero is empty); BPP: frame 0 is 0, below ylim -> left out
    assert len(in0) == 9 and len(in1) == 2 * 9 and len(bars) == len(in0) + len(in1) + 3   # + three legend samples
    for rec, t in zip(in0, range(1, 10)):
        assert (rec[2], rec[4]) == (a0.subpixel(t - 0.15, 0)[0], a0.subpixel(t + 0.15, 0)[0])
        assert (rec[3], rec[5]) == (a0.subpixel(0, kld[t])[1], a0.subpixel(0, 0.0)[1])
    for z, colour, off in ((0, chart.TAB10[0], -0.15), (1, chart.TAB10[1], 0.15)):
        mine = [r for r in in1 if r[1] == chart.rgba(colour)]
        assert len(mine) == 9
        for rec, t in zip(mine, range(1, 10)):
            assert (rec[2], rec[4]) == (a1.subpixel(t + off - 0.15, 0)[0], a1.subpixel(t + off + 0.15, 0)[0])
            assert (rec[3], rec[5]) == (a1.subpixel(0, bpp[z, t])[1], 16 * a1.y1)      # the baseline 0 is below ylim
    # the band: the three labels at their rows and nothing else
    in_band = [rec for rec in dl.table if rec[3] < 16 * top]
    assert all(r[0] == chart.GLYPH for r in in_band)
    assert "".join(chr(r[4]) for r in in_band) == "".join(ROW_LABELS)
    assert sorted({r[3] // 16 for r in in_band}) == label_y and all(r[2] // 16 < sx for r in in_band)
    for r in range(3):
        assert sy + 2 + r * (H + 2) <= label_y[r] <= sy + 2 + r * (H + 2) + H - 14
    # both panels carry a legend; a tick per frame
    text = "".join(chr(c) for c in dl.table[dl.table[:, 0] == chart.GLYPH][:, 4])
    assert "PriorPosterior" in text and text.count("0123456789") == 2 and text.count("Avg.KLD") == 2
    with pytest.raises(ValueError, match="fit"):
        elbo_gap_figure(kld, bpp, 400, 400)


def test_prob_of_t_figure_and_statistics():
    from evaluation_metrics.curves import prob_of_t_figure, prob_of_t_statistics
    from rfn_hip import chart
    rng = np.random.RandomState(5)
    probT = torch.from_numpy((rng.rand(7, 2, 12) * 2 + 1).astype(np.float32))
    mean, ci = prob_of_t_statistics(probT)
    v = probT[:, 0, :].numpy().astype(np.float64)
    assert np.array_equal(mean, v.mean(0)) and np.array_equal(ci, 1.96 * np.std(v, 0) / np.sqrt(np.shape(v)[0]))
    assert mean.dtype == np.float64 and np.array_equal(prob_of_t_statistics(probT[:1])[1], np.zeros(12))
    fig = prob_of_t_figure(probT, 5)
    assert (fig.width, fig.height, fig.legend, len(fig.panels)) == (640, 480, False, 1)
    p = fig.panels[0]
    assert (p.title, p.xlabel, p.ylabel, p.grid) == ("P(X_5 = X_t | X_<5)", "Frame number", "Bits per pixel", True)
    s = p.series[0]
    assert np.array_equal(s.x, 5 + np.arange(12)) and np.array_equal(s.y, mean)
    assert np.array_equal(s.band[0], mean - ci) and np.array_equal(s.band[1], mean + ci)
    dl = chart.build_display_list(fig)
    assert np.array_equal(dl.table, chart.build_display_list(prob_of_t_figure(probT, 5)).table)
    chart.check_table(dl.table)
    layers = np.array(dl.layers)
    assert (layers == "bands").sum() == 11 and (layers == "lines").sum() == 11 and (layers == "grid").sum() > 4
    with pytest.raises(ValueError):
        prob_of_t_statistics(np.zeros((3, 4)))


def test_bpp_ylim_and_minmax_scale():
    from evaluation_metrics.curves import bpp_ylim, minmax_scale, parameter_curves
    _, bpp = _elbo_inputs()
    low = min(min(bpp[0, 1:]), min(bpp[1, 1:]))
    high = max(max(bpp[0, 1:]), max(bpp[1, 1:]))
    assert bpp_ylim(torch.from_numpy(bpp)) == (low - 0.5 * (high - low), high + 0.5 * (high - low))
    assert bpp_ylim(np.ones((2, 5))) is None and bpp_ylim(np.ones((2, 1))) is None
    x = np.array([3.0, -1.0, 0.5, 7.0])
    assert np.array_equal(minmax_scale(x), (x - x.min()) / (x.max() - x.min()))
    assert minmax_scale(x).min() == 0.0 and minmax_scale(x).max() == 1.0
    rng = np.random.RandomState(6)
    sums = [[torch.from_numpy(rng.randint(-50, 50, size=(29, 2)).astype(np.float32)) for _ in range(6)] for _ in range(3)]
    curves = parameter_curves(sums)
    for k in range(6):
        m = np.stack([b[k].numpy().astype(np.float64) for b in sums]).mean(axis=(0, 2))
        assert curves[k].shape == (29,) and np.array_equal(curves[k], (m - m.min()) / (m.max() - m.min()))


def test_param_figure_display_list():
    from evaluation_metrics.curves import BLUE, PARAM_NAMES, RED, param_figure
    from rfn_hip import chart
    rng = np.random.RandomState(7)
    curves = [rng.rand(29) for _ in range(6)]
    hit = np.zeros(30)
    hit[[4, 11, 28]] = 1
    hit[[7, 11 + 1, 29]] = 2          # k + 1 = 30 is outside the x range and is not drawn
    fig = param_figure(curves, hit)
    assert (fig.width, fig.height, fig.rows, fig.top) == (1000, 800, 2, 0)
    for first, p in enumerate(fig.panels):
        assert [s.label for s in p.series] == [PARAM_NAMES[k] for k in (first, first + 2, first + 4)]
        assert all(np.array_equal(s.x, np.arange(1, 30)) for s in p.series) and p.ylabel == "Average"
        assert all(np.array_equal(s.y, curves[k]) for s, k in zip(p.series, (first, first + 2, first + 4)))
    axes = chart.layout(fig)
    assert all(ax.xlim == (1.0, 29.0) for ax in axes) and axes[0].y1 < axes[1].top
    dl = chart.build_display_list(fig)
    assert np.array_equal(dl.table, chart.build_display_list(param_figure(curves, hit)).table)
    chart.check_table(dl.table)
    lines = _boxes(dl, "lines")
    dashed = lines[lines[:, 6] > 0]
    want = [(ax, k + 1, c) for ax in axes for k, c in ((4, RED), (11, RED), (28, RED), (7, BLUE), (12, BLUE))]
    assert len(dashed) == len(want)                 # one dashed box per hit and panel
    for rec, (ax, v, colour) in zip(dashed, want):
        assert (rec[2] + rec[4]) // 2 == ax.subpixel(v, 0)[0] and rec[1] == chart.rgba(colour)
        assert (rec[3], rec[5]) == (16 * ax.y0, 16 * ax.y1)
    text = "".join(chr(c) for c in dl.table[dl.table[:, 0] == chart.GLYPH][:, 4])
    assert "muprior" in text and "sigmabasedist" in text


# ---------------------------------------------------------------------------------------------- driver and Evaluator
class _StubEvaluator(object):
    def __init__(self, log):
        self.log, self.model, self.extra_plots = log, Namespace(temperature=None, kl_temperature=None), False
        self.test_loader = [torch.zeros(2, 30, 1, 8, 8)]

    def param_analysis(self, image, n_predictions, n_conditions):
        self.log.append(("param_analysis", tuple(image.shape), n_predictions, n_conditions))
        return tuple(torch.full((1,), float(k)) for k in range(7))

    def param_plots(self, path, n_conditions):
        import os
        self.log.append(("param_plots", path, n_conditions, os.path.isfile(path + "/param_analysis.pt")))
        return []

    def __getattr__(self, name):
        if name.startswith("plot_"):
            return lambda *a, **k: self.log.append((name,))
        raise AttributeError(name)


@pytest.mark.parametrize("data", ["mnist", "bair"])
def test_driver_eval_parameters(tmp_path, capsys, monkeypatch, data):
    from evaluation_metrics import eval_settings as E
    log = []
    folder = str(tmp_path / "run" / "eval_folder")
    (tmp_path / "run" / "eval_folder").mkdir(parents=True)
    monkeypatch.setattr(E, "build_evaluator",
                        lambda settings, i: (_StubEvaluator(log), Namespace(choose_data=data), folder, None))
    settings = E.parse_args(["--folder_path", str(tmp_path) + "/", "--experiment_names", "run", "--eval_parameters",
                             "--no-calc_eval", "--n_conditions", "4"])
    E.main(settings)
    out = capsys.readouterr().out
    saved = torch.load(folder + "/param_analysis.pt", weights_only=True)
    assert tuple(saved) == E.PARAM_KEYS and log[0] == ("param_analysis", (2, 30, 1, 8, 8), 26, 4)
    calls = [c for c in log if c[0] == "param_plots"]
    assert "is not drawn" not in out
    if data == "mnist":
        assert calls == [("param_plots", folder, 4, True)] and log[1] == calls[0]      # once, after the tensors
        assert "SM-MNIST" not in out
    else:
        assert calls == [] and sum("param_plots need an SM-MNIST run" in line for line in out.splitlines()) == 1
    assert "elbo gap" in E.build_parser().format_help() and "warning is given" not in E.build_parser().format_help()


class _StubModel(object):
    def eval(self):
        return self

    def predict(self, image, n_predictions, n_conditions):
        return None, torch.zeros((n_predictions, image.shape[0]) + tuple(image.shape[2:]))

    def loss(self, x, logdet):
        return torch.tensor(0.0), torch.tensor(1.0), torch.tensor(2.0)

    def probability_future(self, x, n_conditions):
        return torch.full((x.shape[0], 2, x.shape[1] - n_conditions - 1), 64.0 * np.log(2.0))

    def reconstruct_elbo_gap(self, x, sample=True):
        assert sample is False
        nll = torch.zeros(2, x.shape[1], x.shape[0])
        nll[0], nll[1] = 3 * 64.0 * np.log(2.0), 64.0 * np.log(2.0)
        return 0, 0, torch.zeros(x.shape[1], x.shape[0]), nll


def _stub_run(tmp_path, **settings):
    from evaluation_metrics import Evaluator
    pre = lambda x, reverse=False: x.byte() if reverse else x
    solver = Namespace(model=_StubModel(), args=Namespace(n_frames=6, n_conditions=2), device=torch.device("cpu"),
                       preprocess=pre, path=str(tmp_path) + "/")
    ev = Evaluator(solver, settings=Namespace(n_frames=6, start_predictions=2, resample=2, n_trained=5, **settings))
    calls = []
    ev.eval_seq = lambda gt, pred: tuple(torch.ones(gt.shape[0], gt.shape[1]) for _ in range(3))
    ev.plot_elbo_gap = lambda image: calls.append(("plot_elbo_gap", tuple(image.shape))) or "a"
    ev.plot_prob_of_t = lambda probT: calls.append(("plot_prob_of_t", probT.clone())) or "b"
    loader = [torch.zeros(3, 6, 1, 8, 8), torch.ones(3, 6, 1, 8, 8)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = ev.get_eval_values("rfn.pt", loader=loader)
    return out, calls, [str(w.message) for w in caught]


def test_extra_plots_no_longer_warns_and_draws_after_the_loop(tmp_path, capsys):
    plain, calls, caught = _stub_run(tmp_path)
    assert calls == [] and caught == []
    capsys.readouterr()
    out, calls, caught = _stub_run(tmp_path, extra_plots=True)
    printed = capsys.readouterr().out.splitlines()
    assert not any("skipped" in m for m in caught), caught
    assert [t.shape if t is not None else None for t in out] == [t.shape if t is not None else None for t in plain]
    # the three lines, then the two figures: the last batch, and nll_prob of both batches in bits per pixel
    assert printed[0].startswith("BPP Prior:  tensor(3.") and printed[1].startswith("BPP Posterior:  tensor(1.")
    assert printed[2].startswith("Amortization gap: tensor(2.") and len(printed) == 3
    assert [c[0] for c in calls] == ["plot_elbo_gap", "plot_prob_of_t"] and calls[0][1] == (3, 6, 1, 8, 8)
    assert tuple(calls[1][1].shape) == (6, 2, 3) and torch.allclose(calls[1][1], torch.ones(6, 2, 3))
    # debug_plot still draws nothing on the per-draw path, and says so
    _, calls, caught = _stub_run(tmp_path, debug_plot=True)
    assert calls == [] and len(caught) == 1 and "debug_plot" in caught[0] and "skipped" in caught[0]
