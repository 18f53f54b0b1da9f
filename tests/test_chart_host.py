"""CPU tests of the curve figures' host side: evaluation_metrics.curves.curve_statistics against the reference's
expressions, the tick rule and tick labels of rfn_hip.chart, the display list of a fixed figure (deterministic, drawn
in the documented order), the built-in font, the argument checks of ops.render_chart, Evaluator.plot_eval_values /
test_temp_values with render_chart replaced by a recorder, and the driver's last step when its files are absent."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import chart_cases as K


def test_curve_statistics_are_the_references_expressions():
    from evaluation_metrics.curves import curve_statistics
    rng = np.random.RandomState(3)
    for n in (1, 2, 7):
        v = torch.from_numpy(rng.rand(n, 5).astype(np.float32) * 3 - 1)
        s = curve_statistics(v)
        x, alpha = v.numpy().astype(np.float64), 0.05
        # error_metrics.py:836-864 of the reference, on float64
        want = {"mean": x.mean(0), "ci": 1.96 * np.std(x, 0) / np.sqrt(np.shape(x)[0]), "median": np.median(x, 0),
                "q_lo": np.quantile(x, alpha / 2, axis=0), "q_hi": np.quantile(x, 1 - alpha / 2, axis=0)}
        assert set(s) == set(want)
        for k in want:
            assert s[k].dtype == np.float64 and s[k].shape == (5,) and np.array_equal(s[k], want[k]), (n, k)
    assert np.array_equal(curve_statistics(np.ones((1, 3)))["ci"], np.zeros(3))
    with pytest.raises(ValueError):
        curve_statistics(np.zeros(4))


def test_tick_rule():
    from rfn_hip import chart
    rng = np.random.RandomState(0)
    spans = [10.0 ** e for e in np.arange(-4, 3.01, 0.25)]
    for span in spans:
        for lo in (0.0, -span / 3, rng.rand() * 10 * span, 1000 * span, -17.3):
            hi = lo + span
            ticks, decimals = chart.nice_ticks(lo, hi)
            assert 3 <= len(ticks) <= 8, (lo, hi, ticks)
            assert all(lo <= t <= hi for t in ticks), (lo, hi, ticks)
            assert all(b > a for a, b in zip(ticks, ticks[1:]))
            steps = np.diff(ticks)
            assert np.allclose(steps, steps[0], rtol=1e-9)
            mant = steps[0] / 10.0 ** np.floor(np.log10(steps[0]) + 1e-9)
            assert min(abs(mant - m) for m in (1, 2, 2.5, 5, 10)) < 1e-6, (lo, hi, ticks)
            labels = [chart.format_tick(t, decimals) for t in ticks]
            assert len(set(labels)) == len(labels) and [float(l) for l in labels] == ticks
    for v in (0.0, 0.7, -3.0, 1e-4, 1e3):           # a degenerate range
        ticks, _ = chart.nice_ticks(v, v)
        assert 3 <= len(ticks) <= 8 and all(b > a for a, b in zip(ticks, ticks[1:]))
    ticks, decimals = chart.nice_ticks(4.0, 30.2, integer=True)     # the frame axis: whole numbers
    assert ticks == [5.0, 10.0, 15.0, 20.0, 25.0, 30.0] and decimals == 0
    assert chart.nice_ticks(1.9, 5.1, integer=True)[0] == [2.0, 3.0, 4.0, 5.0]
    assert chart.nice_ticks(0.0, 1.0)[0] == [0.0, 0.2, 0.4, 0.6, 0.8, 1.0]
    assert chart.nice_ticks(0.51, 0.69) == ([0.525, 0.55, 0.575, 0.6, 0.625, 0.65, 0.675], 3)


def test_tick_labels_autoscale_and_mapping():
    from rfn_hip import chart
    assert chart.format_tick(0.5, 1) == "0.5" and chart.format_tick(20.0, 0) == "20"
    assert chart.format_tick(-0.0, 1) == "0.0" and chart.format_tick(-1e-9, 2) == "0.00"
    assert chart.format_tick(0.00025, 5) == "0.00025" and chart.format_tick(-12.5, 1) == "-12.5"
    assert chart.format_tick(1000.0, 0) == "1000"
    assert chart.autoscale([1.0, 3.0]) == (0.9, 3.1)                      # matplotlib's 5 % margins
    assert chart.autoscale([2.0, float("nan"), float("inf")]) == (1.9, 2.1)
    assert chart.autoscale([0.0]) == (-0.05, 0.05) and chart.autoscale([]) == (0.0, 1.0)
    # lo lands on p_lo, hi on p_hi, the middle halfway (rounded half up), on a growing and on a falling pixel axis
    assert chart.data_to_subpixel(2.0, 2.0, 6.0, 160, 1760) == 160
    assert chart.data_to_subpixel(6.0, 2.0, 6.0, 160, 1760) == 1760
    assert chart.data_to_subpixel(3.0, 2.0, 6.0, 160, 1760) == 560
    assert chart.data_to_subpixel(0.25, 0.0, 1.0, 1600, 160) == 1240
    assert chart.data_to_subpixel(0.5, 0.0, 1.0, 0, 3) == 2
    assert chart.TAB10[0] == (31, 119, 180) and chart.TAB10[3] == (214, 39, 40) and len(chart.TAB10) == 10
    assert chart.MARKERS == ("o", "v", "x", "*", "^", "s", "H", "P", "X", "1", "2", "3")
    for m in chart.MARKERS:
        recs = chart.marker(m, 1000, 900, 56, (1, 2, 3))
        assert recs and all(len(r) == chart.REC for r in recs)
        assert len(recs) == 3 if m in "123*" else True


def test_display_list_is_deterministic_and_ordered():
    from rfn_hip import chart
    a, b = chart.build_display_list(K.small_figure()), chart.build_display_list(K.small_figure())
    assert a.table.dtype == np.int32 and a.table.shape[1] == 12 and np.array_equal(a.table, b.table)
    assert a.layers == b.layers and len(a.layers) == a.table.shape[0]
    assert (a.width, a.height, a.bg) == (324, 120, (255, 255, 255))
    order = [chart.LAYERS.index(l) for l in a.layers]
    assert chart.LAYERS == ("background", "grid", "bands", "lines", "markers", "frame", "text")
    assert order == sorted(order) and set(a.layers) == set(chart.LAYERS)
    kinds = {l: set(a.table[np.array(a.layers) == l, 0].tolist()) for l in chart.LAYERS}
    assert kinds["background"] == {chart.BOX} and kinds["grid"] == {chart.BOX} and kinds["frame"] == {chart.BOX}
    assert kinds["bands"] == {chart.TRAPEZOID} and kinds["text"] == {chart.GLYPH}
    assert kinds["lines"] == {chart.BOX, chart.CAPSULE} and kinds["markers"] == {chart.BOX, chart.CAPSULE}
    layers = np.array(a.layers)
    assert (layers == "background").sum() == 3 and (layers == "bands").sum() == 3 * 3
    assert (a.table[layers == "bands", 1].view(np.uint32) >> 24 == chart.BAND_ALPHA).all()
    # the dashed lines: panels 0 and 1, at x = 3.5, top to bottom of the axes
    dashed = a.table[(a.table[:, 0] == chart.BOX) & (a.table[:, 6] > 0)]
    axes = chart.layout(K.small_figure())
    assert len(dashed) == 2
    for rec, ax in zip(dashed, axes[:2]):
        x = chart.data_to_subpixel(3.5, ax.xlim[0], ax.xlim[1], 16 * ax.x0, 16 * ax.x1)
        assert (rec[2] + rec[4]) // 2 == x and (rec[3], rec[5]) == (16 * ax.y0, 16 * ax.y1)
        assert rec[5] - rec[3] > rec[4] - rec[2]          # the dash runs along y
    with pytest.raises(ValueError, match="coordinate"):
        chart.check_table(np.array([chart.box(0, 0, 40000, 5, (0, 0, 0))], dtype=np.int32))
    with pytest.raises(ValueError, match="int32"):
        chart.check_table(np.zeros((2, 12), dtype=np.int64))


GLYPH_A = ["01110", "10001", "10001", "10001", "11111", "10001", "10001"]
GLYPH_7 = ["11111", "00001", "00010", "00100", "01000", "01000", "01000"]
GLYPH_PERCENT = ["11000", "11001", "00010", "00100", "01000", "10011", "00011"]


def test_builtin_font():
    from rfn_hip import lib, ops
    assert lib.SIGNATURES["rfn_chart_render_u8"] == [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_long,
                                                                                               ctypes.c_void_p]
    assert lib.SIGNATURES["rfn_chart_font"] == [ctypes.c_void_p] and lib.SIGNATURES["rfn_chart_chunk"] == []
    assert ops.chart_chunk() == 256
    font = ops.chart_font()
    assert font.shape == (95, 5) and font.min() >= 0 and font.max() < 128       # seven rows
    rows = lambda ch: ["".join("1" if (font[ord(ch) - 32, c] >> r) & 1 else "0" for c in range(5)) for r in range(7)]
    assert rows("A") == GLYPH_A and rows("7") == GLYPH_7 and rows("%") == GLYPH_PERCENT
    assert not font[0].any() and all(font[i].any() for i in range(1, 95))        # only the space is empty
    assert len({tuple(g) for g in font.tolist()}) == 95                          # all different
    # argument checks of the entry point: nothing is launched
    L = lib.load()
    assert L.rfn_chart_render_u8(None, 0, 0, 4, 0, 0, 256, None) == -1
    assert L.rfn_chart_render_u8(None, 0, 4, 2049, 0, 0, 256, None) == -1
    assert L.rfn_chart_render_u8(None, 1, 4, 4, 0, 0, 256, None) == -2
    assert L.rfn_chart_render_u8(8, 1, 4, 4, 0, 0, 256, None) == -3              # the table is 16-byte aligned
    assert L.rfn_chart_render_u8(None, 0, 4, 4, 1 << 24, 0, 256, None) == -4
    assert L.rfn_chart_render_u8(None, 0, 4, 4, 0, 2, 256, None) == -4
    assert L.rfn_chart_render_u8(None, 0, 4, 4, 0, 0, 0, None) == -5


def test_render_chart_argument_errors_without_a_gpu():
    from rfn_hip import chart, ops
    tab = K.table(K.primitive_cases()["glyphs"])
    with pytest.raises(TypeError, match="canvas size"):
        ops.render_chart(tab)
    with pytest.raises(ValueError, match="at most 2048"):
        ops.render_chart(tab, 2049, 10)
    with pytest.raises(ValueError, match="int32"):
        ops.render_chart(tab.astype(np.int64), 10, 10)
    with pytest.raises(ValueError, match="int32"):
        ops.render_chart(torch.zeros(3, 11, dtype=torch.int32), 10, 10)
    with pytest.raises(TypeError, match="Figure"):
        ops.render_chart([[0] * 12], 10, 10)
    with pytest.raises(ValueError, match="bg"):
        ops.render_chart(tab, 10, 10, bg=(0, 0, 256))
    with pytest.raises(ValueError, match="out must be"):
        ops.render_chart(tab, 10, 10, out=torch.zeros(10, 10, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="324"):
        ops.render_chart(K.small_figure(), 120, 300)
    bad = tab.copy()
    bad[0, 2] = 40000
    with pytest.raises(ValueError, match="coordinate"):
        ops.render_chart(bad, 10, 10)
    with pytest.raises(ValueError, match="canvas"):
        chart.Figure([chart.Panel()], width=4000)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.render_chart(tab, 10, 10)


class _Recorder(object):
    """stands in for ops.render_chart: keeps the figures, returns blank scanlines"""

    def __init__(self):
        self.figures = []

    def __call__(self, fig, scanlines=False):
        assert scanlines
        self.figures.append(fig)
        return np.zeros((fig.height, 1 + 3 * fig.width), dtype=np.uint8)


def _evaluator(**settings):
    from evaluation_metrics import Evaluator
    return Evaluator(Namespace(model=None, args=Namespace(), device=torch.device("cpu")), settings=Namespace(**settings))


def test_plot_eval_values_on_synthetic_files(tmp_path, monkeypatch):
    from rfn_hip import chart, ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "render_chart", rec)
    root, dicts = K.write_experiments(tmp_path, ["a", "b"])
    state = torch.get_rng_state()
    paths = _evaluator(n_conditions=2, n_trained=5).plot_eval_values(root, ["first", "second"], ["a", "b"])
    assert torch.equal(torch.get_rng_state(), state)
    names = ["eval_plots_max.png", "eval_plots_max_median.png", "eval_plots_mean_mean.png"]
    assert paths == [root + "b/eval_folder/" + n for n in names]           # the LAST experiment's folder
    assert sorted(f for f in os.listdir(root + "b/eval_folder") if f.endswith(".png")) == sorted(names)
    assert os.listdir(root + "a/eval_folder") == ["evaluations.pt"]
    assert len(rec.figures) == 3 and all((f.width, f.height, len(f.panels)) == (1900, 500, 3) for f in rec.figures)
    assert [p.title for p in rec.figures[0].panels] == ["Max. SSIM with 95% CI", "Max. PSNR with 95% CI",
                                                        "Min. LPIPS with 95% CI"]
    assert [p.title for p in rec.figures[1].panels] == ["Max. SSIM with 95% quantiles", "Max. PSNR with 95% quantiles",
                                                        "Min. LPIPS with 95% quantiles"]
    assert [p.title for p in rec.figures[2].panels] == ["Avg. SSIM", "Avg. PSNR", "Avg. LPIPS"]
    for f, fig in enumerate(rec.figures):
        assert [p.ylabel for p in fig.panels] == ["score", "", ""] and all(p.xlabel == "t" for p in fig.panels)
        for panel, key in zip(fig.panels, ("SSIM", "PSNR", "LPIPS")):
            assert panel.vline == 5 and panel.grid and len(panel.series) == 2
            for i, s in enumerate(panel.series):
                assert np.array_equal(s.x, 2 + np.arange(6))               # also in the median-LPIPS panel
                assert s.color == chart.TAB10[i] and s.label == ("first", "second")[i]
                v = dicts[i][key + ("_std_mean" if f == 2 else "_values")].numpy().astype(np.float64)
                if f == 0:
                    ci = 1.96 * np.std(v, 0) / np.sqrt(7)
                    assert s.marker == "ov"[i] and np.array_equal(s.y, v.mean(0))
                    assert np.array_equal(s.band[0], v.mean(0) - ci) and np.array_equal(s.band[1], v.mean(0) + ci)
                elif f == 1:
                    assert s.marker == "ov"[i] and np.array_equal(s.y, np.median(v, 0))
                    assert np.array_equal(s.band[0], np.quantile(v, 0.025, axis=0))
                    assert np.array_equal(s.band[1], np.quantile(v, 0.975, axis=0))
                else:
                    assert s.marker is None and s.band is None and np.array_equal(s.y, v.mean(0))
                    assert np.array_equal(s.yerr, 1.96 * np.std(v, 0) / np.sqrt(7))
    # the display list of the real figure: one dashed line per panel at n_trained, legend text under the panels
    dl = chart.build_display_list(rec.figures[0])
    dashed = dl.table[(dl.table[:, 0] == chart.BOX) & (dl.table[:, 6] > 0)]
    assert len(dashed) == 3
    for r, ax in zip(dashed, chart.layout(rec.figures[0])):
        assert (r[2] + r[4]) // 2 == ax.subpixel(5, 0)[0]
    with pytest.raises(ValueError, match="labels"):
        _evaluator(n_conditions=2, n_trained=5).plot_eval_values(root, ["one"], ["a", "b"])


def test_lpips_panel_without_weights(tmp_path, monkeypatch):
    from evaluation_metrics.curves import NO_LPIPS
    from rfn_hip import chart, ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "render_chart", rec)
    root, _ = K.write_experiments(tmp_path, ["a"], lpips=False)
    _evaluator(n_conditions=2, n_trained=5).plot_eval_values(root, ["first"], ["a"])
    assert NO_LPIPS == "no LPIPS weights"
    for fig, title in zip(rec.figures, ("Min. LPIPS with 95% CI", "Min. LPIPS with 95% quantiles", "Avg. LPIPS")):
        assert len(fig.panels[0].series) == 1 and len(fig.panels[1].series) == 1
        assert fig.panels[2].series == [] and fig.panels[2].message == NO_LPIPS and fig.panels[2].title == title
        dl = chart.build_display_list(fig)
        text = "".join(chr(c) for c in dl.table[dl.table[:, 0] == chart.GLYPH, 4])
        assert NO_LPIPS.replace(" ", "") in text and title.replace(" ", "") in text


def test_test_temp_values_on_synthetic_files(tmp_path, monkeypatch):
    from evaluation_metrics import eval_settings as E
    from rfn_hip import chart, ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "render_chart", rec)
    temps = [0.3, 0.7, 1.0]
    for name in ("x", "y"):
        os.makedirs(str(tmp_path / name / "eval_folder"))
    for k, T in enumerate(temps):
        torch.save(K.eval_dict(50 + k, temperature=T), str(tmp_path / "x" / "eval_folder" / E.temperature_file_name(T)))
    state = torch.get_rng_state()
    ev = _evaluator(n_conditions=3, n_trained=6, temperatures=temps)
    paths = ev.test_temp_values(str(tmp_path) + "/", ["unused"], ["x", "y"])
    assert torch.equal(torch.get_rng_state(), state)
    assert paths == [str(tmp_path) + "/x/eval_folder/" + n for n in                     # experiment 0's folder
                     ("eval_plots_max_temp.png", "eval_plots_max_median_temp.png", "eval_plots_mean_mean_temp.png")]
    assert all(os.path.isfile(p) for p in paths) and os.listdir(str(tmp_path / "y" / "eval_folder")) == []
    for fig in rec.figures:
        for panel in fig.panels:
            assert panel.vline == 6 and [s.label for s in panel.series] == ["T= 0.3", "T= 0.7", "T= 1.0"]
            assert all(np.array_equal(s.x, 3 + np.arange(6)) for s in panel.series)
    assert [s.marker for s in rec.figures[0].panels[0].series] == ["o", "v", "x"]
    assert [s.color for s in rec.figures[0].panels[0].series] == list(chart.TAB10[:3])
    with pytest.raises(ValueError, match="temperatures"):
        _evaluator(n_conditions=3, n_trained=6).test_temp_values(str(tmp_path) + "/", [], ["x"])


def test_driver_skips_the_figures_when_files_are_absent(tmp_path, capsys, monkeypatch):
    from evaluation_metrics import eval_settings as E
    from rfn_hip import ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "render_chart", rec)
    root, _ = K.write_experiments(tmp_path, ["a"])
    os.makedirs(str(tmp_path / "b" / "eval_folder"))
    ev = _evaluator(n_conditions=5, n_trained=10, temperatures=[0.5, 1.0])
    base = ["--folder_path", root, "--model_path", "rfn.pt", "rfn.pt", "--temperatures", "0.5", "1.0"]
    capsys.readouterr()
    # b/eval_folder/evaluations.pt does not exist (--no-calc_eval): one line, nothing drawn
    assert E.draw_curve_figures(E.parse_args(base + ["--experiment_names", "a", "b"]), ev) == []
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "are not drawn" in out and "b/eval_folder/evaluations.pt" in out
    assert E.draw_curve_figures(E.parse_args(base + ["--experiment_names", "a", "--test_temperature"]), ev) == []
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "are not drawn" in out and "t05evaluations.pt" in out
    assert rec.figures == [] and not [f for f in os.listdir(root + "a/eval_folder") if f.endswith(".png")]
    # with the file there: drawn, labelled with the experiment names when the labels run short
    paths = E.draw_curve_figures(E.parse_args(base + ["--experiment_names", "a"]), ev)
    assert len(paths) == 3 and rec.figures[0].panels[0].series[0].label == "RFN-BAIR"
    torch.save(K.eval_dict(9), str(tmp_path / "b" / "eval_folder" / "evaluations.pt"))
    E.draw_curve_figures(E.parse_args(base + ["--experiment_names", "a", "b"]), ev)
    assert [s.label for s in rec.figures[-1].panels[0].series] == ["a", "b"]          # one default label, two runs
