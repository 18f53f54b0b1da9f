"""The curve figures of the evaluation: the statistics the reference plots in Evaluator.plot_eval_values and
Evaluator.test_temp_values (evaluation_metrics/error_metrics.py:600-1003) and the three figures built from them as
rfn_hip.chart.Figure objects.  Host code: the inputs are CPU tensors read from evaluations.pt files (a few hundred
sequences by a few dozen frames), like the Frechet distance this stays in float64 numpy."""
import numpy as np

from rfn_hip import chart

FIGURE_NAMES = ("eval_plots_max", "eval_plots_max_median", "eval_plots_mean_mean")
NO_LPIPS = "no LPIPS weights"


def curve_statistics(values):
    """values [N, T] (sequences x predicted frames) -> dict of five [T] float64 vectors, the reference's expressions
    (error_metrics.py:836-864): mean = values.mean(0); ci = 1.96 * np.std(values, 0) / sqrt(N) (ddof = 0); median =
    np.median(values, 0); q_lo, q_hi = np.quantile(values, 0.025 / 0.975, axis=0) (alpha = 0.05, linear
    interpolation)."""
    if hasattr(values, "detach"):
        values = values.detach().cpu().numpy()
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 2 or v.shape[0] < 1:
        raise ValueError("curve_statistics: need values [N >= 1, T], got %s" % (v.shape,))
    alpha = 0.05
    with np.errstate(invalid="ignore"):   # an infinite PSNR (a perfect frame) gives NaN statistics, which are not drawn
        return {"mean": v.mean(0), "ci": 1.96 * np.std(v, 0) / np.sqrt(v.shape[0]), "median": np.median(v, 0),
                "q_lo": np.quantile(v, alpha / 2, axis=0), "q_hi": np.quantile(v, 1 - alpha / 2, axis=0)}


def build_figures(entries, n_conditions, n_trained, width=1900, height=500, text_scale=2):
    """The reference's three figures as {name of FIGURE_NAMES: chart.Figure}.  entries: [(label, eval_dict)] in
    plotting order, eval_dict with the keys of evaluations.pt; entry i takes colour i of matplotlib's cycle and marker
    i of the reference's list.  Each figure has the panels SSIM, PSNR, LPIPS over x = n_conditions + arange(T):
      eval_plots_max         mean of the best-of-N values with the band mean -+ ci, markers
      eval_plots_max_median  their median with the band q_lo .. q_hi, markers
      eval_plots_mean_mean   mean of the mean-over-draws values with error bars -+ ci, no markers
    a dashed line at n_trained, a grid, the legend under the panels.  If any entry's LPIPS values are None the LPIPS
    panel of every figure shows its title and NO_LPIPS instead."""
    if len(entries) > len(chart.MARKERS):
        raise ValueError("build_figures: %d curves, the reference's marker list has %d" %
                         (len(entries), len(chart.MARKERS)))
    titles = {"eval_plots_max": "%s with 95%% CI", "eval_plots_max_median": "%s with 95%% quantiles",
              "eval_plots_mean_mean": "%s"}
    metrics = (("SSIM", "Max. SSIM", "Avg. SSIM"), ("PSNR", "Max. PSNR", "Avg. PSNR"), ("LPIPS", "Min. LPIPS", "Avg. LPIPS"))
    figures = {}
    for name in FIGURE_NAMES:
        panels = []
        for j, (key, best, avg) in enumerate(metrics):
            mean_mean = name == "eval_plots_mean_mean"
            src = key + ("_std_mean" if mean_mean else "_values")
            title = titles[name] % (avg if mean_mean else best)
            ylabel = "score" if j == 0 else ""
            if any(d.get(src) is None for _, d in entries):
                panels.append(chart.Panel(title=title, xlabel="t", ylabel=ylabel, message=NO_LPIPS))
                continue
            series = []
            for i, (label, d) in enumerate(entries):
                s = curve_statistics(d[src])
                x = n_conditions + np.arange(s["mean"].shape[0])
                colour, mark = chart.TAB10[i % len(chart.TAB10)], chart.MARKERS[i]
                if name == "eval_plots_max":
                    series.append(chart.Series(x, s["mean"], colour, marker=mark, label=label,
                                               band=(s["mean"] - s["ci"], s["mean"] + s["ci"])))
                elif name == "eval_plots_max_median":
                    series.append(chart.Series(x, s["median"], colour, marker=mark, label=label,
                                               band=(s["q_lo"], s["q_hi"])))
                else:
                    series.append(chart.Series(x, s["mean"], colour, yerr=s["ci"], label=label))
            panels.append(chart.Panel(title=title, xlabel="t", ylabel=ylabel, series=series, vline=n_trained))
        figures[name] = chart.Figure(panels, width=width, height=height, text_scale=text_scale)
    return figures
