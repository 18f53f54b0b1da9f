"""The curve figures of the evaluation: the statistics the reference plots in Evaluator.plot_eval_values and
Evaluator.test_temp_values (evaluation_metrics/error_metrics.py:600-1003) and the three figures built from them as
rfn_hip.chart.Figure objects.  Host code: the inputs are CPU tensors read from evaluations.pt files (a few hundred
sequences by a few dozen frames), like the Frechet distance this stays in float64 numpy.  Below them: the statistics
and the Figure objects of the three analysis figures -- plot_elbo_gap (:189-247), plot_prob_of_t (:250-270) and
param_plots (:1069-1218)."""
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


# ------------------------------------------------------ the analysis figures (error_metrics.py:189-270, :1069-1218)
PARAM_NAMES = ("mu prior", "sigma prior", "mu posterior", "sigma posterior", "mu base dist", "sigma base dist")
RED, BLUE = (255, 0, 0), (0, 0, 255)
ROW_LABELS = ("GT:", "Prior:", "Posterior:")


def _f64(values):
    if hasattr(values, "detach"):
        values = values.detach().cpu().numpy()
    return np.asarray(values, dtype=np.float64)


def prob_of_t_statistics(probT):
    """probT [N, 2, T] (sequences x (prior, posterior) x frames) -> (mean, ci), two [T] float64 vectors, the reference's
    expressions (:253, :258) on the prior's values v = probT[:, 0, :]: mean = v.mean(0), ci = 1.96 * np.std(v, 0) /
    sqrt(N) (numpy's population standard deviation)."""
    v = _f64(probT)
    if v.ndim != 3 or v.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError("prob_of_t_statistics: need probT [N >= 1, 2, T], got %s" % (v.shape,))
    v = v[:, 0, :]
    return v.mean(0), 1.96 * np.std(v, 0) / np.sqrt(v.shape[0])


def bpp_ylim(bpp):
    """the BPP panel's y range (:233-236): bpp [2, T] (prior, posterior); low and high over the entries t >= 1 of both
    rows, widened by half their distance on each side.  None (autoscale) when that is no range: fewer than two frames,
    a non-finite value or high == low."""
    v = _f64(bpp)
    if v.ndim != 2 or v.shape[0] != 2:
        raise ValueError("bpp_ylim: need bpp [2, T], got %s" % (v.shape,))
    if v.shape[1] < 2:
        return None
    low, high = float(v[:, 1:].min()), float(v[:, 1:].max())
    if not (np.isfinite(low) and np.isfinite(high) and low < high):
        return None
    return low - 0.5 * (high - low), high + 0.5 * (high - low)


def minmax_scale(x):
    """(x - x.min()) / (x.max() - x.min()) (:1065-1067), float64; a constant curve divides by zero as the reference's"""
    x = _f64(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - x.min()) / (x.max() - x.min())


def parameter_curves(sums):
    """the six plotted curves of param_plots (:1125-1144).  sums: per batch the six [T - 1, B] tensors
    (mu_p, std_p, mu_q, std_q, mu_flow, std_flow), each a parameter tensor summed over (C, H, W).  Each curve is the
    mean over batches and sequences (float64), then minmax_scale: six [T - 1] float64 vectors in the order of
    PARAM_NAMES."""
    if not sums:
        raise ValueError("parameter_curves: no batches")
    return [minmax_scale(np.stack([_f64(batch[k]) for batch in sums]).mean(axis=(0, 2))) for k in range(6)]


def elbo_gap_band(n_frames, H, W, text_scale=2, gutter=2):
    """where plot_elbo_gap's sheet of 3 rows x n_frames cells of H x W pixels lies in the figure's reserved band:
    (top, x, y, label_y) -- the band's height, the sheet's top-left pixel and the y of the three row labels.  The
    labels start at x = pad; the sheet starts behind the widest label and a pad on either side of it."""
    u = int(text_scale)
    pad, ch = 4 * u, 7 * u
    x = pad + chart.text_width(max(ROW_LABELS, key=len), u) + pad
    hs = 3 * H + 4 * gutter
    label_y = [pad + gutter + r * (H + gutter) + H // 2 - ch // 2 for r in range(3)]
    return hs + 2 * pad, x, pad, label_y


def elbo_gap_figure(kld, bpp, H, W, text_scale=2, gutter=2):
    """plot_elbo_gap's figure (:200-245) without the frames.  kld [T]: averageKLDseq[:, 0]; bpp [2, T]:
    averageNLLseq[:, :, 0] in bits per pixel.  Canvas 200 T x 972 pixels (the reference's figsize (2 T, 1.62 * 6) at
    100 dpi); the top band of elbo_gap_band(T, H, W) is reserved for the sheet of frames and holds the row labels;
    below it two stacked panels over x = 0 .. T - 1 with x range (-0.5, T - 0.5) and a tick per frame: "Avg. KLD", bars
    of width 0.3, and "BPP", paired bars "Prior" / "Posterior" at x -+ 0.15, width 0.3, y range bpp_ylim(bpp).  Both
    panels carry a legend."""
    kld, bpp = _f64(kld), _f64(bpp)
    T = int(kld.shape[0])
    if kld.ndim != 1 or bpp.shape != (2, T) or T < 1:
        raise ValueError("elbo_gap_figure: need kld [T >= 1] and bpp [2, T], got %s and %s" % (kld.shape, bpp.shape))
    top, x, _, label_y = elbo_gap_band(T, H, W, text_scale, gutter)
    width, height = 200 * T, 972
    if x + T * W + (T + 1) * gutter > width or top + 200 > height:
        raise ValueError("elbo_gap_figure: %d frames of %dx%d pixels do not fit the %dx%d canvas" %
                         (T, H, W, width, height))
    t = np.arange(T)
    xlim, ticks = (-0.5, T - 0.5), list(range(T))
    blue, orange = chart.TAB10[0], chart.TAB10[1]
    panels = [chart.Panel(ylabel="Avg. KLD", xlim=xlim, xticks=ticks, grid=False,
                          series=[chart.Series(t, kld, blue, line=False, bar=(0.3, 0.0), label="Avg. KLD")]),
              chart.Panel(xlabel="t", ylabel="BPP", xlim=xlim, xticks=ticks, ylim=bpp_ylim(bpp), grid=False,
                          series=[chart.Series(t, bpp[0], blue, line=False, bar=(0.3, -0.15), label="Prior"),
                                  chart.Series(t, bpp[1], orange, line=False, bar=(0.3, 0.15), label="Posterior")])]
    pad = 4 * int(text_scale)
    return chart.Figure(panels, width=width, height=height, text_scale=text_scale, rows=2, top=top,
                        texts=[(pad, y, s) for y, s in zip(label_y, ROW_LABELS)])


def prob_of_t_figure(probT, n_conditions, text_scale=2):
    """plot_prob_of_t's figure (:250-270): the mean of prob_of_t_statistics against x = n_conditions + arange(T) with
    the band mean -+ ci, a grid, the title "P(X_n = X_t | X_<n)" and the axis labels "Bits per pixel" / "Frame number";
    640 x 480 pixels (matplotlib's default figsize at 100 dpi), no legend."""
    mean, ci = prob_of_t_statistics(probT)
    n = int(n_conditions)
    x = n + np.arange(mean.shape[0])
    series = [chart.Series(x, mean, chart.TAB10[0], band=(mean - ci, mean + ci), label="Prior")]
    panel = chart.Panel(title="P(X_%d = X_t | X_<%d)" % (n, n), xlabel="Frame number", ylabel="Bits per pixel",
                        series=series)
    return chart.Figure([panel], width=640, height=480, text_scale=text_scale, legend=False)


def param_figure(curves, hit_boundary, text_scale=2):
    """param_plots' figure (:1165-1217): two stacked panels, "Average" against t = 1 .. T - 1 with x range (1, T - 1);
    the upper one the prior's, the posterior's and the base distribution's mean, the lower one their sigmas (curves in
    the order of PARAM_NAMES), each panel with its legend; a red dashed line at every k + 1 with hit_boundary[k] == 1
    and a blue one at every k + 1 with hit_boundary[k] == 2.  1000 x 800 pixels (figsize (10, 8) at 100 dpi)."""
    curves = [_f64(c) for c in curves]
    if len(curves) != 6 or any(c.ndim != 1 or c.shape != curves[0].shape for c in curves) or curves[0].shape[0] < 2:
        raise ValueError("param_figure: need six curves of one length >= 2")
    hit = _f64(hit_boundary)
    n = curves[0].shape[0]
    x = np.arange(1, n + 1)
    vlines = [(k + 1, RED) for k in np.where(hit == 1)[0]] + [(k + 1, BLUE) for k in np.where(hit == 2)[0]]
    panels = []
    for first in (0, 1):
        series = [chart.Series(x, curves[k], chart.TAB10[j], label=PARAM_NAMES[k])
                  for j, k in enumerate(range(first, 6, 2))]
        panels.append(chart.Panel(xlabel="t", ylabel="Average", series=series, vlines=vlines, xlim=(1, n), grid=False))
    return chart.Figure(panels, width=1000, height=800, text_scale=text_scale, rows=2)
