"""Line charts as display lists for rfn_chart_render_u8 (csrc/chart.hip): what the reference draws with matplotlib in
Evaluator.plot_eval_values / test_temp_values (evaluation_metrics/error_metrics.py:600-1003) -- panels side by side,
per panel a title, axis labels, a grid, series with a line, a marker, a fill_between band or error bars, a dashed
vertical line, and one legend row under the panels -- and, for the figures of plot_elbo_gap / plot_prob_of_t /
param_plots (:189-270, :1069-1218), bar series, several coloured vertical lines, fixed axis limits and x ticks, panels
stacked in rows, a reserved band at the top of the canvas and free text.  Pure host code (numpy, no GPU, no
matplotlib, no font files):
`build_display_list(figure)` turns a Figure into the int32 table the kernel paints; rfn_hip.ops.render_chart runs it.
DESIGN.md section 25 holds the pixel contract, the tick rule and the data-to-pixel mapping stated here.

Units: the kernel's geometry is in 1/16 pixel (SUB = 16), x to the right, y down.  The layout below is in whole pixels
and a function of (width, height, the grid of panels, the reserved top band, text_scale) alone."""
import math

import numpy as np

SUB = 16                      # sub-pixel units per pixel
REC = 12                      # int32 per record: type, rgba, p0 .. p9
BOX, CAPSULE, TRAPEZOID, TRIANGLE, GLYPH = range(5)
COORD_MIN, COORD_MAX = -4096, 36864   # every coordinate of a record, 1/16 pixel (the 2048-pixel canvas + 256 around it)
LENGTH_MAX = 4096                     # capsule half-widths
MAX_SIDE = 2048
MAX_GLYPH_SCALE = 128
LAYERS = ("background", "grid", "bands", "lines", "markers", "frame", "text")   # the drawing order

# matplotlib's default colour cycle (tab10)
TAB10 = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75),
         (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207))
# the reference's marker order (error_metrics.py:609, :822); "1", "2", "3" only for the temperatures
MARKERS = ("o", "v", "x", "*", "^", "s", "H", "P", "X", "1", "2", "3")
BLACK, WHITE, GRID_GREY = (0, 0, 0), (255, 255, 255), (176, 176, 176)
BAND_ALPHA = 51               # the reference's alpha_CI = 0.2 of 255


class Series(object):
    """One curve: x, y (equal lengths), an RGB colour, an optional marker of MARKERS, the line on or off, an optional
    band (lo, hi) drawn translucent, optional error bars yerr (stems y - yerr .. y + yerr), a legend label.  Points with
    a non-finite coordinate are left out (a line or band piece needs both its ends).  bar = (width, offset) in data
    units: every finite point also draws a box from the baseline 0 to y over [x + offset - width / 2,
    x + offset + width / 2], clipped to the axes."""

    def __init__(self, x, y, color, marker=None, line=True, band=None, yerr=None, label=None, bar=None):
        self.x, self.y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if self.x.ndim != 1 or self.x.shape != self.y.shape:
            raise ValueError("Series: x and y must be vectors of one length, got %s and %s" % (self.x.shape, self.y.shape))
        if marker is not None and marker not in MARKERS:
            raise ValueError("Series: marker %r is not one of %s" % (marker, " ".join(MARKERS)))
        self.color, self.marker, self.line, self.label = tuple(int(c) for c in color), marker, bool(line), label
        self.band = None if band is None else tuple(np.asarray(b, dtype=np.float64) for b in band)
        self.yerr = None if yerr is None else np.asarray(yerr, dtype=np.float64)
        self.bar = None if bar is None else (float(bar[0]), float(bar[1]))
        if self.bar is not None and not (math.isfinite(self.bar[0]) and self.bar[0] > 0 and math.isfinite(self.bar[1])):
            raise ValueError("Series: bar needs a positive width and a finite offset, got %r" % (bar,))
        for name, a in (("band", self.band or ()), ("yerr", () if self.yerr is None else (self.yerr,))):
            for b in a:
                if b.shape != self.y.shape:
                    raise ValueError("Series: %s must have y's shape %s, got %s" % (name, self.y.shape, b.shape))


class Panel(object):
    """One set of axes: title, xlabel, ylabel, series, an optional dashed vertical line at x = vline, the grid on or
    off, integer_x (whole-number ticks on the x axis: the frame index) and `message`, a text shown in the middle of the
    axes (a panel without data).  vlines: further dashed vertical lines [(x, (r, g, b)), ...], each in its own
    colour; a line outside the x range is not drawn.  xlim / ylim: a fixed (lo, hi) in place of the autoscaled range.
    xticks: explicit x tick values in place of the tick rule's (those outside the x range are left out)."""

    def __init__(self, title="", xlabel="", ylabel="", series=(), vline=None, grid=True, integer_x=True, message=None,
                 vlines=(), xlim=None, ylim=None, xticks=None):
        self.title, self.xlabel, self.ylabel, self.series = str(title), str(xlabel), str(ylabel), list(series)
        self.vline, self.grid, self.integer_x, self.message = vline, bool(grid), bool(integer_x), message
        self.vlines = [(float(x), tuple(int(c) for c in color)) for x, color in vlines]
        self.xlim, self.ylim = (None if lim is None else (float(lim[0]), float(lim[1])) for lim in (xlim, ylim))
        for nm, lim in (("xlim", self.xlim), ("ylim", self.ylim)):
            if lim is not None and not (math.isfinite(lim[0]) and math.isfinite(lim[1]) and lim[0] < lim[1]):
                raise ValueError("Panel: %s must be finite with lo < hi, got %r" % (nm, lim))
        self.xticks = None if xticks is None else [float(v) for v in xticks]


class Figure(object):
    """Panels side by side on a width x height canvas; text_scale u is the pixels per font dot of tick labels and legend
    (titles and axis labels use u + u // 2); the legend row lists the labelled series of `legend_panel`.  rows: the
    panels fill a grid of `rows` rows in row-major order (their number is a multiple of rows), every row with its own
    legend row, listing the row's panel in column `legend_panel`.  top: that many pixel rows at the top of the canvas
    are reserved -- the grid lies below them and the display list puts nothing there but `texts`.  texts: free text
    [(x, y, string)], the top-left corner in pixels, at scale u."""

    def __init__(self, panels, width=1900, height=500, text_scale=2, legend=True, legend_panel=0, rows=1, top=0,
                 texts=()):
        self.panels, self.width, self.height = list(panels), int(width), int(height)
        self.text_scale, self.legend, self.legend_panel = int(text_scale), bool(legend), int(legend_panel)
        self.rows, self.top = int(rows), int(top)
        self.texts = [(int(x), int(y), str(string)) for x, y, string in texts]
        if not self.panels:
            raise ValueError("Figure: no panels")
        if self.rows < 1 or len(self.panels) % self.rows:
            raise ValueError("Figure: %d panels do not fill %d rows" % (len(self.panels), self.rows))
        if not 0 <= self.top < self.height:
            raise ValueError("Figure: the reserved band of %d rows does not leave a canvas of height %d anything" %
                             (self.top, self.height))
        if not (1 <= self.width <= MAX_SIDE and 1 <= self.height <= MAX_SIDE):
            raise ValueError("Figure: the canvas is at most %d x %d pixels, got %d x %d" %
                             (MAX_SIDE, MAX_SIDE, self.width, self.height))
        if not 1 <= self.text_scale <= 16:
            raise ValueError("Figure: text_scale must be in 1..16, got %d" % self.text_scale)


# ------------------------------------------------------------------------------------------------ ticks and mapping
def nice_ticks(lo, hi, integer=False, max_ticks=8):
    """(ticks, decimals): the multiples of the smallest step m * 10^k, m in (1, 2, 2.5, 5), that puts at most
    `max_ticks` ticks into [lo, hi]; with integer=True only whole steps (1, 2, 5, 10, 20, 25, 50, ...).  Each tick is
    computed as round(n * step, decimals) for whole n, lies in [lo, hi], and the list is strictly increasing.  From the
    step before it holding more than max_ticks follows at least 3 ticks whenever the span is not below 4 steps (always,
    unless integer=True forces a step of 1 on a short span).  lo == hi (or a non-finite end) is widened as autoscale()
    does first.  `decimals` is what format_tick needs to show the step exactly."""
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo >= hi:
        lo, hi = autoscale([lo, hi])
    k = int(math.floor(math.log10((hi - lo) / max_ticks))) - 1
    while True:
        for m, extra in ((1, 0), (2, 0), (2.5, 1), (5, 0)):
            if integer and (k < 0 or (k == 0 and m == 2.5)):
                continue
            decimals = max(0, extra - k)
            step = m * 10.0 ** k
            value = lambda n: round(n * m * 10.0 ** k, decimals) if k < 0 else float(n * m * 10 ** k)
            n0, n1 = int(math.ceil(lo / step)), int(math.floor(hi / step))
            while value(n0) < lo:      # the quotients are rounded: hold the ends exactly
                n0 += 1
            while value(n0 - 1) >= lo:
                n0 -= 1
            while value(n1) > hi:
                n1 -= 1
            while value(n1 + 1) <= hi:
                n1 += 1
            if n1 - n0 + 1 <= max_ticks:
                return [value(n) for n in range(n0, n1 + 1)], decimals
        k += 1


def format_tick(value, decimals):
    """the label of a tick: fixed-point with the axis' `decimals`, "-0" spelt "0" """
    s = "%.*f" % (int(decimals), float(value))
    if float(s) == 0.0:
        s = s.lstrip("-")
    return s


def autoscale(values, margin=0.05):
    """(lo, hi) of an axis: min and max over the finite `values` widened by matplotlib's 5 % of the span on each side;
    a span of zero is widened by 5 % of |value| (0.05 around zero) instead, and no finite value at all gives (0, 1)."""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    if v.size == 0:
        return 0.0, 1.0
    lo, hi = float(v.min()), float(v.max())
    d = (hi - lo) * margin
    if d == 0.0:
        d = abs(lo) * margin or margin
    return lo - d, hi + d


def data_to_subpixel(value, lo, hi, p_lo, p_hi):
    """The data-to-pixel mapping of an axis: data `lo` lands on sub-pixel coordinate p_lo, `hi` on p_hi (1/16 pixel,
    integers; p_hi < p_lo on the y axis, which grows downwards), and in between
        p = p_lo + floor((value - lo) / (hi - lo) * (p_hi - p_lo) + 0.5)
    evaluated in float64.  The pixel that holds the point is (p // 16)."""
    return int(p_lo) + int(math.floor((float(value) - lo) / (hi - lo) * (int(p_hi) - int(p_lo)) + 0.5))


class Axes(object):
    """Where a panel's axes lie (whole pixels, [x0, x1] x [y0, y1], y0 the top) and the data ranges mapped onto them"""

    def __init__(self, x0, y0, x1, y1, xlim, ylim, top=0):
        self.x0, self.y0, self.x1, self.y1, self.xlim, self.ylim = x0, y0, x1, y1, xlim, ylim
        self.top = top   # the first pixel row of the grid row that holds the panel

    def subpixel(self, x, y):
        """(sx, sy) of the data point (x, y) in 1/16 pixel"""
        return (data_to_subpixel(x, self.xlim[0], self.xlim[1], SUB * self.x0, SUB * self.x1),
                data_to_subpixel(y, self.ylim[0], self.ylim[1], SUB * self.y1, SUB * self.y0))


def _metrics(fig):
    u = fig.text_scale
    t = u + u // 2
    return dict(u=u, t=t, pad=4 * u, tick=3 * u, cw=6 * u, ch=7 * u, tcw=6 * t, tch=7 * t, hw=8 * u, r=28 * u)


def layout(fig):
    """[Axes] of the figure's panels.  With u = text_scale, t = u + u // 2, pad = 4u, tick = 3u: panel i owns the
    columns [i * (W // n), (i + 1) * (W // n)); its axes start behind pad + 7t (the y label) + pad + 36u (six tick-label
    characters) + tick + pad and end 18u before the panel's right edge; vertically they run from pad + 7t + pad (the
    title) to H - (tick + pad + 7u + pad + 7t + pad) - (7u + 2 pad) (tick labels, x label, legend row).  The x range
    covers the series' x and the vertical line, the y range their y, bands and error bars, each through autoscale().
    With rows > 1 or a reserved band: n is the number of columns, H the row height (height - top) // rows, and row r
    lies fig.top + r * H lower.  Bars add their x extents and the baseline 0 to the ranges, the coloured vertical
    lines their x; a panel's xlim / ylim replaces the autoscaled range."""
    m = _metrics(fig)
    n = len(fig.panels) // fig.rows
    pw, rh = fig.width // n, (fig.height - fig.top) // fig.rows
    out = []
    for k, panel in enumerate(fig.panels):
        i, top = k % n, fig.top + (k // n) * rh
        y0 = top + m["pad"] + m["tch"] + m["pad"]
        y1 = top + rh - (m["tick"] + m["pad"] + m["ch"] + m["pad"] + m["tch"] + m["pad"]) - (m["ch"] + 2 * m["pad"])
        x0 = i * pw + m["pad"] + m["tch"] + m["pad"] + 6 * m["cw"] + m["tick"] + m["pad"]
        x1 = (i + 1) * pw - 3 * m["cw"]
        xs = [s.x for s in panel.series] + ([[panel.vline]] if panel.vline is not None and panel.series else [])
        if panel.series:
            xs += [[x for x, _ in panel.vlines]]
        ys = []
        for s in panel.series:
            ys.append(s.y)
            if s.bar is not None:
                xs += [s.x + s.bar[1] - s.bar[0] / 2, s.x + s.bar[1] + s.bar[0] / 2]
                ys.append([0.0])
            if s.band is not None:
                ys += list(s.band)
            if s.yerr is not None:
                ys += [s.y - s.yerr, s.y + s.yerr]
        cat = lambda a: np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in a]) if a else np.zeros(0)
        out.append(Axes(x0, y0, max(x1, x0 + 1), max(y1, y0 + 1), panel.xlim or autoscale(cat(xs)),
                        panel.ylim or autoscale(cat(ys)), top))
    return out


# ------------------------------------------------------------------------------------------------ the display list
def rgba(color, alpha=255):
    """r | g<<8 | b<<16 | alpha<<24 as the int32 the table holds"""
    r, g, b = (int(c) for c in color)
    if not all(0 <= c <= 255 for c in (r, g, b, int(alpha))):
        raise ValueError("rgba: channels and alpha are bytes, got %s alpha %s" % ((r, g, b), alpha))
    v = r | g << 8 | b << 16 | int(alpha) << 24
    return v - (1 << 32) if v >= 1 << 31 else v


def box(x0, y0, x1, y1, color, alpha=255, dash=(0, 0)):
    return [BOX, rgba(color, alpha), x0, y0, x1, y1, dash[0], dash[1], 0, 0, 0, 0]


def capsule(ax, ay, bx, by, hw, color, alpha=255):
    return [CAPSULE, rgba(color, alpha), ax, ay, bx, by, hw, 0, 0, 0, 0, 0]


def trapezoid(x0, x1, lo0, lo1, hi0, hi1, color, alpha=255):
    return [TRAPEZOID, rgba(color, alpha), x0, x1, lo0, lo1, hi0, hi1, 0, 0, 0, 0]


def triangle(x0, y0, x1, y1, x2, y2, color, alpha=255):
    return [TRIANGLE, rgba(color, alpha), x0, y0, x1, y1, x2, y2, 0, 0, 0, 0]


def glyph(x, y, char, scale, color, rotated=False, alpha=255):
    return [GLYPH, rgba(color, alpha), x, y, ord(char), scale, 1 if rotated else 0, 0, 0, 0, 0, 0]


def text(x, y, string, scale, color=BLACK, rotated=False):
    """records of a string in pixels: upright from its top-left corner (x, y) to the right, 6 * scale pixels per
    character; rotated (reading upwards) from its bottom-left corner (x, y), 7 * scale pixels wide.  Characters outside
    ASCII 32..126 become '?'."""
    out = []
    for i, ch in enumerate(string):
        ch = ch if 32 <= ord(ch) <= 126 else "?"
        if ch == " ":
            continue
        if rotated:
            out.append(glyph(SUB * x, SUB * (y - i * 6 * scale - 5 * scale), ch, scale, color, True))
        else:
            out.append(glyph(SUB * (x + i * 6 * scale), SUB * y, ch, scale, color))
    return out


def text_width(string, scale):
    return max(0, len(string) * 6 * scale - scale)


def marker(kind, x, y, r, color):
    """records of a marker centred on the sub-pixel point (x, y), r its radius in 1/16 pixel"""
    h, q, e = r // 2, r // 4, r * 7 // 8
    c = lambda ax, ay, bx, by, hw: capsule(x + ax, y + ay, x + bx, y + by, hw, color)
    t = lambda *p: triangle(*[v + (x, y)[k & 1] for k, v in enumerate(p)], color)
    if kind == "o":
        return [c(0, 0, 0, 0, r)]
    if kind == "v":
        return [t(-r, -r, r, -r, 0, r)]
    if kind == "^":
        return [t(-r, r, r, r, 0, -r)]
    if kind == "s":
        return [box(x - r, y - r, x + r, y + r, color)]
    if kind == "x":
        return [c(-r, -r, r, r, q), c(-r, r, r, -r, q)]
    if kind == "X":
        return [c(-e, -e, e, e, h), c(-e, e, e, -e, h)]
    if kind == "*":
        return [c(0, -r, 0, r, q), c(-e, -h, e, h, q), c(-e, h, e, -h, q)]
    if kind == "H":   # a fan over the hexagon's six corners
        v = [(r, 0), (h, e), (-h, e), (-r, 0), (-h, -e), (h, -e)]
        return [t(v[0][0], v[0][1], v[k][0], v[k][1], v[k + 1][0], v[k + 1][1]) for k in range(1, 5)]
    if kind == "P":
        return [box(x - r, y - h, x + r, y + h, color), box(x - h, y - r, x + h, y + r, color)]
    if kind == "1":   # three strokes from the centre: down, up-left, up-right
        return [c(0, 0, 0, r, q), c(0, 0, -e, -h, q), c(0, 0, e, -h, q)]
    if kind == "2":
        return [c(0, 0, 0, -r, q), c(0, 0, -e, h, q), c(0, 0, e, h, q)]
    if kind == "3":
        return [c(0, 0, -r, 0, q), c(0, 0, h, -e, q), c(0, 0, h, e, q)]
    raise ValueError("marker %r is not one of %s" % (kind, " ".join(MARKERS)))


class DisplayList(object):
    """`table`: int32 [n, 12], the records in painting order; `layers`: the LAYERS name of every record; `bg`: the
    canvas colour (r, g, b); width, height in pixels"""

    def __init__(self, table, layers, bg, width, height):
        self.table, self.layers, self.bg, self.width, self.height = table, layers, bg, width, height


def check_table(table):
    """int32 [n, 12] with every coordinate and length inside the kernel's contract (what keeps its products in 64
    bits); returns the table as a contiguous numpy array"""
    t = np.ascontiguousarray(np.asarray(table))
    if t.dtype != np.int32 or t.ndim != 2 or t.shape[1] != REC:
        raise ValueError("chart table: need int32 [n, %d], got %s %s" % (REC, t.dtype, t.shape))
    ncoord = {BOX: 4, CAPSULE: 4, TRAPEZOID: 6, TRIANGLE: 6, GLYPH: 2}
    for ty, k in ncoord.items():
        rows = t[t[:, 0] == ty]
        if rows.size and (rows[:, 2:2 + k].min() < COORD_MIN or rows[:, 2:2 + k].max() > COORD_MAX):
            raise ValueError("chart table: a coordinate of a type-%d record is outside [%d, %d]" %
                             (ty, COORD_MIN, COORD_MAX))
    if ((t[:, 0] < BOX) | (t[:, 0] > GLYPH)).any():
        raise ValueError("chart table: record types are 0..4")
    cap, bx, gl = t[t[:, 0] == CAPSULE], t[t[:, 0] == BOX], t[t[:, 0] == GLYPH]
    if cap.size and (cap[:, 6].min() < 0 or cap[:, 6].max() > LENGTH_MAX):
        raise ValueError("chart table: a capsule half-width is outside [0, %d]" % LENGTH_MAX)
    if bx.size and (bx[:, 6:8].min() < 0 or bx[:, 6:8].max() > COORD_MAX):
        raise ValueError("chart table: dash lengths are in [0, %d]" % COORD_MAX)
    if gl.size and (gl[:, 4].min() < 32 or gl[:, 4].max() > 126 or gl[:, 5].min() < 1 or
                    gl[:, 5].max() > MAX_GLYPH_SCALE or gl[:, 6].min() < 0 or gl[:, 6].max() > 1):
        raise ValueError("chart table: a glyph needs a character 32..126, a scale 1..%d and rotation 0 / 1" %
                         MAX_GLYPH_SCALE)
    return t


def build_display_list(fig):
    """The display list of a Figure.  Records are emitted layer by layer over all panels in the order LAYERS --
    background (the axes' white), grid, bands, lines (with error-bar stems and the dashed vertical line), markers, frame
    (axes and tick marks), text -- bars go with the bands, the coloured vertical lines with the lines, the free text
    comes last -- and inside a layer panel by panel, series by series, point by point: the same
    figure always gives the same table."""
    if not isinstance(fig, Figure):
        raise TypeError("build_display_list: need a chart.Figure, got %s" % type(fig).__name__)
    m = _metrics(fig)
    u, t, pad, tick, hw, r = m["u"], m["t"], m["pad"], m["tick"], m["hw"], m["r"]
    L = {k: [] for k in LAYERS}
    clamp = lambda v: min(max(int(v), COORD_MIN), COORD_MAX)
    lw = max(1, u // 2)   # frame and grid lines, pixels
    for panel, ax in zip(fig.panels, layout(fig)):
        X0, Y0, X1, Y1 = SUB * ax.x0, SUB * ax.y0, SUB * ax.x1, SUB * ax.y1
        L["background"].append(box(X0, Y0, X1, Y1, WHITE))
        sx = lambda v: clamp(data_to_subpixel(v, ax.xlim[0], ax.xlim[1], X0, X1))
        sy = lambda v: clamp(data_to_subpixel(v, ax.ylim[0], ax.ylim[1], Y1, Y0))
        if panel.series:
            xt, xd = nice_ticks(ax.xlim[0], ax.xlim[1], integer=panel.integer_x)
            if panel.xticks is not None:   # explicit ticks: the fewest decimals (at most 6) that show every value
                xt = [v for v in panel.xticks if ax.xlim[0] <= v <= ax.xlim[1]]
                xd = next((d for d in range(6) if all(round(v, d) == v for v in xt)), 6)
            yt, yd = nice_ticks(ax.ylim[0], ax.ylim[1])
        else:
            xt, xd, yt, yd = [], 0, [], 0
        for v in xt:
            p = sx(v)
            if panel.grid:
                L["grid"].append(box(p - 8 * lw, Y0, p + 8 * lw, Y1, GRID_GREY))
            L["frame"].append(box(p - 8 * lw, Y1, p + 8 * lw, Y1 + SUB * tick, BLACK))
            s = format_tick(v, xd)
            L["text"] += text(p // SUB - text_width(s, u) // 2, ax.y1 + tick + pad, s, u)
        for v in yt:
            p = sy(v)
            if panel.grid:
                L["grid"].append(box(X0, p - 8 * lw, X1, p + 8 * lw, GRID_GREY))
            L["frame"].append(box(X0 - SUB * tick, p - 8 * lw, X0, p + 8 * lw, BLACK))
            s = format_tick(v, yd)
            L["text"] += text(ax.x0 - tick - pad // 2 - text_width(s, u), p // SUB - m["ch"] // 2, s, u)
        for s in panel.series:
            ok = np.isfinite(s.x) & np.isfinite(s.y)
            px = [sx(v) if o else 0 for v, o in zip(s.x, ok)]
            py = [sy(v) if o else 0 for v, o in zip(s.y, ok)]
            if s.band is not None:
                bok = ok & np.isfinite(s.band[0]) & np.isfinite(s.band[1])
                # data lo is the lower VALUE: on the canvas (y down) it is the band's far edge
                top = [sy(v) if o else 0 for v, o in zip(s.band[1], bok)]
                bot = [sy(v) if o else 0 for v, o in zip(s.band[0], bok)]
                # the pieces join on whole-pixel columns (x rounded to a multiple of 16): a pixel that two translucent
                # pieces shared would be blended twice and show as a seam
                bx = [(v + SUB // 2) // SUB * SUB for v in px]
                for i in range(len(px) - 1):
                    if bok[i] and bok[i + 1] and bx[i] < bx[i + 1]:
                        L["bands"].append(trapezoid(bx[i], bx[i + 1], top[i], top[i + 1], bot[i], bot[i + 1], s.color,
                                                    BAND_ALPHA))
            if s.bar is not None:   # opaque boxes from the baseline to y, clipped to the axes
                base = sy(0.0)
                for i in range(len(px)):
                    if ok[i]:
                        bx0, bx1 = sx(s.x[i] + s.bar[1] - s.bar[0] / 2), sx(s.x[i] + s.bar[1] + s.bar[0] / 2)
                        bx0, bx1 = max(bx0, X0), min(bx1, X1)
                        by0, by1 = max(min(base, py[i]), Y0), min(max(base, py[i]), Y1)
                        if bx0 < bx1 and by0 < by1:
                            L["bands"].append(box(bx0, by0, bx1, by1, s.color))
            if s.line:
                for i in range(len(px) - 1):
                    if ok[i] and ok[i + 1]:
                        L["lines"].append(capsule(px[i], py[i], px[i + 1], py[i + 1], hw, s.color))
            if s.yerr is not None:
                for i in range(len(px)):
                    if ok[i] and np.isfinite(s.yerr[i]):
                        L["lines"].append(box(px[i] - hw, sy(s.y[i] + s.yerr[i]), px[i] + hw, sy(s.y[i] - s.yerr[i]) + 1,
                                              s.color))
            if s.marker is not None:
                for i in range(len(px)):
                    if ok[i]:
                        L["markers"] += marker(s.marker, px[i], py[i], r, s.color)
        if panel.vline is not None and panel.series:
            p = sx(panel.vline)
            L["lines"].append(box(p - hw, Y0, p + hw, Y1, BLACK, dash=(SUB * 4 * u, SUB * 2 * u)))
        if panel.series:
            for v, colour in panel.vlines:
                if ax.xlim[0] <= v <= ax.xlim[1]:
                    p = sx(v)
                    L["lines"].append(box(p - hw, Y0, p + hw, Y1, colour, dash=(SUB * 4 * u, SUB * 2 * u)))
        for a in (box(X0 - 8 * lw, Y0 - 8 * lw, X1 + 8 * lw, Y0 + 8 * lw, BLACK),
                  box(X0 - 8 * lw, Y1 - 8 * lw, X1 + 8 * lw, Y1 + 8 * lw, BLACK),
                  box(X0 - 8 * lw, Y0, X0 + 8 * lw, Y1, BLACK), box(X1 - 8 * lw, Y0, X1 + 8 * lw, Y1, BLACK)):
            L["frame"].append(a)
        cx = (ax.x0 + ax.x1) // 2
        L["text"] += text(cx - text_width(panel.title, t) // 2, ax.top + pad, panel.title, t)
        L["text"] += text(cx - text_width(panel.xlabel, t) // 2, ax.y1 + tick + pad + m["ch"] + pad, panel.xlabel, t)
        L["text"] += text(ax.x0 - tick - pad - 6 * m["cw"] - pad - m["tch"],
                          (ax.y0 + ax.y1) // 2 + text_width(panel.ylabel, t) // 2, panel.ylabel, t, rotated=True)
        if panel.message:
            L["text"] += text(cx - text_width(panel.message, u) // 2, (ax.y0 + ax.y1) // 2 - m["ch"] // 2,
                              panel.message, u)
    cols, rh = len(fig.panels) // fig.rows, (fig.height - fig.top) // fig.rows
    for row in range(fig.rows if fig.legend and 0 <= fig.legend_panel < cols else 0):
        entries = [s for s in fig.panels[row * cols + fig.legend_panel].series if s.label]
        sample, gap = 24 * u, 2 * m["cw"]
        total = sum(sample + pad + text_width(s.label, u) + gap for s in entries)
        x = fig.width // 10 if fig.width // 10 + total <= fig.width else max(pad, (fig.width - total) // 2)
        y = fig.top + (row + 1) * rh - pad - m["ch"]
        cy = SUB * y + SUB * m["ch"] // 2
        for s in entries:
            if x + sample > fig.width:   # the row is full: the remaining entries would lie off the canvas
                break
            if s.bar is not None:   # a bar series' sample is a filled box
                L["bands"].append(box(SUB * x, SUB * y, SUB * (x + sample), SUB * (y + m["ch"]), s.color))
            if s.line:
                L["lines"].append(capsule(SUB * x, cy, SUB * (x + sample), cy, hw, s.color))
            if s.marker is not None:
                L["markers"] += marker(s.marker, SUB * x + SUB * sample // 2, cy, r, s.color)
            L["text"] += text(x + sample + pad, y, s.label, u)
            x += sample + pad + text_width(s.label, u) + gap
    for x, y, string in fig.texts:
        L["text"] += text(x, y, string, u)
    # a glyph outside the coordinate range lies off the canvas (an over-long title or legend): it is left out
    visible = lambda rec: rec[0] != GLYPH or (COORD_MIN <= rec[2] <= COORD_MAX and COORD_MIN <= rec[3] <= COORD_MAX)
    rows = [rec for k in LAYERS for rec in L[k] if visible(rec)]
    layers = [k for k in LAYERS for rec in L[k] if visible(rec)]
    table = check_table(np.array(rows, dtype=np.int64).reshape(-1, REC).astype(np.int32))
    return DisplayList(table, layers, WHITE, fig.width, fig.height)
