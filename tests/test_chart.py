"""GPU tests of the chart rasteriser (rfn_hip.ops.render_chart -> rfn_chart_render_u8, csrc/chart.hip): every comparison
is byte for byte against tests/chart_ref.py, the int64 numpy restatement of the pixel contract of DESIGN.md section 25.
Each primitive type alone at awkward sub-pixel positions, off and outside the canvas; order and translucency; more
records than one chunk; tiny canvases at every byte alignment with guard bytes; a small whole figure; the data-to-pixel
mapping read back from the picture; Evaluator.plot_eval_values end to end."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import chart_cases as K
from tests import chart_ref as R
from tests.test_sheet_host import decode_png

pytestmark = pytest.mark.gpu

BG = (250, 240, 230)


@pytest.fixture(scope="module")
def font():
    from rfn_hip import ops
    return ops.chart_font()


def _both(records, font, H=K.H, W=K.W, bg=BG):
    """(kernel, reference) pixels [H, W, 3] of a list of records"""
    from rfn_hip import ops
    tab = K.table(records)
    return ops.render_chart(tab, H, W, bg=bg).cpu().numpy(), R.render(tab, H, W, font, bg)


@pytest.mark.parametrize("name", sorted(K.primitive_cases()))
def test_each_primitive_alone(name, font):
    got, want = _both(K.primitive_cases()[name], font)
    assert np.array_equal(got, want), name
    painted = (want != np.array(BG, dtype=np.uint8)).any()
    assert painted == (name not in ("outside", "trapezoid_lo_above_hi", "triangle_degenerate")), name


def test_capsule_case_reaches_all_three_branches():
    """the case named so has samples on the canvas beyond a, beyond b and beside the segment"""
    ax, ay, bx, by, _ = K.primitive_cases()["capsule_three_branches"][0][2:7]
    s = 16 * np.arange(max(K.W, K.H))[:, None] + R.OFFSETS[None, :]
    sx, sy = np.meshgrid(s.reshape(-1)[:4 * K.W], s.reshape(-1)[:4 * K.H])
    dot = (sx - ax) * (bx - ax) + (sy - ay) * (by - ay)
    dd = (bx - ax) ** 2 + (by - ay) ** 2
    assert (dot <= 0).any() and (dot >= dd).any() and ((dot > 0) & (dot < dd)).any()


def test_order_and_translucency(font):
    a, b = K.C.box(50, 40, 400, 300, K.RED, 128), K.C.box(200, 100, 600, 350, K.BLUE, 128)
    ab, ab_ref = _both([a, b], font)
    ba, ba_ref = _both([b, a], font)
    assert np.array_equal(ab, ab_ref) and np.array_equal(ba, ba_ref)
    assert not np.array_equal(ab, ba)
    # two adjoining half-alpha band pieces on one pair of lines, joined on a pixel boundary (x = 13 * 16) as
    # build_display_list joins them: the picture of the one piece spanning both, no seam column
    left = K.C.trapezoid(40, 208, 50, 92, 300, 258, K.GREEN, 128)
    right = K.C.trapezoid(208, 360, 92, 130, 258, 220, K.GREEN, 128)
    whole = K.C.trapezoid(40, 360, 50, 130, 300, 220, K.GREEN, 128)
    two, two_ref = _both([left, right], font)
    one, _ = _both([whole], font)
    assert np.array_equal(two, two_ref) and np.array_equal(two, one)
    seam = two[8, 11:15].astype(int)          # the pixels around x = 208 / 16 on a line inside the band
    assert (seam == seam[0]).all() and tuple(seam[0]) != BG
    # joined inside a pixel (x = 200) the half-open test still gives every sample to exactly one piece
    left, right = K.C.trapezoid(40, 200, 50, 90, 300, 260, K.GREEN, 128), K.C.trapezoid(200, 360, 90, 130, 260, 220, K.GREEN, 128)
    cover = lambda rec: R.coverage(rec[0], rec[2:], 0, K.H, 0, K.W, font)
    assert np.array_equal(cover(left) + cover(right), cover(whole))
    two, two_ref = _both([left, right], font)
    assert np.array_equal(two, two_ref)


@pytest.mark.parametrize("spread", [False, True])
def test_more_records_than_one_chunk(spread, font):
    from rfn_hip import ops
    records = K.order_dependent(ops.chart_chunk() + 37, spread)
    got, want = _both(records, font)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, R.render(K.table(records[::-1]), K.H, K.W, font, BG))   # the order matters


def test_tiny_canvases_alignment_and_guards(font):
    from rfn_hip import ops
    records = K.primitive_cases()["off_left"] + K.primitive_cases()["off_top"] + [K.C.box(0, 0, 16, 16, K.RED, 200)]
    tab = K.table(records)
    dev_tab = torch.from_numpy(tab).cuda()
    for H, W in ((1, 1), (17, 5), (33, 31)):
        for lead in (0, 1):
            want = R.render(tab, H, W, font, BG, lead)
            shape = (H, 1 + 3 * W) if lead else (H, W, 3)
            for offset in range(4):
                buf = torch.full((want.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                out = buf[16 + offset:16 + offset + want.size].view(shape)
                assert out.data_ptr() % 4 == offset
                ret = ops.render_chart(dev_tab, H, W, scanlines=bool(lead), out=out, bg=BG)
                assert ret is out
                host = buf.cpu().numpy()
                assert np.array_equal(host[16 + offset:16 + offset + want.size].reshape(shape), want), (H, W, lead, offset)
                assert (host[:16 + offset] == 0xA5).all() and (host[16 + offset + want.size:] == 0xA5).all()


def test_small_whole_figure_and_the_data_mapping(font):
    from rfn_hip import chart, ops
    fig = K.small_figure()
    dl = chart.build_display_list(fig)
    got = ops.render_chart(fig).cpu().numpy()
    assert got.shape == (fig.height, fig.width, 3)
    assert np.array_equal(got, R.render(dl.table, dl.height, dl.width, font, dl.bg))
    assert np.array_equal(ops.render_chart(dl, scanlines=True).cpu().numpy(),
                          R.render(dl.table, dl.height, dl.width, font, dl.bg, lead=1))
    # reference and kernel share the display list; what ties the picture to the DATA is this: the pixel that
    # data_to_subpixel names for a data point carries the point's series colour (its marker covers that pixel whole)
    for i in (0, 2):
        ax = chart.layout(fig)[i]
        for s in fig.panels[i].series:
            for x, y in zip(s.x, s.y):
                sx = chart.data_to_subpixel(x, ax.xlim[0], ax.xlim[1], 16 * ax.x0, 16 * ax.x1)
                sy = chart.data_to_subpixel(y, ax.ylim[0], ax.ylim[1], 16 * ax.y1, 16 * ax.y0)
                assert (sx, sy) == ax.subpixel(x, y)
                assert ax.x0 <= sx // 16 <= ax.x1 and ax.y0 <= sy // 16 <= ax.y1
                assert tuple(got[sy // 16, sx // 16]) == s.color, (i, x, y)


def test_plot_eval_values_end_to_end(tmp_path, font):
    from evaluation_metrics import Evaluator
    from evaluation_metrics.curves import FIGURE_NAMES, build_figures
    from rfn_hip import ops
    root, dicts = K.write_experiments(tmp_path, ["a", "b"])
    ev = Evaluator(Namespace(model=None, args=Namespace(), device=torch.device("cuda")),
                   settings=Namespace(n_conditions=2, n_trained=5))
    paths = ev.plot_eval_values(root, ["first", "second"], ["a", "b"])
    assert paths == [root + "b/eval_folder/" + n + ".png" for n in FIGURE_NAMES]
    figures = build_figures([("first", dicts[0]), ("second", dicts[1])], 2, 5)
    for path, name in zip(paths, FIGURE_NAMES):
        (w, h), px = decode_png(open(path, "rb").read())
        assert (w, h) == (1900, 500)
        assert np.array_equal(px, ops.render_chart(figures[name]).cpu().numpy()), name
        assert (px != 255).any()
