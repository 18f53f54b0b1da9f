"""Inputs shared by tests/test_chart.py and tests/test_chart_host.py: display-list tables at awkward sub-pixel
positions on a 40 x 24 canvas (640 x 384 in 1/16 pixel), a small whole figure, and synthetic evaluations.pt files."""
import os

import numpy as np
import torch

from rfn_hip import chart as C

W, H = 40, 24
RED, GREEN, BLUE, INK = (200, 30, 40), (20, 160, 60), (30, 60, 220), (10, 20, 30)


def primitive_cases():
    """name -> list of records"""
    cases = {
        "capsule_zero_length": [C.capsule(301, 177, 301, 177, 37, RED)],
        "capsule_three_branches": [C.capsule(83, 61, 401, 250, 45, BLUE, 200)],
        "capsule_hairline": [C.capsule(13, 350, 630, 17, 3, INK)],
        "trapezoid_one_unit_wide": [C.trapezoid(166, 167, 20, 20, 300, 300, RED), C.trapezoid(167, 168, 20, 20, 300, 300, BLUE)],
        "trapezoid_lo_above_hi": [C.trapezoid(40, 600, 200, 210, 100, 90, RED)],
        "trapezoid_sloped": [C.trapezoid(37, 333, 50, 181, 120, 377, GREEN, 128)],
        "trapezoid_crossing": [C.trapezoid(20, 620, 30, 350, 340, 40, GREEN, 255)],
        "box_subpixel": [C.box(35, 21, 250, 27, RED), C.box(401, 99, 407, 371, BLUE, 77)],
        "box_dashed": [C.box(21, 100, 601, 131, INK, dash=(48, 29)), C.box(300, -40, 331, 500, RED, 180, dash=(37, 22)),
                       C.box(100, 200, 420, 230, BLUE, dash=(5, 3))],
        "triangle_both_orientations": [C.triangle(33, 29, 390, 77, 201, 350, RED, 160),
                                       C.triangle(601, 300, 450, 60, 333, 333, BLUE)],
        "triangle_degenerate": [C.triangle(50, 50, 150, 150, 250, 250, INK)],
        "glyphs": [C.glyph(35, 21, "A", 1, INK), C.glyph(150, 19, "g", 3, RED), C.glyph(452, 100, "R", 1, BLUE, True),
                   C.glyph(263, 129, "k", 3, GREEN, True, 130), C.glyph(560, 250, "~", 2, INK), C.glyph(600, 20, " ", 2, RED)],
    }
    # every type partly off each canvas edge (left, top, right, bottom) ...
    shifts = {"left": (-150, 120), "top": (250, -110), "right": (16 * W - 90, 100), "bottom": (200, 16 * H - 70)}
    for edge, (x, y) in shifts.items():
        cases["off_" + edge] = [
            C.box(x - 60, y - 45, x + 130, y + 77, RED, 140), C.capsule(x - 80, y + 60, x + 170, y - 50, 33, BLUE),
            C.trapezoid(x - 100, x + 140, y - 90, y - 10, y + 30, y + 150, GREEN, 90),
            C.triangle(x - 120, y, x + 160, y - 100, x + 40, y + 180, INK, 60), C.glyph(x - 50, y - 50, "W", 2, INK),
            C.glyph(x + 20, y + 10, "Q", 1, RED, True)]
    # ... and wholly outside it
    cases["outside"] = [
        C.box(-900, -800, -5, 4000, RED), C.box(16 * W + 1, 0, 16 * W + 500, 300, RED), C.capsule(-400, -400, -60, 900, 50, BLUE),
        C.capsule(100, 16 * H + 300, 500, 16 * H + 60, 40, BLUE), C.trapezoid(-500, -1, 0, 0, 300, 300, GREEN),
        C.trapezoid(0, 600, -400, -300, -2, -1, GREEN), C.triangle(700, 10, 900, 50, 800, 300, INK),
        C.triangle(10, -10, 300, -200, 500, -3, INK), C.glyph(-4096, 100, "M", 3, INK), C.glyph(100, 16 * H + 2, "M", 1, INK, True),
        C.box(36000, 36000, 36864, 36864, RED), C.capsule(-4096, -4096, 36864, -4000, 10, RED)]
    return cases


def table(records):
    return C.check_table(np.array(records, dtype=np.int64).reshape(-1, C.REC).astype(np.int32))


def order_dependent(n, spread):
    """n tiny translucent boxes whose blend depends on their order: all on the pixels (3..6, 2..5) of one tile, or with
    spread=True wandering over the whole canvas (and partly beyond it)"""
    recs = []
    for i in range(n):
        colour = ((37 * i) % 256, (101 * i + 50) % 256, (211 * i + 90) % 256)
        x, y = ((53 * i) % (16 * W + 60) - 30, (29 * i) % (16 * H + 60) - 30) if spread else (50 + i % 7, 33 + i % 5)
        recs.append(C.box(x, y, x + 41 + i % 3, y + 37 + i % 4, colour, 40 + (i * 7) % 180))
    return recs


def small_figure():
    """about 300 x 120: three panels, three series of four points; bands in panel 0, error bars in panel 1, plain
    lines with markers in panel 2"""
    x = np.array([2.0, 3.0, 4.0, 5.0])
    ys = [np.array([0.10, 0.45, 0.30, 0.20]), np.array([0.55, 0.90, 0.70, 0.62]), np.array([1.00, 1.35, 1.15, 1.40])]
    marks = ("o", "s", "o")
    p0 = [C.Series(x, y, C.TAB10[i], marker=marks[i], band=(y - 0.08, y + 0.05 * (i + 1)), label="s%d" % i)
          for i, y in enumerate(ys)]
    p1 = [C.Series(x, y, C.TAB10[i], yerr=np.full(4, 0.04 * (i + 1))) for i, y in enumerate(ys)]
    p2 = [C.Series(x, y, C.TAB10[i], marker=marks[i]) for i, y in enumerate(ys)]
    panels = [C.Panel("Ab", "t", "y", p0, vline=3.5), C.Panel("Cd", "t", "", p1, vline=3.5), C.Panel("Ef", "t", "", p2)]
    return C.Figure(panels, width=324, height=120, text_scale=1)


def eval_dict(seed, n=7, t=6, lpips=True, temperature=0.7):
    """a synthetic evaluations.pt: the eleven keys of eval_settings.EVAL_KEYS with [n, t] values"""
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(n, t, generator=g)
    return {"SSIM_values": r(0.5, 0.9), "PSNR_values": r(15, 25), "MSE_values": r(0, 0.1),
            "LPIPS_values": r(0.1, 0.4) if lpips else None, "temperature": temperature, "BPD": torch.rand(3, generator=g),
            "DKL": torch.rand(3, generator=g), "RECON": torch.rand(3, generator=g), "SSIM_std_mean": r(0.4, 0.8),
            "PSNR_std_mean": r(12, 22), "LPIPS_std_mean": r(0.2, 0.5) if lpips else None}


def write_experiments(root, names, lpips=True, t=6):
    """root/<name>/eval_folder/evaluations.pt for every name; returns the folder path with a trailing slash and the
    dicts"""
    dicts = []
    for i, name in enumerate(names):
        os.makedirs(os.path.join(str(root), name, "eval_folder"))
        dicts.append(eval_dict(100 + i, lpips=lpips, t=t))
        torch.save(dicts[-1], os.path.join(str(root), name, "eval_folder", "evaluations.pt"))
    return str(root) + "/", dicts
