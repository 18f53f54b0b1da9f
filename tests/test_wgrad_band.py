"""The band kernel of the few-channel 3x3 weight gradients (rfn_conv3x3_wgrad_band_bf16x3), called directly on the
smallest shapes at which each of its parts can go wrong, against the exact three-product fp64 model of
tests/test_conv_grad_model.py and against the route the same operands took before (implicit, or tap scatter + GEMM).

Bounds: those check_wgrad applies to the implicit routes -- e_abs vs the model <= 3 * e_abs(fp32-MFMA kernel vs fp64) +
2e-8 and <= WGRAD_CAP, vs exact fp64 <= SPLIT_BOUND -- with the gradient at 1 and at 2^k for the three SCALES (weight
gradients end in float atomics, so the scaled runs are held to the model, not bit for bit).  Two kernels that are each
within WGRAD_CAP of the model differ by at most 2 * WGRAD_CAP of S = op(|g|, |x|): the cross-route bound.

Cases (N, C1, C2, Cout, H, W, view); what the launch geometry of each must show is asserted from the library's own answer
(rfn_conv3x3_wgrad_band_geometry), not from this table:
  16x16_5+9_24   source boundary inside an 8-channel group, Cout 24 (rows padded to 32), 126 columns, in1 and g views
  8x32_16_16     non-square map, 144 columns, one row tile of 16 real rows
  64x64_16_16    bands of 2 rows: first, inner and last bands of a frame, several bands per frame
  16x16_40_16    Cin > Cout, 360 columns (no multiple of 32) over three column blocks of blockIdx.y
  8x32_64_72     three row tiles over blockIdx.z = 2, four column blocks; 17 frames: 68 units for 64 workgroup slots, so
                 workgroups walk two bands each and the last ones get none
"""
import ctypes

import pytest
import torch

from tests.test_conv_grad_model import (K, SCALES, WGRAD_CAP, check, e_abs, launches, refs64, wgrad_f32,  # noqa: F401
                                        wgrad_op)

pytestmark = pytest.mark.gpu

ENTRY = "rfn_conv3x3_wgrad_band_bf16x3"
CASES = {
    "16x16_5+9_24": (3, 5, 9, 24, 16, 16, True),
    "8x32_16_16":   (2, 16, 0, 16, 8, 32, False),
    "64x64_16_16":  (2, 16, 0, 16, 64, 64, False),
    "16x16_40_16":  (3, 40, 0, 16, 16, 16, True),
    "8x32_64_72":   (17, 64, 0, 72, 8, 32, False),
}


def geometry(K, Cout, Cin, N, H, W):
    from rfn_hip import lib
    out = (ctypes.c_longlong * 6)()
    assert lib.load().rfn_conv3x3_wgrad_band_geometry(Cout, Cin, N, H, W, ctypes.addressof(out)) == 0
    return dict(zip(("R", "CPB", "gx", "gy", "gz", "lds"), out))


def band(K, in1, in2, g, Cout):
    """the entry point itself: the plan would keep shapes this small on their old routes"""
    N, C1, H, W = in1.shape
    C2 = 0 if in2 is None else int(in2.shape[1])
    label = K.kernel_label("rfn_conv3x3_wgrad_band_kernel_label_bf16x3", Cout, C1 + C2, N, H, W)
    assert label.startswith("wgrad_band_kernel<"), label
    gw = K._b3_wgrad((ENTRY, label), 0, [([g], "g", Cout), ([in1], "in1", C1), (None if in2 is None else [in2], "in2", C2)],
                     Cout, 9 * (C1 + C2), (N, H, W), None, " band3x3")
    return gw[0].view(Cout, C1 + C2, 3, 3)


@pytest.fixture(scope="module")
def case_data():
    """per case: host operands, their fp64 references (computed once, never modified)"""
    cache = {}

    def get(name):
        if name not in cache:
            N, C1, C2, Cout, H, W, view = CASES[name]
            gen = torch.Generator().manual_seed(90 + list(CASES).index(name))
            z = torch.randn(N, C1 * (2 if view else 1), H, W, generator=gen) * 3 + 0.5
            c = torch.randn(N, C2, H, W, generator=gen) if C2 else None
            gy = torch.randn(N, Cout + (8 if view else 0), H, W, generator=gen)
            x = z[:, :C1] if c is None else torch.cat([z[:, :C1], c], 1)
            g = gy[:, 4:4 + Cout] if view else gy
            cache[name] = (z, c, gy, refs64(g, x, wgrad_op(3)))
        return cache[name]
    return get


def test_the_cases_reach_what_they_are_for(K):
    geo = {n: geometry(K, c[3], c[1] + c[2], c[0], c[4], c[5]) for n, c in CASES.items()}
    assert geo["64x64_16_16"]["R"] < 64 // 2                      # first, inner and last bands
    assert geo["16x16_5+9_24"]["gy"] == 1 and geo["8x32_16_16"]["gy"] == 1
    assert geo["16x16_40_16"]["gy"] == 3                          # the column split
    g = geo["8x32_64_72"]
    units = 17 * (8 // g["R"])
    per = -(-units // g["gx"])
    assert (g["gy"], g["gz"]) == (4, 2) and per >= 2 and per * (g["gx"] - 1) >= units   # several bands; idle workgroups
    assert all(v["lds"] <= 79 * 1024 for v in geo.values())


@pytest.mark.parametrize("name", list(CASES))
def test_band_vs_model_and_old_route(K, launches, monkeypatch, case_data, name):
    N, C1, C2, Cout, H, W, view = CASES[name]
    z, c, gy, (gm, g64, s) = case_data(name)
    zd, cd, gyd = z.cuda(), None if c is None else c.cuda(), gy.cuda()
    in1 = zd[:, :C1]
    g = gyd[:, 4:4 + Cout] if view else gyd
    n0 = len(launches)
    got = band(K, in1, cd, g, Cout)
    assert [e for e, _ in launches[n0:]] == [ENTRY]
    gf = wgrad_f32(K, in1, cd, g, Cout, 3)
    fig = {"model": e_abs(got, gm, s), "fp64": e_abs(got, g64, s), "f32": e_abs(gf, g64, s)}
    check(name, fig, cap=WGRAD_CAP)
    bound = min(3 * fig["f32"] + 2e-8, WGRAD_CAP)
    for k in SCALES:
        e = e_abs(band(K, in1, cd, g * 2.0 ** k, Cout), gm * 2.0 ** k, s * 2.0 ** k)
        msg = "%s: e_abs vs model at gradient * 2^%d: %.3g" % (name, k, e)
        print(msg)
        assert e <= bound, msg
    # the route these operands had: implicit (Cin <= Cout) or tap scatter + GEMM
    monkeypatch.setenv("RFN_WGRAD_BAND", "0")
    n0 = len(launches)
    old = K.conv2d_wgrad(in1, cd, g, Cout, 3)
    assert ENTRY not in [e for e, _ in launches[n0:]]
    d = e_abs(got, old.detach().cpu().double(), s)
    print("%s: band vs %s: %.3g" % (name, launches[n0][0], d))
    assert d <= 2 * WGRAD_CAP


def test_accumulates_into_the_callers_gw_and_the_plan_runs_it(K, launches, monkeypatch, case_data):
    """gw is added to, not overwritten; and with the threshold lowered conv2d_wgrad takes the band launch and returns
    the same gradient"""
    name = "8x32_16_16"
    N, C1, C2, Cout, H, W, view = CASES[name]
    z, c, gy, (gm, g64, s) = case_data(name)
    zd, gyd = z.cuda(), gy.cuda()
    from rfn_hip import lib
    gw = torch.full((Cout, 9 * C1), 2.0, device="cuda")
    lib.call(ENTRY, *lib.frames(gyd, "g"), Cout, *lib.frames(zd, "in1"), C1, None, 0, 0, lib.dev(gw), N, H, W)
    assert e_abs(gw.view(Cout, C1, 3, 3) - 2.0, gm, s) <= 2 * WGRAD_CAP   # (the 2.0 costs a few ulp of the sum)
    monkeypatch.setenv("RFN_WGRAD_BAND_MIN_PIXELS", "1")
    n0 = len(launches)
    got = K.conv2d_wgrad(zd, None, gyd, Cout, 3)
    assert launches[n0:] == [(ENTRY, "wgrad_band_kernel<1,5,1>")]
    assert e_abs(got, gm, s) <= WGRAD_CAP
