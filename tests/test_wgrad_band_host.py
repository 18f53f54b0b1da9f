"""CPU-only: which shapes the band weight-gradient kernel takes (rfn_conv3x3_wgrad_band_supported, its label and geometry
queries) and where rfn_hip.ops.wgrad_plan routes to it: ungrouped 3x3 gradients with Cout <= 128, Cin <= 128 and
W % 8 == 0 from wgrad_band_min_pixels(Cout) pixels on; everything else keeps the route and the label it had."""
import ctypes

import pytest

BAND = "rfn_conv3x3_wgrad_band_bf16x3"
IMPL = ("rfn_conv3x3_wgrad_implicit_bf16x3", "rfn_conv3x3_wgrad_implicit_grouped_bf16x3")
GEMM = "rfn_gemm_wgrad_bf16x3"
SCATTER = ("rfn_tap_scatter_f32", "tap_scatter")


@pytest.fixture
def K(monkeypatch):
    from rfn_hip import ops
    for knob in ("RFN_WGRAD_BAND", "RFN_WGRAD_BAND_MIN_PIXELS", "RFN_WGRAD_IMPLICIT", "RFN_WGRAD_MIRRORED"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setattr(ops, "CONV_PRECISION", "mixed")
    return ops


def supported(Cout, Cin, H, W):
    from rfn_hip import lib
    return lib.load().rfn_conv3x3_wgrad_band_supported(Cout, Cin, H, W)


def geometry(Cout, Cin, F, H, W):
    from rfn_hip import lib
    out = (ctypes.c_longlong * 6)()
    rc = lib.load().rfn_conv3x3_wgrad_band_geometry(Cout, Cin, F, H, W, ctypes.addressof(out))
    return rc, dict(zip(("R", "CPB", "gx", "gy", "gz", "lds"), out))


@pytest.mark.parametrize("Cout,Cin,H,W,ok", [
    (16, 16, 64, 64, 1), (32, 32, 32, 32, 1), (64, 64, 16, 16, 1), (128, 128, 8, 8, 1), (16, 64, 32, 32, 1),
    (32, 128, 16, 16, 1), (1, 1, 2, 8, 1), (24, 14, 8, 24, 1), (128, 3, 64, 64, 1),
    (129, 16, 16, 16, 0), (16, 129, 16, 16, 0), (16, 16, 16, 12, 0), (16, 16, 16, 4, 0),
    (16, 16, 3, 8, 0),    # no divisor R of H with R * W % 16 == 0
    (16, 16, 1, 16, 1),   # the whole frame as one band of one row
])
def test_supported_and_label(K, Cout, Cin, H, W, ok):
    assert supported(Cout, Cin, H, W) == ok
    label = K.kernel_label("rfn_conv3x3_wgrad_band_kernel_label_bf16x3", Cout, Cin, 4, H, W)
    assert label == (("wgrad_band_kernel<1,5,1>" if Cout <= 32 else "wgrad_band_kernel<2,5,0>") if ok else "")
    rc, g = geometry(Cout, Cin, 4, H, W)
    assert rc == (0 if ok else -2)
    if ok:
        assert H % g["R"] == 0 and g["R"] * W % 16 == 0 and 9 * g["CPB"] <= 160
        assert g["gy"] == -(-Cin // g["CPB"]) and g["gz"] == -(-Cout // (32 if Cout <= 32 else 64))
        assert 16384 <= g["lds"] <= 79 * 1024 and 1 <= g["gx"] <= max(1, 512 // (g["gy"] * g["gz"]))


def test_geometry_of_the_bench_shapes():
    """the shapes of the extractor / upscaler blocks: bands of several k-steps, two workgroups per CU"""
    for Cout, Cin, S in ((16, 16, 64), (32, 16, 32), (32, 32, 32), (64, 32, 16), (64, 64, 16), (128, 128, 8), (16, 64, 32),
                         (32, 128, 16)):
        rc, g = geometry(Cout, Cin, 640, S, S)
        assert rc == 0 and g["R"] * S >= 64 and g["gx"] * g["gy"] * g["gz"] <= 512, (Cout, Cin, S, g)


def test_plan_takes_the_band_route_from_the_threshold_on(K):
    assert K.wgrad_band_min_pixels(32) == 1 << 15 and K.wgrad_band_min_pixels(33) == 1 << 17
    # Cin <= Cout, 64 x 64: 8 frames are 32768 pixels
    plan = K.wgrad_plan(0, 8, 16, 0, 16, 64, 64, 3)
    assert (plan.form, plan.M, plan.Nc, plan.launches) == ("band", 16, 144, [(BAND, "wgrad_band_kernel<1,5,1>")])
    below = K.wgrad_plan(0, 7, 16, 0, 16, 64, 64, 3)
    assert below.form == "implicit" and below.launches == [(IMPL[0], "gemm_wgrad_b3_kernel<1,4,1,2,32,1>")]
    # Cin > Cout, 32 x 32, two sources: 32 frames
    plan = K.wgrad_plan(0, 32, 40, 24, 16, 32, 32, 3)
    assert (plan.form, plan.M, plan.Nc, plan.launches) == ("band", 16, 576, [(BAND, "wgrad_band_kernel<1,5,1>")])
    below = K.wgrad_plan(0, 31, 40, 24, 16, 32, 32, 3)
    label = K.kernel_label("rfn_gemm_wgrad_kernel_label_bf16x3", 144, 64, 144 * 1024, 64 * 1024, 0, 31, 1024)
    assert below.form == "scatter" and below.launches == [SCATTER, (GEMM, label)]
    # more than 32 output channels (two row tiles per block): from 2^17 pixels on, 16 x 16 maps: 512 frames
    plan = K.wgrad_plan(0, 512, 32, 0, 64, 16, 16, 3)
    assert (plan.form, plan.M, plan.Nc, plan.launches) == ("band", 64, 288, [(BAND, "wgrad_band_kernel<2,5,0>")])
    below = K.wgrad_plan(0, 511, 32, 0, 64, 16, 16, 3)
    assert below.form == "implicit" and below.launches == [(IMPL[0], "gemm_wgrad_b3_kernel<2,2,2,2,64,1>")]
    assert K.wgrad_plan(0, 640, 128, 0, 128, 8, 8, 3).form == "implicit"   # 40960 pixels of an 8 x 8 map
    # a Conv2dZeros with few inputs is the same problem
    assert K.wgrad_plan(0, 32, 64, 0, 4, 32, 32, 3, few_out=True).form == "band"


def test_everything_else_keeps_its_route(K, monkeypatch):
    big = 64   # frames: far above the threshold
    grouped = K.wgrad_plan(3, big, 16, 0, 16, 64, 64, 3)
    assert grouped.form == "implicit" and grouped.launches == [(IMPL[1], "gemm_wgrad_b3_kernel<grouped 2,2,2,2,64,1>")]
    assert K.wgrad_plan(3, big, 64, 0, 16, 32, 32, 3, stacked=True).form == "scatter"
    assert K.wgrad_plan(0, big, 16, 0, 129, 64, 64, 3).form == "implicit"      # Cout > 128
    assert K.wgrad_plan(0, big, 129, 0, 16, 64, 64, 3).form == "scatter"       # Cin > 128
    assert K.wgrad_plan(0, big * 16, 16, 0, 16, 12, 12, 3).form == "im2col"    # W % 8 != 0
    assert K.wgrad_plan(0, big * 64, 16, 0, 16, 3, 8, 3).form == "implicit"    # the library names no band kernel
    assert K.wgrad_plan(0, big, 16, 0, 16, 64, 64, 1).form == "gemm"
    monkeypatch.setattr(K, "CONV_PRECISION", "f32")
    assert K.wgrad_plan(0, big, 16, 0, 16, 64, 64, 3).form == "f32"
    monkeypatch.setattr(K, "CONV_PRECISION", "mixed")
    monkeypatch.setenv("RFN_WGRAD_BAND", "0")
    assert K.wgrad_plan(0, big, 16, 0, 16, 64, 64, 3).form == "implicit"
    monkeypatch.delenv("RFN_WGRAD_BAND")
    monkeypatch.setenv("RFN_WGRAD_BAND_MIN_PIXELS", str(64 * 4096 + 1))
    assert K.wgrad_plan(0, big, 16, 0, 16, 64, 64, 3).form == "implicit"
