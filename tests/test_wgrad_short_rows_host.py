"""CPU-only: the short-row 3x3 weight-gradient forms (4 x 4 and 2 x 2 maps, the taps shifted while staging) on the host
side.  rfn_hip.ops.wgrad_plan takes them only with short_rows=True -- with the default every plan is what it was -- and the
four entry points rfn_conv3x3_wgrad_rows[_mirrored][_grouped]_bf16x3 refuse what the existing bodies refuse, in the same
order, plus every map the staging does not cover.  No device and no launch (see tests/test_wgrad_args_host.py: made-up
aligned addresses, every call refused by a check or F = 0)."""
import ctypes

import pytest

from tests.test_wgrad_args_host import A, B, B2, GW, G_OK, TOO_MANY, _arr, _call

SCATTER, IM2COL = ("rfn_tap_scatter_f32", "tap_scatter"), ("rfn_im2col3x3_f32", "im2col3x3")
GEMM_QUERY = "rfn_gemm_wgrad_kernel_label_bf16x3"
ROWS = "rfn_conv3x3_wgrad_rows_bf16x3"
ROWS_MIRRORED = "rfn_conv3x3_wgrad_rows_mirrored_bf16x3"
ROWS4, ROWS2 = "gemm_wgrad_b3_kernel<2,2,2,2,64,2>", "gemm_wgrad_b3_kernel<2,2,2,2,64,3>"


@pytest.fixture
def K(monkeypatch):
    from rfn_hip import ops
    for knob in ("RFN_WGRAD_MIRRORED", "RFN_WGRAD_IMPLICIT", "RFN_WGRAD_SHORT_ROWS"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setattr(ops, "CONV_PRECISION", "mixed")
    return ops


def _grouped(G, entry, label):
    return (entry.replace("_bf16x3", "_grouped_bf16x3"), label.replace("<", "<grouped ")) if G else (entry, label)


def _gemm(K, G, M, Nc, a_ns, b_ns, N, HW):
    return _grouped(G, "rfn_gemm_wgrad_bf16x3", K.kernel_label(GEMM_QUERY, M, Nc, a_ns, b_ns, G, N, HW))


# conv1-type calls (G, N, C1, C2, Cout, H, W) and Conv2dZeros calls (G, N, Cin, C, H, W) of the two deepest flow levels
CONV1 = [(10, 608, 16, 128, 256, 4, 4), (0, 608, 32, 256, 256, 2, 2), (0, 76, 1152, 0, 128, 4, 4), (3, 5, 288, 0, 256, 2, 2)]
ZEROS = [(10, 608, 256, 32, 4, 4), (10, 608, 256, 64, 2, 2), (0, 33, 256, 32, 4, 4), (0, 7, 256, 64, 2, 2)]


@pytest.mark.parametrize("G,N,C1,C2,Cout,H,W", CONV1)
def test_default_plan_of_a_conv_is_todays(K, G, N, C1, C2, Cout, H, W):
    Cin, HW, n = C1 + C2, H * W, max(G, 1)
    plan = K.wgrad_plan(G, N, C1, C2, Cout, H, W, 3)
    assert plan == K.wgrad_plan(G, N, C1, C2, Cout, H, W, 3, short_rows=False)
    if Cin <= Cout:
        assert plan.form == "im2col" and (plan.M, plan.Nc) == (Cout, 9 * Cin)
        assert plan.launches == [IM2COL] * n + [_gemm(K, G, Cout, 9 * Cin, Cout * HW, 9 * Cin * HW, N, HW)]
    else:
        assert plan.form == "scatter" and (plan.M, plan.Nc) == (9 * Cout, Cin)
        assert plan.launches == [SCATTER] * n + [_gemm(K, G, 9 * Cout, Cin, 9 * Cout * HW, Cin * HW, N, HW)]


@pytest.mark.parametrize("G,N,Cin,C,H,W", ZEROS)
def test_default_plan_of_a_zeros_conv_is_todays(K, G, N, Cin, C, H, W):
    HW = H * W
    plan = K.wgrad_plan(G, N, Cin, 0, C, H, W, 3, few_out=True, stacked=bool(G))
    assert plan.form == "scatter" and (plan.M, plan.Nc) == (9 * C, Cin)
    assert plan.launches == [SCATTER] + [_gemm(K, G, 9 * C, Cin, 9 * C * HW, Cin * HW, N, HW)]


@pytest.mark.parametrize("G,N,C1,C2,Cout,H,W", CONV1)
def test_short_rows_plan_of_a_conv_is_one_implicit_launch(K, G, N, C1, C2, Cout, H, W):
    """whatever Cin against Cout: the input planes are the shifted operand, so a two-source input is never concatenated"""
    plan = K.wgrad_plan(G, N, C1, C2, Cout, H, W, 3, short_rows=True)
    label = K.kernel_label(ROWS.replace("_bf16x3", "_kernel_label_bf16x3"), Cout, Cout * H * W, G, N, H, W)
    assert label == (ROWS4 if W == 4 else ROWS2)
    assert plan.form == "implicit_rows" and (plan.M, plan.Nc) == (Cout, 9 * (C1 + C2))
    assert plan.launches == [_grouped(G, ROWS, label)]


@pytest.mark.parametrize("G,N,Cin,C,H,W", ZEROS)
def test_short_rows_plan_of_a_zeros_conv_is_one_mirrored_launch(K, G, N, Cin, C, H, W):
    plan = K.wgrad_plan(G, N, Cin, 0, C, H, W, 3, few_out=True, stacked=bool(G), short_rows=True, min_pixels=1 << 30)
    label = K.kernel_label(ROWS_MIRRORED.replace("_bf16x3", "_kernel_label_bf16x3"), Cin, Cin * H * W, C, G, N, H, W)
    assert label == (ROWS4 if W == 4 else ROWS2)
    assert plan.form == "mirrored_rows" and (plan.M, plan.Nc) == (Cin, 9 * C)
    assert plan.launches == [_grouped(G, ROWS_MIRRORED, label)]


@pytest.mark.parametrize("H,W", [(6, 6), (12, 12), (8, 8), (4, 8), (16, 16), (3, 4), (2, 4), (4, 2)])
def test_maps_the_staging_does_not_cover_keep_their_plan(K, H, W):
    covered = W == 4 and H % 2 == 0
    for few_out in (False, True):
        for G in (0, 3):
            for C1, C2, Cout in ((16, 0 if few_out else 8, 64), (64, 0, 8)):
                args = (G, 5, C1, C2, Cout, H, W, 3)
                new = K.wgrad_plan(*args, few_out=few_out, short_rows=True)
                if covered:
                    assert new.form in ("implicit_rows", "mirrored_rows")
                else:
                    assert new == K.wgrad_plan(*args, few_out=few_out) and not new.form.endswith("_rows")


def test_queries_name_a_kernel_only_for_covered_maps(K):
    for (H, W), want in [((4, 4), ROWS4), ((2, 4), ROWS4), ((6, 4), ROWS4), ((2, 2), ROWS2), ((3, 4), ""), ((4, 2), ""),
                         ((8, 8), ""), ((6, 6), ""), ((12, 12), ""), ((1, 4), ""), ((0, 4), "")]:
        assert K.kernel_label("rfn_conv3x3_wgrad_rows_kernel_label_bf16x3", 64, 64 * H * W, 0, 5, H, W) == want
        assert K.kernel_label("rfn_conv3x3_wgrad_rows_mirrored_kernel_label_bf16x3", 64, 64 * H * W, 8, 3, 5, H, W) == want


def test_f32_and_1x1_keep_their_plan(K, monkeypatch):
    assert K.wgrad_plan(0, 5, 16, 8, 64, 4, 4, 1, short_rows=True) == K.wgrad_plan(0, 5, 16, 8, 64, 4, 4, 1)
    monkeypatch.setattr(K, "CONV_PRECISION", "f32")
    for few_out in (False, True):
        plan = K.wgrad_plan(0, 5, 16, 0, 4, 4, 4, 3, few_out=few_out, short_rows=True)
        assert plan == K.wgrad_plan(0, 5, 16, 0, 4, 4, 4, 3, few_out=few_out)
        assert plan.form in ("f32", "scatter_f32")


def test_the_callers_helper_honours_the_knob(K, monkeypatch):
    assert K.wgrad_short_rows() is True
    monkeypatch.setenv("RFN_WGRAD_SHORT_ROWS", "1")
    assert K.wgrad_short_rows() is True
    monkeypatch.setenv("RFN_WGRAD_SHORT_ROWS", "0")
    assert K.wgrad_short_rows() is False


# ---------------------------------------------------------------------------------------------------- entry points
def _rows(grouped, H=4, W=4):
    d = dict(g=_arr(A) if grouped else A, g_ns=64 * H * W, Cout=64, in1=_arr(B) if grouped else B, in1_ns=8 * H * W, C1=4,
             in2=_arr(B2) if grouped else B2, in2_ns=4 * H * W, C2=4, gw=_arr(GW) if grouped else GW)
    if grouped:
        d["G"] = G_OK
    d.update(F=3, H=H, W=W)
    return d


def _rows_mirrored(grouped, H=4, W=4):
    d = dict(h=_arr(A) if grouped else A, h_ns=64 * H * W, Cin=64, g=_arr(B) if grouped else B, g_ns=4 * H * W, C=4,
             gwT=_arr(GW) if grouped else GW)
    if grouped:
        d["G"] = G_OK
    d.update(F=3, H=H, W=W)
    return d


FORMS = {ROWS: (_rows, ("g", "in1", "in2", "gw"), ("g_ns", "in1_ns", "in2_ns"), ("Cout", "C1"), {"g": A, "in1": B, "in2": B2}),
         ROWS_MIRRORED: (_rows_mirrored, ("h", "g", "gwT"), ("h_ns", "g_ns"), ("Cin", "C"), {"h": A, "g": B})}
ENTRY_POINTS = [(n, g, hw) for n in FORMS for g in (False, True) for hw in ((4, 4), (2, 2))]


def _cases(name, grouped, H, W):
    """(what, arguments, expected code): each violates exactly one condition of the valid call"""
    make, operands, strides, counts, inputs = FORMS[name]
    out = []

    def case(what, code, **changed):
        d = make(grouped, H, W)
        assert set(changed) <= set(d), changed
        d.update(changed)
        out.append((what, d, code))

    for o in operands:
        case("null " + o, -1, **{o: None})
    for c in counts:
        case(c + " = 0", -1, **{c: 0})
        case(c + " < 0", -1, **{c: -3})
    if grouped:
        case("G = 0", -1, G=0)
        case("G = 17", -1, G=17)
    for h, w in ((8, 8), (16, 16), (6, 6), (12, 12), (3, 4), (4, 2), (2, 8), (1, 4)):   # what the staging does not cover
        case("%d x %d" % (h, w), -2, H=h, W=w)
    case("H = 0", -2 if grouped else -1, H=0)
    for s in strides:
        case(s + " % 4 != 0", -2, **{s: make(grouped, H, W)[s] + 2})
    for o, base in inputs.items():
        if grouped:
            case("misaligned %s of the last group" % o, -3, **{o: _arr(base, last=base + 4096 * (G_OK - 1) + 4)})
            case("null %s of the last group" % o, -3, **{o: _arr(base, last=0)})
        else:
            case("misaligned " + o, -3, **{o: base + 8})
    if grouped:
        case("null output of the last group", -3, **{operands[-1]: _arr(GW, last=0)})
    case("F * H * W too large", -4, F=TOO_MANY // (H * W))
    return out


@pytest.mark.parametrize("name,grouped,hw", ENTRY_POINTS)
def test_each_violation_returns_its_code(name, grouped, hw):
    from rfn_hip import lib
    L = lib.load()
    entry = name.replace("_bf16x3", "_grouped_bf16x3") if grouped else name
    cases = _cases(name, grouped, *hw)
    assert len(cases) >= 20
    for what, args, code in cases:
        assert _call(L, entry, args) == code, (entry, what)
        assert L.rfn_last_error(), (entry, what)


@pytest.mark.parametrize("name,grouped,hw", ENTRY_POINTS)
def test_no_frames_returns_zero(name, grouped, hw):
    from rfn_hip import lib
    L = lib.load()
    entry = name.replace("_bf16x3", "_grouped_bf16x3") if grouped else name
    d = FORMS[name][0](grouped, *hw)
    d["F"] = 0
    assert _call(L, entry, d) == 0, entry


def test_existing_entry_points_still_refuse_short_rows():
    from rfn_hip import lib
    from tests.test_wgrad_args_host import _implicit, _mirrored
    L = lib.load()
    for make, name in ((_implicit, "rfn_conv3x3_wgrad_implicit_bf16x3"), (_mirrored, "rfn_conv3x3_wgrad_mirrored_bf16x3")):
        for H, W in ((4, 4), (2, 2)):
            d = make(False)
            d.update(H=H, W=W)
            assert _call(L, name, d) == -2
    assert L.rfn_conv3x3_wgrad_mirrored_kernel_label_bf16x3(256, 256 * 16, 16, 10, 608, 4, 4) == b""
