"""CPU-only: rfn_hip.ops.wgrad_plan, the one decision of the weight-gradient path, on the routes the convolution tables of
tests/test_kernel_routes_host.py do not reach: the Conv2dZeros callers (few_out: the mirrored kernel and its size
threshold, the fp32 tap route), the two environment switches, and stacked / unstacked gradients of a group.  The expected
labels are those of the tables of tests/test_wgrad_mirrored.py, or the library's answer to the launch's own query."""
import pytest

from tests.test_conv_grad_model import WGRAD_CASES
from tests.test_wgrad_mirrored import LABELS

SCATTER = ("rfn_tap_scatter_f32", "tap_scatter")
GEMM = ("rfn_gemm_wgrad_bf16x3", "rfn_gemm_wgrad_grouped_bf16x3")
MIRRORED = ("rfn_conv3x3_wgrad_mirrored_bf16x3", "rfn_conv3x3_wgrad_mirrored_grouped_bf16x3")
GEMM_QUERY, F32_QUERY = "rfn_gemm_wgrad_kernel_label_bf16x3", "rfn_conv2d_wgrad_kernel_label_f32"


@pytest.fixture
def K(monkeypatch):
    from rfn_hip import ops
    for knob in ("RFN_WGRAD_MIRRORED", "RFN_WGRAD_IMPLICIT"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setattr(ops, "CONV_PRECISION", "mixed")
    return ops


def _zeros_plan(K, shape, **kw):
    Cin, Ctot, C, G, N, H, W = shape
    return K.wgrad_plan(G, N, Cin, 0, C, H, W, 3, in1_ns=Ctot * H * W, **kw)


def _scatter_gemm(K, shape, scatters=1):
    """tap scatter + GEMM of a 3x3 gradient with more inputs than outputs: 9 C rows, dense scattered operand"""
    Cin, Ctot, C, G, N, H, W = shape
    label = K.kernel_label(GEMM_QUERY, 9 * C, Cin, 9 * C * H * W, Ctot * H * W, G, N, H * W)
    return [SCATTER] * scatters + [(GEMM[1], label.replace("<", "<grouped ")) if G else (GEMM[0], label)]


@pytest.mark.parametrize("shape,label", LABELS)
def test_few_out_takes_the_mirrored_launch_where_the_library_names_one(K, shape, label):
    G = shape[3]
    plan = _zeros_plan(K, shape, few_out=True, stacked=bool(G))
    if label:
        assert plan.form == "mirrored" and (plan.M, plan.Nc) == (shape[0], 9 * shape[2])
        assert plan.launches == [(MIRRORED[1], label.replace("<", "<grouped ")) if G else (MIRRORED[0], label)]
    else:
        assert plan.form == "scatter" and plan.launches == _scatter_gemm(K, shape)
        assert plan == _zeros_plan(K, shape, few_out=False, stacked=bool(G))
    # a convolution that is no Conv2dZeros never takes it
    assert _zeros_plan(K, shape, stacked=bool(G)).launches == _scatter_gemm(K, shape)


@pytest.mark.parametrize("shape,label", [c for c in LABELS if c[1]])
def test_min_pixels_is_the_first_size_that_takes_the_mirrored_launch(K, shape, label):
    Cin, Ctot, C, G, N, H, W = shape
    pixels = max(G, 1) * N * H * W
    assert _zeros_plan(K, shape, few_out=True, min_pixels=pixels, stacked=bool(G)).form == "mirrored"
    below = _zeros_plan(K, shape, few_out=True, min_pixels=pixels + 1, stacked=bool(G))
    assert below.form == "scatter" and below.launches == _scatter_gemm(K, shape)


@pytest.mark.parametrize("shape,label", [c for c in LABELS if c[1]])
def test_mirrored_switched_off_is_scatter_and_gemm(K, monkeypatch, shape, label):
    monkeypatch.setenv("RFN_WGRAD_MIRRORED", "0")
    assert _zeros_plan(K, shape, few_out=True, stacked=bool(shape[3])).launches == _scatter_gemm(K, shape)


@pytest.mark.parametrize("name", [n for n in WGRAD_CASES if n.startswith("impl_")])
def test_implicit_switched_off_is_im2col_and_gemm(K, monkeypatch, name):
    G, N, C1, C2, Cout, H, W, ks, view, want = WGRAD_CASES[name]
    in1_ns = 2 * C1 * H * W if view else None
    assert K.wgrad_plan(G, N, C1, C2, Cout, H, W, ks, in1_ns=in1_ns).form == "implicit"
    monkeypatch.setenv("RFN_WGRAD_IMPLICIT", "0")
    plan = K.wgrad_plan(G, N, C1, C2, Cout, H, W, ks, in1_ns=in1_ns)
    Nc = 9 * (C1 + C2)
    label = K.kernel_label(GEMM_QUERY, Cout, Nc, Cout * H * W, Nc * H * W, G, N, H * W)
    assert plan.form == "im2col" and (plan.M, plan.Nc) == (Cout, Nc)
    assert plan.launches == [("rfn_im2col3x3_f32", "im2col3x3")] * max(G, 1) + [
        (GEMM[1], label.replace("<", "<grouped ")) if G else (GEMM[0], label)]


F32_TAPS = (3, 16, 4, 6, 6)   # N, Cin, C, H, W of the fp32 case of test_wgrad_mirrored.py::test_plan_is_what_runs_...


def test_fp32_few_out_is_tap_scatter_and_the_fp32_kernel_as_1x1(K, monkeypatch):
    monkeypatch.setattr(K, "CONV_PRECISION", "f32")
    N, Cin, C, H, W = F32_TAPS
    for C in (1, 4, K.TAP_MAX_COUT):
        plan = K.wgrad_plan(0, N, Cin, 0, C, H, W, 3, few_out=True)
        assert plan.form == "scatter_f32" and (plan.M, plan.Nc) == (9 * C, Cin)
        assert plan.launches == [SCATTER, ("rfn_conv2d_wgrad_f32", K.kernel_label(F32_QUERY, 1, Cin, 9 * C, H, W))]


@pytest.mark.parametrize("C,few_out", [(4, False), (9, True), (9, False)])
def test_fp32_otherwise_is_the_fp32_kernel_and_its_finish(K, monkeypatch, C, few_out):
    monkeypatch.setattr(K, "CONV_PRECISION", "f32")
    N, Cin, _, H, W = F32_TAPS
    assert K.TAP_MAX_COUT == 8
    plan = K.wgrad_plan(0, N, Cin, 0, C, H, W, 3, few_out=few_out)
    assert plan.form == "f32"
    assert plan.launches == [("rfn_conv2d_wgrad_f32", K.kernel_label(F32_QUERY, 3, Cin, C, H, W)),
                             ("rfn_wgrad_finish_f32", "wgrad_finish")]
    # a single tap needs no finish
    assert K.wgrad_plan(0, N, Cin, 0, C, H, W, 1, few_out=few_out).launches == [
        ("rfn_conv2d_wgrad_f32", K.kernel_label(F32_QUERY, 1, Cin, C, H, W))]


GROUPED_SCATTER = (20, 20, 4, 2, 3, 4, 4)   # the unstacked group of the same test: rows of 4 pixels


@pytest.mark.parametrize("few_out", [False, True])
def test_a_group_scatters_once_when_stacked_else_once_per_gradient(K, few_out):
    G = GROUPED_SCATTER[3]
    stacked = _zeros_plan(K, GROUPED_SCATTER, few_out=few_out, stacked=True)
    apart = _zeros_plan(K, GROUPED_SCATTER, few_out=few_out, stacked=False)
    assert stacked.form == apart.form == "scatter"
    assert stacked.launches == _scatter_gemm(K, GROUPED_SCATTER, 1)
    assert apart.launches == _scatter_gemm(K, GROUPED_SCATTER, G)
    # (a single gradient has nothing to stack)
    single = GROUPED_SCATTER[:3] + (0,) + GROUPED_SCATTER[4:]
    assert _zeros_plan(K, single, few_out=few_out).launches == _scatter_gemm(K, single, 1)
