"""CPU-only: the kernel the library would launch, asked of the library itself.

The *_kernel_label_* queries of include/rfn_hip.h are answered by the C++ functions the launchers switch on
(choose_conv_b3, choose_conv_f32, choose_wgrad_f32, choose_gemm_wgrad, choose_wgrad_implicit) and need no device, so
the route tables that the GPU tests assert launch by launch (tests/test_conv_grad_model.py, test_conv_split_precision.py)
are checked here on any machine, through the same helper (rfn_hip.ops.kernel_label) and with the same arguments and
decorations (" x6", "+actbwd", "grouped ") the launch wrappers of rfn_hip/ops.py use."""
import pytest

from tests.test_conv_grad_model import ACTBWD_CASES, CONV_CASES, GEMM_CASES, WGRAD_CASES
from tests.test_conv_split_precision import FWD_CASES, X6_KERNELS
from tests.test_wgrad_routes_model import ALL_LABELS, BAND_ENTRY, EXACT_CASES, GEMM, ROUTE_CASES, assert_ring, grouped

B3, F32 = "rfn_conv2d_kernel_label_bf16x3", "rfn_conv2d_kernel_label_f32"


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    return ops


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_cases_take_their_table_route(K, name):
    N, C1, C2, Cout, H, W, ks, flip, label = CONV_CASES[name]
    assert K.kernel_label(B3, 2, ks, C1, C2, Cout, Cout, 0, 0, N, H, W) == label


@pytest.mark.parametrize("acc1", [0, 1])
@pytest.mark.parametrize("HW", [(16, 16), (12, 12)])
def test_conv1x1_ws_takes_split_and_accumulating_outputs(K, HW, acc1):
    """the shapes of test_conv1x1_ws_views_vs_model"""
    H, W = HW
    assert K.kernel_label(B3, 2, 1, 200, 0, 256, 100, acc1, 0, 16384 // (H * W) + 7, H, W) == "conv1x1_ws_kernel<16>"


@pytest.mark.parametrize("name", list(ACTBWD_CASES))
def test_actbwd_cases_take_their_table_route(K, name):
    N, Cmid, Cnext, H, W, ks, act, label = ACTBWD_CASES[name]
    assert K.kernel_label(B3, 2, ks, Cnext, 0, Cmid, Cmid, 0, 4, N, H, W) + "+actbwd" == label


# rfn_conv2d_dgrad_act_rows_bf16x3 for the ACTBWD_CASES shapes, as returned by the build that still derived the generic
# tile sizes by hand beside dispatch_conv_b3
ACTBWD_ROWS = {"ws3_16x16": 256, "ws3_16x32": 256, "ws3_4x16": 256, "ws1_16x16": 256, "g3_8x8": 6, "g3_4x16": 10,
               "g3_1x64": 300, "g1_4x4": 4}


def test_dgrad_act_rows_are_those_of_the_chosen_route():
    from rfn_hip import lib
    assert set(ACTBWD_ROWS) == set(ACTBWD_CASES)
    for name, (N, Cmid, Cnext, H, W, ks, act, label) in ACTBWD_CASES.items():
        assert lib.load().rfn_conv2d_dgrad_act_rows_bf16x3(N, H, W, ks, Cmid, Cnext) == ACTBWD_ROWS[name], name


def test_bf16x6_cases_take_the_generic_routes(K):
    labels = {K.kernel_label(B3, 3, ks, C1, C2, Cout, Cout, 0, 0, N, H, W) for N, C1, C2, Cout, H, W, ks in FWD_CASES}
    assert labels == X6_KERNELS
    # three planes never take a weight-stationary kernel, whatever the shape
    assert K.kernel_label(B3, 3, 1, 256, 0, 256, 256, 0, 0, 70, 16, 16) == "conv_b3_kernel<1,4,1,2,2,32>"
    assert K.kernel_label(B3, 3, 3, 8, 0, 256, 256, 0, 0, 70, 16, 16) == "conv_b3_kernel<3,2,2,1,2,16>"


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_cases_take_their_table_route(K, name):
    G, M, Nc, F_, H, W, view, tile = GEMM_CASES[name]
    HW = H * W
    a_ns, b_ns = (M + (8 if view else 0)) * HW, (Nc + (4 if view else 0)) * HW
    label = K.kernel_label("rfn_gemm_wgrad_kernel_label_bf16x3", M, Nc, a_ns, b_ns, G, F_, HW)
    assert (label.replace("<", "<grouped ") if G else label) == tile


@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_wgrad_cases_take_their_table_routes(K, name):
    """the launches K.conv2d_wgrad / K.conv2d_wgrad_grouped make are those of K.wgrad_plan, which needs no device (`view`:
    in1 is the channel slice z[:, :C1] of a tensor twice as wide -- its frame stride)"""
    G, N, C1, C2, Cout, H, W, ks, view, want = WGRAD_CASES[name]
    plan = K.wgrad_plan(G, N, C1, C2, Cout, H, W, ks, in1_ns=2 * C1 * H * W if view else None, stacked=bool(G))
    assert plan.launches == want


@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_route_model_cases_take_their_table_routes(K, name):
    """the cases of tests/test_wgrad_routes_model.py (mirrored, short rows, level split, and its restatements of the
    GEMM_CASES, WGRAD_CASES and band cases): the launches of K.wgrad_plan / the GEMM label query for the strides of the
    channel-slice views, and the workgroups of a grouped ring launch that change group in mid-range"""
    c = EXACT_CASES[name]
    HW = c.H * c.W
    in1_ns = (c.xview[0] if c.xview else c.C1) * HW
    g_ns = (c.gview[0] if c.gview else c.Cout) * HW
    if c.kind == "gemm":
        label = K.kernel_label("rfn_gemm_wgrad_kernel_label_bf16x3", c.Cout, c.C1, g_ns, in1_ns, c.G, c.N, HW)
        assert [(GEMM[1 if c.G else 0], grouped(label) if c.G else label)] == c.want
    elif c.kind == "band":
        assert [(BAND_ENTRY, K.kernel_label("rfn_conv3x3_wgrad_band_kernel_label_bf16x3", c.Cout, c.C1 + c.C2, c.N, c.H,
                                            c.W))] == c.want
    else:
        plan = K.wgrad_plan(c.G, c.N, c.C1, c.C2, c.Cout, c.H, c.W, c.ks, g_ns=g_ns, in1_ns=in1_ns,
                            few_out=c.kind == "zeros", stacked=bool(c.G) and c.gview is None, short_rows=c.short)
        assert plan.launches == c.want
    assert_ring(c)


def test_route_model_cases_cover_every_weight_gradient_label():
    """every label of kWgradB3Labels, single and grouped (a group never takes the 32-row implicit tiling), and the two of
    the band kernel: 31"""
    seen = {label for c in EXACT_CASES.values() for _, label in c.want if "wgrad" in label}
    assert seen == ALL_LABELS and len(ALL_LABELS) == 31, (sorted(seen - ALL_LABELS), sorted(ALL_LABELS - seen))
    assert all(c.ring is not None for n, c in ROUTE_CASES.items() if n.startswith(("split_", "mir_narrow")))


def test_fp32_1x1_between_65_and_128_outputs_takes_the_128_row_block(K):
    """rfn_conv2d_fwd_f32, 1x1, 64 < Cout <= 128, not few-pixel: one 128-row block (case 6 of its former switch), not the
    256-row tiling that the Python copy of this ladder used to report"""
    assert K.kernel_label(F32, 1, 128, 300, 12, 12) == "conv_mfma_kernel<1,2,2,2,2,32>"
    assert K.kernel_label(F32, 1, 65, 300, 12, 12) == "conv_mfma_kernel<1,2,2,2,2,32>"
    assert K.kernel_label(F32, 1, 129, 300, 12, 12) == "conv_mfma_kernel<1,4,1,2,2,32>"
    assert K.kernel_label(F32, 1, 128, 7, 6, 6) == "conv_mfma_kernel<1,4,1,1,1,32>"     # few pixels
    assert K.kernel_label(F32, 1, 64, 300, 12, 12) == "conv_mfma_kernel<1,1,4,2,1,32>"
    assert K.kernel_label(F32, 3, 128, 300, 12, 12) == "conv_mfma_kernel<3,2,2,2,2,8>"
