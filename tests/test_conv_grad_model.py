"""The bf16x3 gradient convolutions against an exact restatement of their arithmetic.

Every data gradient, every weight gradient and the forward convolutions on 2x2 maps split each fp32 operand into
    hi = bf16(v),  lo = bf16(v - hi)            (round to nearest even; torch: v.bfloat16().float(), bit for bit)
and form  a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi  on three bf16 MFMAs with fp32 accumulation.  Products of bf16 numbers
are exact in fp32, so a correct kernel computes
    y3 = op(a_hi, b_hi + b_lo) + op(a_lo, b_hi)                                   (model64 below, fp64 on the CPU)
up to fp32 ACCUMULATION error only.  Against y3 a single mis-staged plane element (2^-9 of one product) is visible
at any K; against exact fp64 it hides below the representation error of the split.  Measures, as in
test_conv_split_precision:  e_abs = max over outputs of |y - ref| / S,  S = op(|a|, |b|) in fp64.

Per case:
  vs the model  e_abs <= 3 * e_abs(fp32-MFMA kernel of the same operation, same inputs, vs exact fp64) + 2e-8
                (the form the forward test holds bf16x6 to); convolutions (K <= 4608) also <= 4e-7, the project's
                fp32-grade cap; weight gradients (K = 10^3 .. 1.4*10^5, float-atomic partial sums) <= WGRAD_CAP
  vs exact fp64 e_abs <= 1.25 * 2^-16 + 4e-7: each operand keeps 16 significant bits, |v - hi - lo| <= 2^-17 |v|,
                so the two operands contribute 2 * 2^-17, the dropped lo*lo product 2^-9 * 2^-9 = 2^-18, plus
                accumulation.  A model that silently matched a wrong kernel cannot satisfy this one.
  magnitude     data gradients: the input times 2^k, k in {-40, -12, +12}, gives the output times 2^k BIT FOR BIT
                (bf16 keeps the fp32 exponent; the kernels add in a fixed order).  Weight gradients end in float atomics
                and are exempt; they are held to the model tolerance at k = -40.
  route         the label of every launch (the library's own answer: rfn_hip.ops.kernel_label) equals the table entry
                written here from the C++ choices (choose_conv_b3, choose_gemm_wgrad, choose_wgrad_implicit); the set of
                table entries equals ROUTES; tests/test_kernel_routes_host.py asks the same without a device.  profiles/conv_grad_model_kernel_symbols.txt is the list of
                kernel symbols a traced run of this module launched: the device-side confirmation of the table.

Measured on an MI355X (max over the cases of a route; e_abs of bf16x3 vs the model / bf16x3 vs fp64 / fp32 kernel vs fp64):
  data gradients / 2x2-forward convolutions (K = 21 .. 2304)
    conv_b3_kernel<3,1,4,1,1,16>                     9.7e-8 / 3.0e-6 / 2.8e-7
    conv_b3_kernel<3,2,2,1,1,16>  (split-K too)      1.2e-7 / 4.2e-6 / 2.6e-7
    conv_b3_kernel<3,2,2,1,2,16>  (1x64 map too)     2.0e-7 / 9.6e-6 / 3.2e-7
    conv_b3_kernel<1,1,4,1,1,32>                     8.1e-8 / 4.2e-6 / 1.5e-7
    conv_b3_kernel<1,2,2,1,1,32>  (split-K too)      9.9e-8 / 8.1e-6 / 2.6e-7
    conv_b3_kernel<1,2,2,2,2,32>                     1.5e-7 / 5.0e-6 / 2.5e-7
    conv_b3_kernel<1,4,1,2,2,32>                     1.2e-7 / 1.8e-6 / 3.2e-7
    conv1x1_ws_kernel<16>         (4 cases)          1.9e-7 / 3.5e-6 / 3.6e-7
    conv1x1_ws_kernel<16>         (views, 8 cases)   1.8e-7 / 2.5e-6 / 3.9e-7
    conv3x3_ws_kernel<3,2,1>      (10 maps)          2.7e-7 / 6.8e-6 / 4.4e-7
    conv3x3_ws_kernel<5,1,1>      (10 maps)          2.3e-7 / 3.7e-6 / 3.9e-7
    conv3x3_ws_kernel<1,2,0>+actbwd                  1.3e-7 / 9.4e-6 / 3.9e-7
    conv1x1_ws_kernel<16>+actbwd                     1.7e-7 / 2.3e-6 / 3.4e-7
    conv_b3_kernel<3,2,2,1,1,16>+actbwd              3.7e-8 / 5.4e-6 / 2.4e-7
    conv_b3_kernel<3,2,2,1,2,16>+actbwd (1x64 map)   1.1e-7 / 1.0e-5 / 3.0e-7
    conv_b3_kernel<1,2,2,1,1,32>+actbwd              1.5e-8 / 3.5e-6 / 2.4e-7
    the two per-channel sums of +actbwd              1.5e-9 .. 1.7e-8 of their scale (tolerance 9e-7 .. 2.0e-6)
    dgrad_small_kernel            (11 shapes)        8.8e-8 / 2.0e-6 / 2.6e-7
  weight gradients (K = 756 .. 134144; single / grouped)
    gemm_wgrad_dma_kernel<2,4,4,2,32,2>              1.1e-8 / 8.4e-8 / 1.2e-8     1.3e-8 / 1.7e-7 / 2.1e-8
    gemm_wgrad_dma_kernel<1,8,2,1,32,3>              1.5e-8 / 8.7e-8 / 2.5e-8     2.2e-8 / 3.8e-7 / 4.0e-8  (G = 16)
    gemm_wgrad_b3_kernel<4,2,2,3,64>                 1.3e-8 / 1.1e-7 / 1.3e-8     9.8e-9 / 1.1e-7 / 1.6e-8
    gemm_wgrad_b3_kernel<2,4,4,2,64>                 1.4e-8 / 9.2e-8 / 1.3e-8     1.3e-8 / 1.1e-7 / 1.5e-8
    gemm_wgrad_b3_kernel<1,4,2,2,32>                 1.9e-8 / 2.6e-7 / 3.9e-8     1.9e-8 / 2.9e-7 / 3.5e-8
      after im2col3x3 (vector and scalar kernel)     3.8e-8 / 1.1e-6 / 4.8e-8     3.9e-8 / 1.2e-6 / 4.2e-8
    gemm_wgrad_b3_kernel<4,1,2,2,32>                 2.8e-8 / 2.7e-7 / 2.9e-8     2.4e-8 / 2.7e-7 / 3.2e-8
      after tap_scatter                              2.7e-8 / 7.9e-7 / 3.7e-8     3.0e-8 / 8.6e-7 / 4.2e-8
    gemm_wgrad_b3_kernel<2,2,2,2,64>                 1.8e-8 / 2.7e-7 / 3.4e-8     2.5e-8 / 4.9e-7 / 3.8e-8
    gemm_wgrad_dma_impl_kernel<4,2,2,3>              1.4e-8 / 9.7e-8 / 1.8e-8     1.5e-8 / 1.6e-7 / 3.2e-8
    gemm_wgrad_b3_kernel<4,2,2,3,64,1>               1.6e-8 / 1.1e-7 / 2.0e-8     1.3e-8 / 1.2e-7 / 1.7e-8
    gemm_wgrad_b3_kernel<1,4,1,2,32,1>               2.3e-8 / 6.9e-7 / 4.2e-8     (a group takes <2,2,2,2,64,1>)
    gemm_wgrad_b3_kernel<2,2,2,2,64,1>               3.3e-8 / 6.6e-7 / 3.4e-8     4.5e-8 / 9.0e-7 / 4.4e-8
    wgrad_mfma_kernel<3,4,1,1,1,64> (fp32, 3x5 map)  1.9e-7 vs fp64
  Weight gradients over seeds 0, 1, 2 of every case: largest e_abs vs the model 4.81e-8 (a group of 24 x 126
  gradients on 8x24 maps), at gradient * 2^-40 4.75e-8; WGRAD_CAP = 9.7e-8 is twice that.  The fp32-MFMA weight gradient
  on the same inputs: at most 5.9e-8.  SPLIT_BOUND = 1.95e-5; the largest e_abs vs fp64 seen is 1.0e-5.
Wall time of the module on the MI355X machine: 17.8 s, of which the CPU fp64 references 10.4 s and everything else
(input generation, transfers, 617 launches of the package's kernels) 7.4 s.

Two deliberate faults, each in a scratch build (not committed), e_abs vs the model of the affected cases:
  A  the `lo` plane of the last real 8-channel k-group zeroed in conv_b3_kernel<3,2,2,1,2,16>: g3_many_64x64 8.3e-4,
     g3_many_12x12 5.1e-4, g3_1x64_cin8 2.1e-3, actbwd g3_1x64 2.6e-3: all four cases of that instantiation fail, none
     of the other 91.  The existing checks at 2e-5 relative (test_conv2d_fwd_dgrad_wgrad, the fused activation backward,
     the weight-gradient tests) all PASS under this fault; the one existing failure is the cross-kernel comparison of
     test_dgrad_small_rows at 609 frames of 8x8 (relerr 2.8e-4), the only place that instantiation met K = 2304.
  B  edgemask dropped from the implicit 3x3 staging (both gemm_wgrad_b3_kernel<..,1> and gemm_wgrad_dma_impl_kernel):
     impl_dma 3.7e-3, impl_dma_g3 6.1e-3, impl_256x192 8.4e-3, its group 9.8e-3, impl_32x256 4.3e-2, impl_32rows_g3
     4.0e-2, impl_128x128 6.9e-2, its group 6.0e-2: all eight implicit cases fail, nothing else.  A whole border tap is
     a gross fault: the existing suite fails on it too (28 cases of test_conv2d_fwd_dgrad_wgrad,
     test_conv2d_wgrad_grouped and test_conv3x3_wgrad_implicit_big).
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_split_precision import frame_slices
from tests.test_dgrad_small_rows import HALF, SHAPES as SMALL_SHAPES

pytestmark = pytest.mark.gpu

SPLIT_BOUND = 1.25 * 2.0 ** -16 + 4e-7   # vs exact fp64 (derived in the module docstring)
FP32_CAP = 4e-7                          # the project's fp32-grade cap for convolutions with K <= 4608
WGRAD_CAP = 9.7e-8                       # weight gradients vs the model: twice the largest of three seeds (4.81e-8)
SCALES = (-40, -12, 12)
EW = 4 * 2.0 ** -24                      # expf + two fp32 products of the fused activation backward, relative to |gu|


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    assert ops.bwd_b3(), "the gradient arithmetic under test is bf16x3 (RFN_CONV_PRECISION mixed or bf16x3)"
    return ops


@pytest.fixture
def launches(monkeypatch):
    """(entry point, label = meta[1]) of every labelled launch, recorded through rfn_hip.lib.call"""
    from rfn_hip import lib
    seen = []
    orig = lib.call

    def call(name, *args, meta=None):
        if meta is not None:
            seen.append((name, meta[1]))
        return orig(name, *args, meta=meta)
    monkeypatch.setattr(lib, "call", call)
    return seen


# ------------------------------------------------------------------------------------------------ model and measures
def split(x):
    """the kernels' (hi, lo): h = (__bf16)v; lo = (__bf16)(v - (float)h)"""
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def model64(a, b, op):
    """the three-product sum a_hi*b_hi + a_hi*b_lo + a_lo*b_hi of a bilinear `op`, in fp64"""
    ah, al = split(a)
    bh, bl = split(b)
    return op(ah.double(), bh.double() + bl.double()) + op(al.double(), bh.double())


def refs64(a, b, op):
    """(model y3, exact fp64, S = op(|a|, |b|))"""
    return model64(a, b, op), op(a.double(), b.double()), op(a.double().abs(), b.double().abs())


def e_abs(y, ref, s):
    return float(((y.detach().cpu().double() - ref).abs() / (s + 1e-300)).max())


def conv_op(ks):
    return lambda x, w: F.conv2d(x, w, padding=ks // 2)


def gemm64(a, b):
    """sum over frames and pixels of a[f,m,p] * b[f,n,p] in fp64, a few frames at a time"""
    out = torch.zeros(a.shape[1], b.shape[1], dtype=torch.float64)
    step = max(1, (1 << 22) // (max(a.shape[1], b.shape[1]) * a[0, 0].numel()))
    for f in range(0, a.shape[0], step):
        A = a[f:f + step].double().flatten(2).transpose(0, 1).flatten(1)
        B = b[f:f + step].double().flatten(2).transpose(0, 1).flatten(1)
        out += A @ B.t()
    return out


def wgrad_op(ks):
    """weight gradient of conv2d(x, w, padding=ks//2) as a bilinear op(g, x) -> [Cout, Cin, ks, ks]"""
    def op(g, x):
        if ks == 1:
            return gemm64(g, x).view(g.shape[1], x.shape[1], 1, 1)
        H, W = x.shape[2:]
        xp = F.pad(x, (1, 1, 1, 1))
        gw = torch.empty(g.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
        for dy in range(3):
            for dx in range(3):
                gw[:, :, dy, dx] = gemm64(g, xp[:, :, dy:dy + H, dx:dx + W])
        return gw
    return op


def check(what, fig, cap=None):
    """the assertions every case ends in; fig = {"model", "fp64", "f32"} (e_abs maxima)"""
    msg = "%s: e_abs vs model %.3g, vs fp64 %.3g, f32 kernel vs fp64 %.3g" % (what, fig["model"], fig["fp64"], fig["f32"])
    print(msg)
    assert fig["model"] <= 3 * fig["f32"] + 2e-8, msg
    if cap is not None:
        assert fig["model"] <= cap, msg
    assert fig["fp64"] <= SPLIT_BOUND, msg


# ------------------------------------------------------------------------------------------------ 1. convolutions
G3 = "conv_b3_kernel<3,%s,16>"
G1 = "conv_b3_kernel<1,%s,32>"
WS1 = "conv1x1_ws_kernel<16>"
WS3A, WS3B = "conv3x3_ws_kernel<3,2,1>", "conv3x3_ws_kernel<5,1,1>"

# name: (N, C1, C2, Cout, H, W, ks, flip, label).  flip: the weight is packed as a data gradient's (transposed, taps
# mirrored), i.e. the call is the data gradient of a conv Cout -> C1 + C2.  The label is what choose_conv_b3 must
# choose: few_px = N*H*W*ceil(Cout/128) < 32768; 1x1 ws: one source, Cout % 256 == 0, 128 < Cin <= 256, >= 16384 pixels;
# 3x3 ws: Cout % 256 == 0, H and W powers of two, W >= 8, H*W >= 64, H >= TH, >= 16384 pixels, Cin <= 24 -> <3,2>
# (64-pixel tiles, TH = 64 / min(W, 32)), Cin <= 40 -> <5,1> (32-pixel tiles, TH = 32 / min(W, 32)).
CONV_CASES = {
    # the seven generic instantiations at npl == 2
    "g3_cout16_64x64":      (4, 16, 0, 16, 64, 64, 3, True, G3 % "1,4,1,1"),     # Cout <= 32, two column tiles
    "g3_few_2src_6x6":      (3, 3, 5, 40, 6, 6, 3, False, G3 % "2,2,1,1"),       # source boundary inside a group, Cin 8
    "g3_few_3x5":           (37, 24, 0, 96, 3, 5, 3, True, G3 % "2,2,1,1"),      # partial frame tile
    "g3_many_64x64":        (9, 16, 0, 64, 64, 64, 3, True, G3 % "2,2,1,2"),     # 36864 pixels
    "g3_many_12x12":        (230, 20, 0, 48, 12, 12, 3, False, G3 % "2,2,1,2"),  # ragged 16x8 tiles, Cin % 16 != 0
    "g3_2src_8x8":          (5, 4, 14, 256, 8, 8, 3, True, G3 % "2,2,1,1"),      # two cout blocks; 320 pixels: no ws
    "g1_cout24_3x5":        (5, 40, 0, 24, 3, 5, 1, False, G1 % "1,4,1,1"),
    "g1_cout64_12x12":      (6, 100, 0, 64, 12, 12, 1, True, G1 % "2,2,1,1"),
    "g1_few_cout130":       (7, 21, 0, 130, 6, 6, 1, False, G1 % "2,2,1,1"),     # partial cout block, Cin 21
    "g1_cout128_12x12":     (300, 64, 0, 128, 12, 12, 1, True, G1 % "2,2,2,2"),  # 43200 pixels
    "g1_cout288_4x4":       (800, 256, 0, 288, 4, 4, 1, False, G1 % "4,1,2,2"),  # Cout % 256 != 0: not the ws kernel
    # split-K (fewer than 128 workgroups, >= 8 k-chunks, plain output): bitwise repeatability is checked too
    "g3_splitk_4x4":        (4, 256, 0, 512, 4, 4, 3, True, G3 % "2,2,1,1"),
    "g1_splitk_4x4":        (6, 300, 0, 200, 4, 4, 1, True, G1 % "2,2,1,1"),     # Cin 300: 10 chunks of 32
    # 1 x W maps: TH = 2 > H for the 64-pixel-tile variant -> generic kernel (the predicate fix); 2 x 64 has one tile row
    "g3_1x64_cin8":         (300, 8, 0, 256, 1, 64, 3, True, G3 % "2,2,1,2"),
    "ws3a_2x64":            (130, 8, 0, 256, 2, 64, 3, True, WS3A),
    "ws3b_1x64":            (300, 30, 0, 256, 1, 64, 3, False, WS3B),            # 32-pixel tiles: TH = 1, still served
    # weight-stationary 1x1
    "ws1_256_16x16":        (70, 256, 0, 256, 16, 16, 1, True, WS1),
    "ws1_cin200_12x12":     (131, 200, 0, 256, 12, 12, 1, True, WS1),            # 18864 pixels: ragged last 32-pixel tile
    "ws1_cin129_cout512":   (70, 129, 0, 512, 16, 16, 1, False, WS1),
    "ws1_cin200_cout512":   (115, 200, 0, 512, 12, 12, 1, True, WS1),
    # weight-stationary 3x3, 27-unit variant (Cin <= 24): n_tiles = N*H*W/64 is never a multiple of 256
    "ws3a_32x32":           (17, 2, 16, 256, 32, 32, 3, False, WS3A),            # 272 tiles; 2 + 16 sources
    "ws3a_16x16":           (70, 3, 15, 256, 16, 16, 3, True, WS3A),             # 280; boundary inside a group
    "ws3a_8x8":             (300, 10, 0, 256, 8, 8, 3, True, WS3A),              # 300
    "ws3a_16x32":           (33, 24, 0, 256, 16, 32, 3, True, WS3A),             # 264
    "ws3a_32x16":           (33, 5, 12, 256, 32, 16, 3, False, WS3A),
    "ws3a_8x64":            (33, 8, 0, 512, 8, 64, 3, True, WS3A),               # two tiles per image row, two cout blocks
    "ws3a_64x8":            (33, 12, 0, 256, 64, 8, 3, True, WS3A),
    "ws3a_4x16":            (257, 6, 12, 256, 4, 16, 3, True, WS3A),             # one tile = one frame
    "ws3a_2x32":            (259, 20, 0, 256, 2, 32, 3, False, WS3A),
    # 45-unit variant (24 < Cin <= 40): n_tiles = N*H*W/32
    "ws3b_32x32":           (17, 4, 32, 256, 32, 32, 3, False, WS3B),
    "ws3b_16x16":           (70, 5, 30, 256, 16, 16, 3, True, WS3B),             # boundary inside a group
    "ws3b_8x8":             (300, 40, 0, 256, 8, 8, 3, True, WS3B),
    "ws3b_16x32":           (33, 25, 0, 256, 16, 32, 3, True, WS3B),
    "ws3b_32x16":           (33, 3, 30, 512, 32, 16, 3, False, WS3B),
    "ws3b_8x64":            (33, 32, 0, 256, 8, 64, 3, True, WS3B),
    "ws3b_64x8":            (33, 36, 0, 256, 64, 8, 3, True, WS3B),
    "ws3b_4x16":            (257, 7, 26, 256, 4, 16, 3, True, WS3B),
    "ws3b_2x32":            (259, 28, 0, 256, 2, 32, 3, False, WS3B),
}
SPLITK = ("g3_splitk_4x4", "g1_splitk_4x4")


def conv_inputs(case, seed):
    N, C1, C2, Cout, H, W, ks, flip, _ = case
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(N, C1, H, W, generator=g)
    x2 = torch.randn(N, C2, H, W, generator=g) if C2 else None
    wl = torch.randn(Cout, C1 + C2, ks, ks, generator=g) / ((C1 + C2) * ks * ks) ** 0.5  # the conv the kernel computes
    wu = wl.transpose(0, 1).flip(2, 3).contiguous() if flip else wl                        # what the caller packs
    return x1, x2, wl, wu


def conv_figures(y3, yf, x, wl, ks):
    """e_abs maxima over frame_slices of a convolution output y3 (bf16x3) and yf (fp32 MFMA)"""
    fig = {"model": 0.0, "fp64": 0.0, "f32": 0.0}
    for sl in frame_slices(x.shape[0]):
        ym, y64, s = refs64(x[sl], wl, conv_op(ks))
        for k, (y, ref) in {"model": (y3, ym), "fp64": (y3, y64), "f32": (yf, y64)}.items():
            fig[k] = max(fig[k], e_abs(y[sl], ref, s))
    return fig


def run_conv_case(K, launches, name, seed=0):
    case = CONV_CASES[name]
    N, C1, C2, Cout, H, W, ks, flip, label = case
    x1, x2, wl, wu = conv_inputs(case, 1000 + seed)
    x1d, x2d, wd = x1.cuda(), None if x2 is None else x2.cuda(), wu.cuda()
    wp3, wpf = K.pack_weight(wd, flip=flip, prec="bf16x3"), K.pack_weight(wd, flip=flip, prec="f32")
    n0 = len(launches)
    y3 = K.conv2d_raw(x1d, x2d, wp3, Cout, ks, prec="bf16x3")
    assert launches[n0:] == [("rfn_conv2d_fwd_bf16x3", label)], (name, launches[n0:])
    yf = K.conv2d_raw(x1d, x2d, wpf, Cout, ks, prec="f32")
    for k in SCALES:
        yk = K.conv2d_raw(x1d * 2.0 ** k, None if x2d is None else x2d * 2.0 ** k, wp3, Cout, ks, prec="bf16x3")
        assert torch.equal(yk, y3 * 2.0 ** k), (name, "input * 2^%d" % k)
    if name in SPLITK:
        assert torch.equal(K.conv2d_raw(x1d, x2d, wp3, Cout, ks, prec="bf16x3"), y3), (name, "split-K repeatability")
    x = x1 if x2 is None else torch.cat([x1, x2], 1)
    return conv_figures(y3.cpu(), yf.cpu(), x, wl, ks)


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_vs_model(K, launches, name):
    fig = run_conv_case(K, launches, name)
    assert (CONV_CASES[name][1] + CONV_CASES[name][2]) * CONV_CASES[name][6] ** 2 <= 4608
    check(name, fig, cap=FP32_CAP)


@pytest.mark.parametrize("acc1,acc2", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("HW", [(16, 16), (12, 12)])
def test_conv1x1_ws_views_vs_model(K, launches, HW, acc1, acc2):
    """conv1x1_ws_kernel<16> with everything its full epilogue accepts: the input a channel slice of a wider tensor, the
    output split over two channel-slice views (the split inside a wave's 32 channels), each accumulate combination;
    the channels outside the views stay untouched"""
    H, W = HW
    N, Cin, Cout, sp = 16384 // (H * W) + 7, 200, 256, 100
    g = torch.Generator().manual_seed(31)
    wide = torch.randn(N, Cin + 16, H, W, generator=g)
    wl = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    wu = wl.transpose(0, 1).contiguous()
    big1 = torch.randn(N, sp + 5, H, W, generator=g)
    big2 = torch.randn(N, Cout - sp + 3, H, W, generator=g)
    x = wide[:, 8:8 + Cin]
    wd, xd = wu.cuda(), wide.cuda()[:, 8:8 + Cin]
    ys = {}
    for prec in ("bf16x3", "f32"):
        b1, b2 = big1.cuda(), big2.cuda()
        n0 = len(launches)
        K.conv2d_raw(xd, None, K.pack_weight(wd, flip=True, prec=prec), Cout, 1, out1=b1[:, 2:2 + sp],
                     out2=b2[:, :Cout - sp], cout_split=sp, acc1=acc1, acc2=acc2, prec=prec)
        if prec == "bf16x3":
            assert launches[n0:] == [("rfn_conv2d_fwd_bf16x3", WS1)], launches[n0:]
        b1, b2 = b1.cpu(), b2.cpu()
        assert torch.equal(b1[:, :2], big1[:, :2]) and torch.equal(b1[:, 2 + sp:], big1[:, 2 + sp:]), prec
        assert torch.equal(b2[:, Cout - sp:], big2[:, Cout - sp:]), prec
        ys[prec] = torch.cat([b1[:, 2:2 + sp], b2[:, :Cout - sp]], 1)
    base = torch.cat([big1[:, 2:2 + sp] * float(acc1), big2[:, :Cout - sp] * float(acc2)], 1).double()
    fig = {"model": 0.0, "fp64": 0.0, "f32": 0.0}
    for sl in frame_slices(N):
        ym, y64, s = refs64(x[sl], wl, conv_op(1))
        s = s + base[sl].abs()   # out = base + conv: the base enters the error scale
        for k, (y, ref) in {"model": (ys["bf16x3"], ym), "fp64": (ys["bf16x3"], y64), "f32": (ys["f32"], y64)}.items():
            fig[k] = max(fig[k], e_abs(y[sl], ref + base[sl], s))
    check("ws1 views %dx%d acc %d%d" % (H, W, acc1, acc2), fig, cap=FP32_CAP)


# fused activation backward (rfn_conv2d_dgrad_act_bf16x3): name: (N, Cmid, Cnext, H, W, ks, act, label).  The call is
# the data gradient of a conv Cmid -> Cnext, so the kernel's Cin is Cnext and its Cout is Cmid.  3x3 ws variant:
# Cnext <= 8, Cmid % 256 == 0, power-of-two map, >= 16384 pixels; 1x1 ws: 128 < Cnext <= 256, Cmid % 256 == 0.
ACTBWD_CASES = {
    "ws3_16x16":   (70, 256, 8, 16, 16, 3, 2, "conv3x3_ws_kernel<1,2,0>+actbwd"),
    "ws3_16x32":   (35, 256, 4, 16, 32, 3, 1, "conv3x3_ws_kernel<1,2,0>+actbwd"),    # 280 tiles, non-square
    "ws3_4x16":    (257, 512, 6, 4, 16, 3, 2, "conv3x3_ws_kernel<1,2,0>+actbwd"),    # two cout blocks
    "ws1_16x16":   (70, 256, 256, 16, 16, 1, 2, WS1 + "+actbwd"),
    "g3_8x8":      (3, 64, 6, 8, 8, 3, 2, G3 % "2,2,1,1" + "+actbwd"),
    "g3_4x16":     (5, 128, 12, 4, 16, 3, 1, G3 % "2,2,1,1" + "+actbwd"),            # Cnext > 8: never the ws kernel
    "g3_1x64":     (300, 256, 8, 1, 64, 3, 2, G3 % "2,2,1,2" + "+actbwd"),           # TH = 2 > H (the predicate fix)
    "g1_4x4":      (5, 128, 64, 4, 4, 1, 1, G1 % "2,2,1,1" + "+actbwd"),
}


@pytest.mark.parametrize("name", list(ACTBWD_CASES))
def test_dgrad_act_vs_model(K, launches, name):
    """g = conv(go, w^T) -> gu = g * act'(y) * exp(l) and the per-channel sums  Σ gu,  Σ g*y.  gu against the model
    followed by the fp32 elementwise backward (expf and two products: 4 * 2^-24 of |gu| on top); the sums (float
    atomics) against fp64 sums of the model with the error scale  Σ S*|factor|  and, on top of the per-term tolerance,
    2^-24 * sqrt(n/32 + 32) for the fp32 summation of the n terms of a channel: the random-walk figure of a serial chain
    of one partial per 32 pixels (a half wave reduces its 32 pixels by a tree before its partial meets the others in
    LDS and float atomics) plus the tree; a lost tile share is 1/256 of the terms, 6e-5 on this scale."""
    N, Cmid, Cnext, H, W, ks, act, label = ACTBWD_CASES[name]
    g = torch.Generator().manual_seed(33)
    go = torch.randn(N, Cnext, H, W, generator=g)
    w = torch.randn(Cnext, Cmid, ks, ks, generator=g) / (Cnext * ks * ks) ** 0.5   # forward weight of Cmid -> Cnext
    wl = w.transpose(0, 1).flip(2, 3).contiguous()
    pre = torch.randn(N, Cmid, H, W, generator=g)
    y = F.relu(pre) if act == 1 else F.leaky_relu(pre, 0.2)
    logs = torch.randn(Cmid, generator=g) * 0.2
    god, wd, yd, ld = go.cuda(), w.cuda(), y.cuda(), logs.cuda()
    wp3 = K.pack_weight(wd, flip=True, prec="bf16x3")
    n0 = len(launches)
    gu, gb, gl = K.conv2d_dgrad_act(god, wp3, yd, ld, act, Cmid, ks)
    assert launches[n0:] == [("rfn_conv2d_dgrad_act_bf16x3", label)], launches[n0:]
    gf = K.conv2d_raw(god, None, K.pack_weight(wd, flip=True, prec="f32"), Cmid, ks, prec="f32")
    for k in SCALES:
        guk = K.conv2d_dgrad_act(god * 2.0 ** k, wp3, yd, ld, act, Cmid, ks)[0]
        assert torch.equal(guk, gu * 2.0 ** k), (name, "gradient * 2^%d" % k)
    gm, g64, s = refs64(go, wl, conv_op(ks))    # every frame: the sums run over all of them
    slope = torch.where(y > 0, 1.0, 0.0 if act == 1 else 0.2).double()
    fac = slope * logs.double().exp().view(1, -1, 1, 1)
    gu, gb, gl, gf = gu.cpu().double(), gb.cpu().double(), gl.cpu().double(), gf.cpu()
    assert bool((gu[fac == 0] == 0).all())
    fig = {"f32": e_abs(gf, g64, s)}
    for k, ref in (("model", gm), ("fp64", g64)):
        d = ((gu - ref * fac).abs() - EW * (ref * fac).abs()).clamp_min(0.0)
        fig[k] = float((d / (s * fac + 1e-300))[fac != 0].max())
    check("actbwd " + name, fig, cap=FP32_CAP)
    tol = min(3 * fig["f32"] + 2e-8, FP32_CAP) + 2.0 ** -24 * (N * H * W / 32 + 32) ** 0.5
    for what, got, term, scale in (("sum gu", gb, gm * fac, s * fac), ("sum g*y", gl, gm * y.double(), s * y.double().abs())):
        e = float(((got - term.sum((0, 2, 3))).abs() / scale.sum((0, 2, 3))).max())
        print("actbwd %s %s: e_abs %.3g (tolerance %.3g)" % (name, what, e, tol))
        assert e <= tol, (name, what, e, tol)


@pytest.mark.parametrize("N,Cin,Cout,S", SMALL_SHAPES)
def test_smallcout_dgrad_vs_model(K, launches, N, Cin, Cout, S):
    """rfn_conv3x3_smallcout_bf16x3 at the shapes of test_dgrad_small_rows (its layout tests stay there): the same
    three-product arithmetic with the x-shift done on the accumulators"""
    assert K.dgrad_small_ok(N, Cin, Cout, S, S, 3)
    g = torch.Generator().manual_seed(1000 * S + Cout)
    x = torch.randn(N, Cin, S, S, generator=g)
    w = torch.randn(Cin, Cout, 3, 3, generator=g) * 0.05   # forward weight of a conv Cout -> Cin
    wl = w.transpose(0, 1).flip(2, 3).contiguous()
    sp = HALF[Cout]
    xd, wd = x.cuda(), w.cuda()
    wp3 = K.pack_weight(wd, flip=True, prec="bf16x3")

    def small(xin):
        o1 = torch.empty(N, sp, S, S, device="cuda")
        o2 = torch.empty(N, Cout - sp, S, S, device="cuda")
        K.conv3x3_smallcout(xin, wp3, Cout, o1, o2, sp, False, False)
        return torch.cat([o1, o2], 1)
    n0 = len(launches)
    y3 = small(xd)
    assert launches[n0:] == [("rfn_conv3x3_smallcout_bf16x3", "dgrad_small_kernel")], launches[n0:]
    yf = K.conv2d_raw(xd, None, K.pack_weight(wd, flip=True, prec="f32"), Cout, 3, prec="f32")
    for k in SCALES:
        assert torch.equal(small(xd * 2.0 ** k), y3 * 2.0 ** k), "gradient * 2^%d" % k
    assert Cin * 9 <= 4608
    check("smallcout N%d %d->%d %dx%d" % (N, Cin, Cout, S, S), conv_figures(y3.cpu(), yf.cpu(), x, wl, 3), cap=FP32_CAP)


# ------------------------------------------------------------------------------------------------ 2. weight gradients
DMA, B3 = "gemm_wgrad_dma_kernel<%s>", "gemm_wgrad_b3_kernel<%s>"
GEMM = ("rfn_gemm_wgrad_bf16x3", "rfn_gemm_wgrad_grouped_bf16x3")

# plain GEMM gradients gw[M][Nc] = Σ a b^T (K.gemm_wgrad / K.gemm_wgrad_grouped).  name: (G, M, Nc, F, H, W, view, tile).
# view: the operands are channel slices of wider tensors (a_ns = (M + 8) * HW, b_ns = (Nc + 4) * HW).  choose_gemm_wgrad:
# the DMA ring needs HW % 32 == 0, G * F*HW >= 100000, F*HW >= 2048, Nc % 256 == 0 and M >= 192 (256x256) or M <= 64
# (64x256); `big` = M > 128, Nc > 128, F*HW >= 100000 -> 256x192 when ceil(Nc/192)*192 < ceil(Nc/256)*256, else 256x256;
# then M <= 64 -> 64x256, Nc <= 64 -> 256x64, else 128x128.  6x6 maps: HW = 36 keeps the DMA ring out, F*HW is not a
# multiple of the 32- / 64-pixel stage.  No tile divides M or Nc.
GEMM_CASES = {
    "dma256":        (0, 200, 256, 131, 32, 32, True, DMA % "2,4,4,2,32,2"),   # 4192 stages: uneven shares
    "dma256_g3":     (3, 200, 256, 41, 32, 32, True, DMA % "grouped 2,4,4,2,32,2"),
    "dma64":         (0, 36, 256, 99, 32, 32, False, DMA % "1,8,2,1,32,3"),
    "dma64_g16":     (16, 36, 256, 7, 32, 32, True, DMA % "grouped 1,8,2,1,32,3"),
    "r256x192":      (0, 200, 162, 2801, 6, 6, False, B3 % "4,2,2,3,64"),
    "r256x192_g3":   (3, 200, 162, 2801, 6, 6, True, B3 % "grouped 4,2,2,3,64"),
    "r256x256":      (0, 144, 250, 2801, 6, 6, True, B3 % "2,4,4,2,64"),
    "r256x256_g3":   (3, 144, 250, 2801, 6, 6, False, B3 % "grouped 2,4,4,2,64"),
    "r64x256":       (0, 40, 200, 301, 6, 6, True, B3 % "1,4,2,2,32"),
    "r64x256_g3":    (3, 40, 200, 301, 6, 6, False, B3 % "grouped 1,4,2,2,32"),
    "r256x64":       (0, 200, 50, 301, 6, 6, False, B3 % "4,1,2,2,32"),
    "r256x64_g3":    (3, 200, 50, 301, 6, 6, True, B3 % "grouped 4,1,2,2,32"),
    "r128x128":      (0, 100, 130, 301, 6, 6, True, B3 % "2,2,2,2,64"),
    "r128x128_g3":   (3, 100, 130, 301, 6, 6, False, B3 % "grouped 2,2,2,2,64"),
}

IMPL = ("rfn_conv3x3_wgrad_implicit_bf16x3", "rfn_conv3x3_wgrad_implicit_grouped_bf16x3")
# convolution weight gradients (K.conv2d_wgrad / K.conv2d_wgrad_grouped).  name: (G, N, C1, C2, Cout, H, W, ks, view,
# launches).  view: in1 is a channel slice z[:, :C1] of a tensor twice as wide.  3x3 with Cin <= Cout and W % 8 == 0 is
# implicit (choose_wgrad_implicit): Cout > 128, G*N*HW >= 100000, N*HW >= 2048, HW % 32 == 0 -> the DMA ring kernel;
# Cout > 128, N*HW >= 100000 -> 256x192; Cout <= 32 and not grouped -> 32x256; else 128x128.  W % 8 != 0 -> im2col (vector
# kernel when W % 4 == 0, scalar otherwise) + GEMM; Cin > Cout -> tap scatter + GEMM; H*W % 4 != 0 -> the fp32 kernel.
WGRAD_CASES = {
    "impl_dma":         (0, 101, 3, 15, 200, 32, 32, 3, True, [(IMPL[0], "gemm_wgrad_dma_impl_kernel<4,2,2,3>")]),
    "impl_dma_g3":      (3, 41, 2, 16, 256, 32, 32, 3, True, [(IMPL[1], "gemm_wgrad_dma_impl_kernel<grouped 4,2,2,3>")]),
    "impl_256x192":     (0, 2521, 4, 14, 200, 5, 8, 3, False, [(IMPL[0], B3 % "4,2,2,3,64,1")]),   # HW = 40
    "impl_256x192_g3":  (3, 2521, 6, 0, 200, 5, 8, 3, True, [(IMPL[1], B3 % "grouped 4,2,2,3,64,1")]),
    "impl_32x256":      (0, 7, 5, 9, 24, 8, 24, 3, True, [(IMPL[0], B3 % "1,4,1,2,32,1")]),
    "impl_32rows_g3":   (3, 7, 5, 9, 24, 8, 24, 3, False, [(IMPL[1], B3 % "grouped 2,2,2,2,64,1")]),   # p.G != 0
    "impl_128x128":     (0, 37, 6, 14, 72, 8, 8, 3, True, [(IMPL[0], B3 % "2,2,2,2,64,1")]),
    "impl_128x128_g3":  (3, 37, 6, 14, 72, 8, 8, 3, False, [(IMPL[1], B3 % "grouped 2,2,2,2,64,1")]),
    "im2col_v4":        (0, 21, 5, 7, 40, 12, 12, 3, True, [("rfn_im2col3x3_f32", "im2col3x3"),
                                                            (GEMM[0], B3 % "1,4,2,2,32")]),
    "im2col_scalar":    (0, 21, 5, 7, 40, 6, 6, 3, False, [("rfn_im2col3x3_f32", "im2col3x3"),
                                                           (GEMM[0], B3 % "1,4,2,2,32")]),
    "im2col_g3":        (3, 21, 5, 7, 40, 6, 6, 3, False, [("rfn_im2col3x3_f32", "im2col3x3")] * 3 +
                         [(GEMM[1], B3 % "grouped 1,4,2,2,32")]),
    "tap_scatter":      (0, 21, 64, 0, 8, 8, 8, 3, False, [("rfn_tap_scatter_f32", "tap_scatter"),
                                                           (GEMM[0], B3 % "4,1,2,2,32")]),   # 72 x 64
    "tap_scatter_g3":   (3, 21, 60, 4, 8, 8, 8, 3, False, [("rfn_tap_scatter_f32", "tap_scatter"),
                                                           (GEMM[1], B3 % "grouped 4,1,2,2,32")]),
    "conv1x1_g3":       (3, 70, 250, 0, 256, 8, 8, 1, False, [(GEMM[1], B3 % "grouped 2,2,2,2,64")]),   # Nc = 250: no DMA
    "f32_3x5":          (0, 2, 9, 0, 20, 3, 5, 3, False, [("rfn_conv2d_wgrad_f32", "wgrad_mfma_kernel<3,4,1,1,1,64>"),
                                                          ("rfn_wgrad_finish_f32", "wgrad_finish")]),
}


def wgrad_f32(K, in1, in2, g, Cout, ks):
    """the fp32-MFMA weight gradient (rfn_conv2d_wgrad_f32) of the same operation: the yardstick"""
    old = K.CONV_PRECISION
    K.CONV_PRECISION = "f32"
    try:
        return K.conv2d_wgrad(in1, in2, g, Cout, ks)
    finally:
        K.CONV_PRECISION = old


def wgrad_figures(got, got40, gotf, g, x, ks):
    """e_abs of one weight gradient `got` (bf16x3), `got40` (the gradient times 2^-40) and `gotf` (fp32 MFMA)"""
    gm, g64, s = refs64(g, x, wgrad_op(ks))
    shape = gm.shape
    return {"model": e_abs(got.reshape(shape), gm, s), "fp64": e_abs(got.reshape(shape), g64, s),
            "f32": e_abs(gotf.reshape(shape), g64, s), "model_k-40": e_abs(got40.reshape(shape), gm * 2.0 ** -40, s * 2.0 ** -40)}


def merge(figs):
    return {k: max(f[k] for f in figs) for k in figs[0]}


def run_gemm_case(K, launches, name, seed=0):
    G, M, Nc, F_, H, W, view, tile = GEMM_CASES[name]
    g = torch.Generator().manual_seed(70 + seed)
    n = max(G, 1)
    a = [torch.randn(F_, M + (8 if view else 0), H, W, generator=g) for _ in range(n)]
    b = [torch.randn(F_, Nc + (4 if view else 0), H, W, generator=g) for _ in range(n)]
    b[-1] = b[-1] * 3 + 0.5   # the last group is unlike the others in scale and mean
    av = [t[:, :M] for t in a]
    bv = [t[:, 4:] if view else t for t in b]
    ad, bd = [t.cuda() for t in a], [t.cuda() for t in b]
    adv = [t[:, :M] for t in ad]
    bdv = [t[:, 4:] if view else t for t in bd]
    n0 = len(launches)
    if G:
        gw = K.gemm_wgrad_grouped(adv, bdv, M, Nc)
        gw40 = K.gemm_wgrad_grouped([t * 2.0 ** -40 for t in adv], bdv, M, Nc)
    else:
        gw = [K.gemm_wgrad(adv[0], bdv[0], M, Nc)]
        gw40 = [K.gemm_wgrad(adv[0] * 2.0 ** -40, bdv[0], M, Nc)]
    assert launches[n0:] == [(GEMM[1 if G else 0], tile)] * 2, (name, launches[n0:])
    figs = []
    for i in range(n):
        gf = wgrad_f32(K, bdv[i], None, adv[i], M, 1)
        figs.append(wgrad_figures(gw[i].cpu(), gw40[i].cpu(), gf.cpu(), av[i], bv[i], 1))
    return merge(figs)


def run_wgrad_case(K, launches, name, seed=0):
    G, N, C1, C2, Cout, H, W, ks, view, want = WGRAD_CASES[name]
    g = torch.Generator().manual_seed(71 + seed)
    n = max(G, 1)
    z = [torch.randn(N, C1 * (2 if view else 1), H, W, generator=g) for _ in range(n)]
    c = [torch.randn(N, C2, H, W, generator=g) for _ in range(n)] if C2 else None
    gy = torch.randn(n, N, Cout, H, W, generator=g)
    z[-1] = z[-1] * 3 + 0.5   # the last group is unlike the others in scale and mean
    zd, cd, gyd = [t.cuda() for t in z], None if c is None else [t.cuda() for t in c], gy.cuda()
    in1 = [t[:, :C1] for t in zd]
    gy40 = gyd * 2.0 ** -40
    n0 = len(launches)
    if G:
        gw = K.conv2d_wgrad_grouped(in1, cd, [gyd[i] for i in range(n)], Cout, ks, g_stacked=gyd)
        n1 = len(launches)
        gw40 = K.conv2d_wgrad_grouped(in1, cd, [gy40[i] for i in range(n)], Cout, ks, g_stacked=gy40)
    else:
        gw = [K.conv2d_wgrad(in1[0], None if cd is None else cd[0], gyd[0], Cout, ks)]
        n1 = len(launches)
        gw40 = [K.conv2d_wgrad(in1[0], None if cd is None else cd[0], gy40[0], Cout, ks)]
    assert launches[n0:n1] == want, (name, launches[n0:n1])
    figs = []
    for i in range(n):
        gf = wgrad_f32(K, in1[i], None if cd is None else cd[i], gyd[i], Cout, ks)
        x = z[i][:, :C1] if c is None else torch.cat([z[i][:, :C1], c[i]], 1)
        figs.append(wgrad_figures(gw[i].cpu(), gw40[i].cpu(), gf.cpu(), gy[i], x, ks))
    return merge(figs)


def check_wgrad(name, fig):
    check(name, fig, cap=WGRAD_CAP)
    msg = "%s: e_abs vs model at gradient * 2^-40: %.3g" % (name, fig["model_k-40"])
    print(msg)
    assert fig["model_k-40"] <= min(3 * fig["f32"] + 2e-8, WGRAD_CAP), msg


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_wgrad_vs_model(K, launches, name):
    check_wgrad(name, run_gemm_case(K, launches, name))


@pytest.mark.parametrize("name", [n for n in WGRAD_CASES if n != "f32_3x5"])
def test_conv_wgrad_vs_model(K, launches, name):
    check_wgrad(name, run_wgrad_case(K, launches, name))


def test_wgrad_fp32_route_vs_fp64(K, launches):
    """H*W % 4 != 0: conv2d_wgrad takes the fp32-MFMA kernel whatever the gradient arithmetic; fp32-grade vs fp64"""
    G, N, C1, C2, Cout, H, W, ks, view, want = WGRAD_CASES["f32_3x5"]
    g = torch.Generator().manual_seed(75)
    x, gy = torch.randn(N, C1, H, W, generator=g), torch.randn(N, Cout, H, W, generator=g)
    n0 = len(launches)
    gw = K.conv2d_wgrad(x.cuda(), None, gy.cuda(), Cout, ks)
    assert launches[n0:] == want, launches[n0:]
    _, g64, s = refs64(gy, x, wgrad_op(ks))
    e = e_abs(gw.cpu(), g64, s)
    print("f32_3x5: e_abs vs fp64 %.3g" % e)
    assert e <= FP32_CAP, e


# ------------------------------------------------------------------------------------------------ 3. the route set
ROUTES = {
    # choose_conv_b3 at npl == 2
    G3 % "1,4,1,1", G3 % "2,2,1,1", G3 % "2,2,1,2", G1 % "1,4,1,1", G1 % "2,2,1,1", G1 % "2,2,2,2", G1 % "4,1,2,2",
    WS1, WS3A, WS3B,
    # rfn_conv2d_dgrad_act_bf16x3 (ep_mode 4)
    "conv3x3_ws_kernel<1,2,0>+actbwd", WS1 + "+actbwd", G3 % "2,2,1,1" + "+actbwd", G3 % "2,2,1,2" + "+actbwd",
    G1 % "2,2,1,1" + "+actbwd",
    "dgrad_small_kernel",
    # choose_gemm_wgrad, single and grouped
    DMA % "2,4,4,2,32,2", DMA % "1,8,2,1,32,3", B3 % "4,2,2,3,64", B3 % "2,4,4,2,64", B3 % "1,4,2,2,32",
    B3 % "4,1,2,2,32", B3 % "2,2,2,2,64",
    DMA % "grouped 2,4,4,2,32,2", DMA % "grouped 1,8,2,1,32,3", B3 % "grouped 4,2,2,3,64", B3 % "grouped 2,4,4,2,64",
    B3 % "grouped 1,4,2,2,32", B3 % "grouped 4,1,2,2,32", B3 % "grouped 2,2,2,2,64",
    # choose_wgrad_implicit, single and grouped (a group never takes the 32-row tiling)
    "gemm_wgrad_dma_impl_kernel<4,2,2,3>", B3 % "4,2,2,3,64,1", B3 % "1,4,1,2,32,1", B3 % "2,2,2,2,64,1",
    "gemm_wgrad_dma_impl_kernel<grouped 4,2,2,3>", B3 % "grouped 4,2,2,3,64,1", B3 % "grouped 2,2,2,2,64,1",
    # operand expansion and the fp32 weight gradient
    "im2col3x3", "tap_scatter", "wgrad_mfma_kernel<3,4,1,1,1,64>", "wgrad_finish",
}


def test_case_tables_cover_the_route_set():
    """every instantiation the gradient dispatchers can choose is the table entry of at least one case (and each case
    asserts that its launches carry exactly its entry)"""
    table = {c[-1] for c in CONV_CASES.values()} | {c[-1] for c in ACTBWD_CASES.values()} | {"dgrad_small_kernel"}
    table |= {c[-1] for c in GEMM_CASES.values()}
    table |= {label for c in WGRAD_CASES.values() for _, label in c[-1]}
    assert table == ROUTES, (sorted(table - ROUTES), sorted(ROUTES - table))
