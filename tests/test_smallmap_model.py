"""The small-map dense kernels (csrc/smallmap.hip) against the exact three-product model of their arithmetic.

csrc/smallmap.hip runs every 3x3 / pad 1 convolution on a map of at most 16 pixels as ONE dense product
    out[b][(co,po)] = sum_(ci,pi) x[b][(ci,pi)] * M[(ci,pi)][(co,po)],   M = w[co][ci][tap(po, pi)]
on packed bf16 (hi, lo) weights, three MFMAs per product (a_lo*b_hi + a_hi*b_lo + a_hi*b_hi, fp32 accumulation, the eight
waves' partial tiles added through LDS in a fixed order).  Three entry points share the body: rfn_smallmap_dense_bf16x3
(ops.smallmap_dense: per-timestep prior / encoder layers, the ConvLSTM recurrence through `add`, the data gradient
through the transposed pack with the activation backward fused on its input), rfn_smallmap_dense_pair_bf16x3 (two such
products in one launch) and rfn_smallmap_conv_bf16x3 (ops.smallmap_conv: the coupling nets' conv1 / conv3 and conv1's data
gradient at the 2x2 and 4x4 flow levels behind conv2d_raw's contract).  The pack is held bit for bit by
test_conv_split_precision; here the products are held to the model and measures of test_conv_grad_model (imported, not
restated):  y3 = model64(x, w, op),  S = op(|x|, |w|),  e_abs = max |y - ref| / S,  op = F.conv2d(., ., padding=1)
(a transposed pack: the flipped and transposed weight).

Per case
  vs the model  e_abs <= 3 * e_abs(fp32-MFMA kernel ops.conv2d_raw(prec="f32"), same tensors, vs fp64) + 2e-8 and <= FP32_CAP
  vs exact fp64 e_abs <= SPLIT_BOUND (the model alone: 9.7e-6 on these shapes, test_model_leaves_room_under_the_split_bound)
  epilogues     applied in fp64 to y3 and held to the same tolerance times S times the epilogue's local scale (exp(p1) for
                ep_mode 1, exp(3 p1) for 2, 1 for bias / add / mode 3 / accumulation), after EW = 4 * 2^-24 of |result| for
                the epilogue's own fp32 roundings is taken off; relu / leaky_relu are 1-Lipschitz; no output is excluded
  bits          two calls agree; without bias / add / epilogue / acc the input times 2^k, k in SCALES, gives the output
                times 2^k; a_out is the fp32 product a * where(y > 0, 1, slope_in) of torch on the CPU (y holds planted
                +0.0 and -0.0), without y it is a; a pair launch equals two single launches in every output and a_out
  tap(po, pi)   test_dense_matrix_statement: rows @ M, M the fp64 matrix of smallmap_pack_ref before its padding
                (smallmap_dense_matrix), equals F.conv2d to fp64 rounding, exactly and in the three-product form
  guards        every entry point is also called through rfn_hip.lib.call with sentinel-filled buffers: MARGIN floats
                after out / a_out / the wider tensor of a view stay untouched; rejected arguments (codes -1 .. -5) set
                rfn_last_error and write nothing; B == 0 / N == 0 return 0 and write nothing
  route         each call is seen at rfn_hip.lib.call under the entry point meant (the conv form with its label
                smallmap_dense_kernel)
The kernels are called directly, so the module is the same under RFN_CONV_PRECISION = mixed, bf16x3 and f32.

The fp32-MFMA yardstick refuses maps one pixel wide (1x1, 2x1: their halo does not fit its LDS image, code -7); for those
it runs on the frame zero-padded to 2x2, the same sums with exact zero terms added (f32_conv).

Measured on an MI355X (largest over the cases of an entry point; e_abs vs the model / vs fp64 / fp32 kernel vs fp64):
  rfn_smallmap_dense_bf16x3   (10 shapes, forward with 7 epilogue combinations, data gradient with and without y)
                                      1.2e-7 / 1.1e-5 / 3.7e-7
  rfn_smallmap_conv_bf16x3    (K1 = 8 with epilogues 0-3, production shape, data gradient into views x 4 acc)
                                      4.7e-8 / 4.1e-6 / 1.3e-7
  rfn_smallmap_dense_pair_bf16x3      bit-identical to single launches (both orders, B = 33)
  The case nearest its model tolerance uses 0.34 of it (dense forward 32 x 768 -> 256 on 2x2: 3.9e-8 against 1.15e-7).
Wall time of the module on the MI355X machine: 3.4 s (44 tests, 0.3 s the slowest), the same in the three arithmetics.

Deliberate faults in smallmap_dense_body, each in a scratch build (not committed), arithmetic only, run under
RFN_CONV_PRECISION=bf16x3 together with the three older tests of test_hip_kernels (16 cases, relerr < 2e-5 .. 3e-5):
  A   b_lo = 0 in the last k-step: all 26 model cases of this module fail, e_abs vs the model 2.1e-5 (K = 3072) ..
      2.6e-3 (K = 8 .. 72): 180 to 10^4 times the tolerance.  The older tests do NOT pass either: 15 of 16 fail, relerr
      1.1e-4 .. 8.8e-4, 4 to 40 times their bound (K <= 3072 is small enough for 2^-9 of one k-step to show); the one that
      passes is the pair test, bit-identical by construction.  For these kernels the old measure is short of margin and
      of shapes, not blind:
  A2  one element: b_lo[0] of lane 0 zeroed in the last k-step where KS >= 64: the three production cases fail here
      (6.1e-6, 3.2e-5, 1.0e-5 vs the model: 50 to 300 times the tolerance); 6 of the 16 older cases fail at relerr
      2.8e-5 .. 9.1e-5, 1.4 to 3 times their bound, 10 pass.
  C   fault A only where K % 16 == 8, a shape no older test has: the 16 cases of this module with such a K fail (12
      dense cases forward and backward, the four data-gradient view cases; 4.8e-4 .. 2.6e-3 vs the model), all 16 older
      cases PASS: the gap in shapes.
  B   kok = mok in the split of a (the k-tail gate dropped where the values are used, loads unchanged): INVISIBLE, all
      60 cases pass: the upper 8-group of the last k-step then multiplies column 0 .. 7 of a by packed rows K .. K+7, which
      the pack writes as zeros.  The K % 16 == 8 cases stay for the a_out guard (a_out is written under kok: its margin
      and bits are checked) and for fault C.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_grad_model import FP32_CAP, SCALES, SPLIT_BOUND, check, e_abs, model64, refs64, split
from tests.test_conv_split_precision import MARGIN, SENTINEL, _sentinel_buf, smallmap_dense_matrix, smallmap_pack_ref

pytestmark = pytest.mark.gpu

DENSE, PAIR, CONV = "rfn_smallmap_dense_bf16x3", "rfn_smallmap_dense_pair_bf16x3", "rfn_smallmap_conv_bf16x3"
EW = 4 * 2.0 ** -24      # an epilogue's own fp32 roundings, relative to |result| (at most four: add, expf, product, act)
SLOPE = 0.2              # travels as a C float: the references use float32(0.2)
SLOPE32 = float(torch.tensor(SLOPE, dtype=torch.float32))


def OP(x, w):
    return F.conv2d(x, w, padding=1)


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    return ops


@pytest.fixture
def launches(monkeypatch):
    """(entry point, label or None) of every small-map launch, recorded through rfn_hip.lib.call"""
    from rfn_hip import lib
    seen = []
    orig = lib.call

    def call(name, *args, meta=None):
        if name in (DENSE, PAIR, CONV):
            seen.append((name, None if meta is None else meta[1]))
        return orig(name, *args, meta=meta)
    monkeypatch.setattr(lib, "call", call)
    return seen


def note(entry, what, fig):
    """check() of one case, its name led by the entry point (the docstring's maxima are read from these lines)"""
    check("%s %s" % (entry, what), fig, cap=FP32_CAP)


def excess(got, ref, s):
    """max over outputs of (|got - ref| - EW |ref|)+ / s: e_abs with an epilogue's own roundings taken off"""
    d = ((got.detach().cpu().double() - ref).abs() - EW * ref.abs()).clamp_min(0.0)
    return float((d / (s + 1e-300)).max())


def figures(y3, yf, refs, post=None, scale=1.0):
    """{"model", "fp64", "f32"}: y3 (bf16x3, after the fp64 epilogue `post` of local scale `scale`) against the model and
    against exact fp64, the raw fp32-MFMA result yf against exact fp64"""
    ym, y64, s = refs
    if post is None:
        return {"model": e_abs(y3, ym, s), "fp64": e_abs(y3, y64, s), "f32": e_abs(yf, y64, s)}
    return {"model": excess(y3, post(ym), s * scale), "fp64": excess(y3, post(y64), s * scale), "f32": e_abs(yf, y64, s)}


def leaky64(z, slope=SLOPE32):
    return torch.where(z > 0, z, z * slope)


def guarded(t):
    """t on the device as a view of a sentinel-filled buffer with MARGIN floats after it -> (view, buffer)"""
    buf = _sentinel_buf(t.numel() + MARGIN)
    v = buf[:t.numel()].view(t.shape)
    v.copy_(t)
    return v, buf


def margin_ok(buf, used):
    return bool((buf.view(torch.int32)[used:] == SENTINEL).all())


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def f32_conv(K, x1d, x2d, wd, Cout, flip):
    """the yardstick: the fp32-MFMA kernel of the same convolution on the same tensors.  That kernel refuses maps one
    pixel wide (their halo does not fit its LDS image: code -7); for those the frame is zero-padded to 2x2, which IS the
    convolution's own padding: the same sums with exact zero terms added, read back at the frame's pixels"""
    H, W = x1d.shape[2:]
    wpk = K.pack_weight(wd, flip=flip, prec="f32")
    if W > 1:
        return K.conv2d_raw(x1d, x2d, wpk, Cout, 3, prec="f32")
    assert x2d is None and H <= 2
    return K.conv2d_raw(F.pad(x1d, (0, 1, 0, 2 - H)), None, wpk, Cout, 3, prec="f32")[:, :, :H, :W]


# ------------------------------------------------------------------------------------------------ 1. dense entry point
# name: (B, C1, C2, Cout, H, W); K = C1*HW forward, Cout*HW for the data gradient (transposed pack).  The kernel: 8 waves
# share the KS = ceil(K/16) k-steps (wave w takes w, w+8, ..), each k-step two 8-groups (the upper one off when
# K % 16 == 8); 32-row tiles over B, 32-column tiles over N.
DENSE_CASES = {
    "k8_b1":       (1, 2, 0, 2, 2, 2),        # K = 8: one half k-step, 7 idle waves, N = 8 < 32, B = 1
    "k24_k40":     (31, 6, 0, 10, 2, 2),      # K = 24 / 40: both 8 mod 16
    "1x1":         (33, 8, 0, 24, 1, 1),      # centre tap only; two row tiles; K = 8 / 24
    "3x3_b65":     (65, 8, 0, 8, 3, 3),       # three row tiles, K = 72 = 8 mod 16, N = 72: tail tile
    "4x2":         (5, 4, 0, 12, 4, 2),
    "2x1":         (5, 12, 0, 4, 2, 1),
    "3x5":         (7, 8, 0, 8, 3, 5),
    "1x16":        (7, 4, 0, 4, 1, 16),
    "ks9":         (32, 36, 0, 20, 2, 2),     # KS = 9: one wave does two steps, seven do one
    "production":  (32, 768, 0, 256, 2, 2),
}


def inputs(case, seed):
    B, C1, C2, Cout, H, W = case
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(B, C1, H, W, generator=g)
    x2 = torch.randn(B, C2, H, W, generator=g) if C2 else None
    w = torch.randn(Cout, C1 + C2, 3, 3, generator=g) / ((C1 + C2) * 9) ** 0.5
    return g, x1, x2, w


def dense_direct(a, y, slope_in, pk, bias, add, slope_out, n_ch, want_a_out):
    """rfn_smallmap_dense_bf16x3 through lib.call into sentinel-guarded buffers; the margins must be untouched"""
    from rfn_hip import lib as L
    B, HW = a.shape[0], a.shape[2] * a.shape[3]
    Kk, N = a.shape[1] * HW, n_ch * HW
    out = _sentinel_buf(B * N + MARGIN)
    ao = _sentinel_buf(B * Kk + MARGIN) if want_a_out else None
    L.call(DENSE, L.dev(a), L.dev(y), slope_in, L.dev(pk), L.dev(bias), L.dev(add), 0 if slope_out is None else 1,
           0.0 if slope_out is None else slope_out, L.dev(out), L.dev(ao), B, Kk, N, HW)
    assert margin_ok(out, B * N), "written past out[B*N]"
    if want_a_out:
        assert margin_ok(ao, B * Kk), "written past a_out[B*K]"
    return out[:B * N].view(B, n_ch, *a.shape[2:]), None if ao is None else ao[:B * Kk].view(a.shape)


EPILOGUES = [("bias",), ("slope",), ("bias", "slope"), ("add",), ("add", "bias"), ("add", "bias", "slope")]


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_forward_vs_model(K, launches, name):
    """ops.smallmap_dense with the plain pack: the raw product against the model, the bit rules, then every combination
    of bias / add / slope_out against the fp64 epilogue of the model (local scale 1; leaky_relu is 1-Lipschitz, no output
    is excluded), and one direct call into guarded buffers"""
    case = DENSE_CASES[name]
    B, Cin, _, Cout, H, W = case
    g, x, _, w = inputs(case, 300)
    bias, add = torch.randn(Cout, generator=g) * 0.3, torch.randn(B, Cout, H, W, generator=g) * 0.3
    xd, wd, bd, ad = x.cuda(), w.cuda(), bias.cuda(), add.cuda()
    pk = K.smallmap_pack(wd, H, W, False)
    n0 = len(launches)
    y = K.smallmap_dense(xd, pk, Cout)
    assert launches[n0:] == [(DENSE, None)], launches[n0:]
    assert bits_equal(K.smallmap_dense(xd, pk, Cout), y), "two calls"
    for k in SCALES:
        assert torch.equal(K.smallmap_dense(xd * 2.0 ** k, pk, Cout), y * 2.0 ** k), "input * 2^%d" % k
    yf = f32_conv(K, xd, None, wd, Cout, False)
    refs = refs64(x, w, OP)
    note(DENSE, "fwd " + name, figures(y, yf, refs))
    for ep in EPILOGUES:
        kw = dict(bias=bd if "bias" in ep else None, add=ad if "add" in ep else None,
                  slope_out=SLOPE if "slope" in ep else None)

        def post(z):
            z = z + bias.double().view(1, -1, 1, 1) if "bias" in ep else z
            z = z + add.double() if "add" in ep else z
            return leaky64(z) if "slope" in ep else z
        out = K.smallmap_dense(xd, pk, Cout, **kw)
        note(DENSE, "fwd %s %s" % (name, "+".join(ep)), figures(out, yf, refs, post))
    direct, _ = dense_direct(xd, None, 0.0, pk, bd, ad, SLOPE, Cout, False)
    assert bits_equal(direct, out), "direct call, add + bias + slope_out"


def planted(y):
    """exact zeros and negative zeros among y's elements (both take the slope: y > 0 is false)"""
    v = y.view(-1)
    v[0::5] = 0.0
    v[2::7] = -0.0
    return y


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_backward_vs_model(K, launches, name):
    """the data gradient through the transposed pack, with the activation backward fused on the input
    (a' = a * (y > 0 ? 1 : slope_in)): a_out is that single fp32 product bit for bit (without y: a itself), the product
    is held to the model of a'"""
    case = DENSE_CASES[name]
    B, Cin, _, Cout, H, W = case
    g, _, _, w = inputs(case, 310)
    wl = w.transpose(0, 1).flip(2, 3).contiguous()    # the convolution the transposed pack computes: Cout -> Cin
    go = torch.randn(B, Cout, H, W, generator=g)
    y = planted(F.leaky_relu(torch.randn(B, Cout, H, W, generator=g), SLOPE))
    ap = go * torch.where(y > 0, torch.tensor(1.0), torch.tensor(SLOPE))     # fp32 on the CPU: one multiply
    gd, yd, wd = go.cuda(), y.cuda(), w.cuda()
    pb = K.smallmap_pack(wd, H, W, True)
    n0 = len(launches)
    gx, ao = K.smallmap_dense(gd, pb, Cin, y=yd, slope_in=SLOPE, want_a_out=True)
    assert launches[n0:] == [(DENSE, None)], launches[n0:]
    assert bits_equal(ao.cpu(), ap), "a_out"
    gx2, ao2 = dense_direct(gd, yd, SLOPE, pb, None, None, None, Cin, True)
    assert bits_equal(gx2, gx) and bits_equal(ao2, ao), "direct call / two calls"
    gf = f32_conv(K, ap.cuda(), None, wd, Cin, True)
    note(DENSE, "bwd %s with y" % name, figures(gx, gf, refs64(ap, wl, OP)))
    # without y: a_out = a, and the magnitude rule
    gx0, ao0 = K.smallmap_dense(gd, pb, Cin, want_a_out=True)
    assert bits_equal(ao0, gd), "a_out without y"
    assert bits_equal(K.smallmap_dense(gd, pb, Cin), gx0), "two calls"
    for k in SCALES:
        assert torch.equal(K.smallmap_dense(gd * 2.0 ** k, pb, Cin), gx0 * 2.0 ** k), "gradient * 2^%d" % k
    note(DENSE, "bwd " + name, figures(gx0, f32_conv(K, gd, None, wd, Cin, True), refs64(go, wl, OP)))


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("name", ["3x3_b65", "4x2", "2x1", "3x5", "1x16", "1x1"])
def test_dense_matrix_statement(K, name, transpose):
    """An independent statement of tap(po, pi): the rows of a sample times the dense matrix M of smallmap_pack_ref (fp64,
    before its padding) IS the convolution, exactly and in the three-product model, up to fp64 summation: two sums of K
    terms, each within K * 2^-53 of S.  The pack the other tests multiply with is that matrix's, bit for bit."""
    case = DENSE_CASES[name]
    B, Cin, _, Cout, H, W = case
    g, x, _, w = inputs(case, 320)
    if transpose:
        x, wl = torch.randn(B, Cout, H, W, generator=g), w.transpose(0, 1).flip(2, 3).contiguous()
    else:
        wl = w
    ym, y64, s = refs64(x, wl, OP)
    rows = x.reshape(B, -1)
    Kk = rows.shape[1]
    tol = 2 * Kk * 2.0 ** -53
    M = smallmap_dense_matrix(w.double(), H, W, transpose)
    assert M.shape == (Kk, y64[0].numel())
    assert e_abs((rows.double() @ M).view(y64.shape), y64, s) <= tol
    (xh, xl), (mh, ml) = split(rows), split(smallmap_dense_matrix(w, H, W, transpose))
    y3 = xh.double() @ (mh.double() + ml.double()) + xl.double() @ mh.double()
    assert e_abs(y3.view(ym.shape), ym, s) <= 3 * tol   # two products on each side, terms within (1 + 2^-8)^2 of S's
    pk = K.smallmap_pack(w.cuda(), H, W, transpose)
    assert torch.equal(pk.cpu().view(torch.int16), smallmap_pack_ref(w, H, W, 1 if transpose else 0))


def test_model_leaves_room_under_the_split_bound():
    """the reference itself: on every dense shape the three-product model stays within the representation part of
    SPLIT_BOUND (1.25 * 2^-16; the 4e-7 on top is the kernel's accumulation) of exact fp64, forward and transposed"""
    worst = 0.0
    for name, case in DENSE_CASES.items():
        g, x, _, w = inputs(case, 300)
        go = torch.randn(case[0], case[3], case[4], case[5], generator=g)
        for a, wl in ((x, w), (go, w.transpose(0, 1).flip(2, 3).contiguous())):
            worst = max(worst, e_abs(model64(a, wl, OP), OP(a.double(), wl.double()), OP(a.double().abs(), wl.double().abs())))
    print("model vs fp64: e_abs %.3g (SPLIT_BOUND %.3g)" % (worst, SPLIT_BOUND))
    assert worst <= SPLIT_BOUND - FP32_CAP


# ------------------------------------------------------------------------------------------------ 2. conv entry point
# name: (N, C1, C2, Cout, H, W)
CONV_CASES = {
    "k1_8":        (33, 2, 6, 5, 2, 2),       # K1 = 8: the source boundary falls inside the first k-step; two row tiles
    "production":  (70, 32, 256, 256, 2, 2),
}
LABEL = (CONV, "smallmap_dense_kernel")


CONV_EPILOGUES = {"k1_8": [(1, 0), (1, 1), (1, 2), (2, 0), (3, 0)], "production": [(1, 2)]}   # (ep_mode, act)


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_entry_vs_model(K, launches, name):
    """ops.smallmap_conv, two sources (in1 a channel slice of a wider tensor, in2 contiguous): the raw product and the
    bit rules once, then each epilogue: mode 1 (v + p0) * exp(p1) then act, local scale exp(p1); mode 2
    (v + p0) * exp(3 p1), scale exp(3 p1); mode 3 v + p0, scale 1"""
    case = CONV_CASES[name]
    N, C1, C2, Cout, H, W = case
    g, x1, x2, w = inputs(case, 330)
    wide = torch.randn(N, C1 + 3, H, W, generator=g)
    wide[:, 1:1 + C1] = x1
    p0, p1 = torch.randn(Cout, generator=g) * 0.3, torch.randn(Cout, generator=g) * 0.2
    wided, x2d, wd, p0d, p1d = wide.cuda(), x2.cuda(), w.cuda(), p0.cuda(), p1.cuda()
    x1d = wided[:, 1:1 + C1]
    pk = K.smallmap_pack(wd, H, W, False)
    n0 = len(launches)
    y = K.smallmap_conv(x1d, x2d, pk, Cout)
    assert launches[n0:] == [LABEL], launches[n0:]
    assert bits_equal(K.smallmap_conv(x1d, x2d, pk, Cout), y), "two calls"
    for k in SCALES:
        assert torch.equal(K.smallmap_conv(x1d * 2.0 ** k, x2d * 2.0 ** k, pk, Cout), y * 2.0 ** k), "input * 2^%d" % k
    yf = f32_conv(K, x1d, x2d, wd, Cout, False)
    refs = refs64(torch.cat([x1, x2], 1), w, OP)
    note(CONV, "%s raw" % name, figures(y, yf, refs))
    b, e = p0.double().view(1, -1, 1, 1), p1.double().view(1, -1, 1, 1)
    for ep_mode, act in CONV_EPILOGUES[name]:
        scale = e.exp() if ep_mode == 1 else (3 * e).exp() if ep_mode == 2 else torch.ones_like(e)

        def post(z):
            z = (z + b) * scale
            return z.clamp_min(0.0) if act == 1 else leaky64(z) if act == 2 else z
        out = K.smallmap_conv(x1d, x2d, pk, Cout, ep_mode=ep_mode, p0=p0d, p1=p1d if ep_mode in (1, 2) else None, act=act)
        note(CONV, "%s ep %d act %d" % (name, ep_mode, act), figures(out, yf, refs, post, scale))


@pytest.mark.parametrize("acc1,acc2", [(False, False), (True, False), (False, True), (True, True)])
def test_conv_entry_dgrad_views(K, launches, acc1, acc2):
    """the coupling net's conv1 data gradient (dgrad1 == "dense"): a transposed pack behind the conv interface, K = 40
    (8 mod 16), 33 frames, the 6 output channels split 3 + 3 so that nsplit = 12 falls inside the one 32-column tile,
    out1 the first-half view of a wider tensor, out2 a view too, each accumulate combination (the base enters the
    result, so its share of the bound is EW * |result|); everything outside the views keeps its bits"""
    N, Hd, Cf, H, W, sp = 33, 10, 6, 2, 2, 3
    g = torch.Generator().manual_seed(340)
    w = torch.randn(Hd, Cf, 3, 3, generator=g) / (Cf * 9) ** 0.5     # forward weight Cf -> Hd
    wl = w.transpose(0, 1).flip(2, 3).contiguous()
    gh = torch.randn(N, Hd, H, W, generator=g)
    big1, big2 = torch.randn(N, 2 * sp, H, W, generator=g), torch.randn(N, Cf - sp + 2, H, W, generator=g)
    (b1, buf1), (b2, buf2) = guarded(big1), guarded(big2)
    ghd, wd = gh.cuda(), w.cuda()
    pk = K.smallmap_pack(wd, H, W, True)
    n0 = len(launches)
    K.smallmap_conv(ghd, None, pk, Cf, out1=b1[:, :sp], out2=b2[:, 1:1 + Cf - sp], cout_split=sp, acc1=acc1, acc2=acc2)
    assert launches[n0:] == [LABEL], launches[n0:]
    assert margin_ok(buf1, big1.numel()) and margin_ok(buf2, big2.numel())
    o1, o2 = b1.cpu(), b2.cpu()
    assert bits_equal(o1[:, sp:], big1[:, sp:]) and bits_equal(o2[:, :1], big2[:, :1])
    assert bits_equal(o2[:, 1 + Cf - sp:], big2[:, 1 + Cf - sp:])
    got = torch.cat([o1[:, :sp], o2[:, 1:1 + Cf - sp]], 1)
    base = torch.cat([big1[:, :sp] * float(acc1), big2[:, 1:1 + Cf - sp] * float(acc2)], 1).double()
    gf = f32_conv(K, ghd, None, wd, Cf, True)
    note(CONV, "dgrad views acc %d%d" % (acc1, acc2), figures(got, gf, refs64(gh, wl, OP), lambda z: z + base))


# ------------------------------------------------------------------------------------------------ 3. pair entry point
def pair_direct(a, y, slope_in, pk, n_ch):
    """rfn_smallmap_dense_pair_bf16x3 (no bias / add / act_out) with a_out for both, into guarded buffers"""
    from rfn_hip import lib as L
    B, HW = a[0].shape[0], a[0].shape[2] * a[0].shape[3]
    Ks, Ns = [t.shape[1] * HW for t in a], [c * HW for c in n_ch]
    outs, aos = [_sentinel_buf(B * n + MARGIN) for n in Ns], [_sentinel_buf(B * k + MARGIN) for k in Ks]
    args = []
    for i in range(2):
        args += [L.dev(a[i]), L.dev(y[i]), slope_in[i], L.dev(pk[i]), None, None, 0, 0.0, L.dev(outs[i]), L.dev(aos[i]),
                 Ks[i], Ns[i]]
    L.call(PAIR, *args, B, HW)
    for i in range(2):
        assert margin_ok(outs[i], B * Ns[i]) and margin_ok(aos[i], B * Ks[i]), "written past product %d" % i
    return ([outs[i][:B * Ns[i]].view(B, n_ch[i], *a[i].shape[2:]) for i in range(2)],
            [aos[i][:B * Ks[i]].view(a[i].shape) for i in range(2)])


@pytest.mark.parametrize("larger", [1, 0])
def test_pair_equals_two_single_launches(K, launches, larger):
    """one pair launch against two single launches, bit for bit (each single launch is held to the model above): 33 rows
    (two row tiles), 8 -> 8 next to 42 -> 72 channels on 2x2 (K = 32 / 168 = 8 mod 16, N = 32 / 288), so the blocks of the
    smaller product leave at the block-uniform early return, in either order; bias / slope_out / add0 / add1; the data
    gradient with y0 only, y1 only and both, every a_out"""
    B, H, W = 33, 2, 2
    ch = [(8, 8), (42, 72)] if larger == 1 else [(42, 72), (8, 8)]
    g = torch.Generator().manual_seed(350 + larger)
    xs = [torch.randn(B, ci, H, W, generator=g).cuda() for ci, _ in ch]
    ws = [(torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5).cuda() for ci, co in ch]
    bs = [torch.randn(co, generator=g).cuda() for _, co in ch]
    ads = [torch.randn(B, co, H, W, generator=g).cuda() for _, co in ch]
    pf, pb = [K.smallmap_pack(w, H, W, False) for w in ws], [K.smallmap_pack(w, H, W, True) for w in ws]
    co = [c for _, c in ch]
    ci = [c for c, _ in ch]
    for kw0, kw1 in [(dict(bias=bs[0], slope_out=SLOPE), dict(bias=bs[1])),
                     (dict(add=ads[0]), dict(bias=bs[1], slope_out=SLOPE)),
                     (dict(bias=bs[0]), dict(add=ads[1], bias=bs[1], slope_out=SLOPE)),
                     (dict(add=ads[0], bias=bs[0], slope_out=SLOPE), dict(add=ads[1]))]:
        n0 = len(launches)
        y0, y1 = K.smallmap_dense_pair(xs[0], pf[0], co[0], xs[1], pf[1], co[1],
                                       **{k + "0": v for k, v in kw0.items()}, **{k + "1": v for k, v in kw1.items()})
        assert launches[n0:] == [(PAIR, None)], launches[n0:]
        assert bits_equal(y0, K.smallmap_dense(xs[0], pf[0], co[0], **kw0)), (sorted(kw0), sorted(kw1))
        assert bits_equal(y1, K.smallmap_dense(xs[1], pf[1], co[1], **kw1)), (sorted(kw0), sorted(kw1))
    gs = [torch.randn(B, c, H, W, generator=g).cuda() for c in co]
    ys = [planted(F.leaky_relu(torch.randn(B, c, H, W, generator=g), SLOPE)).cuda() for c in co]
    for use in ((False, True), (True, False), (True, True)):
        yy = [ys[i] if use[i] else None for i in range(2)]
        gx0, ga0, gx1, ga1 = K.smallmap_dense_pair(gs[0], pb[0], ci[0], gs[1], pb[1], ci[1], y0=yy[0], y1=yy[1],
                                                   slope_in0=SLOPE, slope_in1=0.1, want_a_out=True)
        for i, (gx, ga, sl) in enumerate(((gx0, ga0, SLOPE), (gx1, ga1, 0.1))):
            if use[i]:
                sx, sa = K.smallmap_dense(gs[i], pb[i], ci[i], y=ys[i], slope_in=sl, want_a_out=True)
                assert bits_equal(gx, sx) and bits_equal(ga, sa), (use, i)
            else:
                assert ga is gs[i] and bits_equal(gx, K.smallmap_dense(gs[i], pb[i], ci[i])), (use, i)
    (d0, d1), (e0, e1) = pair_direct(gs, ys, (SLOPE, 0.1), pb, ci)   # the last loop round: both y
    assert bits_equal(d0, gx0) and bits_equal(d1, gx1) and bits_equal(e0, ga0) and bits_equal(e1, ga1)
    (d0, d1), (e0, e1) = pair_direct(gs, (None, None), (0.0, 0.0), pb, ci)
    assert bits_equal(e0, gs[0]) and bits_equal(e1, gs[1]), "a_out without y"
    assert bits_equal(d0, K.smallmap_dense(gs[0], pb[0], ci[0])) and bits_equal(d1, K.smallmap_dense(gs[1], pb[1], ci[1]))


# ------------------------------------------------------------------------------------------------ 4. entry-point contracts
class Bufs:
    """sentinel-filled device buffers for calls that must not write: 4096 floats each, more than any shape below reads
    or writes, so that a check which wrongly passed would fail the test and not touch foreign memory"""
    def __init__(self, n):
        self.b = [_sentinel_buf(4096) for _ in range(n)]

    def untouched(self):
        return all(margin_ok(b, 0) for b in self.b)


def rejected(name, code, args, bufs):
    from rfn_hip import lib as L
    with pytest.raises(RuntimeError, match=r"%s failed \(code %d\): .*%s" % (name, code, name)):
        L.call(name, *args)
    assert name in L.load().rfn_last_error().decode()
    torch.cuda.synchronize()
    assert bufs.untouched(), (name, code)


def accepted_without_writing(name, args, bufs):
    from rfn_hip import lib as L
    L.call(name, *args)
    torch.cuda.synchronize()
    assert bufs.untouched(), name


def test_dense_entry_contract(K):
    """rfn_smallmap_dense_bf16x3: -1 (null pointer, HW = 17), -2 (K % 8, K % HW), -3 (a / y / a_out not 16-byte aligned)
    set rfn_last_error and write nothing; B == 0 returns 0 and writes nothing"""
    from rfn_hip import lib as L
    a, pk = torch.zeros(4096, device="cuda"), torch.zeros(32768, device="cuda")
    s = Bufs(3)
    out, ao, y = (L.dev(b) for b in s.b)

    def off(b):
        return L.dev(b[1:])

    def args(a=L.dev(a), y=None, out=out, ao=None, B=2, Kk=16, N=8, HW=4):
        return (a, y, 0.2, L.dev(pk), None, None, 0, 0.0, out, ao, B, Kk, N, HW)
    rejected(DENSE, -1, args(a=None), s)
    rejected(DENSE, -1, args(out=None), s)
    rejected(DENSE, -1, args(Kk=136, N=136, HW=17), s)
    rejected(DENSE, -1, args(N=0), s)
    rejected(DENSE, -2, args(Kk=12), s)            # K % 8
    rejected(DENSE, -2, args(Kk=24, N=16, HW=16), s)   # K % HW
    rejected(DENSE, -2, args(N=6), s)              # N % HW
    rejected(DENSE, -3, args(a=off(a)), s)
    rejected(DENSE, -3, args(y=off(s.b[2])), s)
    rejected(DENSE, -3, args(y=y, ao=off(s.b[1])), s)
    accepted_without_writing(DENSE, args(y=y, ao=ao, B=0), s)


def test_pair_entry_contract(K):
    """rfn_smallmap_dense_pair_bf16x3: the same checks for either product (-1 .. -3), B == 0"""
    from rfn_hip import lib as L
    a, pk = torch.zeros(4096, device="cuda"), torch.zeros(32768, device="cuda")
    s = Bufs(5)
    o0, o1, ao, y = (L.dev(b) for b in s.b[:4])

    def args(a1=L.dev(a), y1=None, ao1=None, K0=16, K1=16, N1=8, B=2, HW=4):
        return (L.dev(a), None, 0.2, L.dev(pk), None, None, 0, 0.0, o0, None, K0, 8,
                a1, y1, 0.2, L.dev(pk), None, None, 0, 0.0, o1, ao1, K1, N1, B, HW)
    rejected(PAIR, -1, args(a1=None), s)
    rejected(PAIR, -1, args(K0=136, K1=136, N1=136, HW=17), s)
    rejected(PAIR, -2, args(K0=12), s)
    rejected(PAIR, -2, args(K1=12), s)
    rejected(PAIR, -2, args(N1=6), s)
    rejected(PAIR, -3, args(a1=L.dev(a[1:])), s)
    rejected(PAIR, -3, args(y1=L.dev(s.b[3][1:])), s)
    rejected(PAIR, -3, args(y1=y, ao1=L.dev(s.b[2][1:])), s)
    accepted_without_writing(PAIR, args(y1=y, ao1=ao, B=0), s)


def test_conv_entry_contract(K):
    """rfn_smallmap_conv_bf16x3: each of -1 .. -5; N == 0 returns 0; nothing is written"""
    from rfn_hip import lib as L
    a, pk, p = torch.zeros(4096, device="cuda"), torch.zeros(32768, device="cuda"), torch.zeros(64, device="cuda")
    s = Bufs(2)
    o1, o2 = (L.dev(b) for b in s.b)

    def args(in1=L.dev(a), ns1=16, C1=2, in2=L.dev(a), ns2=8, C2=2, o2=None, Cout=4, split=4, N=2, H=2, W=2, ep=0,
             p0=None, p1=None):
        return (in1, ns1, C1, in2, ns2, C2, L.dev(pk), o1, 16, o2, 16, Cout, split, 0, N, H, W, ep, p0, p1, 0)
    rejected(CONV, -1, args(in1=None), s)
    rejected(CONV, -1, args(in2=None), s)                    # C2 > 0 without in2
    rejected(CONV, -1, args(ns1=136, C1=8, C2=0, H=1, W=17), s)
    rejected(CONV, -2, args(split=3), s)                     # cout_split without out2
    rejected(CONV, -2, args(split=0), s)
    rejected(CONV, -2, args(split=5, o2=o2), s)
    rejected(CONV, -3, args(ep=1, p1=L.dev(p)), s)           # ep_mode without p0
    rejected(CONV, -3, args(ep=2, p0=L.dev(p)), s)           # modes 1 / 2 without p1
    rejected(CONV, -3, args(ep=4, p0=L.dev(p), p1=L.dev(p)), s)
    rejected(CONV, -4, args(C1=1, C2=1), s)                  # C1*HW % 8
    rejected(CONV, -4, args(C2=1), s)                        # (C1+C2)*HW % 8
    rejected(CONV, -4, args(ns1=18), s)                      # in1_ns % 4
    rejected(CONV, -4, args(ns2=10), s)
    rejected(CONV, -5, args(in1=L.dev(a[1:])), s)
    rejected(CONV, -5, args(in2=L.dev(a[1:])), s)
    accepted_without_writing(CONV, args(N=0, split=2, o2=o2), s)
