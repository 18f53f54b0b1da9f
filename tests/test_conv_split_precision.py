"""The split-precision forward convolutions and their weight packs against plain high-precision references.

1. rfn_conv2d_fwd_bf16x6 (three bf16 pieces per operand, six MFMAs per product: the shipped forward arithmetic of every
   unfused convolution on maps larger than 2x2), rfn_conv2d_fwd_bf16x3 and the fp32-MFMA kernel on the same inputs,
   each against F.conv2d in float64 on the CPU.  Two error measures:
     e_rel = max |y - y64| / max |y64|                   (max-norm relative, as relerr in test_hip_kernels)
     e_abs = max over outputs of |y - y64| / S,  S = conv2d(|x|, |w|) in fp64 (the sum of |a*b| of each output)
   fp32 MFMA is a k-ordered fp32 fma chain: about 0.75-1.5e-7 * S at K <= 1024 and 3.5e-7 at K = 4096.
   Measured on an MI355X (FWD_CASES, max over the checked frames), e_abs of f32 / bf16x6 / bf16x3 and, at K <= 160,
   the ratio e_rel(bf16x3) / e_rel(bf16x6):
     K=21   (1x1 21->130, 6x6)        2.6e-7 / 1.1e-7 / 9.4e-6   ratio 106
     K=72   (3+5 -> 40, 6x6)          1.7e-7 / 9.3e-8 / 4.1e-6   ratio 42
     K=144  (16->16, 64x64)           3.2e-7 / 1.4e-7 / 3.6e-6   ratio 25
     K=144  (16->64, 64x64, 9 frames) 3.6e-7 / 3.2e-7 / 3.9e-6   ratio 10.7 (the smallest)
     K=216  (24->96, 32x32, 36 frames) 2.8e-7 / 2.8e-7 / 2.8e-6
     K=256  (1x1 256->288, 4x4)       2.7e-7 / 1.9e-7 / 1.8e-6
     K=2304 (split-K 256->512, 4x4)   4.1e-8 / 3.4e-8 / 8.0e-7
     K=4608 (split-K 300+212->96)     2.7e-8 / 2.1e-8 / 6.2e-7
   The fp32-MFMA maximum (3.6e-7 at K=144) sits above the 0.75-1.5e-7 typical figure: it is the worst of ~1.5 million
   outputs, final rounding included.  With the two third-plane products removed from the bf16x6 kernel, its e_abs rises
   to 1.4-6.1e-6 at K <= 256 and 4.7e-7 / 6.7e-7 at K = 4608 / 2304: every case fails, the large-K ones through the
   comparison with fp32 MFMA.
2. The routes to the weight pack kernels (one-descriptor entry points, host descriptor tables, PackPlan, PackBatch),
   modes 0 / 1 / 2 with two and three planes, and the small-map dense packs, bit for bit against CPU restatements of
   the layouts, with nothing written past the packed extent.
3. The arithmetic every forward convolution of the canonical SM-MNIST model actually gets under RFN_CONV_PRECISION=mixed.
"""
import ctypes
import inspect

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PRECS = ("f32", "bf16x6", "bf16x3")


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    return ops


def ref64(x1, x2, w, ks):
    """fp64 CPU reference of the raw convolution and S = conv2d(|x|, |w|)"""
    x = (x1 if x2 is None else torch.cat([x1, x2], 1)).double()
    w = w.double()
    return F.conv2d(x, w, padding=ks // 2), F.conv2d(x.abs(), w.abs(), padding=ks // 2)


def errs(y, y64, s):
    """(e_rel, e_abs) of a device result y against the fp64 reference y64 with S = s"""
    d = (y.detach().cpu().double() - y64).abs()
    return float(d.max() / (y64.abs().max() + 1e-300)), float((d / (s + 1e-30)).max())


def frame_slices(N):
    """frames the CPU reference covers: all of them, or the first and the last three"""
    return [slice(0, N)] if N <= 6 else [slice(0, 3), slice(N - 3, N)]


def conv(K, prec, x1, x2, w, Cout, ks, **kw):
    return K.conv2d_raw(x1, x2, K.pack_weight(w, prec=prec), Cout, ks, prec=prec, **kw)


@pytest.fixture
def seen_kernels(monkeypatch):
    """labels (meta[1]) of the convolution launches, recorded through rfn_hip.lib.call"""
    from rfn_hip import lib
    seen = []
    orig = lib.call

    def call(name, *args, meta=None):
        if name.startswith("rfn_conv2d_fwd_"):
            seen.append((name, None if meta is None else meta[1]))
        return orig(name, *args, meta=meta)
    monkeypatch.setattr(lib, "call", call)
    return seen


# --------------------------------------------------------------------------------- 1. forward convolution vs fp64
# the seven bf16x6 instantiations of dispatch_conv_b3 (csrc/conv_bf16x3.hip, npl == 3): <KS, WCO, WPX, TCO, TPX, KC>
X6_KERNELS = {"conv_b3_kernel<3,1,4,1,1,16>", "conv_b3_kernel<3,2,2,1,1,16>", "conv_b3_kernel<3,2,2,1,2,16>",
              "conv_b3_kernel<1,1,4,1,1,32>", "conv_b3_kernel<1,2,2,1,1,32>", "conv_b3_kernel<1,2,2,2,2,32>",
              "conv_b3_kernel<1,4,1,2,2,32>"}

FWD_CASES = [
    # N, C1, C2, Cout, H, W, ks
    (4, 16, 0, 16, 64, 64, 3),      # extractor 16 -> 16 on 64x64: Cout <= 32, W = 64 (two column tiles)
    (3, 3, 5, 40, 6, 6, 3),         # two sources, boundary inside an 8-channel group, Cin 8; few pixels, 6x6
    (9, 16, 0, 64, 64, 64, 3),      # many pixels (36864): 64 co x 128 px tiles
    (230, 20, 0, 48, 12, 12, 3),    # many pixels on 12x12 (ragged 16x8 tiles), Cin not a multiple of 16
    (37, 24, 0, 96, 3, 5, 3),       # 3x5 map, odd frame count: partial frame tile
    (5, 4, 14, 256, 8, 8, 3),       # 4 + 14 sources, two cout blocks
    (5, 40, 0, 24, 3, 5, 1),        # 1x1, Cout <= 32, partial frame tile
    (6, 100, 0, 64, 12, 12, 1),     # 1x1, Cout <= 64
    (7, 21, 0, 130, 6, 6, 1),       # 1x1, few pixels, Cout > 128 (partial cout block), Cin 21
    (300, 64, 0, 128, 12, 12, 1),   # 1x1, Cout <= 128, not few-pixel
    (800, 256, 0, 288, 4, 4, 1),    # level-3 tap-expanded Conv2dZeros: 9 * 32 outputs, second 256 block mostly padding
    (4, 256, 0, 512, 4, 4, 3),      # split-K (8 workgroups, 16 chunks), K = 2304
    (3, 300, 212, 96, 4, 4, 3),     # split-K with two sources, K = 4608
    (36, 24, 0, 96, 32, 32, 3),     # many pixels (36864), more than 64 outputs: the fp32 kernel's 128 co x 128 px tile
]


def _x6_label(K, case):
    N, C1, C2, Cout, H, W, ks = case
    return K.kernel_label("rfn_conv2d_kernel_label_bf16x3", 3, ks, C1, C2, Cout, Cout, 0, 0, N, H, W)


def test_forward_cases_reach_every_bf16x6_instantiation(K):
    assert {_x6_label(K, c) for c in FWD_CASES} == X6_KERNELS


# the nine production routes of choose_conv_f32 (csrc/conv.hip), F3_COUT32 to F1_256x64; the RFN_CONV_VARIANT ones are not
F32_KERNELS = {"conv_mfma_kernel<3,1,4,1,2,8>", "conv_mfma_kernel<3,1,4,2,1,8>", "conv_mfma_kernel<3,4,1,1,1,8>",
               "conv_mfma_kernel<3,2,2,2,2,8>", "conv_mfma_kernel<1,1,4,1,2,32>", "conv_mfma_kernel<1,1,4,2,1,32>",
               "conv_mfma_kernel<1,4,1,1,1,32>", "conv_mfma_kernel<1,2,2,2,2,32>", "conv_mfma_kernel<1,4,1,2,2,32>"}


def test_forward_cases_reach_every_fp32_route(K):
    labels = {K.kernel_label("rfn_conv2d_kernel_label_f32", ks, Cout, N, H, W) for N, _, _, Cout, H, W, ks in FWD_CASES}
    assert labels == F32_KERNELS


def _inputs(case, seed):
    N, C1, C2, Cout, H, W, ks = case
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(N, C1, H, W, generator=g)
    x2 = torch.randn(N, C2, H, W, generator=g) if C2 else None
    w = torch.randn(Cout, C1 + C2, ks, ks, generator=g) / ((C1 + C2) * ks * ks) ** 0.5
    return x1, x2, w


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "N%d_%d+%d_%d_%dx%d_k%d" % c)
def test_forward_three_arithmetics_vs_fp64(K, case, seen_kernels):
    """f32 and bf16x6 are fp32-grade (e_abs <= 4e-7 up to K = 4608); bf16x6 tracks the fp32 MFMA kernel on the same
    inputs; and at K <= 160, where the two-piece representation error (2^-17 per operand) dominates fp32 accumulation
    error, bf16x3 is at least 8x worse than bf16x6 -- so a bf16x6 that silently lost its third plane fails here."""
    N, C1, C2, Cout, H, W, ks = case
    Kdim = (C1 + C2) * ks * ks
    x1, x2, w = _inputs(case, 100 + Cout + ks)
    x1d, x2d, wd = x1.cuda(), None if x2 is None else x2.cuda(), w.cuda()
    ys = {p: conv(K, p, x1d, x2d, wd, Cout, ks) for p in PRECS}
    torch.cuda.synchronize()
    assert ("rfn_conv2d_fwd_bf16x6", _x6_label(K, case) + " x6") in seen_kernels
    e = {p: [0.0, 0.0] for p in PRECS}
    for sl in frame_slices(N):
        y64, s = ref64(x1[sl], None if x2 is None else x2[sl], w, ks)
        for p in PRECS:
            r, a = errs(ys[p][sl], y64, s)
            e[p] = [max(e[p][0], r), max(e[p][1], a)]
    msg = "K=%d " % Kdim + " ".join("%s: e_rel %.3g e_abs %.3g" % (p, *e[p]) for p in PRECS)
    print(msg)
    assert e["f32"][1] <= 4e-7, msg
    assert e["bf16x6"][1] <= 4e-7, msg
    assert e["bf16x6"][1] <= 3 * e["f32"][1] + 2e-8, msg
    if Kdim <= 160:
        assert e["bf16x3"][0] >= 8 * e["bf16x6"][0], msg


def test_splitk_forward_is_bitwise_repeatable(K):
    """the split-K slices are added in a fixed order (splitk_reduce): two runs agree bit for bit"""
    case = (4, 256, 0, 512, 4, 4, 3)
    x1, _, w = _inputs(case, 7)
    x, wd = x1.cuda(), w.cuda()
    for p in ("bf16x6", "bf16x3"):
        wpk = K.pack_weight(wd, prec=p)
        a = K.conv2d_raw(x, None, wpk, 512, 3, prec=p)
        b = K.conv2d_raw(x, None, wpk, 512, 3, prec=p)
        assert torch.equal(a, b), p


@pytest.mark.parametrize("acc", [False, True])
def test_forward_channel_slice_views(K, acc):
    """in1 = z[:, :Ch] of a wider tensor (as GlowStepRevFn passes it) plus a second source, the output split over two
    channel-slice views (cout_split) with and without accumulation; channels outside the views stay untouched."""
    g = torch.Generator().manual_seed(11)
    N, Ch, Cc, Cout, split, H, W = 6, 6, 10, 64, 24, 8, 8
    z = torch.randn(N, 2 * Ch, H, W, generator=g)
    cond = torch.randn(N, Cc, H, W, generator=g)
    w = torch.randn(Cout, Ch + Cc, 3, 3, generator=g) / (9 * (Ch + Cc)) ** 0.5
    big1 = torch.randn(N, split + 5, H, W, generator=g)
    big2 = torch.randn(N, Cout - split + 3, H, W, generator=g)
    y64, s = ref64(z[:, :Ch], cond, w, 3)
    if acc:  # out = base + conv: the base enters the error scale
        y64 = y64 + torch.cat([big1[:, 2:2 + split], big2[:, :Cout - split]], 1).double()
        s = s + torch.cat([big1[:, 2:2 + split], big2[:, :Cout - split]], 1).double().abs()
    for p in PRECS:
        b1, b2 = big1.cuda(), big2.cuda()
        conv(K, p, z.cuda()[:, :Ch], cond.cuda(), w.cuda(), Cout, 3, out1=b1[:, 2:2 + split], out2=b2[:, :Cout - split],
             cout_split=split, acc1=acc, acc2=acc)
        b1, b2 = b1.cpu(), b2.cpu()
        assert torch.equal(b1[:, :2], big1[:, :2]) and torch.equal(b1[:, 2 + split:], big1[:, 2 + split:]), p
        assert torch.equal(b2[:, Cout - split:], big2[:, Cout - split:]), p
        y = torch.cat([b1[:, 2:2 + split], b2[:, :Cout - split]], 1)
        e_rel, e_abs = errs(y, y64, s)
        assert e_abs <= (4e-7 if p != "bf16x3" else 2e-5), (p, e_rel, e_abs)


@pytest.mark.parametrize("ep_mode,act", [(1, 0), (1, 1), (1, 2), (2, 0), (3, 0)])
@pytest.mark.parametrize("ks", [3, 1])
def test_bf16x6_epilogues_vs_fp64(K, ep_mode, act, ks):
    """the fused epilogues on the bf16x6 path: Conv2dNorm (ActNorm + activation), Conv2dZeros, biased conv"""
    g = torch.Generator().manual_seed(12 + ep_mode + act)
    N, Cin, Cout, H, W = 4, 20, 48, 6, 6
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    p0 = torch.randn(Cout, generator=g) * 0.3
    p1 = torch.randn(Cout, generator=g) * 0.2
    u = ref64(x, None, w, ks)[0] + p0.double().view(1, -1, 1, 1)
    if ep_mode == 1:
        u = u * p1.double().exp().view(1, -1, 1, 1)
        ref = u if act == 0 else (u.clamp_min(0.0) if act == 1 else torch.where(u > 0, u, 0.2 * u))
    elif ep_mode == 2:
        ref = u * (3 * p1.double()).exp().view(1, -1, 1, 1)
    else:
        ref = u
    out = conv(K, "bf16x6", x.cuda(), None, w.cuda(), Cout, ks, ep_mode=ep_mode, p0=p0.cuda(),
               p1=p1.cuda() if ep_mode != 3 else None, act=act)
    e_rel = errs(out, ref, ref.abs())[0]
    assert e_rel <= 2e-6, e_rel


@pytest.mark.parametrize("N,Cin,C,H,W", [(3, 64, 4, 8, 8), (2, 256, 8, 16, 16), (5, 24, 2, 3, 5)])
def test_bf16x6_tap_expanded_zeros_conv_vs_fp64(K, N, Cin, C, H, W):
    """Conv2dZeros with tiny Cout (1x1 to 9C channels + tap gather, zeros_conv_fwd) in bf16x6: the level-3 / BAIR-shaped
    coupling nets' last convolution"""
    g = torch.Generator().manual_seed(13)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(C, Cin, 3, 3, generator=g) * 0.1
    b = torch.randn(C, generator=g) * 0.2
    l = torch.randn(C, generator=g) * 0.1
    ref = (ref64(x, None, w, 3)[0] + b.double().view(1, C, 1, 1)) * (3 * l.double()).exp().view(1, C, 1, 1)
    o = K.zeros_conv_fwd(x.cuda(), w.cuda(), b.cuda(), l.cuda(), prec="bf16x6")
    assert errs(o, ref, ref.abs())[0] <= 2e-6


# --------------------------------------------------------------------------------- 2. weight packs, bit for bit
def pack_ref(w, mode, npl):
    """CPU restatement of the split-precision weight pack (pack_weights_table_b3_kernel) as int16 bits.
    Logical weight wl[co][ci][tap]: mode 0 = w; mode 1 (data gradient) = w transposed with mirrored taps; mode 2
    (tap-expanded 1x1) = w.permute(2,3,0,1).reshape(9*Cout, Cin).  Planes hi = bf16(v), mid = bf16(v - hi),
    lo = bf16((v - hi) - mid) (round to nearest even; the fp32 subtractions are exact); two-plane packs hold (hi, mid).
    Unit (16 bytes) index (((c16*T + tap)*NPL + plane)*2 + g)*CoutP + co, element j <-> ci = c16*16 + g*8 + j."""
    Cout, Cin, ks = (int(d) for d in w.shape[:3])
    wf = w.reshape(Cout, Cin, ks * ks)
    if mode == 0:
        wl = wf
    elif mode == 1:
        wl = wf.transpose(0, 1).flip(2)
    else:
        wl = wf.permute(2, 0, 1).reshape(ks * ks * Cout, Cin, 1)
    Co, Ci, T = wl.shape
    CoutP, Cin16 = -(-Co // 256) * 256, -(-Ci // 16)
    v = torch.zeros(CoutP, Cin16 * 16, T)
    v[:Co, :Ci] = wl
    hi = v.to(torch.bfloat16)
    r1 = v - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    planes = [p.view(CoutP, Cin16, 2, 8, T).permute(1, 4, 2, 0, 3) for p in (hi, mid, lo)[:npl]]  # [c16,tap,g,co,j]
    return torch.stack(planes, 2).contiguous().view(torch.int16).reshape(-1)


def _weight(shape, seed):
    """random weight over several decades, with bf16 ties (1 + 2^-8: half way between two bf16 numbers; and ties of
    the second piece) and signed zeros among the first elements"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * torch.exp(torch.randn(shape, generator=g) * 3)
    special = torch.tensor([1.0 + 2.0 ** -8, -(1.0 + 3 * 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -17, 0.0, -0.0,
                            3.0 * 2.0 ** -9, 65504.0, -1e-30])
    w.view(-1)[:special.numel()] = special
    return w


SENTINEL = 0x5A5AA5A5  # int32 bit pattern of the untouched buffer


def _sentinel_buf(nfloats):
    return torch.full((nfloats,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _check_pack(buf, ref, what):
    """bit-exact packed extent; everything after it still holds the sentinel"""
    used = ref.numel() // 2  # floats
    assert used <= buf.numel(), what
    got = buf.view(torch.int32).cpu()
    assert torch.equal(got[:used].view(torch.int16), ref), what
    assert bool((got[used:] == SENTINEL).all()), (what, "written past the packed extent")


PACK_SHAPES = [(300, 21, 3), (7, 37, 3), (270, 45, 1), (33, 300, 1), (5, 16, 3)]
MARGIN = 1024  # floats of sentinel after the allocation size the library asks for


def _size(lib, npl, Cout, Cin, ks):
    return int((lib.rfn_packed_weight_size_bf16x6 if npl == 3 else lib.rfn_packed_weight_size_bf16x3)(Cout, Cin, ks))


@pytest.mark.parametrize("npl", [2, 3])
@pytest.mark.parametrize("shape", PACK_SHAPES)
def test_pack_direct_route_bit_exact(K, shape, npl):
    """rfn_pack_conv_weight_bf16x{3,6}: modes 0 and 1; mode 2 as the mode-0 pack of the tap-major 1x1 weight (the
    other route zeros_conv_fwd takes); the size function covers both orientations"""
    from rfn_hip import lib as L
    lib = L.load()
    Cout, Cin, ks = shape
    w = _weight(shape + (ks,), 20 + Cout)
    fn = "rfn_pack_conv_weight_bf16x6" if npl == 3 else "rfn_pack_conv_weight_bf16x3"
    size = _size(lib, npl, Cout, Cin, ks)
    wd = w.cuda()
    for flip in (0, 1):
        ref = pack_ref(w, flip, npl)
        assert ref.numel() // 2 <= size, ("size function", flip)
        buf = _sentinel_buf(size + MARGIN)
        L.call(fn, L.dev(wd), L.dev(buf), ctypes.c_int(Cout), ctypes.c_int(Cin), ctypes.c_int(ks), ctypes.c_int(flip))
        _check_pack(buf, ref, ("direct", shape, npl, flip))
    if ks == 3:
        wt = w.permute(2, 3, 0, 1).reshape(9 * Cout, Cin, 1, 1).contiguous()
        ref = pack_ref(w, 2, npl)
        assert torch.equal(ref, pack_ref(wt, 0, npl))
        buf = _sentinel_buf(_size(lib, npl, 9 * Cout, Cin, 1) + MARGIN)
        L.call(fn, L.dev(wt.cuda()), L.dev(buf), ctypes.c_int(9 * Cout), ctypes.c_int(Cin), ctypes.c_int(1), ctypes.c_int(0))
        _check_pack(buf, ref, ("direct tap-major", shape, npl))


def _desc_items():
    """(weight, mode) over every shape, mode 0 / 1 / 2 (ks 3 only) and plane count"""
    items = []
    for i, (Cout, Cin, ks) in enumerate(PACK_SHAPES):
        w = _weight((Cout, Cin, ks, ks), 40 + i)
        for mode in ((0, 1, 2) if ks == 3 else (0, 1)):
            for x6 in (0, 4):
                items.append((w, mode + x6))
    return items


def _mode_size(lib, w, mode):
    Cout, Cin, ks = (int(d) for d in w.shape[:3])
    npl = 3 if mode & 4 else 2
    return _size(lib, npl, 9 * Cout, Cin, 1) if (mode & 3) == 2 else _size(lib, npl, Cout, Cin, ks)


@pytest.mark.parametrize("n_rep", [1, 3])
def test_pack_hostdescs_route_bit_exact(K, n_rep):
    """rfn_pack_conv_weights_hostdescs_bf16x3 (what PackBatch and PackPlan launch): every mode, two and three planes;
    n_rep=3 hands over 78 descriptors, more than one 64-entry kernel-argument table"""
    from rfn_hip import lib as L
    lib = L.load()
    items = _desc_items() * n_rep
    assert (len(items) > 64) == (n_rep > 1)
    wds = {id(w): w.cuda() for w, _ in items}
    bufs = [_sentinel_buf(_mode_size(lib, w, m) + MARGIN) for w, m in items]
    arr = (L.rfn_pack_desc * len(items))(*[L.rfn_pack_desc(wds[id(w)].data_ptr(), b.data_ptr(), int(w.shape[0]),
                                                           int(w.shape[1]), int(w.shape[2]), m)
                                           for (w, m), b in zip(items, bufs)])
    L.call("rfn_pack_conv_weights_hostdescs_bf16x3", ctypes.cast(arr, ctypes.c_void_p), ctypes.c_int(len(items)))
    for i, ((w, m), b) in enumerate(zip(items, bufs)):
        _check_pack(b, pack_ref(w, m & 3, 3 if m & 4 else 2), ("hostdescs", i, tuple(w.shape), m))


def test_pack_plan_bit_exact(K):
    """PackPlan (the flow's per-step pack plan, descriptors built once, rfn_pack_conv_weights_hostdescs_bf16x3): every
    mode, two and three planes, sentinel-filled buffers; with three repetitions the plan holds 78 descriptors, more
    than one table"""
    for n_rep in (1, 3):
        items = [(w.cuda(), m) for w, m in _desc_items() * n_rep]
        plan = K.PackPlan(items)
        for b in plan.bufs:
            b.view(torch.int32).fill_(SENTINEL)
        plan.run()
        for (w, m), b in zip(items, plan.bufs):
            _check_pack(b, pack_ref(w.cpu(), m & 3, 3 if m & 4 else 2), ("pack plan", n_rep, tuple(w.shape), m))


def smallmap_dense_matrix(w, H, W, transpose):
    """the dense matrix of a 3x3 / pad 1 convolution on an H x W map, in w's dtype and before any padding:
    M[(ci,pi)][(co,po)] = w[co][ci][tap(po, pi)] (transpose: M^T)"""
    Cout, Cin, HW = int(w.shape[0]), int(w.shape[1]), H * W
    M = torch.zeros(Cin * HW, Cout * HW, dtype=w.dtype)
    for po in range(HW):
        for pi in range(HW):
            dy, dx = pi // W - po // W + 1, pi % W - po % W + 1
            if 0 <= dy < 3 and 0 <= dx < 3:
                M[pi::HW, po::HW] = w[:, :, dy, dx].t()
    return M.t() if transpose else M


def smallmap_pack_ref(w, H, W, transpose):
    """CPU restatement of the small-map dense pack (smallmap_pack_batched_kernel) as int16 bits.  Dense matrix
    M[(ci,pi)][(co,po)] = w[co][ci][tap(po, pi)] (transpose: M^T), zero-padded to KS*16 rows and NT*32 columns, split
    into bf16 hi = bf16(v), lo = bf16(v - hi); unit index ((tile*KS + ks)*2 + plane)*64 + lane, element j <->
    k = ks*16 + (lane/32)*8 + j, n = tile*32 + lane%32."""
    M = smallmap_dense_matrix(w, H, W, transpose)
    KS, NT = -(-M.shape[0] // 16), -(-M.shape[1] // 32)
    P = torch.zeros(KS * 16, NT * 32)
    P[:M.shape[0], :M.shape[1]] = M
    hi = P.to(torch.bfloat16)
    lo = (P - hi.float()).to(torch.bfloat16)
    planes = [p.view(KS, 2, 8, NT, 32).permute(3, 0, 1, 4, 2) for p in (hi, lo)]   # [tile, ks, lane/32, lane%32, j]
    return torch.stack(planes, 2).contiguous().view(torch.int16).reshape(-1)


SMALLMAP_SHAPES = [(12, 5, 2, 2), (7, 16, 4, 4), (33, 3, 1, 3), (64, 40, 2, 4), (3, 9, 3, 3)]


@pytest.mark.parametrize("shape", SMALLMAP_SHAPES)
def test_smallmap_pack_direct_route_bit_exact(K, shape):
    """rfn_smallmap_pack_bf16x3 (the one-descriptor entry point), both orientations, sentinel-filled buffers"""
    from rfn_hip import lib as L
    Cout, Cin, H, W = shape
    w = _weight((Cout, Cin, 3, 3), 120 + Cout)
    wd = w.cuda()
    for tr in (0, 1):
        ref = smallmap_pack_ref(w, H, W, tr)
        nbytes = int(L.load().rfn_smallmap_packed_size(Cout, Cin, H, W, tr))
        assert nbytes == 2 * ref.numel(), ("size function", shape, tr)
        buf = _sentinel_buf(nbytes // 4 + MARGIN)
        L.call("rfn_smallmap_pack_bf16x3", L.dev(wd), ctypes.c_int(Cout), ctypes.c_int(Cin), ctypes.c_int(H),
               ctypes.c_int(W), ctypes.c_int(tr), L.dev(buf))
        _check_pack(buf, ref, ("smallmap direct", shape, tr))


def test_pack_batch_of_70_one_launch_per_kind(K, monkeypatch):
    """70 conv packs and 70 small-map packs asked for in ONE PackBatch (two kernel-argument tables each) leave in
    exactly one rfn_pack_conv_weights_hostdescs_bf16x3 and one rfn_smallmap_pack_batched_bf16x3 call, made when the
    batch is left, and land bit for bit where the returned buffers say, in the orientation and plane count asked for"""
    from rfn_hip import lib as L
    calls, real = [], L.call

    def spy(name, *args, **kw):
        calls.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(L, "call", spy)
    asked, dense = [], []
    with K.PackBatch() as pb:
        for i in range(70):
            Cout, Cin, ks = PACK_SHAPES[i % len(PACK_SHAPES)]
            w = _weight((Cout, Cin, ks, ks), 60 + i)
            flip, prec = bool(i % 2), ("bf16x6", "bf16x3")[(i // 2) % 2]
            asked.append((w, flip, prec, pb.conv(w.cuda(), flip=flip, prec=prec)))
            Cout, Cin, H, W = SMALLMAP_SHAPES[i % len(SMALLMAP_SHAPES)]
            w = _weight((Cout, Cin, 3, 3), 140 + i)
            tr = bool((i // 5) % 2)
            dense.append((w, H, W, tr, pb.dense(w.cuda(), H, W, tr)))
        assert calls == []
    assert calls == ["rfn_pack_conv_weights_hostdescs_bf16x3", "rfn_smallmap_pack_batched_bf16x3"]
    for w, flip, prec, b in asked:
        ref = pack_ref(w, int(flip), 3 if prec == "bf16x6" else 2)
        assert torch.equal(b.view(torch.int32).cpu()[:ref.numel() // 2].view(torch.int16), ref), (tuple(w.shape), flip, prec)
    for w, H, W, tr, b in dense:
        ref = smallmap_pack_ref(w, H, W, tr)
        assert ref.numel() == 2 * b.numel(), ("size", tuple(w.shape), H, W, tr)
        assert torch.equal(b.view(torch.int32).cpu().view(torch.int16), ref), (tuple(w.shape), H, W, tr)


# --------------------------------------------------------------------------------- 3. arithmetic of the forward pass
def test_mixed_forward_pass_uses_the_forward_arithmetic(K, monkeypatch):
    """RFN_CONV_PRECISION=mixed, canonical SM-MNIST architecture (all five levels, canonical widths) at B=2, T=3: the
    first training forward (with the data dependent ActNorm init), a second one and a prediction.  Every forward
    convolution through conv2d_raw runs in ops.fwd_prec(H, W) of its map, and the dense small-map kernels only see maps
    of at most 2x2.
    One deliberate exception: the extractor / upscaler convolutions (run_time_batched) run bf16x6 at every map size,
    2x2 included (fwd_prec says bf16x3 there) -- they replace fp32 MIOpen convolutions, so they stay fp32-grade."""
    import main_rfn
    from RFN import RFN
    from Utils import modules as M
    monkeypatch.setattr(K, "CONV_PRECISION", "mixed")
    monkeypatch.setattr(K, "MIXED_FWD", "bf16x6")
    rec, vgg = [], [0]

    def spy(name, fn, first, prec_of=None):
        sig = inspect.signature(fn)

        def wrapped(*a, **k):
            b = sig.bind(*a, **k)
            t = b.arguments[first]
            prec = None
            if prec_of is not None:
                prec = b.arguments.get("prec") or ("bf16x3" if K.bwd_b3() else "f32")
            rec.append((name, int(t.shape[2]), int(t.shape[3]), prec, vgg[0] > 0))
            return fn(*a, **k)
        monkeypatch.setattr(K, name, wrapped)

    spy("conv2d_raw", K.conv2d_raw, "in1", prec_of=True)
    for name, first in (("smallmap_conv", "in1"), ("smallmap_dense", "a"), ("smallmap_dense_pair", "a0")):
        spy(name, getattr(K, name), first)
    orig_rtb = M.run_time_batched

    def rtb(*a, **k):
        vgg[0] += 1
        try:
            return orig_rtb(*a, **k)
        finally:
            vgg[0] -= 1
    monkeypatch.setattr(M, "run_time_batched", rtb)

    B, T = 2, 3
    args = main_rfn.build_parser().parse_args(main_rfn.canonical_smmnist_argv(B, T))
    torch.manual_seed(81)
    m = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(82)
    x = ((torch.rand(B, T, 1, 64, 64, generator=g) * 255).floor() / 256 - 0.5).cuda()
    zshape = tuple(m.z_0.shape)
    draws = []
    for _ in range(T - 1):
        draws += [torch.randn(zshape, generator=g).cuda(), torch.randn(zshape, generator=g).cuda(),
                  (torch.rand(B, 1, 64, 64, generator=g) / 256).cuda()]
    m.loss(x, 0, draws=draws)   # data dependent ActNorm init
    n_first = len(rec)
    kl_fb, kl, nll = m.loss(x, 0, draws=draws)
    assert bool(torch.isfinite(nll))
    pdraws = [torch.randn(zshape, generator=g).cuda() for _ in range(2)]
    pdraws += [torch.randn(s, generator=g).cuda() for s in m._gen_eps_shapes(B)]
    _, pred = m.predict(x, 1, 2, draws=pdraws)
    assert bool(torch.isfinite(pred).all())
    torch.cuda.synchronize()

    convs = [r for r in rec if r[0] == "conv2d_raw"]
    assert n_first > 0 and len(rec) > n_first and convs
    maps = {(h, w) for _, h, w, _, _ in convs}
    assert {(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)} <= maps | {(h, w) for _, h, w, _, _ in rec}, maps
    bad = []
    for name, h, w, prec, in_vgg in convs:
        want = K.fwd_prec(h, w)
        if prec == want or (in_vgg and prec == "bf16x6" and want == "bf16x3"):
            continue
        bad.append((h, w, prec, want, "extractor/upscaler" if in_vgg else ""))
    assert not bad, sorted(set(bad))
    dense = sorted({(h, w) for name, h, w, _, _ in rec if name != "conv2d_raw"})
    assert dense and all(h * w <= 4 for h, w in dense), dense
