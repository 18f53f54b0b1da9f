"""Every split-precision weight-gradient route against the three-product model, and EXACTLY on two-piece operands.

tests/test_conv_grad_model.py holds a bf16x3 kernel to  y3 = op(a_hi, b_hi + b_lo) + op(a_lo, b_hi)  (fp64 on the CPU;
hi = bf16(v), lo = bf16(v - hi)).  The mirrored, short-row and level-split routes were written after it and were held
only to relerr < 2e-5 against fp64, or to equality on integers whose `lo` piece is zero.  This module has two halves.

1. Model bounds (ROUTE_CASES, test_route_vs_model): randn operands, the first input source of the last group times 3
   plus 0.5, inputs channel slices of wider tensors where the case says so, the gradient also times 2^-40; each case ends
   in check_wgrad of test_conv_grad_model, unchanged: e_abs vs the model <= 3 e_abs(fp32-MFMA kernel vs fp64) + 2e-8 and
   <= WGRAD_CAP (the short-row family: ROWS_CAP, derived below), vs fp64 <= SPLIT_BOUND, the 2^-40 figure.  The
   (entry point, label) of every launch and, for the ring launches, the workgroups that change group in mid-range
   (rfn_wgrad_split_parts) are asserted.

2. Exact (EXACT_CASES, test_exact_on_two_piece_operands): operands v = (hi + lo) keep with hi uniform in {-1, 0, 1},
   lo = n 2^-9, n uniform in {-1, 0, 1} and 0 where hi == 0, keep Bernoulli(d).  Asserted on the CPU before the launch:
   split(v) returns exactly these pieces and lo is not all zero; S = op(|a|, |b|) has S.max() 2^9 < 2^22, so every term of
   the three-product sum is a multiple of 2^-9, every partial sum in any order is bounded by S and every fp32 addition,
   float atomics included, is exact; the model is a multiple of 2^-9 and survives .float().double(); it differs from
   op(a, b) (the dropped lo lo terms are multiples of 2^-18) and from op(a_hi, b_hi).  Then the kernel's result must
   EQUAL the model for every group.  A kernel that drops, duplicates or misplaces one lo element anywhere, or that also
   adds lo lo, gives another number.  d is the largest of {1, 1/2, 1/4, 1/8} that keeps S.max() under 4096 (density():
   S concentrates at K (2 d / 3)^2 for K summed pixels); the assertion in the test is the condition, the margin of two
   is for other seeds.  The cases: all of ROUTE_CASES, every row of GEMM_CASES, every split-precision row of
   WGRAD_CASES, the CASES of test_wgrad_band.py -- every label choose_gemm_wgrad, choose_wgrad_implicit,
   choose_wgrad_implicit_mirrored, the rows chooser and the band entry point can return, single and grouped
   (test_cases_cover_every_label; tests/test_kernel_routes_host.py asks the same of the plan without a device).

The fp64 references (three-product model, exact fp64, S) are computed once per (operand values, group) and shared by the
cases whose groups have the same values: a single launch is group 0 of its grouped twin, the mirrored ring and the
tap-scattered ring share 131 frames of 16x16, 256 -> 4.

Measured on an MI355X (max over the cases of a route; e_abs of bf16x3 vs the model / bf16x3 vs fp64 / fp32 kernel vs fp64):
  mirrored (rfn_conv3x3_wgrad_mirrored[_grouped]_bf16x3)        single                       grouped
    gemm_wgrad_dma_impl_kernel<4,2,2,1>                1.6e-8 / 8.1e-8 / 1.7e-8     2.1e-8 / 1.9e-7 / 4.9e-8  (five cases)
    gemm_wgrad_dma_impl_kernel<4,2,2,2>                1.6e-8 / 9.9e-8 / 1.6e-8     1.3e-8 / 1.8e-7 / 3.1e-8
    gemm_wgrad_dma_impl_kernel<4,2,2,3>                                             2.1e-8 / 4.2e-7 / 4.2e-8  (G = 10)
    gemm_wgrad_b3_kernel<2,2,2,2,64,1>, mirror = 1     4.4e-8 / 8.7e-7 / 3.0e-8     4.3e-8 / 9.7e-7 / 3.4e-8
    gemm_wgrad_b3_kernel<4,2,2,3,64,1>, mirror = 1     1.5e-8 / 1.0e-7 / 2.1e-8
  level split (grouped ring launches whose workgroups change group in mid-range)
    gemm_wgrad_dma_kernel<grouped 2,4,4,2,32,2>        G = 10: 2.9e-8 / 3.2e-7 / 3.8e-8    G = 15: 3.0e-8 / 4.2e-7 / 3.9e-8
    gemm_wgrad_dma_kernel<grouped 1,8,2,1,32,3>        1.4e-8 / 1.8e-7 / 4.9e-8  (after tap_scatter)
    gemm_wgrad_dma_impl_kernel<grouped 4,2,2,3>        1.5e-8 / 2.0e-7 / 3.1e-8
  short rows, K = 28 .. 640 pixels (six cases each, single and grouped together)
    gemm_wgrad_b3_kernel<2,2,2,2,64,2>  (4-pixel rows) 1.4e-7 / 4.2e-6 / 1.7e-7
    gemm_wgrad_b3_kernel<2,2,2,2,64,3>  (2 x 2 maps)    3.2e-7 / 1.1e-5 / 2.8e-7
  The sixteen mirrored and level-split cases pass check_wgrad as it is (largest e_abs vs the model 4.4e-8 beside
  WGRAD_CAP = 9.7e-8).  The twelve short-row cases meet 3 e_abs(fp32 kernel) + 2e-8 and exceed WGRAD_CAP: ROWS_CAP below.
  The module behaves the same under RFN_CONV_PRECISION=mixed and bf16x3: the weight-gradient routes do not depend on it.
Exact: 61 cases, 169 groups, every one EQUAL to the model.  Nothing was found wrong in the kernels.
Wall time of the module on the MI355X machine: 123 s for its 90 tests (at most 6.6 s each), of which the fp64 references
73 s (236 sets of values, the three-product model, exact fp64, S and op(a_hi, b_hi) of each) -- the references of the
ring-sized K, which no smaller shape reaches, are the cost.

Three deliberate faults, each in a scratch build of csrc/wgrad_bf16x3.hip (not committed; value-only), run on this
module and on test_wgrad_mirrored / _short_rows / _level_split / _band:
  (a) wg_shift_split4 writes lo[c0 + 3] from the unshifted v[3] when dx > 0 (a lo that is not zero-filled at the row
      end).  Here: all 12 short-row model cases fail at e_abs 3.4e-4 .. 2.8e-2 and all 12 short-row exact cases fail
      (22 .. 31 % of the outputs, by up to 30 x 2^-9); nothing else in the module fails.  The older suite: the fault is
      systematic, and the four test_model_channel_counts_against_fp64 cases (relerr 8.7e-4 .. 1.1e-3) and the level node
      (7.2e-4) fail too; test_exact_on_small_integers (lo == 0) and test_the_plan_is_what_runs pass all 16 cases.
  (b) the grouped ring kernels skip both lo products of the first 32-pixel stage after a change of group.  Here: the
      seven model cases whose workgroups change group fail at e_abs 3.4e-6 .. 2.0e-5 (tolerance 1.1e-7 .. 1.7e-7) and
      nine exact cases fail (those seven and the grouped GEMM_CASES / WGRAD_CASES rows on the 256-row rings, dma256_g3
      and impl_dma_g3, which no model case had chosen for a boundary inside a range): 27 .. 91 % of the outputs of every
      group but the first, by up to 23 x 2^-9.  Cases with no boundary inside a range (mir_narrow_g3: 393 workgroups, none
      crossing) pass, as they must.  The older suite does NOT pass this fault: 11 relerr tests fail at 4.3e-5 .. 2.6e-4
      against their 2e-5 (test_wgrad_mirrored 6, test_wgrad_level_split 5, the level node among them) -- a whole stage
      of a range of 10 .. 26 is more than the representation error on these shapes.
  (c) so a third, finer one: ONE lo element (lane 0 .. 31 of the first A fragment, first k-step) of that stage zeroed, i.e.
      one a_lo b_hi term per output row.  Here: the same seven model cases fail at 5.2e-7 .. 6.0e-6 and the same nine
      exact cases, with 96 .. 6864 outputs per group off by exactly 1 x 2^-9.  The older suite: 8 of the 11 still fail,
      at 1.0 .. 3.4 times their bound (2.0e-5 .. 6.8e-5); test_narrow_tile_three_groups,
      test_channel_slice_of_a_wider_tensor_72_columns and the level node pass.  With randn operands one element of the
      scaled last group is worth several 1e-5 of the largest output; on the two-piece operands it is 2^-9 wherever it
      falls, which is what the exact test is for.
"""
import collections
import time
import zlib

import pytest
import torch

from tests.test_conv_grad_model import (GEMM, GEMM_CASES, IMPL, K, SPLIT_BOUND, WGRAD_CAP, WGRAD_CASES,  # noqa: F401
                                        check, check_wgrad, e_abs, launches, merge, split, wgrad_f32, wgrad_op)
from tests.test_wgrad_band import CASES as BAND_CASES, ENTRY as BAND_ENTRY, band
from tests.test_wgrad_level_split import RING_256, RING_64 as GEMM_RING_64, RING_IMPL, _split
from tests.test_wgrad_mirrored import REG_128, REG_256, RING_128, RING_192, RING_64, _crossings
from tests.test_wgrad_short_rows import EXACT as ROWS_EXACT, LABEL as ROWS_LABEL, MODEL as ROWS_MODEL, ROWS, ROWS_MIRRORED

pytestmark = pytest.mark.gpu

# The short-row cases sum K = 28 .. 640 pixels, where WGRAD_CAP (the project's figure from K = 756 .. 134144) is below
# what fp32 accumulation itself costs: every one of them meets 3 e_abs(fp32-MFMA kernel) + 2e-8 and exceeds WGRAD_CAP
# (1.05e-7 .. 3.15e-7).  The cap of this family is three times the largest yardstick e_abs (fp32-MFMA kernel vs fp64)
# over its twelve cases at seeds 0, 1, 2 (measured on an MI355X; the largest e_abs vs the model at those seeds: 3.15e-7,
# 3.50e-7, 3.09e-7)
ROWS_YARDSTICK = (2.752e-7, 1.970e-7, 1.988e-7)
ROWS_CAP = 3 * max(ROWS_YARDSTICK)   # 8.26e-7

# kind: "gemm" K.gemm_wgrad[_grouped] (g = a [N, Cout, H, W], x = b [N, C1, H, W]); "conv" K.conv2d_wgrad[_grouped];
# "zeros" K.zeros_conv_wgrad[_grouped] (Conv2dZeros, C1 -> Cout: the mirrored forms); "band" the band entry point.
# G = 0: the single form.  xview / gview = (channels of the tensor, first channel): in1 / g is that channel slice of a
# wider tensor (None: dense; a dense gradient of a group is passed stacked).  short: short_rows=True.  want: the
# (entry point, label) of every launch.  ring = (query, argument, expected): _split(G, pixels, tiles = argument) or
# _crossings(G, stages, slots = argument) of the grouped ring launch.
Case = collections.namedtuple("Case", "kind G N C1 C2 Cout H W ks xview gview short want ring")
MIRRORED = ("rfn_conv3x3_wgrad_mirrored_bf16x3", "rfn_conv3x3_wgrad_mirrored_grouped_bf16x3")
TAP_SCATTER = ("rfn_tap_scatter_f32", "tap_scatter")


def grouped(label):
    return label.replace("<", "<grouped ")


def mirrored(G, N, Cin, C, H, W, label, Ctot=None, ring=None):
    """h2 = the LAST Cin channels of a tensor of Ctot"""
    want = [(MIRRORED[1], grouped(label)) if G else (MIRRORED[0], label)]
    return Case("zeros", G, N, Cin, 0, C, H, W, 3, (Ctot, Ctot - Cin) if Ctot else None, None, False, want, ring)


def short_rows(form, G, N, chans, S):
    if form == "implicit":
        Ctot, C1, C2, Cout = chans
        return Case("conv", G, N, C1, C2, Cout, S, S, 3, (Ctot, Ctot - C1) if Ctot != C1 else None, None, True,
                    [(ROWS[1 if G else 0], grouped(ROWS_LABEL[S]) if G else ROWS_LABEL[S])], None)
    Cin, C = chans
    return Case("zeros", G, N, Cin, 0, C, S, S, 3, None, None, True,
                [(ROWS_MIRRORED[1 if G else 0], grouped(ROWS_LABEL[S]) if G else ROWS_LABEL[S])], None)


ROUTE_CASES = {
    # ---- mirrored (the shapes of test_wgrad_mirrored.py)
    "mir_narrow_g3":      mirrored(3, 131, 256, 4, 16, 16, RING_64, ring=("crossings", 512, (393, 0))),
    "mir_narrow_g5":      mirrored(5, 131, 256, 4, 16, 16, RING_64, ring=("crossings", 512, (512, 4))),
    "mir_32px_rows_g4":   mirrored(4, 25, 256, 4, 32, 32, RING_64),
    "mir_72col_slice_g3": mirrored(3, 131, 256, 8, 16, 16, RING_128, Ctot=264),
    "mir_144col_g10":     mirrored(10, 160, 256, 16, 8, 8, RING_192),
    "mir_45col_g3":       mirrored(3, 131, 256, 5, 16, 16, RING_64),
    "mir_200rows_g3":     mirrored(3, 131, 200, 4, 16, 16, RING_64, Ctot=256),
    "mir_single_ring":    mirrored(0, 391, 256, 4, 16, 16, RING_64),              # 100096 pixels: the smallest
    "mir_single_72col":   mirrored(0, 391, 256, 8, 16, 16, RING_128),             # (the single label of the 128-column tile)
    "mir_reg":            mirrored(0, 21, 64, 8, 8, 8, REG_128),
    "mir_reg_g3":         mirrored(3, 21, 64, 8, 8, 8, REG_128),
    "mir_reg_hw24":       mirrored(0, 4200, 256, 4, 3, 8, REG_256),
    # ---- level split (the shapes of test_wgrad_level_split.py)
    "split_ring_g10":     Case("conv", 10, 40, 256, 0, 256, 16, 16, 1, None, None, False, [(GEMM[1], RING_256)],
                               ("split", 1, (256, 320, 8))),
    "split_ring_g15":     Case("conv", 15, 27, 256, 0, 256, 16, 16, 1, None, None, False, [(GEMM[1], RING_256)],
                               ("split", 1, (256, 216, 13))),
    "split_scatter_g3":   Case("conv", 3, 131, 256, 0, 4, 16, 16, 3, None, None, False,
                               [TAP_SCATTER, (GEMM[1], GEMM_RING_64)], ("split", 1, (256, 1048, 2))),
    "split_impl_g3":      Case("conv", 3, 131, 4, 32, 256, 16, 16, 3, (8, 0), None, False, [(IMPL[1], RING_IMPL)],
                               ("split", 2, (128, 1048, 2))),
}
# ---- short rows: the four MODEL rows of test_wgrad_short_rows.py, its four EXACT shapes single and G = 3
for _form, _G, _N, _chans, _S in ROWS_MODEL:
    ROUTE_CASES["rows_%s_%dx%d_g%d" % (_form, _S, _S, _G)] = short_rows(_form, _G, _N, _chans, _S)
for _name in sorted(ROWS_EXACT):
    for _G in (0, 3):
        _form, _S, _N, _chans = ROWS_EXACT[_name]
        ROUTE_CASES["rows_small_%s%s" % (_name, "_g3" if _G else "")] = short_rows(_form, _G, _N, _chans, _S)


def _gemm_case(G, M, Nc, F_, H, W, view, tile):
    return Case("gemm", G, F_, Nc, 0, M, H, W, 1, (Nc + 4, 4) if view else None, (M + 8, 0) if view else None, False,
                [(GEMM[1 if G else 0], tile)], None)


def _wgrad_case(G, N, C1, C2, Cout, H, W, ks, view, want):
    return Case("conv", G, N, C1, C2, Cout, H, W, ks, (2 * C1, 0) if view else None, None, False, want, None)


def _band_case(N, C1, C2, Cout, H, W, view):
    return Case("band", 0, N, C1, C2, Cout, H, W, 3, (2 * C1, 0) if view else None, (Cout + 8, 4) if view else None, False,
                [(BAND_ENTRY, "wgrad_band_kernel<1,5,1>" if Cout <= 32 else "wgrad_band_kernel<2,5,0>")], None)


EXACT_CASES = dict(ROUTE_CASES)
EXACT_CASES.update({"gemm_" + n: _gemm_case(*c) for n, c in GEMM_CASES.items()})
EXACT_CASES.update({"wgrad_" + n: _wgrad_case(*c) for n, c in WGRAD_CASES.items() if n != "f32_3x5"})
EXACT_CASES.update({"band_" + n: _band_case(*c) for n, c in BAND_CASES.items()})


def density(c):
    """the largest d of {1, 1/2, 1/4, 1/8} that keeps S.max() under 4096: |v| is 1 with probability 2 d / 3 (and within
    2^-9 of it), so S of K = N H W summed pixels concentrates at K (2 d / 3)^2 with a standard deviation of its square
    root; six of those above the mean is more than the maximum over the outputs of any case here"""
    K_ = c.N * c.H * c.W
    for d in (1.0, 0.5, 0.25, 0.125):
        mean = K_ * (2 * d / 3) ** 2
        if mean + 6 * mean ** 0.5 < 4096:
            return d
    raise AssertionError("no density for %d pixels" % K_)


# ------------------------------------------------------------------------------------------------ operands
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def two_piece(shape, gen, d):
    """(v, hi, lo) of the exact test's generator, q = 9"""
    hi = torch.randint(-1, 2, shape, generator=gen).float()
    lo = torch.randint(-1, 2, shape, generator=gen).float() * 2.0 ** -9
    lo = torch.where(hi == 0, torch.zeros(()), lo)
    keep = (torch.rand(shape, generator=gen) < d).float()
    return (hi + lo) * keep, hi * keep, lo * keep


def values_key(c, mode, i, seed=0):
    """what the values of group i depend on: cases that agree here share operand values and references"""
    scaled = mode == "randn" and i == max(c.G, 1) - 1
    return (mode, c.N, c.Cout, c.C1 + c.C2, c.C1 if scaled else 0, c.H, c.W, density(c) if mode == "exact" else 0, i, seed)


def draw(mode, shape, gen, d):
    return torch.randn(shape, generator=gen) if mode == "randn" else two_piece(shape, gen, d)[0]


def operands(c, mode, seed=0):
    """per group the dense values g [N, Cout, H, W] and x [N, C1 + C2, H, W] (x = cat(in1, in2)); randn: in1 of the last
    group times 3 plus 0.5, as run_wgrad_case"""
    gs, xs = [], []
    for i in range(max(c.G, 1)):
        key = values_key(c, mode, i, seed)
        gen = _gen(*key)
        g = draw(mode, (c.N, c.Cout, c.H, c.W), gen, key[7])
        x = draw(mode, (c.N, c.C1 + c.C2, c.H, c.W), gen, key[7])
        if key[4]:
            x[:, :c.C1] = x[:, :c.C1] * 3 + 0.5
        gs.append(g)
        xs.append(x)
    return gs, xs


_refs = {}
_ref_seconds = [0.0]   # wall time of the fp64 references so far (printed by the last test)


def cached(key, make):
    if key not in _refs:
        t0 = time.perf_counter()
        _refs[key] = make()
        _ref_seconds[0] += time.perf_counter() - t0
    return _refs[key]


def model_refs(c, mode, i, g, x, seed=0):
    """(three-product model, exact fp64, S, op(a_hi, b_hi) -- exact mode only) of group i, in fp64, computed once per set
    of values"""
    def make():
        op = wgrad_op(c.ks)
        gh, gl = split(g)
        xh, xl = split(x)
        if mode == "exact":
            hh = op(gh.double(), xh.double())
            ym = hh + op(gh.double(), xl.double()) + op(gl.double(), xh.double())
        else:   # (model64)
            hh, ym = None, op(gh.double(), xh.double() + xl.double()) + op(gl.double(), xh.double())
        return ym, op(g.double(), x.double()), op(g.double().abs(), x.double().abs()), hh
    return cached(values_key(c, mode, i, seed) + (c.ks,), make)


class Device:
    """the operands of a case on the device, in the layout the case asks for"""

    def __init__(self, c, name, mode, gs, xs):
        n, d = max(c.G, 1), density(c)
        fill = _gen("fill", name, mode)
        self.c, self.in2s = c, None
        if c.xview:
            Ctot, c0 = c.xview
            wide = [draw(mode, (c.N, Ctot, c.H, c.W), fill, d) for _ in range(n)]
            for w, x in zip(wide, xs):
                w[:, c0:c0 + c.C1] = x[:, :c.C1]
            self.in1s = [w.cuda()[:, c0:c0 + c.C1] for w in wide]
        else:
            self.in1s = [x[:, :c.C1].contiguous().cuda() for x in xs]
        if c.C2:
            self.in2s = [x[:, c.C1:].contiguous().cuda() for x in xs]
        if c.gview:
            Ctot, c0 = c.gview
            wide = [draw(mode, (c.N, Ctot, c.H, c.W), fill, d) for _ in range(n)]
            for w, g in zip(wide, gs):
                w[:, c0:c0 + c.Cout] = g
            self.gwide, self.gst = [w.cuda() for w in wide], None
        else:
            self.gwide, self.gst = None, torch.stack(gs).cuda()

    def gradients(self, scale=1.0):
        """(the groups' gradients, the stacked buffer they are slices of or None)"""
        if self.gwide is not None:
            c0 = self.c.gview[1]
            return [(w * scale)[:, c0:c0 + self.c.Cout] for w in self.gwide], None
        gst = self.gst * scale
        return [gst[i] for i in range(gst.shape[0])], gst


def run(K, c, dev, scale=1.0):
    """the case's weight gradients [Cout, C1 + C2, ks, ks] through the public function of its kind"""
    gl, gst = dev.gradients(scale)
    kw = dict(short_rows=True) if c.short else {}
    in2 = None if dev.in2s is None else dev.in2s[0]
    if c.kind == "gemm":
        out = K.gemm_wgrad_grouped(gl, dev.in1s, c.Cout, c.C1) if c.G else [K.gemm_wgrad(gl[0], dev.in1s[0], c.Cout, c.C1)]
    elif c.kind == "conv":
        out = (K.conv2d_wgrad_grouped(dev.in1s, dev.in2s, gl, c.Cout, c.ks, g_stacked=gst, **kw) if c.G else
               [K.conv2d_wgrad(dev.in1s[0], in2, gl[0], c.Cout, c.ks, **kw)])
    elif c.kind == "zeros":
        out = (K.zeros_conv_wgrad_grouped(dev.in1s, gl, c.Cout, g_stacked=gst, **kw) if c.G else
               [K.zeros_conv_wgrad(dev.in1s[0], gl[0], c.Cout, 3, **kw)])
    else:
        out = [band(K, dev.in1s[0], in2, gl[0], c.Cout)]
    assert len(out) == max(c.G, 1)
    return [t.detach().cpu().double().reshape(c.Cout, c.C1 + c.C2, c.ks, c.ks) for t in out]


def yardstick(K, c, dev, i):
    """the fp32-MFMA weight gradient (rfn_conv2d_wgrad_f32) of group i on the same device operands"""
    gl, _ = dev.gradients()
    gf = wgrad_f32(K, dev.in1s[i], None if dev.in2s is None else dev.in2s[i], gl[i], c.Cout, c.ks)
    return gf.detach().cpu().double().reshape(c.Cout, c.C1 + c.C2, c.ks, c.ks)


def assert_ring(c):
    if c.ring is not None:
        query, arg, expected = c.ring
        if query == "split":
            assert _split(c.G, c.N * c.H * c.W, arg) == expected
        else:
            assert _crossings(c.G, c.N * c.H * c.W // 32, arg) == expected


# ------------------------------------------------------------------------------------------------ 1. model bounds
def run_route_case(K, launches, name, seed=0):
    c = ROUTE_CASES[name]
    assert_ring(c)
    gs, xs = operands(c, "randn", seed)
    dev = Device(c, name, "randn", gs, xs)
    n0 = len(launches)
    got = run(K, c, dev)
    assert launches[n0:] == c.want, (name, launches[n0:])
    got40 = run(K, c, dev, 2.0 ** -40)
    figs = []
    for i in range(max(c.G, 1)):
        gm, g64, s, _ = model_refs(c, "randn", i, gs[i], xs[i], seed)
        figs.append({"model": e_abs(got[i], gm, s), "fp64": e_abs(got[i], g64, s),
                     "f32": e_abs(yardstick(K, c, dev, i), g64, s),
                     "model_k-40": e_abs(got40[i], gm * 2.0 ** -40, s * 2.0 ** -40)})
    return merge(figs)


def check_route(name, fig):
    """check_wgrad; the short-row family with ROWS_CAP in the place of WGRAD_CAP, every other bound as it is"""
    if not ROUTE_CASES[name].short:
        return check_wgrad(name, fig)
    check(name, fig, cap=ROWS_CAP)
    msg = "%s: e_abs vs model at gradient * 2^-40: %.3g" % (name, fig["model_k-40"])
    print(msg)
    assert fig["model_k-40"] <= min(3 * fig["f32"] + 2e-8, ROWS_CAP), msg


@pytest.mark.parametrize("name", list(ROUTE_CASES))
def test_route_vs_model(K, launches, name):
    check_route(name, run_route_case(K, launches, name))


# ------------------------------------------------------------------------------------------------ 2. exact
def exact_refs(c, name, i, g, x):
    """(model, S) of group i of the two-piece operands, after the CPU assertions that make equality the right demand"""
    d = density(c)
    gen = _gen(*values_key(c, "exact", i))
    for v in (g, x):   # the generator again, for its pieces: split() must return exactly them
        vv, hi, lo = two_piece(tuple(v.shape), gen, d)
        assert torch.equal(vv, v)
        sh, sl = split(v)
        assert torch.equal(sh, hi) and torch.equal(sl, lo), (name, i, "split(v) is not (hi, lo)")
        assert bool((lo != 0).any()), (name, i, "lo is all zero")
    ym, full, s, hh = model_refs(c, "exact", i, g, x)
    smax = float(s.max())
    print("%s group %d: d = %g, S.max() = %g" % (name, i, d, smax))
    assert smax * 2.0 ** 9 < 2.0 ** 22, (name, i, smax)
    assert torch.equal((ym * 2.0 ** 9).round(), ym * 2.0 ** 9) and torch.equal(ym.float().double(), ym), (name, i)
    assert not torch.equal(ym, full), (name, i, "the model equals op(a, b): no lo lo term to tell them apart")
    assert not torch.equal(ym, hh), (name, i, "the model equals op(a_hi, b_hi): the lo plane is not live")
    return ym, s


@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_exact_on_two_piece_operands(K, launches, name):
    c = EXACT_CASES[name]
    gs, xs = operands(c, "exact")
    refs = [exact_refs(c, name, i, gs[i], xs[i]) for i in range(max(c.G, 1))]
    dev = Device(c, name, "exact", gs, xs)
    n0 = len(launches)
    got = run(K, c, dev)
    assert launches[n0:] == c.want, (name, launches[n0:])
    bad = []
    for i, (ym, s) in enumerate(refs):
        diff = (got[i] - ym).abs()
        if not torch.equal(got[i], ym):
            bad.append("group %d: %d of %d outputs differ, by at most %g x 2^-9 (e_abs %.3g)" % (
                i, int((diff != 0).sum()), diff.numel(), float(diff.max()) * 2.0 ** 9, float((diff / s.clamp_min(1.0)).max())))
    print("%s: %s" % (name, "; ".join(bad) if bad else "equal to the model in all %d groups" % len(refs)))
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------ 3. the label set
B3, DMA, DMA_IMPL = "gemm_wgrad_b3_kernel<%s>", "gemm_wgrad_dma_kernel<%s>", "gemm_wgrad_dma_impl_kernel<%s>"
# kWgradB3Labels of csrc/wgrad_bf16x3.hip, in its order
WGRAD_B3_LABELS = [DMA % "2,4,4,2,32,2", DMA % "1,8,2,1,32,3", B3 % "4,2,2,3,64", B3 % "2,4,4,2,64", B3 % "1,4,2,2,32",
                   B3 % "4,1,2,2,32", B3 % "2,2,2,2,64", DMA_IMPL % "4,2,2,3", B3 % "4,2,2,3,64,1", B3 % "1,4,1,2,32,1",
                   B3 % "2,2,2,2,64,1", DMA_IMPL % "4,2,2,1", DMA_IMPL % "4,2,2,2", B3 % "2,2,2,2,64,2", B3 % "2,2,2,2,64,3"]
# every label single and grouped -- but a group never takes the 32-row implicit tiling (choose_wgrad_implicit) -- and the
# two instantiations of the band kernel (kWgradBandLabels), which has no grouped form
ALL_LABELS = (set(WGRAD_B3_LABELS) | {grouped(l) for l in WGRAD_B3_LABELS if l != B3 % "1,4,1,2,32,1"} |
              {"wgrad_band_kernel<1,5,1>", "wgrad_band_kernel<2,5,0>"})


def test_cases_cover_every_label():
    """the labels asserted launch by launch in this module are all a split-precision weight gradient can carry"""
    seen = {label for c in EXACT_CASES.values() for _, label in c.want if "wgrad" in label}
    assert seen == ALL_LABELS, (sorted(seen - ALL_LABELS), sorted(ALL_LABELS - seen))
    assert set(ROUTE_CASES) <= set(EXACT_CASES)
    print("fp64 references: %d sets of values, %.1f s" % (len(_refs), _ref_seconds[0]))
