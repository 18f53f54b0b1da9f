"""rfn_conv3x3_smallcout_bf16x3 (csrc/dgrad_small.hip) with the three x-taps stacked as MFMA rows and the x-shift done
on the accumulators: against torch's conv_transpose2d in fp64 on the CPU and against the generic bf16x3 kernel, on
32x32 / 16x16 / 8x8 maps, odd and tiny frame counts (frames per block), every accumulate / split combination, and
inputs whose only contribution falls off the end of an image row (the shift must not leak into the neighbouring row,
frame or lane half).  The host-side truth table of rfn_dgrad_small_supported needs no device."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

# (N, Cin, Cout, W) of the issue: canonical levels 0-2 at odd / tiny / large frame counts, ragged channel counts
SHAPES = [(70, 256, 72, 8), (609, 256, 72, 8), (1, 256, 36, 16), (3, 256, 36, 16), (77, 256, 18, 32), (2, 64, 50, 32),
          (5, 32, 7, 16), (3, 32, 7, 8), (2, 64, 96, 8),
          # the instantiations with two row groups that the list above does not reach: 32x32 with 3-4 stacked row tiles
          # (8-row bands) and 16x16 with 5-6
          (3, 64, 32, 32), (3, 64, 64, 16)]
HALF = {18: 2, 36: 4, 72: 8, 50: 6, 7: 3, 96: 32, 32: 4, 64: 8}  # C/2 of the flow level (or any split) per Cout


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    if not ops.bwd_b3():
        pytest.skip("bf16x3 backward arithmetic only")
    return ops


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def run_case(K, N, Cin, Cout, S, split, acc1, acc2, seed=0):
    g = torch.Generator().manual_seed(1000 * S + Cout + seed)
    Nc = min(N, 8)  # the CPU reference covers the first frames and, for large N, the last ones
    x = torch.randn(N, Cin, S, S, generator=g)
    w = torch.randn(Cin, Cout, 3, 3, generator=g) * 0.05   # FORWARD weight of a conv Cout -> Cin
    base1 = torch.randn(N, split, S, S, generator=g)
    base2 = torch.randn(N, Cout - split, S, S, generator=g) if Cout > split else None
    out1 = base1.clone().cuda()
    out2 = base2.clone().cuda() if base2 is not None else None
    wpk = K.pack_weight(w.cuda(), flip=True)
    K.conv3x3_smallcout(x.cuda(), wpk, Cout, out1, out2, split, acc1, acc2)
    for sl in (slice(0, Nc), slice(N - Nc, N)):
        r = F.conv_transpose2d(x[sl].double(), w.double(), padding=1)  # = data gradient of conv2d(., w, padding=1)
        r1 = r[:, :split] + (base1[sl].double() if acc1 else 0)
        e1 = float((out1[sl].cpu().double() - r1).abs().max())
        print("N%d %d->%d %dx%d split %d acc %d%d: out1 err %.3g of %.3g" % (N, Cin, Cout, S, S, split, acc1, acc2, e1,
                                                                              float(r1.abs().max())))
        assert e1 < 5e-5 * float(r1.abs().max()) + 1e-6
        if base2 is not None:
            r2 = r[:, split:] + (base2[sl].double() if acc2 else 0)
            e2 = float((out2[sl].cpu().double() - r2).abs().max())
            print("    out2 err %.3g of %.3g" % (e2, float(r2.abs().max())))
            assert e2 < 5e-5 * float(r2.abs().max()) + 1e-6
    # and the generic kernel agrees (same arithmetic, different summation order)
    g1 = base1.clone().cuda()
    g2 = base2.clone().cuda() if base2 is not None else None
    K.conv2d_raw(x.cuda(), None, wpk, Cout, 3, 0, None, None, 0, out1=g1, out2=g2, cout_split=split, acc1=acc1,
                 acc2=acc2)
    assert relerr(out1, g1) < 2e-5
    if g2 is not None:
        assert relerr(out2, g2) < 2e-5


@gpu
@pytest.mark.parametrize("N,Cin,Cout,S", SHAPES)
def test_rows_kernel_shapes(K, N, Cin, Cout, S):
    """every shape of the list, split at C/2, the level's own accumulate pattern (gz accumulates, gcond is written)"""
    run_case(K, N, Cin, Cout, S, HALF[Cout], True, False)


@gpu
@pytest.mark.parametrize("acc1", [False, True])
@pytest.mark.parametrize("acc2", [False, True])
@pytest.mark.parametrize("Cout,S", [(18, 32), (36, 16), (72, 8)])
def test_rows_kernel_accumulate_combinations(K, Cout, S, acc1, acc2):
    run_case(K, 5, 256, Cout, S, HALF[Cout], acc1, acc2, seed=1)


@gpu
@pytest.mark.parametrize("Cout,S,split", [(18, 32, 18), (36, 16, 36), (72, 8, 72), (18, 32, 17), (72, 8, 71)])
def test_rows_kernel_splits(K, Cout, S, split):
    """one output tensor (cout_split = Cout, no out2) and a split that is not a multiple of 4"""
    run_case(K, 3, 256, Cout, S, split, split != Cout, True, seed=2)


@gpu
@pytest.mark.parametrize("S,Cout,N", [(32, 18, 3), (16, 36, 3), (8, 72, 3), (8, 72, 513)])  # 513: two 8x8 frames per block
@pytest.mark.parametrize("side", ["right", "left"])
def test_rows_kernel_edge_exactness(K, S, Cout, N, side):
    """input only in the last (first) column and forward weights only at the x-tap that carries it out of the row: the
    output is EXACTLY zero (a shift leaking into the next image row, the next frame of the tile or the other lane half
    would be a non-zero).  Mirror: the same tap from the column next to it lands on column W-1 (0) and nowhere else."""
    Cin, split = 64, HALF[Cout]
    g = torch.Generator().manual_seed(S + (side == "left"))
    kx = 2 if side == "right" else 0   # conv_transpose2d: in[.., x] * w[.., kx] lands on x + kx - 1
    w = torch.zeros(Cin, Cout, 3, 3)
    w[:, :, :, kx] = torch.randn(Cin, Cout, 3, generator=g) * 0.05
    wpk = K.pack_weight(w.cuda(), flip=True)
    for col, land in ((S - 1, None), (S - 2, S - 1)) if side == "right" else ((0, None), (1, 0)):
        x = torch.zeros(N, Cin, S, S)
        x[:, :, :, col] = torch.randn(N, Cin, S, generator=g)
        out1 = torch.full((N, split, S, S), 7.0, device="cuda")
        out2 = torch.full((N, Cout - split, S, S), 7.0, device="cuda")
        K.conv3x3_smallcout(x.cuda(), wpk, Cout, out1, out2, split, False, False)
        out = torch.cat([out1, out2], 1).cpu()
        if land is None:
            assert int((out != 0).sum()) == 0, "a contribution beyond the row end leaked: %d non-zeros" % int((out != 0).sum())
        else:
            ref = F.conv_transpose2d(x.double(), w.double(), padding=1)
            err = float((out.double() - ref).abs().max())
            print("edge %s S%d: err %.3g of %.3g" % (side, S, err, float(ref.abs().max())))
            assert err < 5e-5 * float(ref.abs().max()) + 1e-6
            keep = torch.ones(S, dtype=torch.bool)
            keep[land] = False
            assert int((out[:, :, :, keep] != 0).sum()) == 0
            assert float(out[:, :, :, land].abs().max()) > 0


def test_dgrad_small_supported_truth_table():
    from rfn_hip import lib
    L = lib.load()
    ok = lambda N, Cin, Cout, H, W: bool(L.rfn_dgrad_small_supported(N, Cin, Cout, H, W))
    for (N, Cin, Cout, S) in SHAPES + [(608, 256, 18, 32), (608, 256, 36, 16), (608, 256, 72, 8), (76, 256, 72, 8),
                                       (2, 64, 64, 32), (2, 64, 64, 16), (4095, 256, 18, 32)]:
        assert ok(N, Cin, Cout, S, S), (N, Cin, Cout, S)
    assert not ok(8, 256, 18, 4, 4)            # W = 4
    assert not ok(8, 256, 18, 64, 64)          # W = 64
    assert not ok(8, 48, 18, 32, 32)           # Cin % 32 != 0
    assert not ok(8, 16, 18, 16, 16)
    assert not ok(8, 256, 97, 8, 8)            # Cout > 96
    assert not ok(8, 256, 128, 16, 16)
    assert not ok(8, 256, 18, 16, 32)          # H != W
    assert not ok(8, 256, 18, 32, 16)
    assert not ok(4096, 256, 18, 32, 32)       # 2^32 bytes of input: beyond the 32-bit buffer range
    assert not ok(0, 256, 18, 32, 32)
