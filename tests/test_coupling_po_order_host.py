"""K order of the fused coupling kernels' first 3x3 product (csrc/coupling_po.hip), without a device.

rfn_coupling_po_k_order answers from the constexpr description (po_order / po_unit) that the pack kernel and the kernel
read: a unit is 8 K-values (one lane half of a k-step), k-step s multiplies units 2s and 2s + 1.  Full units are
(tap, 8-channel group) over the 9 real taps; where a narrow leftover is instantiated the Cin % 8 leftover channels form
units of 8 / r' taps x r' channels.  The counts below are the table of DESIGN section 4: units, k-steps per quad, and the
k-steps of the former order (5 tap pairs x ceil(Cin / 8) groups) they replace.
"""
import ctypes

import pytest

# (Cin, bwd) -> units, k-steps per quad (dense), k-steps of the former tap-pair order
TABLE = {
    (18, 0): (21, 11, 15), (36, 0): (41, 21, 25), (72, 0): (81, 41, 45),
    (4, 1): (5, 3, 5), (8, 1): (9, 5, 5), (16, 1): (18, 9, 10),
}
# every instantiation the launchers hold, by a shape that reaches it: (Cin, C, W, bwd)
INSTANCES = [
    (18, 4, 32, 0), (20, 4, 32, 0), (36, 8, 16, 0), (40, 8, 16, 0), (72, 16, 8, 0), (70, 12, 32, 0), (72, 12, 32, 0),
    (4, 4, 32, 1), (8, 8, 32, 1), (4, 4, 16, 1), (8, 8, 16, 1), (16, 16, 8, 1), (12, 12, 8, 1), (12, 12, 32, 1),
    (16, 16, 32, 1),
]
LDS_CAP = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from rfn_hip import lib as L_
    return L_.load()


def units_of(lib, Cin, bwd):
    n = lib.rfn_coupling_po_k_order(Cin, bwd, -1, None, None, None, None)
    out = []
    for u in range(n):
        v = [ctypes.c_longlong() for _ in range(4)]
        ks = lib.rfn_coupling_po_k_order(Cin, bwd, u, *[ctypes.byref(x) for x in v])
        assert ks == u // 2
        out.append(tuple(x.value for x in v))
    return out


@pytest.mark.parametrize("Cin,bwd", sorted(TABLE) + [(70, 0), (12, 1), (20, 0), (17, 0), (35, 0), (2, 1)])
def test_every_tap_channel_pair_in_exactly_one_slot(lib, Cin, bwd):
    seen = {}
    for u, (tap0, n_taps, ch0, n_ch) in enumerate(units_of(lib, Cin, bwd)):
        assert n_taps >= 1 and n_ch >= 1 and n_taps * n_ch <= 8
        assert 0 <= tap0 and tap0 + n_taps <= 9, "a slot names a tap > 8"
        assert 0 <= ch0 and ch0 + n_ch <= Cin, "a slot names a channel >= Cin"
        for t in range(tap0, tap0 + n_taps):
            for c in range(ch0, ch0 + n_ch):
                assert (t, c) not in seen, ("pair in two units", (t, c), seen[(t, c)], u)
                seen[(t, c)] = u
    assert set(seen) == {(t, c) for t in range(9) for c in range(Cin)}


@pytest.mark.parametrize("Cin,bwd", sorted(TABLE))
def test_unit_and_kstep_counts_of_the_table(lib, Cin, bwd):
    n_units, ns1, former = TABLE[(Cin, bwd)]
    assert former == 5 * ((Cin + 7) // 8)
    assert len(units_of(lib, Cin, bwd)) == n_units
    assert (n_units + 1) // 2 == ns1 <= former
    # the stream says the same: per quad 8 fragments per conv1 k-step and 128 of conv2
    C = Cin if bwd else {18: 4, 36: 8, 72: 16}[Cin]
    ngrp = lib.rfn_coupling_po_ring_group(Cin, C, bwd, -1, None, None)
    first, count = ctypes.c_longlong(), ctypes.c_longlong()
    total, nxt, conv1 = 0, 1, 0
    for i in range(ngrp):
        assert lib.rfn_coupling_po_ring_group(Cin, C, bwd, i, ctypes.byref(first), ctypes.byref(count)) == 0
        assert first.value == nxt, "ring groups are consecutive in the stream"
        assert count.value > 0 and count.value % 4 == 0, "the four waves issue the same number of DMA pieces"
        nxt += count.value
        total += count.value
    NP = 0 if bwd else (9 * C + 31) // 32
    assert total == 2 * (8 * ns1 + 128) + 32 * NP
    packed = lib.rfn_coupling_po_bwd_packed_bytes(C) if bwd else lib.rfn_coupling_po_packed_bytes(Cin, C)
    assert packed == 1024 * (1 + total)


@pytest.mark.parametrize("Cin,C,W,bwd", INSTANCES)
def test_lds_of_every_instantiation_fits(lib, Cin, C, W, bwd):
    assert (lib.rfn_coupling_po_bwd_supported(2 * 128, C, W, W) if bwd
            else lib.rfn_coupling_po_supported(2 * 128, C, Cin - C // 2, 256, W, W)), "not a shape of the fused kernels"
    b = lib.rfn_coupling_po_lds_bytes(Cin, C, W, bwd)
    assert 0 < b <= LDS_CAP
    # ring groups fit the slot the LDS figure is made of: 3 slots + 4160 bytes + image (+ backward sums)
    ngrp = lib.rfn_coupling_po_ring_group(Cin, C, bwd, -1, None, None)
    first, count = ctypes.c_longlong(), ctypes.c_longlong()
    biggest = 0
    for i in range(ngrp):
        lib.rfn_coupling_po_ring_group(Cin, C, bwd, i, ctypes.byref(first), ctypes.byref(count))
        biggest = max(biggest, count.value)
    ipos = (128 // W + 2) * (W + 2) if W * W >= 128 else (128 // (W * W)) * (W + 2) ** 2
    assert b == 3 * 1024 * max(biggest, 32) + 4096 + 64 + 2 * ((Cin + 7) // 8) * ipos * 16 + (8192 if bwd else 0)


def test_bad_arguments_are_refused(lib):
    v = [ctypes.c_longlong() for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    assert lib.rfn_coupling_po_k_order(0, 0, -1, *refs) < 0
    assert lib.rfn_coupling_po_k_order(18, 0, 21, *refs) < 0
    assert lib.rfn_coupling_po_k_order(18, 0, 0, None, None, None, None) < 0
