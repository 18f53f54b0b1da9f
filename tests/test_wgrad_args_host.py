"""CPU-only: the argument checks of the six split-precision weight-gradient entry points, through the C ABI.  No device
and no launch: every call here is refused by a check, or has F = 0 frames and returns 0 before the kernel choice.  The
operand addresses are made up (16-byte aligned, non-null) and never dereferenced; the grouped forms read the host arrays
of G such addresses, nothing behind them.

Codes: -1 null operand / size <= 0 / G outside 1..16, -2 a pixel count or stride the 16-byte loads cannot take, -3 a
misaligned operand (grouped: a misaligned or null entry of a group), -4 F*H*W too large for the 32-bit pixel index."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))

A, B, B2, GW = 0x7F0000010000, 0x7F0000020000, 0x7F0000030000, 0x7F0000040000
G_OK = 3
TOO_MANY = (1 << 31) - 4096          # F * H * W must stay below this


def _arr(base, G=G_OK, last=None):
    """host array of G made-up addresses base, base + 4096, ...; `last` replaces the entry of the last group"""
    v = [base + 4096 * i for i in range(G)]
    if last is not None:
        v[-1] = last
    return (ctypes.c_void_p * G)(*v)


# Per entry point: the valid call as a dict (in the C argument order, without the stream) and the names of its operands.
def _gemm(grouped):
    d = dict(a=_arr(A) if grouped else A, a_ns=64 * 16, M=64, b=_arr(B) if grouped else B, b_ns=32 * 16, Nc=32,
             gw=_arr(GW) if grouped else GW)
    if grouped:
        d["G"] = G_OK
    d.update(F=2, HW=16)
    return d


def _implicit(grouped):
    d = dict(g=_arr(A) if grouped else A, g_ns=64 * 64, Cout=64, in1=_arr(B) if grouped else B, in1_ns=8 * 64, C1=4,
             in2=_arr(B2) if grouped else B2, in2_ns=4 * 64, C2=4, gw=_arr(GW) if grouped else GW)
    if grouped:
        d["G"] = G_OK
    d.update(F=2, H=8, W=8)
    return d


def _mirrored(grouped):
    d = dict(h=_arr(A) if grouped else A, h_ns=64 * 64, Cin=64, g=_arr(B) if grouped else B, g_ns=4 * 64, C=4,
             gwT=_arr(GW) if grouped else GW)
    if grouped:
        d["G"] = G_OK
    d.update(F=2, H=8, W=8)
    return d


# name -> (valid arguments, operands, their strides, the row counts that must be positive)
FORMS = {
    "rfn_gemm_wgrad_bf16x3": (_gemm, ("a", "b", "gw"), ("a_ns", "b_ns"), ("M", "Nc")),
    "rfn_conv3x3_wgrad_implicit_bf16x3": (_implicit, ("g", "in1", "in2", "gw"), ("g_ns", "in1_ns", "in2_ns"),
                                          ("Cout", "C1")),
    "rfn_conv3x3_wgrad_mirrored_bf16x3": (_mirrored, ("h", "g", "gwT"), ("h_ns", "g_ns"), ("Cin", "C")),
}
ENTRY_POINTS = [(n, False) for n in FORMS] + [(n.replace("_bf16x3", "_grouped_bf16x3"), True) for n in FORMS]
INPUTS = {"a", "b", "g", "in1", "in2", "h"}   # operands read with 16-byte loads (the outputs take float atomics)


def _call(L, name, args):
    return getattr(L, name)(*args.values(), None)


def _cases(name, grouped):
    """(what, arguments, expected code): each violates exactly one condition of the valid call"""
    make, operands, strides, counts = FORMS[name.replace("_grouped", "")]
    out = []

    def case(what, code, **changed):
        d = make(grouped)
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
    if "HW" in make(grouped):
        case("HW % 4 != 0", -2, HW=18)
    else:
        case("W % 8 != 0", -2, W=12)
        case("W % 8 != 0 (HW % 32 == 0)", -2, H=8, W=4)
    for s in strides:
        case(s + " % 4 != 0", -2, **{s: make(grouped)[s] + 2})
    for o in operands:
        if o not in INPUTS:
            continue
        base = {"a": A, "g": A if "Cout" in make(grouped) else B, "h": A, "b": B, "in1": B, "in2": B2}[o]
        if grouped:
            case("misaligned %s of the last group" % o, -3, **{o: _arr(base, last=base + 4096 * (G_OK - 1) + 4)})
            case("null %s of the last group" % o, -3, **{o: _arr(base, last=0)})
        else:
            case("misaligned " + o, -3, **{o: base + 8})
    if grouped:
        for o in operands:
            if o not in INPUTS:
                case("null %s of the last group" % o, -3, **{o: _arr(GW, last=0)})
    # F * H * W = 2^31 - 4096 exactly: the first count that is refused
    if "HW" in make(grouped):
        case("F * HW too large", -4, F=TOO_MANY // 4096, HW=4096)
    else:
        case("F * H * W too large", -4, F=TOO_MANY // 4096, H=64, W=64)
    return out


@pytest.mark.parametrize("name,grouped", ENTRY_POINTS)
def test_each_violation_returns_its_code(name, grouped):
    from rfn_hip import lib
    L = lib.load()
    cases = _cases(name, grouped)
    assert len(cases) >= 12
    for what, args, code in cases:
        assert _call(L, name, args) == code, (name, what)
        assert L.rfn_last_error(), (name, what)


@pytest.mark.parametrize("name,grouped", ENTRY_POINTS)
def test_no_frames_returns_zero(name, grouped):
    """F = 0 with otherwise valid arguments: 0, nothing launched -- also when H * W alone is large"""
    from rfn_hip import lib
    L = lib.load()
    make = FORMS[name.replace("_grouped", "")][0]
    d = make(grouped)
    d["F"] = 0
    assert _call(L, name, d) == 0, name
    if "HW" in d:
        d["HW"] = 1 << 20
    else:
        d["H"], d["W"] = 1024, 1024
    assert _call(L, name, d) == 0, name


def test_implicit_forms_ignore_the_second_source_without_channels():
    """C2 = 0: in2 and its stride are not looked at (null, odd stride)"""
    from rfn_hip import lib
    L = lib.load()
    for grouped in (False, True):
        d = _implicit(grouped)
        d.update(F=0, C2=0, in2=None, in2_ns=3)
        name = "rfn_conv3x3_wgrad_implicit_%sbf16x3" % ("grouped_" if grouped else "")
        assert _call(L, name, d) == 0, name
