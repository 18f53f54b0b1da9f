"""Launch routes, size limits and argument checks of the Glow shell entry points, without a device.

rfn_glow_shell_fwd_kernel_label / rfn_glow_shell_bwd_kernel_label print the host structs the launchers themselves read
(choose_shell_fwd / choose_shell_bwd in csrc/glow_shell.hip).  The tables below say, from a reading of the kernels, which
branch each shape of tests/test_glow_shell.py takes; this module holds the library to them on any machine, and
test_glow_shell.py runs the same rows on the GPU.  The log-det class is decided on the device, block by block: here the
kernel's three tests are restated per block (ld_classes) and must give the class the label prints.
"""
import ctypes

import pytest
import torch

# (N, C, H, W) -> PB, log-det class, product class of a launch with a head, frames per block of the pow2 path (F)
FWD_CASES = {
    (64, 4, 32, 32): dict(PB=256, ld="frame", prod="global"),          # level-0 training route (B*T = 640 at 1/10)
    (640, 16, 8, 8): dict(PB=128, ld="pow2x64", prod="lds4", F=2),     # level-2 training route
    (1024, 4, 8, 8): dict(PB=256, ld="pow2x64", prod="global", F=4),
    (512, 4, 8, 16): dict(PB=256, ld="pow2x64", prod="global", F=2),   # HW = 128: two 64-lane groups per frame
    (600, 4, 4, 8): dict(PB=64, ld="pow2x32", prod="global", F=2),     # the __shfl_xor step
    (9, 8, 2, 4): dict(PB=32, ld="pow2x8", prod="global", F=4),
    (4, 32, 4, 4): dict(PB=32, ld="pow2x16", prod="lds4", F=2),
    (6, 64, 2, 2): dict(PB=32, ld="pow2x4", prod="lds4", F=8),
    (5, 16, 8, 8): dict(PB=32, ld="frame", prod="lds2"),
    (3, 48, 2, 2): dict(PB=32, ld="pow2x4", prod="lds2", F=8),
    (3, 24, 4, 4): dict(PB=32, ld="pow2x16", prod="global", F=2),      # C >= 16 but 3 outputs per thread
    (3, 6, 6, 6): dict(PB=32, ld="frame+generic", prod="global"),
    (3, 12, 12, 12): dict(PB=32, ld="frame+generic", prod="global"),
    (7, 4, 3, 5): dict(PB=32, ld="generic", prod="global", slots=4),
    (70, 2, 1, 1): dict(PB=32, ld="generic", prod="global", slots=33),
    (37, 2, 1, 2): dict(PB=32, ld="generic", prod="global", slots=17),
    (2, 176, 2, 2): dict(PB=32, ld="pow2x4", prod="lds2", F=8, lds=146432),
    (2, 186, 2, 2): dict(PB=32, ld="pow2x4", prod="global", F=8, lds=162192),   # the forward limit
}
# (N, C, HW) -> kernel ("small4", "small8", "big"), PB, grid, ny, gW class, sweeps; lds = bytes of the TAIL form
BWD_CASES = {
    (80, 4, 1024): dict(kernel="small4", grid=256, sweeps=2),          # 320 tiles on 256 blocks: uneven
    (300, 8, 225): dict(kernel="small8", grid=256, sweeps=2),          # frames not aligned to blocks
    (160, 12, 1024): dict(kernel="big", PB=256, grid=512, ny=1, gW="split", sweeps=2),   # 640 tiles on 512 blocks
    (640, 16, 64): dict(kernel="big", PB=256, grid=160, ny=2, gW="split", sweeps=1),     # training route
    (640, 32, 16): dict(kernel="big", PB=128, grid=80, ny=4, gW="owned", sweeps=1),
    (640, 64, 4): dict(kernel="big", PB=64, grid=40, ny=8, gW="owned", sweeps=1),
    (3, 6, 16): dict(kernel="big", PB=256, grid=1, ny=3, gW="split", sweeps=1),          # 7 pixel groups per entry
    (7, 10, 15): dict(kernel="big", PB=256, grid=1, ny=5, gW="split", sweeps=1),         # ragged single tile
    (4, 96, 16): dict(kernel="big", PB=64, grid=1, ny=8, gW="owned", sweeps=1, lds=88704),
    (2, 144, 4): dict(kernel="big", PB=64, grid=1, ny=8, gW="owned", sweeps=1, lds=160704),  # the tail limit
    (3, 4, 100): dict(kernel="small4", grid=2, sweeps=1),              # the small kernels' single, ragged sweep
    (5, 8, 64): dict(kernel="small8", grid=2, sweeps=1),
}
LDS_CAP = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from rfn_hip import lib as L_
    L_.load()
    return L_


def fields(label):
    """'name k=v k=v ...' -> (name, {k: v}) with integers where they parse"""
    name, *kv = label.split(" ")
    out = {}
    for item in kv:
        k, v = item.split("=")
        out[k] = int(v) if v.isdigit() else v
    return name, out


def fwd_label(lib, N, C, H, W, head=1):
    return lib.load().rfn_glow_shell_fwd_kernel_label(N, C, H, W, head).decode()


def bwd_label(lib, N, C, HW, tail):
    return lib.load().rfn_glow_shell_bwd_kernel_label(N, C, HW, tail).decode()


def ld_classes(N, HW, PB):
    """the log-det branch of every block, by the kernel's own three tests (glow_shell_fwd_kernel)"""
    out = set()
    for b in range((N * HW + PB - 1) // PB):
        n0 = (b * PB) // HW
        if n0 * HW <= b * PB and b * PB + PB <= (n0 + 1) * HW:
            out.add("frame")
        elif HW & (HW - 1) == 0 and 4 <= HW < PB:
            out.add("pow2x%d" % min(HW, 64))
        else:
            out.add("generic")
    return out


def prod_class(C, PB):
    """the form of the head's C x C product, by the kernel's own tests"""
    NG = 256 // PB
    if C >= 16 and C % NG == 0 and (C // NG) % 2 == 0:
        return "lds4" if (C // NG) % 4 == 0 and C % 4 == 0 else "lds2"
    return "global"


@pytest.mark.parametrize("case", list(FWD_CASES), ids=lambda c: "x".join(map(str, c)))
def test_forward_route_is_the_table_row(lib, case):
    N, C, H, W = case
    HW, want = H * W, FWD_CASES[case]
    name, f = fields(fwd_label(lib, N, C, H, W))
    assert name == "glow_shell_fwd_kernel"
    assert (f["PB"], f["ld"], f["prod"]) == (want["PB"], want["ld"], want["prod"]), f
    blocks = (N * HW + f["PB"] - 1) // f["PB"]
    assert f["blocks"] == blocks and f["slots"] == (f["PB"] - 1) // HW + 2
    assert f["slots"] == want.get("slots", want["F"] + 1 if "F" in want else 2)
    assert f["lds"] == want.get("lds", C * f["PB"] * 4 + (C * C * 4 if C >= 16 else 0)) <= LDS_CAP
    assert lib.load().rfn_glow_shell_fwd_ld_floats(N, C, H, W) == blocks * f["slots"]
    # the device-side decisions, restated block by block
    assert "+".join(sorted(ld_classes(N, HW, f["PB"]))) == f["ld"]
    assert prod_class(C, f["PB"]) == f["prod"]
    if "F" in want:
        assert f["PB"] // HW == want["F"]
    # a launch without a head has the same geometry (its partials share the reduce) and no product
    _, t = fields(fwd_label(lib, N, C, H, W, head=0))
    assert t == dict(f, lds=0, prod="none")


@pytest.mark.parametrize("case", list(BWD_CASES), ids=lambda c: "x".join(map(str, c)))
def test_backward_route_is_the_table_row(lib, case):
    N, C, HW = case
    want = BWD_CASES[case]
    for tail in (1, 0):
        name, f = fields(bwd_label(lib, N, C, HW, tail))
        if want["kernel"] != "big":
            Cs = int(want["kernel"][5:])
            assert name == "actnorm_invconv_bwd_small_kernel<%d,%d>" % (Cs, tail)
            assert f == dict(grid=want["grid"], sweeps=want["sweeps"], lds=(Cs * Cs + 5 * Cs) * 4)
            tiles = (N * HW + 255) // 256
            assert f["grid"] == min(tiles, 256) and f["sweeps"] == -(-tiles // f["grid"])
            continue
        assert name == "actnorm_invconv_bwd_kernel<%d>" % tail
        lds = (2 * C * (want["PB"] + 1) + C * C + 2 * C + (3 * C if tail else 0)) * 4
        assert f == dict(PB=want["PB"], grid=want["grid"], ny=want["ny"], gW=want["gW"], sweeps=want["sweeps"], lds=lds)
        if tail and "lds" in want:
            assert lds == want["lds"]
        tiles = (N * HW + f["PB"] - 1) // f["PB"]
        assert f["grid"] == min(tiles, 512) and f["sweeps"] == -(-tiles // f["grid"])
        assert f["gW"] == ("split" if C * C <= 256 else "owned") and f["grid"] * f["ny"] <= 512 and lds <= LDS_CAP


def test_tables_reach_every_route(lib):
    fw = [fields(fwd_label(lib, *c))[1] for c in FWD_CASES]
    assert {f["ld"] for f in fw} == {"frame", "generic", "frame+generic"} | {"pow2x%d" % g for g in (4, 8, 16, 32, 64)}
    assert {f["prod"] for f in fw} == {"global", "lds2", "lds4"}
    assert {f["PB"] for f in fw} == {32, 64, 128, 256}
    assert any(f["lds"] > 65536 for f in fw)
    assert {f["PB"] for f in fw if f["ld"].startswith("pow2")} == {32, 64, 128, 256}
    for tail in (1, 0):
        bw = [fields(bwd_label(lib, *c, tail)) for c in BWD_CASES]
        names = {n for n, _ in bw}
        assert names == {"actnorm_invconv_bwd_small_kernel<4,%d>" % tail, "actnorm_invconv_bwd_small_kernel<8,%d>" % tail,
                         "actnorm_invconv_bwd_kernel<%d>" % tail}
        big = [f for n, f in bw if "small" not in n]
        assert {f["gW"] for f in big} == {"split", "owned"}
        nys = {f["ny"] for f in big}
        assert 1 in nys and 8 in nys and any(v > 1 and v % 2 for v in nys)
        assert {f["PB"] for f in big} == {64, 128, 256}
        assert any(f["sweeps"] > 1 for f in big) and any(f["sweeps"] == 1 for f in big)
        for Cs in (4, 8):
            assert {f["sweeps"] > 1 for n, f in bw if n.startswith("actnorm_invconv_bwd_small_kernel<%d" % Cs)} == {False, True}
        assert any(f["lds"] > 65536 for f in big)


def _dummy():
    buf = ctypes.create_string_buffer(64)       # never dereferenced: every call below returns before a launch
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _fwd(L, N, C, H, W, z=None, P=None, o_in=None, b3=None, l3=None, o_out=None, scale=None, shift=None, logdet=None,
         clamp=3, bias=None, logs=None, Wm=None, znext=None, ld_const=0):
    return L.rfn_glow_shell_fwd_f32(z, 0, P, o_in, 0, b3, l3, o_out, scale, shift, logdet, clamp, bias, logs, Wm, znext, 0,
                                    ld_const, N, C, H, W, None)


def _shell_bwd(L, N, C, HW, p, clamp=3, **kw):
    a = dict(x=p, bias=p, logs=p, Wm=p, gz=p, gW=p, gbias=p, glogs=p, o=p, glogdet=p, scale=p, shift=p, l3=p, gz_prev=p,
             gpre=p, gscale=p, gshift=p, gb3=p, gl3=p)
    a.update(kw)
    return L.rfn_glow_shell_bwd_f32(a["x"], 0, a["bias"], a["logs"], a["Wm"], a["gz"], 0, a["gW"], a["gbias"], a["glogs"],
                                    a["o"], 0, a["glogdet"], a["scale"], a["shift"], a["l3"], a["gz_prev"], 0, a["gpre"],
                                    0, a["gscale"], a["gshift"], a["gb3"], a["gl3"], clamp, 1, N, C, HW, None)


def _bwd_ld(L, N, C, HW, p, **kw):
    a = dict(x=p, bias=p, logs=p, Wm=p, gz=p, gx=p, gW=p, gbias=p, glogs=p, glogdet=p)
    a.update(kw)
    return L.rfn_actnorm_invconv_bwd_ld_f32(a["x"], 0, a["bias"], a["logs"], a["Wm"], a["gz"], 0, a["gx"], 0, a["gW"],
                                            a["gbias"], a["glogs"], a["glogdet"], N, C, HW, None)


def test_size_limits_refuse_before_any_launch(lib):
    """forward C <= 186 (N = 2, 2x2), rfn_actnorm_invconv_bwd_ld_f32 C <= 146, rfn_glow_shell_bwd_f32 C <= 144: the label
    is a route for the first C of a pair and "unsupported" for the second, whose entry point returns its LDS code with
    the channel count in rfn_last_error() -- the code of the size check, which precedes the launch (a failed launch
    returns a positive HIP error)"""
    L = lib.load()
    keep, p = _dummy()
    assert fwd_label(lib, 2, 186, 2, 2).startswith("glow_shell_fwd_kernel ") and fwd_label(lib, 2, 188, 2, 2) == "unsupported"
    assert fields(fwd_label(lib, 4096, 172, 2, 2))[1]["PB"] == 64 and fwd_label(lib, 4096, 174, 2, 2) == "unsupported"
    assert fwd_label(lib, 2, 188, 2, 2, head=0).startswith("glow_shell_fwd_kernel ")    # a tail stages nothing
    assert _fwd(L, 2, 188, 2, 2, z=p, bias=p, logs=p, Wm=p, znext=p) == -6
    assert b"C=188" in L.rfn_last_error() and b"glow_shell_fwd" in L.rfn_last_error()
    assert bwd_label(lib, 2, 146, 4, 0).startswith("actnorm_invconv_bwd_kernel<0> ") and bwd_label(lib, 2, 148, 4, 0) == "unsupported"
    assert _bwd_ld(L, 2, 148, 4, p) == -3
    assert b"C=148" in L.rfn_last_error() and b"actnorm_invconv_bwd" in L.rfn_last_error()
    assert bwd_label(lib, 2, 144, 4, 1).startswith("actnorm_invconv_bwd_kernel<1> ") and bwd_label(lib, 2, 146, 4, 1) == "unsupported"
    assert _shell_bwd(L, 2, 146, 4, p) == -3
    assert b"C=146" in L.rfn_last_error()
    del keep


def test_a_level_is_supported_only_if_it_can_run_both_ways(lib):
    """rfn_glow_shell_supported is the AND of the three limits (so the backward's C <= 144), and GlowLevelFn asks it
    before it launches anything: 146 < C <= 186 used to run forward and fail in backward"""
    L = lib.load()
    for C in (2, 4, 8, 16, 64, 144):
        assert L.rfn_glow_shell_supported(2, C, 2, 2) == 1 and L.rfn_glow_shell_supported(640, C, 8, 8) == 1
    for C in (146, 148, 186, 188, 3, 0, -2):
        assert L.rfn_glow_shell_supported(2, C, 2, 2) == 0, C
    assert L.rfn_glow_shell_supported(0, 16, 2, 2) == 1 and L.rfn_glow_shell_supported(2, 16, 0, 2) == 0
    for C in range(2, 200, 2):
        ok = all(lab != "unsupported" for lab in (fwd_label(lib, 2, C, 2, 2), bwd_label(lib, 2, C, 4, 1), bwd_label(lib, 2, C, 4, 0)))
        assert L.rfn_glow_shell_supported(2, C, 2, 2) == int(ok) == int(C <= 144), C
    from rfn_hip import ops
    C = 148
    x = torch.zeros(2, C, 2, 2)           # host tensors: the refusal comes before any tensor is looked at
    with pytest.raises(RuntimeError, match=r"GlowLevelFn: a flow level of C=148 channels on 2x2 maps"):
        ops.GlowLevelFn.apply(x, torch.zeros(2, 0, 2, 2), torch.zeros(1, C, C), "relu", 3, None,
                              *[torch.zeros(1)] * ops.STEP_NPARAM)


def test_shell_argument_errors_launch_nothing(lib):
    """the argument checks of the four shell entry points: codes -1 .. -7 of rfn_glow_shell_fwd_f32 in order, the
    backward entry points' -1 .. -3; N == 0 returns 0 without a launch"""
    L = lib.load()
    keep, p = _dummy()
    head = dict(bias=p, logs=p, Wm=p, znext=p)
    tail = dict(o_in=p, logdet=p)
    assert _fwd(L, 0, 4, 2, 2, z=p, **head) == 0
    assert _fwd(L, 2, 5, 2, 2, z=p, **head) == -1                                   # odd C
    assert b"rfn_glow_shell_fwd_f32" in L.rfn_last_error()
    assert _fwd(L, 2, 4, 2, 2, z=None, **head) == -1 and _fwd(L, 2, 4, 0, 2, z=p, **head) == -1
    assert _fwd(L, -1, 4, 2, 2, z=p, **head) == -1
    assert _fwd(L, 2, 4, 2, 2, z=p) == -2                                           # neither tail nor head
    assert _fwd(L, 2, 4, 2, 2, z=p, bias=p, logs=p, znext=p) == -2                  # (the head is named by Wm)
    assert _fwd(L, 2, 4, 2, 2, z=p, P=p, b3=p, l3=p, o_out=p, o_in=p, logdet=p) == -3     # both P and o_in
    assert _fwd(L, 2, 4, 2, 2, z=p, o_in=p) == -3                                   # a tail without log-det partials
    for miss in ("b3", "l3", "o_out"):
        a = dict(P=p, b3=p, l3=p, o_out=p, logdet=p)
        a[miss] = None
        assert _fwd(L, 2, 4, 2, 2, z=p, **a) == -3, miss
    assert _fwd(L, 2, 4, 2, 2, z=p, clamp=0, **tail) == -4                          # realnvp clamp without scales
    assert _fwd(L, 2, 4, 2, 2, z=p, clamp=0, scale=p, **tail) == -4
    assert _fwd(L, 2, 4, 2, 2, z=p, clamp=0, bias=p, logs=p, Wm=p) == -5            # (head only: the clamp is not looked at)
    for miss in ("bias", "logs", "znext"):                                          # head without znext / parameters
        a = dict(head)
        a[miss] = None
        assert _fwd(L, 2, 4, 2, 2, z=p, **a) == -5, miss
    assert _fwd(L, 2, 4, 2, 2, z=p, ld_const=1, **tail) == -7                       # ld_const without head
    assert _fwd(L, 2, 4, 2, 2, z=p, ld_const=1, **head) == -7                       # ... or without partials
    assert L.rfn_logdet_reduce_f32(None, 1, p, 0, 2, 4, 2, 2, None) == -1
    assert L.rfn_logdet_reduce_f32(p, 0, p, 0, 2, 4, 2, 2, None) == -1
    assert L.rfn_logdet_reduce_f32(p, 1, None, 0, 2, 4, 2, 2, None) == -1
    assert L.rfn_logdet_reduce_f32(p, 1, p, 0, 0, 4, 2, 2, None) == 0
    assert lib.load().rfn_glow_shell_fwd_ld_floats(0, 4, 2, 2) == 0

    assert _shell_bwd(L, 0, 4, 4, p) == 0
    assert _shell_bwd(L, 2, 5, 4, p) == -1 and b"rfn_glow_shell_bwd_f32" in L.rfn_last_error()
    for miss in ("x", "bias", "logs", "Wm", "gz", "gW", "gbias", "glogs"):
        assert _shell_bwd(L, 2, 4, 4, p, **{miss: None}) == -1, miss
    assert _shell_bwd(L, 2, 4, 0, p) == -1 and _shell_bwd(L, -1, 4, 4, p) == -1
    for miss in ("o", "l3", "gz_prev", "gpre", "gb3", "gl3"):
        assert _shell_bwd(L, 2, 4, 4, p, **{miss: None}) == -2, miss
    for miss in ("scale", "shift", "gscale", "gshift"):
        assert _shell_bwd(L, 2, 4, 4, p, clamp=0, **{miss: None}) == -3, miss
    assert _bwd_ld(L, 0, 4, 4, p) == 0
    for miss in ("x", "bias", "logs", "Wm", "gz", "gx", "gW", "gbias", "glogs"):
        assert _bwd_ld(L, 2, 4, 4, p, **{miss: None}) == -1, miss
    assert b"rfn_actnorm_invconv_bwd_ld_f32" in L.rfn_last_error()
    assert _bwd_ld(L, 2, 0, 4, p) == -1 and _bwd_ld(L, 2, 4, 0, p) == -1
    for q in ((0, 4, 2, 2, 1), (2, 5, 2, 2, 1), (2, 4, 0, 2, 1)):
        assert fwd_label(lib, *q) == "unsupported"
    for q in ((0, 4, 4, 1), (2, 5, 4, 1), (2, 4, 0, 0)):
        assert bwd_label(lib, *q) == "unsupported"
    assert bwd_label(lib, 2, 5, 4, 0).startswith("actnorm_invconv_bwd_kernel<0> ")   # without a tail C may be odd
    del keep


def test_step_parameters_have_one_stated_order():
    """rfn_hip.ops.StepParams is the order in which Flow/ hands a step's parameters to the three Glow nodes and in which
    their backward returns the gradients: the step's ActNorm, then AffineCoupling.nn_params(), tensor by tensor"""
    from rfn_hip import ops
    from Flow.glow_modules import AffineCoupling
    assert ops.StepParams._fields == ("an_bias", "an_logs", "w1", "n1b", "n1l", "w2", "n2b", "n2l", "w3", "b3", "l3",
                                      "scale", "scale_shift")
    assert ops.STEP_NPARAM == 13
    aff = AffineCoupling([2, 4, 4, 4], [2, 3, 4, 4], hidden_units=8, non_lin="relu", clamp_type="realnvp")
    an_bias, an_logs = object(), object()
    p = ops.StepParams(an_bias, an_logs, *aff.nn_params())
    n0, n2, n4 = aff.net[0], aff.net[2], aff.net[4]
    named = dict(an_bias=an_bias, an_logs=an_logs, w1=n0.conv.weight, n1b=n0.norm_type.bias, n1l=n0.norm_type.logs,
                 w2=n2.conv.weight, n2b=n2.norm_type.bias, n2l=n2.norm_type.logs, w3=n4.conv.weight, b3=n4.conv.bias,
                 l3=n4.logs, scale=aff.scale, scale_shift=aff.scale_shift)
    assert tuple(named) == ops.StepParams._fields
    for field in ops.StepParams._fields:
        assert getattr(p, field) is named[field], field
    # without the realnvp clamp the last two are None, in place
    p = ops.StepParams(an_bias, an_logs, *AffineCoupling([2, 4, 4, 4], [2, 0, 4, 4], 8, "relu", "glow").nn_params())
    assert p.scale is None and p.scale_shift is None and p.l3.shape == (4, 1, 1)
