"""rfn_up2x_cat_f32 / rfn_up2x_cat_bwd_f32 and rfn_hip.ops.Up2xCatFn on the GPU.

Forward: a copy, bit-equal to torch.cat((F.interpolate(x, scale_factor=2, mode="nearest"), skip), 1).  Backward: gx = the
2x2 block sums of g[:, :Cx]; the kernel forms each in fp64 and rounds once, so it is within half an ulp of the sum, which
is at most 4 max|addend|: the bound is 2 ulp of the largest addend (2 * 2^-23 * max|addend| per block).  The skip's
gradient is the view g[:, Cx:], bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_recurrent_shell import nan_buf, put
from tests.test_up2x_cat_host import UP_SHAPES, UP_TWO_SWEEPS

pytestmark = pytest.mark.gpu
_i, _l = ctypes.c_int, ctypes.c_long
ids = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def L():
    from rfn_hip import lib
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return lib


def inputs(shape, seed=0):
    N, Cx, Cs, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, Cx, h, w, generator=gen), torch.randn(N, Cs, 2 * h, 2 * w, generator=gen),
            torch.randn(N, Cx + Cs, 2 * h, 2 * w, generator=gen))


def block_sums64(g, Cx):
    N, _, H, W = g.shape
    v = g[:, :Cx].double().view(N, Cx, H // 2, 2, W // 2, 2)
    return v.sum((3, 5)), v.abs().amax((3, 5))


def check_bwd(gx, g, Cx):
    want, big = block_sums64(g.cpu(), Cx)
    err = (gx.cpu().double() - want).abs()
    assert bool((err <= 2.0 * 2.0 ** -23 * big).all()), float((err / big.clamp_min(1e-300)).max() * 2.0 ** 23)


def raw(L, x, skip, g, off=(0, 0, 0, 0, 0)):
    """the two entry points on device copies placed off[i] floats past a 16-byte boundary: x, skip, out, g, gx"""
    N, Cx, h, w = x.shape
    Cs = skip.shape[1]
    xd, sd, gd = put(x, off[0]), put(skip, off[1]), put(g, off[3])
    out, gx = nan_buf((N, Cx + Cs, 2 * h, 2 * w), off[2]), nan_buf((N, Cx, h, w), off[4])
    L.call("rfn_up2x_cat_f32", L.dev(xd), _l(Cx * h * w), L.dev(sd), _l(4 * Cs * h * w), L.dev(out), _i(N), _i(Cx), _i(Cs),
           _i(h), _i(w))
    L.call("rfn_up2x_cat_bwd_f32", L.dev(gd), _l(4 * (Cx + Cs) * h * w), L.dev(gx), _i(N), _i(Cx), _i(h), _i(w))
    torch.cuda.synchronize()
    return out, gx


@pytest.mark.parametrize("off", [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0),
                                 (0, 0, 0, 0, 1)], ids=lambda o: "off" + "".join(map(str, o)))
@pytest.mark.parametrize("shape", list(UP_SHAPES), ids=ids)
def test_up2x_cat_entry_points(L, shape, off):
    x, skip, g = inputs(shape)
    out, gx = raw(L, x, skip, g, off)
    want = torch.cat((F.interpolate(x, scale_factor=2, mode="nearest"), skip), 1)
    assert torch.equal(out.cpu(), want)
    check_bwd(gx, g, x.shape[1])


def test_up2x_cat_reads_channel_slices_in_place(L):
    """x, skip and g as channel slices of wider tensors (frame stride > frame size), aligned and one channel off"""
    N, Cx, Cs, h, w = 3, 4, 6, 2, 3
    gen = torch.Generator().manual_seed(4)
    wx, ws = torch.randn(N, Cx + 3, h, w, generator=gen).cuda(), torch.randn(N, Cs + 2, 2 * h, 2 * w, generator=gen).cuda()
    g = torch.randn(N, Cx + Cs, 2 * h, 2 * w, generator=gen).cuda()
    for c0 in (0, 1):
        x, skip = wx[:, c0:c0 + Cx], ws[:, c0:c0 + Cs]
        out, gx = nan_buf((N, Cx + Cs, 2 * h, 2 * w)), nan_buf((N, Cx, h, w))
        L.call("rfn_up2x_cat_f32", L.dev(x, check_contiguous=False), _l(x.stride(0)), L.dev(skip, check_contiguous=False),
               _l(skip.stride(0)), L.dev(out), _i(N), _i(Cx), _i(Cs), _i(h), _i(w))
        L.call("rfn_up2x_cat_bwd_f32", L.dev(g), _l(g.stride(0)), L.dev(gx), _i(N), _i(Cx), _i(h), _i(w))
        torch.cuda.synchronize()
        assert torch.equal(out, torch.cat((F.interpolate(x, scale_factor=2, mode="nearest"), skip), 1))
        check_bwd(gx, g, Cx)


def test_up2x_cat_two_sweeps(L):
    x, skip, g = inputs(UP_TWO_SWEEPS, 2)
    x, skip = x.cuda(), skip.cuda()
    from rfn_hip import ops as K
    out = K.Up2xCatFn.apply(x, skip)
    assert torch.equal(out, torch.cat((F.interpolate(x, scale_factor=2, mode="nearest"), skip), 1))


@pytest.mark.parametrize("shape", list(UP_SHAPES), ids=ids)
def test_up2x_cat_function(L, shape):
    from rfn_hip import ops as K
    x, skip, g = (t.cuda() for t in inputs(shape, 1))
    xa, sa = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    out = K.Up2xCatFn.apply(xa, sa)
    gx, gs = torch.autograd.grad(out, [xa, sa], g)
    Cx = x.shape[1]
    assert torch.equal(out, torch.cat((F.interpolate(x, scale_factor=2, mode="nearest"), skip), 1))
    assert torch.equal(gs, g[:, Cx:])
    check_bwd(gx, g, Cx)
    (only,) = torch.autograd.grad(K.Up2xCatFn.apply(x, sa), [sa], g)            # x needs no gradient: no launch for it
    assert torch.equal(only, g[:, Cx:])


def test_upscaler_forward_steps_with_and_without_the_fused_launch(L, monkeypatch):
    """VGG_upscaler.forward_steps through Up2xCatFn against RFN_UP2X_CAT=0 (NearestUp2x, then torch.cat): equal outputs,
    gradients equal to rounding (the block sums are rounded once here, three times there)"""
    from Utils import modules as M
    torch.manual_seed(7)
    S, B = 2, 3
    up = M.VGG_upscaler([[8], ["upsample", 6, 6], ["upsample", 4]], 3, 8, norm_type="batchnorm", skips=True,
                        size_skips=[[B, 3, 16, 16], [B, 5, 8, 8], [B, 8, 4, 4]]).cuda().train()
    x = torch.randn(S * B, 8, 4, 4, device="cuda")
    skips = [torch.randn(S * B, 3, 16, 16, device="cuda"), torch.randn(S * B, 5, 8, 8, device="cuda"),
             torch.randn(S * B, 8, 4, 4, device="cuda")]
    state = {k: v.clone() for k, v in up.state_dict().items()}
    calls = {"n": 0}
    real = M.K.Up2xCatFn.apply

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)
    monkeypatch.setattr(M.K.Up2xCatFn, "apply", counted)
    res = {}
    for mode in ("fused", "0"):
        up.load_state_dict(state)
        up.zero_grad(set_to_none=True)
        if mode == "0":
            monkeypatch.setenv("RFN_UP2X_CAT", "0")
        else:
            monkeypatch.delenv("RFN_UP2X_CAT", raising=False)
        xl = x.clone().requires_grad_(True)
        sl = [s.clone().requires_grad_(True) for s in skips]
        before = calls["n"]
        outs = up.forward_steps(xl, S, skip_list=sl)
        sum((o * torch.linspace(-1, 1, o.numel(), device="cuda").view_as(o)).sum() for o in outs).backward()
        torch.cuda.synchronize()
        assert calls["n"] - before == (2 if mode == "fused" else 0)
        res[mode] = ([o.detach() for o in outs], [xl.grad] + [s.grad for s in sl] + [p.grad for p in up.parameters()])
    for a, b in zip(res["fused"][0], res["0"][0]):
        assert torch.equal(a, b)
    for a, b in zip(res["fused"][1], res["0"][1]):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), float((a - b).abs().max() / b.abs().max())
