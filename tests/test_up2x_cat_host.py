"""Launch routes of rfn_up2x_cat_f32 / rfn_up2x_cat_bwd_f32 (nearest 2x up-sampling + channel concatenation in one launch
each way), without a device.  rfn_up2x_cat_kernel_label prints the host struct the launchers read (choose_up2x in
csrc/up2x_cat.hip); `aligned` = every pointer 16-byte aligned and every frame stride a multiple of 4 floats.
tests/test_up2x_cat.py runs the same shapes on the GPU."""
import ctypes

import pytest
import torch

from tests.test_glow_shell_host import fields

UP_GRID_CAP = 8192
# (N, Cx, Cs, h, w) -> access with aligned pointers
UP_SHAPES = {(3, 5, 7, 3, 5): "vec1", (2, 4, 4, 2, 2): "vec4", (1, 1, 1, 1, 1): "vec1", (2, 32, 32, 16, 16): "vec4"}
UP_TWO_SWEEPS = (33, 64, 1, 32, 32)        # forward: 33 * 65 * 64 * 64 / 4 units = 8580 blocks > 8192


@pytest.fixture(scope="module")
def lib():
    from rfn_hip import lib as L_
    L_.load()
    return L_


def up_label(lib, shape, aligned, bwd):
    return lib.load().rfn_up2x_cat_kernel_label(*shape, aligned, bwd).decode()


@pytest.mark.parametrize("shape", list(UP_SHAPES) + [UP_TWO_SWEEPS], ids=lambda s: "x".join(map(str, s)))
def test_up2x_route(lib, shape):
    N, Cx, Cs, h, w = shape
    for bwd in (0, 1):
        for aligned in (0, 1):
            name, f = fields(up_label(lib, shape, aligned, bwd))
            assert name == ("up2x_cat_bwd" if bwd else "up2x_cat")
            vec = bool(aligned) and w % 2 == 0
            assert f["access"] == ("vec4" if vec else "vec1")
            elems = N * Cx * h * w if bwd else 4 * N * (Cx + Cs) * h * w
            units = elems // ((2 if bwd else 4) if vec else 1)
            blocks = -(-units // 256)
            assert f["grid"] == min(blocks, UP_GRID_CAP) and f["sweeps"] == -(-blocks // f["grid"])
    if shape in UP_SHAPES:
        assert fields(up_label(lib, shape, 1, 0))[1]["access"] == UP_SHAPES[shape]
    else:
        assert fields(up_label(lib, shape, 1, 0))[1]["sweeps"] == 2


def test_up2x_refusals(lib):
    L = lib.load()
    assert L.rfn_up2x_cat_kernel_label(0, 1, 1, 1, 1, 1, 0) == b"unsupported"
    assert L.rfn_up2x_cat_kernel_label(2, 1 << 10, 1 << 10, 1 << 9, 1 << 9, 1, 0) == b"unsupported"     # 2^31 and more
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert L.rfn_up2x_cat_f32(p, 4, p, 16, p, 1, 1, 0, 2, 2, None) == -1           # no skip channels: not a concatenation
    assert L.rfn_up2x_cat_f32(p, 3, p, 16, p, 1, 1, 1, 2, 2, None) == -2           # a frame stride shorter than a frame
    assert L.rfn_up2x_cat_bwd_f32(p, 15, p, 1, 1, 2, 2, None) == -2


def test_upscaler_pattern(monkeypatch):
    """Utils.modules._up2x_only: exactly [NearestUp2x()], device fp32 tensors that fit; on the CPU forward_steps keeps
    its separate up-sampling and torch.cat"""
    import torch.nn as nn
    from Utils import modules as M
    x, skip = torch.zeros(2, 3, 4, 4), torch.zeros(2, 5, 8, 8)
    assert not M._up2x_only(nn.Sequential(M.NearestUp2x()), x, skip)                         # CPU tensors
    fake = lambda t: type("T", (), dict(is_cuda=True, dtype=t.dtype, shape=t.shape, dim=t.dim))()
    monkeypatch.delenv("RFN_UP2X_CAT", raising=False)
    assert M._up2x_only(nn.Sequential(M.NearestUp2x()), fake(x), fake(skip))
    assert not M._up2x_only(nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest")), fake(x), fake(skip))
    assert not M._up2x_only(nn.Sequential(M.NearestUp2x(), nn.ReLU()), fake(x), fake(skip))
    assert not M._up2x_only(nn.Sequential(M.NearestUp2x()), fake(x), fake(torch.zeros(2, 5, 8, 6)))
    assert not M._up2x_only(nn.Sequential(M.NearestUp2x()), fake(x.double()), fake(skip))
    monkeypatch.setenv("RFN_UP2X_CAT", "0")
    assert not M._up2x_only(nn.Sequential(M.NearestUp2x()), fake(x), fake(skip))
