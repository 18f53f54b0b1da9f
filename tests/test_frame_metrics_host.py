"""CPU tests of the frame-quality metrics (rfn_frame_quality_u8, rfn_hip.ops.frame_quality, Evaluator.eval_seq): the
library exports and binds the entry point, the numpy restatement used by the GPU tests agrees with a float64 scipy
transcription of skimage 0.17.2's `structural_similarity` / `peak_signal_noise_ratio`, and the product refuses CPU
tensors, non-integer inputs and frames smaller than the 7x7 window.

The restatement below is test infrastructure: the product never imports it."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

WIN = 7


# ---------------------------------------------------------------------------------------------------- restatement
def _window_sums(x):
    """7x7 window sums over the interior windows of an integer image (exact in int64)"""
    return np.lib.stride_tricks.sliding_window_view(x, (WIN, WIN)).sum(axis=(-1, -2))


def ref_ssim_psnr_channel(x, y):
    """(ssim, psnr, sse) of one uint8 channel pair: skimage 0.17.2 defaults (7x7 uniform window, data_range 255,
    K1 0.01, K2 0.03, sample covariance, S averaged over the (H-6) x (W-6) interior) in the exact-integer form"""
    x = np.asarray(x, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    sx, sy = _window_sums(x), _window_sums(y)
    sxx, syy, sxy = _window_sums(x * x), _window_sums(y * y), _window_sums(x * y)
    c1s = (0.01 * 255.0) ** 2 * 2401.0
    c2s = (0.03 * 255.0) ** 2 * 2352.0
    num = (2.0 * (sx * sy) + c1s) * (2.0 * (49 * sxy - sx * sy) + c2s)
    den = ((sx * sx + sy * sy) + c1s) * (((49 * sxx - sx * sx) + (49 * syy - sy * sy)) + c2s)
    ssim = float((num / den).mean())
    sse = int(((x - y) ** 2).sum())
    psnr = math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 / (sse / x.size))
    return ssim, psnr, sse


def ref_frame_quality(a, b):
    """per-frame (mse, psnr, ssim) float64 arrays of uint8 arrays [..., C, H, W]"""
    a, b = np.asarray(a), np.asarray(b)
    C, H, W = a.shape[-3:]
    lead = a.shape[:-3]
    af, bf = a.reshape(-1, C, H, W), b.reshape(-1, C, H, W)
    mse, psnr, ssim = (np.empty(af.shape[0]) for _ in range(3))
    for n in range(af.shape[0]):
        s = [ref_ssim_psnr_channel(af[n, c], bf[n, c]) for c in range(C)]
        ssim[n] = sum(v[0] for v in s) / C
        psnr[n] = sum(v[1] for v in s) / C
        mse[n] = sum(v[2] for v in s) / (C * H * W)
    return mse.reshape(lead), psnr.reshape(lead), ssim.reshape(lead)


def _skimage_ssim_scipy(x, y):
    """float64 transcription of skimage 0.17.2 structural_similarity(x, y) on uint8 2-D images with its defaults"""
    from scipy.ndimage import uniform_filter
    X, Y = x.astype(np.float64), y.astype(np.float64)
    NP = WIN ** 2
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(X, size=WIN), uniform_filter(Y, size=WIN)
    uxx, uyy, uxy = uniform_filter(X * X, size=WIN), uniform_filter(Y * Y, size=WIN), uniform_filter(X * Y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    R = 255
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (WIN - 1) // 2
    return S[pad:-pad, pad:-pad].mean(dtype=np.float64)


def _skimage_psnr(x, y):
    err = np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2)
    with np.errstate(divide="ignore"):
        return 10 * np.log10((255.0 ** 2) / err)


def _pairs(seed):
    rng = np.random.default_rng(seed)
    out = []
    for H, W in ((7, 7), (16, 16), (37, 53), (64, 64)):
        x = rng.integers(0, 256, (H, W), dtype=np.uint8)
        noise = rng.integers(-40, 41, (H, W))
        out.append((x, rng.integers(0, 256, (H, W), dtype=np.uint8)))           # unrelated
        out.append((x, np.clip(x.astype(np.int64) + noise, 0, 255).astype(np.uint8)))  # correlated
    return out


# ---------------------------------------------------------------------------------------------------- tests
def test_library_exports_and_binds_frame_quality():
    import ctypes
    from rfn_hip import lib
    L = lib.load()
    assert hasattr(L, "rfn_frame_quality_u8")
    assert lib.SIGNATURES["rfn_frame_quality_u8"] == [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert L.rfn_abi_version() == lib.ABI_VERSION == 2


def test_restatement_matches_skimage_transcription():
    pytest.importorskip("scipy")
    for x, y in _pairs(0):
        ssim, psnr, _ = ref_ssim_psnr_channel(x, y)
        want = _skimage_ssim_scipy(x, y)
        assert abs(ssim - want) <= 1e-12, (x.shape, ssim, want)
        assert psnr == _skimage_psnr(x, y) or abs(psnr - _skimage_psnr(x, y)) <= 1e-12 * abs(psnr)


def test_restatement_identity_and_symmetry():
    for x, y in _pairs(1):
        s, p, e = ref_ssim_psnr_channel(x, x)
        assert abs(s - 1.0) <= 1e-15 and p == math.inf and e == 0
        assert ref_ssim_psnr_channel(x, y) == ref_ssim_psnr_channel(y, x)
    a = np.random.default_rng(2).integers(0, 256, (2, 3, 3, 9, 11), dtype=np.uint8)
    mse, psnr, ssim = ref_frame_quality(a, a)
    assert mse.shape == (2, 3) and (mse == 0).all() and np.isinf(psnr).all() and np.allclose(ssim, 1.0, atol=1e-15)


def _evaluator():
    from evaluation_metrics import Evaluator
    solver = SimpleNamespace(model=None, args=SimpleNamespace(n_frames=4), device=torch.device("cpu"))
    return Evaluator(solver)


def test_frame_quality_refuses_bad_inputs():
    from rfn_hip import ops
    a = torch.zeros(2, 1, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.frame_quality(a, a)
    with pytest.raises(TypeError, match="uint8"):
        ops.frame_quality(a.float() + 0.5, a.float())
    with pytest.raises(TypeError, match="uint8"):
        ops.frame_quality(a.float(), a.float())
    for shape in ((2, 1, 6, 16), (2, 1, 16, 6)):
        small = torch.zeros(shape, dtype=torch.uint8)
        with pytest.raises(ValueError, match="window"):
            ops.frame_quality(small, small)
    with pytest.raises(ValueError, match="shapes differ"):
        ops.frame_quality(a, torch.zeros(2, 1, 16, 17, dtype=torch.uint8))


def test_eval_seq_refuses_bad_inputs():
    ev = _evaluator()
    x = torch.zeros(2, 3, 1, 16, 16)
    with pytest.raises(RuntimeError, match="device tensors"):
        ev.eval_seq(x, x)
    with pytest.raises(RuntimeError, match="device tensors"):
        ev.eval_seq(x.byte(), x.byte())
    for bad in (x + 0.5, x - 1.0, x + 256.0, torch.full_like(x, float("nan"))):
        with pytest.raises(ValueError):
            ev.eval_seq(bad, x)
    with pytest.raises(ValueError):
        ev.eval_seq(x.long(), x.long())
    for shape in ((2, 3, 1, 6, 16), (2, 3, 1, 16, 6)):
        small = torch.zeros(shape)
        with pytest.raises(ValueError, match="window"):
            ev.eval_seq(small, small)
    with pytest.raises(ValueError):
        ev.eval_seq(x[0], x[0])
