"""GPU tests of rfn_frames_resize_u8 (through rfn_hip.ops.frames_resize): bit for bit against the numpy restatement of
its definition (tests/clip_folder_ref.py) at every size at which the kernel takes another route -- identity, whole-block
shrink, shrink in one axis and enlarge in the other, the KTH frame cropped and stretched, enlarging from one pixel,
source rows longer than one staging pass (byte-wise and 16-byte loads), more source rows than one pass holds, an
unaligned row pitch behind an odd base address, the 64-bit division -- plus the channel rules, constants, determinism
and every argument error."""
import numpy as np
import pytest
import torch

from tests.clip_folder_ref import resize_ref, weighted_sums, window_ref

pytestmark = pytest.mark.gpu


def rand_frames(F, Hs, Ws, Cs, seed):
    return np.random.default_rng(seed).integers(0, 256, (F, Hs, Ws, Cs), dtype=np.uint8)


def run(src, H, W, Cd, window=None):
    from rfn_hip import ops
    out = ops.frames_resize(torch.from_numpy(src).cuda(), H, W, Cd, window)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (src.shape[0], H, W, Cd) and out.is_contiguous()
    return out.cpu().numpy()


# (F, Hs, Ws, Cs, H, W, Cd, mode)
CASES = [
    (2, 8, 8, 1, 8, 8, 1, "stretch"), (2, 8, 8, 3, 8, 8, 3, "stretch"),      # identity
    (2, 8, 8, 1, 4, 4, 1, "stretch"),                                          # whole 2x2 blocks
    (2, 7, 5, 1, 3, 4, 1, "stretch"), (2, 7, 5, 3, 3, 4, 3, "stretch"),      # shrinks in y, enlarges in x
    (3, 120, 160, 1, 64, 64, 1, "crop"), (3, 120, 160, 1, 64, 64, 1, "stretch"),
    (2, 120, 160, 3, 64, 64, 3, "crop"),
    (2, 1, 1, 1, 4, 4, 1, "stretch"), (2, 1, 1, 3, 4, 4, 3, "stretch"),
    (2, 1, 2100, 1, 1, 3, 1, "stretch"),                                       # a row longer than a pass, single bytes
    (2, 1, 2112, 1, 1, 3, 1, "stretch"),                                       # ... with 16-byte loads
    (1, 2, 704, 3, 1, 2, 3, "stretch"),                                        # ... three channels (2112 bytes)
    (1, 40, 2100, 1, 3, 5, 1, "stretch"),                                      # more rows than a pass holds, too
    (1, 300, 48, 1, 2, 7, 1, "stretch"),                                       # many short rows in 16-byte loads
    (3, 5, 6, 3, 2, 3, 3, "stretch"),                                          # pitch 18: no multiple of 16
    (2, 12, 16, 3, 8, 8, 1, "crop"), (2, 10, 10, 1, 8, 8, 3, "stretch"),      # 3 -> 1 and 1 -> 3
    (2, 9, 300, 1, 5, 300, 1, "stretch"),                                      # W > 256: two column tiles
    (1, 16, 16, 1, 40, 24, 1, "crop"),                                         # enlarging, non-square target
]


@pytest.mark.parametrize("F,Hs,Ws,Cs,H,W,Cd,mode", CASES)
def test_matches_the_definition(F, Hs, Ws, Cs, H, W, Cd, mode):
    from rfn_hip import ops
    src = rand_frames(F, Hs, Ws, Cs, Hs * 31 + Ws)
    window = ops.resize_window(Hs, Ws, H, W, mode)
    assert window == window_ref(Hs, Ws, H, W, mode)
    want = resize_ref(src, H, W, Cd, window)
    got = run(src, H, W, Cd, window)
    assert np.array_equal(got, want)
    assert np.array_equal(run(src, H, W, Cd, window), got)                     # a second launch repeats bit for bit
    assert F < 2 or H * W < 16 or not np.array_equal(got[0], got[1])           # distinct frames stay distinct
    if Cs == Cd:
        s, area = weighted_sums(src, H, W, window)
        assert float(np.abs(got.astype(np.float64) - s.astype(np.float64) / area).max()) <= 0.5
    if (Hs, Ws, Cs) == (H, W, Cd):
        assert np.array_equal(got, src)
    if (Hs, Ws, H, W, Cs) == (8, 8, 4, 4, 1):
        blocks = src.astype(np.int64).reshape(F, 4, 2, 4, 2, 1).sum(axis=(2, 4))
        assert np.array_equal(got, (blocks + 2) // 4)


def test_kth_window():
    from rfn_hip import ops
    assert ops.resize_window(120, 160, 64, 64, "crop") == (0, 20, 120, 120)
    assert ops.resize_window(120, 160, 64, 64, "stretch") == (0, 0, 120, 160)
    assert ops.resize_window(160, 120, 64, 64, "crop") == (20, 0, 120, 120)
    assert ops.resize_window(1, 500, 64, 1, "crop") == (0, 249, 1, 1)          # never empty


def test_odd_base_address():
    """the 5x6x3 frames as a view that starts at an odd byte of its allocation"""
    from rfn_hip import ops
    src = rand_frames(3, 5, 6, 3, 7)
    flat = torch.zeros(src.size + 16, dtype=torch.uint8, device="cuda")
    flat[1:1 + src.size] = torch.from_numpy(src).cuda().reshape(-1)
    view = flat[1:1 + src.size].view(3, 5, 6, 3)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    assert np.array_equal(ops.frames_resize(view, 2, 3, 3).cpu().numpy(), resize_ref(src, 2, 3, 3))
    # an aligned pitch behind an unaligned base goes byte by byte as well
    src = rand_frames(2, 6, 16, 1, 8)
    flat = torch.zeros(src.size + 16, dtype=torch.uint8, device="cuda")
    flat[3:3 + src.size] = torch.from_numpy(src).cuda().reshape(-1)
    assert np.array_equal(ops.frames_resize(flat[3:3 + src.size].view(2, 6, 16, 1), 4, 5, 1).cpu().numpy(),
                          resize_ref(src, 4, 5, 1))


@pytest.mark.parametrize("Cs,Cd", [(1, 1), (3, 3), (3, 1), (1, 3)])
def test_constant_frames_stay_constant(Cs, Cd):
    for value in (0, 255):
        src = np.full((2, 13, 9, Cs), value, dtype=np.uint8)
        for H, W in ((5, 4), (13, 9), (20, 30)):
            got = run(src, H, W, Cd)
            assert got.shape == (2, H, W, Cd) and (got == value).all()


def test_window_inside_the_frame():
    """a window that touches neither border: nothing outside it is read"""
    src = rand_frames(2, 20, 32, 1, 3)
    window = (3, 5, 11, 17)
    want = resize_ref(src, 4, 6, 1, window)
    outside = src.copy()
    outside[:, :3], outside[:, 14:], outside[:, :, :5], outside[:, :, 22:] = 0, 255, 7, 9
    assert np.array_equal(run(src, 4, 6, 1, window), want) and np.array_equal(run(outside, 4, 6, 1, window), want)


def test_large_window_takes_the_64_bit_division():
    """Hc * Wc > 2^24: the rounded sum no longer fits 32 bits"""
    src = rand_frames(1, 513, 32768, 1, 5)
    src[:, :, 16384:] |= 0xc0                                                  # two clearly different halves
    assert 513 * 32768 > 1 << 24
    assert np.array_equal(run(src, 1, 2, 1), resize_ref(src, 1, 2, 1))
    assert (run(np.full((1, 513, 32768, 1), 255, dtype=np.uint8), 2, 1, 1) == 255).all()


def test_no_frames():
    from rfn_hip import ops
    out = ops.frames_resize(torch.empty((0, 9, 7, 3), dtype=torch.uint8, device="cuda"), 4, 4, 1)
    assert tuple(out.shape) == (0, 4, 4, 1) and out.dtype == torch.uint8 and out.is_cuda


def test_side_stream():
    from rfn_hip import ops
    src = rand_frames(4, 30, 40, 3, 9)
    dev = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ops.frames_resize(dev, 16, 16, 3, ops.resize_window(30, 40, 16, 16, "crop"))
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), resize_ref(src, 16, 16, 3, window_ref(30, 40, 16, 16, "crop")))


def test_error_codes_launch_nothing():
    """every negative return of the entry point, with rfn_last_error naming it, and the output untouched"""
    from rfn_hip import lib
    L = lib.load()
    src = torch.from_numpy(rand_frames(2, 8, 8, 1, 1)).cuda()
    out = torch.full((2, 4, 4, 1), 77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(F=2, Hs=8, Ws=8, Cs=1, H=4, W=4, Cd=1, y0=0, x0=0, Hc=8, Wc=8, s=src.data_ptr(), d=out.data_ptr()):
        return L.rfn_frames_resize_u8(s, d, F, Hs, Ws, Cs, H, W, Cd, y0, x0, Hc, Wc, stream)

    bad = [(-1, dict(F=-1)), (-1, dict(Hs=0)), (-1, dict(Ws=0)), (-1, dict(H=0)), (-1, dict(W=0)),
           (-1, dict(Hs=32769, Hc=1)), (-1, dict(W=32769)),
           (-2, dict(Cs=2)), (-2, dict(Cd=4)), (-2, dict(Cs=0)),
           (-3, dict(Hc=0)), (-3, dict(Wc=0)), (-3, dict(y0=-1)), (-3, dict(x0=-1)), (-3, dict(y0=1)), (-3, dict(x0=1)),
           (-3, dict(Hc=9)), (-3, dict(y0=2, Hc=7)), (-3, dict(x0=5, Wc=4)),
           (-4, dict(F=1 << 31, H=4)), (-5, dict(s=None)), (-5, dict(d=0))]
    for code, kw in bad:
        assert call(**kw) == code, kw
        assert b"rfn_frames_resize_u8" in L.rfn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert call(F=0, s=None, d=0) == 0                                      # nothing to do is no error
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), resize_ref(src.cpu().numpy(), 4, 4, 1))


def test_argument_errors():
    from rfn_hip import ops
    src = torch.from_numpy(rand_frames(2, 8, 8, 3, 2)).cuda()
    ops.frames_resize(src, 4, 4, 3)
    for bad, exc in ((src.float(), TypeError), ("frames", TypeError), (src[0], ValueError), (src[..., :2], ValueError),
                     (src[:, :0], ValueError), (src.cpu(), ValueError)):
        with pytest.raises(exc):
            ops.frames_resize(bad, 4, 4, 3)
    for H, W, Cd, window in ((0, 4, 3, None), (4, 0, 3, None), (4, 32769, 3, None), (4, 4, 2, None),
                             (4, 4, 3, (0, 0, 9, 8)), (4, 4, 3, (0, 1, 8, 8)), (4, 4, 3, (-1, 0, 4, 4)),
                             (4, 4, 3, (0, 0, 0, 8))):
        with pytest.raises(ValueError):
            ops.frames_resize(src, H, W, Cd, window)
    with pytest.raises(ValueError):
        ops.resize_window(8, 8, 4, 4, "pad")
