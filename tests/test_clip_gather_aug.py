"""GPU tests of rfn_clip_gather_aug_u8_f32 (through rfn_hip.ops.clip_gather_aug): bit for bit the existing gather when
nothing is asked of it; the mirror, the time reversal and the stride against torch's own flips and explicit frame indices
and against the numpy restatement (tests/clip_folder_ref.py), on the vector path, the two-run frame, the pixel-by-pixel
path and a vectorised frame whose width is no multiple of 4; the guard; the empty batch; capture and replay."""
import numpy as np
import pytest
import torch

from tests.clip_folder_ref import gather_aug_ref
from tests.test_clip_gather import make_store

pytestmark = pytest.mark.gpu

# (Cs, C, H, W): the vector path; two runs per frame; the scalar path twice; W = 4 (one group per row); a frame that
# loads 16 bytes at a time but whose rows hold no whole groups (mirrored clips go pixel by pixel); three channels of it
SHAPES = [(3, 3, 64, 64), (1, 1, 64, 64), (1, 3, 36, 36), (3, 3, 36, 36), (3, 3, 5, 7), (1, 1, 2, 6), (1, 1, 8, 4),
          (3, 3, 4, 4), (1, 1, 8, 6), (3, 3, 8, 6)]


def dev(values, dtype):
    return torch.tensor(values, dtype=dtype, device="cuda")


def ref(store, first, T, C, step=1, flags=None):
    return torch.from_numpy(gather_aug_ref(store.cpu().numpy(), first.cpu().numpy(), T, C, step,
                                           None if flags is None else flags.cpu().numpy())).cuda()


def same(a, b):
    """bit for bit, NaN rows included"""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("Cs,C", [(1, 1), (1, 3), (3, 3)])
@pytest.mark.parametrize("H,W", [(64, 64), (36, 36), (5, 7)])
def test_plain_call_is_the_existing_gather(Cs, C, H, W):
    from rfn_hip import ops
    T, F = 3, 11
    store = make_store(F, H, W, Cs, H + Cs)
    first = dev([F - T, 0, 4, -1, F - T + 1], torch.int64)
    want = ops.clip_gather(store, first, T, C)
    assert same(ops.clip_gather_aug(store, first, T, C), want)
    assert same(ops.clip_gather_aug(store, first, T, C, step=1, flags=torch.zeros(5, dtype=torch.int32, device="cuda")),
                want)
    assert same(ops.clip_gather_aug(store, first, T, C, flags=dev([4, 8, 1 << 30, -4, 12], torch.int32)), want)


@pytest.mark.parametrize("Cs,C,H,W", SHAPES)
def test_mirror_reverse_and_stride(Cs, C, H, W):
    from rfn_hip import ops
    T, F = 3, 12
    store = make_store(F, H, W, Cs, 3 * H + W)
    first = dev([2, 0, F - T, 5, 1], torch.int64)
    plain = ops.clip_gather(store, first, T, C)
    for bits, want in ((1, plain.flip(-1)), (2, plain.flip(1)), (3, plain.flip(-1).flip(1))):
        got = ops.clip_gather_aug(store, first, T, C, flags=torch.full((5,), bits, dtype=torch.int32, device="cuda"))
        assert got.is_contiguous() and torch.equal(got, want), bits
    # one batch, another augmentation per row
    flags = dev([0, 1, 2, 3, 1], torch.int32)
    got = ops.clip_gather_aug(store, first, T, C, flags=flags)
    for b, bits in enumerate([0, 1, 2, 3, 1]):
        want = plain[b]
        want = want.flip(-1) if bits & 1 else want
        want = want.flip(0) if bits & 2 else want
        assert torch.equal(got[b], want), (b, bits)
    assert same(got, ref(store, first, T, C, 1, flags))
    # strides: the explicit frames, one single-frame gather each
    for step in (2, 3):
        starts = [0, F - 1 - (T - 1) * step, 1, 2, 0]
        first = dev(starts, torch.int64)
        got = ops.clip_gather_aug(store, first, T, C, step=step)
        frames = dev([s + t * step for s in starts for t in range(T)], torch.int64)
        assert torch.equal(got, ops.clip_gather(store, frames, 1, C).reshape(5, T, C, H, W))
        got = ops.clip_gather_aug(store, first, T, C, step=step, flags=flags)
        assert same(got, ref(store, first, T, C, step, flags))


@pytest.mark.parametrize("Cs,C,H,W", [(3, 3, 64, 64), (1, 3, 36, 36), (3, 3, 5, 7), (1, 1, 8, 6)])
@pytest.mark.parametrize("step", [1, 3])
def test_guard(Cs, C, H, W, step):
    from rfn_hip import ops
    T, F = 3, 10
    store = make_store(F, H, W, Cs, 17)
    last = F - 1 - (T - 1) * step                       # the last valid start
    first = dev([last, last + 1, 2, -1, 0, F - (T - 1) * step, F + 100, -(1 << 62), 1 << 62, last], torch.int64)
    flags = dev([3, 3, 1, 1, 2, 0, 3, 1, 2, 0], torch.int32)
    out = ops.clip_gather_aug(store, first, T, C, step=step, flags=flags)
    bad, good = [1, 3, 5, 6, 7, 8], [0, 2, 4, 9]
    assert int(first[5]) + (T - 1) * step == F          # the clip's last frame would be frame n_frames
    assert bool(torch.isnan(out[bad]).all())
    assert not bool(torch.isnan(out[good]).any())
    assert same(out, ref(store, first, T, C, step, flags))


def test_empty_batch():
    from rfn_hip import ops
    store = make_store(9, 16, 16, 3, 2)
    out = ops.clip_gather_aug(store, torch.zeros(0, dtype=torch.int64, device="cuda"), 4, 3, step=2,
                              flags=torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert tuple(out.shape) == (0, 4, 3, 16, 16) and out.dtype == torch.float32 and out.is_cuda


def test_capture_and_replay():
    from rfn_hip import ops
    T, F = 4, 20
    store = make_store(F, 16, 16, 3, 4)
    first = dev([3, 0, 9], torch.int64)
    flags = dev([1, 2, 3], torch.int32)
    eager = ops.clip_gather_aug(store, first, T, 3, step=2, flags=flags)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.clip_gather_aug(store, first, T, 3, step=2, flags=flags)       # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.clip_gather_aug(store, first, T, 3, step=2, flags=flags)
    first.copy_(dev([1, 5, 2], torch.int64))             # the replay reads the tables, not the capture's values
    flags.copy_(dev([3, 0, 1], torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.clip_gather_aug(store, first, T, 3, step=2, flags=flags))
    assert not torch.equal(out, eager)


def test_argument_errors():
    from rfn_hip import ops
    store = make_store(6, 4, 4, 3, 1)
    first = torch.zeros(2, dtype=torch.int64, device="cuda")
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.clip_gather_aug(store, first, 2, 3, 1, flags)
    for bad, exc in ((flags.long(), TypeError), ([0, 0], TypeError), (flags[:1], ValueError), (flags.cpu(), ValueError),
                     (flags[:, None], ValueError)):
        with pytest.raises(exc):
            ops.clip_gather_aug(store, first, 2, 3, 1, bad)
    for step in (0, -1, 1.5, True, 1 << 31):
        with pytest.raises(ValueError):
            ops.clip_gather_aug(store, first, 2, 3, step)
    with pytest.raises(TypeError):
        ops.clip_gather_aug(store.float(), first, 2, 3)
    with pytest.raises(ValueError):
        ops.clip_gather_aug(store, first.cpu(), 2, 3)
    with pytest.raises(ValueError):
        ops.clip_gather_aug(store, first, 2, 1)
    # the entry point's own codes, nothing launched
    from rfn_hip import lib
    L = lib.load()
    out = torch.full((2, 2, 3, 4, 4), 5.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda st=store.data_ptr(), fi=first.data_ptr(), fl=flags.data_ptr(), o=out.data_ptr(), B=2, T=2, C=3, Cs=3, \
        H=4, W=4, step=1: L.rfn_clip_gather_aug_u8_f32(st, 6, fi, fl, o, B, T, C, Cs, H, W, step, s)
    for code, kw in ((-1, dict(step=0)), (-1, dict(T=0)), (-1, dict(B=-1)), (-2, dict(C=1)), (-2, dict(Cs=2)),
                     (-3, dict(H=1 << 15, W=1 << 15)), (-4, dict(B=1 << 30, T=4)), (-5, dict(st=None)),
                     (-5, dict(fi=None)), (-5, dict(o=None)), (-6, dict(fl=flags.data_ptr() + 2))):
        assert call(**kw) == code, kw
        assert b"rfn_clip_gather_aug_u8_f32" in L.rfn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert call(fl=None) == 0
