"""GPU tests of the two kernels of csrc/iw_bound.hip through rfn_hip.ops: latent_iw against the float64 formula and
against LatentStepFn's bits, keyed_uniform against the host restatement of tests/iw_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import iw_ref

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- latent_iw
def _softplus64(r):
    return torch.where(r > 20, r, torch.log1p(torch.exp(r)))


def _latent_inputs(rows, ZHW, seed):
    """enc, pri [rows, 2*ZHW] and eps [rows, ZHW]: locs ~ N(0, 1), raw scales spread over -10 .. 25 with the values
    around softplus' threshold 20 among them"""
    g = torch.Generator().manual_seed(seed)
    marks = torch.tensor([-10.0, 19.99, 20.0, 20.01, 25.0, 0.0])
    out = []
    for _ in range(2):
        loc = torch.randn(rows, ZHW, generator=g)
        raw = -10.0 + 35.0 * torch.rand(rows, ZHW, generator=g)
        n = min(ZHW, marks.numel())
        for r in range(rows):
            idx = torch.randperm(ZHW, generator=g)[:n]
            raw[r, idx] = marks[torch.randperm(marks.numel(), generator=g)[:n]]
        out.append(torch.cat((loc, raw), 1))
    return out[0].cuda(), out[1].cuda(), torch.randn(rows, ZHW, generator=g).cuda()


def _latent_ref(enc, pri, eps, res_q, step_q, step_p):
    """(z, logr, sum_j |term_j|) in float64.  z: the definition from the raw inputs, softplus in float64.  The terms:
    the float64 formula on the quantities the definition names -- the scales "exactly as rfn_latent_step computes them"
    (step_q: LatentStepFn's outputs for these inputs, step_p: for pri in enc's place, whose enc_std is the prior's
    scale) and the sample z^x_t as it is handed on (step_q's zxt).  A term's four parts nearly cancel where posterior
    and prior are close, so a scale that is one fp32 rounding off would move a term by more than its own size; with
    the step's own scales the comparison is about the term and the sum, as the bound's derivation assumes."""
    enc, pri, eps = enc.double().cpu(), pri.double().cpu(), eps.double().cpu()
    Z = enc.shape[1] // 2
    em, es64 = enc[:, :Z], _softplus64(enc[:, Z:])
    pm, ps64 = pri[:, :Z], _softplus64(pri[:, Z:])
    if res_q:
        em = em + pm
    z64 = em + es64 * eps
    es, ps, z = step_q[4].double().cpu(), step_p[4].double().cpu(), step_q[1].double().cpu()
    assert bool(((es - es64).abs() <= 1e-6 * es64).all()) and bool(((ps - ps64).abs() <= 1e-6 * ps64).all())
    terms = -0.5 * ((z - pm) / ps) ** 2 - ps.log() + 0.5 * eps ** 2 + es.log()
    return z64, terms.sum(1), terms.abs().sum(1)


@pytest.mark.parametrize("res_q", [False, True], ids=["plain", "res_q"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("ZHW", [1, 63, 64, 65, 257])
def test_latent_iw(ZHW, rows, res_q):
    from rfn_hip import ops
    enc, pri, eps = _latent_inputs(rows, ZHW, 1000 * ZHW + 10 * rows + int(res_q))
    zxt, logr = ops.latent_iw(enc, pri, eps, res_q)
    assert tuple(zxt.shape) == (rows, ZHW) and tuple(logr.shape) == (rows,)
    assert zxt.dtype == torch.float32 and logr.dtype == torch.float32
    step = ops.LatentStepFn.apply(enc, pri, torch.zeros_like(eps), eps, res_q)
    step_p = ops.LatentStepFn.apply(pri, pri, torch.zeros_like(eps), eps, False)
    z64, want, size = _latent_ref(enc, pri, eps, res_q, step, step_p)
    err = (logr.double().cpu() - want).abs()
    print("ZHW %d rows %d res_q %d: max |logr - ref| / sum|term| = %.3e" % (ZHW, rows, res_q, float((err / size).max())))
    assert bool((err <= 1e-5 * size).all()), (err, size)
    assert bool((zxt.double().cpu() - z64).abs().max() <= 1e-6 * z64.abs().max())
    # the sample is rfn_latent_step_fwd_f32's, bit for bit
    assert torch.equal(zxt, step[1])
    # a row's bits depend on that row alone
    for r in range(rows):
        z1, l1 = ops.latent_iw(enc[r:r + 1], pri[r:r + 1], eps[r:r + 1], res_q)
        assert torch.equal(z1[0], zxt[r]) and torch.equal(l1[0], logr[r])


def test_latent_iw_takes_conv_shaped_inputs_and_refuses_grad():
    from rfn_hip import ops
    enc, pri, eps = _latent_inputs(3, 4 * 3 * 3, 7)
    flat = ops.latent_iw(enc, pri, eps, True)
    shaped = ops.latent_iw(enc.view(3, 8, 3, 3), pri.view(3, 8, 3, 3), eps.view(3, 4, 3, 3), True)
    assert tuple(shaped[0].shape) == (3, 4, 3, 3)
    assert torch.equal(shaped[0].view(3, -1), flat[0]) and torch.equal(shaped[1], flat[1])
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.latent_iw(enc.clone().requires_grad_(True), pri, eps, False)


def test_latent_iw_entry_point_refuses_empty_sizes():
    from rfn_hip import lib as L
    lib = L.load()
    enc, pri, eps = _latent_inputs(2, 8, 3)
    z = torch.full((2, 8), 7.0, device="cuda")
    lr = torch.full((2,), 7.0, device="cuda")
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in (enc, pri, eps, z, lr)]
    for rows, ZHW in ((0, 8), (2, 0), (-1, 8)):
        assert lib.rfn_latent_iw_f32(*ptrs, rows, ZHW, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((lr == 7.0).all())


# ---------------------------------------------------------------------------------------------- keyed_uniform
def _filled(n_steps, rows, numel, aligned, **address):
    """keyed_uniform into a prepared buffer whose base is 16-byte aligned or 4 bytes past that; returns (tensor, guard
    floats before and after it)"""
    from rfn_hip import ops
    n = n_steps * rows * numel
    buf = torch.full((n + 8,), -1.0, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = 4 if aligned else 5
    out = buf[off:off + n].view(n_steps, rows, numel)
    assert (out.data_ptr() % 16 == 0) == aligned
    got = ops.keyed_uniform(None, out=out, n_steps=n_steps, **address)
    assert got is out
    return out, torch.cat((buf[:off], buf[off + n:]))


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("numel", [1, 7, 8, 13, 256])
def test_keyed_uniform_equals_the_restatement(numel, aligned):
    B, P, S, scale = 3, 2, 2, 2.0 ** -8
    address = dict(B=B, n_draws=P, seed=20261019, first_step=3, scale=scale, first_seq=11, first_draw=4)
    out, guard = _filled(S, P * B, numel, aligned, **address)
    want = iw_ref.keyed_uniform_ref(numel, B, P, 20261019, 3, n_steps=S, scale=scale, first_seq=11, first_draw=4)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    assert bool((guard == -1.0).all())          # nothing outside the tensor
    assert float(out.min()) >= 0.0 and float(out.max()) < scale


def test_keyed_uniform_range_steps_and_splits():
    from rfn_hip import ops
    B, P, S, shape = 2, 5, 3, (3, 4, 5)
    for scale in (1.0, 0.3, 3.0):
        v = ops.keyed_uniform((1 << 12,), B, P, 5, 0, scale=scale, device="cuda")
        assert float(v.min()) >= 0.0 and float(v.max()) < np.float32(scale)
    whole = ops.keyed_uniform(shape, B, P, 9, 2, n_steps=S, first_seq=6, device="cuda")
    assert tuple(whole.shape) == (S, P * B) + shape and whole.dtype == torch.float32
    want = iw_ref.keyed_uniform_ref(60, B, P, 9, 2, n_steps=S, first_seq=6)
    assert torch.equal(whole.cpu().view(S, P * B, 60), torch.from_numpy(want))
    # n_steps = 3 is three one-step launches
    for s in range(S):
        one = ops.keyed_uniform(shape, B, P, 9, 2 + s, first_seq=6, device="cuda")
        assert torch.equal(one[0], whole[s])
    # any split of the draws into calls gives the same bits
    for cuts in ((0, 1, 5), (0, 2, 4, 5), (0, 5)):
        parts = [ops.keyed_uniform(shape, B, b - a, 9, 2, n_steps=S, first_seq=6, first_draw=a, device="cuda")
                 for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(torch.cat(parts, 1), whole)
    # a sequence keeps its numbers wherever it sits in the batch
    solo = ops.keyed_uniform(shape, 1, P, 9, 2, n_steps=S, first_seq=7, device="cuda")
    assert torch.equal(solo, whole.view(S, P, B, *shape)[:, :, 1])
    # first_seq, seed and slot each change the values; the scale only scales them
    for other in (dict(first_seq=7), dict(seed=10, first_seq=6), dict(slot=25, first_seq=6)):
        kw = dict(seed=9, first_seq=6)
        kw.update(other)
        seed = kw.pop("seed")
        assert not torch.equal(ops.keyed_uniform(shape, B, P, seed, 2, n_steps=S, device="cuda", **kw), whole)
    half = ops.keyed_uniform(shape, B, P, 9, 2, n_steps=S, first_seq=6, scale=0.5, device="cuda")
    assert torch.equal(half, whole * 0.5)
    # torch's generators are not touched
    torch.manual_seed(3)
    cpu, gpu = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    ops.keyed_uniform(shape, B, P, 9, 2, device="cuda")
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), gpu)


def test_keyed_uniform_bad_argument_writes_nothing():
    from rfn_hip import lib as L
    from rfn_hip import ops
    lib = L.load()
    out = torch.full((2, 6, 8), -1.0, device="cuda")
    p = ctypes.c_void_p(out.data_ptr())
    #        n_steps rows B numel scale seed first_step slot first_seq first_draw
    good = [2, 6, 3, 8, 1.0, 1, 0, 24, 0, 0]
    bad = {1: 7,            # rows no multiple of B
           2: 0,            # B
           3: -1,           # numel
           4: 0.0,          # scale
           5: -1,           # seed
           6: -1,           # first_step
           7: 7,            # a slot of keyed_normal
           8: -1, 9: -1}    # first_seq, first_draw
    for i, v in bad.items():
        args = list(good)
        args[i] = v
        assert lib.rfn_keyed_uniform_f32(p, *args, None) != 0, (i, v)
        assert b"rfn_keyed_uniform_f32" in lib.rfn_last_error()
    args = list(good)
    args[4] = float("nan")
    assert lib.rfn_keyed_uniform_f32(p, *args, None) != 0
    args = list(good)
    args[6] = (1 << 31) - 1      # the second step would leave the key's 32-bit word
    assert lib.rfn_keyed_uniform_f32(p, *args, None) != 0
    assert lib.rfn_keyed_uniform_f32(ctypes.c_void_p(out.data_ptr() + 2), *good, None) != 0   # no float address
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    for kw in (dict(slot=3), dict(scale=-1.0), dict(first_seq=-1)):
        with pytest.raises(ValueError):
            ops.keyed_uniform(None, 3, 2, 1, 0, n_steps=2, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert lib.rfn_keyed_uniform_f32(p, *good, None) == 0
    torch.cuda.synchronize()
    assert bool((out >= 0.0).all())
