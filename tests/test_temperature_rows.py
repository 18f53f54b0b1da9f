"""GPU tests of the two kernels behind per-row temperatures: rfn_gauss_sample_rows_f32 (csrc/gauss.hip; one temperature
per frame, the same kernel as the scalar entry point) against fp64 and against the scalar call's bits, and the tiled
addressed noise rfn_keyed_normal_tiled_f32 (csrc/keyed_normal.hip through ops.keyed_normal(tiles=K)) against the untiled
call, plus the argument errors of both wrappers.

Shapes (N, Cz, HW) of the Gaussian test: (3, 3, 5) and (3, 5, 64) -- 15 and 320 elements per frame, i.e. one and two
sweeps of the block's 256 threads, the two branches of the element loop -- and the three-frame rows of GAUSS_CASES.  The
bound is EW_BOUND of tests/test_recurrent_shell.py, the bound of the scalar kernel; the reference takes the float32
temperatures the kernel is given."""
import ctypes

import pytest
import torch

from tests.test_glow_shell import SENT, untouched, view_of
from tests.test_recurrent_shell import EW_BOUND, relerr
from tests.test_recurrent_shell_host import GAUSS_CASES, gauss_sample_ref

pytestmark = pytest.mark.gpu

_i, _l, _f = ctypes.c_int, ctypes.c_long, ctypes.c_float
ids = lambda c: "x".join(map(str, c))
ROW_TEMPERATURES = (0.0, 1e-9, 2.0)
CASES = [(3, 3, 5), (3, 5, 64)] + [c for c in GAUSS_CASES if c[0] == len(ROW_TEMPERATURES)]


@pytest.fixture(scope="module")
def L():
    from rfn_hip import lib
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return lib


def gauss_inputs(case, std_mode):
    N, Cz, HW = case
    gen = torch.Generator().manual_seed(900 + CASES.index(case) * 2 + std_mode)
    return torch.randn(N, 2 * Cz, HW, generator=gen), torch.randn(N, Cz, HW, generator=gen)


def test_cases_reach_both_branches_of_the_element_loop():
    assert {-(-Cz * HW // 256) > 1 for _, Cz, HW in CASES[:2]} == {False, True}
    assert all(N == len(ROW_TEMPERATURES) for N, _, _ in CASES)


@pytest.mark.parametrize("std_mode", (0, 1), ids=("softplus", "exp"))
@pytest.mark.parametrize("layout", (0, 1), ids=("cross", "split"))
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gauss_sample_rows_vs_fp64(L, case, layout, std_mode):
    N, Cz, HW = case
    o, eps = gauss_inputs(case, std_mode)
    temps = torch.tensor(ROW_TEMPERATURES, dtype=torch.float32)
    ref = gauss_sample_ref(o.double(), eps.double(), temps.double().view(N, 1, 1), layout, std_mode)
    mean = gauss_sample_ref(o.double(), eps.double(), 0.0, layout, std_mode)
    (opar, od) = view_of(o)
    op, ons = L.frames(od, "o")
    runs = []
    for _ in range(2):
        (zpar, z) = view_of((N, Cz, HW))
        zp, zns = L.frames(z, "z")
        L.call("rfn_gauss_sample_rows_f32", op, _l(ons), L.dev(eps.cuda()), zp, _l(zns), L.dev(temps.cuda()), _i(layout),
               _i(std_mode), _i(N), _i(Cz), _i(HW))
        torch.cuda.synchronize()
        assert untouched(zpar) and untouched(opar), "wrote outside a channel slice"
        runs.append(z.cpu())
    got = runs[0]
    errs = [relerr(got[n], ref[n]) for n in range(N)]
    print("\nGAUSS ROWS %s %s %s | %s" % (ids(case), ("cross", "split")[layout], ("softplus", "exp")[std_mode],
                                         " ".join("T=%g %.1e" % (t, e) for t, e in zip(ROW_TEMPERATURES, errs))))
    assert all(e < EW_BOUND for e in errs), errs
    assert relerr(got, ref) < EW_BOUND
    assert torch.equal(got[0].double(), mean[0].float().double()), "temperature 0 is the mean, exactly"
    assert torch.equal(runs[0], runs[1]), "two runs differ"


@pytest.mark.parametrize("std_mode", (0, 1), ids=("softplus", "exp"))
@pytest.mark.parametrize("layout", (0, 1), ids=("cross", "split"))
@pytest.mark.parametrize("case", CASES[:2], ids=ids)
def test_gauss_sample_rows_give_the_scalars_bits(case, layout, std_mode):
    from rfn_hip import ops
    N, Cz, HW = case
    o, eps = gauss_inputs(case, std_mode)
    o, eps = o.cuda().view(N, 2 * Cz, HW, 1), eps.cuda().view(N, Cz, HW, 1)     # the wrapper takes [N, C, H, W]
    scalar = ops.gauss_sample(o, eps, layout, std_mode, 0.7)
    assert tuple(scalar.shape) == (N, Cz, HW, 1) and not bool(torch.isnan(scalar).any())
    rows = ops.gauss_sample(o, eps, layout, std_mode, torch.full((N,), 0.7, device="cuda"))
    again = ops.gauss_sample(o, eps, layout, std_mode, torch.full((N,), 0.7, device="cuda"))
    assert torch.equal(rows, scalar) and torch.equal(rows, again)
    # one value per frame: every frame equals the scalar call at its own temperature
    temps = torch.tensor([0.3, 1.0, 0.7], device="cuda")
    mixed = ops.gauss_sample(o, eps, layout, std_mode, temps)
    for n in range(N):
        one = ops.gauss_sample(o, eps, layout, std_mode, float(temps[n]))
        assert torch.equal(mixed[n], one[n])


# ------------------------------------------------------------------------------------------------ tiled addressed noise
B, R, TILES, SEED = 2, 3, 3, 20261019
ADDR = dict(step=7, first_seq=(1 << 40) + 3, first_draw=5)
SHAPES = [(5,), (8,), (24,)]      # a tail block with single stores; one and three Philox blocks on the 16-byte path


def test_keyed_normal_tiles_repeat_the_untiled_rows():
    from rfn_hip import ops
    plain = ops.keyed_normal(SHAPES, B, R, SEED, device="cuda", **ADDR)
    tiled = ops.keyed_normal(SHAPES, B, R, SEED, device="cuda", tiles=TILES, **ADDR)
    for sh, p, t in zip(SHAPES, plain, tiled):
        assert tuple(t.shape) == (TILES * R * B,) + sh and t.dtype == torch.float32
        for k in range(TILES):
            assert torch.equal(t[k * R * B:(k + 1) * R * B], p), (sh, k)
    # the documented row: (k * n_draws + r) * B + b holds draw first_draw + r of sequence first_seq + b
    one = ops.keyed_normal(SHAPES, 1, 1, SEED, ADDR["step"], ADDR["first_seq"] + 1, ADDR["first_draw"] + 2, device="cuda")
    for t, o in zip(tiled, one):
        for k in range(TILES):
            assert torch.equal(t[ops.keyed_normal_tiled_row(k, 2, 1, R, B)], o[0])
    again = ops.keyed_normal(SHAPES, B, R, SEED, device="cuda", tiles=TILES, **ADDR)
    assert all(torch.equal(a, b) for a, b in zip(tiled, again))


def test_keyed_normal_tiles_into_a_misaligned_tensor_and_past_a_skipped_slot():
    """out tensors inside sentinel-filled buffers; the 24-value slot starts 4 bytes past a 16-byte boundary, so it takes
    the single stores although its rows are a multiple of 8 values; slot 1 is skipped and stays skipped"""
    from rfn_hip import ops
    rows = TILES * R * B
    bufs, views = [], []
    for n, off in ((8, 4), (24, 1)):
        buf = torch.full((rows * n + 12,), SENT, device="cuda", dtype=torch.float32)
        v = buf[off:off + rows * n].view(rows, n)
        assert v.data_ptr() % 16 == (0 if off == 4 else 4)
        bufs.append((buf, off, rows * n))
        views.append(v)
    outs = ops.keyed_normal(None, B, R, SEED, out=[views[0], None, views[1]], tiles=TILES, **ADDR)
    torch.cuda.synchronize()
    assert outs[1] is None and outs[0] is views[0] and outs[2] is views[1]
    plain = ops.keyed_normal([(8,), None, (24,)], B, R, SEED, device="cuda", **ADDR)
    assert plain[1] is None
    for j, v in ((0, views[0]), (2, views[1])):
        for k in range(TILES):
            assert torch.equal(v[k * R * B:(k + 1) * R * B], plain[j]), (j, k)
    for buf, off, n in bufs:
        assert bool((buf[:off] == SENT).all()) and bool((buf[off + n:] == SENT).all()), "wrote outside the tensor"
    fresh = ops.keyed_normal([(8,), None, (24,)], B, R, SEED, device="cuda", tiles=TILES, **ADDR)
    assert fresh[1] is None and torch.equal(fresh[0], views[0]) and torch.equal(fresh[2], views[1])


def test_one_tile_is_todays_call():
    from rfn_hip import ops
    a = ops.keyed_normal(SHAPES, B, R, SEED, device="cuda", **ADDR)
    b = ops.keyed_normal(SHAPES, B, R, SEED, device="cuda", tiles=1, **ADDR)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert ops.keyed_normal(SHAPES, B, 0, SEED, device="cuda", tiles=2, **ADDR)[0].shape[0] == 0   # no rows: no launch


def test_argument_errors():
    from rfn_hip import ops
    o, eps = torch.zeros(3, 4, 2, 2, device="cuda"), torch.zeros(3, 2, 2, 2, device="cuda")
    with pytest.raises(ValueError, match="temperature is on cpu"):
        ops.gauss_sample(o, eps, 0, 0, torch.zeros(3))
    with pytest.raises(ValueError, match="temperature holds 4 values for 3 frames"):
        ops.gauss_sample(o, eps, 0, 0, torch.zeros(4, device="cuda"))
    with pytest.raises(TypeError, match="temperature tensor must be float32"):
        ops.gauss_sample(o, eps, 0, 0, torch.zeros(3, device="cuda", dtype=torch.float16))
    with pytest.raises(TypeError, match="temperature must be a number"):
        ops.gauss_sample(o, eps, 0, 0, [0.7] * 3)
    with pytest.raises(ValueError, match="tiles must be at least 1"):
        ops.keyed_normal(SHAPES, B, R, SEED, 0, device="cuda", tiles=0)
    with pytest.raises(TypeError, match="tiles must be an int"):
        ops.keyed_normal(SHAPES, B, R, SEED, 0, device="cuda", tiles=2.5)
    with pytest.raises(ValueError, match="must have 18 rows"):
        ops.keyed_normal(None, B, R, SEED, 0, out=[torch.zeros(R * B, 8, device="cuda")], tiles=TILES)
    with pytest.raises(ValueError, match="rows exceed one launch"):
        ops.keyed_normal(SHAPES, 1 << 20, 1 << 10, SEED, 0, device="cuda", tiles=4)
