"""GPU tests of the sample sheets: the compose kernel (rfn_hip.ops.compose_sheet -> rfn_sheet_compose_u8) against a
restatement written here from torch on the CPU -- Solver.preprocess(reverse=True) plus slice assignment into a
background-filled array -- bit for bit; the pixel rule at every bin edge; no write outside the output; the same bits on
every launch and stream; and the callers: Solver.plotter, Solver.train with --plot_every, Evaluator.plot_samples."""
import functools
import os
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_moving_mnist_host import _solver_argv
from tests.test_sheet_host import decode_png

pytestmark = pytest.mark.gpu

BG = 200
#          R  N  C  H   W  gutter
CASES = [(1, 1, 1, 5, 7, 0),
         (2, 3, 3, 5, 7, 2),
         (5, 4, 1, 8, 8, 1),
         (3, 2, 3, 64, 64, 2),
         (2, 5, 1, 9, 13, 3)]    # lines of 249 (250 with the lead byte) bytes, odd cell offsets: ragged store ends


def to_bytes(x, n_bits=8, preprocess_range="0.5"):
    """Solver.preprocess(x, reverse=True) on the CPU"""
    from RFN.trainer import Solver
    return Solver.preprocess(SimpleNamespace(n_bits=n_bits, preprocess_range=preprocess_range), x.cpu(), reverse=True)


def restate(rows, n_cols, gutter, bg, n_bits=8, preprocess_range="0.5"):
    """the sheet [Hs, Ws, 3] of CPU row tensors [n, C, H, W] (fp32 in model space or uint8)"""
    C, H, W = rows[0].shape[1:]
    Hs, Ws = len(rows) * H + (len(rows) + 1) * gutter, n_cols * W + (n_cols + 1) * gutter
    sheet = torch.full((Hs, Ws, 3), bg, dtype=torch.uint8)
    for r, t in enumerate(rows):
        u8 = t if t.dtype == torch.uint8 else to_bytes(t, n_bits, preprocess_range)
        for i in range(t.shape[0]):
            y0, x0 = gutter + r * (H + gutter), gutter + i * (W + gutter)
            sheet[y0:y0 + H, x0:x0 + W, :] = u8[i].permute(1, 2, 0).expand(H, W, 3)
    return sheet


@functools.lru_cache(maxsize=None)
def case(R, N, C, H, W, gutter):
    """CPU parents [B, T, ...] / [T, B, ...] (B = 3) of the R rows, how to view them, and the expected sheet; rows are
    taken alternately from parent[0] of [B, T, C, H, W] and parent[:, 0] of [T, B, C, H, W]; rows 1, 4, ... are uint8;
    the last row has N - 1 frames (where N > 1)"""
    g = torch.Generator().manual_seed(R * 1000 + N * 100 + H)
    parents, views = [], []
    for r in range(R):
        n = N - 1 if (r == R - 1 and N > 1) else N
        shape = (3, n, C, H, W) if r % 2 == 0 else (n, 3, C, H, W)
        if r % 3 == 1:
            p = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        else:
            p = torch.rand(shape, generator=g) * 1.2 - 0.6    # some values clamp at either end
        parents.append(p)
        views.append((lambda t: t[0]) if r % 2 == 0 else (lambda t: t[:, 0]))
    want = restate([v(p) for v, p in zip(views, parents)], N, gutter, BG)
    return parents, views, want


@pytest.mark.parametrize("scanlines", [False, True])
@pytest.mark.parametrize("R,N,C,H,W,gutter", CASES)
def test_kernel_matches_restatement(R, N, C, H, W, gutter, scanlines):
    from rfn_hip import ops
    parents, views, want = case(R, N, C, H, W, gutter)
    rows = [v(p.cuda()) for v, p in zip(views, parents)]
    if R > 1:
        assert {t.dtype for t in rows} == {torch.float32, torch.uint8}
        assert rows[-1].shape[0] == N - 1 and not rows[1].is_contiguous()
    got = ops.compose_sheet(rows, N, gutter=gutter, bg=BG, scanlines=scanlines).cpu()
    Hs, Ws = ops.sheet_shape(R, N, H, W, gutter)
    if scanlines:
        assert tuple(got.shape) == (Hs, 1 + 3 * Ws)
        assert not got[:, 0].any(), "the lead column is the PNG filter type 0"
        got = got[:, 1:].reshape(Hs, Ws, 3)
    assert tuple(got.shape) == tuple(want.shape) == (Hs, Ws, 3)
    assert torch.equal(got, want)


@pytest.mark.parametrize("preprocess_range", ["0.5", "1.0"])
@pytest.mark.parametrize("n_bits", [8, 5])
def test_pixel_rule_at_every_bin_edge(n_bits, preprocess_range):
    from rfn_hip import ops
    n_bins = 2 ** n_bits
    shift = 0.5 if preprocess_range == "0.5" else 0.0
    edges = (torch.arange(n_bins + 1, dtype=torch.float32) / n_bins - shift).numpy()    # exact in fp32
    down, up = np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))
    vals = np.concatenate([edges[:-1], down[:-1], up[:-1],
                           np.array([-3.0, 3.0, np.inf, -np.inf, down[-1]], dtype=np.float32)]).astype(np.float32)
    x = torch.from_numpy(vals).reshape(1, 1, 1, -1)
    want = to_bytes(x, n_bits, preprocess_range)
    assert len(torch.unique(want)) >= n_bins    # (x + 0.5 rounds the value below the top edge up to 1.0: torch decides)
    got = ops.compose_sheet([x.cuda()], 1, gutter=0, n_bits=n_bits, preprocess_range=preprocess_range).cpu()
    assert tuple(got.shape) == (1, vals.size, 3)
    assert torch.equal(got, want.reshape(1, -1, 1).expand(1, vals.size, 3))
    nan = torch.full((1, 3, 2, 5), float("nan")).cuda()
    assert not ops.compose_sheet([nan], 1, gutter=0, n_bits=n_bits, preprocess_range=preprocess_range).any()


def test_no_write_outside_out_and_no_read_needed_outside_the_frames():
    """out is a slice at an odd byte address in the middle of a 0xA5-filled allocation, the sources are slices of
    larger allocations whose other elements are NaN / 0x5A"""
    from rfn_hip import ops
    R, N, C, H, W, gutter = CASES[4]
    parents, views, want = case(R, N, C, H, W, gutter)
    rows = []
    for v, p in zip(views, parents):
        big = torch.full((p.shape[0] + 2,) + tuple(p.shape[1:]), float("nan") if p.dtype == torch.float32 else 0x5A,
                         dtype=p.dtype).cuda()
        big[1:-1] = p.cuda()
        rows.append(v(big[1:-1]))
    Hs, Ws = ops.sheet_shape(R, N, H, W, gutter)
    for scanlines, shape in ((True, (Hs, 1 + 3 * Ws)), (False, (Hs, Ws, 3))):
        total, pad = int(np.prod(shape)), 1021
        guard = torch.full((pad + total + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        out = guard[pad:pad + total].view(shape)
        assert out.data_ptr() % 2 == 1
        ret = ops.compose_sheet(rows, N, gutter=gutter, bg=BG, scanlines=scanlines, out=out)
        assert ret.data_ptr() == out.data_ptr()
        g = guard.cpu()
        assert bool((g[:pad] == 0xA5).all()) and bool((g[pad + total:] == 0xA5).all())
        got = g[pad:pad + total].view(shape)
        got = got[:, 1:].reshape(Hs, Ws, 3) if scanlines else got
        assert torch.equal(got, want)


def test_same_bits_on_every_launch_and_stream():
    from rfn_hip import ops
    R, N, C, H, W, gutter = CASES[3]
    parents, views, want = case(R, N, C, H, W, gutter)
    rows = [v(p.cuda()) for v, p in zip(views, parents)]
    a = ops.compose_sheet(rows, N, gutter=gutter, bg=BG, scanlines=True)
    b = ops.compose_sheet(rows, N, gutter=gutter, bg=BG, scanlines=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.compose_sheet(rows, N, gutter=gutter, bg=BG, scanlines=True)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a.cpu()[:, 1:].reshape(want.shape), want)


def _tiny_solver(tmp_path, extra):
    import main_rfn
    from RFN.trainer import Solver
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv(
        "--synthetic_data --choose_data mnist --n_conditions 2 --n_predictions 1 --path %s %s" % (rel, extra)))
    torch.manual_seed(0)
    s = Solver(args)
    s.build()
    return s


def _state_bytes(model):
    return {k: v.detach().cpu().numpy().tobytes() for k, v in model.state_dict().items()}


def test_plotter_writes_the_sheet_and_leaves_the_run_as_it_was(tmp_path):
    from rfn_hip import ops
    s = _tiny_solver(tmp_path, "")
    T, S = s.n_frames, s.image_size
    assert (T, S, s.n_conditions + s.n_predictions) == (4, 32, 3)
    with pytest.raises(RuntimeError, match="not initialised yet"):
        s.plotter()                                  # a fresh model: generating would mark ActNorm layers initialised
    assert s.plot_counter == 0 and os.listdir(s.path + "png_folder") == []
    s.model.train()
    s.train_step(next(iter(s.train_loader)).to(s.device))
    torch.cuda.synchronize()
    for training in (True, False):
        s.model.train(training)
        k = s.plot_counter
        before, cpu_rng, gpu_rng = _state_bytes(s.model), torch.get_rng_state(), torch.cuda.get_rng_state(s.device)
        path = s.plotter()
        assert s.model.training is training
        assert s.plot_counter == k + 1
        assert torch.equal(torch.get_rng_state(), cpu_rng)
        assert torch.equal(torch.cuda.get_rng_state(s.device), gpu_rng)
        assert _state_bytes(s.model) == before
        assert path == s.path + "png_folder/samples%d.png" % k and os.path.isfile(path)
        Hs, Ws = ops.sheet_shape(5, T, S, S, 2)
        (w, h), px = decode_png(open(path, "rb").read())
        assert (h, w) == (Hs, Ws)
        # the generator state is the one the plotter started from: the loader hands out the same first test batch
        image = next(iter(s.test_loader))
        torch.set_rng_state(cpu_rng)
        truth = to_bytes(s.preprocess(image))[0]     # [T, 1, S, S]
        cell = lambda r, i: px[2 + r * (S + 2):2 + r * (S + 2) + S, 2 + i * (S + 2):2 + i * (S + 2) + S]
        for i in range(T):
            assert np.array_equal(cell(0, i), truth[i, 0].numpy()[:, :, None].repeat(3, 2))
        assert (cell(2, T - 1) == 255).all(), "no prediction for the last frame: background"
        # the prediction row starts with the conditioning frames
        for i in range(s.n_conditions):
            assert np.array_equal(cell(2, i), cell(0, i))
        assert (px[:2] == 255).all() and (px[:, :2] == 255).all()
        for r in (1, 2, 3, 4):                        # the other cells hold frames, not background
            assert cell(r, 1).min() < 255
    assert sorted(os.listdir(s.path + "png_folder")) == ["samples0.png", "samples1.png"]


def test_train_writes_sheets_only_when_asked(tmp_path):
    s = _tiny_solver(tmp_path / "on", "--plot_every 1 --max_steps 2 --n_epochs 2")
    s.train()
    assert os.listdir(s.path + "png_folder") == ["samples0.png"] and s.plot_counter == 1
    assert s.counter == 2
    off = _tiny_solver(tmp_path / "off", "--max_steps 2 --n_epochs 2")
    off.train()
    assert os.listdir(off.path + "png_folder") == [] and off.plot_counter == 0
    assert off.counter == 2


def test_evaluator_plot_samples(tmp_path):
    from evaluation_metrics import Evaluator
    g = torch.Generator().manual_seed(5)
    pred = torch.randint(0, 256, (3, 4, 3, 8, 8), generator=g, dtype=torch.uint8)
    true = torch.randint(0, 256, (3, 4, 3, 8, 8), generator=g, dtype=torch.uint8)
    solver = SimpleNamespace(model=None, args=Namespace(), device=torch.device("cuda"), path=str(tmp_path) + "/")
    path = Evaluator(solver).plot_samples(pred.cuda(), true, name="best", n=2)    # inputs on either device
    assert path == str(tmp_path) + "/eval_folder/best.png"
    (w, h), px = decode_png(open(path, "rb").read())
    assert (h, w) == (4 * 8 + 5 * 2, 4 * 8 + 5 * 2)
    want = restate([true[0], pred[0], true[1], pred[1]], 4, 2, 255)
    assert np.array_equal(px, want.numpy())
    for r, src in enumerate((true[0], pred[0], true[1], pred[1])):
        for i in range(4):
            assert np.array_equal(px[2 + 10 * r:10 + 10 * r, 2 + 10 * i:10 + 10 * i], src[i].permute(1, 2, 0).numpy())
    assert os.listdir(str(tmp_path) + "/eval_folder") == ["best.png"]
