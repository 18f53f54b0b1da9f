"""GPU tests of the animated clips: rfn_hip.ops.compose_clip (csrc/clip_compose.hip) bit for bit against the CPU
restatement tests/clip_compose_ref.py in both output layouts -- grids, zoom, rings, gutters, both kinds, the three
modes, strided views, held last frames, empty cells, G up to the limit, values beyond the clamp ends and NaN, writes into
a canary-framed view at every byte offset, repeat launches and a side stream -- and the callers: Evaluator.plot_clips
and tools/predict_clips.py on one-step synthetic runs (rfn.pt and vrnn.pt)."""
import importlib.util
import os
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.clip_compose_ref import clip_shape, compose_clip_ref, to_bytes
from tests.test_clip_compose_host import parse_apng
from tests.test_moving_mnist_host import _solver_argv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = 201


def frames_of(rs, kind, shape):
    """random frames on the CPU: uint8, or fp32 in model space reaching past both clamp ends"""
    if kind == 1:
        return torch.from_numpy(rs.randint(0, 256, size=shape).astype(np.uint8))
    return torch.from_numpy(rs.uniform(-0.6, 0.6, size=shape).astype(np.float32))


def grid(R, N, C, H, W, T, seed):
    """cells on the CPU for an R x N grid: kinds alternate, modes and group sizes cycle, counts run from 1 to T + 1
    (fewer than T: the last frame is held), switch_at is 0, in the middle or beyond T, the colours differ per cell, and
    from 3 cells on one is empty"""
    from rfn_hip import ops
    rs = np.random.RandomState(seed)
    cells, k = [], 0
    for r in range(R):
        row = []
        for i in range(N):
            k += 1
            if R * N >= 3 and k == 2:
                row.append(None)
                continue
            mode = ("frame", "mean", "spread")[k % 3]
            G = (1, 2, 5)[(k // 3) % 3]
            n = 1 + (k * 2) % (T + 1)
            shape = (n, C, H, W) if mode == "frame" else (n, G, C, H, W)
            row.append(ops.ClipCell(frames_of(rs, k % 2, shape), mode, gain=1 + (5 * k) % 16,
                                    switch_at=(0, T // 2, T + 3)[k % 3], before=(k, 160, 3 * k), after=(208, 2 * k, 255 - k)))
        cells.append(row)
    return cells


def on_gpu(cells):
    from rfn_hip import ops
    return [[None if c is None else ops.ClipCell(c.frames.cuda(), c.mode, c.gain, c.switch_at, c.before, c.after)
             for c in row] for row in cells]


def check(cells_cpu, cells_gpu, T, **kw):
    from rfn_hip import ops
    for scanlines in (False, True):
        want = compose_clip_ref(cells_cpu, T, bg=BG, scanlines=scanlines, **kw)
        got = ops.compose_clip(cells_gpu, T, bg=BG, scanlines=scanlines, **kw)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (scanlines, kw)


#        R, N, C, H, W, zoom, border, gutter, T: line lengths with every ragged store end, every value of the issue's lists
CASES = [(1, 1, 1, 1, 1, 1, 0, 0, 1), (1, 1, 3, 1, 1, 1, 1, 2, 3), (1, 2, 1, 5, 7, 2, 0, 2, 4), (2, 1, 3, 5, 7, 3, 2, 0, 3),
         (2, 3, 1, 9, 13, 1, 1, 2, 4), (3, 4, 3, 9, 13, 2, 2, 2, 3), (3, 4, 1, 5, 7, 3, 1, 0, 1), (2, 2, 3, 9, 13, 1, 0, 0, 4),
         (1, 3, 1, 5, 7, 1, 2, 2, 3), (3, 2, 3, 1, 1, 2, 0, 2, 4)]


@pytest.mark.parametrize("R,N,C,H,W,zoom,border,gutter,T", CASES)
def test_kernel_matches_restatement(R, N, C, H, W, zoom, border, gutter, T):
    from rfn_hip import ops
    cells = grid(R, N, C, H, W, T, seed=R * 100 + N * 10 + T)
    assert ops.clip_shape(R, N, H, W, zoom, border, gutter) == clip_shape(R, N, H, W, zoom, border, gutter)
    check(cells, on_gpu(cells), T, zoom=zoom, border=border, gutter=gutter)


@pytest.mark.parametrize("n_bits,preprocess_range", [(8, "0.5"), (5, "0.5"), (8, "1.0")])
def test_pixel_rule_beyond_the_clamp_ends_and_nan(n_bits, preprocess_range):
    from rfn_hip import ops
    rs = np.random.RandomState(n_bits)
    x = torch.from_numpy(rs.uniform(-1.5, 1.5, size=(2, 3, 1, 4, 6)).astype(np.float32))
    x[0, 0, 0, 0, :] = torch.tensor([float("nan"), -1e30, 1e30, float("inf"), -float("inf"), 0.4999])
    x[1, 1, 0, 1, 0] = float("nan")
    cells = [[ops.ClipCell(x[:, 0]), ops.ClipCell(x, "mean"), ops.ClipCell(x, "spread", gain=3)]]
    check(cells, on_gpu(cells), 2, n_bits=n_bits, preprocess_range=preprocess_range, zoom=2, border=1)
    b = to_bytes(x, n_bits, preprocess_range)
    assert b.min() == 0 and b.max() == 255 and b[0, 0, 0, 0, 0] == 0


def test_views_with_odd_strides():
    """p[0] of [B, T, ...], p[:, 0] of [T, B, ...] and p[:, :, b] of [n, G, B, ...]: nothing is copied, the other
    elements of the parents are NaN / 0x5A in the kernel's copies and are never shown"""
    from rfn_hip import ops
    rs = np.random.RandomState(3)
    C, H, W, T = 3, 5, 7, 3
    a = frames_of(rs, 1, (2, T, C, H, W))          # [B, T, ...]
    b = frames_of(rs, 0, (T, 3, C, H, W))          # [T, B, ...]
    c = frames_of(rs, 0, (T, 5, 4, C, H, W))       # [n, G, B, ...]
    d = frames_of(rs, 1, (T, 2, 3, C, H, W))
    views = [lambda p: p[0], lambda p: p[:, 0], lambda p: p[:, :, 2], lambda p: p[:, :, 1]]
    modes = ["frame", "frame", "mean", "spread"]
    cpu = [[ops.ClipCell(v(p), m, switch_at=1) for v, p, m in zip(views, (a, b, c, d), modes)]]
    gpu_parents = []
    for v, p in zip(views, (a, b, c, d)):
        big = torch.full(p.shape, float("nan") if p.dtype == torch.float32 else 0x5A, dtype=p.dtype).cuda()
        v(big).copy_(v(p))
        gpu_parents.append(big)
    gpu = [[ops.ClipCell(v(p), m, switch_at=1) for v, p, m in zip(views, gpu_parents, modes)]]
    assert not gpu[0][2].frames.is_contiguous() and gpu[0][2].frames.data_ptr() != gpu_parents[2].data_ptr()
    check(cpu, gpu, T, zoom=2, border=1)


@pytest.mark.parametrize("kind", [0, 1])
def test_the_largest_group(kind):
    from rfn_hip import ops
    G = ops.clip_limits()[0]
    assert G == 1024
    rs = np.random.RandomState(kind)
    x = frames_of(rs, kind, (2, G, 1, 2, 2))
    if kind == 1:   # the largest radicand: half the members 0, half 255, at the largest gain
        x[0, :G // 2, 0, 0, 0], x[0, G // 2:, 0, 0, 0] = 0, 255
    cells = [[ops.ClipCell(x, "mean"), ops.ClipCell(x, "spread", gain=16), ops.ClipCell(x, "spread", gain=1)]]
    check(cells, on_gpu(cells), 2, gutter=1)


def test_spread_of_equal_members_is_zero_and_a_wide_one_saturates():
    from rfn_hip import ops
    same = torch.full((1, 5, 1, 3, 3), 77, dtype=torch.uint8)
    wide = torch.zeros((1, 2, 1, 3, 3), dtype=torch.uint8)
    wide[0, 1] = 255
    cells = [[ops.ClipCell(same, "spread", gain=16), ops.ClipCell(wide, "spread", gain=2),
              ops.ClipCell(wide, "spread", gain=1)]]
    got = ops.compose_clip(on_gpu(cells), 1, gutter=0, bg=BG).cpu().numpy()
    assert got.shape == (1, 3, 9, 3)
    assert (got[0, :, 0:3] == 0).all() and (got[0, :, 3:6] == 255).all() and (got[0, :, 6:9] == 127).all()
    assert np.array_equal(got, compose_clip_ref(cells, 1, gutter=0, bg=BG))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_no_write_outside_out(offset):
    """out is a view at byte offset 1, 2 or 3 from an aligned address inside a 0xA5-filled allocation"""
    from rfn_hip import ops
    R, N, C, H, W, zoom, border, gutter, T = CASES[4]
    cells = grid(R, N, C, H, W, T, seed=offset)
    gpu = on_gpu(cells)
    Hs, Ws = clip_shape(R, N, H, W, zoom, border, gutter)
    for scanlines, shape in ((True, (T, Hs, 1 + 3 * Ws)), (False, (T, Hs, Ws, 3))):
        total, pad = int(np.prod(shape)), 1024 + offset
        guard = torch.full((pad + total + 1024,), 0xA5, dtype=torch.uint8, device="cuda")
        out = guard[pad:pad + total].view(shape)
        assert guard.data_ptr() % 4 == 0 and out.data_ptr() % 4 == offset
        ret = ops.compose_clip(gpu, T, zoom=zoom, border=border, gutter=gutter, bg=BG, scanlines=scanlines, out=out)
        assert ret.data_ptr() == out.data_ptr()
        g = guard.cpu()
        assert bool((g[:pad] == 0xA5).all()) and bool((g[pad + total:] == 0xA5).all())
        want = compose_clip_ref(cells, T, zoom=zoom, border=border, gutter=gutter, bg=BG, scanlines=scanlines)
        assert np.array_equal(g[pad:pad + total].view(shape).numpy(), want)


def test_same_bits_on_every_launch_and_stream():
    from rfn_hip import ops
    R, N, C, H, W, zoom, border, gutter, T = CASES[5]
    cells = grid(R, N, C, H, W, T, seed=9)
    gpu = on_gpu(cells)
    kw = dict(zoom=zoom, border=border, gutter=gutter, bg=BG, scanlines=True)
    a = ops.compose_clip(gpu, T, **kw)
    b = ops.compose_clip(gpu, T, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.compose_clip(gpu, T, **kw)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert np.array_equal(a.cpu().numpy(), compose_clip_ref(cells, T, **kw))


# ------------------------------------------------------------------------------------------------ the callers
def test_evaluator_plot_clips(tmp_path):
    from evaluation_metrics import Evaluator
    from rfn_hip import ops
    g = torch.Generator().manual_seed(5)
    pred = torch.randint(0, 256, (3, 2, 4, 3, 8, 8), generator=g, dtype=torch.uint8)    # [D, bs, T, C, H, W]
    true = torch.randint(0, 256, (2, 4, 3, 8, 8), generator=g, dtype=torch.uint8)
    solver = SimpleNamespace(model=None, args=Namespace(n_conditions=1), device=torch.device("cuda"),
                             path=str(tmp_path) + "/")
    ev = Evaluator(solver)
    path = ev.plot_clips(pred.cuda(), true, n=2, n_conditions=2, zoom=2, border=2, gain=3, delay_ms=80)
    assert path == str(tmp_path) + "/eval_folder/clips.png"
    w, h, plays, frames = parse_apng(open(path, "rb").read())
    assert (h, w) == clip_shape(2, 6, 8, 8, 2, 2, 2) and plays == 0 and len(frames) == 4
    cell = lambda fr, mode="frame": ops.ClipCell(fr, mode, gain=3, switch_at=2)
    layout = [[cell(true[k])] + [cell(pred[d, k]) for d in range(3)] +
              [cell(pred[:, k].transpose(0, 1), "mean"), cell(pred[:, k].transpose(0, 1), "spread")] for k in range(2)]
    want = compose_clip_ref(layout, 4, zoom=2, border=2)
    for t, (num, den, px) in enumerate(frames):
        assert (num, den) == (80, 1000)
        assert np.array_equal(px, want[t]), t
    # the ring is green on the given frames and red on the generated ones; the ground truth sits inside it
    assert frames[1][2][2, 2].tolist() == [0, 160, 0] and frames[2][2][2, 2].tolist() == [208, 0, 0]
    assert np.array_equal(frames[3][2][4:20:2, 4:20:2], true[0, 3].permute(1, 2, 0).numpy())
    # one draw without the draw dimension; n_conditions defaults to the run's
    path = ev.plot_clips(pred[0], true.cuda(), name="one", n=1)
    w, h, _, frames = parse_apng(open(path, "rb").read())
    assert (h, w) == clip_shape(1, 4, 8, 8, 2, 2, 2) and len(frames) == 4
    assert frames[0][2][2, 2].tolist() == [0, 160, 0] and frames[1][2][2, 2].tolist() == [208, 0, 0]
    x0 = 2 + 3 * (20 + 2)
    assert not frames[2][2][4:20, x0 + 2:x0 + 18].any(), "the spread of one draw is zero"
    assert sorted(os.listdir(str(tmp_path) + "/eval_folder")) == ["clips.png", "one.png"]
    with pytest.raises(ValueError, match="differ in shape"):
        ev.plot_clips(pred[:, :1].cuda(), true)
    with pytest.raises(ValueError, match="uint8 tensor"):
        ev.plot_clips(pred.float(), true)


def _tool():
    spec = importlib.util.spec_from_file_location("predict_clips", os.path.join(ROOT, "tools", "predict_clips.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _one_step_run(exp, model_name):
    """a checkpoint written after one Solver step on synthetic data (as tests/test_srnn_eval.py builds its run)"""
    rel = "/" + os.path.relpath(str(exp), os.getcwd()) + "/"
    torch.manual_seed(3)
    if model_name == "rfn.pt":
        import main_rfn
        from RFN.trainer import Solver
        s = Solver(main_rfn.build_parser().parse_args(_solver_argv("--synthetic_data --choose_data mnist --path %s" % rel)))
        s.build()
        s.model.train()
        s.train_step(next(iter(s.train_loader)).to(s.device))
        s.checkpoint("rfn.pt", 1, 0.0)
    else:
        import main_vrnn
        from VRNN.trainer import Solver
        s = Solver(main_vrnn.build_parser().parse_args(
            ("--synthetic_data --max_steps 1 --n_epochs 1 --batch_size 2 --n_frames 3 --image_size 32 --digit_size 12 "
             "--x_dim 2 1 32 32 --condition_dim 2 1 32 32 --h_dim 8 --z_dim 4 --n_logistics 3 --num_workers 0 "
             "--path " + rel).split()))
        s.build()
        s.train()
    assert os.path.isfile(str(exp / "model_folder" / model_name))


@pytest.mark.parametrize("model_name", ["rfn.pt", "vrnn.pt"])
def test_predict_clips_tool(tmp_path, capsys, model_name):
    """the tool end to end on a one-step synthetic run, for RFN and for a baseline the evaluation driver refuses"""
    from evaluation_metrics import eval_settings
    tool = _tool()
    if model_name != "rfn.pt":
        with pytest.raises(ValueError):
            eval_settings.solver_class(model_name)
    assert tool.solver_class(model_name).checkpoint_names[0] == model_name
    exp = tmp_path / "run"
    exp.mkdir()
    _one_step_run(exp, model_name)
    argv = ("--folder_path %s/ --experiment_names run --model_path %s --n_frames 5 --start_predictions 2 --draws 3 "
            "--show_draws 2 --sequences 2 --seed 4 --zoom 2 --delay_ms 60 --gain 4" % (tmp_path, model_name)).split()
    capsys.readouterr()
    paths = tool.main(tool.parse_args(argv))
    assert paths == [str(exp) + "/eval_folder/clips.png"] and capsys.readouterr().out.strip().endswith(paths[0])
    blob = open(paths[0], "rb").read()
    w, h, plays, frames = parse_apng(blob)
    Hc = 2 * 32 + 4
    assert (h, w) == clip_shape(2, 5, 32, 32, 2, 2, 2) == (2 * Hc + 6, 5 * Hc + 12)
    assert len(frames) == 5 and plays == 0 and all((num, den) == (60, 1000) for num, den, _ in frames)
    cell = lambda px, r, i: px[2 + r * (Hc + 2):2 + r * (Hc + 2) + Hc, 2 + i * (Hc + 2):2 + i * (Hc + 2) + Hc]
    for t, (_, _, px) in enumerate(frames):
        ring = [0, 160, 0] if t < 2 else [208, 0, 0]
        for r in range(2):
            for i in range(5):
                assert cell(px, r, i)[0, 0].tolist() == ring and cell(px, r, i)[-1, -1].tolist() == ring
            if t < 2:   # the given frames: every draw column and the mean show the ground truth, the spread is black
                for i in (1, 2, 3):
                    assert np.array_equal(cell(px, r, i), cell(px, r, 0)), (t, r, i)
                assert not cell(px, r, 4)[2:-2, 2:-2].any(), (t, r)
    tool.main(tool.parse_args(argv))
    assert open(paths[0], "rb").read() == blob, "the same seed gives the same file"
    assert [f for f in os.listdir(str(exp) + "/eval_folder") if f.endswith(".png")] == ["clips.png"]
