"""The linear-extrapolation baseline on the GPU (csrc/linear_extrap.hip, rfn_hip.ops.linear_extrap_loss /
linear_extrap_rollout / gauss_quality, AverageModel/, main_average.py) against float64 torch restatements of the
reference's expressions (averagemodel/averagemodel.py:65-113 and pytorch_msssim's Gaussian-window SSIM), written here.

Bounds (DESIGN.md section 26 records the worst error / bound ratios measured):
  prediction   per pixel (F + 4) 2^-24 (|b| + sum_f |W_f| |feat_f|), evaluated in float64: holds for any fp32 summation
               order of the F + 1 terms with once-rounded differences;
  loss, g_f    max(4 |g32 - g64|, 1e-5 A): g32 the torch float32 chain on the CPU, A the float64 mean of the summed
               magnitudes (|2 r feat_f|, |2 r|, r^2); 1e-5 is 168 fp32 roundings on that sum, above any fixed-order tree
               over these <= 2000 pixels;
  rollout      per frame max(4 max|roll32 - roll64|, 1e-6 max|roll64|);
  SSIM         max(4 |s32 - s64|, 2e-5), near-flat frames 1e-3 (fp32 cancellation of g*(X X) - mu^2 against C2 = 58.5);
               MSE 1e-5 relative; identical frames: SSIM within 1e-6 of 1, PSNR +inf.
Weights are W = e_{n-1} + 0.05 N(0, 1), bias = 0.01, so a rollout does not explode."""
import functools
import os
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24

# (B, T, start, n, C, H, W)
LOSS_SHAPES = [(3, 4, 1, 2, 1, 5, 7),      # 35 pixels (scalar tail), non-zero start, T > n + 1
               (2, 6, 0, 5, 3, 16, 20),    # the reference's n
               (1, 2, 0, 1, 1, 4, 4),      # n = 1: no differences, one thread's worth of work
               (2, 11, 0, 10, 1, 8, 8)]    # the frame limit
ROLLOUTS = [((2, 6, 0, 5, 3, 16, 20), 12),   # longer than the window: the last frames come from predictions alone
            ((3, 4, 1, 2, 1, 5, 7), 3)]


# ---- the reference's expressions as torch ops (any dtype, on the CPU)
def lagged_differences(x):
    """averagemodel.py:65-71"""
    length = x.shape[1]
    out = [x[:, 0:(length - k - 1)] - x[:, (k + 1):length] for k in range(0, length - 1)]
    return torch.cat(out, dim=1) if out else x[:, 0:0]


def features(x_use):
    f = torch.cat((x_use, lagged_differences(x_use)), dim=1)
    return f.view(*f.shape[0:2], -1)


def prediction(x_use, W, bias):
    """averagemodel.py:72-81, the channel count from the data"""
    p = torch.matmul(W, features(x_use)) + bias
    return p.view(x_use.shape[0], *x_use.shape[2:5])


def chain_loss(x, W, bias, n, start=0):
    """averagemodel.py:82-90"""
    return Fn.mse_loss(prediction(x[:, start:start + n], W, bias), x[:, start + n])


def chain_rollout(x, W, bias, n, P, start=0):
    """averagemodel.py:105-113"""
    x_use, out = x[:, start:start + n], []
    for _ in range(P):
        p = prediction(x_use, W, bias)
        x_use = torch.cat((x_use, p.unsqueeze(1)), dim=1)[:, 1:]
        out.append(p.unsqueeze(1))
    return torch.cat(out, dim=1)


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs and references of one shape, computed once"""
    B, T, start, n, C, H, W_ = shape
    g = torch.Generator().manual_seed(sum(p * q for p, q in zip(shape, (1, 3, 5, 7, 11, 13, 17))))
    F = n * (n + 1) // 2
    x = torch.rand(B, T, C, H, W_, generator=g)
    W = 0.05 * torch.randn(1, F, generator=g)
    W[0, n - 1] += 1.0
    bias = torch.full((1, 1), 0.01)
    c = {"x": x, "W": W, "bias": bias, "F": F}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        Wd, bd = W.clone().to(dt).requires_grad_(), bias.clone().to(dt).requires_grad_()
        loss = chain_loss(x.to(dt), Wd, bd, n, start)
        gW, gb = torch.autograd.grad(loss, (Wd, bd))
        c["g" + name] = torch.cat((loss.detach().view(1), gW.view(-1), gb.view(-1))).double()
    # the magnitudes A: mean r^2, mean |2 r feat_f|, mean |2 r|
    xd, Wd, bd = x.double(), W.double(), bias.double()
    feat = features(xd[:, start:start + n])                                   # [B, F, CHW]
    r = (torch.matmul(Wd, feat) + bd).view(B, -1) - xd[:, start + n].reshape(B, -1)
    c["A"] = torch.cat(((r * r).mean().view(1), (2 * r.unsqueeze(1) * feat).abs().mean((0, 2)), (2 * r).abs().mean().view(1)))
    # the per-pixel bound of one prediction
    mag = bd.abs() + torch.matmul(Wd.abs(), feat.abs())
    c["pred64"] = prediction(xd[:, start:start + n], Wd, bd)
    c["pred_bound"] = ((F + 4) * U24 * mag).view_as(c["pred64"])
    return c


def on_device(c):
    return c["x"].to(DEV), c["W"].to(DEV), c["bias"].to(DEV)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradients(shape):
    from rfn_hip import ops
    B, T, start, n, C, H, W_ = shape
    c = case(shape)
    x, W, bias = on_device(c)
    keep = x.clone()
    outs = []
    for _ in range(2):
        Wp, bp = W.clone().requires_grad_(), bias.clone().requires_grad_()
        loss = ops.linear_extrap_loss(x, Wp, bp, n, start)
        assert loss.shape == () and loss.requires_grad
        loss.backward()
        assert Wp.grad.shape == W.shape and bp.grad.shape == bias.shape
        outs.append(torch.cat((loss.detach().view(1), Wp.grad.view(-1), bp.grad.view(-1))))
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    assert torch.equal(x, keep)
    got = outs[0].cpu().double()
    err = (got - c["g64"]).abs()
    bound = torch.maximum(4 * (c["g32"] - c["g64"]).abs(), 1e-5 * c["A"])
    ratio = float((err / bound).max())
    print("loss+grad %s: worst error %.3e, error / bound %.3f (float32 torch error %.1e)"
          % (shape, float(err.max()), ratio, float((c["g32"] - c["g64"]).abs().max())))
    assert bool((err <= bound).all()), (err, bound)
    # the autograd path: an upstream factor 0.3 scales the unscaled gradients by one fp32 multiply
    Wp, bp = W.clone().requires_grad_(), bias.clone().requires_grad_()
    ops.linear_extrap_loss(x, Wp, bp, n, start).backward(torch.tensor(0.3, device=DEV))
    up = torch.tensor(0.3, device=DEV)
    assert torch.equal(Wp.grad.view(-1), outs[0][1:1 + c["F"]] * up)
    assert torch.equal(bp.grad.view(-1), outs[0][1 + c["F"]:] * up)
    # no gradient to x
    xg = x.clone().requires_grad_()
    ops.linear_extrap_loss(xg, W.clone().requires_grad_(), bias, n, start).backward()
    assert xg.grad is None


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prediction_per_pixel(shape):
    from rfn_hip import ops
    B, T, start, n, C, H, W_ = shape
    c = case(shape)
    x, W, bias = on_device(c)
    got = ops.linear_extrap_rollout(x, W, bias, n, 1, start)
    assert got.shape == (B, 1, C, H, W_)
    err = (got[:, 0].cpu().double() - c["pred64"]).abs()
    print("prediction %s: worst error %.3e, error / bound %.3f" % (shape, float(err.max()), float((err / c["pred_bound"]).max())))
    assert bool((err <= c["pred_bound"]).all())


@pytest.mark.parametrize("shape,P", ROLLOUTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "P%d" % v)
def test_rollout(shape, P):
    from rfn_hip import ops
    B, T, start, n, C, H, W_ = shape
    c = case(shape)
    x, W, bias = on_device(c)
    keep = x.clone()
    got = ops.linear_extrap_rollout(x, W, bias, n, P, start)
    again = ops.linear_extrap_rollout(x, W, bias, n, P, start)
    assert got.shape == (B, P, C, H, W_) and torch.equal(got, again) and torch.equal(x, keep)
    assert not got.requires_grad
    roll32 = chain_rollout(c["x"], c["W"], c["bias"], n, P, start).double()
    roll64 = chain_rollout(c["x"].double(), c["W"].double(), c["bias"].double(), n, P, start)
    err = (got.cpu().double() - roll64).abs()
    worst = 0.0
    for t in range(P):
        bound = max(4 * float((roll32[:, t] - roll64[:, t]).abs().max()), 1e-6 * float(roll64.abs().max()))
        worst = max(worst, float(err[:, t].max()) / bound)
        assert float(err[:, t].max()) <= bound, (t, float(err[:, t].max()), bound)
    print("rollout %s P=%d: worst error %.3e, error / bound %.3f" % (shape, P, float(err.max()), worst))
    # frame 0 obeys the per-pixel bound of one prediction
    assert bool((err[:, 0] <= c["pred_bound"]).all())
    # a window that is a view along T (x[:, start:]) is read in place and gives the same bits
    assert torch.equal(ops.linear_extrap_rollout(x[:, start:], W, bias, n, P), got)


# ---- Gaussian-window SSIM (pytorch_msssim.ssim with data_range 255) and the MSE as torch ops
def gauss_ref(X, Y, dtype):
    """(ssim [N], mse [N]) of float32 frames in [0, 1] taken as clamp(255 v, 0, 255), in `dtype` on their device"""
    X, Y = (torch.clamp(255 * v.to(dtype), 0, 255) for v in (X, Y))
    i = torch.arange(11, dtype=dtype, device=X.device)
    g = torch.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    C = X.shape[1]

    def filt(v):
        v = Fn.conv2d(v, g.view(1, 1, 11, 1).repeat(C, 1, 1, 1), groups=C)
        return Fn.conv2d(v, g.view(1, 1, 1, 11).repeat(C, 1, 1, 1), groups=C)

    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    mu1, mu2 = filt(X), filt(Y)
    s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s1 + s2 + C2))
    return smap.flatten(2).mean(-1).mean(1).double(), ((X - Y) ** 2).mean((1, 2, 3)).double()


GAUSS_SHAPES = [(3, 1, 12, 13),      # 2 x 3 valid outputs: a window or crop slip is O(0.1)
                (2, 3, 16, 20),
                (1, 1, 128, 128)]    # the size limit
GAUSS_KINDS = ["uniform", "smooth", "flat", "identical"]


@functools.lru_cache(maxsize=None)
def gauss_case(shape, kind):
    N, C, H, W_ = shape
    g = torch.Generator().manual_seed(100 * GAUSS_KINDS.index(kind) + N + 2 * C + H + W_)
    if kind == "flat":
        X = 200.0 / 255 + 3.0 / 255 * torch.rand(shape, generator=g)
        Y = X + torch.randn(shape, generator=g) / 255
    else:
        X = torch.rand(shape, generator=g)
        if kind == "smooth":
            X = Fn.avg_pool2d(Fn.pad(X, (2, 2, 2, 2), mode="replicate"), 5, stride=1)
        Y = X.clone() if kind == "identical" else X + torch.randn(shape, generator=g) * (20.0 / 255)
    s32, m32 = gauss_ref(X, Y, torch.float32)
    s64, m64 = gauss_ref(X, Y, torch.float64)
    return {"X": X, "Y": Y, "s32": s32, "s64": s64, "m64": m64}


@pytest.mark.parametrize("kind", GAUSS_KINDS)
@pytest.mark.parametrize("shape", GAUSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gauss_quality(shape, kind):
    from rfn_hip import ops
    c = gauss_case(shape, kind)
    X, Y = c["X"].to(DEV), c["Y"].to(DEV)
    kx, ky = X.clone(), Y.clone()
    ssim, psnr, mse = ops.gauss_quality(X, Y)
    again = ops.gauss_quality(X, Y)
    assert all(torch.equal(a, b) for a, b in zip((ssim, psnr, mse), again)), "two calls differ"
    assert torch.equal(X, kx) and torch.equal(Y, ky)
    assert ssim.shape == psnr.shape == mse.shape == (shape[0],)
    # PSNR is the formula applied to the MSE
    assert torch.equal(psnr, 10.0 * torch.log10(255.0 ** 2 / mse))
    s_err = (ssim.cpu().double() - c["s64"]).abs()
    s32_err = (c["s32"] - c["s64"]).abs()
    print("gauss_quality %s %s: SSIM error %.3e (float32 torch %.1e), MSE relative error %.3e"
          % (shape, kind, float(s_err.max()), float(s32_err.max()),
             float(((mse.cpu().double() - c["m64"]).abs() / c["m64"].clamp(min=1e-300)).max())))
    if kind == "identical":
        assert bool((s_err <= 1e-6).all()) and bool((c["s64"] - 1).abs().max() < 1e-12)
        assert bool((mse == 0).all()) and bool(torch.isinf(psnr).all()) and bool((psnr > 0).all())
        return
    floor = 1e-3 if kind == "flat" else 2e-5
    bound = torch.clamp(4 * s32_err, min=floor)
    assert bool((s_err <= bound).all()), (s_err, bound)
    if kind == "uniform":   # the clamp matters: scaled values leave [0, 255]
        assert float((255 * c["Y"]).max()) > 255 and float((255 * c["Y"]).min()) < 0
    if kind != "flat":
        assert bool(((mse.cpu().double() - c["m64"]).abs() <= 1e-5 * c["m64"]).all())
    assert bool(torch.isfinite(psnr).all())


def test_gauss_quality_reads_strided_inputs_and_other_scales():
    from rfn_hip import ops
    c = gauss_case((2, 3, 16, 20), "uniform")
    X, Y = c["X"].to(DEV), c["Y"].to(DEV)
    want = ops.gauss_quality(X, Y)
    # frames already on the 0..255 scale, clamped by the caller
    got = ops.gauss_quality(torch.clamp(255 * X, 0, 255), torch.clamp(255 * Y, 0, 255), scale=1.0)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    wide = torch.stack((X, Y), dim=1)            # [N, 2, C, H, W]: the two arguments are views
    got = ops.gauss_quality(wide[:, 0], wide[:, 1])
    assert all(torch.equal(a, b) for a, b in zip(want, got))


# ---- model and Solver
class RestatedModel(torch.nn.Module):
    """the reference's module, parameters only"""

    def __init__(self, n):
        super().__init__()
        self.W = torch.nn.Parameter(torch.zeros(1, n + (n - 1) * n // 2))
        self.bias = torch.nn.Parameter(torch.zeros(1, 1))


def test_model_state_dict_and_methods(tmp_path):
    from AverageModel import SimpleLinearModel
    shape = (2, 6, 0, 5, 3, 16, 20)
    c = case(shape)
    n = 5
    model = SimpleLinearModel(num_cond_frames=n).to(DEV)
    sd = model.state_dict()
    assert list(sd) == ["W", "bias"] and tuple(sd["W"].shape) == (1, 15) and tuple(sd["bias"].shape) == (1, 1)
    ref = RestatedModel(n)
    with torch.no_grad():
        ref.W.copy_(c["W"])
        ref.bias.copy_(c["bias"])
    torch.save(ref.state_dict(), str(tmp_path / "ref.pt"))
    model.load_state_dict(torch.load(str(tmp_path / "ref.pt"), weights_only=True))
    assert torch.equal(model.W.cpu(), c["W"]) and torch.equal(model.bias.cpu(), c["bias"])
    x = c["x"].to(DEV)
    from rfn_hip import ops
    loss = model(x)
    assert torch.equal(loss.detach(), ops.linear_extrap_loss(x, model.W, model.bias, n).detach())
    loss.backward()
    assert model.W.grad.shape == (1, 15) and model.bias.grad.shape == (1, 1)
    assert torch.equal(model.sample(x, 3), ops.linear_extrap_rollout(x, model.W, model.bias, n, 3))
    assert torch.equal(model.get_prediction(x[:, 0:n]), model.sample(x, 1)[:, 0])
    # the reference's metric methods on frames of the 0..255 scale
    X, Y = torch.clamp(255 * x[:, 0], 0, 255), torch.clamp(255 * x[:, 1], 0, 255)
    ssim, psnr, _ = ops.gauss_quality(x[:, 0], x[:, 1])
    assert torch.equal(model.ssim_val(X, Y), ssim.mean()) and torch.equal(model.PSNRbatch(X, Y), psnr.mean())
    # get_lagged_differences is the torch expression
    assert torch.equal(model.get_lagged_differences(c["x"]), lagged_differences(c["x"]))


def solver_args(path, extra=()):
    import main_average
    return main_average.build_parser().parse_args(
        ["--synthetic_data", "--batch_size", "4", "--n_conditions", "2", "--x_dim", "4", "1", "16", "16", "--image_size",
         "16", "--digit_size", "6", "--num_workers", "0", "--path", path] + list(extra))


def run_solver(path, steps):
    from AverageModel.trainer import Solver
    torch.manual_seed(11)
    solver = Solver(solver_args(path, ["--max_steps", str(steps), "--n_frames", "6"]))
    solver.build()
    fixed = solver.batch(next(iter(solver.test_loader)))
    with torch.no_grad():
        before = float(solver.model(fixed))
    torch.manual_seed(12)
    solver.train()
    with torch.no_grad():
        after = float(solver.model(fixed))
    return solver, before, after


def test_solver_trains_reproducibly_and_the_checkpoint_round_trips(tmp_path, monkeypatch):
    from AverageModel.trainer import Solver
    monkeypatch.chdir(tmp_path)
    a, before, after = run_solver("/a/", 30)
    b, before_b, after_b = run_solver("/b/", 30)
    assert a.counter == 30 and len(a.losses) == 30
    print("solver: loss on a fixed test batch %.6f -> %.6f; first / last step loss %.6f / %.6f"
          % (before, after, a.losses[0], a.losses[-1]))
    # "lower than they start" is read on one fixed test batch: the per-step losses are those of 30 different batches of
    # four sequences, whose spread (0.06 .. 0.12 here) exceeds what 30 steps at lr 1e-3 can gain
    assert after < before
    assert (before, after) == (before_b, after_b) and a.losses == b.losses
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)
    # the train loader yields n + 1 frames, the test loader --n_frames
    assert next(iter(a.train_loader)).shape == (4, 3, 1, 16, 16) and next(iter(a.test_loader)).shape == (4, 6, 1, 16, 16)
    # average.pt
    ckpt = Solver.read_checkpoint(str(tmp_path / "a" / "model_folder" / "average.pt"))
    assert {"model_state_dict", "args"} <= set(ckpt)
    assert vars(ckpt["args"]) == vars(a.args)
    fresh = Solver(ckpt["args"])
    fresh.build()
    fresh.load(ckpt)
    for (k, p), q in zip(a.model.state_dict().items(), fresh.model.state_dict().values()):
        assert torch.equal(p, q) and q.is_cuda, k


def test_driver_end_to_end(tmp_path, monkeypatch):
    import main_average
    from AverageModel.trainer import Solver
    from evaluation_metrics.error_metrics import Evaluator
    from rfn_hip import ops
    monkeypatch.chdir(tmp_path)
    seen = []
    batch = Solver.batch
    monkeypatch.setattr(Solver, "batch", lambda self, image: seen.append(batch(self, image)) or seen[-1])
    torch.manual_seed(5)
    args = solver_args("/run/", ["--n_frames", "6", "--n_predictions", "3", "--max_steps", "5", "--max_batches", "2"])
    solver = main_average.main(args)
    assert solver.counter == 5
    folder = str(tmp_path / "run" / "eval_folder")
    ref = torch.load(os.path.join(folder, "SSIM_PSNR_bair_averagemodel_trained_on_3_frames.pt"), weights_only=True)
    assert set(ref) == {"SSIM_values", "PSNR_values", "SSIM_values_mean", "PSNR_values_mean"}
    assert ref["SSIM_values"].shape == ref["PSNR_values"].shape == (2, 3)
    assert ref["SSIM_values_mean"].shape == ref["PSNR_values_mean"].shape == (3,)
    assert torch.equal(ref["SSIM_values_mean"], ref["SSIM_values"].mean(0))
    tests = [t for t in seen if t.shape[1] == 6]
    assert len(seen) == 5 + 2 and len(tests) == 2
    n, P = 2, 3
    for b, image in enumerate(tests):
        pred = ops.linear_extrap_rollout(image, solver.model.W, solver.model.bias, n, P)
        for i in range(P):
            ssim, psnr, _ = ops.gauss_quality(pred[:, i], image[:, n + i])
            assert abs(float(ssim.mean()) - float(ref["SSIM_values"][b, i])) <= 1e-6
            assert abs(float(psnr.mean()) - float(ref["PSNR_values"][b, i])) <= 1e-4
    d = torch.load(os.path.join(folder, "evaluations.pt"), map_location="cpu", weights_only=True)
    from evaluation_metrics.eval_settings import eval_dict
    assert set(d) == set(eval_dict((None,) * 10, None))
    for k in ("SSIM", "PSNR", "MSE"):
        assert d[k + "_values"].shape == (8, 3)
    for k in ("SSIM", "PSNR"):
        assert torch.equal(d[k + "_std_mean"], d[k + "_values"])
    assert all(d[k] is None for k in ("LPIPS_values", "LPIPS_std_mean", "temperature", "BPD", "DKL", "RECON"))
    # the Evaluator's definitions: frame_quality on the uint8 frames
    image = tests[0]
    pred = ops.linear_extrap_rollout(image, solver.model.W, solver.model.bias, n, P)
    mse8, psnr8, ssim8 = ops.frame_quality(torch.clamp(255 * image[:, n:n + P], 0, 255).byte(),
                                           torch.clamp(255 * pred, 0, 255).byte())
    assert torch.equal(d["SSIM_values"][:4], ssim8.cpu()) and torch.equal(d["MSE_values"][:4], mse8.cpu())
    # the curve figures draw it
    ev = Evaluator(Namespace(model=None, args=Namespace(), device=torch.device(DEV)),
                   settings=Namespace(n_conditions=2, n_trained=3))
    paths = ev._curve_figures([("linear", d)], str(tmp_path / "figs"), "")
    assert len(paths) == 3
    for p in paths:
        assert p.endswith(".png") and os.path.getsize(p) > 0
    # --load_model evaluates the saved weights: the same figures again
    torch.manual_seed(5)
    again = main_average.main(solver_args("/run/", ["--n_frames", "6", "--n_predictions", "3", "--max_batches", "2",
                                                    "--load_model"]))
    assert again.counter == 0
    for p, q in zip(solver.model.parameters(), again.model.parameters()):
        assert torch.equal(p, q)
