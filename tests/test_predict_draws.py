"""GPU tests of RFN.predict_draws (n_draws draws of every sequence as one batch, addressed noise from
rfn_hip.ops.keyed_normal) and of the Evaluator's draws_per_pass path built on it: equality with the verified
predict(draws=...) path fed the same numbers, independence of how the draws are batched, the shape-keyed graph cache,
best-of-N against the restatement of tests/test_frame_metrics_host.py, the sample sheets, and LPIPS in the new path."""
import os
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_frame_metrics_host import ref_frame_quality
from tests.test_lpips_host import make_state
from tests.test_sheet_host import decode_png

pytestmark = pytest.mark.gpu


def close(a, b, rtol=1e-4, atol=1e-5):
    """tests/test_hip_modules.py close(): |a-b| <= atol' + rtol*|b| with atol' scaled by the tensor's magnitude (fp32
    results of different summation orders agree norm-wise) -- the project's "equal up to summation order" in generation"""
    b = b.float()
    scale = float(b.abs().max()) if b.numel() else 0.0
    torch.testing.assert_close(a.detach().cpu(), b.detach().cpu(), rtol=rtol, atol=atol + rtol * scale)


def _close64(a, b, rtol=1e-6, atol=0.0):
    a, b = a.double(), b.double()
    inf = torch.isinf(b)
    assert torch.equal(torch.isinf(a), inf)
    assert bool(((a[~inf] - b[~inf]).abs() <= atol + rtol * b[~inf].abs()).all()), (a - b).abs().max()


@pytest.fixture(scope="module")
def tiny():
    """the tiny model of __graft_entry__._tiny_args() after its data dependent init, in eval mode, and a batch"""
    import __graft_entry__ as ge
    from RFN import RFN
    args = ge._tiny_args()
    torch.manual_seed(5)
    m = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(args.batch_size, 5, *args.x_dim[1:], generator=g) - 0.5).cuda()
    m.loss(x, 0)
    m.eval()
    return m, x


def _graph_mode(monkeypatch, graph):
    import rfn_hip
    if graph and not rfn_hip.graph_capture_safe():
        pytest.skip("hipGraph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before the HIP runtime starts")
    monkeypatch.setenv("RFN_GEN_GRAPH", "1" if graph else "0")


def _draw_list(m, B, n_predictions, n_conditions, seed, draw, first_seq=0):
    """the `draws` list of RFN.predict for one draw id, from ops.keyed_normal at predict_draws' addresses"""
    from rfn_hip import ops
    z = tuple(m.z_0.shape[1:])
    draws = []
    for i in range(1, n_conditions):
        draws += ops.keyed_normal([z, z], B, 1, seed, i, first_seq, draw, device="cuda")
    gen = [tuple(sh[1:]) for sh in m._gen_eps_shapes(B)]
    for i in range(n_predictions):
        out = ops.keyed_normal([gen[0], None] + gen[1:], B, 1, seed, n_conditions + i, first_seq, draw, device="cuda")
        draws += [t for t in out if t is not None]
    return draws


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_equal_to_predict_with_the_same_noise(tiny, monkeypatch, graph):
    _graph_mode(monkeypatch, graph)
    m, x = tiny
    B = x.shape[0]
    true_x, pd = m.predict_draws(x, 3, 2, n_draws=3, seed=9)
    assert pd.device.type == "cpu" and tuple(pd.shape) == (3, 3, B) + tuple(x.shape[2:])
    assert tuple(true_x.shape) == (2, B) + tuple(x.shape[2:]) and true_x.device.type == "cpu"
    dev = m._predict_draws_device(x, 3, 2, 3, 9)[1]
    assert dev.is_cuda and torch.equal(dev.cpu(), pd)
    for r in range(3):
        tx, ref = m.predict(x, 3, 2, draws=_draw_list(m, B, 3, 2, 9, r))
        assert torch.equal(tx, true_x)
        close(pd[:, r], ref)
    # the draws differ from one another
    assert float((pd[:, 0] - pd[:, 1]).abs().max()) > 1e-3


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_independent_of_batching(tiny, monkeypatch, graph):
    _graph_mode(monkeypatch, graph)
    m, x = tiny
    _, whole = m.predict_draws(x, 3, 2, n_draws=4, seed=9)
    for r in range(4):
        _, one = m.predict_draws(x, 3, 2, n_draws=1, seed=9, first_draw=r)
        close(one[:, 0], whole[:, r])
    for h in range(2):
        _, two = m.predict_draws(x, 3, 2, n_draws=2, seed=9, first_draw=2 * h)
        close(two, whole[:, 2 * h:2 * h + 2])
    # first_seq shifts the noise; a sequence keeps its noise wherever it sits in the batch
    _, moved = m.predict_draws(x, 3, 2, n_draws=4, seed=9, first_seq=100)
    assert float((moved - whole).abs().max()) > 1e-3
    _, other_seed = m.predict_draws(x, 3, 2, n_draws=4, seed=10)
    assert float((other_seed - whole).abs().max()) > 1e-3
    # same arguments: the same bits, whatever torch's generator holds
    torch.manual_seed(123)
    _, again = m.predict_draws(x, 3, 2, n_draws=4, seed=9)
    assert torch.equal(again, whole)


def test_generator_untouched_and_training_mode_raises(tiny):
    m, x = tiny
    torch.manual_seed(77)
    before = torch.cuda.get_rng_state().clone()
    m.predict_draws(x, 2, 2, n_draws=2, seed=1)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            m.predict_draws(x, 2, 2, n_draws=2, seed=1)
    finally:
        m.eval()
    with pytest.raises(ValueError, match="n_draws"):
        m.predict_draws(x, 2, 2, n_draws=0, seed=1)


def test_graphs_are_kept_per_shape(tiny, monkeypatch):
    """predict (batch B), predict_draws (batch 3 B), predict at unchanged weights: at most two graph builds"""
    monkeypatch.setenv("RFN_GEN_GRAPH", "1")
    m, x = tiny
    before = getattr(m, "_gen_graph_builds", 0)
    m.predict(x, 2, 2)
    m.predict_draws(x, 2, 2, n_draws=3, seed=4)
    m.predict(x, 2, 2)
    m.predict_draws(x, 2, 2, n_draws=3, seed=4)
    assert getattr(m, "_gen_graph_builds", 0) - before <= 2
    import rfn_hip
    if rfn_hip.graph_capture_safe():
        assert m._gen_graph is not None and len(m._gen_graphs) >= 2


# ------------------------------------------------------------------------------------------------ the Evaluator
def _tiny_solver_args(B=2):
    """the tiny solver configuration of tests/test_frame_metrics.py (_tiny_solver_args)"""
    import __graft_entry__ as ge
    args = ge._tiny_args()
    args.batch_size = B
    args.x_dim = [B, 1, 16, 16]
    args.condition_dim = [B, 1, 16, 16]
    for k, v in dict(n_bits=8, n_epochs=1, learning_rate=1e-3, verbose=False, path="/eval_tmp/", patience_lr=1,
                     factor_lr=0.5, min_lr=0.0, patience_es=1, beta_max=0.5, beta_min=0.5, beta_steps=10,
                     choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=16,
                     preprocess_range="0.5", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                     n_conditions=2, scheduler_type="linear", use_validation_set=False).items():
        setattr(args, k, v)
    return args


B_, T_, START, R_ = 2, 6, 2, 3


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    from RFN import RFN
    from RFN.trainer import Solver
    args = _tiny_solver_args()
    torch.manual_seed(3)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.path = str(tmp_path_factory.mktemp("eval")) + "/"
    s.model = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(8)
    batches = [torch.rand(B_, T_, 1, 16, 16, generator=g) for _ in range(3)]
    with torch.no_grad():
        s.model.loss(s.preprocess(batches[0][:, :args.n_frames].cuda()), 0)   # data dependent init
    return s, args, batches


def _run(s, args, batches, **extra):
    """get_eval_values with draws_per_pass = 2 and spies: the draws of the padded last pass that lie beyond `resample`
    are replaced by the ground truth (a perfect score) before the Evaluator sees them -- they must not count"""
    from evaluation_metrics import Evaluator
    settings = Namespace(n_frames=T_, start_predictions=START, resample=R_, n_trained=args.n_frames, draws_per_pass=2,
                         seed=21, **extra)
    ev = Evaluator(s, settings=settings)
    seen, losses = [], []
    plain_draws, plain_loss = s.model._predict_draws_device, s.model.loss

    def draws_spy(image, n_pred, n_cond, P, seed, first_seq=0, first_draw=0):
        tx, pr = plain_draws(image, n_pred, n_cond, P, seed, first_seq=first_seq, first_draw=first_draw)
        assert pr.is_cuda and tuple(pr.shape) == (n_pred, P, image.shape[0]) + tuple(image.shape[2:])
        pr = pr.clone()
        for d in range(P):
            if first_draw + d >= R_:
                pr[:, d] = image[:, n_cond:n_cond + n_pred].transpose(0, 1)
        seen.append((P, seed, first_seq, first_draw, pr.clone()))
        return tx, pr

    def loss_spy(*a, **k):
        out = plain_loss(*a, **k)
        losses.append((out[1].detach().clone(), out[2].detach().clone(), tuple(a[0].shape)))
        return out

    s.model._predict_draws_device, s.model.loss = draws_spy, loss_spy
    try:
        out = ev.get_eval_values("rfn.pt", loader=batches, max_batches=2)
    finally:
        del s.model._predict_draws_device, s.model.loss
    return ev, out, seen, losses


@pytest.fixture(scope="module")
def evaluated(solver):
    s, args, batches = solver
    return _run(s, args, batches, debug_plot=True)


def _expected(s, batches, seen):
    """best-of-N over draws 0..R-1 in ascending draw id from the predictions the Evaluator saw, by the restatement;
    also the draw that holds every sequence's best time-mean SSIM"""
    exp = {k: [] for k in ("mse", "psnr", "ssim", "ssim_std", "psnr_std", "best_draw")}
    quirk_seen = False
    for bi in range(2):
        gt = s.preprocess(s.preprocess(batches[bi].cuda()), reverse=True)[:, START:].cpu().numpy()
        passes = [e for e in seen if e[2] == bi * B_]
        assert [e[3] for e in passes] == [0, 2] and all(e[0] == 2 and e[1] == 21 for e in passes)
        draws = []
        for r in range(R_):
            pr = passes[r // 2][4][:, r % 2]
            pred = s.preprocess(pr, reverse=True).permute(1, 0, 2, 3, 4).cpu().numpy()
            assert pred.shape == gt.shape
            draws.append(ref_frame_quality(gt, pred))   # (mse, psnr, ssim) [B, n_pred] float64
        for m in range(3):   # the selection compares time-means: no near-ties between draws
            means = np.stack([d[m].mean(-1) for d in draws])
            for i in range(R_):
                for j in range(i):
                    assert (np.abs(means[i] - means[j]) >= 1e-4).all(), (m, means)
        best = [draws[0][m].copy() for m in range(3)]
        best_draw = np.zeros(B_, dtype=np.int64)
        for r in range(1, R_):
            for m, better in ((0, lambda cur, new: cur > new), (1, lambda cur, new: cur < new),
                              (2, lambda cur, new: cur < new)):
                sel = better(best[m].mean(-1), draws[r][m].mean(-1))
                best[m][sel] = draws[r][m][sel]
                if m == 2:
                    best_draw[sel] = r
        exp["mse"].append(best[0])
        exp["psnr"].append(best[1])
        exp["ssim"].append(best[2])
        exp["ssim_std"].append((best[2] + sum(d[2] for d in draws[1:])) / R_)
        exp["psnr_std"].append((best[1] + sum(d[1] for d in draws[1:])) / R_)
        exp["best_draw"].append(best_draw)
        quirk_seen = quirk_seen or not np.allclose(exp["ssim_std"][-1], sum(d[2] for d in draws) / R_, rtol=0, atol=1e-6)
    return {k: torch.from_numpy(np.concatenate(v)) for k, v in exp.items()}, quirk_seen


def test_evaluator_best_of_n_with_batched_draws(solver, evaluated):
    s, args, batches = solver
    ev, out, seen, losses = evaluated
    mse_v, psnr_v, ssim_v, lpips_v, bpd, dkl, recon, ssim_std, psnr_std, lpips_std = out
    assert len(seen) == 2 * 2          # ceil(3 / 2) passes per batch
    assert len(losses) == 2            # model.loss once per batch
    assert lpips_v is None and lpips_std is None
    n_pred = T_ - START
    for t in (mse_v, psnr_v, ssim_v, ssim_std, psnr_std):
        assert tuple(t.shape) == (2 * B_, n_pred) and t.dtype == torch.float32 and t.device.type == "cpu"
    exp, quirk_seen = _expected(s, batches, seen)
    _close64(mse_v, exp["mse"])
    _close64(psnr_v, exp["psnr"])
    _close64(ssim_v, exp["ssim"], rtol=0.0, atol=1e-6)
    _close64(psnr_std, exp["psnr_std"])
    _close64(ssim_std, exp["ssim_std"], rtol=0.0, atol=1e-6)
    # the padded draw (ground truth, a perfect score) did not count
    assert bool(torch.isfinite(psnr_v).all()) and float(ssim_v.max()) < 1.0
    assert quirk_seen
    want = []
    for kl, nll, shp in losses:
        assert shp == (B_, args.n_frames, 1, 16, 16)
        want.append(ev.compute_loss(nll=nll, kl=kl, dims=shp[2:], t=shp[1] - 1))
    for k, got in enumerate((bpd, dkl, recon)):
        assert torch.equal(got, torch.FloatTensor([w[k] for w in want])), (k, got, want)
    # the best prediction of every sequence by SSIM stays on the device
    bp = ev.best_preds_ssim
    assert bp.is_cuda and bp.dtype == torch.uint8 and tuple(bp.shape) == (2 * B_, n_pred, 1, 16, 16)
    for i in range(2 * B_):
        bi, b = divmod(i, B_)
        r = int(exp["best_draw"][i])
        pr = [e for e in seen if e[2] == bi * B_][r // 2][4][:, r % 2, b]
        assert torch.equal(bp[i], s.preprocess(pr, reverse=True))


def test_evaluator_is_reproducible(solver, evaluated):
    """the same settings twice: an identical tuple, whatever torch's generator did in between (the loss figures are one
    stochastic evaluation per batch from torch's generator: compared after the same manual seed)"""
    s, args, batches = solver
    torch.manual_seed(1)
    a = _run(s, args, batches)[1]
    torch.randn(100, device="cuda")
    torch.manual_seed(2)
    b = _run(s, args, batches)[1]
    for k in (0, 1, 2, 7, 8):
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], evaluated[1][k]), k
    torch.manual_seed(1)
    c = _run(s, args, batches)[1]
    for x, y in zip(a, c):
        assert (x is None and y is None) or torch.equal(x, y)


def test_evaluator_debug_sheets(solver, evaluated):
    from rfn_hip import ops
    s, args, batches = solver
    ev, out, seen, _ = evaluated
    folder = s.path + "eval_folder/"
    n_pred = T_ - START
    shapes = {"random_samples_ssim": ops.sheet_shape(2 * B_, n_pred, 16, 16, 2),       # the last batch's B sequences
              "best_samples": ops.sheet_shape(2 * 4, n_pred, 16, 16, 2),               # min(5, 4 sequences)
              "worst_samples": ops.sheet_shape(2 * 4, n_pred, 16, 16, 2)}
    px = {}
    for name, (Hs, Ws) in shapes.items():
        assert os.path.isfile(folder + name + ".png"), name
        (w, h), px[name] = decode_png(open(folder + name + ".png", "rb").read())
        assert (h, w) == (Hs, Ws), name
    # the first row pair of best_samples: ground truth and best prediction of the sequence with the highest time-mean SSIM
    top = int(torch.argsort(out[2].mean(-1), descending=True)[0])
    bi, b = divmod(top, B_)
    gt = s.preprocess(s.preprocess(batches[bi].cuda()), reverse=True)[b, START:].cpu()
    pred = ev.best_preds_ssim[top].cpu()
    sheet = np.asarray(px["best_samples"])
    for row, frames in enumerate((gt, pred)):
        for i in range(n_pred):
            y0, x0 = 2 + row * 18, 2 + i * 18
            cell = sheet[y0:y0 + 16, x0:x0 + 16]
            assert np.array_equal(cell, frames[i, 0].numpy()[:, :, None].repeat(3, 2)), (row, i)
    # worst_samples ends with the sequence of the lowest time-mean SSIM
    low = int(torch.argsort(out[2].mean(-1), descending=True)[-1])
    sheet = np.asarray(px["worst_samples"])
    cell = sheet[2 + 7 * 18:2 + 7 * 18 + 16, 2:18]
    assert np.array_equal(cell, ev.best_preds_ssim[low, 0, 0].cpu().numpy()[:, :, None].repeat(3, 2))


def test_unset_draws_per_pass_draws_from_torchs_generator(solver):
    from evaluation_metrics import Evaluator
    s, args, batches = solver
    ev = Evaluator(s, settings=Namespace(n_frames=T_, start_predictions=START, resample=1, n_trained=args.n_frames))
    assert ev.draws_per_pass is None
    seen = []
    plain = s.model.predict

    def predict_spy(*a, **k):
        out = plain(*a, **k)
        seen.append(out[1].clone())
        return out

    def no_draws(*a, **k):
        raise AssertionError("the sequential path must not call _predict_draws_device")

    s.model.predict, s.model._predict_draws_device = predict_spy, no_draws
    try:
        torch.manual_seed(13)
        ev.get_eval_values("rfn.pt", loader=batches, max_batches=1)
    finally:
        del s.model.predict, s.model._predict_draws_device
    assert len(seen) == 1
    torch.manual_seed(13)
    s.model.eval()
    _, direct = s.model.predict(s.preprocess(batches[0].cuda()), T_ - START, START)
    close(seen[0], direct)


# ------------------------------------------------------------------------------------------------ LPIPS in the new path
def _preprocess(x, reverse=False):
    """the solver's 8-bit preprocess on grey levels 0..255 (tests/test_lpips.py)"""
    if not reverse:
        return x / 256 - 0.5
    return torch.clamp(torch.floor((x + 0.5) * 256), 0, 255).byte()


def test_lpips_with_batched_draws(tmp_path, monkeypatch):
    """one batch of B = 3 sequences, 2 conditioning + 2 predicted frames of 1 x 32 x 32, resample = 2 in one pass of
    P = 2 (a stub model hands out prepared predictions: LPIPS needs 31 x 31 frames at least): the values equal
    ops.lpips_alex applied draw by draw; one trunk pass for the ground truth, one for the P*B*T predicted frames"""
    from evaluation_metrics import Evaluator
    from rfn_hip import ops
    from tests.test_lpips import A, R
    alex, lin = make_state(0)
    torch.save(alex, tmp_path / "alexnet-owt-test.pth")
    torch.save(lin, tmp_path / "alex.pth")
    B, T, start, P = 3, 4, 2, 2
    g = torch.Generator().manual_seed(31)
    batch = torch.randint(0, 256, (B, T, 1, 32, 32), generator=g).float()
    amp = torch.tensor([[40, 10, 25], [10, 25, 40]])
    gt = batch[:, start:]
    preds = []
    for r in range(P):
        noise = (torch.rand(gt.shape, generator=g) * 2 - 1) * amp[r].view(B, 1, 1, 1, 1)
        preds.append(_preprocess((gt + noise).round().clamp(0, 255)).permute(1, 0, 2, 3, 4))   # [n_pred, B, C, H, W]
    stacked = torch.stack(preds, 1).contiguous().cuda()                                          # [n_pred, P, B, ...]
    calls = {"draws": [], "loss": 0}

    class Model(object):
        def eval(self):
            return self

        def _predict_draws_device(self, image, n_pred, n_cond, n_draws, seed, first_seq=0, first_draw=0):
            calls["draws"].append((n_pred, n_cond, n_draws, seed, first_seq, first_draw))
            return None, stacked

        def loss(self, image, _):
            calls["loss"] += 1
            return None, torch.tensor(1.0), torch.tensor(2.0)

    solver = SimpleNamespace(model=Model(), args=SimpleNamespace(n_frames=T, n_conditions=start, choose_data="mnist"),
                             device=torch.device("cuda"), preprocess=_preprocess)
    ev = Evaluator(solver, settings=SimpleNamespace(n_frames=T, start_predictions=start, resample=2, n_trained=T,
                                                    draws_per_pass=P, seed=5, lpips_weights=str(tmp_path)))
    trunk_calls = []
    plain_features = ops.lpips_alex_features

    def features_spy(w, frames, **k):
        trunk_calls.append(tuple(frames.shape))
        return plain_features(w, frames, **k)

    monkeypatch.setattr(ops, "lpips_alex_features", features_spy)
    out = ev.get_eval_values("rfn.pt", loader=[batch])
    monkeypatch.setattr(ops, "lpips_alex_features", plain_features)
    assert calls == {"draws": [(T - start, start, P, 5, 0, 0)], "loss": 1}
    assert trunk_calls == [(B, T - start, 1, 32, 32), (P, B, T - start, 1, 32, 32)]
    lpips_v, lpips_std = out[3], out[9]
    for t in (lpips_v, lpips_std):
        assert tuple(t.shape) == (B, T - start) and t.dtype == torch.float32 and t.device.type == "cpu"
    w = ops.lpips_alex_load(str(tmp_path), "cuda")
    gt_u8 = gt.to(torch.uint8).cuda()
    draws = [ops.lpips_alex(w, _preprocess(stacked[:, r], reverse=True).permute(1, 0, 2, 3, 4).contiguous(), gt_u8)
             .cpu().double() for r in range(P)]
    assert bool(((draws[0].mean(-1) - draws[1].mean(-1)).abs() >= 1e-4).all())
    best = draws[0].clone()
    sel = best.mean(-1) > draws[1].mean(-1)
    assert bool(sel.any()) and not bool(sel.all())
    best[sel] = draws[1][sel]
    mean = (best + draws[1]) / 2          # draw 0 of the mean over draws is the best-so-far tensor
    assert bool(((lpips_v.double() - best).abs() <= A + R * best).all()), (lpips_v, best)
    assert bool(((lpips_std.double() - mean).abs() <= A + R * mean).all()), (lpips_std, mean)
