"""GPU tests of the frame-quality metrics: rfn_frame_quality_u8 through rfn_hip.ops.frame_quality against the numpy
restatement of skimage 0.17.2's SSIM / PSNR (tests/test_frame_metrics_host.py), Evaluator.eval_seq against a
restatement of the reference's per-frame loop (error_metrics.py:154-171), and Evaluator.get_eval_values (:419-598:
best-of-N over resampled predictions) recomputed from the predictions and losses it saw."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.test_frame_metrics_host import ref_frame_quality, ref_ssim_psnr_channel

pytestmark = pytest.mark.gpu


def _pair(N, C, H, W, seed):
    """uint8 frames a and a noisy copy b (SSIM well inside (0, 1)), plus one unrelated frame pair every fourth frame"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 256, (N, C, H, W), generator=g, dtype=torch.int64)
    noise = torch.randint(-48, 49, (N, C, H, W), generator=g)
    b = (a + noise).clamp(0, 255)
    b[::4] = torch.randint(0, 256, b[::4].shape, generator=g)
    return a.to(torch.uint8), b.to(torch.uint8)


def _check(got, a, b):
    """kernel (mse, psnr, ssim) against the restatement: SSIM |d| <= 1e-6, PSNR and MSE relative 1e-6, infinities
    exactly where expected"""
    mse, psnr, ssim = (t.cpu().double().numpy() for t in got)
    rm, rp, rs = ref_frame_quality(a.cpu().numpy(), b.cpu().numpy())
    assert mse.shape == rm.shape and psnr.shape == rp.shape and ssim.shape == rs.shape
    assert np.abs(ssim - rs).max(initial=0) <= 1e-6, np.abs(ssim - rs).max()
    assert (np.abs(mse - rm) <= 1e-6 * np.abs(rm)).all(), np.abs(mse - rm).max()
    inf = np.isinf(rp)
    assert (np.isinf(psnr) == inf).all() and (psnr[inf] > 0).all()
    assert (np.abs(psnr[~inf] - rp[~inf]) <= 1e-6 * np.abs(rp[~inf])).all()


@pytest.mark.parametrize("N,C,H,W", [(1, 1, 7, 7), (5, 3, 7, 7), (17, 1, 16, 16), (9, 3, 16, 16), (33, 1, 64, 64),
                                     (12, 3, 64, 64), (7, 1, 37, 53), (6, 3, 37, 53), (2, 1, 256, 256),
                                     (1, 3, 256, 256), (3, 2, 41, 300), (1000, 1, 16, 16), (320, 3, 64, 64)])
def test_frame_quality_vs_restatement(N, C, H, W):
    from rfn_hip import ops
    a, b = _pair(N, C, H, W, seed=N * 1000 + C * 100 + H + W)
    _check(ops.frame_quality(a.cuda(), b.cuda()), a, b)


def test_frame_quality_edge_cases():
    from rfn_hip import ops
    a, b = _pair(6, 3, 16, 16, seed=5)
    # identical frames: mse 0, psnr +inf, ssim 1
    mse, psnr, ssim = ops.frame_quality(a.cuda(), a.cuda())
    assert (mse.cpu() == 0).all() and torch.isinf(psnr.cpu()).all() and (psnr.cpu() > 0).all()
    assert (ssim.cpu() == 1).all()
    _check((mse, psnr, ssim), a, a)
    # one identical channel out of three: the channel mean of psnr is +inf, as numpy gives it
    c = b.clone()
    c[:, 1] = a[:, 1]
    _check(ops.frame_quality(a.cuda(), c.cuda()), a, c)
    # all-0 against all-255
    z, f = torch.zeros(4, 2, 16, 16, dtype=torch.uint8), torch.full((4, 2, 16, 16), 255, dtype=torch.uint8)
    got = ops.frame_quality(z.cuda(), f.cuda())
    _check(got, z, f)
    assert (got[0].cpu() == 65025).all() and (got[1].cpu() == 0).all()
    # a constant frame against noise, both ways round
    k = torch.full_like(a, 77)
    _check(ops.frame_quality(k.cuda(), a.cuda()), k, a)
    _check(ops.frame_quality(a.cuda(), k.cuda()), a, k)
    # channel-slice views (frame stride 3*H*W, no copy) and the [:, start:] view of a 5-D tensor
    ad, bd = a.cuda(), b.cuda()
    _check(ops.frame_quality(ad[:, 1:2], bd[:, 2:3]), a[:, 1:2], b[:, 2:3])
    _check(ops.frame_quality(ad[:, 1:], bd[:, :2]), a[:, 1:], b[:, :2])
    x5, y5 = _pair(15, 2, 16, 16, seed=6)
    x5, y5 = x5.view(3, 5, 2, 16, 16), y5.view(3, 5, 2, 16, 16)
    got = ops.frame_quality(x5.cuda()[:, 2:], y5.cuda()[:, 2:])
    assert tuple(got[0].shape) == (3, 3)
    _check(got, x5[:, 2:], y5[:, 2:])
    # an empty batch is no launch
    e = torch.zeros(0, 1, 8, 8, dtype=torch.uint8, device="cuda")
    assert all(t.shape == (0,) for t in ops.frame_quality(e, e))


def test_frame_quality_bit_reproducible():
    from rfn_hip import ops
    for N, C, H, W in ((320, 3, 64, 64), (2, 1, 256, 256)):
        a, b = _pair(N, C, H, W, seed=9)
        a, b = a.cuda(), b.cuda()
        r1 = [t.clone() for t in ops.frame_quality(a, b)]
        r2 = ops.frame_quality(a, b)
        for x, y in zip(r1, r2):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _ref_eval_seq(gt, pred):
    """the reference's eval_seq (error_metrics.py:154-171) with skimage replaced by the restatement"""
    gt, pred = gt.cpu(), pred.cpu()
    bs, T, C = gt.shape[:3]
    ssim, psnr, mse = torch.zeros((bs, T)), torch.zeros((bs, T)), torch.zeros((bs, T))
    for i in range(bs):
        for t in range(T):
            for c in range(C):
                s, p, _ = ref_ssim_psnr_channel(np.uint8(gt[i, t, c].numpy()), np.uint8(pred[i, t, c].numpy()))
                ssim[i, t] += s
                psnr[i, t] += p
            ssim[i, t] /= C
            psnr[i, t] /= C
            mse[i, t] = torch.mean((gt[i, t] - pred[i, t]) ** 2, dim=[0, 1, 2])
    return mse, ssim, psnr


def _close(a, b, rtol=1e-6, atol=0.0):
    a, b = a.double(), b.double()
    inf = torch.isinf(b)
    assert torch.equal(torch.isinf(a), inf)
    assert bool(((a[~inf] - b[~inf]).abs() <= atol + rtol * b[~inf].abs()).all()), (a - b).abs().max()


def test_eval_seq_vs_reference_loop():
    from evaluation_metrics import Evaluator
    from types import SimpleNamespace
    ev = Evaluator(SimpleNamespace(model=None, args=SimpleNamespace(n_frames=4), device=torch.device("cuda")))
    for C in (1, 3):
        a, b = _pair(4 * 5, C, 16, 16, seed=20 + C)
        gt = a.view(4, 5, C, 16, 16).float().cuda()
        pred = b.view(4, 5, C, 16, 16).float().cuda()
        pred[0, 1] = gt[0, 1]
        mse, ssim, psnr = ev.eval_seq(gt, pred)
        assert mse.device.type == "cpu" and mse.dtype == torch.float32 and tuple(mse.shape) == (4, 5)
        rm, rs, rp = _ref_eval_seq(gt, pred)
        _close(mse, rm)
        _close(psnr, rp)
        _close(ssim, rs, rtol=0.0, atol=1e-6)
        # uint8 inputs give the same numbers
        for x, y in zip(ev.eval_seq(gt.byte(), pred.byte()), (mse, ssim, psnr)):
            assert torch.equal(x, y)


def _tiny_solver_args(B=2):
    """the tiny solver configuration of tests/test_hip_modules.py (_tiny_solver_args)"""
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


def test_get_eval_values_best_of_n():
    """get_eval_values on the tiny model (B=2, T=6, 2 conditioning frames, 3 resamples, 2 batches) against the
    restatement applied to the predictions and losses it saw: best-of-N per metric (strict comparisons on the
    time-means), the mean over draws with the reference's aliasing of draw 0, and BPD / DKL / RECON of the last draw."""
    from RFN import RFN
    from RFN.trainer import Solver
    from evaluation_metrics import Evaluator
    args = _tiny_solver_args()
    torch.manual_seed(3)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.model = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(8)
    B, T, start, R = 2, 6, 2, 3
    batches = [torch.rand(B, T, 1, 16, 16, generator=g) for _ in range(3)]
    with torch.no_grad():
        s.model.loss(s.preprocess(batches[0][:, :args.n_frames].cuda()), 0)   # data dependent init
    settings = Namespace(n_frames=T, start_predictions=start, resample=R, n_trained=args.n_frames)
    ev = Evaluator(s, settings=settings)
    seen_pred, seen_loss = [], []
    plain_predict, plain_loss = s.model.predict, s.model.loss

    def predict_spy(*a, **k):
        out = plain_predict(*a, **k)
        seen_pred.append(out[1].clone())
        return out

    def loss_spy(*a, **k):
        out = plain_loss(*a, **k)
        seen_loss.append((out[1].detach().clone(), out[2].detach().clone(), tuple(a[0].shape)))
        return out

    s.model.predict, s.model.loss = predict_spy, loss_spy
    try:
        out = ev.get_eval_values("rfn.pt", loader=batches, max_batches=2)
    finally:
        del s.model.predict, s.model.loss
    mse_v, psnr_v, ssim_v, lpips_v, bpd, dkl, recon, ssim_std, psnr_std, lpips_std = out
    assert len(seen_pred) == 2 * R and len(seen_loss) == 2 * R
    assert lpips_v is None and lpips_std is None
    n_pred = T - start
    for t in (mse_v, psnr_v, ssim_v, ssim_std, psnr_std):
        assert tuple(t.shape) == (2 * B, n_pred) and t.dtype == torch.float32 and t.device.type == "cpu"

    quirk_seen = False
    exp = {k: [] for k in ("mse", "psnr", "ssim", "ssim_std", "psnr_std", "bpd", "dkl", "recon")}
    for bi in range(2):
        gt = s.preprocess(s.preprocess(batches[bi].cuda()), reverse=True)[:, start:].cpu().numpy()
        draws = []
        for r in range(R):
            pred = s.preprocess(seen_pred[bi * R + r], reverse=True).permute(1, 0, 2, 3, 4).numpy()
            assert pred.shape == gt.shape
            draws.append(ref_frame_quality(gt, pred))   # (mse, psnr, ssim) [B, n_pred] float64
        for m in range(3):   # the selection compares time-means: no near-ties between draws
            means = np.stack([d[m].mean(-1) for d in draws])
            for i in range(R):
                for j in range(i):
                    assert (np.abs(means[i] - means[j]) >= 1e-4).all(), (m, means)
        best = [draws[0][m].copy() for m in range(3)]
        plain_ssim = sum(d[2] for d in draws) / R
        for r in range(1, R):
            for m, better in ((0, lambda cur, new: cur > new), (1, lambda cur, new: cur < new),
                              (2, lambda cur, new: cur < new)):
                sel = better(best[m].mean(-1), draws[r][m].mean(-1))
                best[m][sel] = draws[r][m][sel]
        exp["mse"].append(best[0])
        exp["psnr"].append(best[1])
        exp["ssim"].append(best[2])
        # draw 0 of the mean over draws IS the best-so-far tensor in the reference: it holds the final best values
        exp["ssim_std"].append((best[2] + sum(d[2] for d in draws[1:])) / R)
        exp["psnr_std"].append((best[1] + sum(d[1] for d in draws[1:])) / R)
        quirk_seen = quirk_seen or not np.allclose(exp["ssim_std"][-1], plain_ssim, rtol=0, atol=1e-6)
        kl, nll, shp = seen_loss[bi * R + R - 1]
        assert shp == (B, args.n_frames, 1, 16, 16)
        b_, k_, n_ = ev.compute_loss(nll=nll, kl=kl, dims=shp[2:], t=shp[1] - 1)
        exp["bpd"].append(b_)
        exp["dkl"].append(k_)
        exp["recon"].append(n_)
    cat = {k: torch.from_numpy(np.concatenate(v)) for k, v in exp.items() if k not in ("bpd", "dkl", "recon")}
    _close(mse_v, cat["mse"])
    _close(psnr_v, cat["psnr"])
    _close(ssim_v, cat["ssim"], rtol=0.0, atol=1e-6)
    _close(psnr_std, cat["psnr_std"])
    _close(ssim_std, cat["ssim_std"], rtol=0.0, atol=1e-6)
    for k, got in (("bpd", bpd), ("dkl", dkl), ("recon", recon)):
        assert torch.equal(got, torch.FloatTensor(exp[k])), (k, got, exp[k])
    # the quirk matters here: some sequence's best SSIM draw is not draw 0, so the reported mean over draws is not the
    # plain mean of the three draws
    assert quirk_seen
