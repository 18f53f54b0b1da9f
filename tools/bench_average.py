#!/usr/bin/env python3
"""Developer tool: cost of the linear-extrapolation kernels (csrc/linear_extrap.hip).  Prints ONE JSON line.

  python tools/bench_average.py [--B 256 --n 5 --C 3 --H 64 --P 10 --reps 5 --out profiles/average_model_bench.json]

Three pairs, each the fused kernels against the torch op chain of the reference's expressions in float32 on the same
device (tests/test_average.py holds the restatements):
  train     loss and all gradients: rfn_hip.ops.linear_extrap_loss + backward, against forward + backward of the chain
            (cat of the n (n + 1) / 2 feature frames, matmul, mse_loss);
  rollout   P frames: rfn_hip.ops.linear_extrap_rollout, against the chain's loop of predictions and cats;
  quality   rfn_hip.ops.gauss_quality of N = B frame pairs, against the Gaussian-window SSIM and the MSE as grouped
            convolutions and elementwise ops.
Each figure is the median / min / max of `--reps` repetitions, kernels and op chain alternated repetition by
repetition; a repetition times `--inner` back-to-back calls between two events on the stream after two warm-up calls.
Profiler off.  needed_bytes = the bytes a call NEEDS (train: the n + 1 frames read once; rollout: n frames read, P
written; quality: both frames read once); hbm_fraction = needed_bytes / median time over the 8 TB/s peak.  The inputs
of the default shape (75 MB) fit the 256 MiB Infinity Cache, so back-to-back calls may be served from it: the fraction
is a rate of needed bytes, not a measurement of HBM traffic."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)

PEAK_HBM_GBS = 8000.0   # MI355X_MICROARCH.md (bench.py's roof)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def timer(fn, inner):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3   # microseconds per call
    return once


def main(a):
    import torch
    from rfn_hip import ops as K
    from tests import test_average as R
    assert torch.cuda.is_available(), "bench_average.py needs a GPU"
    B, n, C, H, P = a.B, a.n, a.C, a.H, a.P
    F = n * (n + 1) // 2
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(B, n + 1, C, H, H, generator=g, device="cuda")
    W = 0.05 * torch.randn(1, F, generator=g, device="cuda")
    W[0, n - 1] += 1.0
    bias = torch.full((1, 1), 0.01, device="cuda")
    Wg, bg = W.clone().requires_grad_(), bias.clone().requires_grad_()
    X, Y = x[:, 0].contiguous(), (x[:, 0] + 20.0 / 255 * torch.randn(B, C, H, H, generator=g, device="cuda")).contiguous()

    def k_train():
        Wg.grad = bg.grad = None
        K.linear_extrap_loss(x, Wg, bg, n).backward()

    def t_train():
        Wg.grad = bg.grad = None
        R.chain_loss(x, Wg, bg, n).backward()

    def k_rollout():
        K.linear_extrap_rollout(x, W, bias, n, P)

    def t_rollout():
        with torch.no_grad():
            R.chain_rollout(x, W, bias, n, P)

    def k_quality():
        K.gauss_quality(X, Y)

    def t_quality():
        with torch.no_grad():
            R.gauss_ref(X, Y, torch.float32)

    # the two routes agree before they are timed
    k_train()
    got = torch.cat((Wg.grad.view(-1), bg.grad.view(-1))).clone()
    t_train()
    want = torch.cat((Wg.grad.view(-1), bg.grad.view(-1)))
    agree = {"grad_max_abs_diff": float((got - want).abs().max()),
             "rollout_max_abs_diff": float((K.linear_extrap_rollout(x, W, bias, n, P) - R.chain_rollout(x, W, bias, n, P)).abs().max()),
             "ssim_max_abs_diff": float((K.gauss_quality(X, Y)[0].double().cpu() - R.gauss_ref(X.cpu(), Y.cpu(), torch.float64)[0]).abs().max())}

    timers = {"train": timer(k_train, a.inner), "torch_train": timer(t_train, a.inner),
              "rollout": timer(k_rollout, a.inner), "torch_rollout": timer(t_rollout, a.inner),
              "quality": timer(k_quality, a.inner), "torch_quality": timer(t_quality, a.inner)}
    t = {k: [] for k in timers}
    for _ in range(a.reps):      # alternated: one repetition of each, then the next round
        for k, f in timers.items():
            t[k].append(f())
    px = 4.0 * B * C * H * H
    need = {"train": px * (n + 1), "rollout": px * (n + P), "quality": px * 2}
    med = {k: statistics.median(v) for k, v in t.items()}
    line = json.dumps({
        "tool": "bench_average", "device": torch.cuda.get_device_name(0),
        "protocol": "median/min/max of %d alternated repetitions, each %d back-to-back calls between stream events, two "
                    "warm-up calls, profiler off" % (a.reps, a.inner),
        "shape": {"B": B, "n": n, "F": F, "C": C, "H": H, "W": H, "P": P}, "hbm_peak_GBs": PEAK_HBM_GBS,
        "us": {k: summary(v) for k, v in t.items()}, "needed_bytes": need,
        "needed_GBs": {k: need[k] / (med[k] * 1e-6) / 1e9 for k in need},
        "hbm_fraction": {k: need[k] / (med[k] * 1e-6) / 1e9 / PEAK_HBM_GBS for k in need},
        "torch_over_kernel": {k: med["torch_" + k] / med[k] for k in need}, "agreement": agree})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--C", type=int, default=3)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--P", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    main(ap.parse_args())
