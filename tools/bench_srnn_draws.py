#!/usr/bin/env python3
"""Developer tool: what batching the draws of best-of-N evaluation buys for the SRNN baseline, and what the keyed
mixture sampler costs.  Prints ONE JSON line.

  python tools/bench_srnn_draws.py [--B 32 --reps 5]

SRNN with main_srnn.py's defaults (h_dim = a_dim = 60, z_dim = 20, batch norm, loss_type mol, M = 10) at B sequences of
64x64 gray frames, 5 conditioning and 15 predicted frames, eval mode, freshly initialised weights (the time does not
depend on them).  Wall time, device synchronised, of
  * R = 8 sequential SRNN._predict_device calls (what Evaluator.get_eval_values does per batch without draws_per_pass)
  * SRNN._predict_draws_device at P = 1, 4, 8 draws per pass (8 / P calls: the same 8 draws),
as the median of `--reps` repetitions with min and max, after a warm-up of every shape; the configurations alternate
within a repetition (the protocol of tools/bench_predict_draws.py).
The sampler alone at N = 256 frames (8 draws x 32 sequences), C = 1, M = 10: rfn_hip.ops.mol_sample_keyed against the two
torch.empty().uniform_() draws + mol_sample it replaces, with the protocol of tools/bench_mol.py (median / min / max of
`--reps` alternated repetitions, each `--inner` back-to-back calls between two stream events, two warm-up calls)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)

NC, NP, R = 5, 15, 8


def summary(v, scale=1.0, digits=2):
    return {"median": round(scale * statistics.median(v), digits), "min": round(scale * min(v), digits),
            "max": round(scale * max(v), digits), "n": len(v)}


def event_timer(fn, inner):
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
    import main_srnn
    from SRNN import SRNN
    from rfn_hip import ops as K
    assert torch.cuda.is_available(), "bench_srnn_draws.py needs a GPU"
    B, H, M = a.B, 64, 10
    args = main_srnn.build_parser().parse_args(
        ("--batch_size %d --x_dim %d 1 %d %d --condition_dim %d 1 %d %d --n_logistics %d" % (B, B, H, H, B, H, H, M)).split())
    torch.manual_seed(0)
    m = SRNN(args).to("cuda").eval()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = 2.0 * torch.randint(0, 256, (B, NC + NP, 1, H, H), generator=g, device="cuda").float() / 255.0 - 1.0

    def sequential():
        for _ in range(R):
            m._predict_device(x, NP, NC)

    def batched(P):
        def run():
            for ps in range(R // P):
                m._predict_draws_device(x, NP, NC, P, 1, first_draw=ps * P)
        return run

    configs = [("predict_x8", sequential)] + [("predict_draws_p%d" % P, batched(P)) for P in (1, 4, 8)]
    times = {name: [] for name, _ in configs}
    with torch.no_grad():
        for _, fn in configs:          # warm-up: every shape
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in configs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)

    # the sampler alone: 256 frames, the logits of tools/bench_mol.py's recipe
    N = 8 * B
    l = torch.empty(N, 3 * M, H, H, device="cuda")
    l[:, :M] = 2.0 * torch.randn(N, M, H, H, generator=g, device="cuda")
    l[:, M:2 * M] = torch.rand(N, M, H, H, generator=g, device="cuda") * 2.0 - 1.0
    l[:, 2 * M:] = torch.rand(N, M, H, H, generator=g, device="cuda") * 7.5 - 8.0

    def keyed():
        K.mol_sample_keyed(l, B, 1, NC, channels=1)

    def drawn():
        u_mix = torch.empty((N, H, H, M), device="cuda").uniform_(1e-5, 1.0 - 1e-5)
        u_x = torch.empty((N, H, H, 1), device="cuda").uniform_(1e-5, 1.0 - 1e-5)
        K.mol_sample(l, u_mix, u_x)

    timers = {"mol_sample_keyed": event_timer(keyed, a.inner), "uniform_x2_mol_sample": event_timer(drawn, a.inner)}
    sampler = {k: [] for k in timers}
    for _ in range(a.reps):
        for k, f in timers.items():
            sampler[k].append(f())

    units = R * B * NP   # (sequence, draw, generated frame) per timed window
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "bench": "srnn_draws", "B": B, "n_conditions": NC, "n_predictions": NP, "draws": R, "reps": a.reps,
        "frame": [1, H, H], "n_logistics": M, "mode": "eval",
        "ms_per_8_draws": {k: summary(v, 1e3) for k, v in times.items()},
        "us_per_seq_draw_frame": {k: round(1e6 * v / units, 3) for k, v in med.items()},
        "predict_x8_over": {k: round(med["predict_x8"] / v, 3) for k, v in med.items() if k != "predict_x8"},
        "sampler_frames": N, "sampler_uniform_mb_removed": round(4.0 * N * H * H * (M + 1) / 1e6, 1),
        "sampler_us": {k: summary(v) for k, v in sampler.items()},
        "sampler_protocol": "median/min/max of %d alternated repetitions, each %d back-to-back calls between stream "
                            "events, two warm-up calls, profiler off" % (a.reps, a.inner)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    main(ap.parse_args())
