#!/usr/bin/env python3
"""Developer tool: cost of the frame-quality metrics (rfn_frame_quality_u8 / rfn_hip.ops.frame_quality) and of one
best-of-N evaluation batch (Evaluator.get_eval_values) on the canonical SM-MNIST model.  Prints one JSON line:
  kernel:  us per launch (HIP events over `reps` back-to-back launches) and frames/s for N = 32 x 10 frames of 1x64x64
           and 3x64x64;
  eval:    ms per batch of get_eval_values (B = 32 sequences, 5 conditioning + 10 predicted frames, `resample` draws),
           split into predict / loss / metrics (host clock, device synchronised around each part)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch


def time_kernel(C, N, reps):
    from rfn_hip import ops
    g = torch.Generator().manual_seed(C)
    a = torch.randint(0, 256, (N, C, 64, 64), generator=g, dtype=torch.uint8).cuda()
    b = torch.randint(0, 256, (N, C, 64, 64), generator=g, dtype=torch.uint8).cuda()
    for _ in range(10):
        ops.frame_quality(a, b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.frame_quality(a, b)
    e1.record()
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / reps
    return {"shape": [N, C, 64, 64], "us_per_launch": round(us, 2), "frames_per_s": round(N / (us * 1e-6)),
            "bytes_read": 2 * N * C * 64 * 64}


def time_eval(B, resample, n_cond, n_pred, rounds):
    import bench
    from argparse import Namespace
    from evaluation_metrics import Evaluator
    solver, args = bench.build_solver(B, 10, torch.device("cuda"))
    solver.train_step(bench.make_batch(B, 10, 5, "cuda"))   # ActNorm data dependent init
    batch = bench.make_batch(B, n_cond + n_pred, 6, "cuda")
    ev = Evaluator(solver, settings=Namespace(n_frames=n_cond + n_pred, start_predictions=n_cond, resample=resample,
                                              n_trained=args.n_frames))
    spent = {"predict": 0.0, "loss": 0.0, "metrics": 0.0}

    def timed(part, fn):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            spent[part] += time.perf_counter() - t0
            return out
        return run

    m = solver.model
    m.predict, m.loss, ev.eval_seq = timed("predict", m.predict), timed("loss", m.loss), timed("metrics", ev.eval_seq)
    ev.get_eval_values("rfn.pt", loader=[batch])       # warm-up: generation graph, code objects
    for k in spent:
        spent[k] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        ev.get_eval_values("rfn.pt", loader=[batch])
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    res = {"B": B, "n_conditions": n_cond, "n_predictions": n_pred, "resample": resample,
           "ms_per_batch": round(1e3 * total / rounds, 2)}
    res.update({"ms_" + k: round(1e3 * v / rounds, 2) for k, v in spent.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--resample", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-eval", action="store_true", help="kernel timings only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frame_metrics needs a GPU"
    out = {"kernel": [time_kernel(C, 32 * 10, a.reps) for C in (1, 3)]}
    if not a.no_eval:
        out["eval"] = time_eval(32, a.resample, 5, 10, a.rounds)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
