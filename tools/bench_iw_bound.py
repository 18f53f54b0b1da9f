#!/usr/bin/env python3
"""Developer tool: what running the chains of RFN's importance-weighted bound as one batch buys.  Canonical model,
B = 32 sequences of T = 10 frames, K = 20 chains.  Wall time per (sequence, chain, frame), device synchronised, of
  * K eval-mode RFN.loss calls under no_grad (K one-sample ELBO evaluations: what a user could do without
    RFN.iw_log_weights), and
  * RFN.iw_log_weights at P = 1, 4, 20 chains per pass (K / P passes, i.e. the same K chains),
and torch.cuda.max_memory_allocated of each configuration (peak statistics reset before its timed runs).  Every time is
the median of REPS (default 5) repetitions after a warm-up of every shape; the configurations alternate within a
repetition.  Prints one JSON line."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch, bench
B, T, K = int(os.environ.get("B", 32)), int(os.environ.get("T", 10)), int(os.environ.get("K", 20))
PS = tuple(int(p) for p in os.environ.get("P", "1,4,20").split(","))
REPS = max(5, int(os.environ.get("REPS", 5)))
solver, args = bench.build_solver(B, T, torch.device("cuda"))
x = bench.make_batch(B, T, 5, "cuda")
solver.train_step(x)  # ActNorm init
m = solver.model.eval()
xin = solver.preprocess(x)


def loss_calls():
    for _ in range(K):
        m.loss(xin, 0)


def chains(P):
    return lambda: m.iw_log_weights(xin, K, 1, chains_per_pass=P)


configs = [("loss_x%d" % K, loss_calls)] + [("iw_p%d" % P, chains(P)) for P in PS]
times = {name: [] for name, _ in configs}
peak = {}
with torch.no_grad():
    for name, fn in configs:          # warm-up: every shape; the peak memory of each configuration on its own
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
    for rep in range(REPS):
        for name, fn in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    whole = m.iw_log_weights(xin, K, 1)
    bound = float(m.elbo_importance_weighting(xin, K, seed=1))
    one = float(-whole.mean())

units = B * K * (T - 1)   # (sequence, chain, frame) per timed window
print(json.dumps({
    "bench": "iw_bound", "B": B, "T": T, "K": K, "reps": REPS,
    "us_per_seq_chain_frame": {k: round(1e6 * statistics.median(v) / units, 3) for k, v in times.items()},
    "us_per_seq_chain_frame_min_max": {k: [round(1e6 * min(v) / units, 3), round(1e6 * max(v) / units, 3)]
                                       for k, v in times.items()},
    "ms_per_%d_chains" % K: {k: round(1e3 * statistics.median(v), 2) for k, v in times.items()},
    "max_memory_allocated_mb": {k: round(v / 2 ** 20, 1) for k, v in peak.items()},
    "nats_per_seq": {"iw_bound_K%d" % K: round(bound, 3), "mean_single_chain": round(one, 3)}}))
