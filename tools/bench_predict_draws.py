#!/usr/bin/env python3
"""Developer tool: what batching the draws of best-of-N evaluation buys.  Canonical model, B = 32 sequences,
5 conditioning and 15 predicted frames.  Wall time per (sequence, draw, generated frame), device synchronised, of
  * R = 8 sequential RFN.predict calls (what Evaluator.get_eval_values does per batch without draws_per_pass), and
  * RFN.predict_draws at P = 1, 4, 8 draws per pass (8 / P calls, i.e. the same 8 draws),
plus the time of one rfn_keyed_normal_f32 launch filling the slots of a generation step (HIP events around a run of
launches).  Every figure is the median of REPS (default 5) repetitions after a warm-up of every shape; the
configurations alternate within a repetition.  Prints one JSON line.  RFN_GEN_GRAPH=0: eager launches."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch, bench
from rfn_hip import ops
B, NC, NP, R = int(os.environ.get("B", 32)), 5, 15, 8
REPS = max(5, int(os.environ.get("REPS", 5)))
solver, args = bench.build_solver(B, NC + NP, torch.device("cuda"))
x = bench.make_batch(B, NC + NP, 5, "cuda")
solver.train_step(x)  # ActNorm init
m = solver.model.eval()
xin = solver.preprocess(x)


def sequential():
    for _ in range(R):
        m._predict_device(xin, NP, NC)


def batched(P):
    def run():
        for ps in range(R // P):
            m._predict_draws_device(xin, NP, NC, P, 1, first_draw=ps * P)
    return run


configs = [("predict_x8", sequential)] + [("predict_draws_p%d" % P, batched(P)) for P in (1, 4, 8)]
times = {name: [] for name, _ in configs}
with torch.no_grad():
    for name, fn in configs:          # warm-up: every shape, every graph
        fn()
    torch.cuda.synchronize()
    for rep in range(REPS):
        for name, fn in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)

# one keyed_normal launch of a generation step (slot 1, the encoder eps, is not drawn there)
noise_us, noise_mb = {}, {}
LAUNCHES = 200
for P in (1, 4, 8):
    shapes = [tuple(sh[1:]) for sh in m._gen_eps_shapes(P * B)]
    outs = ops.keyed_normal([shapes[0], None] + shapes[1:], B, P, 1, NC, device="cuda")
    noise_mb[P] = sum(t.numel() for t in outs if t is not None) * 4 / 1e6
    per = []
    for rep in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(LAUNCHES):
            ops.keyed_normal(None, B, P, 1, NC + i, out=outs)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            per.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    noise_us[P] = statistics.median(per)

units = R * B * NP   # (sequence, draw, generated frame) per timed window
print(json.dumps({
    "bench": "predict_draws", "B": B, "n_conditions": NC, "n_predictions": NP, "draws": R, "reps": REPS,
    "mode": "graph" if os.environ.get("RFN_GEN_GRAPH", "1") != "0" else "eager",
    "us_per_seq_draw_frame": {k: round(1e6 * statistics.median(v) / units, 3) for k, v in times.items()},
    "ms_per_8_draws": {k: round(1e3 * statistics.median(v), 2) for k, v in times.items()},
    "ms_per_8_draws_min_max": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in times.items()},
    "keyed_normal_us_per_step": {"p%d" % P: round(noise_us[P], 2) for P in noise_us},
    "keyed_normal_mb_per_step": {"p%d" % P: round(noise_mb[P], 3) for P in noise_mb},
    "graph_builds": getattr(m, "_gen_graph_builds", 0)}))
