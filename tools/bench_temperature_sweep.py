#!/usr/bin/env python3
"""Developer tool: what making the temperatures per-row inputs of generation buys a temperature sweep.  Canonical model,
B = 32 sequences, 5 conditioning and 15 predicted frames, K = 6 temperatures, 8 draws of every sequence at every
temperature.  Wall time, device synchronised, of
  (a) sequential:   K RFN.predict_draws runs of 8 draws (8*B rows) with model.temperature set in front of each -- what a
                    sweep costs without per-row temperatures: the graph's key holds the value, so every change of
                    temperature rebuilds the generation graph;
  (b) rows_small:   per-row calls of K temperatures x P = max(1, 8 // K) draws, 8 / P of them: about (a)'s rows per call
                    (K*P*B against 8*B) -- what Evaluator.get_eval_values_temperatures does at draws_per_pass = 8;
  (c) rows_large:   one per-row call of K temperatures x 8 draws (K*8*B rows).
All three generate the same K * 8 * B * 15 frames.  Every figure is the median of REPS (default 5) repetitions after
one warm-up of each configuration, the configurations alternating within a repetition; min and max are reported beside
it, and the number of generation graphs built in the warm-up and per timed repetition.  Prints one JSON line.
RFN_GEN_GRAPH=0: eager launches."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch, bench
B, NC, NP, R = int(os.environ.get("B", 32)), 5, 15, 8
TEMPS = [0.001, 0.3, 0.5, 0.7, 1.0, 2.0]
K = len(TEMPS)
REPS = max(5, int(os.environ.get("REPS", 5)))
solver, args = bench.build_solver(B, NC + NP, torch.device("cuda"))
x = bench.make_batch(B, NC + NP, 5, "cuda")
solver.train_step(x)  # ActNorm init
m = solver.model.eval()
xin = solver.preprocess(x)
P_SMALL = max(1, R // K)


def sequential():
    keep = m.temperature
    try:
        for T in TEMPS:
            m.temperature = T
            m._predict_draws_device(xin, NP, NC, R, 1)
    finally:
        m.temperature = keep


def rows_small():
    for ps in range(R // P_SMALL):
        m._predict_draws_device(xin, NP, NC, P_SMALL, 1, first_draw=ps * P_SMALL, temperatures=TEMPS)


def rows_large():
    m._predict_draws_device(xin, NP, NC, R, 1, temperatures=TEMPS)


configs = [("sequential", sequential), ("rows_small", rows_small), ("rows_large", rows_large)]
times = {name: [] for name, _ in configs}
builds = {name: {"warmup": 0, "timed": 0} for name, _ in configs}
count = lambda: getattr(m, "_gen_graph_builds", 0)
with torch.no_grad():
    for name, fn in configs:
        n0 = count()
        fn()
        builds[name]["warmup"] = count() - n0
    torch.cuda.synchronize()
    for rep in range(REPS):
        for name, fn in configs:
            n0 = count()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            builds[name]["timed"] += count() - n0

units = K * R * B * NP   # (temperature, sequence, draw, generated frame) per timed window
print(json.dumps({
    "bench": "temperature_sweep", "B": B, "n_conditions": NC, "n_predictions": NP, "temperatures": TEMPS, "draws": R,
    "reps": REPS, "mode": "graph" if os.environ.get("RFN_GEN_GRAPH", "1") != "0" else "eager",
    "rows_per_call": {"sequential": R * B, "rows_small": K * P_SMALL * B, "rows_large": K * R * B},
    "calls": {"sequential": K, "rows_small": R // P_SMALL, "rows_large": 1},
    "us_per_temp_seq_draw_frame": {k: round(1e6 * statistics.median(v) / units, 3) for k, v in times.items()},
    "ms_per_sweep": {k: round(1e3 * statistics.median(v), 2) for k, v in times.items()},
    "ms_per_sweep_min_max": {k: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in times.items()},
    "graph_builds": {k: {"warmup": v["warmup"], "per_timed_rep": v["timed"] / REPS} for k, v in builds.items()}}))
