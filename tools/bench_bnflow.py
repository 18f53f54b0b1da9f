#!/usr/bin/env python3
"""Developer tool: cost of the batch-norm flow step (--flow_norm batchnorm).  Prints ONE JSON line.

  python tools/bench_bnflow.py kernels [--B 32 --S 19]
      rfn_bnflow_{fwd,bwd,apply}_f32 at the five level shapes of the canonical flow, as hipGraph replays of 20 launches
      (kernel time, no Python), against the torch expression of BatchNormFlow run as S per-step calls (the per-step
      semantics at the cost of the unfused module; forward, and forward + backward through autograd), alternated
      repetition by repetition.  Per entry: median / min / max of the repetitions in microseconds, and the bytes the
      pass NEEDS (x and z once forward, x, gz and gx once backward) over the median as a share of the HBM peak.
  python tools/bench_bnflow.py step [--flow_norm batchnorm] [--base_norm actnorm]
      one B x T training step (hipGraph replay, fwd + bwd + Adam) of the canonical SM-MNIST configuration with these
      norms, in the package RFN_PKG_DIR names (default: this tree's): ms/step of `--windows` windows of `--steps` steps.
  python tools/bench_bnflow.py ab --parent DIR [--rounds 3]
      `step` in fresh child processes, DIR (another build of the package) and this tree's alternated `--rounds` times;
      median / min / max over all windows of each side.  With --flow_norm batchnorm this compares COST only: a parent
      that takes its statistics over all B*(T-1) frames at once computes something else.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
if "torch" not in sys.modules:
    os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
PKG = os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)

PEAK_HBM_GBS = 8000.0   # MI355X_MICROARCH.md (bench.py's roof)
LEVELS = ((4, 32), (8, 16), (16, 8), (32, 4), (64, 2))   # (C, H = W) of the canonical flow's five levels
EPS = 1e-5


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def graphed(fn, reps):
    """fn captured `reps` times into one hipGraph (after warm-ups on a side stream) -> a callable timing one replay in
    microseconds per fn"""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    return once


def kernels(a):
    import torch
    from rfn_hip import lib as L
    from rfn_hip import ops as K
    assert torch.cuda.is_available(), "bench_bnflow.py needs a GPU"
    S, B = a.S, a.B
    out = []
    for C, H in LEVELS:
        E = C * H * H
        r = lambda *s: torch.randn(*s, device="cuda")
        x, gz, lg, beta, gdl = r(S * B, E) + r(E), r(S * B, E), 0.1 * r(E), r(E), r(S)
        z, gx, mean, var, dl = torch.empty_like(x), torch.empty_like(x), r(S, E), r(S, E), r(S)
        rm, rv, glg, gb, dl1 = torch.zeros(E, device="cuda"), torch.ones(E, device="cuda"), r(E), r(E), r(1)
        cf, decay = K.bnflow_coef(S, 0.3)
        cf = cf.float().cuda()
        scr = torch.empty(int(L.load().rfn_bnflow_scratch_floats(S, B, E, 1)), device="cuda")  # (>= the forward's)

        def fwd():
            L.call("rfn_bnflow_fwd_f32", L.dev(x), L.dev(lg), L.dev(beta), L.dev(z), L.dev(mean), L.dev(var), L.dev(dl),
                   L.dev(scr), L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cf), decay, S, B, E, EPS)

        def bwd():
            L.call("rfn_bnflow_bwd_f32", L.dev(x), L.dev(lg), L.dev(gz), L.dev(gdl), L.dev(mean), L.dev(var), L.dev(gx),
                   L.dev(glg), L.dev(gb), L.dev(scr), S, B, E)

        def apply():
            L.call("rfn_bnflow_apply_f32", L.dev(x), L.dev(lg), L.dev(beta), L.dev(rm), L.dev(rv), L.dev(z), L.dev(dl1),
                   S * B, E, 0)

        # the torch expression of the unfused module (glow_modules.py:76-98 of the reference), one call per step
        lgp, bp = lg.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        xs = x.view(S, B, E)

        def torch_step(xt, m=0.3):
            mu = xt.mean(0)
            v = (xt - mu).pow(2).mean(0) + EPS
            rm.mul_(m).add_(mu.data * (1 - m))
            rv.mul_(m).add_(v.data * (1 - m))
            return torch.exp(lgp) * ((xt - mu) / v.sqrt()) + bp, torch.sum(lgp - 0.5 * torch.log(v))

        def torch_fwd():
            with torch.no_grad():
                for s in range(S):
                    torch_step(xs[s])

        xg = x.clone().requires_grad_(True)

        def torch_fwd_bwd():
            loss = 0
            for s in range(S):
                zz, d = torch_step(xg.view(S, B, E)[s])
                loss = loss + (zz * gz.view(S, B, E)[s]).sum() + d * gdl[s]
            xg.grad = lgp.grad = bp.grad = None
            loss.backward()

        fwd(); bwd()
        torch.cuda.synchronize()
        timers = {"fwd": graphed(fwd, 20), "bwd": graphed(bwd, 20), "apply": graphed(apply, 20),
                  "torch_fwd": graphed(torch_fwd, 2)}
        try:
            timers["torch_fwd_bwd"] = graphed(torch_fwd_bwd, 2)
        except Exception as e:  # noqa: BLE001 - autograd under capture: report that it could not be timed
            torch.cuda.synchronize()
            print("torch_fwd_bwd not captured: %r" % (e,), file=sys.stderr)
        t = {k: [] for k in timers}
        for _ in range(a.reps):      # alternated: one repetition of each, then the next round
            for k, f in timers.items():
                t[k].append(f())
        by = 4.0 * S * B * E
        need = {"fwd": 2 * by, "bwd": 3 * by, "apply": 2 * by}
        row = {"shape": [S, B, C, H, H], "us": {k: summary(v) for k, v in t.items()},
               "needed_bytes_over_time_share_of_hbm_peak": {
                   k: need[k] / (statistics.median(t[k]) * 1e-6) / 1e9 / PEAK_HBM_GBS for k in need}}
        out.append(row)
        print("S%d B%d C%d %dx%d  " % (S, B, C, H, H) + "  ".join("%s %.1f us" % (k, statistics.median(v))
                                                                    for k, v in t.items()), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "bench_bnflow kernels", "protocol": "hipGraph replays, median/min/max of %d alternated "
                      "repetitions, profiler off" % a.reps, "hbm_peak_GBs": PEAK_HBM_GBS, "rows": out}))


def step(a):
    import time
    import torch
    import bench
    import main_rfn
    dev = torch.device("cuda")
    argv = main_rfn.canonical_smmnist_argv(a.batch, a.frames)
    argv[argv.index("--flow_norm") + 1] = a.flow_norm
    argv += ["--base_norm", a.base_norm]
    solver, args = bench.build_solver(a.batch, a.frames, dev, argv=argv)
    batches = [bench.make_batch(a.batch, a.frames, 100 + i, dev) for i in range(2)]
    for i in range(4):
        solver.train_step(batches[i % 2])
    ok = solver.capture_graph(batches[0])
    solver.train_step(batches[0])
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        for i in range(a.steps):
            solver.train_step(batches[i % 2])
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / a.steps)
    solver.flush_log()
    print(json.dumps({"tool": "bench_bnflow step", "pkg": PKG, "flow_norm": a.flow_norm, "base_norm": a.base_norm,
                      "batch": a.batch, "frames": a.frames, "graph": bool(ok),
                      "graph_error": None if ok else getattr(solver, "_graph_error", ""), "ms_per_step": ms,
                      "bits_per_dim_last_step": float(solver.bits[-1])}))


def ab(a):
    sides = {"parent": os.path.abspath(a.parent), "new": os.path.join(ROOT, "recurrent-flows-msc_amd")}
    ms, runs = {k: [] for k in sides}, []
    for _ in range(a.rounds):
        for side, pkg in sides.items():     # alternated: parent, new, parent, new, ...
            env = dict(os.environ, RFN_PKG_DIR=pkg)
            cmd = [sys.executable, os.path.abspath(__file__), "step", "--flow_norm", a.flow_norm, "--base_norm", a.base_norm,
                   "--batch", str(a.batch), "--frames", str(a.frames), "--windows", str(a.windows), "--steps", str(a.steps)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:   # nothing more is started after a child that failed
                print(p.stderr[-3000:], file=sys.stderr)
                raise SystemExit("child (%s) ended with %d" % (side, p.returncode))
            r = json.loads(p.stdout.strip().splitlines()[-1])
            r["side"] = side
            runs.append(r)
            ms[side] += r["ms_per_step"]
            print("%s: %s" % (side, " ".join("%.2f" % v for v in r["ms_per_step"])), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "bench_bnflow ab", "flow_norm": a.flow_norm, "base_norm": a.base_norm, "batch": a.batch,
                      "frames": a.frames, "protocol": "fresh child per run, parent and new alternated, %d rounds x %d "
                      "windows x %d hipGraph-replayed steps, profiler off" % (a.rounds, a.windows, a.steps),
                      "ms_per_step": {k: summary(v) for k, v in ms.items()}, "runs": runs}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "step", "ab"))
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--S", type=int, default=19)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--flow_norm", default="batchnorm")
    ap.add_argument("--base_norm", default="actnorm")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=400)
    a = ap.parse_args()
    {"kernels": kernels, "step": step, "ab": ab}[a.mode](a)
