#!/usr/bin/env python3
"""Developer tool: cost of the Polyak average inside the Adam launch.  Four `rfn_hip.optim.HipAdam`
instances over tensors with the shapes of the canonical model's parameter list, each with its own parameters, gradients,
moments (and averages): plain (rfn_adam_step_f32) against plain + ema (rfn_adam_ema_step_f32), and guarded
(rfn_grad_sumsq_f32's two launches, rfn_grad_guard_f32, rfn_adam_step_guarded_f32) against guarded + ema
(... rfn_adam_ema_step_guarded_f32).  The gradient tensors stay put, so nobody rebuilds a table: the steady path of
hipGraph mode.  Also timed: swap_ema() (one rfn_param_swap_f32 launch, 16 B per element).

Two timings per variant, `--rounds` times with the variants alternating within a round; median, min and max over the
rounds are reported.  `<name>_us`: HIP events around `--iters` back-to-back `step()` calls, what a training step pays;
with 925 tensors `step()` spends more host time (pointer keys, step counts) than the kernel runs, so this figure is the
host's.  `<name>_kernel_us`: the device time of the Adam launch alone, from the events `rfn_hip.lib.call` records around
each launch (`--kernel_iters` launches a round, their median), and `<name>_kernel_gbps`, the bytes the launch needs over
it.  One plain launch streams 28 B per element (p, g, m, v read; p, m, v written), one ema launch 36 B (the average read
and written as well): from the bytes alone the expected ratio is 36 / 28 = 1.29.  The working set is several times the
256 MiB Infinity Cache, so back-to-back launches do not find their operands cached.  Prints one JSON line; --out also
writes it to a file."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch

from bench_adam_guard import canonical_shapes, make, timed

GUARD = dict(max_grad_norm=1.0, skip_nonfinite=True)
VARIANTS = (("plain", {}, 28.0), ("ema", dict(ema_decay=0.999), 36.0),
            ("guarded", GUARD, 32.0), ("guarded_ema", dict(GUARD, ema_decay=0.999), 40.0))


def timed_swap(opt, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(2 * (iters // 2)):   # an even count: the weights end where they were
        opt.swap_ema()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (2 * (iters // 2))


def kernel_us(fn, iters, prefix):
    """median device time of one launch whose entry point starts with `prefix`, over `iters` calls of fn(): the HIP
    events rfn_hip.lib.call records around every launch when PROFILE is a list.  `step()` spends more host time on its
    925 tensors than the kernel runs, so back-to-back steps measure the host; this is the kernel itself."""
    from rfn_hip import lib as L
    L.PROFILE = rec = []
    try:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    finally:
        L.PROFILE = None
    return round(statistics.median(1e3 * e0.elapsed_time(e1) for name, _, e0, e1 in rec if name.startswith(prefix)), 2)


def spread(rounds, key):
    vals = [r[key] for r in rounds]
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernel_iters", type=int, default=50, help="launches per round timed one by one with events")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_adam_ema needs a GPU"
    shapes = canonical_shapes(a.batch)
    n = sum(int(torch.Size(sh).numel()) for sh in shapes)
    opts = {name: make(shapes, 1 + i, **kw) for i, (name, kw, _) in enumerate(VARIANTS)}
    for opt in opts.values():
        for _ in range(a.warmup):
            opt.step()
    opts["ema"].swap_ema(); opts["ema"].swap_ema()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(a.rounds):
        r = {name + "_us": round(timed(opts[name], a.iters), 2) for name, _, _ in VARIANTS}
        r["swap_us"] = round(timed_swap(opts["ema"], a.iters), 2)
        for name, _, _ in VARIANTS:
            r[name + "_kernel_us"] = kernel_us(opts[name].step, a.kernel_iters, "rfn_adam_")
        r["swap_kernel_us"] = kernel_us(opts["ema"].swap_ema, 2 * (a.kernel_iters // 2), "rfn_param_swap")
        rounds.append(r)
    for name in ("guarded", "guarded_ema"):
        gs = opts[name].guard_stats()
        assert gs["skipped_steps"] == 0 and 0.0 < gs["scale"] <= 1.0, gs
    res = {"tensors": len(shapes), "elements": n}
    for name, _, nbytes in VARIANTS:
        res[name + "_us"] = spread(rounds, name + "_us")
        res[name + "_kernel_us"] = spread(rounds, name + "_kernel_us")
        # bytes the Adam launch needs (the guard's second read of g belongs to its own launches) over its device time
        kbytes = nbytes - (4.0 if name.startswith("guarded") else 0.0)
        res[name + "_kernel_gbps"] = round(kbytes * n / res[name + "_kernel_us"]["median"] / 1e3, 1)
    res["swap_us"] = spread(rounds, "swap_us")
    res["swap_kernel_us"] = spread(rounds, "swap_kernel_us")
    res["swap_kernel_gbps"] = round(16.0 * n / res["swap_kernel_us"]["median"] / 1e3, 1)
    for a_, b_ in (("ema", "plain"), ("guarded_ema", "guarded")):
        res[a_ + "_over_" + b_] = round(res[a_ + "_us"]["median"] / res[b_ + "_us"]["median"], 3)
        res[a_ + "_over_" + b_ + "_kernel"] = round(res[a_ + "_kernel_us"]["median"] / res[b_ + "_kernel_us"]["median"], 3)
    line = json.dumps({"adam_ema": res, "iters": a.iters, "warmup": a.warmup, "rounds": rounds})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
