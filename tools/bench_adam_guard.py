#!/usr/bin/env python3
"""Developer tool: cost of the guard of the Adam step.  Two `rfn_hip.optim.HipAdam` instances over tensors
with the shapes of the canonical model's parameter list (36.5 M elements in 925 tensors at batch 32), each with its own
parameters, gradients and moments: one plain (one rfn_adam_step_f32 launch), one with `max_grad_norm` and
`skip_nonfinite` on (rfn_grad_sumsq_f32's two launches, rfn_grad_guard_f32, rfn_adam_step_guarded_f32).  The gradient
tensors stay put, so neither rebuilds its table: the steady path of hipGraph mode.

Timing: HIP events around `--iters` back-to-back steps after a warm-up, `--rounds` times, plain and guarded alternating;
the median round is reported.  One step streams 0.58 GB of p, g, m, v, more than twice the 256 MiB Infinity Cache, so
back-to-back steps do not find their operands cached; the guarded step's second read of g (146 MB) can hit that cache,
as it can in training.  Prints one JSON line:
  plain_us / guarded_us: per step; ratio; *_gbps: bytes the algorithm needs (28 B and 32 B per element) over that time;
  rounds: every round's figures, for the spread."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch


def canonical_shapes(batch):
    import main_rfn
    from RFN import RFN
    args = main_rfn.build_parser().parse_args(main_rfn.canonical_smmnist_argv(batch, 20))
    return [tuple(p.shape) for p in RFN(args).parameters()]


def make(shapes, seed, **guard):
    from rfn_hip.optim import HipAdam
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(sh, device="cuda", generator=g) * 0.05) for sh in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 0.01
    return HipAdam(ps, lr=1e-4, **guard)


def timed(opt, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_adam_guard needs a GPU"
    shapes = canonical_shapes(a.batch)
    n = sum(int(torch.Size(sh).numel()) for sh in shapes)
    plain = make(shapes, 1)
    guarded = make(shapes, 2, max_grad_norm=1.0, skip_nonfinite=True)
    for opt in (plain, guarded):
        for _ in range(a.warmup):
            opt.step()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(a.rounds):
        rounds.append({"plain_us": round(timed(plain, a.iters), 2), "guarded_us": round(timed(guarded, a.iters), 2)})
    p = statistics.median(r["plain_us"] for r in rounds)
    q = statistics.median(r["guarded_us"] for r in rounds)
    gs = guarded.guard_stats()
    assert gs["skipped_steps"] == 0 and 0.0 < gs["scale"] <= 1.0, gs
    print(json.dumps({"adam_guard": {"tensors": len(shapes), "elements": n, "plain_us": p, "guarded_us": q,
                                     "ratio": round(q / p, 3), "plain_gbps": round(28.0 * n / p / 1e3, 1),
                                     "guarded_gbps": round(32.0 * n / q / 1e3, 1), "grad_norm": gs["grad_norm"],
                                     "scale": gs["scale"]},
                      "iters": a.iters, "warmup": a.warmup, "rounds": rounds}), flush=True)


if __name__ == "__main__":
    main()
