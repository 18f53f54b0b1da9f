#!/usr/bin/env python3
"""Developer tool: cost of the mixture-of-discretized-logistics kernels (csrc/mol.hip).  Prints ONE JSON line.

  python tools/bench_mol.py [--N 608 --H 64 --M 10 --reps 5]

Per colour mode (C = 1 and C = 3): rfn_hip.ops.mol_nll forward, forward + backward and mol_sample, against the same
likelihood written with torch ops (tests/mol_ref.py, the tests' restatement, here in float32 on the GPU: forward under
no_grad, forward + backward through autograd, and its sampler).  Inputs follow the recipe of tests/golden/mol*.pt, so
every branch of the likelihood is taken.  Each figure is the median / min / max of `--reps` repetitions, kernels and op
chain alternated repetition by repetition; a repetition times `--inner` back-to-back calls between two events on the
stream (the launches of a call are far shorter than its kernels, so the queue never runs dry) after two warm-up calls.
Profiler off.  GB/s = the bytes a pass NEEDS (l and x read once, nll_pix and the log-sum-exp written; backward: l, x, the
log-sum-exp and the upstream read, dl written; sampler: the mixture logits, the chosen component's rows, the uniforms,
the frame) over the median time."""
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


def inputs(N, C, M, H, W, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = 3 if C == 3 else 2
    k = torch.randint(0, 256, (N, C, H, W), generator=g, device="cuda")
    k[:, :, 0], k[:, :, -1] = 0, 255
    x = 2.0 * k.float() / 255.0 - 1.0
    l = torch.empty(N, M * (1 + P * C), H, W, device="cuda")
    rn = lambda: torch.randn(N, M, H, W, generator=g, device="cuda")
    l[:, :M] = 2.0 * rn()
    for c in range(C):
        o = M + c * P * M
        l[:, o:o + M] = x[:, c:c + 1] + 0.15 * rn()
        l[:, o + M:o + 2 * M] = torch.rand(N, M, H, W, generator=g, device="cuda") * 7.5 - 8.0
        if P == 3:
            l[:, o + 2 * M:o + 3 * M] = rn()
    u_mix = torch.empty(N, H, W, M, device="cuda").uniform_(1e-5, 1 - 1e-5, generator=g)
    u_x = torch.empty(N, H, W, C, device="cuda").uniform_(1e-5, 1 - 1e-5, generator=g)
    return x, l, u_mix, u_x


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
    from tests import mol_ref as R
    assert torch.cuda.is_available(), "bench_mol.py needs a GPU"
    rows = []
    for C in (1, 3):
        N, M, H = a.N, a.M, a.H
        x, l, u_mix, u_x = inputs(N, C, M, H, H, 7 + C)
        Cl, HW = l.shape[1], H * H
        lg = l.clone().requires_grad_(True)
        up = torch.rand(N, device="cuda") + 0.5

        def k_fwd():
            with torch.no_grad():
                K.mol_nll(x, l, reduce="frame")

        def k_fwd_bwd():
            lg.grad = None
            (K.mol_nll(x, lg, reduce="frame") * up).sum().backward()

        def k_sample():
            K.mol_sample(l, u_mix, u_x)

        def t_fwd():
            with torch.no_grad():
                R.nll_pix(x, l).reshape(N, -1).sum(1)

        def t_fwd_bwd():
            lg.grad = None
            (R.nll_pix(x, lg).reshape(N, -1).sum(1) * up).sum().backward()

        def t_sample():
            with torch.no_grad():
                R.sample(l, u_mix, u_x)

        timers = {"fwd": timer(k_fwd, a.inner), "fwd_bwd": timer(k_fwd_bwd, a.inner), "sample": timer(k_sample, a.inner),
                  "torch_fwd": timer(t_fwd, 1), "torch_fwd_bwd": timer(t_fwd_bwd, 1), "torch_sample": timer(t_sample, 1)}
        t = {k: [] for k in timers}
        for _ in range(a.reps):      # alternated: one repetition of each, then the next round
            for k, f in timers.items():
                t[k].append(f())
        px = 4.0 * N * HW
        need = {"fwd": px * (Cl + C + 2), "fwd_bwd": px * (Cl + C + 2) + px * (2 * Cl + C + 1) + 4.0 * N,
                "sample": px * (M + (3 if C == 3 else 2) * C + M + 2 * C)}   # (logits, the chosen rows, uniforms, frame)
        med = {k: statistics.median(v) for k, v in t.items()}
        rows.append({"shape": {"N": N, "C": C, "M": M, "H": H, "W": H, "Cl": Cl},
                     "us": {k: summary(v) for k, v in t.items()},
                     "needed_GBs": {k: need[k] / (med[k] * 1e-6) / 1e9 for k in need},
                     "bwd_alone_us_by_difference": med["fwd_bwd"] - med["fwd"],
                     "torch_over_kernel": {k: med["torch_" + k] / med[k] for k in need}})
        print("C%d  " % C + "  ".join("%s %.0f us" % (k, v) for k, v in med.items()), file=sys.stderr, flush=True)
        del x, l, u_mix, u_x, lg
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "bench_mol", "protocol": "median/min/max of %d alternated repetitions, each %d back-to-back "
                      "calls between stream events (op chain: 1), two warm-up calls, profiler off" % (a.reps, a.inner),
                      "hbm_peak_GBs": PEAK_HBM_GBS, "rows": rows}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=608)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--M", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    main(ap.parse_args())
