#!/usr/bin/env python3
"""Developer tool: cost of the pixel log-likelihood kernels of the baselines' bound (csrc/pixel_loglik.hip).  Prints
ONE JSON line and writes the same line to --out (default profiles/pixel_loglik_bench.json).  Profiler off.

  python tools/bench_pixel_loglik.py [--K 20 --B 32 --T 10 --reps 5 --warmup 3 --inner 20 --skip_models]

(a) rfn_hip.ops.pixel_loglik at R = K*B rows of 1x64x64 and 3x64x64, every mode ("gaussian" with the per-row
    dequantisation noise of VRNN / SRNN), against the torch chain it replaces in the models, in the same process:
    x.repeat(K, 1, 1, 1), td.Bernoulli(probs=).log_prob / td.Normal(mu, scale * ones_like(mu)).log_prob(x_rep + u) /
    MSELoss(reduction="none"), summed per row.  needed_GBs = the bytes the pass NEEDS (pred and, with noise, the uniforms
    read once, the B frames once, R floats written) over the median time; share_of_8TBs is that over 8000 GB/s.
(b) rfn_hip.ops.normal_logvar_pair at B = 32, Z = 10 and 64 against the two td.Normal(mu, exp(logvar / 2))
    .log_prob(z).sum(-1) chains.  Both sides are launch-bound: the figure is host enqueue time per call as much as
    device time, which is what the k loop of SVG's bound pays.
(c) one elbo_importance_weighting(x, K) call (B sequences of T frames, 64x64 gray, eval mode, no_grad) of main_vrnn.py's
    default model with --loss_type bernoulli (its default "mol" has the mol_nll kernel and takes neither route) and of
    main_svg.py's default model (mse), with RFN_PIXEL_LOGLIK=0 and =1 in the same process.  RFN_PKG_DIR=<another build
    of the package> runs the tool on that build (a parent commit has no switch: its two columns are the same code).
Every figure is the median / min / max of --reps repetitions after --warmup warm-up repetitions, the two sides
alternated repetition by repetition; a repetition of (a) and (b) times --inner back-to-back calls between two events on
the stream, a repetition of (c) one call."""
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

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3   # microseconds per call
    return once


def alternate(timers, reps, warmup):
    """{name: [microseconds] * reps}: `warmup` untimed rounds, then one repetition of each timer per round"""
    t = {k: [] for k in timers}
    for r in range(warmup + reps):
        for k, f in timers.items():
            v = f()
            if r >= warmup:
                t[k].append(v)
    return t


def bench_loglik(a, K):
    import torch
    import torch.distributions as td
    rows = []
    mse = torch.nn.MSELoss(reduction="none")
    for C in (1, 3):
        Kk, B, N = a.K, a.B, C * 64 * 64
        R = Kk * B
        g = torch.Generator(device="cuda").manual_seed(3 + C)
        pred = torch.rand(R, C, 64, 64, generator=g, device="cuda") * 0.98 + 0.01
        x = torch.randint(0, 256, (B, C, 64, 64), generator=g, device="cuda").float() / 255.0
        xb = (x > 0.5).float()
        u = torch.rand(R, C, 64, 64, generator=g, device="cuda") / 256.0
        scale = 0.7
        kernel = {"bernoulli": lambda: K.pixel_loglik(pred, xb, "bernoulli"),
                  "gaussian": lambda: K.pixel_loglik(pred, x, "gaussian", scale=scale, noise=u),
                  "mse": lambda: K.pixel_loglik(pred, x, "mse")}
        chain = {"bernoulli": lambda: td.Bernoulli(probs=pred).log_prob(xb.repeat(Kk, 1, 1, 1)).sum([1, 2, 3]),
                 "gaussian": lambda: td.Normal(pred, scale * torch.ones_like(pred)).log_prob(
                     x.repeat(Kk, 1, 1, 1) + u).sum([1, 2, 3]),
                 "mse": lambda: -mse(pred, x.repeat(Kk, 1, 1, 1)).sum([1, 2, 3])}
        timers = {}
        with torch.no_grad():
            for m in kernel:
                rel = float(((kernel[m]() - chain[m]()).abs() / chain[m]().abs()).max())
                assert rel <= 1e-5, (m, rel)     # faster and different is not faster
                timers[m] = timer(kernel[m], a.inner)
                timers["torch_" + m] = timer(chain[m], a.inner)
            t = alternate(timers, a.reps, a.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        need = {m: 4.0 * (R * N * (2 if m == "gaussian" else 1) + B * N + R) for m in kernel}
        rows.append({"shape": {"K": Kk, "B": B, "C": C, "H": 64, "W": 64, "R": R, "N": N},
                     "us": {k: summary(v) for k, v in t.items()},
                     "needed_MB": {m: need[m] / 1e6 for m in kernel},
                     "needed_GBs": {m: need[m] / (med[m] * 1e-6) / 1e9 for m in kernel},
                     "share_of_8TBs": {m: need[m] / (med[m] * 1e-6) / 1e9 / PEAK_HBM_GBS for m in kernel},
                     "torch_over_kernel": {m: med["torch_" + m] / med[m] for m in kernel}})
        print("C%d  " % C + "  ".join("%s %.1f us" % (k, v) for k, v in med.items()), file=sys.stderr, flush=True)
    return rows


def bench_pair(a, K):
    import torch
    import torch.distributions as td
    rows = []
    for Z in (10, 64):
        B = a.B
        g = torch.Generator(device="cuda").manual_seed(Z)
        mu_a, z_a, mu_b, z_b = (torch.randn(B, Z, generator=g, device="cuda") for _ in range(4))
        lv_a, lv_b = (torch.rand(B, Z, generator=g, device="cuda") * 4.0 - 3.0 for _ in range(2))

        def chain():
            return (td.Normal(mu_a, torch.exp(lv_a * 0.5)).log_prob(z_a).sum([-1]),
                    td.Normal(mu_b, torch.exp(lv_b * 0.5)).log_prob(z_b).sum([-1]))
        with torch.no_grad():
            timers = {"kernel": timer(lambda: K.normal_logvar_pair(mu_a, lv_a, z_a, mu_b, lv_b, z_b), a.inner),
                      "torch": timer(chain, a.inner)}
            t = alternate(timers, a.reps, a.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        rows.append({"shape": {"B": B, "Z": Z}, "us": {k: summary(v) for k, v in t.items()},
                     "torch_over_kernel": med["torch"] / med["kernel"]})
        print("Z%d  " % Z + "  ".join("%s %.1f us" % (k, v) for k, v in med.items()), file=sys.stderr, flush=True)
    return rows


def bench_bound(a):
    import torch
    import main_svg
    import main_vrnn
    from SVG import SVG
    from VRNN import VRNN
    dims = "--batch_size %d --x_dim %d 1 64 64 --condition_dim %d 1 64 64" % (a.B, a.B, a.B)
    rows = []
    for name, cls, main, flags in (("vrnn", VRNN, main_vrnn, dims + " --loss_type bernoulli"), ("svg", SVG, main_svg, dims)):
        torch.manual_seed(1)
        m = cls(main.build_parser().parse_args(flags.split())).to("cuda").eval()
        g = torch.Generator(device="cuda").manual_seed(2)
        x = (torch.rand(a.B, a.T, 1, 64, 64, generator=g, device="cuda") > 0.5).float()
        values = {}

        def call(env):
            def run():
                os.environ["RFN_PIXEL_LOGLIK"] = env
                torch.manual_seed(4)
                with torch.no_grad():
                    values[env] = float(m.elbo_importance_weighting(x, a.K))
            return run
        before = os.environ.get("RFN_PIXEL_LOGLIK")
        try:
            t = alternate({"torch_chain_0": timer(call("0"), 1), "kernels_1": timer(call("1"), 1)}, a.reps, a.warmup)
        finally:
            os.environ.pop("RFN_PIXEL_LOGLIK", None)
            if before is not None:
                os.environ["RFN_PIXEL_LOGLIK"] = before
        med = {k: statistics.median(v) for k, v in t.items()}
        rows.append({"model": name, "flags": flags, "K": a.K, "B": a.B, "T": a.T, "us": {k: summary(v) for k, v in t.items()},
                     "bound": {"torch_chain_0": values["0"], "kernels_1": values["1"]},
                     "torch_chain_over_kernels": med["torch_chain_0"] / med["kernels_1"]})
        print("%s  " % name + "  ".join("%s %.0f us" % (k, v) for k, v in med.items()), file=sys.stderr, flush=True)
        del m
        torch.cuda.empty_cache()
    return rows


def main(a):
    import torch
    from rfn_hip import ops as K
    assert torch.cuda.is_available(), "bench_pixel_loglik.py needs a GPU"
    out = {"tool": "bench_pixel_loglik", "package": os.path.relpath(PKG, ROOT),
           "protocol": "median/min/max of %d alternated repetitions after %d warm-up repetitions; (a), (b): %d back-to-back "
                       "calls between stream events per repetition; (c): one call per repetition; profiler off"
                       % (a.reps, a.warmup, a.inner), "hbm_peak_GBs": PEAK_HBM_GBS}
    if hasattr(K, "pixel_loglik"):
        out["pixel_loglik"] = bench_loglik(a, K)
        out["normal_logvar_pair"] = bench_pair(a, K)
    if not a.skip_models:
        out["elbo_importance_weighting"] = bench_bound(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=20)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip_models", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_loglik_bench.json"))
    main(ap.parse_args())
