#!/usr/bin/env python3
"""Developer tool: the fused BatchNorm + activation + 2x2 max-pool launches (rfn_hip.ops.StepBatchNormActPoolFn) and the
fused up-sampling + concatenation (rfn_hip.ops.Up2xCatFn) against the routes they replace (StepBatchNormActFn +
F.max_pool2d; NearestUp2x + torch.cat), on the five pool shapes and the four up-sampling shapes of the canonical step
(B = 32, T = 20), forward and backward apart.  Five alternated repetitions of `--iters` calls each; per case min / median /
max ms per call and GB/s of the bytes the operation needs (inputs read once per launch that needs them, outputs written
once).  One JSON document on stdout, or in the file given as the first argument."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch
import torch.nn.functional as F

from rfn_hip import ops as K
from Utils.modules import NearestUp2x

S, B = 20, 32
POOL = [(16, 64), (32, 32), (64, 16), (128, 8), (256, 4)]                 # (C, H = W) of x [S*B, C, H, W]
UP = [(256, 256, 2), (128, 128, 4), (64, 64, 8), (32, 32, 16)]             # (Cx, Cs, h = w) of x [(S-1)*B, Cx, h, w]
REPS, ITERS = 5, int(os.environ.get("ITERS", "20"))


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def stats(ms, nbytes):
    ms = sorted(ms)
    return {"ms_min": ms[0], "ms_median": ms[len(ms) // 2], "ms_max": ms[-1], "GBps_at_median": nbytes / ms[len(ms) // 2] / 1e6}


def pool_case(C, H):
    x = torch.randn(S * B, C, H, H, device="cuda").mul_(2).add_(0.7).requires_grad_(True)
    gamma = (0.5 + torch.rand(C, device="cuda")).requires_grad_(True)
    beta = (torch.rand(C, device="cuda") - 0.5).requires_grad_(True)
    gp = torch.randn(S * B, C, H // 2, H // 2, device="cuda")
    fwd = {"fused": lambda: K.StepBatchNormActPoolFn.apply(x, gamma, beta, S, 1e-5, 1, 0.0, None)[0],
           "composed": lambda: F.max_pool2d(K.StepBatchNormActFn.apply(x, gamma, beta, S, 1e-5, 1, 0.0, None)[0], 2, 2)}
    nx = 4.0 * x.numel()
    # x read by the statistics and the apply launch, p written | x and gp read by the reduce and the apply launch, gx written
    need = {"fwd": 2.25 * nx, "bwd": 3.5 * nx}
    return fwd, (x, gamma, beta), gp, need


def up_case(Cx, Cs, h):
    N = (S - 1) * B
    x = torch.randn(N, Cx, h, h, device="cuda", requires_grad=True)
    skip = torch.randn(N, Cs, 2 * h, 2 * h, device="cuda", requires_grad=True)
    g = torch.randn(N, Cx + Cs, 2 * h, 2 * h, device="cuda")
    up = NearestUp2x()
    fwd = {"fused": lambda: K.Up2xCatFn.apply(x, skip), "composed": lambda: torch.cat((up(x), skip), 1)}
    # x and skip read, out written | the first Cx channels of g read, gx written (the skip's gradient is a view)
    need = {"fwd": 4.0 * (x.numel() + skip.numel() + g.numel()), "bwd": 4.0 * (4 * x.numel() + x.numel())}
    return fwd, (x, skip), g, need


def run(name, case):
    fwd, wrt, g, need = case
    out = {"case": name}
    t = {(r, d): [] for r in fwd for d in ("fwd", "bwd")}
    for _ in range(REPS):                                   # alternated: fused, composed, fused, ...
        for r, f in fwd.items():
            t[(r, "fwd")].append(timed(f))
            y = f()
            t[(r, "bwd")].append(timed(lambda: torch.autograd.grad(y, wrt, g, retain_graph=True)))
            del y
    for (r, d), ms in t.items():
        out["%s_%s" % (r, d)] = stats(ms, need[d])
    return out


def main():
    assert torch.cuda.is_available()
    res = {"iters": ITERS, "reps": REPS, "S": S, "B": B, "cases": []}
    for C, H in POOL:
        res["cases"].append(run("pool [%d, %d, %d, %d]" % (S * B, C, H, H), pool_case(C, H)))
    for Cx, Cs, h in UP:
        res["cases"].append(run("up2x_cat x [%d, %d, %d, %d] + skip %d" % ((S - 1) * B, Cx, h, h, Cs), up_case(Cx, Cs, h)))
    text = json.dumps(res, indent=1)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    for c in res["cases"]:
        print(c["case"], " ".join("%s %.4f" % (k, v["ms_median"]) for k, v in c.items() if k != "case"), flush=True)


if __name__ == "__main__":
    main()
