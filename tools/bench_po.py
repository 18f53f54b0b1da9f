"""developer probe: time the fused coupling-net kernels alone -- the forward (coupling_po_fwd) against the unfused
kernels, and the backward data-gradient chain (coupling_po_bwd) -- at the three canonical level shapes and the
BAIR-shaped level 0 (N = 608 / 76 frames).  Every row is the min / median / max over --reps repetitions of a timed loop
of --iters launches, so that two builds can be compared on one box:
    python tools/bench_po.py [--reps 5] [--iters 10] [--no-unfused]
    RFN_PKG_DIR=<other package dir> python tools/bench_po.py      (or RFN_LIB=<librfn_hip.so>, header beside it)
One JSON line per row follows the table ("PO_ROW {...}")."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")):
    sys.path.insert(0, p)
import torch
from rfn_hip import ops as K
from rfn_hip import lib as _L
if os.environ.get("RFN_LIB"):   # A/B of two builds of the library on one box
    _L.LIB_PATH = os.path.join(ROOT, os.environ["RFN_LIB"])
    if os.path.exists(os.path.join(os.path.dirname(_L.LIB_PATH), "rfn_hip.h")):
        _L.HEADER_PATH = os.path.join(os.path.dirname(_L.LIB_PATH), "rfn_hip.h")


def timed(fn, reps, iters):
    """ms per launch: [min, median, max] over `reps` timed loops of `iters` launches"""
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return min(out), statistics.median(out), max(out)


def report(shape, name, t, flops):
    print("%-22s %-12s min %.3f  med %.3f  max %.3f ms   %.1f TFLOP/s fp32-equiv" % (
        shape, name, t[0], t[1], t[2], flops / (t[1] * 1e-3) / 1e12), flush=True)
    print("PO_ROW " + json.dumps({"shape": shape, "kernel": name, "ms_min": t[0], "ms_med": t[1], "ms_max": t[2]}), flush=True)


def run(N, C, Cc, S, reps, iters, unfused_too, bwd_too):
    g = torch.Generator().manual_seed(0)
    Ch, Cin = C // 2, C // 2 + Cc
    z = torch.randn(N, C, S, S, generator=g).cuda()
    cond = torch.randn(N, Cc, S, S, generator=g).cuda()
    w1 = (torch.randn(256, Cin, 3, 3, generator=g) * 0.05).cuda()
    w2 = (torch.randn(256, 256, 1, 1, generator=g) * 0.05).cuda()
    w3 = (torch.randn(C, 256, 3, 3, generator=g) * 0.05).cuda()
    nb = (torch.randn(256, generator=g) * 0.1).cuda()
    nl = (torch.randn(256, generator=g) * 0.1).cuda()
    plan = K.POPackPlan([(w1, w2, w3)])
    plan.run()
    shape = "N%d C%d Cc%d %dx%d" % (N, C, Cc, S, S)
    def fused():
        return K.coupling_po_fwd(z, cond, plan.bufs[0], nb, nl, nb, nl, C, 1, want_masks=True)
    fl = 2.0 * N * S * S * (9 * Cin * 256 + 65536 + 9 * C * 256)
    report(shape, "fwd fused", timed(fused, reps, iters), fl)
    if bwd_too:
        masks = fused()[3]
        go = torch.randn(N, C, S, S, generator=g).cuda()
        def chain():
            return K.coupling_po_bwd(go, plan.bwd_bufs[0], nl, nl, masks, 1)
        report(shape, "bwd chain", timed(chain, reps, iters), 2.0 * N * S * S * (9 * C * 256 + 65536))
    if unfused_too:
        pk1, pk2 = K.pack_weight(w1), K.pack_weight(w2)
        w3t = w3.permute(2, 3, 0, 1).reshape(9 * C, 256, 1, 1).contiguous()
        pk3 = K.pack_weight(w3t)
        def unfused():
            h1 = K.conv2d_raw(z[:, :Ch], cond, pk1, 256, 3, 1, nb, nl, 1)
            h2 = K.conv2d_raw(h1, None, pk2, 256, 1, 1, nb, nl, 1)
            P = K.conv2d_raw(h2, None, pk3, 9 * C, 1)
            return h1, h2, P
        report(shape, "fwd unfused", timed(unfused, reps, iters), fl)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-unfused", action="store_true", help="skip the unfused forward rows")
    a = ap.parse_args()
    run(608, 4, 16, 32, a.reps, a.iters, not a.no_unfused, True)
    run(608, 8, 32, 16, a.reps, a.iters, not a.no_unfused, True)
    run(608, 16, 64, 8, a.reps, a.iters, not a.no_unfused, True)
    run(76, 12, 64, 32, a.reps, a.iters, not a.no_unfused, False)
