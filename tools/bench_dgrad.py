#!/usr/bin/env python3
"""Developer tool: the few-output-channel 3x3 data-gradient kernel (csrc/dgrad_small.hip) against the generic bf16x3
implicit-GEMM kernel on the canonical level-0 / level-1 / level-2 shapes, at the full (N = 608) and the sharded (N = 76)
frame count.  RFN_PKG_DIR selects another build of the package (A/B on the same box, as bench.py)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch
from rfn_hip import ops as K

def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n

for (N, Cin, Cout, S, split) in [(N, 256, Cout, S, split) for N in (608, 76)
                                 for (Cout, S, split) in ((18, 32, 2), (36, 16, 4), (72, 8, 8))]:
    x = torch.randn(N, Cin, S, S, device="cuda")
    w = torch.randn(Cin, Cout, 3, 3, device="cuda") * 0.05
    wpk = K.pack_weight(w, flip=True)
    o1 = torch.zeros(N, split, S, S, device="cuda")
    o2 = torch.zeros(N, Cout - split, S, S, device="cuda")
    t_new = None
    if K.dgrad_small_ok(N, Cin, Cout, S, S, 3):
        t_new = timeit(lambda: K.conv3x3_smallcout(x, wpk, Cout, o1, o2, split, True, False))
    t_old = timeit(lambda: K.conv2d_raw(x, None, wpk, Cout, 3, 0, None, None, 0, out1=o1, out2=o2, cout_split=split,
                                        acc1=True, acc2=False))
    gb = 4.0 * N * S * S * (Cin + Cout) / 1e9
    print("N%d %d->%d %dx%d: dgrad_small %s   generic %.3f ms (%.0f GB/s)" %
          (N, Cin, Cout, S, S, "not supported" if t_new is None else "%.3f ms (%.0f GB/s)" % (t_new, gb / t_new * 1e3),
           t_old, gb / t_old * 1e3), flush=True)
