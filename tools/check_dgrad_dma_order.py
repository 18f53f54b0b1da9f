#!/usr/bin/env python3
"""Developer tool: compile csrc/dgrad_small.hip to gfx950 assembly and check, for every instantiation of
dgrad_small_kernel and every stretch of code between two s_barrier, that the weight LDS-DMA pieces (global_load_lds) are
not interleaved with the image loads (buffer_load) and that the last vmcnt wait before the barrier allows no more
operations in flight than image loads were issued after the last DMA piece (vector-memory operations complete in issue
order, so the DMA has then landed).  A stretch that ends in vmcnt(0) is safe whatever its order.  Exit status 1 on a
violation."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(ROOT, "recurrent-flows-msc_amd", "csrc", "dgrad_small.hip")
with tempfile.TemporaryDirectory() as d:
    out = os.path.join(d, "k.s")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-fPIC", "-std=c++17",
                           "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-S", "--cuda-device-only",
                           src, "-o", out], stderr=subprocess.DEVNULL)
    s = open(out).read()
bad = 0
for m in re.finditer(r"^_Z18dgrad_small_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E\w+:", s, re.M):
    body = s[m.end():s.index("s_endpgm", m.end())].split("\n")
    seg, rows = [], []
    for l in body + ["s_barrier"]:
        t = l.strip()
        if t.startswith("global_load_lds"):
            seg.append("D")
        elif t.startswith("buffer_load"):
            seg.append("L")
        elif t.startswith("s_waitcnt") and "vmcnt" in t:
            seg.append(int(re.search(r"vmcnt\((\d+)\)", t).group(1)))
        elif t.startswith("s_barrier"):
            if "D" in seg:
                first = seg.index("D")
                last = len(seg) - 1 - seg[::-1].index("D")
                after = seg[last + 1:].count("L")
                waits = [o for o in seg[last + 1:] if isinstance(o, int)]
                w = waits[-1] if waits else None
                ok = w is not None and (w == 0 or (w <= after and "L" not in seg[first:last]))
                rows.append("DMA %d, loads after %d, vmcnt(%s)%s" % (seg.count("D"), after, w, "" if ok else "  <-- UNSAFE"))
                bad += not ok
            seg = []
    print("<%s,%s,%s,%s>: %s" % (m.group(1), m.group(2), m.group(3), m.group(4), "; ".join(rows)))
sys.exit(1 if bad else 0)
