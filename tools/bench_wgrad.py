"""developer probe: the big weight-gradient GEMMs of the shallow flow levels (N = 608 frames), LDS-DMA ring kernel
against the register-staged one.  python tools/bench_wgrad.py   (RFN_WGRAD_DMA=0 for the register-staged kernel)
python tools/bench_wgrad.py level [frames ...]: the three weight gradients of a Glow step at flow levels 0 - 2 (K = 10
steps per level), as ten single launches and as one grouped launch, GEMM launches only (HIP events of rfn_hip.lib.PROFILE).
conv3 gets a second row, `mirrored`: tap scatter + GEMM (both launches counted) beside the one mirrored launch that shifts
the gradient while staging.  python tools/bench_wgrad.py conv3 [frames ...]: the conv3 rows only.
python tools/bench_wgrad.py rows [frames ...]: conv1 and conv3 of the two deepest levels (4 x 4 and 2 x 2 maps, ten groups):
the expanding route -- its im2col / tap-scatter passes and its GEMM reported apart -- beside the one short-row launch
(builds without the short-row forms print the expanding route only).
python tools/bench_wgrad.py band [frames ...]: the 3x3 weight gradients of the few-channel layers (extractor / upscaler
blocks; both orientations), all launches of the old route (implicit, or tap scatter + GEMM; RFN_WGRAD_BAND=0) beside the
one band launch, ms and TB/s of the operand bytes (builds without the band kernel print the old route only).
RFN_PKG_DIR selects another build of the package (A/B on the same box, as bench.py)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")):
    sys.path.insert(0, p)
import torch
from rfn_hip import ops as K
from rfn_hip import lib as L


def run(F_, M, Nc, S, reps=10):
    g = torch.Generator().manual_seed(0)
    a = torch.randn(F_, M, S, S, generator=g).cuda()
    b = torch.randn(F_, Nc, S, S, generator=g).cuda()
    K.gemm_wgrad(a, b, M, Nc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        K.gemm_wgrad(a, b, M, Nc)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    by = 4.0 * F_ * S * S * (M + Nc)
    print("F%d %dx%d %dx%d  %s  %.3f ms  %.2f TB/s  %.0f TFLOP/s" % (
        F_, M, Nc, S, S, K.kernel_label("rfn_gemm_wgrad_kernel_label_bf16x3", M, Nc, M * S * S, Nc * S * S, 0, F_,
                                        S * S).split("<")[0], dt * 1e3, by / dt / 1e12,
        2.0 * F_ * S * S * M * Nc / dt / 1e12), flush=True)


def run_implicit(F_, C1, C2, S, reps=10):
    g = torch.Generator().manual_seed(0)
    z = torch.randn(F_, C1, S, S, generator=g).cuda()
    cond = torch.randn(F_, C2, S, S, generator=g).cuda()
    ga = torch.randn(F_, 256, S, S, generator=g).cuda()
    K.conv2d_wgrad(z, cond, ga, 256, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        K.conv2d_wgrad(z, cond, ga, 256, 3)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    by = 4.0 * F_ * S * S * (256 + C1 + C2)
    print("F%d 256x%d %dx%d implicit3x3  %.3f ms  %.2f TB/s" % (F_, 9 * (C1 + C2), S, S, dt * 1e3, by / dt / 1e12), flush=True)


def _wgrad_ms(fn, reps=5, also=()):
    """fn() reps times after one warm-up: (median over the reps of the summed weight-gradient GEMM time in ms, launches
    per call, label of the first); `also`: shell launches (by name) that count as well"""
    fn()
    torch.cuda.synchronize()
    sums = []
    for _ in range(reps):
        L.PROFILE = []
        fn()
        torch.cuda.synchronize()
        ev = [(m[1], e0.elapsed_time(e1)) for (_, m, e0, e1) in L.PROFILE if m is not None and (m[0] == "wgrad" or m[1] in also)]
        L.PROFILE = None
        sums.append(sum(t for _, t in ev))
    sums.sort()
    return sums[len(sums) // 2], len(ev), ev[0][0]


def level(F_, G=10, only=None):
    """conv1 (3x3, C/2 + cond -> 256), conv2 (1x1, 256 -> 256), conv3 (3x3, 256 -> C) of levels 0 - 2"""
    torch.manual_seed(0)
    rn = lambda *shape: torch.randn(*shape, device="cuda")
    for lvl, (C, Cc, S) in enumerate([(4, 16, 32), (8, 32, 16), (16, 64, 8)]):
        h = [rn(F_, 256, S, S) for _ in range(G)]       # h1 / h2 stand-ins
        gh = [rn(F_, 256, S, S) for _ in range(G)]      # gh1 / gh2 stand-ins
        z = [rn(F_, C, S, S) for _ in range(G)]
        cond = rn(F_, Cc, S, S)
        go = rn(G, F_, C, S, S)
        cases = [("conv1 256x%d" % (9 * (C // 2 + Cc)), [t[:, :C // 2] for t in z], [cond] * G, gh, 256, 3, None),
                 ("conv2 256x256", h, None, gh, 256, 1, None),
                 ("conv3 %dx256" % (9 * C), h, None, [go[i] for i in range(G)], C, 3, go)]
        for name, in1, in2, gl, Cout, ks, stacked in cases:
            if only is not None and not name.startswith(only):
                continue
            one = lambda: [K.conv2d_wgrad(in1[i], None if in2 is None else in2[i], gl[i], Cout, ks) for i in range(G)]
            grp = lambda: K.conv2d_wgrad_grouped(in1, in2, gl, Cout, ks, g_stacked=stacked)
            t1, n1, l1 = _wgrad_ms(one)
            tg, ng, lg = _wgrad_ms(grp)
            print("F%d level %d %-14s  %d singles %7.3f ms (%s)   grouped G%d %7.3f ms in %d launch (%s)" % (
                F_, lvl, name, n1, t1, l1, G, tg, ng, lg), flush=True)
            if stacked is not None:
                ts, ns, _ = _wgrad_ms(grp, also=("tap_scatter",))
                row = "F%d level %d %-14s  scatter + GEMM %7.3f ms in %d launches" % (F_, lvl, "mirrored", ts, ns)
                if hasattr(K, "zeros_conv_wgrad_grouped"):
                    tm, nm, lm = _wgrad_ms(lambda: K.zeros_conv_wgrad_grouped(in1, gl, Cout, g_stacked=stacked))
                    row += "   mirrored G%d %7.3f ms in %d launch (%s)" % (G, tm, nm, lm)
                print(row, flush=True)
        del h, gh, z, cond, go


def _parts_ms(fn, reps=5):
    """fn() reps times after one warm-up: median ms of (expansion passes, weight-gradient launches), launches per call"""
    fn()
    torch.cuda.synchronize()
    rows = []
    for _ in range(reps):
        L.PROFILE = []
        fn()
        torch.cuda.synchronize()
        ev = [(m[0], m[1], e0.elapsed_time(e1)) for (_, m, e0, e1) in L.PROFILE if m is not None]
        L.PROFILE = None
        rows.append((sum(t for k, n, t in ev if n in ("tap_scatter", "im2col3x3")), sum(t for k, n, t in ev if k == "wgrad")))
    med = lambda v: sorted(v)[len(v) // 2]
    return med([r[0] for r in rows]), med([r[1] for r in rows]), len(ev)


def rows(F_, G=10):
    """conv1 (3x3, C/2 + cond -> 256) and conv3 (3x3, 256 -> C) of levels 3 (4 x 4) and 4 (2 x 2)"""
    torch.manual_seed(0)
    rn = lambda *shape: torch.randn(*shape, device="cuda")
    has_rows = hasattr(K, "wgrad_short_rows")
    for lvl, (C, Cc, S) in ((3, (32, 128, 4)), (4, (64, 256, 2))):
        h, gh = [rn(F_, 256, S, S) for _ in range(G)], [rn(F_, 256, S, S) for _ in range(G)]
        z, cond, go = [rn(F_, C, S, S) for _ in range(G)], rn(F_, Cc, S, S), rn(G, F_, C, S, S)
        z1, gl = [t[:, :C // 2] for t in z], [go[i] for i in range(G)]
        for name, old, new in (
                ("conv1 256x%d" % (9 * (C // 2 + Cc)), lambda **kw: K.conv2d_wgrad_grouped(z1, [cond] * G, gh, 256, 3, **kw),
                 None),
                ("conv3 %dx256" % (9 * C), lambda **kw: K.zeros_conv_wgrad_grouped(h, gl, C, g_stacked=go, **kw), None)):
            tp, tg, n = _parts_ms(old)
            row = "F%d level %d %-15s passes %7.3f + GEMM %7.3f = %7.3f ms in %2d launches" % (F_, lvl, name, tp, tg, tp + tg, n)
            if has_rows:
                _, tr, nr = _parts_ms(lambda: old(short_rows=True))
                row += "   short rows %7.3f ms in %d launch" % (tr, nr)
            print(row, flush=True)
        del h, gh, z, cond, go


# (Cout, Cin, S): the implicit few-channel rows of a B = 32 step, then the Cin > Cout layers
BAND_SHAPES = ((16, 16, 64), (16, 16, 32), (32, 32, 32), (32, 16, 32), (32, 32, 16), (64, 64, 16), (64, 32, 16), (64, 64, 8),
               (128, 128, 8), (16, 64, 32), (32, 128, 16))


def _route_ms(fn, reps=7):
    """fn() reps times after a warm-up: median over the reps of the summed time of ALL its launches, launches, first label"""
    fn()
    torch.cuda.synchronize()
    sums = []
    for _ in range(reps):
        L.PROFILE = []
        fn()
        torch.cuda.synchronize()
        ev = [(m[1], e0.elapsed_time(e1)) for (_, m, e0, e1) in L.PROFILE if m is not None]
        L.PROFILE = None
        sums.append(sum(t for _, t in ev))
    return sorted(sums)[len(sums) // 2], len(ev), ev[-1][0]


def band(F_):
    torch.manual_seed(0)
    has_band = hasattr(K, "wgrad_band_min_pixels")
    for Cout, Cin, S in BAND_SHAPES:
        x, g = torch.randn(F_, Cin, S, S, device="cuda"), torch.randn(F_, Cout, S, S, device="cuda")
        by = 4.0 * F_ * S * S * (Cin + Cout)
        os.environ["RFN_WGRAD_BAND"] = "0"
        t0, n0, l0 = _route_ms(lambda: K.conv2d_wgrad(x, None, g, Cout, 3))
        row = "F%d %3dx%-4d HW%-4d  old %7.4f ms %5.2f TB/s in %d (%s)" % (F_, Cout, 9 * Cin, S * S, t0, by / t0 / 1e9, n0, l0)
        if has_band:
            os.environ["RFN_WGRAD_BAND"] = "1"
            os.environ["RFN_WGRAD_BAND_MIN_PIXELS"] = "1"
            t1, n1, l1 = _route_ms(lambda: K.conv2d_wgrad(x, None, g, Cout, 3))
            del os.environ["RFN_WGRAD_BAND_MIN_PIXELS"]
            row += "   band %7.4f ms %5.2f TB/s in %d (%s)  x%.2f" % (t1, by / t1 / 1e9, n1, l1, t0 / t1)
        print(row, flush=True)
        del x, g


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "band":
        for F_ in [int(v) for v in sys.argv[2:]] or [640, 608]:
            band(F_)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "rows":
        for F_ in [int(v) for v in sys.argv[2:]] or [608, 76]:
            rows(F_)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] in ("level", "conv3"):
        for F_ in [int(v) for v in sys.argv[2:]] or [608, 76]:
            level(F_, only="conv3" if sys.argv[1] == "conv3" else None)
        sys.exit(0)
    run_implicit(608, 2, 16, 32)
    run_implicit(608, 4, 32, 16)
    run(608, 256, 256, 32)
    run(608, 256, 256, 16)
    run(608, 36, 256, 32)
    run(608, 72, 256, 16)
    run(608, 256, 256, 8)
