#!/usr/bin/env python3
"""Developer tool: time of one curve figure of the evaluation (1900 x 500 pixels, three panels, 9 series of 25 points
with bands and markers: Evaluator.plot_eval_values over nine experiments) through rfn_hip.ops.render_chart.  Prints one
JSON line:
  kernel_ms: the median over `--rounds` (default 5) rounds, each the mean of `--launches` back-to-back
      rfn_chart_render_u8 launches on a table already on the device, timed with HIP events after a warm-up (every
      round is listed as well);
  host_ms: the median over the same rounds of ONE whole figure on the host clock, ending in a device synchronise:
      statistics -> display list -> upload -> kernel -> scanlines on the host -> PNG bytes (zlib), as the Evaluator
      writes it;
  records: the length of the display list; bytes_out: the scanline bytes written."""
import argparse, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch


def eval_dict(seed, n=256, t=25):
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(n, t, generator=g) * torch.linspace(1.0, 0.6, t)
    return {"SSIM_values": r(0.5, 0.9), "PSNR_values": r(15, 25), "LPIPS_values": r(0.1, 0.4),
            "SSIM_std_mean": r(0.4, 0.8), "PSNR_std_mean": r(12, 22), "LPIPS_std_mean": r(0.2, 0.5), "temperature": 0.7}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from evaluation_metrics.curves import build_figures
    from rfn_hip import chart, ops
    from Utils.png import write_png
    entries = [("experiment %d" % i, eval_dict(i)) for i in range(9)]
    fig = build_figures(entries, 5, 10)["eval_plots_max"]
    dl = chart.build_display_list(fig)
    table = torch.from_numpy(dl.table).cuda()
    out = torch.empty((dl.height, 1 + 3 * dl.width), dtype=torch.uint8, device="cuda")
    for _ in range(a.warmup):
        ops.render_chart(table, dl.height, dl.width, scanlines=True, out=out)
    torch.cuda.synchronize()
    kernel, host = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                ops.render_chart(table, dl.height, dl.width, scanlines=True, out=out)
            e1.record()
            torch.cuda.synchronize()
            kernel.append(e0.elapsed_time(e1) / a.launches)
            t0 = time.perf_counter()
            f = build_figures(entries, 5, 10)["eval_plots_max"]
            write_png(os.path.join(tmp, "figure.png"), ops.render_chart(f, scanlines=True))   # .cpu() synchronises
            host.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"figure": [dl.height, dl.width], "series": 9, "points": 25, "records": int(dl.table.shape[0]),
                      "bytes_out": out.numel(), "kernel_ms": round(statistics.median(kernel), 4),
                      "kernel_rounds_ms": [round(v, 4) for v in kernel], "host_ms": round(statistics.median(host), 2),
                      "host_rounds_ms": [round(v, 2) for v in host], "launches": a.launches, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
