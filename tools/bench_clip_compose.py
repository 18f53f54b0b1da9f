#!/usr/bin/env python3
"""Developer tool: time of one animated clip of the evaluation through rfn_hip.ops.compose_clip -- 4 sequences x 11
columns (ground truth, D = 8 draws, MEAN, SPREAD) of 64 x 64 one-channel uint8 frames, zoom 2, ring 2, T = 30: 30 frames
of 538 x 1476 pixels.  The frames are synthetic: a bright square that moves over a dark ground, each draw with its own
jitter once generation starts.  Prints one JSON line and saves it as profiles/clip_compose_bench.json.  Each figure is
the median of `--rounds` (default 5) timings after a warm-up, with their min and max:
  kernel_ms: ONE rfn_clip_compose_u8 launch, between HIP events recorded around the call on its stream (the cell
      table's upload is outside);
  torch_chain_ms: the same bytes made by torch ops on the device (sums, integer square root, repeat_interleave, slice
      assignment per cell; checked equal to the kernel's once), between HIP events;
  zlib_ms: zlib.compress (level 6) of the T frames' scanlines on the host, one frame at a time as Utils.png.write_apng
      does, on the host clock.
Three separate costs, each named for what it is; no ratio between them is formed or asserted."""
import argparse, json, os, statistics, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch

R, D, S, T, START, ZOOM, BORDER, GUTTER, GAIN = 4, 8, 64, 30, 5, 2, 2, 2, 4
BEFORE, AFTER = (0, 160, 0), (208, 0, 0)


def synthetic(seed=0, device="cuda"):
    """(truth uint8 [R, T, 1, S, S], draws uint8 [D, R, T, 1, S, S]) on `device`"""
    g = torch.Generator().manual_seed(seed)
    truth = torch.zeros(R, T, 1, S, S, dtype=torch.uint8)
    draws = torch.zeros(D, R, T, 1, S, S, dtype=torch.uint8)
    for r in range(R):
        for t in range(T):
            y, x = (3 + 2 * t + 7 * r) % (S - 16), (5 + 3 * t + 11 * r) % (S - 16)
            truth[r, t, 0, y:y + 16, x:x + 16] = 230
            for d in range(D):
                if t >= START:
                    dy, dx = (int(v) for v in torch.randint(-(t - START) // 4 - 1, (t - START) // 4 + 2, (2,), generator=g))
                else:
                    dy = dx = 0
                yy, xx = min(max(y + dy, 0), S - 16), min(max(x + dx, 0), S - 16)
                draws[d, r, t, 0, yy:yy + 16, xx:xx + 16] = 230
    return truth.to(device), draws.to(device)


def grid(truth, draws):
    from rfn_hip import ops
    cell = lambda f, mode="frame": ops.ClipCell(f, mode, gain=GAIN, switch_at=START, before=BEFORE, after=AFTER)
    return [[cell(truth[k])] + [cell(draws[d, k]) for d in range(D)] +
            [cell(draws[:, k].transpose(0, 1), "mean"), cell(draws[:, k].transpose(0, 1), "spread")] for k in range(R)]


def torch_chain(truth, draws, Hs, Ws):
    """the clip's scanlines [T, Hs, 1 + 3*Ws] by torch ops on the device"""
    Hc = ZOOM * S + 2 * BORDER
    b = draws.to(torch.int64)
    s1, s2 = b.sum(0), (b * b).sum(0)
    mean = ((s1 + D // 2) // D).to(torch.uint8)
    rad = GAIN * GAIN * (D * s2 - s1 * s1)
    root = torch.sqrt(rad.to(torch.float64)).to(torch.int64)
    root = root - (root * root > rad).to(torch.int64)
    root = root + ((root + 1) * (root + 1) <= rad).to(torch.int64)
    spread = torch.clamp(root // D, max=255).to(torch.uint8)
    out = torch.full((T, Hs, Ws, 3), 255, dtype=torch.uint8, device=truth.device)
    ring = torch.tensor([BEFORE] * START + [AFTER] * (T - START), dtype=torch.uint8, device=truth.device).view(T, 1, 1, 3)
    for k in range(R):
        cols = [truth[k]] + [draws[d, k] for d in range(D)] + [mean[k], spread[k]]
        for i, f in enumerate(cols):   # f [T, 1, S, S]
            y0, x0 = GUTTER + k * (Hc + GUTTER), GUTTER + i * (Hc + GUTTER)
            out[:, y0:y0 + Hc, x0:x0 + Hc] = ring
            z = f[:, 0].repeat_interleave(ZOOM, 1).repeat_interleave(ZOOM, 2)
            out[:, y0 + BORDER:y0 + BORDER + ZOOM * S, x0 + BORDER:x0 + BORDER + ZOOM * S] = z.unsqueeze(-1)
    lines = torch.zeros((T, Hs, 1 + 3 * Ws), dtype=torch.uint8, device=truth.device)
    lines[:, :, 1:] = out.view(T, Hs, 3 * Ws)
    return lines


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_compose_bench.json"))
    a = ap.parse_args()
    from rfn_hip import lib, ops
    truth, draws = synthetic()
    cells = grid(truth, draws)
    Hs, Ws = ops.clip_shape(R, D + 3, S, S, ZOOM, BORDER, GUTTER)
    out = torch.empty((T, Hs, 1 + 3 * Ws), dtype=torch.uint8, device="cuda")
    kw = dict(zoom=ZOOM, border=BORDER, gutter=GUTTER, scanlines=True, out=out)
    for _ in range(a.warmup):
        ops.compose_clip(cells, T, **kw)
        chain = torch_chain(truth, draws, Hs, Ws)
    torch.cuda.synchronize()
    assert torch.equal(out, chain), "the torch chain and the kernel disagree"
    kernel, torch_ms, zl = [], [], []
    host = out.cpu().numpy()
    for _ in range(a.rounds):
        lib.PROFILE = []
        ops.compose_clip(cells, T, **kw)
        torch.cuda.synchronize()
        (_, _, e0, e1), = lib.PROFILE
        lib.PROFILE = None
        kernel.append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_chain(truth, draws, Hs, Ws)
        e1.record()
        torch.cuda.synchronize()
        torch_ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        packed = sum(len(zlib.compress(host[t].tobytes(), 6)) for t in range(T))
        zl.append((time.perf_counter() - t0) * 1e3)
    line = json.dumps({"grid": [R, D + 3], "frame": [S, S], "zoom": ZOOM, "border": BORDER, "T": T, "D": D,
                       "clip": [T, Hs, Ws], "bytes_out": out.numel(), "bytes_deflated": packed,
                       "kernel_ms": stats(kernel), "torch_chain_ms": stats(torch_ms), "zlib_ms": stats(zl),
                       "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
