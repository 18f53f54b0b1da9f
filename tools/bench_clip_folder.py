#!/usr/bin/env python3
"""Developer tool: what `--choose_data folder` costs on the GPU.  Prints one JSON line.

gather: the BAIR-sized batch B = 32, T = 20, 3x64x64 from a store of `--frames` random frames (default 131072: 1.6 GB,
    several times the Infinity Cache), every batch reading fresh uniformly random clips through one int64 table, as the
    loader does.  Four variants alternate inside each of `--rounds` rounds, `--batches` back-to-back batches each, timed
    with HIP events after a warm-up: the existing ops.clip_gather; ops.clip_gather_aug with no flags; with every row
    mirrored and reversed; with step 2.  Per variant the median, minimum and maximum over the rounds in ms per batch,
    and GB/s = (store bytes read + float32 bytes written) / median.  `inside_existing_spread` says whether a variant's
    median lies inside the existing kernel's own min-max of this call; `ratio` is median over the existing median.
    The outputs are compared before anything is timed (no flags: bit for bit the existing kernel; mirrored and reversed:
    its flip in x and t).
ingest: `--ingest_frames` (default 10000) frames 120x160x1 resampled to 64x64 over the centred 120x120 window:
    upload + ops.frames_resize + download in chunks, as clips.pack_resized_or_load does, the kernel alone (HIP events),
    and, for information, PIL's Image.resize(..., BOX) of the cropped frames on the host."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
import numpy as np
import torch


def timed(fn, table, B, batches, warmup):
    for i in range(warmup):
        fn(table[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(batches):
        fn(table[(warmup + i) * B:(warmup + i + 1) * B])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / batches


def bench_gather(F, B, T, C, S, batches, warmup, rounds):
    from rfn_hip import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    store = torch.randint(0, 256, (F, S, S, C), generator=g, dtype=torch.uint8, device="cuda")
    # starts that are valid for step 2 as well: all variants read the same table
    table = torch.randint(0, F - 2 * (T - 1), ((batches + warmup) * B,), generator=g, dtype=torch.int64, device="cuda")
    both = torch.full((B,), 3, dtype=torch.int32, device="cuda")
    variants = [("clip_gather", lambda f: ops.clip_gather(store, f, T, C)),
                ("aug_no_flags", lambda f: ops.clip_gather_aug(store, f, T, C)),
                ("aug_mirror_reverse", lambda f: ops.clip_gather_aug(store, f, T, C, flags=both)),
                ("aug_step2", lambda f: ops.clip_gather_aug(store, f, T, C, step=2))]
    first = table[:B]
    want = variants[0][1](first)
    if not torch.equal(variants[1][1](first), want) or not torch.equal(variants[2][1](first), want.flip(-1).flip(1)):
        raise SystemExit("clip_gather_aug disagrees with clip_gather")
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(timed(fn, table, B, batches, warmup))
    nbytes = B * T * S * S * (C + 4 * C)
    base = times["clip_gather"]
    out = {"shape": [B, T, C, S, S], "store_frames": F, "bytes_per_batch": nbytes, "batches": batches, "rounds": rounds}
    for name, _ in variants:
        v = times[name]
        m = statistics.median(v)
        out[name] = {"median_ms": round(m, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                     "GB_per_s": round(nbytes / (m * 1e-3) / 1e9, 1), "ratio": round(m / statistics.median(base), 4),
                     "inside_existing_spread": bool(min(base) <= m <= max(base)), "rounds_ms": [round(t, 4) for t in v]}
    return out


def bench_ingest(F, rounds):
    from rfn_hip import ops
    from data_generators import clips
    src = np.random.default_rng(0).integers(0, 256, (F, 120, 160, 1), dtype=np.uint8)
    window = ops.resize_window(120, 160, 64, 64, "crop")
    per = max(1, clips.RESIZE_CHUNK_BYTES // (120 * 160))

    def ingest():
        return np.concatenate([ops.frames_resize(torch.from_numpy(src[k:k + per]).cuda(), 64, 64, 1, window).cpu().numpy()
                               for k in range(0, F, per)])

    got = ingest()
    whole, kernel = [], []
    dev = torch.from_numpy(src[:per]).cuda()
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ingest()
        whole.append(time.perf_counter() - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.frames_resize(dev, 64, 64, 1, window)
        e1.record()
        torch.cuda.synchronize()
        kernel.append(e0.elapsed_time(e1) * 1e-3 * F / dev.shape[0])
    from PIL import Image
    n_pil = min(F, 1000)
    t0 = time.perf_counter()
    pil = np.stack([np.asarray(Image.fromarray(a[:, 20:140, 0]).resize((64, 64), Image.BOX)) for a in src[:n_pil]])
    t_pil = (time.perf_counter() - t0) * F / n_pil
    diff = np.abs(pil.astype(np.int32) - got[:n_pil, :, :, 0].astype(np.int32))
    nbytes = F * (120 * 120 + 64 * 64)
    k = statistics.median(kernel)
    return {"frames": F, "source": [120, 160, 1], "target": [64, 64, 1], "window": list(window), "frames_per_upload": per,
            "upload_resize_download_s": round(statistics.median(whole), 4), "kernel_s": round(k, 6),
            "kernel_GB_per_s": round(nbytes / k / 1e9, 1), "kernel_rounds_s": [round(v, 6) for v in kernel],
            "pil_box_host_s": round(t_pil, 4), "pil_frames_timed": n_pil,
            "max_abs_diff_to_pil_box": int(diff.max()), "pixels_differing_from_pil_box": float((diff > 0).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=131072)
    ap.add_argument("--ingest_frames", type=int, default=10000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_folder.py measures on the GPU; none is visible")
    res = {"gather": bench_gather(a.frames, 32, 20, 3, 64, a.batches, a.warmup, a.rounds),
           "ingest": bench_ingest(a.ingest_frames, a.rounds), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
