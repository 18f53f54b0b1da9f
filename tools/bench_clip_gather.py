#!/usr/bin/env python3
"""Developer tool: cost of a BAIR / KTH batch gathered on the GPU (rfn_clip_gather_u8_f32 through
rfn_hip.ops.clip_gather, data_generators.ClipLoader's path) and, in the same process, of the same batch composed from
torch operations (first + arange, index_select, permute, float32 in the batch layout, divide by 255; the divisor is a
device tensor, because torch's GPU kernel multiplies by float32(1 / 255) when it is a Python number, which gives another
float for 126 of the 256 bytes, and the two batches are compared bit for bit before anything is timed).  Prints one JSON
line; per configuration (the BAIR batch B = 32, T = 20, 3x64x64, and KTH's one stored channel as 1 and as 3 copies):
  kernel_ms_per_batch / torch_ms_per_batch: medians over `--rounds` alternating rounds of `--batches` back-to-back
      batches each, timed with HIP events after a warm-up (every round is listed as well);
  bytes_per_batch: store bytes read plus float32 bytes written; kernel_GB_per_s = bytes_per_batch / kernel time.
The store holds `--frames` random frames (default 131072: 1.6 GB at 3x64x64, several times the Infinity Cache) and every
batch reads fresh uniformly random clips through one int64 table on the device, as the loader does."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch


def torch_batch(store, first, steps, C, div):
    idx = (first[:, None] + steps).reshape(-1)
    x = store.index_select(0, idx).view(first.shape[0], steps.shape[0], *store.shape[1:]).permute(0, 1, 4, 2, 3)
    if x.shape[2] != C:
        x = x.expand(-1, -1, C, -1, -1)
    return x.to(torch.float32, memory_format=torch.contiguous_format) / div


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


def bench(F, B, T, Cs, C, S, batches, warmup, rounds):
    from rfn_hip import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    store = torch.randint(0, 256, (F, S, S, Cs), generator=g, dtype=torch.uint8, device="cuda")
    table = torch.randint(0, F - T + 1, ((batches + warmup) * B,), generator=g, dtype=torch.int64, device="cuda")
    steps = torch.arange(T, device="cuda")
    div = torch.full((), 255., device="cuda")
    first = table[:B]
    if not torch.equal(ops.clip_gather(store, first, T, C), torch_batch(store, first, steps, C, div)):
        raise SystemExit("clip_gather and the torch composition disagree")
    kernel, composed = [], []
    for _ in range(rounds):
        kernel.append(timed(lambda f: ops.clip_gather(store, f, T, C), table, B, batches, warmup))
        composed.append(timed(lambda f: torch_batch(store, f, steps, C, div), table, B, batches, warmup))
    nbytes = B * T * S * S * (Cs + 4 * C)
    k, t = statistics.median(kernel), statistics.median(composed)
    return {"shape": [B, T, C, S, S], "stored_channels": Cs, "store_frames": F, "bytes_per_batch": nbytes,
            "kernel_ms_per_batch": round(k, 4), "kernel_GB_per_s": round(nbytes / (k * 1e-3) / 1e9, 1),
            "torch_ms_per_batch": round(t, 4), "kernel_rounds_ms": [round(v, 4) for v in kernel],
            "torch_rounds_ms": [round(v, 4) for v in composed]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=131072)
    a = ap.parse_args()
    if a.batches < 100:
        ap.error("--batches must be at least 100")
    res = {"configs": [bench(a.frames, 32, 20, Cs, C, 64, a.batches, a.warmup, a.rounds)
                       for Cs, C in ((3, 3), (1, 1), (1, 3))],
           "batches": a.batches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
