#!/usr/bin/env python3
"""Developer tool: cost of rendering Stochastic Moving MNIST on the GPU (rfn_moving_mnist_render_f32 through
data_generators.MovingMNISTLoader's path, rfn_hip.ops.moving_mnist_render).  Prints one JSON line:
  gpu:  us per canonical batch (B = 32, T = 20, 64x64, 2 digits, stochastic walk; C = 1 and the C = 3 variant) from HIP
        events over `--batches` back-to-back batches after a warm-up, bytes written per batch and the implied GB/s;
  cpu:  for context, ms per batch of the CPU SyntheticMovingMNIST + DataLoader path (--synthetic_data) at
        `--num_workers` workers.
The digit table is random bytes of MNIST's train-split shape (60000 x 28 x 28): the kernel's cost does not depend on
the pixel values."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch


def time_gpu(digits, B, T, C, S, nd, L, batches, warmup):
    from rfn_hip import ops
    args = (digits, B, T, C, S, nd, L, False, 0, 0)
    for i in range(warmup):
        ops.moving_mnist_render(*args, i * B)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(batches):
        ops.moving_mnist_render(*args, (warmup + i) * B)
    e1.record()
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / batches
    nbytes = 4 * B * T * C * S * S
    return {"shape": [B, T, C, S, S], "num_digits": nd, "us_per_batch": round(us, 2), "bytes_written": nbytes,
            "GB_per_s": round(nbytes / (us * 1e-6) / 1e9, 1)}


def time_cpu(B, T, S, nd, L, workers, batches):
    from torch.utils.data import DataLoader
    from data_generators import SyntheticMovingMNIST
    ds = SyntheticMovingMNIST(seq_len=T, image_size=S, digit_size=28, num_digits=nd, step_length=L, channels=1,
                              length=B * (batches + 4), seed=0)
    ld = DataLoader(ds, batch_size=B, num_workers=workers, shuffle=True, drop_last=True)
    it = iter(ld)
    for _ in range(2):   # worker start-up
        next(it)
    t0 = time.perf_counter()
    n = 0
    for _ in range(batches):
        next(it)
        n += 1
    return {"shape": [B, T, 1, S, S], "num_workers": workers, "ms_per_batch": round(1e3 * (time.perf_counter() - t0) / n, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--cpu_batches", type=int, default=20)
    a = ap.parse_args()
    if a.batches < 200:
        ap.error("--batches must be at least 200")
    g = torch.Generator().manual_seed(0)
    digits = torch.randint(0, 256, (60000, 28, 28), generator=g, dtype=torch.uint8).cuda()
    res = {"gpu": [time_gpu(digits, 32, 20, C, 64, 2, 4, a.batches, a.warmup) for C in (1, 3)],
           "cpu_synthetic_dataloader": time_cpu(32, 20, 64, 2, 4, a.num_workers, a.cpu_batches),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
