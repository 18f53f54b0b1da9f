#!/usr/bin/env python3
"""Developer tool: the synchronized Moving MNIST render (rfn_moving_mnist_sync_render_f32) next to the plain one
(rfn_moving_mnist_render_f32), and how long Evaluator.param_plots takes end to end.  Prints one JSON line:
  plain, sync:  us per batch of B = 32, T = 30, 64x64, 2 digits, C = 1, stochastic walk: the median of `--repeats` (5)
                measurements with their min / max, each measurement HIP events over `--batches` back-to-back batches
                after a warm-up; sync with its trajectory and hit outputs off (the plain entry's work) and on;
  sync_over_plain: the ratio of the medians;
  param_plots:  (with --param_plots) seconds of one Evaluator.param_plots call after a warm-up call: 400 synchronized
                sequences of 30 frames at 64x64 in batches of 32 through a small RFN (random weights; the smoke
                test's configuration: z 4x16x16, h 8, L = 2, K = 2), its three PNG files written to a temporary
                folder.  The MNIST files are random bytes of the test split's shape, in torchvision's raw layout.
The digit table is random bytes: the kernels' cost does not depend on the pixel values."""
import argparse, contextlib, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
import torch

SHAPE = dict(B=32, T=30, C=1, S=64, nd=2, L=4)


def time_render(render, digits, batches, warmup, repeats, **kw):
    s = SHAPE
    args = (digits, s["B"], s["T"], s["C"], s["S"], s["nd"], s["L"], False, 0, 0)
    for i in range(warmup):
        render(*args, i * s["B"], **kw)
    torch.cuda.synchronize()
    us = []
    for r in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(batches):
            render(*args, (warmup + r * batches + i) * s["B"], **kw)
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / batches)
    return {"us_per_batch_median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def write_random_mnist(root, n=10000):
    import numpy as np
    d = os.path.join(root, "MNIST", "raw")
    os.makedirs(d, exist_ok=True)
    images = np.random.RandomState(0).randint(0, 256, size=(n, 28, 28)).astype(np.uint8)
    with open(os.path.join(d, "t10k-images-idx3-ubyte"), "wb") as f:
        f.write(b"".join(v.to_bytes(4, "big") for v in (2051, n, 28, 28)) + images.tobytes())


def time_param_plots(tmp):
    import __graft_entry__ as ge
    from RFN import RFN
    from RFN.trainer import Solver
    from evaluation_metrics import Evaluator
    B, S = 32, 64
    write_random_mnist(tmp)
    args = ge._tiny_args()
    for k, v in dict(batch_size=B, x_dim=[B, 1, S, S], condition_dim=[B, 1, S, S], n_bits=8,
                     n_epochs=1, learning_rate=1e-3, verbose=False, path="/" + os.path.relpath(tmp, os.getcwd()) + "/",
                     patience_lr=1, factor_lr=0.5, min_lr=0.0, patience_es=1, beta_max=0.5, beta_min=0.5, beta_steps=10,
                     choose_data="mnist", n_frames=30, digit_size=28, step_length=4, num_digits=2, image_size=S,
                     preprocess_range="0.5", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=25,
                     n_conditions=5, scheduler_type="linear", use_validation_set=False, mnist_root=tmp).items():
        setattr(args, k, v)
    torch.manual_seed(0)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.model = RFN(args).cuda().train()
    with torch.no_grad():
        s.model.loss(s.preprocess(torch.rand(B, 4, 1, S, S).cuda()), 0)   # data dependent init
    ev = Evaluator(s, args)
    out = os.path.join(tmp, "figures")
    with contextlib.redirect_stdout(sys.stderr):   # param_plots prints its two lines; stdout is the JSON line's
        ev.param_plots(out, 5, n_sequences=64)    # warm-up: two batches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = ev.param_plots(out, 5)
        torch.cuda.synchronize()
    return {"seconds": round(time.perf_counter() - t0, 3), "sequences": 400, "batch_size": B, "frames": 30,
            "image_size": S, "files": [os.path.basename(p) for p in paths]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--param_plots", action="store_true")
    a = ap.parse_args()
    if a.batches < 200:
        ap.error("--batches must be at least 200")
    from rfn_hip import ops
    g = torch.Generator().manual_seed(0)
    digits = torch.randint(0, 256, (60000, 28, 28), generator=g, dtype=torch.uint8).cuda()
    t = lambda render, **kw: time_render(render, digits, a.batches, a.warmup, a.repeats, **kw)
    res = {"shape": [SHAPE[k] for k in ("B", "T", "C", "S", "S")], "num_digits": SHAPE["nd"],
           "plain": t(ops.moving_mnist_render), "sync": t(ops.moving_mnist_sync_render),
           "sync_with_traj_and_hit": t(ops.moving_mnist_sync_render, trajectories=True, hits=True)}
    res["sync_over_plain"] = round(res["sync"]["us_per_batch_median"] / res["plain"]["us_per_batch_median"], 4)
    if a.param_plots:
        with tempfile.TemporaryDirectory(dir=os.getcwd()) as tmp:
            res["param_plots"] = time_param_plots(tmp)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
