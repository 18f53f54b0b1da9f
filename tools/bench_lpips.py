#!/usr/bin/env python3
"""Developer tool: cost of LPIPS on the AlexNet trunk (rfn_lpips_alex_features_u8 / rfn_lpips_alex_distance through
rfn_hip.ops) for N = 32 x 10 frame pairs of 1x64x64 and 3x64x64, with seeded random weights.  Prints one JSON line:
  hip:    us per trunk pass over the N frames and per head launch (HIP events over `reps` back-to-back calls);
  torch:  the same two figures for a plain torch-on-GPU evaluation (F.conv2d / F.max_pool2d, float32) of the same
          weights."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch
import torch.nn.functional as F

CHANNELS = (64, 192, 384, 256, 256)
CONVS = ((0, 3, 11, 4, 2), (3, 64, 5, 1, 2), (6, 192, 3, 1, 1), (8, 384, 3, 1, 1), (10, 256, 3, 1, 1))


def random_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    st = {}
    for l, (idx, cin, ks, _, _) in enumerate(CONVS):
        st["features.%d.weight" % idx] = torch.randn(CHANNELS[l], cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        st["features.%d.bias" % idx] = torch.randn(CHANNELS[l], generator=g) * 0.1
    for l, c in enumerate(CHANNELS):
        st["lin%d.model.1.weight" % l] = torch.rand(1, c, 1, 1, generator=g)
    return st


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 2)


def torch_trunk(st, x):
    x = x.float()
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    x = x / 255 * 2 - 1
    x = (x - st["shift"]) / st["scale"]
    taps = []
    for l, (idx, _, _, stride, pad) in enumerate(CONVS):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, st["features.%d.weight" % idx], st["features.%d.bias" % idx], stride=stride, padding=pad))
        taps.append(x)
    return taps


def torch_head(st, fa, fb):
    d = 0
    for l, (x, y) in enumerate(zip(fa, fb)):
        nx = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + 1e-10)
        ny = y / (torch.sqrt((y * y).sum(1, keepdim=True)) + 1e-10)
        d = d + (st["lin%d.model.1.weight" % l] * (nx - ny) ** 2).sum(1).mean((1, 2))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=320)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lpips needs a GPU"
    from rfn_hip import ops
    st = random_state()
    w = ops.lpips_alex_pack(st, "cuda")
    dst = {k: v.cuda() for k, v in st.items()}
    dst["shift"] = torch.tensor((-.030, -.088, -.188), device="cuda").view(1, 3, 1, 1)
    dst["scale"] = torch.tensor((.458, .448, .450), device="cuda").view(1, 3, 1, 1)
    rows = []
    for C in (1, 3):
        g = torch.Generator().manual_seed(C)
        x = torch.randint(0, 256, (a.frames, C, 64, 64), generator=g, dtype=torch.uint8).cuda()
        y = torch.randint(0, 256, (a.frames, C, 64, 64), generator=g, dtype=torch.uint8).cuda()
        fx, fy = ops.lpips_alex_features(w, x), ops.lpips_alex_features(w, y)
        tx, ty = torch_trunk(dst, x), torch_trunk(dst, y)
        d_hip, d_torch = ops.lpips_alex_distance(w, fx, fy), torch_head(dst, tx, ty)
        rows.append({"shape": [a.frames, C, 64, 64],
                     "hip": {"trunk_us": timed(lambda: ops.lpips_alex_features(w, x), a.reps),
                             "head_us": timed(lambda: ops.lpips_alex_distance(w, fx, fy), a.reps)},
                     "torch": {"trunk_us": timed(lambda: torch_trunk(dst, x), a.reps),
                               "head_us": timed(lambda: torch_head(dst, tx, ty), a.reps)},
                     "max_rel_diff_hip_vs_torch": float(((d_hip - d_torch).abs() / d_torch).max())})
    print(json.dumps({"lpips_alex": rows, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
