#!/usr/bin/env python3
"""Developer tool: cost of the I3D embedding behind the Frechet Video Distance (rfn_hip.ops.i3d_embed: resize to 224x224,
trunk, head) for 16 and 256 videos of 16x1x64x64 and 16x3x64x64, with seeded random weights.  Prints one JSON line:
  hip_ms:    ms per i3d_embed call over all the videos (HIP events over `reps` back-to-back calls after one warm-up);
  torch_ms:  the same for a plain torch-on-GPU evaluation (F.conv3d / F.max_pool3d, float32, channels-first) of the same
             folded weights on the resized input, 16 videos at a time;
  max_diff_over_rms: largest |hip - torch| over the logits of the first 16 videos, as a fraction of their RMS."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import torch
import torch.nn.functional as F


def random_state(units, seed=0):
    """a state dict in the PyTorch port's naming: convolutions randn * sqrt(2 / (Cin k^3)), gamma and var uniform
    [0.5, 1.5], beta and mean randn * 0.1, the logits bias randn * 0.1"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, u in units.items():
        cin, cout, k = u["cin"], u["cout"], u["k"]
        sd[name + ".conv3d.weight"] = torch.randn(cout, cin, k, k, k, generator=g) * (2.0 / (cin * k ** 3)) ** 0.5
        if u["bn"]:
            sd[name + ".bn.weight"] = torch.rand(cout, generator=g) + 0.5
            sd[name + ".bn.bias"] = torch.randn(cout, generator=g) * 0.1
            sd[name + ".bn.running_mean"] = torch.randn(cout, generator=g) * 0.1
            sd[name + ".bn.running_var"] = torch.rand(cout, generator=g) + 0.5
        else:
            sd[name + ".conv3d.bias"] = torch.randn(cout, generator=g) * 0.1
    return sd


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps, 2)


class TorchI3D(object):
    """the network on torch's own kernels, with the folded weights unpacked from the HIP pack"""

    def __init__(self, i3d, w):
        self.i3d, self.p = i3d, {}
        for name, u in i3d.UNITS.items():
            wp, b = w.unit(name)
            kpad, cpad = w.layout[name][2:]
            K, k = u["cin"] * u["k"] ** 3, u["k"]
            wt = wp.view(kpad, cpad)[:K, :u["cout"]].reshape(k, k, k, u["cin"], u["cout"]).permute(4, 3, 0, 1, 2)
            self.p[name] = (wt.contiguous(), b[:u["cout"]].contiguous())

    @staticmethod
    def _pad(x, k3, s3, value):
        pads = []
        for n, k, s in zip(x.shape[:1:-1], k3[::-1], s3[::-1]):      # F.pad wants the last axis first
            total = max((-(-n // s) - 1) * s + k - n, 0)
            pads += [total // 2, total - total // 2]
        return F.pad(x, pads, value=value)

    def unit(self, name, x):
        u = self.i3d.UNITS[name]
        w, b = self.p[name]
        y = F.conv3d(self._pad(x, (u["k"],) * 3, (u["stride"],) * 3, 0.0), w, b, stride=u["stride"])
        return F.relu(y) if u["relu"] else y

    def pool(self, x, k3, s3):
        return F.max_pool3d(self._pad(x, k3, s3, float("-inf")), k3, s3)

    def __call__(self, x):
        """x channels-last [N, T, H, W, 3] -> [N, 400]"""
        x = x.permute(0, 4, 1, 2, 3)
        for kind, what in self.i3d.TRUNK:
            if kind == "unit":
                x = self.unit(what, x)
            elif kind == "pool":
                kt, khw, st, shw = what
                x = self.pool(x, (kt, khw, khw), (st, shw, shw))
            else:
                u = lambda br, t: self.unit(what + "." + br, t)
                x = torch.cat([u("b0", x), u("b1b", u("b1a", x)), u("b2b", u("b2a", x)),
                               u("b3b", self.pool(x, (3, 3, 3), (1, 1, 1)))], 1)
        y = self.unit("logits", F.avg_pool3d(x, (2, 7, 7), 1))
        return y.squeeze(4).squeeze(3).mean(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--videos", type=int, nargs="+", default=[16, 256])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_i3d needs a GPU"
    from rfn_hip import i3d, ops
    w = ops.i3d_pack(random_state(i3d.UNITS), "cuda")
    ref = TorchI3D(i3d, w)

    def torch_embed(v):
        with torch.no_grad():
            return torch.cat([ref(ops.i3d_preprocess(v[n0:n0 + 16])) for n0 in range(0, v.shape[0], 16)])

    rows = []
    for N in a.videos:
        for C in (1, 3):
            g = torch.Generator().manual_seed(N + C)
            v = torch.randint(0, 256, (N, 16, C, 64, 64), generator=g, dtype=torch.uint8).cuda()
            e_hip, e_torch = ops.i3d_embed(w, v[:16]), torch_embed(v[:16])
            rows.append({"shape": [N, 16, C, 64, 64],
                         "hip_ms": timed(lambda: ops.i3d_embed(w, v), a.reps),
                         "torch_ms": timed(lambda: torch_embed(v), a.reps),
                         "max_diff_over_rms": float((e_hip - e_torch).abs().max() / e_torch.pow(2).mean().sqrt())})
    print(json.dumps({"i3d_embed": rows, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
