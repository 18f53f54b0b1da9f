"""Frechet Video Distance: the Inflated-3D Inception trunk (I3D, Kinetics-400, RGB stream) on the GPU (csrc/i3d.hip) from
weight files the user supplies, and the Frechet distance on its logits (the reference: evaluation_metrics/FVD.py,
FVD_score.py, error_metrics.py:1006-1063; TF-hub module deepmind/i3d-kinetics-400/1, output RGB/inception_i3d/Mean).

Definition (DESIGN.md section 14 is the contract).  uint8 videos [N, T, C, H, W], C in {1, 3} (one channel stands for all
three).  Every frame is resized to 224x224 with TF1's resize_bilinear (align_corners=False, no half-pixel centres:
src = dst * (in / out), i0 = floor(src), i1 = min(i0 + 1, in - 1), weight src - i0, all in float32), then
x = 2 v / 255 - 1.  Activations are channels-last [N, T, H, W, C]; every convolution and pool pads as TF "SAME"
(out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before = pad_total // 2).  A unit is a convolution
without bias, inference BatchNorm (eps 1e-3) and ReLU; the loader folds the BatchNorm into weights and a bias in float64.
The layers are TRUNK below; the head averages over windows of 2 x 7 x 7 (stride 1, VALID), applies the 1x1x1 logits
convolution 1024 -> 400 (bias, no BatchNorm, no ReLU) and takes the mean over the remaining time axis: [N, 400].
The final map must be 7x7 (input side 193..224) and T at least 9.

Weights are read from local files only; nothing is ever fetched.  There is no CPU fallback for the trunk;
frechet_distance is float64 host arithmetic on 400 x 400 matrices."""
import ctypes
import os

import numpy as np
import torch

from . import lib as L
from .frame_metrics import _u8_frames


SIDE = 224                    # the public path resizes every frame to SIDE x SIDE
MIN_SIDE, MAX_SIDE = 193, 224   # trunk input sides that end in a 7x7 map
MIN_T = 9                     # two time steps must be left for the average pool
FINAL_SIDE = 7
N_LOGITS = 400
BN_EPS = 1e-3
MIN_VIDEOS = 16               # the reference asserts a whole chunk of 16 videos
_WORKSPACE_FLOATS = 1 << 28   # default bound of the activation workspace: 1 GiB

# ---------------------------------------------------------------------------------------------------- the network
# inception block -> (input channels, (a, b, c, d, e, f)): branches 1x1 -> a | 1x1 -> b, 3x3 -> c | 1x1 -> d, 3x3 -> e |
# max pool 3x3x3 stride 1, 1x1 -> f, concatenated in this order
MIXED = {
    "Mixed_3b": (192, (64, 96, 128, 16, 32, 32)),
    "Mixed_3c": (256, (128, 128, 192, 32, 96, 64)),
    "Mixed_4b": (480, (192, 96, 208, 16, 48, 64)),
    "Mixed_4c": (512, (160, 112, 224, 24, 64, 64)),
    "Mixed_4d": (512, (128, 128, 256, 24, 64, 64)),
    "Mixed_4e": (512, (112, 144, 288, 32, 64, 64)),
    "Mixed_4f": (528, (256, 160, 320, 32, 128, 128)),
    "Mixed_5b": (832, (256, 160, 320, 32, 128, 128)),
    "Mixed_5c": (832, (384, 192, 384, 48, 128, 128)),
}
# ("unit", name) | ("pool", (kt, khw, st, shw)) | ("mixed", name), in order
TRUNK = (("unit", "Conv3d_1a_7x7"), ("pool", (1, 3, 1, 2)), ("unit", "Conv3d_2b_1x1"), ("unit", "Conv3d_2c_3x3"),
         ("pool", (1, 3, 1, 2)), ("mixed", "Mixed_3b"), ("mixed", "Mixed_3c"), ("pool", (3, 3, 2, 2)),
         ("mixed", "Mixed_4b"), ("mixed", "Mixed_4c"), ("mixed", "Mixed_4d"), ("mixed", "Mixed_4e"), ("mixed", "Mixed_4f"),
         ("pool", (2, 2, 2, 2)), ("mixed", "Mixed_5b"), ("mixed", "Mixed_5c"))
LOGITS = "logits"
# the six units of a block: (name in the PyTorch port, TF scope, index of its input width or None for the block input,
# index of its output width, kernel side)
_BRANCH_UNITS = (("b0", "Branch_0/Conv3d_0a_1x1", None, 0, 1), ("b1a", "Branch_1/Conv3d_0a_1x1", None, 1, 1),
                 ("b1b", "Branch_1/Conv3d_0b_3x3", 1, 2, 3), ("b2a", "Branch_2/Conv3d_0a_1x1", None, 3, 1),
                 ("b2b", "Branch_2/Conv3d_0b_3x3", 3, 4, 3), ("b3b", "Branch_3/Conv3d_0b_1x1", None, 5, 1))
_TF_ROOT = "RGB/inception_i3d/"


def mixed_width(name):
    a, b, c, d, e, f = MIXED[name][1]
    return a + c + e + f


def _build_units():
    """THE name table.  unit -> dict(cin, cout, k, stride, relu, bn, pt = key prefix of the PyTorch port (format A),
    tf = TF scopes under RGB/inception_i3d/ (format B; the first is the canonical one))"""
    u = {}

    def add(name, cin, cout, k, stride, tf, relu=True, bn=True):
        u[name] = dict(cin=cin, cout=cout, k=k, stride=stride, relu=relu, bn=bn, pt=name, tf=tuple(tf))

    add("Conv3d_1a_7x7", 3, 64, 7, 2, ["Conv3d_1a_7x7"])
    add("Conv3d_2b_1x1", 64, 64, 1, 1, ["Conv3d_2b_1x1"])
    add("Conv3d_2c_3x3", 64, 192, 3, 1, ["Conv3d_2c_3x3"])
    for block, (cin, widths) in MIXED.items():
        for pt, tf, src, dst, k in _BRANCH_UNITS:
            scopes = [block + "/" + tf]
            if block == "Mixed_5b" and pt == "b2b":      # upstream naming quirk of this one unit
                scopes.append(block + "/Branch_2/Conv3d_0a_3x3")
            add(block + "." + pt, cin if src is None else widths[src], widths[dst], k, 1, scopes)
    add(LOGITS, 1024, N_LOGITS, 1, 1, ["Logits/Conv3d_0c_1x1"], relu=False, bn=False)
    return u


UNITS = _build_units()


def i3d_same(n, k, s):
    """(output extent, pad before) of one axis under TF "SAME" padding"""
    out = (ctypes.c_longlong * 2)()
    if L.load().rfn_i3d_same(int(n), int(k), int(s), out) != 0:
        raise ValueError("i3d_same: extent, kernel and stride must be at least 1, got %s" % ((n, k, s),))
    return int(out[0]), int(out[1])


def _pack_dims(cin, cout, k):
    out = (ctypes.c_longlong * 2)()
    if L.load().rfn_i3d_conv_pack_dims(int(cin), int(cout), int(k), out) != 0:
        raise RuntimeError("rfn_i3d_conv_pack_dims failed: %s" % L.load().rfn_last_error().decode())
    return int(out[0]), int(out[1])


def _same3(shape, k3, s3):
    return tuple(i3d_same(n, k, s)[0] for n, k, s in zip(shape, k3, s3))


def i3d_sizes(T, H, W):
    """Map sizes and workspace need of the trunk on an input [T, H, W, 3].  Returns (maps, main, scratch): maps = the
    (T, H, W, C) after every entry of TRUNK, main = floats of the largest map per video, scratch = floats per video of the
    three side maps of an inception block (the two bottlenecks and the pooled input).  ValueError names the broken rule.
    Host only: no GPU needed."""
    T, H, W = int(T), int(H), int(W)
    if T < MIN_T:
        raise ValueError("i3d: T must be at least %d so that two time steps are left for the average pool, got %d" %
                         (MIN_T, T))
    if not (MIN_SIDE <= H <= MAX_SIDE and MIN_SIDE <= W <= MAX_SIDE):
        raise ValueError("i3d: the final map must be %dx%d, so the trunk input side must be in %d..%d, got %dx%d" %
                         (FINAL_SIDE, FINAL_SIDE, MIN_SIDE, MAX_SIDE, H, W))
    maps, cur, C = [], (T, H, W), 3
    main, scratch = T * H * W * 3, [0, 0, 0]
    for kind, what in TRUNK:
        if kind == "unit":
            u = UNITS[what]
            cur, C = _same3(cur, (u["k"],) * 3, (u["stride"],) * 3), u["cout"]
        elif kind == "pool":
            kt, khw, st, shw = what
            cur = _same3(cur, (kt, khw, khw), (st, shw, shw))
        else:
            cin, widths = MIXED[what]
            assert cin == C, (what, cin, C)
            cells = cur[0] * cur[1] * cur[2]
            for j, c in enumerate((widths[1], widths[3], cin)):
                scratch[j] = max(scratch[j], cells * c)
            C = mixed_width(what)
        maps.append(cur + (C,))
        main = max(main, cur[0] * cur[1] * cur[2] * C)
    assert maps[-1][1:] == (FINAL_SIDE, FINAL_SIDE, 1024) and maps[-1][0] >= 2, maps[-1]
    return tuple(maps), main, tuple(scratch)


# ---------------------------------------------------------------------------------------------------- weights
class I3DWeights(object):
    """one weight load: `data`, one float32 buffer holding per unit the packed [Kpad][Coutpad] convolution
    (k = ((kt k + ky) k + kx) Cin + ci, BatchNorm folded in, zero rows and columns in the padding) and its Coutpad biases;
    `layout`: unit -> (weight offset, bias offset, Kpad, Coutpad)"""

    def __init__(self, data, layout):
        self.data, self.layout = data, layout
        self.device = data.device

    def unit(self, name):
        wo, bo, kpad, cpad = self.layout[name]
        return self.data[wo:wo + kpad * cpad], self.data[bo:bo + cpad]


def _files_of(paths):
    if isinstance(paths, (str, os.PathLike)):
        p = os.fspath(paths)
        if os.path.isdir(p):
            return sorted(os.path.join(p, f) for f in os.listdir(p) if f.endswith((".pth", ".pt", ".npz")))
        return [p]
    return [os.fspath(p) for p in paths]


def _read_files(paths):
    files = _files_of(paths)
    merged = {}
    for f in files:
        if f.endswith(".npz"):
            with np.load(f, allow_pickle=False) as z:
                merged.update({k: torch.from_numpy(np.asarray(z[k])) for k in z.files})
        else:
            sd = torch.load(f, map_location="cpu", weights_only=True)
            if not isinstance(sd, dict):
                raise ValueError("i3d_load: %s does not hold a state dict" % f)
            merged.update(sd)
    return merged, files


def i3d_pack(state, device, files=("<state dict>",)):
    """I3DWeights from a merged dict of tensors in either naming (other keys are ignored).
    Format A, the common PyTorch port: `<unit>.conv3d.weight` [O, I, T, H, W], `<unit>.bn.{weight, bias, running_mean,
    running_var}` [O], `logits.conv3d.{weight, bias}`, with <unit> = Conv3d_1a_7x7, ..., Mixed_3b.{b0,b1a,b1b,b2a,b2b,b3b}.
    Format B, the TF variables: `RGB/inception_i3d/<scope>/conv_3d/w` [T, H, W, I, O], `<scope>/batch_norm/{beta,
    moving_mean, moving_variance}` [1, 1, 1, 1, O] (`gamma` optional; missing means 1), `Logits/Conv3d_0c_1x1/conv_3d/{w, b}`,
    with <scope> = Conv3d_1a_7x7, ..., Mixed_3b/Branch_1/Conv3d_0b_3x3 (UNITS holds every name).  A unit is read in the
    format its convolution weight is found in.  A missing or mis-shaped key is a ValueError naming the key, the expected
    shape and the files."""
    files = list(files)

    def need(key, shape, optional=False):
        t = state.get(key)
        if not isinstance(t, torch.Tensor):
            if optional:
                return None
            raise ValueError("i3d_load: key %s (expected shape %s) is missing from %s" % (key, tuple(shape), files))
        if tuple(t.shape) != tuple(shape):
            raise ValueError("i3d_load: key %s has shape %s, expected %s (files %s)" %
                             (key, tuple(t.shape), tuple(shape), files))
        return t.detach().to(torch.float64)

    layout, total = {}, 0
    for name, u in UNITS.items():
        kpad, cpad = _pack_dims(u["cin"], u["cout"], u["k"])
        layout[name] = (total, total + kpad * cpad, kpad, cpad)
        total += kpad * cpad + cpad
    data = torch.zeros(total, dtype=torch.float32)
    for name, u in UNITS.items():
        cin, cout, k = u["cin"], u["cout"], u["k"]
        key_a = u["pt"] + ".conv3d.weight"
        scope = next((s for s in u["tf"] if _TF_ROOT + s + "/conv_3d/w" in state), None)
        if key_a in state:
            w = need(key_a, (cout, cin, k, k, k)).permute(2, 3, 4, 1, 0)
            if u["bn"]:
                gamma = need(u["pt"] + ".bn.weight", (cout,), optional=True)
                beta, mean, var = (need(u["pt"] + ".bn." + s, (cout,)) for s in ("bias", "running_mean", "running_var"))
            else:
                bias = need(u["pt"] + ".conv3d.bias", (cout,))
        elif scope is not None:
            w = need(_TF_ROOT + scope + "/conv_3d/w", (k, k, k, cin, cout))
            if u["bn"]:
                bshape = (1, 1, 1, 1, cout)
                gamma = need(_TF_ROOT + scope + "/batch_norm/gamma", bshape, optional=True)
                beta, mean, var = (need(_TF_ROOT + scope + "/batch_norm/" + s, bshape).reshape(-1)
                                   for s in ("beta", "moving_mean", "moving_variance"))
                gamma = None if gamma is None else gamma.reshape(-1)
            else:
                bias = need(_TF_ROOT + scope + "/conv_3d/b", (cout,))
        else:
            raise ValueError("i3d_load: key %s (expected shape %s) or %s (expected shape %s) is missing from %s" %
                             (key_a, (cout, cin, k, k, k), " / ".join(_TF_ROOT + s + "/conv_3d/w" for s in u["tf"]),
                              (k, k, k, cin, cout), files))
        if u["bn"]:     # fold: g = gamma / sqrt(var + eps), w' = w g, b' = beta - mean g
            g = (1.0 if gamma is None else gamma) / torch.sqrt(var + BN_EPS)
            w, bias = w * g, beta - mean * g
        wo, bo, kpad, cpad = layout[name]
        K = cin * k * k * k
        data[wo:wo + kpad * cpad].view(kpad, cpad)[:K, :cout] = w.reshape(K, cout).to(torch.float32)
        data[bo:bo + cout] = bias.to(torch.float32)
    return I3DWeights(data.to(device), layout)


def i3d_load(paths, device):
    """Read the I3D weights from local files: `paths` is a directory (its *.pth / *.pt / *.npz files) or a list of files;
    torch state dicts (format A) and .npz archives of the TF variables (format B) are merged (i3d_pack lists the keys).
    Returns the packed device buffer (I3DWeights)."""
    state, files = _read_files(paths)
    return i3d_pack(state, device, files)


# ---------------------------------------------------------------------------------------------------- layer wrappers
def _check_map(w, x, nm, who, C=None):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, got %s" % (who, nm, type(x).__name__))
    if not x.is_cuda:
        raise RuntimeError("rfn_hip kernels need device tensors; %s is on %s (no CPU fallback)" % (nm, x.device))
    if w is not None and w.device != x.device:
        raise ValueError("%s: the weights are on %s, %s on %s" % (who, w.device, nm, x.device))
    if x.dim() != 5 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("%s: %s must be a dense float32 [N, T, H, W, C] map, got %s %s" %
                         (who, nm, x.dtype, tuple(x.shape)))
    if C is not None and int(x.shape[4]) != C:
        raise ValueError("%s: %s must have %d channels, got %d" % (who, nm, C, int(x.shape[4])))
    return tuple(int(d) for d in x.shape)


def i3d_unit(w, name, x, out=None, coff=0):
    """One unit of the network (UNITS[name]: convolution with the folded BatchNorm bias and ReLU; `logits` has a bias and
    no ReLU) on a channels-last map x [N, T, H, W, Cin] (rfn_i3d_conv3d_f32).  Writes the Cout channels at channel offset
    `coff` of `out` [N, To, Ho, Wo, pitch] (other channels are left alone) and returns `out`; without `out` a new
    [N, To, Ho, Wo, Cout] map."""
    u = UNITS[name]
    N, T, H, W, _ = _check_map(w, x, "x", "i3d_unit", u["cin"])
    shape = (N,) + _same3((T, H, W), (u["k"],) * 3, (u["stride"],) * 3)
    if out is None:
        out = torch.empty(shape + (u["cout"],), device=x.device, dtype=torch.float32)
    o = _check_map(w, out, "out", "i3d_unit")
    if o[:4] != shape or not 0 <= coff <= o[4] - u["cout"]:
        raise ValueError("i3d_unit: out must be %s + (at least %d channels), got %s" % (shape, coff + u["cout"], o))
    if N:
        wp, b = w.unit(name)
        with torch.cuda.device(x.device):
            L.call("rfn_i3d_conv3d_f32", L.dev(x), x.numel(), N, T, H, W, u["cin"], L.dev(wp), wp.numel(), L.dev(b),
                   u["cout"], u["k"], u["stride"], 1 if u["relu"] else 0, L.dev(out), out.numel(), coff, o[4],
                   meta=("shell", "i3d_conv3d", 2.0 * (out.numel() // o[4]) * u["cout"] * u["cin"] * u["k"] ** 3,
                         "%s %s" % (name, "x".join(map(str, x.shape))), 4.0 * (x.numel() + out.numel())))
    return out


def i3d_maxpool(x, kt, khw, st, shw, out=None):
    """SAME max pool with window kt x khw x khw and stride st x shw x shw of a channels-last map (rfn_i3d_maxpool3d_f32);
    cells outside the map are ignored"""
    N, T, H, W, C = _check_map(None, x, "x", "i3d_maxpool")
    shape = (N,) + _same3((T, H, W), (kt, khw, khw), (st, shw, shw)) + (C,)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    if _check_map(None, out, "out", "i3d_maxpool") != shape:
        raise ValueError("i3d_maxpool: out must be %s, got %s" % (shape, tuple(out.shape)))
    if N:
        with torch.cuda.device(x.device):
            L.call("rfn_i3d_maxpool3d_f32", L.dev(x), x.numel(), N, T, H, W, C, kt, khw,
                   st, shw, L.dev(out), out.numel(),
                   meta=("shell", "i3d_maxpool3d", 0.0, "x".join(map(str, x.shape)), 4.0 * (x.numel() + out.numel())))
    return out


def i3d_inception(w, name, x, out=None, scratch=None):
    """One inception block (MIXED[name]) on x [N, T, H, W, Cin]: seven launches, every branch writing its columns of the
    concatenated output directly.  `scratch`: three maps for the two bottlenecks and the pooled input (allocated when
    missing)."""
    cin, (a, b, c, d, e, f) = MIXED[name]
    N, T, H, W, _ = _check_map(w, x, "x", "i3d_inception", cin)
    if out is None:
        out = torch.empty((N, T, H, W, a + c + e + f), device=x.device, dtype=torch.float32)
    if scratch is None:
        scratch = tuple(torch.empty((N, T, H, W, ch), device=x.device, dtype=torch.float32) for ch in (b, d, cin))
    s1, s2, s3 = scratch
    i3d_unit(w, name + ".b0", x, out, 0)
    i3d_unit(w, name + ".b1a", x, s1)
    i3d_unit(w, name + ".b1b", s1, out, a)
    i3d_unit(w, name + ".b2a", x, s2)
    i3d_unit(w, name + ".b2b", s2, out, a + c)
    i3d_maxpool(x, 3, 3, 1, 1, s3)
    i3d_unit(w, name + ".b3b", s3, out, a + c + e)
    return out


def i3d_head(w, x):
    """The head on the last map x [N, T', 7, 7, 1024] (T' >= 2): average over windows of 2 x 7 x 7, the logits
    convolution, the mean over the T' - 1 windows -> [N, 400] (rfn_i3d_head_f32)"""
    N, Tp, H, W, C = _check_map(w, x, "x", "i3d_head", 1024)
    if (H, W) != (FINAL_SIDE, FINAL_SIDE) or Tp < 2:
        raise ValueError("i3d_head: the last map must be [N, T' >= 2, 7, 7, 1024], got %s" % (tuple(x.shape),))
    out = torch.empty((N, N_LOGITS), device=x.device, dtype=torch.float32)
    if N:
        wp, b = w.unit(LOGITS)
        with torch.cuda.device(x.device):
            L.call("rfn_i3d_head_f32", L.dev(x), x.numel(), N, Tp, H * W, C, L.dev(wp), wp.numel(), L.dev(b), N_LOGITS,
                   L.dev(out), meta=("shell", "i3d_head", 0.0, "x".join(map(str, x.shape)), 4.0 * x.numel()))
    return out


# ---------------------------------------------------------------------------------------------------- the network
def _check_videos(v, who):
    if not isinstance(v, torch.Tensor):
        raise TypeError("%s: videos must be a tensor, got %s" % (who, type(v).__name__))
    if v.dtype != torch.uint8:
        raise TypeError("%s: videos must be uint8, got %s" % (who, v.dtype))
    if v.dim() != 5:
        raise ValueError("%s: videos must be [N, T, C, H, W], got shape %s" % (who, tuple(v.shape)))
    N, T, C, H, W = (int(d) for d in v.shape)
    if C not in (1, 3):
        raise ValueError("%s: videos must have 1 or 3 channels, got %d" % (who, C))
    if H < 1 or W < 1:
        raise ValueError("%s: empty frames %dx%d" % (who, H, W))
    if not v.is_cuda:
        raise RuntimeError("rfn_hip kernels need device tensors; videos is on %s (no CPU fallback)" % v.device)
    return N, T, C, H, W


def _resize_into(videos, out):
    N, T, C, H, W = (int(d) for d in videos.shape)
    if N * T:
        v, p, ns = _u8_frames(videos, C, H, W)
        with torch.cuda.device(videos.device):
            L.call("rfn_i3d_resize_u8", p, ns, N * T, C, H, W, L.dev(out), out.numel(),
                   meta=("shell", "i3d_resize", 0.0, "x".join(map(str, videos.shape)), 4.0 * out.numel()))
    return out


def i3d_preprocess(videos_u8):
    """uint8 videos [N, T, C, H, W] (C in {1, 3}) -> float32 [N, T, 224, 224, 3]: TF1 bilinear resize of every frame,
    then 2 v / 255 - 1 (rfn_i3d_resize_u8); one channel is written three times"""
    N, T, C, H, W = _check_videos(videos_u8, "i3d_preprocess")
    out = torch.empty((N, T, SIDE, SIDE, 3), device=videos_u8.device, dtype=torch.float32)
    return _resize_into(videos_u8, out)


class _Workspace(object):
    """the activation buffers of one chunk: two maps that alternate as input and output, and the three side maps of an
    inception block"""

    def __init__(self, chunk, main, scratch, device, extra=0):
        self.flat = torch.empty(chunk * (2 * main + sum(scratch) + extra), device=device, dtype=torch.float32)
        o, self.parts = 0, []
        for size in (main, main) + tuple(scratch) + (extra,):
            self.parts.append(self.flat[o:o + chunk * size])
            o += chunk * size

    def view(self, j, shape):
        n = 1
        for d in shape:
            n *= d
        return self.parts[j][:n].view(shape)


def _trunk(w, x, ws):
    """logits [n, 400] of one chunk x [n, T, H, W, 3]"""
    n = int(x.shape[0])
    cur, side = x, 0
    for kind, what in TRUNK:
        T, H, W = (int(d) for d in cur.shape[1:4])
        if kind == "unit":
            u = UNITS[what]
            out = ws.view(side, (n,) + _same3((T, H, W), (u["k"],) * 3, (u["stride"],) * 3) + (u["cout"],))
            i3d_unit(w, what, cur, out)
        elif kind == "pool":
            kt, khw, st, shw = what
            out = ws.view(side, (n,) + _same3((T, H, W), (kt, khw, khw), (st, shw, shw)) + (int(cur.shape[4]),))
            i3d_maxpool(cur, kt, khw, st, shw, out)
        else:
            cin, widths = MIXED[what]
            out = ws.view(side, (n, T, H, W, mixed_width(what)))
            scratch = tuple(ws.view(2 + j, (n, T, H, W, c)) for j, c in enumerate((widths[1], widths[3], cin)))
            i3d_inception(w, what, cur, out, scratch)
        cur, side = out, 1 - side
    return i3d_head(w, cur)


def _chunk(chunk, per_video, N, who):
    if chunk is None:
        chunk = max(1, _WORKSPACE_FLOATS // per_video)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("%s: chunk must be at least 1, got %d" % (who, chunk))
    return min(chunk, N)


def i3d_logits(w, x, chunk=None):
    """Logits [N, 400] of channels-last float32 input x [N, T, H, W, 3] (T >= 9, sides in 193..224): the trunk and the
    head, 71 launches per chunk of videos.  Videos are processed `chunk` at a time (default: as many as keep the
    activation workspace under 1 GiB); a video's logits do not depend on the chunking."""
    N, T, H, W, _ = _check_map(w, x, "x", "i3d_logits", 3)
    _, main, scratch = i3d_sizes(T, H, W)
    out = torch.empty((N, N_LOGITS), device=x.device, dtype=torch.float32)
    if N == 0:
        return out
    chunk = _chunk(chunk, 2 * main + sum(scratch), N, "i3d_logits")
    ws = _Workspace(chunk, main, scratch, x.device)
    for n0 in range(0, N, chunk):
        out[n0:n0 + chunk] = _trunk(w, x[n0:n0 + chunk], ws)
    return out


def i3d_embed(w, videos_u8, chunk=None):
    """The public path: I3D logits [N, 400] of uint8 videos [N, T, C, H, W] (C in {1, 3}, T >= 9, any frame size):
    i3d_preprocess and i3d_logits, `chunk` videos at a time in one workspace (default: under 1 GiB), so that nothing but
    the result grows with N.  Bit for bit i3d_logits(i3d_preprocess(videos)), whatever the chunking."""
    N, T, C, H, W = _check_videos(videos_u8, "i3d_embed")
    if w.device != videos_u8.device:
        raise ValueError("i3d_embed: the weights are on %s, videos on %s" % (w.device, videos_u8.device))
    _, main, scratch = i3d_sizes(T, SIDE, SIDE)
    out = torch.empty((N, N_LOGITS), device=videos_u8.device, dtype=torch.float32)
    if N == 0:
        return out
    frames = T * SIDE * SIDE * 3
    chunk = _chunk(chunk, 2 * main + sum(scratch) + frames, N, "i3d_embed")
    ws = _Workspace(chunk, main, scratch, videos_u8.device, extra=frames)
    for n0 in range(0, N, chunk):
        v = videos_u8[n0:n0 + chunk]
        x = _resize_into(v, ws.view(5, (int(v.shape[0]), T, SIDE, SIDE, 3)))
        out[n0:n0 + chunk] = _trunk(w, x, ws)
    return out


# ---------------------------------------------------------------------------------------------------- Frechet distance
def _symsqrt(a):
    """U diag(s_i < 1e-10 ? s_i : sqrt(s_i)) V^T from the SVD of a"""
    u, s, vt = np.linalg.svd(a)
    return (u * np.where(s < 1e-10, s, np.sqrt(s))) @ vt


def frechet_distance(real, fake):
    """Frechet distance of two sets of embeddings [n, d] (tensors or arrays), as
    tf.contrib.gan.eval.frechet_classifier_distance_from_activations of TF 1.15, in float64 on the host:
    m = mean, S = (X - m)^T (X - m) / (n - 1), r = trace(symsqrt(symsqrt(S_r) S_g symsqrt(S_r))),
    d = trace(S_r + S_g) - 2 r + |m_r - m_g|^2.  Fewer than 16 embeddings in either set is a ValueError."""
    sets = []
    for x, nm in ((real, "real"), (fake, "fake")):
        if isinstance(x, torch.Tensor):
            x = x.detach().to("cpu", torch.float64).numpy()
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("frechet_distance: %s must be [n, d], got shape %s" % (nm, x.shape))
        if x.shape[0] < MIN_VIDEOS:
            raise ValueError("frechet_distance: at least %d embeddings are needed, %s has %d" %
                             (MIN_VIDEOS, nm, x.shape[0]))
        sets.append(x)
    if sets[0].shape[1] != sets[1].shape[1]:
        raise ValueError("frechet_distance: the sets differ in dimension: %d vs %d" % (sets[0].shape[1], sets[1].shape[1]))
    (m_r, s_r), (m_g, s_g) = ((x.mean(0), (x - x.mean(0)).T @ (x - x.mean(0)) / (x.shape[0] - 1)) for x in sets)
    root = _symsqrt(s_r)
    r = np.trace(_symsqrt(root @ s_g @ root))
    return float(np.trace(s_r + s_g) - 2.0 * r + ((m_r - m_g) ** 2).sum())
