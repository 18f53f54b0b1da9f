"""LPIPS with the AlexNet trunk on the GPU (csrc/lpips.hip; the reference scores every predicted frame with
lpips.LPIPS(net='alex'), evaluation_metrics/error_metrics.py:72, :173-187), from weight files the user supplies.

Definition (`lpips` 0.1.3, net='alex', version 0.1, lpips=True, spatial=False, eval mode).  Two uint8 frames [C, H, W],
C in {1, 3}; one channel is repeated three times.  Pixel p -> x = p/255*2 - 1 -> (x - shift[c]) / scale[c] with
shift = (-.030, -.088, -.188), scale = (.458, .448, .450).  Five taps, each after a ReLU; every convolution has a bias and
pads with zeros in the scaled domain (not with pixel value 0):
    1  conv 3->64 11x11 stride 4 pad 2
    2  maxpool 3x3 stride 2 (floor, no pad), conv 64->192 5x5 pad 2
    3  maxpool 3x3 stride 2, conv 192->384 3x3 pad 1
    4  conv 384->256 3x3 pad 1
    5  conv 256->256 3x3 pad 1
Head: per tap l and pixel n(f) = f / (sqrt(sum_c f_c^2) + 1e-10) (epsilon outside the root);
d_l = mean over pixels of sum_c w_l[c] (n(f0)_c - n(f1)_c)^2 with w_l the 1x1 "lin" weight of the tap (no bias; the Dropout
in front of it is the identity in eval mode); d = d_1 + ... + d_5.  Frames smaller than 31x31 are refused: the second pool
needs a 3x3 map.

Weights are read from local files only (torchvision's `alexnet-owt-*.pth` and the lpips package's
`lpips/weights/v0.1/alex.pth`); nothing is ever fetched.  There is no CPU fallback."""
import ctypes
import os

import torch

from . import lib as L
from .frame_metrics import _u8_frames


MIN_SIDE = 31
CHANNELS = (64, 192, 384, 256, 256)
# (state-dict index of torchvision's AlexNet.features, Cin, kernel size) of the five convolutions
_CONVS = ((0, 3, 11), (3, 64, 5), (6, 192, 3), (8, 384, 3), (10, 256, 3))
_WORKSPACE_FLOATS = 1 << 24      # default bound of the pooled-map workspace: 64 MiB
_MAX_CHUNK = 1024


def lpips_alex_sizes(H, W):
    """((rows, columns) of the five taps, floats per frame of the feature pack, workspace floats per frame); ValueError
    for frames under 31x31.  Host only: no GPU needed."""
    out = (ctypes.c_longlong * 12)()
    if L.load().rfn_lpips_alex_sizes(int(H), int(W), out) != 0:
        raise ValueError("lpips_alex: frames must be at least %dx%d (the second max pool needs a 3x3 map), got %dx%d" %
                         (MIN_SIDE, MIN_SIDE, H, W))
    return tuple((int(out[2 * l]), int(out[2 * l + 1])) for l in range(5)), int(out[10]), int(out[11])


class LpipsAlexWeights(object):
    """packed device tensors of one weight load: `trunk` (the five convolutions in the kernel's [Kpad][Cout] order with
    their biases, laid out by rfn_lpips_alex_weight_layout) and `lin` (the 1152 lin weights in tap order)"""

    def __init__(self, trunk, lin):
        self.trunk, self.lin = trunk, lin
        self.device = trunk.device


class LpipsFeatures(object):
    """feature pack of a batch of frames: `data` float32 [N, floats per frame] (per frame the five taps one after the
    other, each [pixels][channels]), the frames' leading shape `lead` and their size (H, W)"""

    def __init__(self, data, lead, H, W):
        self.data, self.lead, self.H, self.W = data, tuple(lead), H, W


def _state_dicts(paths):
    if isinstance(paths, (str, os.PathLike)):
        p = os.fspath(paths)
        if os.path.isdir(p):
            files = sorted(os.path.join(p, f) for f in os.listdir(p) if f.endswith((".pth", ".pt")))
        else:
            files = [p]
    else:
        files = [os.fspath(p) for p in paths]
    merged = {}
    for f in files:
        sd = torch.load(f, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict):
            raise ValueError("lpips_alex_load: %s does not hold a state dict" % f)
        merged.update(sd)
    return merged, files


def lpips_alex_pack(state, device, files=("<state dict>",)):
    """LpipsAlexWeights from a merged state dict (torchvision's AlexNet naming `features.{0,3,6,8,10}.{weight,bias}` and
    the lpips package's `lin{0..4}.model.1.weight` of shape [1, C, 1, 1]; other keys are ignored)"""
    def need(key, shape):
        t = state.get(key)
        if not isinstance(t, torch.Tensor):
            raise ValueError("lpips_alex_load: key %s is missing from %s" % (key, list(files)))
        if tuple(t.shape) != tuple(shape):
            raise ValueError("lpips_alex_load: key %s has shape %s, expected %s (files %s)" %
                             (key, tuple(t.shape), tuple(shape), list(files)))
        return t.detach().to(torch.float32)

    lay = (ctypes.c_longlong * 16)()
    if L.load().rfn_lpips_alex_weight_layout(lay) != 0:
        raise RuntimeError("rfn_lpips_alex_weight_layout failed")
    trunk = torch.zeros(int(lay[15]), dtype=torch.float32)
    lin = []
    for l, (idx, cin, ks) in enumerate(_CONVS):
        cout = CHANNELS[l]
        w = need("features.%d.weight" % idx, (cout, cin, ks, ks))
        b = need("features.%d.bias" % idx, (cout,))
        K = cin * ks * ks
        assert K <= int(lay[10 + l])
        # k = (ky*ks + kx)*Cin + ci, Cout contiguous; rows K .. Kpad-1 stay zero
        trunk[int(lay[l]):int(lay[l]) + K * cout] = w.permute(2, 3, 1, 0).reshape(-1)
        trunk[int(lay[5 + l]):int(lay[5 + l]) + cout] = b
        lin.append(need("lin%d.model.1.weight" % l, (1, cout, 1, 1)).reshape(-1))
    return LpipsAlexWeights(trunk.to(device), torch.cat(lin).contiguous().to(device))


def lpips_alex_load(paths, device):
    """Read the LPIPS-alex weights from local files: `paths` is a directory (its *.pth / *.pt files) or a list of files;
    all state dicts found are merged.  Needed are torchvision's AlexNet keys `features.{0,3,6,8,10}.{weight,bias}`
    (classifier keys are ignored) and the lpips package's `lin{0..4}.model.1.weight` [1, C, 1, 1]: the two upstream files
    `alexnet-owt-*.pth` and `lpips/weights/v0.1/alex.pth`.  A missing or mis-shaped key is a ValueError naming the key
    and the files.  Returns the packed device tensors (LpipsAlexWeights)."""
    state, files = _state_dicts(paths)
    return lpips_alex_pack(state, device, files)


def _check_frames(t, nm, who):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, got %s" % (who, nm, type(t).__name__))
    if t.dtype != torch.uint8:
        raise TypeError("%s: %s must be uint8, got %s" % (who, nm, t.dtype))
    if t.dim() < 3:
        raise ValueError("%s: %s must be [..., C, H, W], got shape %s" % (who, nm, tuple(t.shape)))
    C, H, W = (int(d) for d in t.shape[-3:])
    if C not in (1, 3):
        raise ValueError("%s: %s must have 1 or 3 channels, got %d" % (who, nm, C))
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError("%s: frames must be at least %dx%d (the second max pool needs a 3x3 map), got %dx%d" %
                         (who, MIN_SIDE, MIN_SIDE, H, W))
    return C, H, W


def _check_device(w, t, nm, who):
    if not t.is_cuda:
        raise RuntimeError("rfn_hip kernels need device tensors; %s is on %s (no CPU fallback)" % (nm, t.device))
    if w.device != t.device:
        raise ValueError("%s: the weights are on %s, %s on %s" % (who, w.device, nm, t.device))


def lpips_alex_features(w, frames, chunk=None):
    """AlexNet features (the five taps) of uint8 frames [..., C, H, W], C in {1, 3}, on the GPU
    (rfn_lpips_alex_features_u8): an LpipsFeatures pack.  Frames are processed `chunk` at a time (default: as many as keep
    the pooled-map workspace under 64 MiB, at most 1024); a frame's features do not depend on the chunking.  Views such as
    x[:, start:] or a channel slice are accepted."""
    C, H, W = _check_frames(frames, "frames", "lpips_alex_features")
    _, F, work = lpips_alex_sizes(H, W)
    _check_device(w, frames, "frames", "lpips_alex_features")
    lead = tuple(frames.shape[:-3])
    N = 1
    for d in lead:
        N *= int(d)
    data = torch.empty((N, F), device=frames.device, dtype=torch.float32)
    if N == 0:
        return LpipsFeatures(data, lead, H, W)
    if chunk is None:
        chunk = max(1, min(_MAX_CHUNK, _WORKSPACE_FLOATS // work))
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("lpips_alex_features: chunk must be at least 1, got %d" % chunk)
    chunk = min(chunk, N)
    v, _, ns = _u8_frames(frames, C, H, W)
    ws = torch.empty(chunk * work, device=frames.device, dtype=torch.float32)
    with torch.cuda.device(frames.device):
        for n0 in range(0, N, chunk):
            n = min(chunk, N - n0)
            L.call("rfn_lpips_alex_features_u8", v.data_ptr() + n0 * ns, ns, n, C, H,
                   W, L.dev(w.trunk), w.trunk.numel(), L.dev(data[n0:n0 + n]), L.dev(ws), ws.numel(),
                   meta=("shell", "lpips_alex_features", 0.0, "%dx%dx%dx%d" % (n, C, H, W), 4.0 * n * F))
    return LpipsFeatures(data, lead, H, W)


def lpips_alex_distance(w, fa, fb, per_layer=False):
    """LPIPS distance of two feature packs of equal shape (rfn_lpips_alex_distance): float32 over the frames' leading
    shape; with per_layer=True also the [..., 5] per-tap values.  Exactly 0 on equal features; (fa, fb) and (fb, fa) give
    the same bits."""
    for t, nm in ((fa, "fa"), (fb, "fb")):
        if not isinstance(t, LpipsFeatures):
            raise TypeError("lpips_alex_distance: %s must come from lpips_alex_features, got %s" % (nm, type(t).__name__))
    if (fa.lead, fa.H, fa.W) != (fb.lead, fb.H, fb.W):
        raise ValueError("lpips_alex_distance: shapes differ: %s %dx%d vs %s %dx%d" %
                         (fa.lead, fa.H, fa.W, fb.lead, fb.H, fb.W))
    _check_device(w, fa.data, "fa", "lpips_alex_distance")
    _check_device(w, fb.data, "fb", "lpips_alex_distance")
    N = int(fa.data.shape[0])
    d = torch.empty(fa.lead, device=fa.data.device, dtype=torch.float32)
    taps = torch.empty(fa.lead + (5,), device=fa.data.device, dtype=torch.float32)
    if N:
        with torch.cuda.device(fa.data.device):
            L.call("rfn_lpips_alex_distance", L.dev(fa.data), L.dev(fb.data), L.dev(w.lin), N, fa.H, fa.W,
                   L.dev(taps), L.dev(d),
                   meta=("shell", "lpips_alex_distance", 0.0, "%dx%dx%d" % (N, fa.H, fa.W), 8.0 * fa.data.numel()))
    return (d, taps) if per_layer else d


def lpips_alex(w, a, b, per_layer=False, chunk=None):
    """LPIPS-alex distance of two uint8 video tensors [..., C, H, W] of equal shape on the GPU: float32 over the leading
    shape (lpips_alex_features of each, then lpips_alex_distance)."""
    _check_frames(a, "a", "lpips_alex")
    _check_frames(b, "b", "lpips_alex")
    if a.shape != b.shape:
        raise ValueError("lpips_alex: shapes differ: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    for t, nm in ((a, "a"), (b, "b")):
        _check_device(w, t, nm, "lpips_alex")
    return lpips_alex_distance(w, lpips_alex_features(w, a, chunk=chunk), lpips_alex_features(w, b, chunk=chunk),
                               per_layer=per_layer)
