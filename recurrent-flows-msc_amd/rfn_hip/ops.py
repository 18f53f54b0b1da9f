"""Tensor-level wrappers and autograd Functions over the C ABI (include/rfn_hip.h).

Everything here runs on the GPU through librfn_hip.so; torch is used for memory, streams and autograd plumbing.
Frame-batched layout: tensors are [N, C, H, W] fp32 where N = all frames handed over by the caller (the RFN driver
time-batches B*(T-1) frames into one call).

This module holds the training core (the convolutions and their gradients, the Glow nodes, the latent step and the
ConvLSTM), whose functions read CONV_PRECISION / MIXED_FWD and call each other through this namespace.  Every other
wrapper family has a module of its own, named after the csrc file it wraps; the block at the bottom re-exports their
public names, so callers write rfn_hip.ops.X for all of them ("Where the Python wrappers live").
"""
import collections
import functools
import itertools

import torch

from . import lib as L
from .args import flat as _f, shell as _shell

import os

# Arithmetic of the MFMA convolutions (RFN_CONV_PRECISION):
#   "mixed"  (default) forward pass fp32-grade, gradients split precision:
#              forward  coupling nets of the shallow levels: fused kernel, two scaled fp16 pieces per operand ("f16x3s",
#                       22 significant bits, csrc/coupling_po.hip); every other forward convolution on a map larger than
#                       2x2: fp32 MFMA (v_mfma_f32_32x32x2_f32); 2x2 maps (latent nets, ConvLSTM, deepest flow level):
#                       bf16x3 -- tools/precision_study.py: bits/dim error 1.3e-5 vs 1.0e-5 all-fp32-grade, 4.9e-4 all-bf16x3
#              backward bf16x3 (data and weight gradients)
#   "bf16x3" every convolution on two bf16 pieces per operand, three v_mfma_f32_32x32x16_bf16 per product (16 bits)
#   "f32"    every convolution on v_mfma_f32_32x32x2_f32
CONV_PRECISION = os.environ.get("RFN_CONV_PRECISION", "mixed")


def bwd_b3():
    """gradient convolutions run split precision (bf16x3)"""
    return CONV_PRECISION in ("bf16x3", "mixed")


MIXED_FWD = os.environ.get("RFN_MIXED_FWD", "bf16x6")  # fp32-grade arithmetic of the unfused forward convs: bf16x6 | f32


def fwd_prec(H, W):
    """arithmetic of an (unfused) forward convolution on an H x W map: 'bf16x3', 'bf16x6' (three bf16 pieces per operand,
    six MFMAs per product: fp32-grade at a third of the fp32-MFMA cost) or 'f32'"""
    if CONV_PRECISION == "mixed":
        return "bf16x3" if H * W <= 4 else MIXED_FWD
    return CONV_PRECISION

ACT = {"none": 0, "relu": 1, "leakyrelu": 2}
CLAMP = {"realnvp": 0, "glow": 1, "softclamp": 2, "none": 3}


def _hw(t):
    return int(t.shape[2]) * int(t.shape[3])


# ----------------------------------------------------------------------------------------------- raw kernels
def squeeze2d_raw(x, undo=False):
    N, C, H, W = x.shape
    xp, xns = L.frames(x, "x")
    if not undo:
        y = torch.empty((N, C * 4, H // 2, W // 2), device=x.device, dtype=x.dtype)
    else:
        y = torch.empty((N, C // 4, H * 2, W * 2), device=x.device, dtype=x.dtype)
    yp, yns = L.frames(y, "y")
    L.call("rfn_squeeze2d_f32", xp, xns, yp, yns, N, C, H, W, 1 if undo else 0, meta=_shell("squeeze2d", x, 2))
    return y


@functools.lru_cache(maxsize=None)
def kernel_label(query, *args):
    """the kernel instantiation the library launches for the integer arguments `args` of its host-only query `query`
    (the *_kernel_label_* functions of include/rfn_hip.h, answered by the function the launcher itself switches on): the
    label of a launch's profiling metadata.  Memoised: the library reads its selector knobs once per process."""
    return getattr(L.load(), query)(*args).decode()


def channel_stats(x):
    """per-channel (mean, unbiased variance) over (N,H,W) — ActNorm data dependent init."""
    N, C = x.shape[0], x.shape[1]
    xp, xns = L.frames(x, "x")
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    var = torch.empty(C, device=x.device, dtype=torch.float32)
    L.call("rfn_channel_stats_f32", xp, xns, L.dev(mean), L.dev(var), N, C, _hw(x))
    return mean, var


def actnorm_invconv_fwd(x, bias, logs, Wm):
    N, C = x.shape[0], x.shape[1]
    xp, xns = L.frames(x, "x")
    z = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    zp, zns = L.frames(z, "z")
    bias, logs, Wm = bias.contiguous(), logs.contiguous(), Wm.contiguous()  # held until the launch is enqueued
    L.call("rfn_actnorm_invconv_fwd_f32", xp, xns, L.dev(bias), L.dev(logs), L.dev(Wm), zp, zns, N, C,
           _hw(x), meta=_shell("actnorm_invconv_fwd", x, 2))
    return z


class ZeroArena:
    """one zero-filled allocation handed out in slices: the accumulate-into outputs of a backward node (weight
    gradients, per-channel sums) share ONE fill launch instead of one torch.zeros each."""

    def __init__(self, numel, device):
        self.buf = torch.zeros(int(numel), device=device, dtype=torch.float32)
        self.off = 0

    def take(self, *shape):
        n = 1
        for d in shape:
            n *= int(d)
        n_al = (n + 3) // 4 * 4  # keep every slice 16-byte aligned
        assert self.off + n <= self.buf.numel(), "ZeroArena exhausted"
        t = self.buf[self.off:self.off + n].view(*shape)
        self.off += n_al
        return t


def _zeros(arena, *shape, device=None):
    return arena.take(*shape) if arena is not None else torch.zeros(shape, device=device, dtype=torch.float32)


def actnorm_invconv_bwd(x, bias, logs, Wm, gz, arena=None, acc=None, glogdet=None):
    """returns (gx, gW, gb, gl).  `acc` (optional): zero-filled (gW, gb, gl) of the caller's to accumulate into.
    `glogdet` [N] (optional): the gradient of a per-frame log-det that includes this ActNorm's term H*W * sum logs, which
    the kernel then adds to gl (rfn_actnorm_invconv_bwd_ld_f32: the first step of a level node)."""
    N, C = x.shape[0], x.shape[1]
    xp, xns = L.frames(x, "x")
    gzp, gzns = L.frames(gz, "gz")
    gx = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    gxp, gxns = L.frames(gx, "gx")
    gW, gb, gl = acc if acc is not None else [_zeros(arena, *s, device=x.device) for s in ((C, C), (C,), (C,))]
    bias, logs, Wm = bias.contiguous(), logs.contiguous(), Wm.contiguous()  # held until the launch is enqueued
    entry, ld = ("rfn_actnorm_invconv_bwd_f32", ()) if glogdet is None else ("rfn_actnorm_invconv_bwd_ld_f32", (L.dev(glogdet),))
    L.call(entry, xp, xns, L.dev(bias), L.dev(logs), L.dev(Wm), gzp, gzns, gxp, gxns, L.dev(gW), L.dev(gb),
           L.dev(gl), *ld, N, C, _hw(x), meta=_shell("actnorm_invconv_bwd", x, 3))
    return gx, gW, gb, gl


def invconv_actnorm_rev(z, bias, logs, Winv):
    N, C = z.shape[0], z.shape[1]
    zp, zns = L.frames(z, "z")
    x = torch.empty(z.shape, device=z.device, dtype=z.dtype)
    xp, xns = L.frames(x, "x")
    bias, logs, Winv = bias.contiguous(), logs.contiguous(), Winv.contiguous()  # held until the launch is enqueued
    L.call("rfn_invconv_actnorm_rev_f32", zp, zns, L.dev(bias), L.dev(logs), L.dev(Winv), xp, xns, N, C, _hw(z))
    return x


class PackBatch:
    """The weight packs one piece of code asks for back to back, launched together (weights change every optimizer
    step: they are re-packed per call).  conv() / dense() return the buffers; leaving the `with` block fills them with at
    most one rfn_pack_conv_weights_hostdescs_bf16x3 and one rfn_smallmap_pack_batched_bf16x3 call, on the stream
    current then.  No buffer may be read before the block is left."""

    def __init__(self):
        self._conv, self._dense, self._keep = [], [], []

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            if self._conv:
                arr = (L.rfn_pack_desc * len(self._conv))(*self._conv)
                L.call("rfn_pack_conv_weights_hostdescs_bf16x3", arr, len(arr))
            if self._dense:
                arr = (L.rfn_smallmap_pack_desc * len(self._dense))(*self._dense)
                L.call("rfn_smallmap_pack_batched_bf16x3", arr, len(arr))
        self._conv, self._dense, self._keep = [], [], []   # (the contiguous weights were held until the launch)

    def conv(self, w, flip=False, prec=None):
        """w [Cout,Cin,k,k] in the layout of the MFMA conv kernels (flip=True: data-gradient conv).  prec: 'bf16x3' |
        'bf16x6' | 'f32' (default: the gradient arithmetic, which is what un-annotated callers are); the f32 pack is
        launched at once."""
        Cout, Cin, ks = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        prec = prec if prec is not None else ("bf16x3" if bwd_b3() else "f32")
        sfx = {"bf16x3": "_bf16x3", "bf16x6": "_bf16x6", "f32": ""}[prec]
        wpk = torch.empty(getattr(L.load(), "rfn_packed_weight_size" + sfx)(Cout, Cin, ks), device=w.device,
                          dtype=torch.float32)
        wc = w.detach().contiguous()
        if prec == "f32":
            L.call("rfn_pack_conv_weight_f32", L.dev(wc, "w"), L.dev(wpk), Cout, Cin, ks, 1 if flip else 0)
            return wpk
        self._conv.append(L.rfn_pack_desc(L.dev(wc, "w").value, wpk.data_ptr(), Cout, Cin, ks,
                                        (1 if flip else 0) + (4 if prec == "bf16x6" else 0)))
        self._keep += [wc, wpk]
        return wpk

    def dense(self, w, H, W, transpose):
        """w [Cout, Cin, 3, 3] -> MFMA-fragment-ordered bf16 (hi, lo) dense matrix of the H x W map (smallmap_dense)"""
        Cout, Cin = int(w.shape[0]), int(w.shape[1])
        nbytes = int(L.load().rfn_smallmap_packed_size(Cout, Cin, H, W, 1 if transpose else 0))
        buf = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
        wc = w.detach().contiguous()
        self._dense.append(L.rfn_smallmap_pack_desc(L.dev(wc, "w").value, buf.data_ptr(), Cout, Cin, int(H), int(W),
                                             1 if transpose else 0, 0))
        self._keep += [wc, buf]
        return buf


def pack_weight(w, flip=False, prec=None):
    """PackBatch.conv of one weight: the buffer is filled when the call returns."""
    with PackBatch() as b:
        return b.conv(w, flip, prec)


def conv2d_dgrad_act(gin, wpk_flip, y, logs, act, Cout, ks, arena=None):
    """data-gradient conv + backward through the producer's ActNorm/activation in one kernel
    (rfn_conv2d_dgrad_act_bf16x3).  Returns (gu, grad_bias[Cout], grad_logs[Cout]); the two per-channel sums are
    accumulated by the kernel (float atomics) into a zeroed [2, Cout] slice of `arena`."""
    N, Cin, H, W = gin.shape
    gp, gns = L.frames(gin, "gin")
    yp, yns = L.frames(y, "y")
    gu = torch.empty((N, Cout, H, W), device=gin.device, dtype=torch.float32)
    up, uns = L.frames(gu, "gu")
    sums = _zeros(arena, 2, Cout, device=gin.device)
    L.call("rfn_conv2d_dgrad_act_bf16x3", gp, gns, Cin, L.dev(wpk_flip), yp, yns, L.dev(logs), act, up,
           uns, L.dev(sums), Cout, N, H, W, ks,
           meta=("conv", kernel_label("rfn_conv2d_kernel_label_bf16x3", 2, ks, Cin, 0, Cout, Cout, 0, 4, N, H, W) + "+actbwd",
                 2.0 * N * H * W * Cin * Cout * ks * ks,
                 "N%d %d->%d %dx%d k%d dgrad+actbwd" % (N, Cin, Cout, H, W, ks),
                 4.0 * (N * H * W * (Cin + 2 * Cout) + Cin * Cout * ks * ks)))
    return gu, sums[0], sums[1]


class PackPlan:
    """Persistent packed-weight buffers for a list of (weight, mode) and the descriptors that refresh all of them
    (rfn_pack_conv_weights_hostdescs_bf16x3, 64 per launch).  mode: 0 forward, 1 data-gradient, 2 tap-expanded 1x1
    (tiny-Cout 3x3); + 4: three planes per operand (bf16x6)."""

    def __init__(self, items):
        self.items = list(items)
        self.ptrs = [w.data_ptr() for w, _ in self.items]
        lib = L.load()
        self.bufs = []
        for w, mode in self.items:
            Cout, Cin, ks = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
            assert w.is_contiguous() and w.dtype == torch.float32
            lc, lk = (9 * Cout, 1) if (mode & 3) == 2 else (Cout, ks)
            size_fn = lib.rfn_packed_weight_size_bf16x6 if (mode & 4) else lib.rfn_packed_weight_size_bf16x3
            self.bufs.append(torch.empty(size_fn(lc, Cin, lk), device=w.device, dtype=torch.float32))
        self.descs = (L.rfn_pack_desc * len(self.items))(*[
            L.rfn_pack_desc(w.data_ptr(), b.data_ptr(), int(w.shape[0]), int(w.shape[1]), int(w.shape[2]), mode)
            for (w, mode), b in zip(self.items, self.bufs)])

    def valid_for(self, items):
        return (len(items) == len(self.items) and all(w.data_ptr() == p for (w, _), p in zip(items, self.ptrs))
                and all(m == m0 for (_, m), (_, m0) in zip(items, self.items)))

    def run(self):
        L.call("rfn_pack_conv_weights_hostdescs_bf16x3", self.descs, len(self.descs))


# ------------------------------------------------------------------------------------------------ fused coupling net
def coupling_po_ok(N, C, Cc, Hd, H, W, w1, w3, any_size=False):
    """shapes the fused forward kernel (csrc/coupling_po.hip) takes; both 3x3 convs must really be 3x3.
    Policy on top of the capability (skipped with any_size): the wide instantiations (more than 40 input channels: level
    2 of the canonical flow) take ~65 us per 128-pixel round -- with fewer rounds than half the CUs (a local batch of 4
    or 8) the three unfused launches, which spread the same work over the whole chip, are faster."""
    if os.environ.get("RFN_COUPLING_PO") == "0" or CONV_PRECISION != "mixed":
        return False
    if tuple(w1.shape[2:]) != (3, 3) or tuple(w3.shape[2:]) != (3, 3):
        return False
    if not any_size and C // 2 + Cc > 40 and N * H * W < 128 * 128:
        return False
    return bool(L.load().rfn_coupling_po_supported(int(N), int(C), int(Cc), int(Hd), int(H), int(W)))


class POPackPlan:
    """Persistent fragment-ordered weight streams of a list of coupling nets [(w1, w2, w3)] and ONE launch that
    refreshes all of them (rfn_coupling_po_pack): weights change every optimizer step."""

    def __init__(self, nets):
        self.nets = [tuple(n) for n in nets]
        self.ptrs = [tuple(w.data_ptr() for w in n) for n in self.nets]
        dev = self.nets[0][0].device
        lib = L.load()
        rec = []
        self.bufs = []
        for w1, w2, w3 in self.nets:
            Cin, C = int(w1.shape[1]), int(w3.shape[0])
            for w in (w1, w2, w3):
                assert w.is_contiguous() and w.dtype == torch.float32
            assert tuple(w2.shape) == (256, 256, 1, 1) and int(w1.shape[0]) == 256 and int(w3.shape[1]) == 256
            buf = torch.empty(int(lib.rfn_coupling_po_packed_bytes(Cin, C)) // 4, device=dev, dtype=torch.float32)
            self.bufs.append(buf)
            rec.append((w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), buf.data_ptr(), Cin, C))
        self.table = torch.frombuffer(self.host_table(rec), dtype=torch.uint8).to(dev)

        # the backward kernel's streams (w3 transposed + mirrored, w2 transposed) for the nets whose gradient image has
        # at most 16 channels (two 8-channel groups: rfn_coupling_po_bwd_supported)
        self.bwd_bufs = [None] * len(self.nets)
        recb = []
        for i, (w1, w2, w3) in enumerate(self.nets):
            C = int(w3.shape[0])
            if C <= 16:
                buf = torch.empty(int(lib.rfn_coupling_po_bwd_packed_bytes(C)) // 4, device=dev, dtype=torch.float32)
                self.bwd_bufs[i] = buf
                recb.append((w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), buf.data_ptr(), int(w1.shape[1]), C))
        self.n_bwd = len(recb)
        if recb:
            self.table_bwd = torch.frombuffer(self.host_table(recb), dtype=torch.uint8).to(dev)

    @staticmethod
    def host_table(rec):
        """the rfn_po_pack_desc array of rows (w1, w2, w3, dst, Cin, C), addresses as ints"""
        return (L.rfn_po_pack_desc * len(rec))(*[L.rfn_po_pack_desc(*r) for r in rec])

    def valid_for(self, nets):
        return len(nets) == len(self.nets) and all(tuple(w.data_ptr() for w in n) == p for n, p in zip(nets, self.ptrs))

    def run(self, bwd=True):
        """`bwd`: also refresh the backward streams (not needed when no gradient will be asked for)"""
        L.call("rfn_coupling_po_pack", self.table.data_ptr(), len(self.nets))
        if bwd and self.n_bwd:
            L.call("rfn_coupling_po_pack_bwd", self.table_bwd.data_ptr(), self.n_bwd)


def coupling_po_fwd(z, cond, wpk, n1b, n1l, n2b, n2l, C, act, want_masks=False):
    """h1, h2, P, masks = fused coupling net on z[:, :C/2] | cond (rfn_coupling_po_fwd); P is the tap-expanded conv3
    output; masks = (m1, m2): the 1-bit "h <= 0" masks of h1 / h2 in the backward kernel's order (None unless asked)."""
    N, _, H, W = z.shape
    Cc = 0 if cond is None else int(cond.shape[1])
    zp, zns = L.frames(z, "z")
    cp, cns = (None, 0) if cond is None else L.frames(cond, "cond")
    h1 = torch.empty((N, 256, H, W), device=z.device, dtype=torch.float32)
    h2 = torch.empty((N, 256, H, W), device=z.device, dtype=torch.float32)
    P = torch.empty((N, 9 * C, H, W), device=z.device, dtype=torch.float32)
    Cin = C // 2 + Cc
    npx = float(N * H * W)
    masks = None
    if want_masks and act != 0:
        nm = int(L.load().rfn_coupling_po_mask_floats(N, H, W))
        masks = (torch.empty(nm, device=z.device, dtype=torch.float32), torch.empty(nm, device=z.device, dtype=torch.float32))
    m1, m2 = masks if masks is not None else (None, None)
    L.call("rfn_coupling_po_fwd", zp, zns, cp, cns, L.dev(wpk), L.dev(n1b), L.dev(n1l), L.dev(n2b), L.dev(n2l),
           L.dev(h1), 256 * H * W, L.dev(h2), 256 * H * W, L.dev(P), 9 * C * H * W, L.dev(m1), L.dev(m2),
           N, C, Cc, H, W, act,
           meta=("conv", "coupling_po_fwd_kernel", 2.0 * npx * (9 * Cin * 256 + 256 * 256 + 9 * C * 256),
                 "N%d %d+%d->256->256->9x%d %dx%d" % (N, C // 2, Cc, C, H, W),
                 4.0 * npx * (Cin + 512 + 9 * C + (16 if masks is not None else 0))
                 + 4.0 * (9 * Cin * 256 + 65536 + 9 * C * 256)))
    return h1, h2, P, masks


def coupling_po_bwd_ok(N, C, H, W):
    return (os.environ.get("RFN_COUPLING_PO_BWD") != "0" and CONV_PRECISION == "mixed"
            and bool(L.load().rfn_coupling_po_bwd_supported(int(N), int(C), int(H), int(W))))


def coupling_po_bwd(go, wpk_bwd, n1l, n2l, masks, act):
    """ga2, ga1, part = fused data-gradient chain of the coupling net from `go` (gradient at conv3's output):
    rfn_coupling_po_bwd.  ga2 / ga1 [N,256,H,W]: gradients at the outputs of conv2 / conv1; part: per-workgroup sums."""
    N, C, H, W = go.shape
    gp, gns = L.frames(go, "go")
    ga2 = torch.empty((N, 256, H, W), device=go.device, dtype=torch.float32)
    ga1 = torch.empty((N, 256, H, W), device=go.device, dtype=torch.float32)
    part = torch.empty(int(L.load().rfn_coupling_po_bwd_part_floats(N, H, W)), device=go.device, dtype=torch.float32)
    m1, m2 = masks if masks is not None else (None, None)
    npx = float(N * H * W)
    L.call("rfn_coupling_po_bwd", gp, gns, L.dev(wpk_bwd), L.dev(n1l), L.dev(n2l), L.dev(m1), L.dev(m2),
           L.dev(ga2), 256 * H * W, L.dev(ga1), 256 * H * W, L.dev(part), N, C, H, W, act,
           meta=("conv", "coupling_po_bwd_kernel", 2.0 * npx * (9 * C * 256 + 256 * 256),
                 "N%d %d->256->256 %dx%d dgrad chain" % (N, C, H, W),
                 4.0 * npx * (C + 512 + (16 if masks is not None else 0)) + 4.0 * (9 * C * 256 + 65536)))
    return ga2, ga1, part


# what rfn_coupling_po_bwd_finish reads of one net, in the order of its arguments, and `step`: the step of a level node
# whose weight gradients gw1 / gw2 the ticket waits for (_net_bwd leaves them None when they are computed later)
FinishTicket = collections.namedtuple("FinishTicket", "part w1 gw1 n1b w2 gw2 n2b out step", defaults=(None,))


def coupling_po_bwd_finish(tickets):
    """ActNorm gradients of the hidden layers of up to 16 nets per launch (rfn_coupling_po_bwd_finish); a ticket is a
    FinishTicket or any sequence (part, w1, gw1, n1b, w2, gw2, n2b, out[4,256]); `out` is written."""
    for i0 in range(0, len(tickets), 16):
        tk = tickets[i0:i0 + 16]
        cols = [L.ptr_array([t[j].detach() for t in tk], "finish") for j in range(8)]
        nblk = int(tk[0][0].numel()) // 512
        K1 = int(tk[0][1].numel()) // 256
        for t in tk:
            assert t[0].numel() == nblk * 512 and t[1].numel() == K1 * 256 and t[2].numel() == K1 * 256
            assert t[4].numel() == 65536 and t[5].numel() == 65536 and t[2].is_contiguous() and t[5].is_contiguous()
        L.call("rfn_coupling_po_bwd_finish", *cols, len(tk), nblk, K1,
               meta=_shell("po_bwd_finish", tk[0][7], len(tk) * (nblk * 512 + 512 * K1 + 131072 + 1024) / 1024.0))


def conv2d_raw(in1, in2, wpk, Cout, ks, ep_mode=0, p0=None, p1=None, act=0, out1=None, out2=None, cout_split=None,
               acc1=False, acc2=False, prec=None):
    """out = epilogue(conv(cat(in1,in2))) ; see rfn_conv2d_fwd_f32.  prec: arithmetic `wpk` was packed for ('bf16x3' |
    'f32'; default: the gradient arithmetic)."""
    N, C1, H, W = in1.shape
    C2 = 0 if in2 is None else int(in2.shape[1])
    i1p, i1ns = L.frames(in1, "in1")
    i2p, i2ns = (None, 0) if in2 is None else L.frames(in2, "in2")
    if cout_split is None:
        cout_split = Cout
    if out1 is None:
        out1 = torch.empty((N, cout_split, H, W), device=in1.device, dtype=torch.float32)
    o1p, o1ns = L.frames(out1, "out1")
    o2p, o2ns = (None, 0) if out2 is None else L.frames(out2, "out2")
    prec = prec if prec is not None else ("bf16x3" if bwd_b3() else "f32")
    fn = {"bf16x3": "rfn_conv2d_fwd_bf16x3", "bf16x6": "rfn_conv2d_fwd_bf16x6", "f32": "rfn_conv2d_fwd_f32"}[prec]
    x6 = prec == "bf16x6"
    kname = (kernel_label("rfn_conv2d_kernel_label_f32", ks, Cout, N, H, W) if prec == "f32" else
             kernel_label("rfn_conv2d_kernel_label_bf16x3", 3 if x6 else 2, ks, C1, C2, Cout, cout_split, 1 if acc1 else 0,
                          ep_mode, N, H, W) + (" x6" if x6 else ""))
    L.call(fn, i1p, i1ns, C1, i2p, i2ns, C2, L.dev(wpk), o1p, o1ns, o2p, o2ns, Cout, cout_split, 1 if acc1 else 0,
           1 if acc2 else 0, N, H, W, ks, ep_mode, L.dev(p0), L.dev(p1), act,
           meta=("conv", kname,
                 2.0 * N * H * W * (C1 + C2) * Cout * ks * ks,
                 "N%d %d+%d->%d %dx%d k%d ep%d%s" % (N, C1, C2, Cout, H, W, ks, ep_mode,
                                                  "" if cout_split == Cout else " split"),
                 4.0 * (N * H * W * (C1 + C2 + Cout) + (C1 + C2) * Cout * ks * ks)))
    return out1


def wgrad_b3(H, W):
    """weight gradients on an H x W map run split precision: the gradient arithmetic, and whole 4-pixel groups for the
    GEMM forms (wgrad_plan; coupling_route defers a level's gradients to grouped launches only then)"""
    return bwd_b3() and H * W % 4 == 0


def _frame_stride(t):   # (as L.frames, layout unchecked)
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]) * _hw(t)


def _b3_launch(G, entry, *args):
    """(entry point, label) of a split-precision weight-gradient launch for G groups (0: the single form `entry`; else its
    _grouped form and the 'grouped' decoration): the label is the library's answer to `entry`'s query for `args`"""
    label = kernel_label(entry.replace("_bf16x3", "_kernel_label_bf16x3"), *args)
    return (entry.replace("_bf16x3", "_grouped_bf16x3"), label.replace("<", "<grouped ")) if G else (entry, label)


def _b3_wgrad(launch, G, operands, M, Nc, dims, arena, tag=""):
    """ONE launch of a GEMM-form entry point, `launch` = (entry point, label), single (G = 0) or grouped: returns the zeroed
    and accumulated gw [max(G, 1), M, Nc].  operands: (the groups' tensors or None, name, channels) in the entry point's
    order, each passed as pointer (G: host array of the groups' pointers), frame stride (the first tensor's, whose layout
    is checked), channels; dims: its last arguments, (frames, pixels) or (frames, H, W).  `tag` names a 3x3 form, whose
    Nc = 9 x channels columns are planes shifted while staging."""
    args = []
    for ts, name, C in operands:
        p, ns = (None, 0) if ts is None else L.frames(ts[0], name)
        args += [L.ptr_array(ts, name) if G and ts is not None else p, ns, C]
    n, F_, HW = max(G, 1), dims[0], dims[1] * (dims[2] if len(dims) > 2 else 1)
    gw = _zeros(arena, n, M, Nc, device=operands[0][0][0].device)
    L.call(launch[0], *args, L.ptr_array(gw.unbind(0), "gw") if G else L.dev(gw), *((G,) if G else ()), *dims,
           meta=("wgrad", launch[1], 2.0 * n * F_ * HW * M * Nc,
                 "%sF%d %dx%d HW%d%s" % ("G%d " % G if G else "", F_, M, Nc, HW, tag),
                 4.0 * n * (F_ * HW * (M + (Nc // 9 if tag else Nc)) + M * Nc)))
    return gw


def _gemm_wgrad(G, a_list, b_list, M, Nc, arena, launch=None):
    """gw [max(G, 1), M, Nc], gw[g] = Σ_{frames,pixels} a_g[f,m,p] b_g[f,n,p] on the split-precision MFMA GEMM
    (rfn_gemm_wgrad[_grouped]_bf16x3): one launch.  `launch`: as a WgradPlan names it, where one does."""
    F_, HW = int(a_list[0].shape[0]), _hw(a_list[0])
    launch = launch or _b3_launch(G, "rfn_gemm_wgrad_bf16x3", M, Nc, _frame_stride(a_list[0]), _frame_stride(b_list[0]), G,
                                  F_, HW)
    return _b3_wgrad(launch, G, [(a_list, "a", M), (b_list, "b", Nc)], M, Nc, (F_, HW), arena)


def gemm_wgrad(a, b, M, Nc, arena=None):
    return _gemm_wgrad(0, [a], [b], M, Nc, arena)[0]


def gemm_wgrad_grouped(a_list, b_list, M, Nc, arena=None):
    """G gradients of one shape (at most 16) in ONE launch"""
    return _gemm_wgrad(len(a_list), a_list, b_list, M, Nc, arena)


_grouped_wgrad_budget = {}  # device index -> bytes


def grouped_wgrad_budget(device):
    """bytes of operands a flow level may keep alive to compute its 3 K weight gradients in grouped launches:
    RFN_WGRAD_GROUPED_MAX_BYTES, or one eighth of the device's memory (read once per device)"""
    env = os.environ.get("RFN_WGRAD_GROUPED_MAX_BYTES")
    if env is not None:
        return int(env)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _grouped_wgrad_budget:
        _grouped_wgrad_budget[idx] = torch.cuda.get_device_properties(idx).total_memory // 8
    return _grouped_wgrad_budget[idx]


def grouped_wgrad_retained_bytes(Kn, N, Hd, HW, o_numel):
    """what deferring the weight gradients of a level of Kn steps keeps alive until the level ends: the two hidden
    gradients gh1, gh2 [N, Hd, HW] of every step, and the Kn conv3-output gradients stacked in one buffer (o_numel
    elements each); h1 / h2 and the step inputs are saved tensors either way"""
    return 4 * Kn * (2 * N * Hd * HW + o_numel)


def group_level_wgrad(Kn, N, Hd, HW, o_numel, device):
    """grouped launches add no atomic bytes and idle no CU at any shape (the ring kernels split the flat stage space of
    the groups evenly): memory is the only reason not to group.  RFN_WGRAD_GROUPED=0: one launch per step."""
    return (1 < Kn <= 16 and os.environ.get("RFN_WGRAD_GROUPED") != "0" and
            grouped_wgrad_retained_bytes(Kn, N, Hd, HW, o_numel) <= grouped_wgrad_budget(device))


WgradPlan = collections.namedtuple("WgradPlan", "form G M Nc launches")
_TAP_SCATTER, _IM2COL = ("rfn_tap_scatter_f32", "tap_scatter"), ("rfn_im2col3x3_f32", "im2col3x3")


def wgrad_short_rows():
    """what the training path passes as wgrad_plan's `short_rows`: true unless RFN_WGRAD_SHORT_ROWS=0 (A/B runs)"""
    return os.environ.get("RFN_WGRAD_SHORT_ROWS") != "0"


WGRAD_BAND_MIN_PIXELS = (1 << 15, 1 << 17)


def wgrad_band_min_pixels(Cout=1):
    """fewest pixels N * H * W at which an ungrouped 3x3 gradient with Cout <= 128 and Cin <= 128 takes the band kernel:
    RFN_WGRAD_BAND_MIN_PIXELS, or 2^15 up to 32 output channels (one row tile: the kernel that prefetches the next band)
    and 2^17 above (two row tiles, a longer tail of atomics: between 2^13 and 2^17 pixels it loses to the implicit
    kernel on some shapes) -- tools/bench_wgrad.py band, DESIGN.md section 4.  RFN_WGRAD_BAND=0: never."""
    env = os.environ.get("RFN_WGRAD_BAND_MIN_PIXELS")
    return int(env) if env is not None else WGRAD_BAND_MIN_PIXELS[0 if Cout <= 32 else 1]


def wgrad_plan(G, N, C1, C2, Cout, H, W, ks, g_ns=None, in1_ns=None, few_out=False, min_pixels=0, stacked=False,
               short_rows=False):
    """How the weight gradient(s) [Cout, C1 + C2, ks, ks] of a convolution on N frames of H x W are computed, from shapes,
    strides and options alone (no tensor, no device): the one decision of the path, which _wgrad_run executes and the
    host tests query.  G = 0: one gradient; G >= 1: G of one shape in grouped launches.  g_ns / in1_ns: frame strides
    of the output gradient and of the first input source (default: dense).  few_out: the caller is a Conv2dZeros
    (one-source input), which alone may take the mirrored kernel (from `min_pixels` pixels G * N * H * W) or the fp32
    tap route.  stacked: the G output gradients are the slices of one contiguous [G, N, Cout, H, W] buffer.
    short_rows: on maps whose rows are shorter than a staging unit (4 x 4, 2 x 2: where the library's query names a
    kernel) a split-precision 3x3 gradient is ONE launch that shifts the taps while staging -- "mirrored_rows" for a
    Conv2dZeros, "implicit_rows" for every other conv whatever Cin against Cout (no cat of a two-source input) --
    instead of im2col / tap scatter + GEMM.  The training path passes wgrad_short_rows().
    "band": an ungrouped split-precision 3x3 gradient with Cout <= 128, Cin <= 128 and W % 8 == 0 on at least
    wgrad_band_min_pixels(Cout) pixels N * H * W, where the library names a band kernel -- one launch, either orientation.
    Returns WgradPlan(form, G, M, Nc, launches): the form (table in DESIGN.md, "Where the labels come from"), the GEMM
    dimensions gw[M][Nc] and, in order, the (entry point, label) of every library launch.  CONV_PRECISION,
    RFN_WGRAD_IMPLICIT, RFN_WGRAD_MIRRORED, RFN_WGRAD_BAND[_MIN_PIXELS] and the label queries are read on every call."""
    Cin, HW, n = C1 + C2, H * W, max(G, 1)
    g_ns = Cout * HW if g_ns is None else g_ns
    in1_ns = C1 * HW if in1_ns is None else in1_ns
    x_ns = in1_ns if C2 == 0 else Cin * HW   # the input as ONE GEMM operand: in1 itself, or cat(in1, in2)
    b3 = wgrad_b3(H, W)
    scatter = [_TAP_SCATTER] * (1 if stacked else n)   # a launch per gradient, or one over the stacked G * N frames
    assert not (few_out and C2)

    def plan(form, M, Nc, *launches):
        return WgradPlan(form, G, M, Nc, list(launches))

    def gemm(M, Nc, a_ns, b_ns):
        return _b3_launch(G, "rfn_gemm_wgrad_bf16x3", M, Nc, a_ns, b_ns, G, N, HW)

    def f32(k, Co):
        return ("rfn_conv2d_wgrad_f32", kernel_label("rfn_conv2d_wgrad_kernel_label_f32", k, Cin, Co, H, W))

    if not b3 and not G:   # the fp32-MFMA kernel (a group is always split precision: CouplingRoute.defer_wgrad)
        if few_out and ks == 3 and Cout <= TAP_MAX_COUT:   # as a 1x1 conv to the 9 Cout tap-scattered channels
            return plan("scatter_f32", 9 * Cout, Cin, *scatter, f32(1, 9 * Cout))
        return plan("f32", Cout, ks * ks * Cin, f32(ks, Cout), *([("rfn_wgrad_finish_f32", "wgrad_finish")] if ks > 1 else []))
    if ks == 1:
        return plan("gemm", Cout, Cin, gemm(Cout, Cin, g_ns, x_ns))
    if short_rows and b3 and ks == 3:
        if few_out:
            launch = _b3_launch(G, "rfn_conv3x3_wgrad_rows_mirrored_bf16x3", Cin, in1_ns, Cout, G, N, H, W)
            if launch[1]:   # ('': the short-row staging does not cover this map)
                return plan("mirrored_rows", Cin, 9 * Cout, launch)
        else:
            launch = _b3_launch(G, "rfn_conv3x3_wgrad_rows_bf16x3", Cout, g_ns, G, N, H, W)
            if launch[1]:
                return plan("implicit_rows", Cout, 9 * Cin, launch)
    if (ks == 3 and b3 and not G and Cout <= 128 and Cin <= 128 and W % 8 == 0 and N * HW >= wgrad_band_min_pixels(Cout)
            and os.environ.get("RFN_WGRAD_BAND") != "0"):
        # both channel counts small, whichever is larger: bands of image rows staged once, every tap an LDS address
        launch = _b3_launch(0, "rfn_conv3x3_wgrad_band_bf16x3", Cout, Cin, N, H, W)
        if launch[1]:   # ('': no band of this map fits the kernel's LDS image)
            return plan("band", Cout, 9 * Cin, launch)
    if Cin <= Cout:   # the input is the small operand: its shifted planes built while staging, or expanded in memory
        if W % 8 == 0 and os.environ.get("RFN_WGRAD_IMPLICIT") != "0":
            return plan("implicit", Cout, 9 * Cin,
                        _b3_launch(G, "rfn_conv3x3_wgrad_implicit_bf16x3", Cout, g_ns, G, N, H, W))
        return plan("im2col", Cout, 9 * Cin, *[_IM2COL] * n, gemm(Cout, 9 * Cin, g_ns, 9 * Cin * HW))
    if few_out and ks == 3 and b3 and os.environ.get("RFN_WGRAD_MIRRORED") != "0" and n * N * HW >= min_pixels:
        launch = _b3_launch(G, "rfn_conv3x3_wgrad_mirrored_bf16x3", Cin, in1_ns, Cout, G, N, H, W)
        if launch[1]:   # ('': the library names no mirrored kernel for this shape)
            return plan("mirrored", Cin, 9 * Cout, launch)
    return plan("scatter", 9 * Cout, Cin, *scatter, gemm(9 * Cout, Cin, 9 * Cout * HW, x_ns))


def _wgrad_run(plan, in1s, in2s, gs, ks, arena=None, g_stacked=None):
    """The launches of `plan` and the layout fix-up: the n = max(plan.G, 1) weight gradients (list of contiguous tensors or
    views [Cout, Cin, ks, ks]) of the convolutions of cat(in1s[i], in2s[i]) -- in2s None: one source -- with output
    gradients gs[i].  `plan` is wgrad_plan of these operands; every launch takes its entry point and label from
    plan.launches, in order.  g_stacked: the gradients as one buffer, iff the plan was made with `stacked`.  Strided
    frames go to the implicit and GEMM forms as they are; the scatter and mirrored forms make their gradient dense.
    One arena take and one transposing copy per call, whatever G."""
    G, n, form = plan.G, max(plan.G, 1), plan.form
    N, C1, H, W = in1s[0].shape
    C2 = 0 if in2s is None else int(in2s[0].shape[1])
    Cin, Cout, dev_ = C1 + C2, int(gs[0].shape[1]), in1s[0].device
    todo = iter(plan.launches)

    def cat():
        return in1s if in2s is None else [torch.cat((a, b), 1) for a, b in zip(in1s, in2s)]

    def tap_scatter():
        """the gradients' tap-scattered copies [N, 9 Cout, H, W]: a launch each, or one over the n * N frames of g_stacked"""
        srcs = gs if g_stacked is None else [g_stacked]
        outs = [torch.empty(tuple(s.shape[:-3]) + (9 * Cout, H, W), device=dev_, dtype=torch.float32) for s in srcs]
        for s, o in zip(srcs, outs):
            entry, label = next(todo)
            L.call(entry, L.dev(s.contiguous()), L.dev(o), o.numel() // (9 * Cout * H * W), Cout, H, W,
                   meta=_shell(label, o, 10.0 / 9.0))
        return outs if g_stacked is None else list(outs[0].unbind(0))

    if form in ("f32", "scatter_f32"):
        g, Co, k = (gs[0], Cout, ks) if form == "f32" else (tap_scatter()[0], 9 * Cout, 1)
        i1p, i1ns = L.frames(in1s[0], "in1")
        i2p, i2ns = (None, 0) if in2s is None else L.frames(in2s[0], "in2")
        gp, gns = L.frames(g, "g")
        gwt = _zeros(arena, k * k, Co, Cin, device=dev_)
        entry, label = next(todo)
        L.call(entry, i1p, i1ns, C1, i2p, i2ns, C2, gp, gns, Co, L.dev(gwt), N, H, W, k,
               meta=("wgrad", label, 2.0 * N * H * W * Cin * Co * k * k, "N%d %d->%d %dx%d k%d" % (N, Cin, Co, H, W, k),
                     4.0 * (N * H * W * (Cin + Co) + Cin * Co * k * k)))
        if form == "scatter_f32":
            out = [gwt.view(3, 3, Cout, Cin).permute(2, 3, 0, 1).contiguous()]   # from [tap * Cout + co][ci]
        elif ks == 1:
            out = [gwt.view(Cout, Cin, 1, 1)]  # tap-major == torch layout when there is a single tap
        else:
            out = [torch.empty((Cout, Cin, ks, ks), device=dev_, dtype=torch.float32)]
            entry, label = next(todo)
            L.call(entry, L.dev(gwt), L.dev(out[0]), Cout, Cin, ks, 0, meta=_shell(label, out[0], 2))
    elif form == "gemm":
        out = [t.view(Cout, Cin, 1, 1) for t in _gemm_wgrad(G, gs, cat(), Cout, Cin, arena, next(todo))]
    elif form in ("implicit", "implicit_rows", "band"):   # rows (ci, tap) of the shifted operand: already the torch layout
        gw = _b3_wgrad(next(todo), G, [(gs, "g", Cout), (in1s, "in1", C1), (in2s, "in2", C2)], Cout, 9 * Cin, (N, H, W), arena,
                       " %s3x3" % form)
        out = [t.view(Cout, Cin, 3, 3) for t in gw]
    elif form == "im2col":
        x9s = [torch.empty((N, 9 * Cin, H, W), device=dev_, dtype=torch.float32) for _ in range(n)]
        for i, x9 in enumerate(x9s):
            i1p, i1ns = L.frames(in1s[i], "in1")
            i2p, i2ns = (None, 0) if in2s is None else L.frames(in2s[i], "in2")
            entry, label = next(todo)
            L.call(entry, i1p, i1ns, C1, i2p, i2ns, C2, L.dev(x9), N, H, W, meta=_shell(label, x9, 10.0 / 9.0))
        gw = _gemm_wgrad(G, gs, x9s, Cout, 9 * Cin, arena, next(todo))  # [g][co][tap*Cin + ci]
        out = list(gw.view(n, Cout, 9, Cin).permute(0, 1, 3, 2).reshape(n, Cout, Cin, 3, 3))  # one copy for all groups
    elif form == "scatter":
        xs, gss = cat(), tap_scatter()
        gw = _gemm_wgrad(G, gss, xs, 9 * Cout, Cin, arena, next(todo))  # [g][tap*Cout + co][ci]
        out = list(gw.view(n, 3, 3, Cout, Cin).permute(0, 3, 4, 1, 2).contiguous())
    else:   # mirrored[_rows]: the input as it is, the (dense) gradient shifted while staging; gw is [g][ci][co][tap]
        assert form in ("mirrored", "mirrored_rows"), plan
        gw = _b3_wgrad(next(todo), G, [(in1s, "x", Cin), ([g.contiguous() for g in gs], "g", Cout)], Cin, 9 * Cout, (N, H, W),
                       arena, " %s3x3" % form)
        out = list(gw.view(n, Cin, Cout, 3, 3).permute(0, 2, 1, 3, 4).contiguous())
    assert next(todo, None) is None, plan
    return out


def _conv_wgrad(G, in1s, in2s, gs, Cout, ks, arena, g_stacked=None, few_out=False, min_pixels=0, short_rows=False):
    """wgrad_plan of the operands, executed: what every public weight-gradient function of a convolution is"""
    N, C1, H, W = in1s[0].shape
    if in2s is not None and in2s[0] is None:
        in2s = None
    if not (G and g_stacked is not None and g_stacked.is_contiguous() and tuple(g_stacked.shape) == (G, N, Cout, H, W)):
        g_stacked = None   # (else the G gradients are its slices, in list order)
    plan = wgrad_plan(G, N, C1, 0 if in2s is None else int(in2s[0].shape[1]), Cout, H, W, ks, _frame_stride(gs[0]),
                      _frame_stride(in1s[0]), few_out, min_pixels, g_stacked is not None, short_rows)
    return _wgrad_run(plan, in1s, in2s, gs, ks, arena, g_stacked)


def conv2d_wgrad_grouped(in1_list, in2_list, g_list, Cout, ks, arena=None, g_stacked=None, short_rows=False):
    """the weight gradients of G convolutions of ONE shape (the K steps of a flow level) in grouped launches: list of G
    tensors [Cout, Cin, ks, ks].  g_stacked: the buffer the G gradients are slices of, if they are."""
    return _conv_wgrad(len(g_list), in1_list, in2_list, g_list, Cout, ks, arena, g_stacked, short_rows=short_rows)


def conv2d_wgrad(in1, in2, g, Cout, ks, arena=None, short_rows=False):
    """returns gw [Cout, Cin, ks, ks]"""
    return _conv_wgrad(0, [in1], None if in2 is None else [in2], [g], Cout, ks, arena, short_rows=short_rows)[0]


TAP_MAX_COUT = 8  # 3x3 convs with at most this many outputs run tap-expanded (1x1 to 9*C channels + shift-add)


def zeros_conv_uses_taps(w):
    return int(w.shape[2]) == 3 and int(w.shape[0]) <= TAP_MAX_COUT


def _tap_expanded(w):   # w [C, Cin, 3, 3] as the 1x1 weight [tap * C + co][ci]
    return w.detach().permute(2, 3, 0, 1).reshape(9 * int(w.shape[0]), int(w.shape[1]), 1, 1).contiguous()


def zeros_conv_fwd(x, w, b, logs, wpk=None, prec=None, taps=None):
    """Conv2dZeros forward (glow_modules.py:119-121): (conv3x3(x) + b) * exp(3 logs).  Tiny Cout -> tap-expanded
    (`taps`; default zeros_conv_uses_taps(w)).  `wpk` (optional): pre-packed weight (mode 2 = tap-expanded with `taps`,
    else mode 0), packed for `prec` (default: this map's forward arithmetic)."""
    C, ks = int(w.shape[0]), int(w.shape[2])
    N, _, H, W = x.shape
    if prec is None:
        prec = fwd_prec(H, W)
    if not (zeros_conv_uses_taps(w) if taps is None else taps):
        return conv2d_raw(x, None, wpk if wpk is not None else pack_weight(w, prec=prec), C, ks, 2, b, logs, 0, prec=prec)
    if wpk is None:
        wpk = pack_weight(_tap_expanded(w), prec=prec)
    P = conv2d_raw(x, None, wpk, 9 * C, 1, prec=prec)
    o = torch.empty((N, C, H, W), device=x.device, dtype=torch.float32)
    L.call("rfn_tap_gather_f32", L.dev(P), L.dev(b), L.dev(logs), L.dev(o), N, C, H, W,
           meta=_shell("tap_gather", P, 10.0 / 9.0))
    return o


def zeros_conv_wgrad(x, g_pre, C, ks, arena=None, short_rows=False):
    """weight gradient of the conv inside Conv2dZeros given g_pre = grad wrt (conv + b): wgrad_plan with few_out"""
    return _conv_wgrad(0, [x], None, [g_pre], C, ks, arena, few_out=True, short_rows=short_rows)[0]


LEVEL_MIRRORED_MIN_PIXELS = 1 << 17


def level_mirrored_min_pixels():
    """fewest pixels G * N * H * W of a flow level's K conv3 gradients at which the level node takes the mirrored launch:
    RFN_WGRAD_MIRRORED_MIN_PIXELS, or 2^17.  Smaller levels keep tap scatter + GEMM, the route they had: just above the
    ring threshold (100 000 pixels) the two routes are within 8 us of each other either way."""
    env = os.environ.get("RFN_WGRAD_MIRRORED_MIN_PIXELS")
    return int(env) if env is not None else LEVEL_MIRRORED_MIN_PIXELS


def zeros_conv_wgrad_grouped(h2_list, go_list, C, arena=None, g_stacked=None, ks=3, min_pixels=0, short_rows=False):
    """zeros_conv_wgrad for the G convolutions of one shape of a flow level: list of G tensors [C, Cin, ks, ks]; the
    mirrored launch only where the G groups have `min_pixels` pixels together"""
    return _conv_wgrad(len(go_list), h2_list, None, go_list, C, ks, arena, g_stacked, True, min_pixels, short_rows)


def conv_epilogue_bwd(y, gy, logs, ep_mode, act, want_gl=True, arena=None, inplace=True):
    """gu from gy (in place on gy, or -- inplace=False: gy is somebody else's tensor -- into a new one); returns
    (gu, gb, gl).  gb / gl are accumulated by the kernel: one zero fill for both."""
    N, C = gy.shape[0], gy.shape[1]
    yp, yns = (None, 0) if y is None else L.frames(y, "y")
    gp, gns = L.frames(gy, "gy")
    gu = gy if inplace else torch.empty_like(gy, memory_format=torch.contiguous_format)
    up, uns = L.frames(gu, "gu")
    gbl = _zeros(arena, 2 if want_gl else 1, C, device=gy.device)
    gb, gl = gbl[0], (gbl[1] if want_gl else None)
    L.call("rfn_conv_epilogue_bwd_f32", yp, yns, gp, gns, up, uns, L.dev(logs), L.dev(gb), L.dev(gl),
           N, C, _hw(gy), ep_mode, act, meta=_shell("conv_epilogue_bwd", gy, 3))
    return gu, gb, gl


def affine_coupling_(z, o, scale, scale_shift, logdet, clamp_type, reverse):
    """in place on z's second channel half; logdet [N] updated in place (may be None)."""
    N, C = z.shape[0], z.shape[1]
    zp, zns = L.frames(z, "z")
    op, ons = L.frames(o, "o")
    L.call("rfn_affine_coupling_f32", zp, zns, op, ons, L.dev(scale), L.dev(scale_shift), L.dev(logdet),
           clamp_type, 1 if reverse else 0, N, C, _hw(z), meta=_shell("affine_coupling", z, 2))


def gather_affine_(z, o, P, b3, l3, scale, scale_shift, clamp_type):
    """fused shell tail of the forward Glow step (rfn_gather_affine_f32): with P the tap-expanded Conv2dZeros output is
    gathered, biased and scaled here (written to a fresh o); z's second channel half is coupled in place.
    Returns (o, dlogdet[N]) -- dlogdet is written by the kernel, not accumulated."""
    N, C, H, W = z.shape
    zp, zns = L.frames(z, "z")
    dlogdet = torch.empty(N, device=z.device, dtype=torch.float32)
    if P is not None:
        o = torch.empty((N, C, H, W), device=z.device, dtype=torch.float32)
        L.call("rfn_gather_affine_f32", L.dev(P), None, 0, L.dev(b3), L.dev(l3), L.dev(o), zp, zns, L.dev(scale),
               L.dev(scale_shift), L.dev(dlogdet), clamp_type, N, C, H, W,
               meta=_shell("gather_affine", z, 9 + 1 + 1))  # P read (9x), o written, z2 read + written (2 x 1/2)
    else:
        op, ons = L.frames(o, "o")
        L.call("rfn_gather_affine_f32", None, op, ons, None, None, None, zp, zns, L.dev(scale), L.dev(scale_shift),
               L.dev(dlogdet), clamp_type, N, C, H, W, meta=_shell("gather_affine", z, 2))
    return o, dlogdet


def gauss_logp(z, o, layout, std_mode):
    N, Cz = z.shape[0], z.shape[1]
    zp, zns = L.frames(z, "z")
    op, ons = L.frames(o, "o")
    logp = torch.zeros(N, device=z.device, dtype=torch.float32)
    L.call("rfn_gauss_logp_f32", zp, zns, op, ons, L.dev(logp), layout, std_mode, N, Cz,
           _hw(z), meta=_shell("gauss_logp", z, 3))
    return logp


def gauss_sample(o, eps, layout, std_mode, temperature):
    """z = mean + std * temperature * eps (rfn_gauss_sample_f32).  temperature: a number, or a float32 device tensor of N
    elements, one temperature per frame (rfn_gauss_sample_rows_f32: the same kernel, so rows holding a number's value
    give that number's bits)."""
    N, C2 = o.shape[0], o.shape[1]
    Cz = C2 // 2
    if isinstance(temperature, torch.Tensor):
        if temperature.dtype != torch.float32:
            raise TypeError("gauss_sample: a temperature tensor must be float32, got %s" % temperature.dtype)
        if temperature.device != o.device:
            raise ValueError("gauss_sample: temperature is on %s, o on %s" % (temperature.device, o.device))
        if temperature.numel() != N:
            raise ValueError("gauss_sample: temperature holds %d values for %d frames" % (temperature.numel(), N))
        temperature = temperature.contiguous()
    elif isinstance(temperature, bool) or not isinstance(temperature, (int, float)):
        raise TypeError("gauss_sample: temperature must be a number or a float32 tensor, got %s" %
                        type(temperature).__name__)
    z = torch.empty((N, Cz) + tuple(o.shape[2:]), device=o.device, dtype=torch.float32)
    op, ons = L.frames(o, "o")
    zp, zns = L.frames(z, "z")
    if isinstance(temperature, torch.Tensor):
        L.call("rfn_gauss_sample_rows_f32", op, ons, L.dev(eps.contiguous(), "eps"), zp, zns,
               L.dev(temperature, "temperature"), layout, std_mode, N, Cz, _hw(o))
    else:
        L.call("rfn_gauss_sample_f32", op, ons, L.dev(eps.contiguous(), "eps"), zp, zns,
               float(temperature), layout, std_mode, N, Cz, _hw(o))
    return z


# ----------------------------------------------------------------------------------------------- autograd Functions
class Squeeze2dFn(torch.autograd.Function):
    """Flow/glow_modules.py:298-310; backward = the opposite permutation."""

    @staticmethod
    def forward(ctx, x, undo):
        ctx.undo = undo
        return squeeze2d_raw(x, undo)

    @staticmethod
    def backward(ctx, g):
        return squeeze2d_raw(g.contiguous(), not ctx.undo), None


def fewcin_ok(in1, in2, w, ep_mode):
    """the direct fp32 kernel for 3x3 convolutions of 1 .. 4-channel images (csrc/conv.hip, rfn_conv3x3_fewcin_fwd_f32)"""
    return (in2 is None and ep_mode == 0 and tuple(w.shape[2:]) == (3, 3) and os.environ.get("RFN_FEWCIN") != "0"
            and bool(L.load().rfn_conv3x3_fewcin_supported(int(w.shape[1]), int(w.shape[0]))))


def conv3x3_fewcin(x, w):
    N, Cin, H, W = x.shape
    Cout = int(w.shape[0])
    xp, xns = L.frames(x, "x")
    out = torch.empty((N, Cout, H, W), device=x.device, dtype=torch.float32)
    wc = w.detach().contiguous()
    L.call("rfn_conv3x3_fewcin_fwd_f32", xp, xns, Cin, L.dev(wc), L.dev(out), Cout * H * W, Cout, N,
           H, W, meta=_shell("conv3x3_fewcin_fwd", out, 1.0 + Cin / Cout))
    return out


def conv3x3_c1_wgrad16(x, g):
    N, _, H, W = x.shape
    xp, xns = L.frames(x, "x")
    gp, gns = L.frames(g, "g")
    gw = torch.zeros((16, 1, 3, 3), device=x.device, dtype=torch.float32)
    L.call("rfn_conv3x3_c1_wgrad16_f32", xp, xns, gp, gns, L.dev(gw), N, H, W,
           meta=_shell("conv3x3_c1_wgrad", g, 1.0 + 1.0 / 16))
    return gw


class ConvFn(torch.autograd.Function):
    """epilogue(conv(cat(in1, in2), w)) with the epilogue of rfn_conv2d_fwd_f32.
    p0/p1: ep_mode 1 -> (actnorm bias, actnorm logs); 2 -> (conv bias, logs); 3 -> (conv bias, None)."""

    @staticmethod
    def forward(ctx, in1, in2, w, p0, p1, ep_mode, act, prec=None, packs=None):
        # packs: (forward pack, data-gradient pack or None) from the caller's PackBatch (run_time_batched), else packed here
        Cout, ks = int(w.shape[0]), int(w.shape[2])
        ctx.pk_b = None if packs is None else packs[1]
        p0f = None if p0 is None else p0.detach().reshape(-1).contiguous()
        p1f = None if p1 is None else p1.detach().reshape(-1).contiguous()
        fp = prec if prec is not None else fwd_prec(int(in1.shape[2]), int(in1.shape[3]))
        if fewcin_ok(in1, in2, w, ep_mode):
            y = conv3x3_fewcin(in1, w)   # the extractor's first convolution (1 .. 4 image channels): exact fp32 FMAs
        else:
            y = conv2d_raw(in1, in2, packs[0] if packs is not None and packs[0] is not None else pack_weight(w, prec=fp),
                           Cout, ks, ep_mode, p0f, p1f, act, prec=fp)
        ctx.save_for_backward(in1, in2, w, p1f, y)
        ctx.cfg = (ep_mode, act, None if p0 is None else p0.shape, None if p1 is None else p1.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        in1, in2, w, p1f, y = ctx.saved_tensors
        ep_mode, act, p0shape, p1shape = ctx.cfg
        Cout, Cin, ks = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        gy = gy.contiguous()
        gp0 = gp1 = None
        if ep_mode != 0:
            # (out of place: the incoming gradient belongs to autograd)
            gy, gb, gl = conv_epilogue_bwd(y if ep_mode != 3 else None, gy, p1f, ep_mode, act, ep_mode != 3, inplace=False)
            gp0 = gb.view(p0shape)
            gp1 = gl.view(p1shape) if gl is not None else None
        g1 = g2 = gw = None
        C1 = int(in1.shape[1])
        need1, need2 = ctx.needs_input_grad[0], in2 is not None and ctx.needs_input_grad[1]
        if need1 or need2:
            wt = ctx.pk_b if ctx.pk_b is not None else pack_weight(w, flip=True)
            N, _, H, W = in1.shape
            g1 = torch.empty(in1.shape, device=gy.device, dtype=torch.float32)
            if in2 is not None:
                g2 = torch.empty(in2.shape, device=gy.device, dtype=torch.float32)
            conv2d_raw(gy, None, wt, Cin, ks, 0, None, None, 0, out1=g1, out2=g2, cout_split=C1)
        if ctx.needs_input_grad[2]:
            if fewcin_ok(in1, in2, w, ep_mode) and Cin == 1 and Cout == 16:
                gw = conv3x3_c1_wgrad16(in1, gy)
            else:
                gw = conv2d_wgrad(in1, in2, gy, Cout, ks, short_rows=wgrad_short_rows())
        return g1, g2, gw, gp0, gp1, None, None, None, None


def conv_ep(in1, in2, w, p0, p1, ep_mode, act, prec=None, packs=None):
    """`prec` (optional): forward arithmetic ('bf16x3' | 'bf16x6' | 'f32') instead of this map size's default;
    `packs` (optional): (forward pack in that arithmetic, data-gradient pack or None) already packed by the caller"""
    return ConvFn.apply(in1, in2, w, p0, p1, ep_mode, act, prec, packs)


# the packed weights of one Glow step's coupling net, kept fresh by the caller (Flow/glow.py ListGlow._packed_weights).
# *_fwd / *_dgrad: conv packs of the forward (in the map's split forward arithmetic) / data-gradient convolutions;
# po_fwd / po_bwd: the fused kernels' weight streams (POPackPlan); *_dense_*: dense small-map packs (smallmap_conv).
# CouplingRoute.packs names the fields a step reads; one that is read and left None is packed on the spot (_pack).
StepPacks = collections.namedtuple("StepPacks", ["w1_fwd", "w1_dgrad", "w2_fwd", "w2_dgrad", "w3_fwd", "w3_dgrad",
                                                 "po_fwd", "po_bwd", "w1_dense_fwd", "w3_dense_fwd", "w1_dense_dgrad"],
                                   defaults=(None,) * 11)


def _pack(pk, name, make):
    """the pack `name` of a step from `pk` (a dict of StepPacks fields); one not given is packed now and kept there"""
    if pk.get(name) is None:
        pk[name] = make()
    return pk[name]


def dgrad_small_ok(N, Cin, Cout, H, W, ks):
    """the dedicated few-output-channel 3x3 kernel (csrc/dgrad_small.hip) serves this data-gradient convolution"""
    return (ks == 3 and bwd_b3() and os.environ.get("RFN_DGRAD_SMALL") != "0"
            and bool(L.load().rfn_dgrad_small_supported(int(N), int(Cin), int(Cout), int(H), int(W))))


def conv3x3_smallcout(x, wpk, Cout, out1, out2=None, cout_split=None, acc1=False, acc2=False):
    """rfn_conv3x3_smallcout_bf16x3: 3x3 / pad 1 convolution of x [N, Cin, H, W] with the packed weight `wpk`
    (pack_weight(..., flip=True) for a data gradient) into out1 (channels [0, cout_split)) and out2 (the rest)."""
    N, Cin, H, W = x.shape
    if cout_split is None:
        cout_split = Cout
    xp, xns = L.frames(x, "x")
    o1p, o1ns = L.frames(out1, "out1")
    o2p, o2ns = (None, 0) if out2 is None else L.frames(out2, "out2")
    L.call("rfn_conv3x3_smallcout_bf16x3", xp, xns, Cin, L.dev(wpk), o1p, o1ns, o2p, o2ns, Cout,
           cout_split, 1 if acc1 else 0, 1 if acc2 else 0, N, H, W,
           meta=("conv", "dgrad_small_kernel", 2.0 * N * H * W * Cin * Cout * 9,
                 "N%d %d->%d %dx%d k3 dgrad" % (N, Cin, Cout, H, W), 4.0 * (N * H * W * (Cin + Cout) + Cin * Cout * 9)))
    return out1


CouplingRoute = collections.namedtuple("CouplingRoute", "fwd fwd_prec conv1 conv3 masks bwd_chain dgrad1 defer_wgrad packs")
_WeightShape = collections.namedtuple("_WeightShape", "shape")   # all that the predicates read of a weight


def coupling_route(N, C, Cc, Hd, H, W, k1, k2, k3, act, grad, reverse=False):
    """The kernels that serve the net C/2 + Cc -> Hd -> Hd -> C (kernel sizes k1, k2, k3, activation code `act`) of a Glow
    step on N frames of H x W, and the StepPacks fields they read: a function of the shape, CONV_PRECISION and the RFN_*
    knobs, all read on every call.  The coupling path asks the predicates here and nowhere else; DESIGN.md ("Where the
    labels come from") lists the fields.  The backward fields are None / False unless `grad` (a backward may follow).
    `reverse`: generation, which has no backward, keeps to the conv kernels and keeps forward packs in any arithmetic."""
    Ch, back = C // 2, grad and not reverse
    w1, w3 = _WeightShape((Hd, Ch + Cc, k1, k1)), _WeightShape((C, Hd, k3, k3))
    k33, b3, fp = k1 == 3 and k3 == 3, bwd_b3() and Hd % 64 == 0, fwd_prec(H, W)
    po = k2 == 1 and coupling_po_ok(N, C, Cc, Hd, H, W, w1, w3)
    conv1 = "dense" if k33 and not reverse and smallmap_conv_ok(H, W, Ch, Cc, Hd, N) else "conv"
    conv3 = ("taps" if zeros_conv_uses_taps(w3) else
             "dense" if k33 and not reverse and smallmap_conv_ok(H, W, Hd, 0, C, N) else "conv")
    packs = (("po_fwd",) if po else () if fp == "f32" and not reverse else   # (a step's forward packs are split ones)
             ("w1_dense_fwd" if conv1 == "dense" else "w1_fwd", "w2_fwd", "w3_dense_fwd" if conv3 == "dense" else "w3_fwd"))
    po_bwd = back and coupling_po_bwd_ok(N, C, H, W)
    chain = dgrad1 = None
    if back:
        chain = "po" if po_bwd and k33 and k2 == 1 and Hd == 256 else "dgrad_act" if b3 else "epilogue"
        dgrad1 = ("dense" if k33 and smallmap_conv_ok(H, W, Hd, 0, Ch + Cc, N, bwd=True) else
                  "small" if dgrad_small_ok(N, Hd, Ch + Cc, H, W, k1) else "conv")
        packs += (("po_bwd",) if chain == "po" else ("w3_dgrad", "w2_dgrad")) + (
            "w1_dense_dgrad" if dgrad1 == "dense" else "w1_dgrad",)
    return CouplingRoute("po" if po else "convs", fp, conv1, conv3, bool(po and po_bwd and act != 0), chain, dgrad1,
                         bool(back and Hd % 64 == 0 and wgrad_b3(H, W)), packs)


# The parameters of one Glow step, in the order in which the three nodes' apply() takes them and their backward returns
# the gradients: the step's ActNorm, then what AffineCoupling.nn_params() (Flow/glow_modules.py) returns -- conv1 with
# its ActNorm, conv2 with its ActNorm, Conv2dZeros (weight, bias, logs), the realnvp clamp's scale and shift (or None).
StepParams = collections.namedtuple("StepParams", "an_bias an_logs w1 n1b n1l w2 n2b n2l w3 b3 l3 scale scale_shift")
STEP_NPARAM = len(StepParams._fields)


def _net_dims(p, cond):
    """(Hd, Cc, k1, k2, k3): hidden width, condition channels and kernel sizes of the coupling net of the step `p`"""
    return (int(p.w1.shape[0]), int(cond.shape[1]), *(int(w.shape[2]) for w in (p.w1, p.w2, p.w3)))


def _step_route(x, cond, p, act, grad, reverse=False):
    (N, C, H, W), (Hd, Cc, k1, k2, k3) = x.shape, _net_dims(p, cond)
    return coupling_route(N, C, Cc, Hd, H, W, k1, k2, k3, act, grad, reverse)


def _net_fwd(z, cond, p, act, route, pk):
    """coupling network of one Glow step `p` (glow_modules.py:232-238) on z's first channel half and `cond`, as `route`
    says.  Returns (h1, h2, o, P, masks): either o (finished Conv2dZeros output) or P (its tap-expanded pre-gather form,
    fused kernel) is None; masks: the fused kernel's activation masks (or None).  `pk`: see _pack."""
    N, C, H, W = z.shape
    (Hd, Cc, k1, k2, _), fp = _net_dims(p, cond), route.fwd_prec
    z1, cin2 = z[:, :C // 2], (cond if Cc > 0 else None)
    if route.fwd == "po":
        def stream():
            plan = POPackPlan([(p.w1.detach(), p.w2.detach(), p.w3.detach())])
            plan.run()
            return plan.bufs[0]
        # (the masks serve the backward stream only, which POPackPlan builds for at most 16 channels)
        h1, h2, P, masks = coupling_po_fwd(z, cin2, _pack(pk, "po_fwd", stream), _f(p.n1b), _f(p.n1l), _f(p.n2b),
                                           _f(p.n2l), C, act, want_masks=route.masks and pk.get("po_bwd") is not None)
        return h1, h2, None, P, masks
    if "w2_fwd" not in route.packs:
        pk = {}   # (fp32 forward convs: a step's forward conv packs are split-precision ones)
    if route.conv1 == "dense":
        h1 = smallmap_conv(z1, cin2, _pack(pk, "w1_dense_fwd", lambda: smallmap_pack(p.w1, H, W, False)), Hd, 1,
                           _f(p.n1b), _f(p.n1l), act)
    else:
        h1 = conv2d_raw(z1, cin2, _pack(pk, "w1_fwd", lambda: pack_weight(p.w1, prec=fp)), Hd, k1, 1, _f(p.n1b),
                        _f(p.n1l), act, prec=fp)
    h2 = conv2d_raw(h1, None, _pack(pk, "w2_fwd", lambda: pack_weight(p.w2, prec=fp)), Hd, k2, 1, _f(p.n2b),
                    _f(p.n2l), act, prec=fp)
    if route.conv3 == "dense":
        o = smallmap_conv(h2, None, _pack(pk, "w3_dense_fwd", lambda: smallmap_pack(p.w3, H, W, False)), C, 2, _f(p.b3),
                          _f(p.l3), 0)
    else:
        taps = route.conv3 == "taps"
        w3p = _pack(pk, "w3_fwd", lambda: pack_weight(_tap_expanded(p.w3) if taps else p.w3, prec=fp))
        o = zeros_conv_fwd(h2, p.w3, _f(p.b3), _f(p.l3), w3p, prec=fp, taps=taps)
    return h1, h2, o, None, None


NetGrads = collections.namedtuple("NetGrads", "w1 n1b n1l w2 n2b n2l w3")   # of a coupling net, flat as the kernels write
# the operands of a level's 3 K weight gradients, computed at the end K of one shape per launch: one list per operand,
# indexed by step (conv1: z1, c2, gh1; conv2: h1, gh2; conv3: h2, go)
WgradOperands = collections.namedtuple("WgradOperands", "z1 c2 gh1 h1 gh2 h2 go")


def _net_bwd(go, out, cond, h1, h2, p, act, route, pk, arena, gz, gcond, acc_cond, defer=None, masks=None, fin=None,
             step=None):
    """backward of the coupling network of the step `p` from `go` = gradient at conv3's output, as `route` says: returns
    the parameter gradients (NetGrads); the data gradient of conv1 is ADDED to gz[:, :C/2] and written (acc_cond: added)
    to gcond.  With `defer` (a WgradOperands) the weight gradients are NOT computed: their operands are stored at
    defer.*[step] and None is returned in their place (grouped launch by the caller).  The "po" chain reads `masks` (the
    fused forward kernel's) and no activation; it leaves the four ActNorm gradients to rfn_coupling_po_bwd_finish, which
    needs the weight gradients: a FinishTicket of `step` is appended to `fin` (the caller fills in gw1 / gw2 when they
    are deferred) or, without `fin`, finished here."""
    N, C, H, W = out.shape
    w1, n1b, n1l, w2, n2b, n2l, w3 = p.w1, p.n1b, p.n1l, p.w2, p.n2b, p.n2l, p.w3
    Ch, (Hd, Cc, k1, k2, k3) = C // 2, _net_dims(p, cond)
    dfr = defer is not None
    rows = wgrad_short_rows()
    gw3 = None if dfr else zeros_conv_wgrad(h2, go, C, k3, arena, rows)
    # the fused kernel needs the step's backward stream (POPackPlan: at most 16 channels) and, past an activation, the
    # forward's masks; what admits "po" ('mixed' arithmetic, Hd = 256) admits "dgrad_act" in its place
    chain = route.bwd_chain
    if chain == "po" and (pk.get("po_bwd") is None or (masks is None and act != 0)):
        chain = "dgrad_act"
    if chain != "po":
        with PackBatch() as b:
            w3f = _pack(pk, "w3_dgrad", lambda: b.conv(w3, True))
            w2f = _pack(pk, "w2_dgrad", lambda: b.conv(w2, True))
    if chain == "po":
        gh2, gh1, part = coupling_po_bwd(go.contiguous(), pk["po_bwd"], _f(n1l), _f(n2l), masks, act)
        gw2 = None if dfr else conv2d_wgrad(h1, None, gh2, Hd, k2, arena, rows)
        o4 = torch.empty((4, 256), device=go.device, dtype=torch.float32)
        gn1b, gn1l, gn2b, gn2l = o4[0], o4[1], o4[2], o4[3]
    elif chain == "dgrad_act":
        gh2, gn2b, gn2l = conv2d_dgrad_act(go, w3f, h2, _f(n2l), act, Hd, k3, arena)
        gw2 = None if dfr else conv2d_wgrad(h1, None, gh2, Hd, k2, arena, rows)
        gh1, gn1b, gn1l = conv2d_dgrad_act(gh2, w2f, h1, _f(n1l), act, Hd, k2, arena)
    else:
        gh2 = conv2d_raw(go, None, w3f, Hd, k3)
        # ---- actnorm2 + act bwd, conv2 (1x1) bwd
        gh2, gn2b, gn2l = conv_epilogue_bwd(h2, gh2, _f(n2l), 1, act, arena=arena)
        gw2 = conv2d_wgrad(h1, None, gh2, Hd, k2, arena, rows)
        gh1 = conv2d_raw(gh2, None, w2f, Hd, k2)
        # ---- actnorm1 + act bwd, conv1 bwd (grad flows to z1 (accumulated into gz's first half) and to cond)
        gh1, gn1b, gn1l = conv_epilogue_bwd(h1, gh1, _f(n1l), 1, act, arena=arena)
    z1, c2 = out[:, :Ch], (cond if Cc > 0 else None)
    gw1 = None if dfr else conv2d_wgrad(z1, c2, gh1, Hd, k1, arena, rows)
    if chain == "po":
        ticket = FinishTicket(part, w1, gw1, _f(n1b), w2, gw2, _f(n2b), o4, step)
        if fin is not None:
            fin.append(ticket)
        else:
            assert not dfr
            coupling_po_bwd_finish([ticket])
    if dfr:
        defer.z1[step], defer.c2[step], defer.gh1[step] = z1, c2, gh1
        defer.h1[step], defer.gh2[step] = h1, gh2
        defer.h2[step], defer.go[step] = h2, go
    g1, g2 = gz[:, :Ch], (gcond if Cc > 0 else None)
    if route.dgrad1 == "dense":
        smallmap_conv(gh1, None, _pack(pk, "w1_dense_dgrad", lambda: smallmap_pack(w1, H, W, True)), Ch + Cc, 0, out1=g1,
                      out2=g2, cout_split=Ch, acc1=True, acc2=acc_cond)
    elif route.dgrad1 == "small":
        conv3x3_smallcout(gh1, _pack(pk, "w1_dgrad", lambda: pack_weight(w1, True)), Ch + Cc, g1, g2, Ch, True, acc_cond)
    else:
        conv2d_raw(gh1, None, _pack(pk, "w1_dgrad", lambda: pack_weight(w1, True)), Ch + Cc, k1, 0, None, None, 0,
                   out1=g1, out2=g2, cout_split=Ch, acc1=True, acc2=acc_cond)
    return NetGrads(gw1, gn1b, gn1l, gw2, gn2b, gn2l, gw3)


def _net_arena_numel(C, p, cond):
    """floats of zero-filled arena that one step's backward takes: _net_bwd, a shell tail and an ActNorm / InvConv head"""
    Ch, (Hd, Cc, k1, k2, k3) = C // 2, _net_dims(p, cond)
    return (2 * Ch + 8 + 3 * 2 * (Hd + 4) + 2 * (C + 4) + k1 * k1 * Hd * (Ch + Cc) + k2 * k2 * Hd * Hd
            + max(k3 * k3 * C * Hd, 9 * C * Hd) + C * C + 2 * C + 64)


def _step_grads(p, net, tail, gab, gal):
    """the 13 gradients of the step `p` in StepParams order, shaped like the parameters, from its NetGrads, the TailGrads
    of its coupling tail and its ActNorm's gab / gal (scale / scale_shift: None unless the clamp is realnvp)"""
    def like(g, t):
        return None if g is None else g.view(t.shape)
    return StepParams(like(gab, p.an_bias), like(gal, p.an_logs), net.w1, net.n1b.view(1, -1, 1, 1), like(net.n1l, p.n1l),
                      net.w2, net.n2b.view(1, -1, 1, 1), like(net.n2l, p.n2l), net.w3, tail.gb3, like(tail.gl3, p.l3),
                      like(tail.gscale, p.scale), like(tail.gshift, p.scale_shift))


# ---- the shell launches of the Glow nodes, one wrapper per entry point
# what a backward coupling tail (coupling + Conv2dZeros epilogue) returns: gz = gradient at the step's post-InvConv
# tensor, go = gradient at conv3's output, and the flat gradients of scale, scale_shift (realnvp only), b3 and l3
TailGrads = collections.namedtuple("TailGrads", "gz go gscale gshift gb3 gl3")


def _tail_grads(gout, o, clamp_type, arena, go=None):
    """the outputs of a backward coupling tail, to be written (gz, go) or accumulated into (the rest, from `arena`)"""
    C = int(o.shape[1])
    gz, go = torch.empty_like(gout), (torch.empty_like(o) if go is None else go)
    gscale, gshift = (arena.take(C // 2), arena.take(C // 2)) if clamp_type == 0 else (None, None)
    return TailGrads(gz, go, gscale, gshift, arena.take(C), arena.take(C))


def _affine_zeros_bwd(out, o, gout, gdl, p, clamp_type, arena, go=None):
    """rfn_affine_zeros_bwd_f32, the stand-alone coupling tail of the step `p` backward: returns TailGrads"""
    N, C, H, W = out.shape
    t = _tail_grads(gout, o, clamp_type, arena, go)
    op, ons = L.frames(o, "o")
    outp, outns = L.frames(out, "out")
    gop, gons = L.frames(gout, "gout")
    gzp, gzns = L.frames(t.gz, "gz")
    gonp, gonns = L.frames(t.go, "go")
    scf, shf, l3f = _f(p.scale), _f(p.scale_shift), _f(p.l3)
    L.call("rfn_affine_zeros_bwd_f32", outp, outns, op, ons, gop, gons, L.dev(gdl), L.dev(scf),
           L.dev(shf), L.dev(l3f), gzp, gzns, gonp, gonns, L.dev(t.gscale), L.dev(t.gshift), L.dev(t.gb3),
           L.dev(t.gl3), clamp_type, N, C, H * W, meta=_shell("affine_zeros_bwd", gout, 4.5))
    return t


def _glow_shell_bwd(x, head, Wm, gz, gW, gab, gal, o, gdl, tail, clamp_type, arena, go=None):
    """rfn_glow_shell_bwd_f32: ActNorm / InvConv backward of the step `head` (input x, matrix Wm, gradient gz at its
    post-InvConv tensor; gW, gab, gal are accumulated into), whose result feeds the coupling tail of the step before it,
    `tail` (Conv2dZeros output o), from registers.  Returns that tail's TailGrads, as _affine_zeros_bwd."""
    N, C, H, W = x.shape
    t = _tail_grads(gz, o, clamp_type, arena, go)
    xp, xns = L.frames(x, "x")
    gzp, gzns = L.frames(gz, "gz")
    op, ons = L.frames(o, "o")
    gznp, gznns = L.frames(t.gz, "gz_prev")
    gonp, gonns = L.frames(t.go, "gpre")
    abf, alf, scf, shf, l3f = (_f(v) for v in (head.an_bias, head.an_logs, tail.scale, tail.scale_shift, tail.l3))
    L.call("rfn_glow_shell_bwd_f32", xp, xns, L.dev(abf), L.dev(alf), L.dev(Wm), gzp, gzns, L.dev(gW),
           L.dev(gab), L.dev(gal), op, ons, L.dev(gdl), L.dev(scf), L.dev(shf), L.dev(l3f), gznp, gznns, gonp,
           gonns, L.dev(t.gscale), L.dev(t.gshift), L.dev(t.gb3), L.dev(t.gl3), clamp_type, 1, N, C,
           H * W, meta=_shell("glow_shell_bwd", x, 5.5))
    return t


def _glow_shell_fwd(z, ld, clamp_type=0, tail=None, o=None, P=None, head=None, Wm=None):
    """rfn_glow_shell_fwd_f32: the coupling tail of the step `tail` on z, in place, from the finished Conv2dZeros output
    `o` or from its tap-expanded form `P` (fused kernel; gathered here into a fresh o), then the ActNorm / InvConv head
    of the step `head` (matrix Wm) into a new tensor.  Without `tail` only the head runs (first launch of a level),
    without `head` only the tail (last).  `ld`: the launch's slice of log-det partial sums, written.  Returns (o, znext)."""
    N, C, H, W = z.shape
    zp, zns = L.frames(z, "z")
    zn, znp, znns = None, None, 0
    hb = hl = sc = sh = b3 = l3 = None   # flat views of the parameters, held until the launch is enqueued
    if head is not None:
        zn, hb, hl = torch.empty_like(z), _f(head.an_bias), _f(head.an_logs)
        znp, znns = L.frames(zn, "znext")
    if tail is None:
        src, nt = (None, None, 0, None, None, None), 2
    else:
        sc, sh = _f(tail.scale), _f(tail.scale_shift)
        if P is not None:
            b3, l3, o = _f(tail.b3), _f(tail.l3), torch.empty((N, C, H, W), device=z.device, dtype=torch.float32)
            src, nt = (L.dev(P), None, 0, L.dev(b3), L.dev(l3), L.dev(o)), 12 + (0 if head is None else 1)
        else:
            op, ons = L.frames(o, "o")
            src, nt = (None, op, ons, None, None, None), 2 + (0 if head is None else 1.5)
    L.call("rfn_glow_shell_fwd_f32", zp, zns, *src, L.dev(sc), L.dev(sh), L.dev(ld), clamp_type, L.dev(hb),
           L.dev(hl), None if head is None else L.dev(Wm), znp, znns, 0 if head is None else 1, N, C,
           H, W, meta=_shell("glow_shell_fwd", z, nt))
    return o, zn


class GlowStepFn(torch.autograd.Function):
    """One forward Glow step (Flow/glow.py:31-36) as a single autograd node:
         y  = (x + an_bias) * exp(an_logs)                       glow_modules.py:38-45
         z  = Wm y                                               glow_modules.py:209-216
         h1 = act(actnorm(conv3x3(cat(z1, cond))))               glow_modules.py:232-238, 139-142
         h2 = act(actnorm(conv1x1(h1)))
         o  = (conv3x3(h2) + b3) * exp(3 logs3)                  glow_modules.py:119-121
         z2 <- (z2 + o[0::2]) * exp(clamp(o[1::2]))              glow_modules.py:276-285
       Returns (out, dlogdet[N]) where dlogdet holds only the data dependent Σ clamp(s) part; the parameter-only
       terms (Σlogs + Σlog_s)·H·W are added by the caller.
       apply(x, cond, Wm, *the step's parameters in StepParams order, act, clamp_type, packs).
       Saved for backward (_save_step): x, cond, out, h1, h2, o (activations stay resident in HBM, 288 GB is plenty).
       (The K steps of a level normally run as ONE node, GlowLevelFn; this one serves the first, data-initialising
       call and stand-alone coupling layers.)"""

    @staticmethod
    def forward(ctx, x, cond, Wm, an_bias, an_logs, w1, n1b, n1l, w2, n2b, n2l, w3, b3, l3, scale, scale_shift,
                act, clamp_type, packs=None):
        """`packs` (optional): the step's StepPacks (or a sequence in its field order)"""
        p = StepParams(an_bias, an_logs, w1, n1b, n1l, w2, n2b, n2l, w3, b3, l3, scale, scale_shift)
        out = actnorm_invconv_fwd(x, _f(an_bias), _f(an_logs), Wm.detach())
        ctx.packs = pk = StepPacks(*packs)._asdict() if packs is not None else {}
        ctx.route = route = _step_route(x, cond, p, act, any(ctx.needs_input_grad))
        h1, h2, o, P, masks = _net_fwd(out, cond, p, act, route, pk)
        o, dlogdet = gather_affine_(out, o, P, _f(b3), _f(l3), _f(scale), _f(scale_shift), clamp_type)
        _save_step(ctx, x, cond, Wm, p, out, h1, h2, o, masks)
        ctx.cfg = (act, clamp_type)
        return out, dlogdet

    @staticmethod
    def backward(ctx, gout, gdl):
        x, cond, Wm, p, out, h1, h2, o, masks = _saved_step(ctx.saved_tensors)
        act, clamp_type = ctx.cfg
        C = int(x.shape[1])
        gout = gout.contiguous()
        gdl = None if gdl is None else gdl.contiguous()
        # every accumulate-into output of this node lives in one zero-filled arena (1 fill launch instead of 14)
        arena = ZeroArena(_net_arena_numel(C, p, cond), x.device)
        # ---- affine coupling bwd + Conv2dZeros epilogue bwd in one launch: gz (whole tensor), go = grad at conv3's output
        tail = _affine_zeros_bwd(out, o, gout, gdl, p, clamp_type, arena)
        gcond = torch.empty_like(cond) if cond.shape[1] > 0 else torch.zeros_like(cond)
        net = _net_bwd(tail.go, out, cond, h1, h2, p, act, ctx.route, ctx.packs, arena, tail.gz, gcond, False, masks=masks)
        # ---- invconv + actnorm bwd
        gx, gW, gab, gal = actnorm_invconv_bwd(x, _f(p.an_bias), _f(p.an_logs), Wm.detach(), tail.gz, arena)
        return (gx, gcond, gW, *_step_grads(p, net, tail, gab, gal), None, None, None)


# ---- what the two training nodes save for backward, in which order, and how it comes back: (x, cond, W, the
# StepParams, out, h1, h2, o, masks), for the level node with lists over the K steps from the StepParams on
def _save_step(ctx, x, cond, Wm, p, out, h1, h2, o, masks):
    ctx.save_for_backward(x, cond, Wm, p.an_bias, p.an_logs, p.w1, p.n1l, p.w2, p.n2l, p.w3, p.l3, p.scale, p.scale_shift,
                          out, h1, h2, o, p.n1b, p.n2b, *(masks if masks is not None else ()))


def _saved_step(sv):
    (x, cond, Wm, an_bias, an_logs, w1, n1l, w2, n2l, w3, l3, scale, scale_shift, out, h1, h2, o, n1b, n2b, *masks) = sv
    p = StepParams(an_bias, an_logs, w1, n1b, n1l, w2, n2b, n2l, w3, None, l3, scale, scale_shift)   # (b3 is not read)
    return x, cond, Wm, p, out, h1, h2, o, tuple(masks) if masks else None


def _save_level(ctx, x, cond, Wst, flat, outs, h1s, h2s, os_, mks):
    """x, cond, Wst, the 13 K parameters, then K each of out / h1 / h2 / o and, if every step has them, of the two masks"""
    m1, m2 = zip(*mks) if all(m is not None for m in mks) else ((), ())
    ctx.save_for_backward(x, cond, Wst, *flat, *outs, *h1s, *h2s, *os_, *m1, *m2)


def _saved_level(sv):
    Kn, it = int(sv[2].shape[0]), iter(sv)
    (x, cond, Wst), *steps, outs, h1s, h2s, os_, m1, m2 = (
        list(itertools.islice(it, n)) for n in [3] + [STEP_NPARAM] * Kn + [Kn] * 6)
    return x, cond, Wst, [StepParams(*s) for s in steps], outs, h1s, h2s, os_, list(zip(m1, m2)) or [None] * Kn


class GlowLevelFn(torch.autograd.Function):
    """The K Glow steps of one flow level (Flow/glow.py:105-117, inner loop) as ONE autograd node.  Between two steps a
    single launch each way does the shell work (rfn_glow_shell_fwd_f32: coupling tail of step k + ActNorm/InvConv head
    of step k+1; rfn_glow_shell_bwd_f32: the mirror image); the gradient wrt the shared condition map accumulates
    inside the data-gradient kernels and the per-frame log-det inside the shell kernel, so autograd adds nothing.
    apply(x, cond, Wst[K,C,C], act, clamp_type, packs (None, or a list of K StepPacks or sequences in its field order),
    *the K steps' parameters, step by step, each in StepParams order)
    -> (out, dlogdet[N] = sum over the K steps of the data dependent log-det AND of the ActNorm parameter term
    H*W * sum_c logs[c]; the InvConv term sum log|s| * H*W stays with the caller, who builds the matrices)."""

    @staticmethod
    def forward(ctx, x, cond, Wst, act, clamp_type, packs, *flat):
        Kn = int(Wst.shape[0])
        assert len(flat) == STEP_NPARAM * Kn
        N, C, H, W = x.shape
        # the forward shell accepts more channels than the backward ones: refuse here what could not be differentiated
        if not L.load().rfn_glow_shell_supported(N, C, H, W):
            raise RuntimeError("GlowLevelFn: a flow level of C=%d channels on %dx%d maps does not fit the shell kernels "
                               "(C must be even and at most 144: rfn_glow_shell_supported)" % (C, H, W))
        prm = [StepParams(*flat[STEP_NPARAM * k:STEP_NPARAM * (k + 1)]) for k in range(Kn)]
        pks = [StepPacks(*packs[k])._asdict() if packs is not None and packs[k] is not None else {} for k in range(Kn)]
        route = _step_route(x, cond, prm[0], act, any(ctx.needs_input_grad))   # of all K steps
        Wd = Wst.detach().contiguous()
        # log-det: every shell launch WRITES its per-block partial sums into its own slice; one reduce launch adds them
        # per frame in a fixed order (no float atomics anywhere in the forward pass: bit-reproducible)
        ldf = int(L.load().rfn_glow_shell_fwd_ld_floats(N, C, H, W))
        ldp = torch.empty((Kn + 1, ldf), device=x.device, dtype=torch.float32)
        dl = torch.empty(N, device=x.device, dtype=torch.float32)
        _, z = _glow_shell_fwd(x, ldp[0], head=prm[0], Wm=Wd[0])
        kept = []   # per step: out, h1, h2, o, masks
        heads = [*zip(prm[1:], Wd[1:]), (None, None)]   # the step whose head follows the tail of step k, and its matrix
        for k in range(Kn):
            h1, h2, o, P, masks = _net_fwd(z, cond, prm[k], act, route, pks[k])
            o, zn = _glow_shell_fwd(z, ldp[k + 1], clamp_type, prm[k], o, P, *heads[k])
            kept.append((z, h1, h2, o, masks))
            z = zn
        L.call("rfn_logdet_reduce_f32", L.dev(ldp), Kn + 1, L.dev(dl), 0, N, C, H, W,
               meta=_shell("logdet_reduce", ldp, 1))
        _save_level(ctx, x, cond, Wst, flat, *zip(*kept))
        ctx.cfg = (act, clamp_type, pks, route)
        return kept[-1][0], dl

    @staticmethod
    def backward(ctx, gout, gdl):
        act, clamp_type, pks, route = ctx.cfg
        x, cond, Wst, prm, outs, h1s, h2s, os_, mks = _saved_level(ctx.saved_tensors)
        Kn, (N, C, H, W), (Hd, Cc, k1, k2, k3) = len(prm), x.shape, _net_dims(prm[0], cond)
        gout = gout.contiguous()
        gdl = None if gdl is None else gdl.contiguous()
        Wd = Wst.detach().contiguous()
        # one zero-filled arena for the accumulate-into outputs of all K steps
        arena = ZeroArena(Kn * _net_arena_numel(C, prm[0], cond), x.device)
        gWst = arena.take(Kn, C, C)
        gcond = torch.empty_like(cond) if Cc > 0 else torch.zeros_like(cond)
        # the 3 K weight gradients are computed at the end, K of one shape per launch (one atomic tail per launch
        # instead of K); their operands stay alive until then, which is what group_level_wgrad budgets
        # (the K conv3-output gradients then live in one buffer, go_all: one tap-scatter for all; else each in its own)
        grouped = group_level_wgrad(Kn, N, Hd, H * W, os_[0].numel(), x.device)
        go_all = torch.empty((Kn,) + tuple(os_[0].shape), device=x.device, dtype=torch.float32) if grouped else [None] * Kn
        defer = WgradOperands(*([None] * Kn for _ in WgradOperands._fields)) if grouped and route.defer_wgrad else None
        fin = []   # ActNorm-gradient tickets of the fused backward kernel, finished in one launch at the end
        grads = [None] * Kn   # per step, in StepParams order
        # `tail`: the coupling tail's gradients of the step the loop is about to visit.  They are produced one iteration
        # before they are consumed: for the last step by the stand-alone launch here, for step k - 1 by the shell launch
        # of iteration k, which runs the ActNorm / InvConv backward of step k and the tail of step k - 1 in one kernel.
        tail = _affine_zeros_bwd(outs[-1], os_[-1], gout, gdl, prm[-1], clamp_type, arena, go_all[-1])
        for k in range(Kn - 1, -1, -1):
            net = _net_bwd(tail.go, outs[k], cond, h1s[k], h2s[k], prm[k], act, route, pks[k], arena, tail.gz, gcond,
                           k != Kn - 1, defer, mks[k], fin, k)
            gab, gal = arena.take(C), arena.take(C)
            grads[k] = _step_grads(prm[k], net, tail, gab, gal)
            if k == 0:
                gx = actnorm_invconv_bwd(x, _f(prm[0].an_bias), _f(prm[0].an_logs), Wd[0], tail.gz, acc=(gWst[0], gab, gal),
                                         glogdet=gdl)[0]
            else:
                tail = _glow_shell_bwd(outs[k - 1], prm[k], Wd[k], tail.gz, gWst[k], gab, gal, os_[k - 1], gdl, prm[k - 1],
                                       clamp_type, arena, go_all[k - 1])
        if defer is not None:
            rows = wgrad_short_rows()
            gw1 = conv2d_wgrad_grouped(defer.z1, None if defer.c2[0] is None else defer.c2, defer.gh1, Hd, k1, arena,
                                       short_rows=rows)
            gw2 = conv2d_wgrad_grouped(defer.h1, None, defer.gh2, Hd, k2, arena, short_rows=rows)
            gw3 = zeros_conv_wgrad_grouped(defer.h2, defer.go, C, arena, g_stacked=go_all, ks=k3,
                                           min_pixels=level_mirrored_min_pixels(), short_rows=rows)
            grads = [g._replace(w1=a, w2=b, w3=c) for g, a, b, c in zip(grads, gw1, gw2, gw3)]
        if fin:
            coupling_po_bwd_finish([t._replace(gw1=grads[t.step].w1, gw2=grads[t.step].w2) for t in fin])
        return (gx, gcond, gWst, None, None, None, *(g for step in grads for g in step))


class GlowStepRevFn(torch.autograd.Function):
    """Reverse Glow step (Flow/glow.py:37-41) for generation; no gradient (the reference samples under no_grad).
    apply(x, cond, Winv, *the step's parameters in StepParams order, act, clamp_type, pkcache)."""

    @staticmethod
    def forward(ctx, x, cond, Winv, an_bias, an_logs, w1, n1b, n1l, w2, n2b, n2l, w3, b3, l3, scale, scale_shift,
                act, clamp_type, pkcache=None):
        """`pkcache` (optional dict, owned by the caller): packed weights of this step, filled on first use and reused
        while the caller keeps it -- autoregressive generation runs the same step once per frame on unchanged weights."""
        N, C, H, W = x.shape
        p = StepParams(an_bias, an_logs, w1, n1b, n1l, w2, n2b, n2l, w3, b3, l3, scale, scale_shift)
        z = x.detach().clone()
        route = _step_route(x, cond, p, act, False, reverse=True)
        # (one set of packs per forward arithmetic: CONV_PRECISION may change while the caller keeps the dict)
        pk = (pkcache if pkcache is not None else {}).setdefault(route.fwd_prec, {})
        _, _, o, P, _ = _net_fwd(z, cond, p, act, route, pk)
        if P is not None:
            o = torch.empty((N, C, H, W), device=x.device, dtype=torch.float32)
            b3f, l3f = _f(b3), _f(l3)
            L.call("rfn_tap_gather_f32", L.dev(P), L.dev(b3f), L.dev(l3f), L.dev(o), N, C, H, W)
        dlogdet = torch.zeros(N, device=x.device, dtype=torch.float32)
        affine_coupling_(z, o, _f(scale), _f(scale_shift), dlogdet, clamp_type, True)
        out = invconv_actnorm_rev(z, _f(an_bias), _f(an_logs), Winv.detach())
        ctx.mark_non_differentiable(out, dlogdet)
        return out, dlogdet


class GaussLogpFn(torch.autograd.Function):
    """Σ log N(z; mean, std) per frame (glow_modules.py:358-365 layout 0/softplus; glow.py:135-140 layout 1/exp)."""

    @staticmethod
    def forward(ctx, z, o, layout, std_mode):
        ctx.save_for_backward(z, o)
        ctx.cfg = (layout, std_mode)
        return gauss_logp(z, o, layout, std_mode)

    @staticmethod
    def backward(ctx, g):
        z, o = ctx.saved_tensors
        layout, std_mode = ctx.cfg
        N, Cz = z.shape[0], z.shape[1]
        gz = torch.empty(z.shape, device=z.device, dtype=torch.float32)
        go = torch.empty(o.shape, device=z.device, dtype=torch.float32)
        zp, zns = L.frames(z, "z")
        op, ons = L.frames(o, "o")
        gzp, gzns = L.frames(gz, "gz")
        gop, gons = L.frames(go, "go")
        L.call("rfn_gauss_logp_bwd_f32", zp, zns, op, ons, L.dev(g.contiguous()), gzp, gzns, gop, gons,
               layout, std_mode, N, Cz, _hw(z), meta=_shell("gauss_logp_bwd", z, 6))
        return gz, go, None, None


# ------------------------------------------------------------------------------------------------ small-map dense convs
def smallmap_arith_ok(H, W):
    """the dense small-map kernels compute forward AND backward in bf16x3: allowed when that is this map's forward
    arithmetic ('bf16x3' mode; 'mixed' mode on maps of at most 2x2)"""
    return CONV_PRECISION == "bf16x3" or (CONV_PRECISION == "mixed" and H * W <= 4)


def smallmap_supported(conv, H, W):
    """3x3 / stride 1 / pad 1 convolution on an H x W <= 16 map whose sample rows are 16-byte friendly"""
    return (smallmap_arith_ok(H, W) and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1)
            and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.bias is not None and H * W <= 16 and (conv.in_channels * H * W) % 8 == 0
            and (conv.out_channels * H * W) % 8 == 0)


def smallmap_pack(w, H, W, transpose):
    """PackBatch.dense of one weight: the buffer is filled when the call returns."""
    with PackBatch() as b:
        return b.dense(w, H, W, transpose)


def smallmap_dense(a, packed, n_channels, bias=None, slope_out=None, y=None, slope_in=0.0, want_a_out=False, add=None):
    """out[B, n_channels, H, W] = a'[B, C, H, W] (as rows) x packed (+ bias, leaky_relu) -- rfn_smallmap_dense_bf16x3.
    With y: a' = a * (y > 0 ? 1 : slope_in); returns (out, a') when want_a_out."""
    a = a.contiguous()
    B, H, W = int(a.shape[0]), int(a.shape[2]), int(a.shape[3])
    K, HW = int(a.shape[1]) * H * W, H * W
    out = torch.empty((B, n_channels, H, W), device=a.device, dtype=torch.float32)
    a_out = torch.empty_like(a) if want_a_out else None
    yc = None if y is None else y.contiguous()
    addc = None if add is None else add.contiguous()  # held until the launch is enqueued
    L.call("rfn_smallmap_dense_bf16x3", L.dev(a), L.dev(yc), slope_in, L.dev(packed), L.dev(bias),
           L.dev(addc), 0 if slope_out is None else 1, 0.0 if slope_out is None else slope_out, L.dev(out),
           L.dev(a_out), B, K, n_channels * HW, HW)
    return (out, a_out) if want_a_out else out


def smallmap_dense_pair(a0, packed0, n_ch0, a1, packed1, n_ch1, bias0=None, bias1=None, slope_out0=None, slope_out1=None,
                        y0=None, y1=None, slope_in0=0.0, slope_in1=0.0, want_a_out=False, add0=None, add1=None):
    """two independent smallmap_dense products in ONE launch (rfn_smallmap_dense_pair_bf16x3): same batch and map size.
    Returns (out0, out1) or (out0, a0', out1, a1') with want_a_out.  add0 / add1: optional [B, n_ch, H, W] addends."""
    a0, a1 = a0.contiguous(), a1.contiguous()
    B, H, W = int(a0.shape[0]), int(a0.shape[2]), int(a0.shape[3])
    assert int(a1.shape[0]) == B and tuple(a1.shape[2:]) == (H, W)
    HW = H * W
    K0, K1 = int(a0.shape[1]) * HW, int(a1.shape[1]) * HW
    out0 = torch.empty((B, n_ch0, H, W), device=a0.device, dtype=torch.float32)
    out1 = torch.empty((B, n_ch1, H, W), device=a0.device, dtype=torch.float32)
    ao0 = torch.empty_like(a0) if want_a_out and y0 is not None else None
    ao1 = torch.empty_like(a1) if want_a_out and y1 is not None else None
    y0c = None if y0 is None else y0.contiguous()  # held until the launch is enqueued
    y1c = None if y1 is None else y1.contiguous()
    ad0 = None if add0 is None else add0.contiguous()
    ad1 = None if add1 is None else add1.contiguous()
    L.call("rfn_smallmap_dense_pair_bf16x3",
           L.dev(a0), L.dev(y0c), slope_in0, L.dev(packed0), L.dev(bias0), L.dev(ad0), 0 if slope_out0 is None else 1,
           0.0 if slope_out0 is None else slope_out0, L.dev(out0), L.dev(ao0), K0, n_ch0 * HW,
           L.dev(a1), L.dev(y1c), slope_in1, L.dev(packed1), L.dev(bias1), L.dev(ad1), 0 if slope_out1 is None else 1,
           0.0 if slope_out1 is None else slope_out1, L.dev(out1), L.dev(ao1), K1, n_ch1 * HW, B, HW)
    if want_a_out:
        return out0, (ao0 if ao0 is not None else a0), out1, (ao1 if ao1 is not None else a1)
    return out0, out1


def smallmap_conv_ok(H, W, C1, C2, Cout, N, bwd=False):
    """3x3 conv on a map small enough for the dense kernels (rfn_smallmap_conv_bf16x3), and few enough frames: every
    32-frame row tile streams the whole dense matrix ((C1+C2)*HW x Cout*HW, on a 4x4 map more than half structural
    zeros), so the product is only used while that stream stays L2 / Infinity-Cache sized."""
    HW = H * W
    stream = -(-N // 32) * (C1 + C2) * HW * Cout * HW
    return ((bwd_b3() if bwd else smallmap_arith_ok(H, W)) and HW <= 16 and (C1 * HW) % 8 == 0 and ((C1 + C2) * HW) % 8 == 0
            and stream <= 32 * 1024 * 1024 and os.environ.get("RFN_SMALLMAP_GLOW") != "0")


def smallmap_conv(in1, in2, packed, Cout, ep_mode=0, p0=None, p1=None, act=0, out1=None, out2=None, cout_split=None,
                  acc1=False, acc2=False):
    """conv2d_raw's contract (3x3, pad 1) on an H*W <= 16 map through the dense split-precision product."""
    N, C1, H, W = in1.shape
    C2 = 0 if in2 is None else int(in2.shape[1])
    if cout_split is None:
        cout_split = Cout
    if out1 is None:
        out1 = torch.empty((N, cout_split, H, W), device=in1.device, dtype=torch.float32)
    i1p, i1ns = L.frames(in1, "in1")
    i2p, i2ns = (None, 0) if in2 is None else L.frames(in2, "in2")
    o1p, o1ns = L.frames(out1, "out1")
    o2p, o2ns = (None, 0) if out2 is None else L.frames(out2, "out2")
    L.call("rfn_smallmap_conv_bf16x3", i1p, i1ns, C1, i2p, i2ns, C2, L.dev(packed), o1p, o1ns, o2p, o2ns, Cout,
           cout_split, (1 if acc1 else 0) | (2 if acc2 else 0), N, H, W, ep_mode, L.dev(p0), L.dev(p1), act,
           meta=("conv", "smallmap_dense_kernel", 2.0 * N * H * W * (C1 + C2) * Cout * 9,
                 "N%d %d+%d->%d %dx%d k3 ep%d dense" % (N, C1, C2, Cout, H, W, ep_mode),
                 4.0 * (N * H * W * (C1 + C2 + Cout) + (C1 + C2) * Cout * H * W * H * W)))
    return out1


INVCONV_MAX_STEPS, INVCONV_MAX_CHANNELS = L.CONSTANTS["RFN_INVCONV_MAX_STEPS"], L.CONSTANTS["RFN_INVCONV_MAX_CHANNELS"]


def invconv_weights_ok(ics):
    """the K InvConv layers of a flow level the one-launch kernels take: LU parameterised, on the GPU, C <= 96"""
    return (0 < len(ics) <= INVCONV_MAX_STEPS and all(ic.LU_decomposed for ic in ics) and ics[0].lower.is_cuda
            and int(ics[0].lower.shape[0]) <= INVCONV_MAX_CHANNELS and os.environ.get("RFN_INVCONV_KERNEL") != "0")


class InvConvWeightsFn(torch.autograd.Function):
    """InvConv.get_weight (glow_modules.py:178-207) of the K steps of a flow level: (W [K, C, C], HW * sum log_s) in one
    launch, and one launch back to (lower, upper, log_s) gradients (rfn_invconv_weights_{fwd,bwd}_f32).
    apply(hw, K, p_1..p_K, sign_1..sign_K, lower_1..lower_K, upper_1..upper_K, log_s_1..log_s_K)."""

    @staticmethod
    def _pointers(P, S, Lw, U, LS):
        """host arrays of the K device pointers per parameter kind, in the entry points' argument order (the tensors are
        the modules' own parameters / buffers: dense, alive and at fixed addresses)"""
        out = []
        for grp, nm in ((P, "p"), (Lw, "lower"), (U, "upper"), (LS, "log_s"), (S, "sign_s")):
            for x in grp:
                L.dev(x, nm)  # fp32, device, contiguous -- raises otherwise
            out.append(L.ptr_array(list(grp), nm))
        return out

    @staticmethod
    def forward(ctx, hw, Kn, *t):
        ctx.set_materialize_grads(False)
        P, S, Lw, U, LS = (t[i * Kn:(i + 1) * Kn] for i in range(5))
        C = int(Lw[0].shape[0])
        arrs = InvConvWeightsFn._pointers(P, S, Lw, U, LS)
        W = torch.empty((Kn, C, C), device=Lw[0].device, dtype=torch.float32)
        c = torch.empty((), device=Lw[0].device, dtype=torch.float32)   # written by the kernel
        L.call("rfn_invconv_weights_fwd_f32", *arrs, L.dev(W), L.dev(c), Kn, C, int(hw),
               meta=_shell("invconv_weights_fwd", W, 4))
        ctx.cfg = (int(hw), Kn, C)
        ctx.save_for_backward(*t)
        return W, c

    @staticmethod
    def backward(ctx, gW, gc):
        hw, Kn, C = ctx.cfg
        t = ctx.saved_tensors
        P, S, Lw, U, LS = (t[i * Kn:(i + 1) * Kn] for i in range(5))
        dev_ = Lw[0].device
        if gW is None:
            gW = torch.zeros((Kn, C, C), device=dev_, dtype=torch.float32)
        arrs = InvConvWeightsFn._pointers(P, S, Lw, U, LS)
        gl = torch.empty((Kn, C, C), device=dev_, dtype=torch.float32)
        gu = torch.empty((Kn, C, C), device=dev_, dtype=torch.float32)
        gs = torch.empty((Kn, C), device=dev_, dtype=torch.float32)
        gcc = None if gc is None else gc.contiguous()
        L.call("rfn_invconv_weights_bwd_f32", *arrs, L.dev(gW.contiguous()), L.dev(gcc), L.dev(gl), L.dev(gu), L.dev(gs),
               Kn, C, hw, meta=_shell("invconv_weights_bwd", gW, 4))
        return (None, None) + (None,) * (2 * Kn) + tuple(gl.unbind(0)) + tuple(gu.unbind(0)) + tuple(gs.unbind(0))


class LatentStepFn(torch.autograd.Function):
    """one SRNN latent step (RFN_new.py:167-184,206-207): from the raw outputs of the encoder / prior parameter convs
    to (z_t, z^x_t, KL, enc_mean, enc_std) in one kernel each way (rfn_latent_step_{fwd,bwd}_f32)."""

    @staticmethod
    def forward(ctx, enc, pri, eps_p, eps_q, res_q):
        ctx.set_materialize_grads(False)  # unused outputs (enc_mean / enc_std without overshooting) arrive as None
        B = int(enc.shape[0])
        shp = (B, enc.shape[1] // 2) + tuple(enc.shape[2:])
        ZHW = 1
        for d in shp[1:]:
            ZHW *= int(d)
        enc, pri, eps_p, eps_q = enc.contiguous(), pri.contiguous(), eps_p.contiguous(), eps_q.contiguous()
        outs = [torch.empty(shp, device=enc.device, dtype=torch.float32) for _ in range(5)]
        L.call("rfn_latent_step_fwd_f32", L.dev(enc), L.dev(pri), L.dev(eps_p), L.dev(eps_q), *[L.dev(o) for o in outs],
               B, ZHW, 1 if res_q else 0, meta=_shell("latent_step_fwd", enc, 5.5))
        ctx.save_for_backward(enc, pri, eps_p, eps_q)
        ctx.cfg = (B, ZHW, bool(res_q))
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_zt, g_zxt, g_kl, g_em, g_es):
        enc, pri, eps_p, eps_q = ctx.saved_tensors
        B, ZHW, res_q = ctx.cfg
        # g_zt / g_zxt usually arrive as channel slices of the next step's input gradient: read in place (row stride)
        strided, keep = [], []
        for g in (g_zt, g_zxt):
            if g is None:
                strided += [None, 0]
                continue
            if B > 0 and (not g[0].is_contiguous() or (B > 1 and g.stride(0) < ZHW)):
                g = g.contiguous()
            keep.append(g)
            gp, gns = L.frames(g, "g_z")
            strided += [gp, gns]
        # keep the contiguous copies alive until the launch is enqueued (a freed temporary's block would be reused)
        gs = [None if g is None else g.contiguous() for g in (g_kl, g_em, g_es)]
        g_enc, g_pri = torch.empty_like(enc), torch.empty_like(pri)
        L.call("rfn_latent_step_bwd_f32", L.dev(enc), L.dev(pri), L.dev(eps_p), L.dev(eps_q), *strided,
               *[L.dev(g) for g in gs], L.dev(g_enc), L.dev(g_pri), B, ZHW, 1 if res_q else 0)
        return g_enc, g_pri, None, None, None


def latent_iw(enc_raw, pri_raw, eps_q, res_q):
    """one latent step of the chains of RFN.iw_log_weights in one launch (rfn_latent_iw_f32; include/rfn_hip.h and DESIGN
    section 24 hold the definition): from the raw outputs [rows, 2*Z, H, W] of the encoder / prior parameter convs and
    eps_q [rows, Z, H, W] to (zxt [rows, Z, H, W], logr [rows]), zxt = em + es*eps_q with LatentStepFn's bits and logr the
    row sum of log N(zxt; pm, ps) - log N(zxt; em, es).  Forward only: an input that requires grad is an error.  No CPU
    fallback."""
    for t, nm in ((enc_raw, "enc_raw"), (pri_raw, "pri_raw"), (eps_q, "eps_q")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("latent_iw: %s must be a tensor, got %s" % (nm, type(t).__name__))
        if t.requires_grad:
            raise RuntimeError("latent_iw has no backward: %s requires grad (compute it under torch.no_grad())" % nm)
    if enc_raw.dim() < 2 or enc_raw.shape != pri_raw.shape or int(enc_raw.shape[1]) % 2:
        raise ValueError("latent_iw: enc_raw and pri_raw must both be [rows, 2*Z, ...], got %s and %s" %
                         (tuple(enc_raw.shape), tuple(pri_raw.shape)))
    shp = (int(enc_raw.shape[0]), int(enc_raw.shape[1]) // 2) + tuple(int(d) for d in enc_raw.shape[2:])
    if tuple(eps_q.shape) != shp:
        raise ValueError("latent_iw: eps_q must be %s, got %s" % (shp, tuple(eps_q.shape)))
    rows, ZHW = shp[0], 1
    for d in shp[1:]:
        ZHW *= d
    if rows < 1 or ZHW < 1:
        raise ValueError("latent_iw: need rows >= 1 and Z*H*W >= 1, got %s" % (shp,))
    enc_raw, pri_raw, eps_q = enc_raw.contiguous(), pri_raw.contiguous(), eps_q.contiguous()
    ptrs = [L.dev(enc_raw, "enc_raw"), L.dev(pri_raw, "pri_raw"), L.dev(eps_q, "eps_q")]
    zxt = torch.empty(shp, device=enc_raw.device, dtype=torch.float32)
    logr = torch.empty((rows,), device=enc_raw.device, dtype=torch.float32)
    with torch.cuda.device(enc_raw.device):
        L.call("rfn_latent_iw_f32", *ptrs, L.dev(zxt), L.dev(logr), rows, ZHW, 1 if res_q else 0,
               meta=_shell("latent_iw", enc_raw, 3.0))
    return zxt, logr


class ConvLSTMCellFn(torch.autograd.Function):
    """ConvLSTMLayer.forward (Utils/modules.py:355-377): conv3x3(cat(x,h))+b on the MFMA conv kernel, then the fused
    gate update.  Peephole tensors may be None (== 0)."""

    @staticmethod
    def forward(ctx, x, h, c, w, b, wci, wcf, wco):
        N, Cx, H, W = x.shape
        Hc = int(w.shape[0]) // 4
        ks = int(w.shape[2])
        HW = H * W
        fp = fwd_prec(H, W)
        cc = conv2d_raw(x, h, pack_weight(w, prec=fp), 4 * Hc, ks, 3 if b is not None else 0,
                        None if b is None else b.detach().contiguous(), None, 0, prec=fp)
        h_out = torch.empty((N, Hc, H, W), device=x.device, dtype=torch.float32)
        c_out = torch.empty((N, Hc, H, W), device=x.device, dtype=torch.float32)
        gates = torch.empty((N, 4 * Hc, H, W), device=x.device, dtype=torch.float32)
        cp, cns = L.frames(c, "c")
        hp, hns = L.frames(h_out, "h_out")
        cop, cons = L.frames(c_out, "c_out")
        pe = [None if t is None else t.detach().reshape(-1).contiguous() for t in (wci, wcf, wco)]
        L.call("rfn_convlstm_gates_fwd_f32", L.dev(cc), cp, cns, L.dev(pe[0]), L.dev(pe[1]), L.dev(pe[2]), hp,
               hns, cop, cons, L.dev(gates), N, Hc, HW, meta=_shell("convlstm_gates_fwd", gates, 2.75))
        ctx.save_for_backward(x, h, c, w, gates, c_out, *[t for t in pe if t is not None])
        ctx.has_bias = b is not None
        ctx.has_pe = pe[0] is not None
        return h_out, c_out

    @staticmethod
    def backward(ctx, gh, gc):
        saved = ctx.saved_tensors
        x, h, c, w, gates, c_out = saved[:6]
        pe = list(saved[6:9]) if ctx.has_pe else [None, None, None]
        N, Cx, H, W = x.shape
        Hc = int(w.shape[0]) // 4
        ks = int(w.shape[2])
        HW = H * W
        gcc = torch.empty_like(gates)
        gc_prev = torch.empty_like(c)
        cp, cns = L.frames(c, "c")
        cop, cons = L.frames(c_out, "c_out")
        ghp, ghns = (None, 0) if gh is None else L.frames(gh.contiguous(), "gh")
        gcp, gcns = (None, 0) if gc is None else L.frames(gc.contiguous(), "gc")
        gpp, gpns = L.frames(gc_prev, "gc_prev")
        L.call("rfn_convlstm_gates_bwd_f32", L.dev(gates), cp, cns, cop, cons, ghp, ghns, gcp, gcns,
               L.dev(pe[0]), L.dev(pe[1]), L.dev(pe[2]), L.dev(gcc), gpp, gpns, N, Hc, HW,
               meta=_shell("convlstm_gates_bwd", gates, 3.25))
        gb = conv_epilogue_bwd(None, gcc, None, 3, 0, want_gl=False)[1] if ctx.has_bias else None
        gw = conv2d_wgrad(x, h, gcc, 4 * Hc, ks, short_rows=wgrad_short_rows())
        gx = torch.empty_like(x)
        ghp_ = torch.empty_like(h)
        conv2d_raw(gcc, None, pack_weight(w, True), Cx + Hc, ks, 0, None, None, 0, out1=gx, out2=ghp_, cout_split=Cx)
        return gx, ghp_, gc_prev, gw, gb, None, None, None


def convlstm_seq_supported(w, Cx, H, W):
    """time-batched ConvLSTM path: 3x3 kernel on a small map, both weight halves dense-packable"""
    Hc = int(w.shape[0]) // 4
    return (smallmap_arith_ok(H, W) and tuple(w.shape[2:]) == (3, 3) and H * W <= 16 and (Cx * H * W) % 8 == 0
            and (Hc * H * W) % 8 == 0 and int(w.shape[1]) == Cx + Hc)


class ConvLSTMSeqFn(torch.autograd.Function):
    """A whole ConvLSTM sequence (Utils/modules.py:396-414 looping :355-377) on a small map as ONE autograd node.
    conv(cat(x_t, h_{t-1})) = Wx*x_t + Wh*h_{t-1}: the input projection of all S steps is one time-batched dense
    product, only Wh*h_{t-1} (Hc of the Cx+Hc input channels) stays in the recurrence; the backward pass keeps only
    Wh^T*gcc_t in its loop and computes the input gradient, the weight gradient and the bias gradient once over the S
    steps.  x_all [S,B,Cx,H,W] -> h_all [S,B,Hc,H,W], c_S."""

    @staticmethod
    def forward(ctx, x_all, h0, c0, w, b):
        S, B, Cx, H, W = (int(v) for v in x_all.shape)
        Hc, HW = int(w.shape[0]) // 4, H * W
        x_all, h0, c0 = x_all.contiguous(), h0.contiguous(), c0.contiguous()
        wd = w.detach()
        wx, wh = wd[:, :Cx].contiguous(), wd[:, Cx:].contiguous()
        with PackBatch() as pb:
            pk_xf, pk_hf = pb.dense(wx, H, W, False), pb.dense(wh, H, W, False)
        pre = smallmap_dense(x_all.view(S * B, Cx, H, W), pk_xf, 4 * Hc, bias=None if b is None else b.detach())
        pre = pre.view(S, B, 4 * Hc, H, W)
        h_all = torch.empty((S, B, Hc, H, W), device=x_all.device, dtype=torch.float32)
        c_all = torch.empty((S, B, Hc, H, W), device=x_all.device, dtype=torch.float32)
        gates = torch.empty((S, B, 4 * Hc, H, W), device=x_all.device, dtype=torch.float32)
        h_prev, c_prev = h0, c0
        ns = Hc * HW
        for t in range(S):
            cc = smallmap_dense(h_prev, pk_hf, 4 * Hc, add=pre[t])
            L.call("rfn_convlstm_gates_fwd_f32", L.dev(cc), L.dev(c_prev), ns, None, None, None, L.dev(h_all[t]), ns,
                   L.dev(c_all[t]), ns, L.dev(gates[t]), B, Hc, HW, meta=_shell("convlstm_gates_fwd", gates[t], 2.75))
            h_prev, c_prev = h_all[t], c_all[t]
        ctx.save_for_backward(x_all, h0, c0, w, h_all, c_all, gates)
        ctx.has_bias = b is not None
        return h_all, c_all[S - 1]

    @staticmethod
    def backward(ctx, g_hall, g_cS):
        x_all, h0, c0, w, h_all, c_all, gates = ctx.saved_tensors
        S, B, Cx, H, W = (int(v) for v in x_all.shape)
        Hc, HW = int(w.shape[0]) // 4, H * W
        ns = Hc * HW
        wd = w.detach()
        wx, wh = wd[:, :Cx].contiguous(), wd[:, Cx:].contiguous()
        with PackBatch() as pb:
            pk_xb, pk_hb = pb.dense(wx, H, W, True), pb.dense(wh, H, W, True)
        g_hall = None if g_hall is None else g_hall.contiguous()
        gcc = torch.empty_like(gates)
        gh_rec, gc = None, (None if g_cS is None else g_cS.contiguous())
        for t in range(S - 1, -1, -1):
            if g_hall is None:
                gh = gh_rec
            elif gh_rec is None:
                gh = g_hall[t]
            else:
                gh = g_hall[t] + gh_rec
            c_prev = c_all[t - 1] if t > 0 else c0
            gc_prev = torch.empty_like(c0)
            L.call("rfn_convlstm_gates_bwd_f32", L.dev(gates[t]), L.dev(c_prev), ns, L.dev(c_all[t]), ns, L.dev(gh),
                   ns if gh is not None else 0, L.dev(gc), ns if gc is not None else 0, None, None, None, L.dev(gcc[t]),
                   L.dev(gc_prev), ns, B, Hc, HW, meta=_shell("convlstm_gates_bwd", gates[t], 3.25))
            gh_rec = smallmap_dense(gcc[t], pk_hb, Hc)
            gc = gc_prev
        G = gcc.view(S * B, 4 * Hc, H, W)
        gx_all = smallmap_dense(G, pk_xb, Cx).view(S, B, Cx, H, W) if ctx.needs_input_grad[0] else None
        h_prev_all = torch.cat([h0.unsqueeze(0), h_all[:S - 1]], 0).view(S * B, Hc, H, W)
        gw = conv2d_wgrad(x_all.view(S * B, Cx, H, W), h_prev_all, G, 4 * Hc, 3, short_rows=wgrad_short_rows())
        gb = G.sum(dim=(0, 2, 3)) if ctx.has_bias else None
        return gx_all, gh_rec, gc, gw, gb


# ----------------------------------------------------------------------------------------------- the other families
# Each lives in the module named after the csrc file it wraps and is re-exported here: rfn_hip.ops is the import surface
# (callers and tests reach, and patch, these names as attributes of it), the module is the home.  None of them reads
# the precision switches or calls into the core, and none imports this module.
from .gauss_heads import GAUSS_HEADS_OUTPUTS, GaussHeadsFn, gauss_heads, gauss_heads_check  # noqa: E402,F401
from .lstm_cell import (LSTM_CELL_KERNEL_DEFAULT, LSTMCellFn, lstm_cell, lstm_cell_check, lstm_cell_route,  # noqa: E402,F401
                        lstm_cell_torch)
from .stepbn import StepBatchNormActFn, StepBatchNormActPoolFn, Up2xCatFn  # noqa: E402,F401
from .bnflow import BatchNormFlowFn, bnflow_apply, bnflow_coef  # noqa: E402,F401
from .mol import (MOL_KEYED_SLOT_COLOUR, MOL_KEYED_SLOT_MIX, MolNllFn, mol_dims, mol_keyed_uniforms, mol_nll,  # noqa: E402,F401
                  mol_sample, mol_sample_keyed)
from .pixel_loglik import (PIXEL_LOGLIK_KERNEL_DEFAULT, PIXEL_LOGLIK_MODES, normal_logvar_pair,  # noqa: E402,F401
                           normal_logvar_pair_check, pixel_loglik, pixel_loglik_check, pixel_loglik_route)
from .frame_metrics import frame_quality  # noqa: E402,F401
from .linext import (LinearExtrapLossFn, gauss_quality, gauss_quality_check, linear_extrap_check,  # noqa: E402,F401
                     linear_extrap_loss, linear_extrap_pairs, linear_extrap_rollout, linext_limits)
from .frames import (CLIP_MIRROR, CLIP_REVERSE, RESIZE_MAX_SIDE, clip_gather, clip_gather_aug, frames_resize,  # noqa: E402,F401
                     moving_mnist_render, moving_mnist_sync_render, resize_window)
from .noise import (KEYED_NORMAL_MAX_SLOTS, KEYED_UNIFORM_SLOT_DEQUANT, keyed_normal, keyed_normal_tiled_row,  # noqa: E402,F401
                    keyed_uniform)
from .pictures import SHEET_MAX_ROWS, chart_chunk, chart_font, compose_sheet, render_chart, sheet_shape  # noqa: E402,F401
from .clip_compose import CLIP_MODES, ClipCell, clip_limits, clip_shape, compose_clip  # noqa: E402,F401

# LPIPS with the AlexNet trunk (rfn_hip/lpips.py holds the loader and the wrappers of csrc/lpips.hip)
from .lpips import (LpipsAlexWeights, LpipsFeatures, lpips_alex, lpips_alex_distance, lpips_alex_features,  # noqa: E402,F401
                    lpips_alex_load, lpips_alex_pack, lpips_alex_sizes)

# Frechet Video Distance: the I3D trunk and the Frechet distance (rfn_hip/i3d.py holds the layer table, the loader and the
# wrappers of csrc/i3d.hip)
from .i3d import (I3DWeights, frechet_distance, i3d_embed, i3d_head, i3d_inception, i3d_load, i3d_logits,  # noqa: E402,F401
                  i3d_maxpool, i3d_pack, i3d_preprocess, i3d_same, i3d_sizes, i3d_unit)
