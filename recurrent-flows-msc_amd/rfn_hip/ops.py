"""Tensor-level wrappers and autograd Functions over the C ABI (include/rfn_hip.h).

Everything here runs on the GPU through librfn_hip.so; torch is used for memory, streams and autograd plumbing.
Frame-batched layout: tensors are [N, C, H, W] fp32 where N = all frames handed over by the caller (the RFN driver
time-batches B*(T-1) frames into one call).
"""
import collections
import ctypes
import functools
import itertools

import torch

from . import lib as L

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


def _shell(name, t, n_tensors):
    """profiling metadata of a memory-bound shell launch: algorithmic bytes = n_tensors x the tensor's fp32 size"""
    return ("shell", name, 0.0, "x".join(str(int(d)) for d in t.shape), 4.0 * n_tensors * t.numel())


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


def _f(t):
    return None if t is None else t.detach().reshape(-1).contiguous()


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


GAUSS_HEADS_OUTPUTS = ("z_q", "z_p", "q_scale", "p_scale", "kl", "logq", "logp")
# what each output reads beside p_loc / p_raw, which every call needs
_GAUSS_HEADS_NEEDS = {"z_q": ("q_loc", "q_raw", "eps_q"), "z_p": ("eps_p",), "q_scale": ("q_loc", "q_raw"), "p_scale": (),
                      "kl": ("q_loc", "q_raw"), "logq": ("q_loc", "q_raw", "eps_q"), "logp": ("eps_p",)}


def gauss_heads_check(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want):
    """(B, Z) of a gauss_heads call, or a ValueError naming what does not fit.  Needs no device."""
    given = {"q_loc": q_loc, "q_raw": q_raw, "p_loc": p_loc, "p_raw": p_raw, "eps_q": eps_q, "eps_p": eps_p}
    want = tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in GAUSS_HEADS_OUTPUTS for w in want):
        raise ValueError("gauss_heads: want must name distinct outputs of %s, got %r" % (GAUSS_HEADS_OUTPUTS, want))
    if p_loc is None or p_raw is None:
        raise ValueError("gauss_heads: p_loc and p_raw are always needed")
    if (q_loc is None) != (q_raw is None):
        raise ValueError("gauss_heads: q_loc and q_raw come together (both None: the prior-only form)")
    if q_loc is None and eps_q is not None:
        raise ValueError("gauss_heads: eps_q without q_loc / q_raw")
    for w in want:
        missing = [n for n in _GAUSS_HEADS_NEEDS[w] if given[n] is None]
        if missing:
            raise ValueError("gauss_heads: output %r needs %s" % (w, ", ".join(missing)))
    if p_loc.dim() != 2 or p_loc.shape[0] < 1 or p_loc.shape[1] < 1:
        raise ValueError("gauss_heads: inputs are [B, Z] with B, Z >= 1, got p_loc %s" % (tuple(p_loc.shape),))
    for n, t in given.items():
        if t is not None and tuple(t.shape) != tuple(p_loc.shape):
            raise ValueError("gauss_heads: %s has shape %s, p_loc %s" % (n, tuple(t.shape), tuple(p_loc.shape)))
    return int(p_loc.shape[0]), int(p_loc.shape[1])


class GaussHeadsFn(torch.autograd.Function):
    """the diagonal Gaussians of one VRNN step in one kernel each way (rfn_gauss_heads_{fwd,bwd}_f32, include/rfn_hip.h):
    returns the seven GAUSS_HEADS_OUTPUTS in that order, None where `want` does not name one.  Saves the six inputs
    only; the backward recomputes sigma."""

    @staticmethod
    def forward(ctx, q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want):
        ctx.set_materialize_grads(False)  # unused outputs arrive as None
        B, Z = gauss_heads_check(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want)
        ins = [None if t is None else t.contiguous() for t in (q_loc, q_raw, p_loc, p_raw, eps_q, eps_p)]
        ptrs = [L.dev(t, n) for t, n in zip(ins, ("q_loc", "q_raw", "p_loc", "p_raw", "eps_q", "eps_p"))]
        outs = []
        for name in GAUSS_HEADS_OUTPUTS:
            shape = (B,) if name in ("kl", "logq", "logp") else (B, Z)
            outs.append(torch.empty(shape, device=p_loc.device, dtype=torch.float32) if name in want else None)
        L.call("rfn_gauss_heads_fwd_f32", *ptrs, *[L.dev(o) for o in outs], B, Z,
               meta=_shell("gauss_heads_fwd", p_loc, sum(t is not None for t in ins + outs)))
        ctx.save_for_backward(*ins)
        ctx.cfg = (B, Z)
        # the ABI has no upstream gradient for the scales: they are values (the KL and the densities are outputs of their own)
        ctx.mark_non_differentiable(*[o for o in outs[2:4] if o is not None])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_zq, g_zp, g_qs, g_ps, g_kl, g_logq, g_logp):
        ins = ctx.saved_tensors
        q_loc, p_loc = ins[0], ins[2]
        B, Z = ctx.cfg
        # g_zq / g_zp may arrive as column slices of a wider gradient: read in place (row stride)
        strided, keep = [], []
        for g in (g_zq, g_zp):
            if g is None:
                strided += [None, 0]
                continue
            if (Z > 1 and g.stride(1) != 1) or (B > 1 and g.stride(0) < Z):
                g = g.contiguous()
            keep.append(g)
            strided += [L.dev(g, "g_z", check_contiguous=False), int(g.stride(0)) if B > 1 else Z]
        gs = [None if g is None else g.contiguous() for g in (g_kl, g_logq, g_logp)]
        g_q = [None, None] if q_loc is None else [torch.empty_like(q_loc), torch.empty_like(q_loc)]
        g_p = [torch.empty_like(p_loc), torch.empty_like(p_loc)]
        L.call("rfn_gauss_heads_bwd_f32", *[L.dev(t) for t in ins], *strided, *[L.dev(g) for g in gs],
               *[L.dev(g) for g in g_q + g_p], B, Z, meta=_shell("gauss_heads_bwd", p_loc, 10))
        return g_q[0], g_q[1], g_p[0], g_p[1], None, None, None


def gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=None, eps_p=None, want=("z_q", "kl")):
    """The outputs named in `want`, in that order, of the [B, Z] Gaussians N(q_loc, softplus(q_raw)) and N(p_loc,
    softplus(p_raw)): "z_q" / "z_p" = loc + sigma * eps, "q_scale" / "p_scale" = sigma (no gradient is taken through
    them), "kl" [B] = KL(q || p) summed over the row, "logq" / "logp" [B] = the row-summed log-density of each
    distribution at its own sample.  q_loc = q_raw = eps_q = None is the prior-only form.  One launch each way on the
    current stream; no CPU fallback."""
    gauss_heads_check(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, want)
    outs = GaussHeadsFn.apply(q_loc, q_raw, p_loc, p_raw, eps_q, eps_p, tuple(want))
    return tuple(outs[GAUSS_HEADS_OUTPUTS.index(w)] for w in want)


def lstm_cell_check(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """(B, I, H) of an lstm_cell call, or a ValueError naming what does not fit.  Needs no device."""
    given = {"x": x, "h": h, "c": c, "w_ih": w_ih, "w_hh": w_hh, "b_ih": b_ih, "b_hh": b_hh}
    for n, t in given.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError("lstm_cell: %s must be a tensor, got %s" % (n, type(t).__name__))
        if t.dtype != x.dtype or t.dtype not in (torch.float32, torch.float64):
            raise ValueError("lstm_cell: tensors are float32 (float64 on the torch route) and of one dtype; %s is %s, x %s"
                             % (n, t.dtype, x.dtype))
        if t.device != x.device:
            raise ValueError("lstm_cell: %s is on %s, x on %s" % (n, t.device, x.device))
        if not t.is_contiguous():
            raise ValueError("lstm_cell: %s must be contiguous, got shape %s stride %s"
                             % (n, tuple(t.shape), tuple(t.stride())))
    if x.dim() != 2 or h.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1 or h.shape[1] < 1:
        raise ValueError("lstm_cell: x is [B, I] and h [B, H] with B, I, H >= 1, got x %s, h %s"
                         % (tuple(x.shape), tuple(h.shape)))
    B, I, H = int(x.shape[0]), int(x.shape[1]), int(h.shape[1])
    for n, shape in (("h", (B, H)), ("c", (B, H)), ("w_ih", (4 * H, I)), ("w_hh", (4 * H, H)), ("b_ih", (4 * H,)),
                     ("b_hh", (4 * H,))):
        if tuple(given[n].shape) != shape:
            raise ValueError("lstm_cell: %s has shape %s, B = %d, I = %d, H = %d need %s"
                             % (n, tuple(given[n].shape), B, I, H, shape))
    return B, I, H


# Route of lstm_cell for device tensors when RFN_LSTM_CELL is unset (DESIGN.md section 22 has the measurement it follows):
# True = the kernels, False = the torch ops.
LSTM_CELL_KERNEL_DEFAULT = True


def lstm_cell_route(x):
    """"kernel" or "torch" for an lstm_cell call on x: CPU tensors and float64 always take the torch ops; for float32
    device tensors RFN_LSTM_CELL=0 / 1 chooses (read at every call, as RFN_UP2X_CAT is), else LSTM_CELL_KERNEL_DEFAULT"""
    if not x.is_cuda or x.dtype != torch.float32:
        return "torch"
    env = os.environ.get("RFN_LSTM_CELL")
    if env in ("0", "1"):
        return "kernel" if env == "1" else "torch"
    return "kernel" if LSTM_CELL_KERNEL_DEFAULT else "torch"


def lstm_cell_torch(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """the formulas of lstm_cell as torch ops (the RFN_LSTM_CELL=0 route, and the only one for CPU tensors)"""
    H = h.shape[1]
    pre = torch.addmm(b_ih + b_hh, x, w_ih.t()) + torch.mm(h, w_hh.t())
    i, f, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
    g = torch.tanh(pre[:, 2 * H:3 * H])
    c_new = f * c + i * g
    return o * torch.tanh(c_new), c_new


class LSTMCellFn(torch.autograd.Function):
    """one torch.nn.LSTMCell call in one kernel each way (rfn_lstm_cell_{fwd,bwd}_f32, include/rfn_hip.h): returns
    (h', c').  Saves x, h, c, the weights, c' and the gate activations [B, 4H]; the backward kernel gives D, g_c and the
    bias gradient, the four matrix products of the backward are torch.mm calls."""

    @staticmethod
    def forward(ctx, x, h, c, w_ih, w_hh, b_ih, b_hh):
        ctx.set_materialize_grads(False)  # a missing upstream arrives as None and travels as a NULL pointer
        B, I, H = lstm_cell_check(x, h, c, w_ih, w_hh, b_ih, b_hh)
        h_out, c_out = torch.empty_like(h), torch.empty_like(c)
        gates = torch.empty((B, 4 * H), device=x.device, dtype=torch.float32)
        L.call("rfn_lstm_cell_fwd_f32", L.dev(x, "x"), L.dev(h, "h"), L.dev(c, "c"), L.dev(w_ih, "w_ih"),
               L.dev(w_hh, "w_hh"), L.dev(b_ih, "b_ih"), L.dev(b_hh, "b_hh"), L.dev(h_out), L.dev(c_out), L.dev(gates),
               B, I, H, meta=_shell("lstm_cell_fwd", gates, 4))
        ctx.save_for_backward(x, h, c, w_ih, w_hh, c_out, gates)
        ctx.cfg = (B, I, H)
        return h_out, c_out

    @staticmethod
    def backward(ctx, gh, gc):
        x, h, c, w_ih, w_hh, c_out, gates = ctx.saved_tensors
        if gh is None and gc is None:
            return (None,) * 7
        B, I, H = ctx.cfg
        gh = None if gh is None else gh.contiguous()
        gc = None if gc is None else gc.contiguous()
        D, g_c, g_bias = torch.empty_like(gates), torch.empty_like(c), torch.empty(4 * H, device=x.device, dtype=torch.float32)
        L.call("rfn_lstm_cell_bwd_f32", L.dev(gh, "gh"), L.dev(gc, "gc"), L.dev(gates), L.dev(c), L.dev(c_out), L.dev(D),
               L.dev(g_c), L.dev(g_bias), B, H, meta=_shell("lstm_cell_bwd", gates, 3))
        need = ctx.needs_input_grad
        return (torch.mm(D, w_ih) if need[0] else None, torch.mm(D, w_hh) if need[1] else None,
                g_c if need[2] else None, torch.mm(D.t(), x) if need[3] else None,
                torch.mm(D.t(), h) if need[4] else None, g_bias if need[5] else None, g_bias if need[6] else None)


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh, route=None):
    """(h', c') of torch.nn.LSTMCell with these parameters on x [B, I] and the state (h, c) [B, H]; gate order i, f, g, o.
    route: None (lstm_cell_route decides), "kernel" (one launch each way on the current stream, float32 device tensors
    only: anything else raises, there is no fallback) or "torch"."""
    lstm_cell_check(x, h, c, w_ih, w_hh, b_ih, b_hh)
    route = lstm_cell_route(x) if route is None else route
    if route == "kernel":
        return LSTMCellFn.apply(x, h, c, w_ih, w_hh, b_ih, b_hh)
    if route != "torch":
        raise ValueError("lstm_cell: route is None, 'kernel' or 'torch', got %r" % (route,))
    return lstm_cell_torch(x, h, c, w_ih, w_hh, b_ih, b_hh)


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


def _stepbn_fwd_buffers(x, gamma, beta, S, pooled=False):
    """What a per-step BatchNorm forward (plain, synchronised or pooled) allocates for x [S*B, C, H, W]: (B, mean [S, C],
    var [S, C], the output, the detached gamma and beta, the floats of scratch either direction needs, the scratch)."""
    SB, C, H, W = (int(v) for v in x.shape)
    B = SB // S
    mean = torch.empty((S, C), device=x.device, dtype=torch.float32)
    var = torch.empty((S, C), device=x.device, dtype=torch.float32)
    out = torch.empty((SB, C, H // 2, W // 2), device=x.device, dtype=torch.float32) if pooled else torch.empty_like(x)
    gm = None if gamma is None else gamma.detach().contiguous()
    bt = None if beta is None else beta.detach().contiguous()
    nscr = int(L.load().rfn_stepbn_scratch_floats(S, B, C))  # partial sums of the split reductions (either way)
    acc = torch.empty((nscr,), device=x.device, dtype=torch.float32)
    return B, mean, var, out, gm, bt, nscr, acc


def _stepbn_running_args(running):
    """the running-statistics arguments of rfn_stepbn_fwd_f32 / rfn_stepbn_pool_fwd_f32 from `running` (or None)"""
    if running is None:
        return None, None, None, None, 1.0, None
    rm, rv, cf, cfu, decay, nbt = running
    if nbt is not None and (nbt.dtype != torch.int64 or not nbt.is_cuda):
        raise RuntimeError("num_batches_tracked must be an int64 device tensor")
    return L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cfu), decay, None if nbt is None else nbt.data_ptr()


def _stepbn_bwd_buffers(x, C, affine, nscr):
    """what a per-step BatchNorm backward allocates: (sums, gx, ggamma, gbeta); the last two None without affine"""
    sums = torch.empty((nscr,), device=x.device, dtype=torch.float32)
    gx = torch.empty_like(x)
    ggamma = torch.empty((C,), device=x.device, dtype=torch.float32) if affine else None
    gbeta = torch.empty((C,), device=x.device, dtype=torch.float32) if affine else None
    return sums, gx, ggamma, gbeta


class StepBatchNormActFn(torch.autograd.Function):
    """Training-mode BatchNorm2d with per-timestep statistics on a step-major time-batched tensor [S*B, C, H, W],
    fused with the activation that follows it (rfn_stepbn_{fwd,bwd}_f32: two launches each way).  Returns (y, mean[S, C],
    biased var[S, C]).  act: 0 none, 1 relu, 2 leaky_relu(slope), 3 tanh.  running (optional) = (running_mean, running_var,
    coef[S], coef_u[S], decay, num_batches_tracked or None): the S exponential-average updates of the step-wise calls,
    applied by the same launch (r <- decay r + sum_s coef[s] stat[s]); without it the caller does them."""

    @staticmethod
    def forward(ctx, x, gamma, beta, S, eps, act, slope, running=None):
        ctx.set_materialize_grads(False)  # mean / var are not differentiable: no zero gradients built for them
        x = x.contiguous()
        from . import dist as rdist
        if rdist.sync_batchnorm_on():
            return StepBatchNormActFn._forward_sync(ctx, x, gamma, beta, S, eps, act, slope, running)
        ctx.world = 1
        C, HW = int(x.shape[1]), int(x.shape[2]) * int(x.shape[3])
        B, mean, var, y, gm, bt, nscr, acc = _stepbn_fwd_buffers(x, gamma, beta, S)
        L.call("rfn_stepbn_fwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(y), L.dev(mean), L.dev(var), L.dev(acc),
               *_stepbn_running_args(running), S, B, C, HW, eps, act, slope, meta=_shell("stepbn_fwd", x, 3))
        ctx.save_for_backward(x, mean, var, gm, bt)
        ctx.cfg = (S, B, C, HW, eps, act, slope, gamma is not None, nscr)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def _forward_sync(ctx, x, gamma, beta, S, eps, act, slope, running):
        """synchronised BatchNorm (rfn_hip.dist.sync_batchnorm_on): the statistics of every step are those of the GLOBAL
        batch -- local moments, one all-gather of [2, S, C] floats, equal-count combination, apply with the given
        statistics; the running statistics follow the global moments (torch ops on [C] vectors)."""
        import torch.distributed as dist
        from . import dist as rdist
        C, HW = int(x.shape[1]), int(x.shape[2]) * int(x.shape[3])
        world = dist.get_world_size()
        B, mean, var, y, gm, bt, nscr, acc = _stepbn_fwd_buffers(x, gamma, beta, S)
        L.call("rfn_stepbn_fwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(y), L.dev(mean), L.dev(var), L.dev(acc),
               *_stepbn_running_args(None), S, B, C, HW, eps, act, slope)
        st = rdist.all_gather_cat(torch.stack((mean, var)).unsqueeze(0))          # [world, 2, S, C]
        mean = st[:, 0].mean(0).contiguous()
        var = (st[:, 1].mean(0) + (st[:, 0] - mean).pow(2).mean(0)).contiguous()  # equal counts per rank
        L.call("rfn_stepbn_apply_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(y), L.dev(mean), L.dev(var), S, B,
               C, HW, eps, act, slope)
        if running is not None:
            rm, rv, cf, cfu, decay, nbt = running
            n = B * HW * world
            cfu_g = cf * (n / max(n - 1, 1))          # unbiased variance of the global batch
            rm.mul_(decay).add_((cf.view(-1, 1) * mean).sum(0))
            rv.mul_(decay).add_((cfu_g.view(-1, 1) * var).sum(0))
            if nbt is not None:
                nbt.add_(S)
        ctx.save_for_backward(x, mean, var, gm, bt)
        ctx.cfg = (S, B, C, HW, eps, act, slope, gamma is not None, nscr)
        ctx.world = world
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, g, _gm, _gv):
        x, mean, var, gm, bt = ctx.saved_tensors
        S, B, C, HW, eps, act, slope, affine, nscr = ctx.cfg
        if g is None:
            return (None,) * 8
        g = g.contiguous()
        sums, gx, ggamma, gbeta = _stepbn_bwd_buffers(x, C, affine, nscr)
        args = (L.dev(x), L.dev(gm), L.dev(bt), L.dev(g), L.dev(mean), L.dev(var), L.dev(sums), L.dev(gx), L.dev(ggamma),
                L.dev(gbeta), S, B, C, HW, eps, act, slope)
        if ctx.world > 1:   # synchronised: partial sums, added over the ranks, apply
            from . import dist as rdist
            L.call("rfn_stepbn_bwd_f32", *args, 1, ctx.world)
            rdist.all_reduce_sum_(sums)
            L.call("rfn_stepbn_bwd_f32", *args, 2, ctx.world)
        else:
            L.call("rfn_stepbn_bwd_f32", *args, 0, 1)
        return gx, ggamma, gbeta, None, None, None, None, None


class StepBatchNormActPoolFn(torch.autograd.Function):
    """StepBatchNormActFn followed by MaxPool2d(2, 2) (rfn_stepbn_pool_{fwd,bwd}_f32: two launches each way).  Only the
    pooled map is written; the backward recomputes every window's winner from x, so no full-resolution activation, index
    map or full-resolution gradient exists.  Returns (p [S*B, C, H/2, W/2], mean[S, C], biased var[S, C]); arguments as
    StepBatchNormActFn.  H and W even; not for synchronised BatchNorm (the caller keeps the unfused route there)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, S, eps, act, slope, running=None):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        C, H, W = (int(v) for v in x.shape[1:])
        B, mean, var, p, gm, bt, nscr, acc = _stepbn_fwd_buffers(x, gamma, beta, S, pooled=True)
        # x read by the statistics and by the apply launch, a quarter of it written
        L.call("rfn_stepbn_pool_fwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(p), L.dev(mean), L.dev(var), L.dev(acc),
               *_stepbn_running_args(running), S, B, C, H, W, eps, act, slope, meta=_shell("stepbn_pool_fwd", x, 2.25))
        ctx.save_for_backward(x, mean, var, gm, bt)
        ctx.cfg = (S, B, C, H, W, eps, act, slope, gamma is not None, nscr)
        ctx.mark_non_differentiable(mean, var)
        return p, mean, var

    @staticmethod
    def backward(ctx, gp, _gm, _gv):
        x, mean, var, gm, bt = ctx.saved_tensors
        S, B, C, H, W, eps, act, slope, affine, nscr = ctx.cfg
        if gp is None:
            return (None,) * 8
        gp = gp.contiguous()
        sums, gx, ggamma, gbeta = _stepbn_bwd_buffers(x, C, affine, nscr)
        # x and the pooled gradient read by the reduce and by the apply launch, gx written
        L.call("rfn_stepbn_pool_bwd_f32", L.dev(x), L.dev(gm), L.dev(bt), L.dev(gp), L.dev(mean), L.dev(var), L.dev(sums),
               L.dev(gx), L.dev(ggamma), L.dev(gbeta), S, B, C, H, W, eps, act, slope, 0, 1,
               meta=_shell("stepbn_pool_bwd", x, 3.5))
        return gx, ggamma, gbeta, None, None, None, None, None


class Up2xCatFn(torch.autograd.Function):
    """torch.cat((nearest_up2x(x), skip), 1) in one launch (rfn_up2x_cat_f32); backward: gx = the 2x2 block sums of
    g[:, :Cx] read in place (rfn_up2x_cat_bwd_f32), the skip's gradient is the view g[:, Cx:]."""

    @staticmethod
    def forward(ctx, x, skip):
        N, Cx, h, w = (int(v) for v in x.shape)
        Cs = int(skip.shape[1])
        if tuple(skip.shape) != (N, Cs, 2 * h, 2 * w):
            raise RuntimeError("Up2xCatFn: skip %s does not fit x %s" % (tuple(skip.shape), tuple(x.shape)))
        dense = lambda t: all(t.shape[d] == 1 or t.stride(d) == e for d, e in
                              ((3, 1), (2, t.shape[3]), (1, t.shape[2] * t.shape[3])))
        x, skip = (t if dense(t) else t.contiguous() for t in (x, skip))   # channel-slice views are read in place
        xp, xns = L.frames(x, "x")
        sp, sns = L.frames(skip, "skip")
        out = torch.empty((N, Cx + Cs, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
        L.call("rfn_up2x_cat_f32", xp, xns, sp, sns, L.dev(out), N, Cx, Cs, h, w,
               meta=_shell("up2x_cat", out, 1.0 + (0.25 * Cx + Cs) / (Cx + Cs)))
        ctx.cfg = (N, Cx, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        N, Cx, h, w = ctx.cfg
        g = g.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gp, gns = L.frames(g, "g")
            gx = torch.empty((N, Cx, h, w), device=g.device, dtype=torch.float32)
            L.call("rfn_up2x_cat_bwd_f32", gp, gns, L.dev(gx), N, Cx, h, w, meta=_shell("up2x_cat_bwd", gx, 5))
        return gx, (g[:, Cx:] if ctx.needs_input_grad[1] else None)


def bnflow_coef(steps, momentum):
    """(coef [steps] as float64, decay) of the closed form of `steps` running-statistics updates r <- m r + (1 - m) stat_s of
    BatchNormFlow (glow_modules.py:81-87; the momentum weights the OLD value): r <- decay r + sum_s coef[s] stat_s with
    decay = m^S, coef[s] = (1 - m) m^(S-1-s) and 0^0 = 1.  Needs no device."""
    m = float(momentum)
    coef = (1.0 - m) * torch.tensor([m ** (steps - 1 - s) for s in range(steps)], dtype=torch.float64)
    return coef, m ** steps


class BatchNormFlowFn(torch.autograd.Function):
    """BatchNormFlow in training mode, forward direction (glow_modules.py:76-98), on a step-major time-batched tensor
    x [steps*B, C, H, W] with the statistics of EACH step's B rows (rfn_bnflow_{fwd,bwd}_f32, two launches each way).
    log_gamma / beta: [1, C, H, W].  Returns (z, dl [steps]); dl[s] belongs to the log-det of every row of step s.
    running = (running_mean, running_var, coef [steps] device tensor, decay) or None: the `steps` updates of the
    step-wise calls, applied by the same launches in closed form (bnflow_coef)."""

    @staticmethod
    def forward(ctx, x, log_gamma, beta, steps, eps, running=None):
        x = x.contiguous()
        S, B = int(steps), int(x.shape[0]) // int(steps)
        E = x[0].numel()
        if S * B != x.shape[0] or log_gamma.numel() != E or beta.numel() != E:
            raise RuntimeError("BatchNormFlowFn: x %s is not %d steps of rows of %d elements" % (tuple(x.shape), S, log_gamma.numel()))
        lg, bt = _f(log_gamma), _f(beta)
        z = torch.empty_like(x)
        mean = torch.empty((S, E), device=x.device, dtype=torch.float32)
        var = torch.empty((S, E), device=x.device, dtype=torch.float32)
        dl = torch.empty((S,), device=x.device, dtype=torch.float32)
        scr = torch.empty((int(L.load().rfn_bnflow_scratch_floats(S, B, E, 0)),), device=x.device, dtype=torch.float32)
        rm = rv = cf = None
        decay = 1.0
        if running is not None:
            rm, rv, cf, decay = running
            if not (rm.is_contiguous() and rv.is_contiguous()) or rm.numel() != E or rv.numel() != E or cf.numel() != S:
                raise RuntimeError("BatchNormFlowFn: running statistics must be dense [%d] tensors, coef [%d]" % (E, S))
        L.call("rfn_bnflow_fwd_f32", L.dev(x), L.dev(lg), L.dev(bt), L.dev(z), L.dev(mean), L.dev(var), L.dev(dl),
               L.dev(scr), L.dev(rm), L.dev(rv), L.dev(cf), L.dev(cf), decay, S, B, E,
               eps, meta=_shell("bnflow_fwd", x, 2))
        ctx.save_for_backward(x, lg, mean, var)
        ctx.cfg = (S, B, E, log_gamma.shape)
        return z, dl

    @staticmethod
    def backward(ctx, gz, gdl):
        x, lg, mean, var = ctx.saved_tensors
        S, B, E, pshape = ctx.cfg
        gz = torch.zeros_like(x) if gz is None else gz.contiguous()
        gdl = None if gdl is None else gdl.contiguous()
        gx = torch.empty_like(x)
        glg = torch.empty(pshape, device=x.device, dtype=torch.float32)
        gbt = torch.empty(pshape, device=x.device, dtype=torch.float32)
        scr = torch.empty((int(L.load().rfn_bnflow_scratch_floats(S, B, E, 1)),), device=x.device, dtype=torch.float32)
        L.call("rfn_bnflow_bwd_f32", L.dev(x), L.dev(lg), L.dev(gz), L.dev(gdl), L.dev(mean), L.dev(var), L.dev(gx),
               L.dev(glg), L.dev(gbt), L.dev(scr), S, B, E, meta=_shell("bnflow_bwd", x, 3))
        return gx, glg, gbt, None, None, None


def bnflow_apply(x, log_gamma, beta, running_mean, running_var, reverse):
    """BatchNormFlow with GIVEN statistics (glow_modules.py:90-103: eval mode, and the reverse direction in any mode), no
    gradient: (y, dl [1]) by rfn_bnflow_apply_f32; dl is to be ADDED to the log-det of every row (it carries the reverse
    direction's minus sign)."""
    x = x.detach().contiguous()
    N, E = int(x.shape[0]), x[0].numel()
    y = torch.empty_like(x)
    dl = torch.empty((1,), device=x.device, dtype=torch.float32)
    lg, bt, rm, rv = _f(log_gamma), _f(beta), _f(running_mean), _f(running_var)
    if not (lg.numel() == bt.numel() == rm.numel() == rv.numel() == E):
        raise RuntimeError("bnflow_apply: parameters do not match rows of %d elements" % E)
    L.call("rfn_bnflow_apply_f32", L.dev(x), L.dev(lg), L.dev(bt), L.dev(rm), L.dev(rv), L.dev(y), L.dev(dl), N, E,
           1 if reverse else 0, meta=_shell("bnflow_apply", x, 2))
    return y, dl


# ----------------------------------------------------------------------------------------------- mixture of logistics
def mol_dims(x, l):
    """(N, C, M, HW) of a mixture-of-discretized-logistics call, or a RuntimeError naming what does not fit.  x [N,C,H,W]
    with C in {1, 3}; l [N,Cl,H,W] with Cl = 10 M (C = 3) or 3 M (C = 1).  Needs no device."""
    if x.dim() != 4 or l.dim() != 4:
        raise RuntimeError("mol: x and l must be [N,C,H,W], got %s and %s" % (tuple(x.shape), tuple(l.shape)))
    N, C, H, W = (int(d) for d in x.shape)
    if C not in (1, 3):
        raise RuntimeError("mol: x must have 1 or 3 channels, got %d" % C)
    per = 10 if C == 3 else 3
    Cl = int(l.shape[1])
    if (int(l.shape[0]), int(l.shape[2]), int(l.shape[3])) != (N, H, W) or Cl < per or Cl % per:
        raise RuntimeError("mol: logits %s do not fit x %s: need [%d, %d*M, %d, %d] with M >= 1" %
                           (tuple(l.shape), tuple(x.shape), N, per, H, W))
    return N, C, Cl // per, H * W


class MolNllFn(torch.autograd.Function):
    """nll_pix [N,H,W] (reduce = 0) or its per-frame sum nll [N] (reduce = 1) of x under the mixture of discretized
    logistics with parameters l (rfn_mol_nll_fwd / rfn_mol_nll_bwd).  Gradient into l only."""

    @staticmethod
    def forward(ctx, x, l, per_frame):
        N, C, M, HW = mol_dims(x, l)
        x, l = x.detach().contiguous(), l.contiguous()
        L.dev(x, "x"), L.dev(l, "l")  # (device fp32 tensors, before anything is allocated or loaded)
        nll_pix =torch.empty((N, x.shape[2], x.shape[3]), device=l.device, dtype=torch.float32)
        lse = torch.empty_like(nll_pix)
        nll = torch.empty((N,), device=l.device, dtype=torch.float32)
        part = torch.empty((int(L.load().rfn_mol_part_floats(N, HW)),), device=l.device, dtype=torch.float32)
        L.call("rfn_mol_nll_fwd", L.dev(x, "x"), L.dev(l, "l"), L.dev(nll_pix), L.dev(lse), L.dev(nll), L.dev(part), N, C,
               M, HW, meta=_shell("mol_nll_fwd", l, 1))
        ctx.save_for_backward(x, l, lse)
        ctx.cfg = (N, C, M, HW, per_frame)
        return nll if per_frame else nll_pix

    @staticmethod
    def backward(ctx, g):
        x, l, lse = ctx.saved_tensors
        N, C, M, HW, per_frame = ctx.cfg
        g = g.contiguous()
        dl = torch.empty_like(l)
        L.call("rfn_mol_nll_bwd", L.dev(x), L.dev(l), L.dev(lse), L.dev(g, "grad"), 0 if per_frame else 1, L.dev(dl),
               N, C, M, HW, meta=_shell("mol_nll_bwd", l, 2))
        return None, dl, None


def mol_nll(x, l, reduce="frame"):
    """Negative log-likelihood of x [N,C,H,W] in [-1,1] under the mixture of discretized logistics l [N,Cl,H,W]:
    reduce="pixel" -> [N,H,W], reduce="frame" -> [N], each frame's pixels summed in a fixed order (the bits of a frame do
    not depend on the other frames of the call).  Differentiable in l; x must not require a gradient."""
    if reduce not in ("frame", "pixel"):
        raise ValueError("mol_nll: reduce must be 'frame' or 'pixel', got %r" % (reduce,))
    if x.requires_grad:
        raise RuntimeError("mol_nll: no gradient flows into x; pass x.detach()")
    return MolNllFn.apply(x, l, reduce == "frame")


def mol_sample(l, u_mix=None, u_x=None, generator=None, channels=None):
    """Draw x [N,C,H,W] from the mixture l [N,Cl,H,W] (rfn_mol_sample); no gradient.  u_mix [N,H,W,M] and u_x [N,H,W,C]
    are the reference's two uniform draws, in (1e-5, 1 - 1e-5); drawn here, in that order, from `generator` when not
    given.  C is `channels`, else the last extent of u_x, else what Cl allows (10 M: RGB, 3 M: gray); a Cl that allows
    both (30, 60, ...) needs one of the two."""
    if l.dim() != 4:
        raise RuntimeError("mol_sample: l must be [N,Cl,H,W], got %s" % (tuple(l.shape),))
    N, Cl, H, W = (int(d) for d in l.shape)
    C = channels
    if C is None and u_x is not None:
        C = int(u_x.shape[-1])
    if C is None:
        fits = [c for c, per in ((3, 10), (1, 3)) if Cl >= per and Cl % per == 0]
        if len(fits) != 1:
            raise RuntimeError("mol_sample: %d logit channels %s; pass channels=1 or 3" %
                               (Cl, "fit both RGB and gray" if fits else "fit neither 10*M nor 3*M"))
        C = fits[0]
    per = 10 if C == 3 else 3
    if C not in (1, 3) or Cl < per or Cl % per:
        raise RuntimeError("mol_sample: %d logit channels do not fit %d colour channels (need %d*M)" % (Cl, C, per))
    M = Cl // per
    l = l.detach().contiguous()
    L.dev(l, "l")
    if u_mix is None:
        u_mix = torch.empty((N, H, W, M), device=l.device, dtype=torch.float32).uniform_(1e-5, 1. - 1e-5, generator=generator)
    if u_x is None:
        u_x = torch.empty((N, H, W, C), device=l.device, dtype=torch.float32).uniform_(1e-5, 1. - 1e-5, generator=generator)
    if tuple(u_mix.shape) != (N, H, W, M) or tuple(u_x.shape) != (N, H, W, C):
        raise RuntimeError("mol_sample: uniforms must be [N,H,W,M] = %s and [N,H,W,C] = %s, got %s and %s" %
                           ((N, H, W, M), (N, H, W, C), tuple(u_mix.shape), tuple(u_x.shape)))
    u_mix, u_x = u_mix.contiguous(), u_x.contiguous()
    out = torch.empty((N, C, H, W), device=l.device, dtype=torch.float32)
    L.call("rfn_mol_sample", L.dev(l), L.dev(u_mix, "u_mix"), L.dev(u_x, "u_x"), L.dev(out), N, C, M,
           H * W, meta=_shell("mol_sample", l, 1))
    return out


MOL_KEYED_SLOT_MIX, MOL_KEYED_SLOT_COLOUR = 16, 17   # the key's slot word (keyed_normal owns 0 .. 7)


def _mol_channels(who, Cl, channels):
    """(C, M) of Cl logit channels: C is `channels`, else what Cl allows (10 M: RGB, 3 M: gray)"""
    C = channels
    if C is None:
        fits = [c for c, per in ((3, 10), (1, 3)) if Cl >= per and Cl % per == 0]
        if len(fits) != 1:
            raise RuntimeError("%s: %d logit channels %s; pass channels=1 or 3" %
                               (who, Cl, "fit both RGB and gray" if fits else "fit neither 10*M nor 3*M"))
        C = fits[0]
    per = 10 if C == 3 else 3
    if C not in (1, 3) or Cl < per or Cl % per:
        raise RuntimeError("%s: %d logit channels do not fit %d colour channels (need %d*M)" % (who, Cl, C, per))
    return C, Cl // per


def _mol_keyed_address(who, rows, B, seed, step, first_seq, first_draw):
    B, seed, step, first_seq, first_draw = (int(v) for v in (B, seed, step, first_seq, first_draw))
    if B < 1 or rows < 1 or rows % B:
        raise ValueError("%s: %d rows are no positive multiple of B = %d (row r*B + b is draw first_draw + r of sequence "
                         "first_seq + b)" % (who, rows, B))
    for v, nm in ((seed, "seed"), (first_seq, "first_seq"), (first_draw, "first_draw")):
        if not 0 <= v < 1 << 63:
            raise ValueError("%s: %s %d not in [0, 2^63)" % (who, nm, v))
    if not 0 <= step < 1 << 31:
        raise ValueError("%s: step %d not in [0, 2^31)" % (who, step))
    return B, seed, step, first_seq, first_draw


def mol_sample_keyed(l, B, seed, step, first_seq=0, first_draw=0, channels=None):
    """mol_sample with addressed uniforms (rfn_mol_sample_keyed; include/rfn_hip.h and DESIGN section 20 hold the
    definition): x [rows,C,H,W] from the mixture l [rows,Cl,H,W], rows a multiple of B.  Row r*B + b is draw first_draw +
    r of sequence first_seq + b, and a pixel's uniforms depend only on (seed, step, sequence, draw, pixel, element): the
    same for any B, number of draws and split of the draws into calls.  No uniform tensor exists and torch's generator
    is not touched; mol_keyed_uniforms writes the numbers out.  One launch on the current stream; no CPU fallback."""
    if l.dim() != 4:
        raise RuntimeError("mol_sample_keyed: l must be [rows,Cl,H,W], got %s" % (tuple(l.shape),))
    rows, Cl, H, W = (int(d) for d in l.shape)
    C, M = _mol_channels("mol_sample_keyed", Cl, channels)
    B, seed, step, first_seq, first_draw = _mol_keyed_address("mol_sample_keyed", rows, B, seed, step, first_seq,
                                                              first_draw)
    l = l.detach().contiguous()
    L.dev(l, "l")
    out = torch.empty((rows, C, H, W), device=l.device, dtype=torch.float32)
    with torch.cuda.device(l.device):
        L.call("rfn_mol_sample_keyed", L.dev(l), L.dev(out), rows, B, C, M, H * W, seed, step, first_seq, first_draw,
               meta=_shell("mol_sample_keyed", l, 1))
    return out


def mol_keyed_uniforms(shape_or_l, B, M, channels, seed, step, first_seq=0, first_draw=0, device=None):
    """(u_mix [rows,H,W,M], u_x [rows,H,W,C]): the uniforms mol_sample_keyed uses at that address
    (rfn_mol_keyed_uniforms), so that mol_sample(l, u_mix, u_x) replays it bit for bit.  shape_or_l: the logits (their
    rows, H, W and device are taken) or (rows, H, W); device: where the tensors go for a shape (default: the current
    GPU)."""
    if isinstance(shape_or_l, torch.Tensor):
        if shape_or_l.dim() != 4:
            raise RuntimeError("mol_keyed_uniforms: l must be [rows,Cl,H,W], got %s" % (tuple(shape_or_l.shape),))
        rows, _, H, W = (int(d) for d in shape_or_l.shape)
        device = shape_or_l.device
    else:
        if len(shape_or_l) != 3:
            raise ValueError("mol_keyed_uniforms: give the logits or (rows, H, W), got %s" % (tuple(shape_or_l),))
        rows, H, W = (int(d) for d in shape_or_l)
    M, C = int(M), int(channels)
    if M < 1 or C not in (1, 3) or H < 1 or W < 1:
        raise ValueError("mol_keyed_uniforms: need M >= 1, channels 1 or 3 and a non-empty frame (got M = %d, channels = "
                         "%d, %dx%d)" % (M, C, H, W))
    B, seed, step, first_seq, first_draw = _mol_keyed_address("mol_keyed_uniforms", rows, B, seed, step, first_seq,
                                                              first_draw)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rfn_hip kernels need device tensors; mol_keyed_uniforms was asked for %s (no CPU fallback)" %
                           device)
    u_mix = torch.empty((rows, H, W, M), device=device, dtype=torch.float32)
    u_x = torch.empty((rows, H, W, C), device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        L.call("rfn_mol_keyed_uniforms", L.dev(u_mix), L.dev(u_x), rows, B, C, M, H * W, seed, step, first_seq,
               first_draw, meta=("shell", "mol_keyed_uniforms", 0.0, "%dx%dx%d" % (rows, H * W, M + C),
                                 4.0 * (u_mix.numel() + u_x.numel())))
    return u_mix, u_x


# ----------------------------------------------------------------------------------------------- evaluation metrics
def _u8_frames(t, C, H, W):
    """(tensor, pointer, frame stride) of a uint8 device tensor [..., C, H, W] seen as [N, C, H, W] frames (lib.dev stays
    fp32-only): no copy when the leading dims collapse to one frame stride and every frame is dense and disjoint (e.g.
    a channel slice), a contiguous copy otherwise (e.g. `x[:, start:]` of [B, T, C, H, W]).  Returns the tensor the
    pointer refers to as well: the caller keeps it alive over the launch."""
    v = t.reshape(-1, C, H, W)
    s = v.stride()
    dense = s[3] == 1 and s[2] == W and (s[1] == H * W or C == 1)
    if not dense or (v.shape[0] > 1 and s[0] < C * H * W):
        v = v.contiguous()
    ns = v.stride(0) if v.shape[0] > 1 else C * H * W
    return v, v.data_ptr(), int(ns)


def frame_quality(a, b):
    """Per-frame (mse, psnr, ssim) of two uint8 video tensors [..., C, H, W] on the GPU (rfn_frame_quality_u8: the
    reference's Evaluator.eval_seq, error_metrics.py:154-171, with skimage 0.17.2's SSIM / PSNR defaults): float32
    tensors over the leading shape.  mse = sum of squared differences / (C*H*W); psnr, ssim = means over channels of the
    single-channel figures (psnr is +inf on an identical channel).  No CPU fallback."""
    for t, nm in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("frame_quality: %s must be a tensor, got %s" % (nm, type(t).__name__))
        if t.dtype != torch.uint8:
            raise TypeError("frame_quality: %s must be uint8, got %s" % (nm, t.dtype))
        if t.dim() < 3:
            raise ValueError("frame_quality: %s must be [..., C, H, W], got shape %s" % (nm, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("frame_quality: shapes differ: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    C, H, W = (int(d) for d in a.shape[-3:])
    if H < 7 or W < 7:
        raise ValueError("frame_quality: the 7x7 SSIM window exceeds the %dx%d frame" % (H, W))
    if C < 1:
        raise ValueError("frame_quality: frames have no channel")
    for t, nm in ((a, "a"), (b, "b")):
        if not t.is_cuda:
            raise RuntimeError("rfn_hip kernels need device tensors; %s is on %s (no CPU fallback)" % (nm, t.device))
    if a.device != b.device:
        raise ValueError("frame_quality: a is on %s, b on %s" % (a.device, b.device))
    lead = tuple(a.shape[:-3])
    mse = torch.empty(lead, device=a.device, dtype=torch.float32)
    psnr = torch.empty_like(mse)
    ssim = torch.empty_like(mse)
    N = mse.numel()
    if N == 0:
        return mse, psnr, ssim
    av, ap, ans = _u8_frames(a, C, H, W)
    bv, bp, bns = _u8_frames(b, C, H, W)
    with torch.cuda.device(a.device):
        L.call("rfn_frame_quality_u8", ap, ans, bp, bns, L.dev(mse), L.dev(psnr), L.dev(ssim), N, C,
               H, W, meta=("shell", "frame_quality", 0.0, "x".join(str(int(d)) for d in a.shape),
                                  2.0 * a.numel()))
    return mse, psnr, ssim


# ----------------------------------------------------------------------------------------------- linear-extrapolation baseline
@functools.lru_cache(maxsize=None)
def linext_limits():
    """(most conditioning frames, smallest and largest frame side of gauss_quality): the library's host-only queries
    (include/rfn_hip.h), read once; needs no device"""
    lib = L.load()
    return lib.rfn_linext_max_frames(), lib.rfn_gauss_quality_min_side(), lib.rfn_gauss_quality_max_side()


def linear_extrap_pairs(n):
    """the features of a window of n frames in the kernels' order (SimpleLinearModel.get_prediction): a list of
    (i, j or None), frame i itself or the difference frame i - frame j; n (n + 1) / 2 entries"""
    n = int(n)
    if n < 1:
        raise ValueError("linear_extrap_pairs: n must be >= 1, got %d" % n)
    pairs = [(f, None) for f in range(n)]
    for k in range(n - 1):
        pairs += [(j, j + k + 1) for j in range(n - k - 1)]
    return pairs


def linear_extrap_check(x, W, bias, n, start=0, P=None):
    """(B, T, CHW, F) of a linear_extrap_loss (P None) or linear_extrap_rollout call, or a ValueError naming what does
    not fit.  Needs no device."""
    who = "linear_extrap_loss" if P is None else "linear_extrap_rollout"
    for nm, v in (("n", n), ("start", start)) + ((("P", P),) if P is not None else ()):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s: %s must be an int, got %r" % (who, nm, v))
    if not 1 <= n <= linext_limits()[0]:
        raise ValueError("%s: n must be in 1..%d, got %d" % (who, linext_limits()[0], n))
    if start < 0:
        raise ValueError("%s: start must be >= 0, got %d" % (who, start))
    if P is not None and P < 1:
        raise ValueError("%s: P must be >= 1, got %d" % (who, P))
    for nm, t in (("x", x), ("W", W), ("bias", bias)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, nm, type(t).__name__))
        if t.dtype != torch.float32:
            raise ValueError("%s: %s must be float32, got %s" % (who, nm, t.dtype))
        if t.device != x.device:
            raise ValueError("%s: %s is on %s, x on %s" % (who, nm, t.device, x.device))
    if x.dim() != 5 or min(x.shape) < 1:
        raise ValueError("%s: x must be [B, T, C, H, W] with no empty dimension, got shape %s" % (who, tuple(x.shape)))
    B, T = int(x.shape[0]), int(x.shape[1])
    need = start + n + (1 if P is None else 0)
    if T < need:
        raise ValueError("%s: T = %d frames, start = %d and n = %d need T >= %d%s"
                         % (who, T, start, n, need, " (the window and its target)" if P is None else ""))
    F = n * (n + 1) // 2
    if W.numel() != F:
        raise ValueError("%s: W has %d elements (shape %s), n = %d needs F = n (n + 1) / 2 = %d"
                         % (who, W.numel(), tuple(W.shape), n, F))
    if bias.numel() != 1:
        raise ValueError("%s: bias has %d elements (shape %s), 1 is needed" % (who, bias.numel(), tuple(bias.shape)))
    CHW = int(x.shape[2]) * int(x.shape[3]) * int(x.shape[4])
    if B >= 2 ** 31 or (P is not None and P >= 2 ** 31):
        raise ValueError("%s: B and P must fit an int32" % who)
    return B, T, CHW, F


def _linext_frames(x):
    """(tensor, sequence stride, frame stride) of x [B, T, C, H, W] for the linear-extrapolation kernels: x itself when
    every frame is a dense block (a slice along B or T is read in place), a contiguous copy otherwise"""
    _, T, C, H, W = x.shape
    s = x.stride()
    dense = (W == 1 or s[4] == 1) and (H == 1 or s[3] == W) and (C == 1 or s[2] == H * W)
    if not dense or (T > 1 and s[1] < C * H * W) or (x.shape[0] > 1 and s[0] < (T - 1) * s[1] + C * H * W):
        x = x.contiguous()
        s = x.stride()
    fs = int(s[1]) if T > 1 else C * H * W
    ss = int(s[0]) if x.shape[0] > 1 else (T - 1) * fs + C * H * W
    return x, ss, fs


class LinearExtrapLossFn(torch.autograd.Function):
    """the MSE of the one-step prediction and the gradients of its 16-odd parameters in one pass over the frames
    (rfn_linext_train_f32, include/rfn_hip.h).  Saves the gradients; the backward scales them by the incoming scalar.
    There is no gradient to x."""

    @staticmethod
    def forward(ctx, x, W, bias, n, start):
        B, T, CHW, F = linear_extrap_check(x, W, bias, n, start)
        xv, ss, fs = _linext_frames(x.detach())
        w, b = W.detach().contiguous(), bias.detach().contiguous()
        ptrs = (L.dev(xv, "x", check_contiguous=False), L.dev(w, "W"), L.dev(b, "bias"))   # (device tensors or an error)
        partials = torch.empty(L.load().rfn_linext_max_blocks() * (F + 2), device=x.device, dtype=torch.float32)
        out = torch.empty(F + 2, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            L.call("rfn_linext_train_f32", ptrs[0], ss, fs, start, ptrs[1], ptrs[2], L.dev(partials), partials.numel(), L.dev(out), B, T, n, CHW,
                   meta=("shell", "linext_train", 0.0, "x".join(str(int(d)) for d in x.shape), 4.0 * B * (n + 1) * CHW))
        ctx.save_for_backward(out)
        ctx.shapes = (tuple(W.shape), tuple(bias.shape), F)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        w_shape, b_shape, F = ctx.shapes
        need = ctx.needs_input_grad
        scaled = out[1:] * g    # one fp32 multiply per gradient
        return (None, scaled[:F].reshape(w_shape) if need[1] else None,
                scaled[F:].reshape(b_shape) if need[2] else None, None, None)


def linear_extrap_loss(x, W, bias, n, start=0):
    """MSE (mean over B*C*H*W) between the linear-extrapolation prediction from frames start .. start+n-1 of x
    [B, T, C, H, W] and frame start+n, differentiable in W [F] (any shape of F elements) and bias (one element).  Two
    launches on the current stream (the pass over the frames and the fixed-order sum of its partials); no CPU fallback."""
    linear_extrap_check(x, W, bias, n, start)
    return LinearExtrapLossFn.apply(x, W, bias, n, start)


def linear_extrap_rollout(x, W, bias, n, P, start=0):
    """[B, P, C, H, W]: P frames predicted autoregressively from the window x[:, start:start+n], each prediction
    replacing the window's oldest frame (SimpleLinearModel.sample; P = 1 is get_prediction).  No clamping, no gradient.
    One launch on the current stream; no CPU fallback."""
    B, T, CHW, _ = linear_extrap_check(x, W, bias, n, start, P)
    xv, ss, fs = _linext_frames(x.detach())
    w, b = W.detach().contiguous(), bias.detach().contiguous()
    ptrs = (L.dev(xv, "x", check_contiguous=False), L.dev(w, "W"), L.dev(b, "bias"))   # (device tensors or an error)
    out = torch.empty((B, P) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        L.call("rfn_linext_rollout_f32", ptrs[0], ss, fs, start, ptrs[1], ptrs[2], L.dev(out), B, T, n, P, CHW,
               meta=("shell", "linext_rollout", 0.0, "x".join(str(int(d)) for d in out.shape), 4.0 * B * (n + P) * CHW))
    return out


def gauss_quality_check(pred, true, scale=255.0, lo=0.0, hi=255.0):
    """(N, C, H, W) of a gauss_quality call, or a ValueError naming what does not fit.  Needs no device."""
    for nm, t in (("pred", pred), ("true", true)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("gauss_quality: %s must be a tensor, got %s" % (nm, type(t).__name__))
        if t.dtype != torch.float32:
            raise ValueError("gauss_quality: %s must be float32, got %s" % (nm, t.dtype))
        if t.dim() != 4 or min(t.shape) < 1:
            raise ValueError("gauss_quality: %s must be [N, C, H, W] with no empty dimension, got shape %s"
                             % (nm, tuple(t.shape)))
    if tuple(pred.shape) != tuple(true.shape):
        raise ValueError("gauss_quality: shapes differ: pred %s, true %s" % (tuple(pred.shape), tuple(true.shape)))
    if pred.device != true.device:
        raise ValueError("gauss_quality: pred is on %s, true on %s" % (pred.device, true.device))
    N, C, H, W = (int(d) for d in pred.shape)
    _, side_min, side_max = linext_limits()
    for nm, v in (("H", H), ("W", W)):
        if not side_min <= v <= side_max:
            raise ValueError("gauss_quality: %s = %d, frames of %d..%d rows and columns are supported (the 11-tap window "
                             "needs 11; the kernel holds rows of at most 128)"
                             % (nm, v, side_min, side_max))
    scale, lo, hi = float(scale), float(lo), float(hi)
    if not (scale == scale and lo <= hi):
        raise ValueError("gauss_quality: scale must be a number and lo <= hi, got scale %r, lo %r, hi %r" % (scale, lo, hi))
    return N, C, H, W


def gauss_quality(pred, true, scale=255.0, lo=0.0, hi=255.0):
    """(ssim [N], psnr [N], mse [N]) of float32 frames [N, C, H, W], each read once as clamp(v * scale, lo, hi) (no
    scaled copy is written): ssim is pytorch_msssim.ssim(X, Y, data_range=255) per image (11-tap Gaussian window,
    sigma 1.5, no padding; DESIGN.md section 26 states it), mse the mean squared difference over C*H*W,
    psnr = 10 log10(255^2 / mse), +inf where mse == 0.  The data range of ssim and psnr is 255 whatever the scale.  One
    launch on the current stream; no CPU fallback."""
    N, C, H, W = gauss_quality_check(pred, true, scale, lo, hi)
    p, t = pred.detach().contiguous(), true.detach().contiguous()
    ptrs = (L.dev(p, "pred"), L.dev(t, "true"))   # (device tensors or an error)
    ssim = torch.empty(N, device=pred.device, dtype=torch.float32)
    mse = torch.empty_like(ssim)
    with torch.cuda.device(pred.device):
        L.call("rfn_gauss_quality_f32", ptrs[0], ptrs[1], L.dev(ssim), L.dev(mse), N, C, H, W,
               float(scale), float(lo), float(hi),
               meta=("shell", "gauss_quality", 0.0, "x".join(str(int(d)) for d in pred.shape), 8.0 * pred.numel()))
    psnr = 10.0 * torch.log10(255.0 ** 2 / mse)   # (+inf at mse == 0: IEEE division)
    return ssim, psnr, mse


def _moving_mnist_args(fn, digits, B, T, C, S, num_digits, step_length, seed, split, first_id):
    """the argument checks the two Moving MNIST renderers share; returns the contiguous digits and the integers"""
    if not isinstance(digits, torch.Tensor) or digits.dtype != torch.uint8:
        raise TypeError("%s: digits must be a uint8 tensor, got %s" %
                        (fn, digits.dtype if isinstance(digits, torch.Tensor) else type(digits).__name__))
    if digits.dim() != 3 or tuple(digits.shape[1:]) != (28, 28) or digits.shape[0] < 1:
        raise ValueError("%s: digits must be [N >= 1, 28, 28], got %s" % (fn, tuple(digits.shape),))
    if not digits.is_cuda:
        raise RuntimeError("rfn_hip kernels need device tensors; digits is on %s (no CPU fallback)" % digits.device)
    B, T, C, S, nd, L_, seed, split, first_id = (int(v) for v in (B, T, C, S, num_digits, step_length, seed, split,
                                                                  first_id))
    if B < 0 or T < 1 or C < 1:
        raise ValueError("%s: need B >= 0, T >= 1, C >= 1 (got %d, %d, %d)" % (fn, B, T, C))
    if not 28 < S <= 4096:
        raise ValueError("%s: image size %d must exceed the digit size 28 (and be <= 4096)" % (fn, S))
    if not 1 <= nd <= 8:
        raise ValueError("%s: num_digits %d not in [1, 8]" % (fn, nd))
    if not 1 <= L_ <= 1 << 20:
        raise ValueError("%s: step_length %d must be >= 1" % (fn, L_))
    for v, nm in ((seed, "seed"), (split, "split"), (first_id, "first_id")):
        if not 0 <= v < 1 << 63:
            raise ValueError("%s: %s %d not in [0, 2^63)" % (fn, nm, v))
    if B * T > 0x7fffffff:
        raise ValueError("%s: B * T = %d frames exceed one launch" % (fn, B * T))
    return digits.contiguous(), B, T, C, S, nd, L_, seed, split, first_id


def moving_mnist_render(digits, B, T, C, S, num_digits, step_length, deterministic, seed, split, first_id,
                        trajectories=False):
    """Stochastic Moving MNIST batch rendered on the GPU (rfn_moving_mnist_render_f32: the reference's
    MovingMNIST.__getitem__, stochasticMovingMnist.py:48-127, with addressed random draws): a fresh float32 tensor
    [B, T, C, S, S] in [0, 1] on the digits' device, sequence b having the id first_id + b; with trajectories=True also
    the int64 [B, num_digits, T, 3] (digit index, y, x) of every digit and frame.  `digits`: uint8 [N, 28, 28] device
    table.  One launch on the current stream; no CPU fallback."""
    digits, B, T, C, S, nd, L_, seed, split, first_id = _moving_mnist_args(
        "moving_mnist_render", digits, B, T, C, S, num_digits, step_length, seed, split, first_id)
    out = torch.empty((B, T, C, S, S), device=digits.device, dtype=torch.float32)
    traj = torch.empty((B, nd, T, 3), device=digits.device, dtype=torch.int64) if trajectories else None
    if B:
        with torch.cuda.device(digits.device):
            L.call("rfn_moving_mnist_render_f32", digits.data_ptr(), int(digits.shape[0]),
                   L.dev(out), traj.data_ptr() if traj is not None else None, B, T, C,
                   S, nd, L_, 1 if deterministic else 0, seed, split, first_id,
                   meta=("shell", "moving_mnist", 0.0, "%dx%dx%dx%dx%d" % (B, T, C, S, S), 4.0 * out.numel()))
    return (out, traj) if trajectories else out


def moving_mnist_sync_render(digits, B, T, C, S, num_digits, step_length, deterministic, seed, split, first_id,
                             trajectories=False, hits=False):
    """Synchronized Moving MNIST batch (rfn_moving_mnist_sync_render_f32: the reference's MovingMNIST_synchronized,
    stochasticMovingMnist.py:131-248): moving_mnist_render's arguments and outputs, but all sequences share one
    trajectory per digit (start position drawn, velocity (3, 3), the bounces with step_length / deterministic) and only
    the digit identities depend on the sequence id.  With hits=True also the int32 [B, T] hit table: the largest
    n + 1 over the digits clamped at a wall on frame t, 0 if none (every row the same).  Returns out, or the tuple
    (out[, traj][, hit]).  One launch on the current stream; no CPU fallback."""
    digits, B, T, C, S, nd, L_, seed, split, first_id = _moving_mnist_args(
        "moving_mnist_sync_render", digits, B, T, C, S, num_digits, step_length, seed, split, first_id)
    out = torch.empty((B, T, C, S, S), device=digits.device, dtype=torch.float32)
    traj = torch.empty((B, nd, T, 3), device=digits.device, dtype=torch.int64) if trajectories else None
    hit = torch.empty((B, T), device=digits.device, dtype=torch.int32) if hits else None
    if B:
        with torch.cuda.device(digits.device):
            L.call("rfn_moving_mnist_sync_render_f32", digits.data_ptr(), int(digits.shape[0]),
                   L.dev(out), traj.data_ptr() if traj is not None else None,
                   hit.data_ptr() if hit is not None else 0, B, T, C,
                   S, nd, L_, 1 if deterministic else 0, seed, split, first_id,
                   meta=("shell", "moving_mnist_sync", 0.0, "%dx%dx%dx%dx%d" % (B, T, C, S, S), 4.0 * out.numel()))
    extra = tuple(v for v in (traj, hit) if v is not None)
    return (out,) + extra if extra else out


def _clip_gather_args(fn, store, first, T, C):
    """the argument checks the two clip gathers share; returns the contiguous tensors and the integers"""
    for t, nm, dt in ((store, "store", torch.uint8), (first, "first", torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError("%s: %s must be a %s tensor, got %s" %
                            (fn, nm, str(dt).replace("torch.", ""),
                             t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
    if store.dim() != 4 or min(int(d) for d in store.shape[1:3]) < 1:
        raise ValueError("%s: store must be [F, H >= 1, W >= 1, Cs], got %s" % (fn, tuple(store.shape),))
    if first.dim() != 1:
        raise ValueError("%s: first must be [B], got %s" % (fn, tuple(first.shape),))
    F, H, W, Cs = (int(d) for d in store.shape)
    B, T, C = int(first.shape[0]), int(T), int(C)
    if T < 1:
        raise ValueError("%s: need T >= 1, got %d" % (fn, T))
    if (C, Cs) not in ((1, 1), (3, 1), (3, 3)):
        raise ValueError("%s: %d output channels from %d stored ones (C == Cs in {1, 3}, or 3 copies of 1)" %
                         (fn, C, Cs))
    for t, nm in ((store, "store"), (first, "first")):
        if not t.is_cuda:
            raise ValueError("%s: %s is on %s; the kernel needs device tensors (no CPU fallback)" % (fn, nm, t.device))
    if store.device != first.device:
        raise ValueError("%s: store is on %s, first on %s" % (fn, store.device, first.device))
    if B and F < 1:
        raise ValueError("%s: the store holds no frame" % fn)
    chunks = -(-H * W // 1024)
    if H * W > 0x7fffffff // 4 or B * T * chunks > 0x7fffffff:
        raise ValueError("%s: %d clips of %d frames of %dx%d exceed one launch" % (fn, B, T, H, W))
    return store.contiguous(), first.contiguous(), F, H, W, Cs, B, T, C


def clip_gather(store, first, T, C):
    """Clips of a device-resident frame store as one float32 batch (rfn_clip_gather_u8_f32: what the reference's
    PushDataset / KTH __getitem__ and the DataLoader's collation produce, bair_push.py:66-109, kth.py:34-65,
    trainer.py:132-161): a fresh [B, T, C, H, W] tensor on the store's device, clip b being frames first[b] ..
    first[b] + T - 1 as float32(byte) / 255.  `store`: uint8 [F, H, W, Cs] device tensor, Cs in {1, 3}; `first`: int64
    [B] on the same device; C == Cs, or C == 3 copies of a one-channel store.  A clip that would leave the store is
    NaN (nothing is read).  One launch on the current stream; no CPU fallback."""
    store, first, F, H, W, Cs, B, T, C = _clip_gather_args("clip_gather", store, first, T, C)
    out = torch.empty((B, T, C, H, W), device=store.device, dtype=torch.float32)
    if B:
        with torch.cuda.device(store.device):
            L.call("rfn_clip_gather_u8_f32", store.data_ptr(), F, first.data_ptr(), L.dev(out), B, T, C, Cs, H, W,
                   meta=("shell", "clip_gather", 0.0, "%dx%dx%dx%dx%d" % (B, T, C, H, W),
                         4.0 * out.numel() + float(B * T * H * W * Cs)))
    return out


CLIP_MIRROR, CLIP_REVERSE = 1, 2   # the bits of clip_gather_aug's flags


def clip_gather_aug(store, first, T, C, step=1, flags=None):
    """clip_gather with a temporal stride and per-clip augmentations (rfn_clip_gather_aug_u8_f32): clip b is the T
    frames first[b], first[b] + step, ...; `flags`: None, or int32 [B] on the store's device, bit 0 (CLIP_MIRROR)
    mirrors the clip's frames in x, bit 1 (CLIP_REVERSE) reverses its frames in time, other bits are ignored.  A clip
    with first[b] < 0 or first[b] + (T - 1) * step + 1 > F is NaN (nothing is read).  With step 1 and no flags the
    result is clip_gather's bit for bit.  One launch on the current stream; no CPU fallback."""
    store, first, F, H, W, Cs, B, T, C = _clip_gather_args("clip_gather_aug", store, first, T, C)
    if isinstance(step, bool) or not isinstance(step, int) or not 1 <= step <= 0x7fffffff:
        raise ValueError("clip_gather_aug: step must be an int in [1, 2^31), got %r" % (step,))
    if flags is not None:
        if not isinstance(flags, torch.Tensor) or flags.dtype != torch.int32:
            raise TypeError("clip_gather_aug: flags must be an int32 tensor, got %s" %
                            (flags.dtype if isinstance(flags, torch.Tensor) else type(flags).__name__))
        if tuple(flags.shape) != (B,):
            raise ValueError("clip_gather_aug: flags must be [%d], got %s" % (B, tuple(flags.shape)))
        if flags.device != store.device:
            raise ValueError("clip_gather_aug: store is on %s, flags on %s (no CPU fallback)" %
                             (store.device, flags.device))
        flags = flags.contiguous()
    out = torch.empty((B, T, C, H, W), device=store.device, dtype=torch.float32)
    if B:
        with torch.cuda.device(store.device):
            L.call("rfn_clip_gather_aug_u8_f32", store.data_ptr(), F, first.data_ptr(),
                   flags.data_ptr() if flags is not None else None, L.dev(out), B, T, C, Cs, H, W, step,
                   meta=("shell", "clip_gather_aug", 0.0, "%dx%dx%dx%dx%d" % (B, T, C, H, W),
                         4.0 * out.numel() + float(B * T * H * W * Cs)))
    return out


RESIZE_MAX_SIDE = 32768   # rfn_frames_resize_u8's largest source or target side


def resize_window(Hs, Ws, H, W, mode="crop"):
    """the crop window (y0, x0, Hc, Wc) of an Hs x Ws frame for frames_resize to H x W: "stretch" is the whole frame,
    "crop" the largest centred window of the target's aspect ratio (the longer side is cut; integer floor)."""
    Hs, Ws, H, W = int(Hs), int(Ws), int(H), int(W)
    if min(Hs, Ws, H, W) < 1:
        raise ValueError("resize_window: sizes must be >= 1, got %dx%d -> %dx%d" % (Hs, Ws, H, W))
    if mode == "stretch":
        return 0, 0, Hs, Ws
    if mode != "crop":
        raise ValueError("resize_window: mode must be 'crop' or 'stretch', got %r" % (mode,))
    if Ws * H >= Hs * W:
        Hc, Wc = Hs, max(1, Hs * W // H)
    else:
        Hc, Wc = max(1, Ws * H // W), Ws
    return (Hs - Hc) // 2, (Ws - Wc) // 2, Hc, Wc


def frames_resize(src, H, W, Cd, window=None):
    """Frames resampled into another geometry on the GPU (rfn_frames_resize_u8; include/rfn_hip.h states the
    arithmetic): `src` uint8 [F, Hs, Ws, Cs] device tensor, Cs in {1, 3}; returns a fresh uint8 [F, H, W, Cd], Cd in
    {1, 3}, the exact integer area mean (rounded half up) of `window` = (y0, x0, Hc, Wc) of every frame (default: the
    whole frame), then 3 -> 1 channels by the integer luma weights or 1 -> 3 by copies.  One launch on the current
    stream; no CPU fallback."""
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8:
        raise TypeError("frames_resize: src must be a uint8 tensor, got %s" %
                        (src.dtype if isinstance(src, torch.Tensor) else type(src).__name__))
    if src.dim() != 4:
        raise ValueError("frames_resize: src must be [F, Hs, Ws, Cs], got %s" % (tuple(src.shape),))
    F, Hs, Ws, Cs = (int(d) for d in src.shape)
    H, W, Cd = int(H), int(W), int(Cd)
    if not (1 <= Hs <= RESIZE_MAX_SIDE and 1 <= Ws <= RESIZE_MAX_SIDE and 1 <= H <= RESIZE_MAX_SIDE and
            1 <= W <= RESIZE_MAX_SIDE):
        raise ValueError("frames_resize: sides must be in [1, %d], got %dx%d -> %dx%d" % (RESIZE_MAX_SIDE, Hs, Ws, H, W))
    if Cs not in (1, 3) or Cd not in (1, 3):
        raise ValueError("frames_resize: 1 or 3 channels on either side, got %d -> %d" % (Cs, Cd))
    y0, x0, Hc, Wc = (int(v) for v in (window if window is not None else (0, 0, Hs, Ws)))
    if Hc < 1 or Wc < 1 or y0 < 0 or x0 < 0 or y0 + Hc > Hs or x0 + Wc > Ws:
        raise ValueError("frames_resize: the window (y0 %d, x0 %d, %dx%d) is empty or leaves the %dx%d frame" %
                         (y0, x0, Hc, Wc, Hs, Ws))
    if not src.is_cuda:
        raise ValueError("frames_resize: src is on %s; the kernel needs device tensors (no CPU fallback)" % (src.device,))
    bands = -(-H // min(H, max(1, 256 // min(W, 256))))
    if F * bands > 0x7fffffff:
        raise ValueError("frames_resize: %d frames of %dx%d exceed one launch" % (F, H, W))
    src = src.contiguous()
    out = torch.empty((F, H, W, Cd), device=src.device, dtype=torch.uint8)
    if F:
        with torch.cuda.device(src.device):
            L.call("rfn_frames_resize_u8", src.data_ptr(), out.data_ptr(), F, Hs, Ws, Cs, H, W, Cd, y0, x0, Hc, Wc,
                   meta=("shell", "frames_resize", 0.0, "%dx%dx%dx%d>%dx%dx%d" % (F, Hs, Ws, Cs, H, W, Cd),
                         float(F * (Hc * Wc * Cs + H * W * Cd))))
    return out


KEYED_NORMAL_MAX_SLOTS = 8


def keyed_normal_tiled_row(k, r, b, n_draws, B):
    """the row of tile k, draw r (local to the call), sequence b (local to the batch) in a tensor of keyed_normal(...,
    tiles=K): tile-major, then draw-major.  It holds what row r*B + b holds with tiles = 1.  The batch of a
    temperature sweep (RFN.predict_draws(temperatures=...)) has the same layout, k being the temperature."""
    return (k * n_draws + r) * B + b


def keyed_normal(shapes, B, n_draws, seed, step, first_seq=0, first_draw=0, out=None, device=None, tiles=1):
    """Addressed N(0,1) noise (rfn_keyed_normal_f32; include/rfn_hip.h and DESIGN section 16 hold the definition): a list
    of float32 tensors [n_draws*B, *shape_j], slot j being the list position (at most 8).  Row r*B + b of every tensor
    stands for draw first_draw + r of sequence first_seq + b, and a value depends only on (seed, step, slot, sequence,
    draw, position in the row): the same on any grid, for any B, n_draws and split of the draws into calls.  An entry
    None of `shapes` skips that slot (None in the result).  out: tensors to fill in place instead of fresh ones (None
    where the slot is skipped), each contiguous float32 of n_draws*B rows on one device; with out, `shapes` may be None.
    device: where fresh tensors go (default: the current GPU).  One launch on the current stream; no CPU fallback.
    tiles = K > 1 (rfn_keyed_normal_tiled_f32): every tensor has K*n_draws*B rows and row (k*n_draws + r)*B + b holds
    exactly what row r*B + b holds with tiles = 1, for every k (the blocks of a temperature sweep share their noise);
    still one launch.  tiles = 1 is the untiled entry point."""
    B, n_draws, seed, step, first_seq, first_draw = (int(v) for v in (B, n_draws, seed, step, first_seq, first_draw))
    if isinstance(tiles, bool) or not isinstance(tiles, int):
        raise TypeError("keyed_normal: tiles must be an int, got %s" % type(tiles).__name__)
    if tiles < 1:
        raise ValueError("keyed_normal: tiles must be at least 1, got %d" % tiles)
    if B < 1 or n_draws < 0:
        raise ValueError("keyed_normal: need B >= 1 and n_draws >= 0 (got %d, %d)" % (B, n_draws))
    for v, nm in ((seed, "seed"), (first_seq, "first_seq"), (first_draw, "first_draw")):
        if not 0 <= v < 1 << 63:
            raise ValueError("keyed_normal: %s %d not in [0, 2^63)" % (nm, v))
    if not 0 <= step < 1 << 31:
        raise ValueError("keyed_normal: step %d not in [0, 2^31)" % step)
    tile_rows = n_draws * B          # the rows that are computed; every tensor holds them `tiles` times
    rows = tiles * tile_rows
    if rows > 0x7fffffff:
        raise ValueError("keyed_normal: %d rows exceed one launch" % rows)
    if out is None:
        if shapes is None:
            raise TypeError("keyed_normal: give shapes or out")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("rfn_hip kernels need device tensors; keyed_normal was asked for %s (no CPU fallback)" %
                               device)
        out = [None if sh is None else torch.empty((rows,) + tuple(int(d) for d in sh), device=device,
                                                   dtype=torch.float32) for sh in shapes]
    else:
        out = list(out)
        if shapes is not None and len(shapes) != len(out):
            raise ValueError("keyed_normal: %d shapes for %d out tensors" % (len(shapes), len(out)))
        for j, t in enumerate(out):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError("keyed_normal: out[%d] must be a tensor, got %s" % (j, type(t).__name__))
            if t.dim() < 1 or int(t.shape[0]) != rows:
                raise ValueError("keyed_normal: out[%d] must have %d rows, got shape %s" % (j, rows, tuple(t.shape)))
            if shapes is not None and shapes[j] is not None and tuple(t.shape[1:]) != tuple(int(d) for d in shapes[j]):
                raise ValueError("keyed_normal: out[%d] has rows %s, shapes[%d] is %s" %
                                 (j, tuple(t.shape[1:]), j, tuple(shapes[j])))
    if not 1 <= len(out) <= KEYED_NORMAL_MAX_SLOTS:
        raise ValueError("keyed_normal: %d slots, one launch fills 1 to %d" % (len(out), KEYED_NORMAL_MAX_SLOTS))
    live = [t for t in out if t is not None]
    for t in live:
        if t.device != live[0].device:
            raise ValueError("keyed_normal: the tensors are on %s and %s" % (live[0].device, t.device))
    ptrs = (ctypes.c_void_p * len(out))()
    numels = (ctypes.c_int * len(out))()
    total = 0
    for j, t in enumerate(out):
        if t is None or rows == 0:
            continue
        n = t.numel() // rows
        if n > 0x7fffffff:
            raise ValueError("keyed_normal: rows of %d values exceed one launch" % n)
        if n:
            ptrs[j] = L.dev(t, "out[%d]" % j).value
        numels[j] = n
        total += t.numel()
    if total:
        with torch.cuda.device(live[0].device):
            if tiles == 1:
                L.call("rfn_keyed_normal_f32", ptrs, numels, len(out), rows, B, seed, step, first_seq, first_draw,
                       meta=("shell", "keyed_normal", 0.0, "%dx%d" % (rows, total // rows), 4.0 * total))
            else:
                L.call("rfn_keyed_normal_tiled_f32", ptrs, numels, len(out), tile_rows, B, tiles, seed, step, first_seq,
                       first_draw,
                       meta=("shell", "keyed_normal", 0.0, "%dx%dx%d" % (tiles, tile_rows, total // rows), 4.0 * total))
    return out


KEYED_UNIFORM_SLOT_DEQUANT = 24   # the dequantisation noise of RFN.iw_log_weights (keyed_normal: 0 .. 7, mol: 16, 17)


def keyed_uniform(shape, B, n_draws, seed, first_step, n_steps=1, slot=KEYED_UNIFORM_SLOT_DEQUANT, scale=1.0, first_seq=0,
                  first_draw=0, device=None, out=None):
    """Addressed uniform noise in [0, scale) (rfn_keyed_uniform_f32; include/rfn_hip.h and DESIGN section 24 hold the
    definition): a float32 tensor [n_steps, n_draws*B, *shape].  Step-block s stands for step first_step + s, row r*B + b
    of every block for draw first_draw + r of sequence first_seq + b, and a value depends only on (seed, step, slot,
    sequence, draw, position in the row): the same on any grid, for any B, n_draws, n_steps and split into calls.  slot
    in [8, 2^31): keyed_normal owns the slots below.  out: a contiguous float32 tensor of that shape to fill in place
    instead of a fresh one (`shape` may then be None); device: where a fresh tensor goes (default: the current GPU).
    One launch on the current stream for all steps; torch's generators are not touched; no CPU fallback."""
    B, n_draws, seed, first_step, n_steps, first_seq, first_draw = (int(v) for v in (B, n_draws, seed, first_step, n_steps,
                                                                                  first_seq, first_draw))
    if isinstance(slot, bool) or not isinstance(slot, int):
        raise TypeError("keyed_uniform: slot must be an int, got %s" % type(slot).__name__)
    scale = float(scale)
    if B < 1 or n_draws < 0 or n_steps < 0:
        raise ValueError("keyed_uniform: need B >= 1, n_draws >= 0 and n_steps >= 0 (got %d, %d, %d)" %
                         (B, n_draws, n_steps))
    for v, nm in ((seed, "seed"), (first_seq, "first_seq"), (first_draw, "first_draw")):
        if not 0 <= v < 1 << 63:
            raise ValueError("keyed_uniform: %s %d not in [0, 2^63)" % (nm, v))
    if first_step < 0 or first_step + n_steps > 1 << 31:
        raise ValueError("keyed_uniform: steps %d .. %d not in [0, 2^31)" % (first_step, first_step + n_steps - 1))
    if not 8 <= slot < 1 << 31:
        raise ValueError("keyed_uniform: slot %d not in [8, 2^31) (keyed_normal owns slots 0 .. 7)" % slot)
    if not 0.0 < scale < float("inf"):
        raise ValueError("keyed_uniform: scale must be finite and positive, got %r" % scale)
    rows = n_draws * B
    if rows > 0x7fffffff:
        raise ValueError("keyed_uniform: %d rows exceed one launch" % rows)
    if out is None:
        if shape is None:
            raise TypeError("keyed_uniform: give shape or out")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("rfn_hip kernels need device tensors; keyed_uniform was asked for %s (no CPU fallback)" %
                               device)
        out = torch.empty((n_steps, rows) + tuple(int(d) for d in shape), device=device, dtype=torch.float32)
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError("keyed_uniform: out must be a tensor, got %s" % type(out).__name__)
        if out.dim() < 2 or tuple(out.shape[:2]) != (n_steps, rows):
            raise ValueError("keyed_uniform: out must be [%d, %d, ...], got shape %s" % (n_steps, rows, tuple(out.shape)))
        if shape is not None and tuple(out.shape[2:]) != tuple(int(d) for d in shape):
            raise ValueError("keyed_uniform: out has rows %s, shape is %s" % (tuple(out.shape[2:]), tuple(shape)))
    total = out.numel()
    if total:
        numel = total // (n_steps * rows)
        if numel > 0x7fffffff or -(-numel // 8) * rows * n_steps > 0x7fffffff * 256:
            raise ValueError("keyed_uniform: %d steps of %d rows of %d values exceed one launch" % (n_steps, rows, numel))
        ptr = L.dev(out, "out")
        with torch.cuda.device(out.device):
            L.call("rfn_keyed_uniform_f32", ptr, n_steps, rows, B, numel, scale, seed, first_step, slot,
                   first_seq, first_draw,
                   meta=("shell", "keyed_uniform", 0.0, "%dx%dx%d" % (n_steps, rows, numel), 4.0 * total))
    return out


SHEET_MAX_ROWS = L.CONSTANTS["RFN_SHEET_MAX_ROWS"]   # the row descriptors travel in the launch's arguments


def sheet_shape(n_rows, n_cols, H, W, gutter):
    """(Hs, Ws) of a sheet of n_rows x n_cols cells of H x W pixels with `gutter` pixels between and around them"""
    return n_rows * H + (n_rows + 1) * gutter, n_cols * W + (n_cols + 1) * gutter


def compose_sheet(rows, n_cols, gutter=2, bg=255, n_bits=8, preprocess_range="0.5", scanlines=False, out=None):
    """A sheet of frames as 8-bit RGB pixels (rfn_sheet_compose_u8: the subplot grids of the reference's plotter and
    Evaluator.plot_samples, trainer.py:325-417, error_metrics.py:128-152, as pixels only).  `rows`: a list of device
    tensors [n, C, H, W], n <= n_cols, fp32 in model space or uint8, each with dense CHW frames and any stride along n
    (pass views such as image[0] of [B, T, C, H, W] or samples[:, 0] of [T, B, C, H, W]: nothing is copied).  Row r fills
    the first n cells of sheet row r, the rest is background `bg`; cells are `gutter` pixels apart.  fp32 frames become
    bytes exactly as Solver.preprocess(x, reverse=True) with this n_bits / preprocess_range makes them; uint8 frames are
    copied; C == 1 is written to R, G and B.  Returns uint8 [Hs, Ws, 3], or with scanlines=True [Hs, 1 + 3*Ws] whose
    lines start with the PNG filter byte 0 (Utils.png.write_png takes either); `out` (optional) is a contiguous uint8
    tensor of that shape on the rows' device to write into, at any byte address.  One launch on the current stream; no
    CPU fallback."""
    if not isinstance(rows, (list, tuple)) or not rows:
        raise TypeError("compose_sheet: rows must be a non-empty list of tensors, got %s" % type(rows).__name__)
    for r, t in enumerate(rows):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.uint8):
            raise TypeError("compose_sheet: row %d must be a float32 or uint8 tensor, got %s" %
                            (r, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.dim() != 4:
            raise ValueError("compose_sheet: row %d must be [n, C, H, W], got %s" % (r, tuple(t.shape)))
    n_cols, gutter, bg, n_bits = int(n_cols), int(gutter), int(bg), int(n_bits)
    C, H, W = (int(d) for d in rows[0].shape[1:])
    if C not in (1, 3) or H < 1 or W < 1:
        raise ValueError("compose_sheet: frames must be [C in {1, 3}, H >= 1, W >= 1], got %s" % ((C, H, W),))
    for r, t in enumerate(rows):
        if tuple(t.shape[1:]) != (C, H, W):
            raise ValueError("compose_sheet: row %d has frames %s, row 0 has %s" % (r, tuple(t.shape[1:]), (C, H, W)))
        s = t.stride()
        if not ((W == 1 or s[3] == 1) and (H == 1 or s[2] == W) and (C == 1 or s[1] == H * W)):
            raise ValueError("compose_sheet: the frames of row %d must be dense CHW, got shape %s stride %s" %
                             (r, tuple(t.shape), tuple(s)))
    if n_cols < 1 or gutter < 0 or not 0 <= bg <= 255 or not 1 <= n_bits <= 8:
        raise ValueError("compose_sheet: need n_cols >= 1, gutter >= 0, bg in [0, 255], n_bits in [1, 8] (got %d, %d, "
                         "%d, %d)" % (n_cols, gutter, bg, n_bits))
    if len(rows) > SHEET_MAX_ROWS:
        raise ValueError("compose_sheet: %d rows exceed the %d of one launch" % (len(rows), SHEET_MAX_ROWS))
    for r, t in enumerate(rows):
        if int(t.shape[0]) > n_cols:
            raise ValueError("compose_sheet: row %d holds %d frames for %d columns" % (r, int(t.shape[0]), n_cols))
    for r, t in enumerate(rows):
        if not t.is_cuda:
            raise ValueError("compose_sheet: row %d is on %s; the kernel needs device tensors (no CPU fallback)" %
                             (r, t.device))
        if t.device != rows[0].device:
            raise ValueError("compose_sheet: row 0 is on %s, row %d on %s" % (rows[0].device, r, t.device))
    Hs, Ws = sheet_shape(len(rows), n_cols, H, W, gutter)
    if Hs > 0x7fffffff or 3 * Ws + 1 > 0x7fffffff or C * H * W > 0x7fffffff:
        raise ValueError("compose_sheet: a %dx%d sheet of %dx%dx%d frames exceeds one launch" % (Hs, Ws, C, H, W))
    tab = (L.rfn_sheet_row * len(rows))()
    for r, t in enumerate(rows):
        n = int(t.shape[0])
        tab[r].ptr = t.data_ptr() if n else None
        tab[r].step = int(t.stride(0)) if n > 1 else 0
        tab[r].kind = 1 if t.dtype == torch.uint8 else 0
        tab[r].count = n
    dev = rows[0].device
    shape = (Hs, 1 + 3 * Ws) if scanlines else (Hs, Ws, 3)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or
          not out.is_contiguous() or out.device != dev):
        raise ValueError("compose_sheet: out must be a contiguous uint8 tensor %s on %s" % (shape, dev))
    with torch.cuda.device(dev):
        L.call("rfn_sheet_compose_u8", tab, len(rows), n_cols, C, H, W, gutter, bg, n_bits,
               1 if preprocess_range == "0.5" else 0, 1 if scanlines else 0, out.data_ptr(),
               meta=("shell", "sheet_compose", 0.0, "%dx%dx%dx%dx%d" % (len(rows), n_cols, C, H, W),
                     float(out.numel()) + sum(float(t.numel() * t.element_size()) for t in rows)))
    return out


def chart_chunk():
    """records one workgroup of the chart kernel culls at a time (rfn_chart_chunk); the picture does not depend on it"""
    return int(L.load().rfn_chart_chunk())


def chart_font():
    """the kernel's built-in 5x7 font (rfn_chart_font): int32 numpy [95, 5], row ch = character 32 + ch, one entry per
    column from the left, bit r = the dot in row r from the top"""
    import numpy as np
    buf = (ctypes.c_longlong * (95 * 5))()
    rc = L.load().rfn_chart_font(ctypes.cast(buf, ctypes.c_void_p))
    if rc != 0:
        raise RuntimeError("rfn_chart_font failed (code %d)" % rc)
    return np.frombuffer(buf, dtype=np.int64).astype(np.int32).reshape(95, 5)


def render_chart(chart, H=None, W=None, scanlines=False, out=None, bg=(255, 255, 255), device=None):
    """A line chart as 8-bit RGB pixels (rfn_chart_render_u8; the pixel contract is DESIGN.md section 25).  `chart`: a
    rfn_hip.chart.Figure or DisplayList (H, W and bg come from it; a given H / W must agree), or a display-list table
    int32 [n, 12] -- a numpy array or CPU tensor, checked against the contract's coordinate bounds and uploaded, or a
    contiguous device tensor, taken as it is -- painted on an H x W canvas of colour `bg` (r, g, b).  Returns uint8
    [H, W, 3], or with scanlines=True [H, 1 + 3*W] whose lines start with the PNG filter byte 0 (Utils.png.write_png
    takes either); `out` (optional) is a contiguous uint8 device tensor of that shape, at any byte address.  The device
    is that of `out`, of a device table, `device`, or the current one.  One launch on the current stream; no CPU
    fallback."""
    import numpy as np
    from . import chart as C
    if isinstance(chart, C.Figure):
        chart = C.build_display_list(chart)
    if isinstance(chart, C.DisplayList):
        if (H is not None and int(H) != chart.height) or (W is not None and int(W) != chart.width):
            raise ValueError("render_chart: the figure is %dx%d, H x W = %sx%s was asked for" %
                             (chart.height, chart.width, H, W))
        H, W, bg, table = chart.height, chart.width, chart.bg, chart.table
    else:
        table = chart
    if H is None or W is None:
        raise TypeError("render_chart: a table needs the canvas size H, W")
    H, W = int(H), int(W)
    if not (1 <= H <= C.MAX_SIDE and 1 <= W <= C.MAX_SIDE):
        raise ValueError("render_chart: the canvas is at most %d x %d pixels, got %d x %d" %
                         (C.MAX_SIDE, C.MAX_SIDE, H, W))
    bg = tuple(int(c) for c in bg)
    if len(bg) != 3 or not all(0 <= c <= 255 for c in bg):
        raise ValueError("render_chart: bg must be three bytes (r, g, b), got %s" % (bg,))
    on_device = isinstance(table, torch.Tensor) and table.is_cuda
    if on_device:
        if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != C.REC or not table.is_contiguous():
            raise ValueError("render_chart: a device table must be contiguous int32 [n, %d], got %s %s" %
                             (C.REC, table.dtype, tuple(table.shape)))
    elif isinstance(table, (torch.Tensor, np.ndarray)):
        table = C.check_table(table.numpy() if isinstance(table, torch.Tensor) else table)
    else:
        raise TypeError("render_chart: need a chart.Figure, a chart.DisplayList or an int32 [n, %d] table, got %s" %
                        (C.REC, type(chart).__name__))
    shape = (H, 1 + 3 * W) if scanlines else (H, W, 3)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or
                            tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda):
        raise ValueError("render_chart: out must be a contiguous uint8 device tensor %s" % (shape,))
    if out is not None:
        dev = out.device
    elif on_device:
        dev = table.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("render_chart: the chart kernel needs a GPU (no CPU fallback)")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("render_chart: the chart kernel needs a GPU, got device %s (no CPU fallback)" % dev)
    if on_device and table.device != dev:
        raise ValueError("render_chart: the table is on %s, out on %s" % (table.device, dev))
    if not on_device:
        table = torch.from_numpy(table).to(dev)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    n = int(table.shape[0])
    with torch.cuda.device(dev):
        L.call("rfn_chart_render_u8", table.data_ptr() if n else None, n, H, W, bg[0] | bg[1] << 8 | bg[2] << 16,
               1 if scanlines else 0, out.data_ptr(),
               meta=("shell", "chart_render", 0.0, "%dx%dx%d" % (n, H, W), float(out.numel()) + 48.0 * n))
    return out


# LPIPS with the AlexNet trunk (rfn_hip/lpips.py holds the loader and the wrappers of csrc/lpips.hip)
from .lpips import (LpipsAlexWeights, LpipsFeatures, lpips_alex, lpips_alex_distance, lpips_alex_features,  # noqa: E402,F401
                    lpips_alex_load, lpips_alex_pack, lpips_alex_sizes)

# Frechet Video Distance: the I3D trunk and the Frechet distance (rfn_hip/i3d.py holds the layer table, the loader and the
# wrappers of csrc/i3d.hip)
from .i3d import (I3DWeights, frechet_distance, i3d_embed, i3d_head, i3d_inception, i3d_load, i3d_logits,  # noqa: E402,F401
                  i3d_maxpool, i3d_pack, i3d_preprocess, i3d_same, i3d_sizes, i3d_unit)
