"""torch.nn.LSTMCell in one kernel each way: wrappers of csrc/lstm_cell.hip.  rfn_hip.ops re-exports the public names."""
import os

import torch

from . import lib as L
from .args import shell


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
               B, I, H, meta=shell("lstm_cell_fwd", gates, 4))
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
               L.dev(g_c), L.dev(g_bias), B, H, meta=shell("lstm_cell_bwd", gates, 3))
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
