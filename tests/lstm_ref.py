"""Float64 restatement of the LSTM cell's DEFINITION (include/rfn_hip.h, rfn_lstm_cell_{fwd,bwd}_f32), forward and
backward, written from that paragraph with explicit sums and formulas: no autograd, no nn.LSTMCell.  The yardstick of
tests/test_lstm_cell.py; tests/test_lstm_cell_host.py holds it against torch.nn.LSTMCell in float64."""
import torch

NAMES = ("x", "h", "c", "w_ih", "w_hh", "b_ih", "b_hh")


def forward64(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """{"h_out", "c_out", "gates" [B, 4H] = (i | f | g | o), "A" [B, H]}; A[b, j] is the largest over the four gates of
    sum_k |x w_ih| + sum_k |h w_hh| + |b_ih| + |b_hh|, the scale of the pre-activations' round-off"""
    x, h, c, w_ih, w_hh, b_ih, b_hh = [t.double() for t in (x, h, c, w_ih, w_hh, b_ih, b_hh)]
    B, H = h.shape
    pre = (x[:, None, :] * w_ih[None, :, :]).sum(-1) + (h[:, None, :] * w_hh[None, :, :]).sum(-1) + b_ih + b_hh
    mag = ((x[:, None, :] * w_ih[None, :, :]).abs().sum(-1) + (h[:, None, :] * w_hh[None, :, :]).abs().sum(-1)
           + b_ih.abs() + b_hh.abs())
    i, f, o = [1.0 / (1.0 + torch.exp(-pre[:, g * H:(g + 1) * H])) for g in (0, 1, 3)]
    g = torch.tanh(pre[:, 2 * H:3 * H])
    c_out = f * c + i * g
    return {"h_out": o * torch.tanh(c_out), "c_out": c_out, "gates": torch.cat([i, f, g, o], 1),
            "A": mag.view(B, 4, H).max(1).values}


def backward64(fw, gh, gc, x, h, c, w_ih, w_hh):
    """the gradients of the definition from the forward's values `fw`; gh / gc None = zero.  Also the sums of absolute
    terms of every matrix product and of the bias gradient ("abs_<name>")"""
    x, h, c, w_ih, w_hh = [t.double() for t in (x, h, c, w_ih, w_hh)]
    B, H = h.shape
    gh = torch.zeros_like(h) if gh is None else gh.double()
    gc = torch.zeros_like(h) if gc is None else gc.double()
    i, f, g, o = [fw["gates"][:, k * H:(k + 1) * H] for k in range(4)]
    t = torch.tanh(fw["c_out"])
    gct = gc + gh * o * (1 - t * t)
    D = torch.cat([gct * g * i * (1 - i), gct * c * f * (1 - f), gct * i * (1 - g * g), gh * t * o * (1 - o)], 1)
    aD = D.abs()
    return {"D": D, "g_c": gct * f, "g_bias": D.sum(0), "g_x": D @ w_ih, "g_h": D @ w_hh, "g_w_ih": D.t() @ x,
            "g_w_hh": D.t() @ h, "abs_g_bias": aD.sum(0), "abs_g_x": aD @ w_ih.abs(), "abs_g_h": aD @ w_hh.abs(),
            "abs_g_w_ih": aD.t() @ x.abs(), "abs_g_w_hh": aD.t() @ h.abs()}


def make_inputs(B, I, H, w_scale, seed=0):
    """float32 CPU inputs: x, h ~ N(0, 1), c ~ N(0, 1), weights and biases ~ N(0, w_scale^2)"""
    g = torch.Generator().manual_seed(seed + 1000003 * B + 1009 * I + H)
    return {"x": torch.randn(B, I, generator=g), "h": torch.randn(B, H, generator=g), "c": torch.randn(B, H, generator=g),
            "w_ih": torch.randn(4 * H, I, generator=g) * w_scale, "w_hh": torch.randn(4 * H, H, generator=g) * w_scale,
            "b_ih": torch.randn(4 * H, generator=g) * w_scale, "b_hh": torch.randn(4 * H, generator=g) * w_scale}
