"""Host side of the LSTM cell (csrc/lstm_cell.hip, rfn_hip.ops.lstm_cell): the float64 restatement of tests/lstm_ref.py
against torch.nn.LSTMCell with autograd in float64 (the yardstick of the GPU tests is checked here, without a device), the
argument checks of rfn_hip.ops.lstm_cell_check, the declarations of both entry points and what the binding derives from
them, and the torch route on CPU tensors."""
import ctypes
import os

import pytest
import torch

from tests import lstm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 5, 7), (4, 16, 16)]
GRADS = ("g_x", "g_h", "g_c", "g_w_ih", "g_w_hh", "g_bias")


def module64(v):
    H, I = v["w_hh"].shape[1], v["w_ih"].shape[1]
    m = torch.nn.LSTMCell(I, H).double()
    with torch.no_grad():
        for n, k in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            getattr(m, n).copy_(v[k].double())
    return m


def autograd64(v, gh, gc):
    """(h', c', gradients) of nn.LSTMCell in float64 for the upstreams gh, gc (None = not used)"""
    m = module64(v)
    x, h, c = [v[n].double().requires_grad_(True) for n in ("x", "h", "c")]
    h_out, c_out = m(x, (h, c))
    total = sum((o * u.double()).sum() for o, u in ((h_out, gh), (c_out, gc)) if u is not None)
    gs = torch.autograd.grad(total, [x, h, c, m.weight_ih, m.weight_hh, m.bias_ih, m.bias_hh])
    assert torch.equal(gs[5], gs[6])
    return h_out.detach(), c_out.detach(), dict(zip(GRADS, gs[:6]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ups", ["both", "gh", "gc"])
def test_restatement_equals_nn_lstmcell_in_float64(shape, ups):
    B, I, H = shape
    v = R.make_inputs(B, I, H, H ** -0.5)
    g = torch.Generator().manual_seed(5)
    gh = torch.randn(B, H, generator=g) if ups != "gc" else None
    gc = torch.randn(B, H, generator=g) if ups != "gh" else None
    fw = R.forward64(*[v[n] for n in R.NAMES])
    bw = R.backward64(fw, gh, gc, v["x"], v["h"], v["c"], v["w_ih"], v["w_hh"])
    h_out, c_out, grads = autograd64(v, gh, gc)
    assert float((fw["h_out"] - h_out).abs().max()) <= 1e-12
    assert float((fw["c_out"] - c_out).abs().max()) <= 1e-12
    for n in GRADS:
        assert bw[n].shape == grads[n].shape, n
        assert float((bw[n] - grads[n]).abs().max()) <= 1e-12 * max(1.0, float(grads[n].abs().max())), n
    assert fw["gates"].shape == (B, 4 * H) and fw["A"].shape == (B, H) and bw["D"].shape == (B, 4 * H)
    assert bool((fw["A"] > 0).all())


def test_lstm_cell_check_refusals():
    from rfn_hip import ops
    v = R.make_inputs(3, 5, 7, 0.3)
    a = [v[n] for n in R.NAMES]
    assert ops.lstm_cell_check(*a) == (3, 5, 7)

    def bad(i, t, match):
        b = list(a)
        b[i] = t
        with pytest.raises(ValueError, match=match):
            ops.lstm_cell_check(*b)
        with pytest.raises(ValueError, match=match):
            ops.lstm_cell(*b)
    bad(1, torch.zeros(2, 7), "h has shape")
    bad(2, torch.zeros(3, 6), "c has shape")
    bad(3, torch.zeros(28, 4), "w_ih has shape")
    bad(3, torch.zeros(24, 5), "w_ih has shape")        # 4H of another H
    bad(4, torch.zeros(28, 5), "w_hh has shape")
    bad(5, torch.zeros(27), "b_ih has shape")
    bad(6, torch.zeros(28, 1), "b_hh has shape")
    bad(0, torch.zeros(3, 5, 1), r"\[B, I\]")
    bad(0, torch.zeros(0, 5), r"B, I, H >= 1")
    bad(0, v["x"].double(), "one dtype")
    bad(4, v["w_hh"].half(), "one dtype")
    bad(0, torch.zeros(3, 5, dtype=torch.int32), "float32")
    bad(0, torch.zeros(5, 3).t(), "contiguous")
    bad(3, torch.zeros(5, 28).t(), "contiguous")
    bad(2, None, "must be a tensor")
    with pytest.raises(ValueError, match="route"):
        ops.lstm_cell(*a, route="fast")
    # the kernel route has no CPU path behind it
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lstm_cell(*a, route="kernel")


def test_header_declares_both_entry_points_and_the_binding_derives_them():
    from rfn_hip import lib
    with open(os.path.join(ROOT, "include", "rfn_hip.h")) as f:
        text = f.read()
    sigs, res, _ = lib.parse_header(text)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert sigs["rfn_lstm_cell_fwd_f32"] == [P] * 10 + [I, I, I, P]
    assert sigs["rfn_lstm_cell_bwd_f32"] == [P] * 8 + [I, I, P]
    assert res["rfn_lstm_cell_fwd_f32"] is I and res["rfn_lstm_cell_bwd_f32"] is I
    assert "rfn_lstm_cell_fwd_f32(const float* x, const float* h, const float* c, const float* w_ih" in text
    assert "rfn_lstm_cell_bwd_f32(const float* gh, const float* gc, const float* gates" in text
    with open(os.path.join(ROOT, "recurrent-flows-msc_amd", "csrc", "Makefile")) as f:
        assert "lstm_cell.hip" in f.read()
    if os.path.exists(lib.HEADER_PATH):      # a built tree: the copy the loader reads says the same
        assert lib.SIGNATURES["rfn_lstm_cell_fwd_f32"] == sigs["rfn_lstm_cell_fwd_f32"]
        assert lib.SIGNATURES["rfn_lstm_cell_bwd_f32"] == sigs["rfn_lstm_cell_bwd_f32"]


def test_route(monkeypatch):
    from rfn_hip import ops
    x = torch.zeros(2, 3)
    for env in (None, "0", "1"):
        if env is None:
            monkeypatch.delenv("RFN_LSTM_CELL", raising=False)
        else:
            monkeypatch.setenv("RFN_LSTM_CELL", env)
        assert ops.lstm_cell_route(x) == "torch"                # CPU tensors always
    assert isinstance(ops.LSTM_CELL_KERNEL_DEFAULT, bool)


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_route_on_cpu_tensors(shape, monkeypatch):
    from rfn_hip import ops
    monkeypatch.setenv("RFN_LSTM_CELL", "1")                     # CPU tensors take the torch route all the same
    B, I, H = shape
    v = R.make_inputs(B, I, H, H ** -0.5)
    g = torch.Generator().manual_seed(6)
    gh, gc = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    fw = R.forward64(*[v[n] for n in R.NAMES])
    bw = R.backward64(fw, gh, gc, v["x"], v["h"], v["c"], v["w_ih"], v["w_hh"])
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-5)):
        leaves = [v[n].to(dtype).requires_grad_(True) for n in R.NAMES]
        h_out, c_out = ops.lstm_cell(*leaves)
        assert h_out.dtype == dtype and h_out.shape == (B, H)
        assert float((h_out.detach().double() - fw["h_out"]).abs().max()) <= tol
        assert float((c_out.detach().double() - fw["c_out"]).abs().max()) <= tol
        gs = torch.autograd.grad((h_out * gh.to(dtype)).sum() + (c_out * gc.to(dtype)).sum(), leaves)
        for n, got in zip(("g_x", "g_h", "g_c", "g_w_ih", "g_w_hh", "g_bias", "g_bias"), gs):
            assert float((got.double() - bw[n]).abs().max()) <= tol * max(1.0, float(bw[n].abs().max())), n
    # and it is what nn.LSTMCell computes
    m = module64(v).float()
    with torch.no_grad():
        want = m(v["x"], (v["h"], v["c"]))
        got = ops.lstm_cell(*[v[n] for n in R.NAMES])
    assert float((got[0] - want[0]).abs().max()) <= 2e-6 and float((got[1] - want[1]).abs().max()) <= 2e-6
