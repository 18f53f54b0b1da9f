"""GPU parity of the drop-in modules (Flow.*, Utils.ConvLSTM, RFN.loss) against the golden vectors produced by the
reference (tests/golden/*.pt) and against the CPU oracle.  Calls go through the C ABI (ctypes -> librfn_hip.so)."""
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["mixed", "bf16x3", "f32"], autouse=True)
def conv_precision(request):
    """every test runs with the three arithmetics of the convolutions (RFN_CONV_PRECISION): the shipped 'mixed' path
    (forward fp32-grade: fused f16x3s kernel / fp32 MFMA, gradients bf16x3), all-bf16x3 and all-fp32-MFMA."""
    from rfn_hip import ops
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = request.param
    yield request.param
    ops.CONV_PRECISION = old

from oracle import rfn_oracle as O  # noqa: E402


def cu(t):
    return t.cuda()


def close(a, b, rtol=1e-4, atol=1e-5):
    """element-wise |a-b| <= atol' + rtol*|b| with atol' scaled by the tensor's magnitude: fp32 results of different
    summation orders (MFMA k-order vs CPU conv) agree norm-wise, not element-wise next to zero crossings or after
    exp() amplification."""
    b = b.float()
    scale = float(b.abs().max()) if b.numel() else 0.0
    torch.testing.assert_close(a.detach().cpu(), b, rtol=rtol, atol=atol + rtol * scale)


def nll_rel(a, b, rtol=1e-4):
    """north_star's budget on a log-likelihood: |a - b| <= 1e-4 |b| per sample (relative only, no absolute slack)"""
    a, b = a.detach().cpu().double(), b.double()
    assert bool(((a - b).abs() <= rtol * b.abs()).all()), ((a - b).abs() / b.abs()).max()


def load_sd(m, sd):
    m.load_state_dict({k: (v.float() if v.dtype == torch.float16 else v) for k, v in sd.items()}, strict=True)
    return m.cuda()


def grads_close(m, grads, rtol=2e-3, atol_scale=2e-4):
    named = dict(m.named_parameters())
    for k, g in grads.items():
        got = named[k].grad
        got = torch.zeros_like(g) if got is None else got.detach().cpu()
        torch.testing.assert_close(got, g, rtol=rtol, atol=atol_scale * float(g.abs().max()) + 1e-6, msg=lambda s: k + ": " + s)


def test_actnorm_init(golden):
    from Flow import ActNorm
    f = golden("modules.pt")["actnorm_init"]
    an = ActNorm(5).cuda().train()
    y, ld = an(cu(f["x"]), torch.zeros(3, device="cuda"), reverse=False)
    close(an.bias, f["sd"]["bias"], 1e-5, 1e-6)
    close(an.logs, f["sd"]["logs"], 1e-5, 1e-6)
    assert int(an.initialized) == 1
    close(y, f["y"], 1e-5, 1e-5)
    close(ld, f["logdet"], 1e-5, 1e-5)
    xb, ldb = an(y.detach(), torch.zeros(3, device="cuda"), reverse=True)
    close(xb, f["x_back"], 1e-5, 1e-5)
    close(ldb, f["logdet_back"], 1e-5, 1e-5)


@pytest.mark.parametrize("C", [4, 8])
def test_invconv(golden, C):
    from Flow import InvConv
    f = golden("modules.pt")["invconv_lu_%d" % C]
    ic = load_sd(InvConv(C, True), f["sd"])
    w, dld = ic.get_weight(cu(f["x"]), False)
    close(w, f["weight"], 1e-5, 1e-6)
    x = cu(f["x"]).requires_grad_(True)
    z, ld = ic(x, torch.zeros(2, device="cuda"), False)
    close(z, f["z"], 1e-5, 1e-5)
    close(ld, f["logdet"], 1e-5, 1e-5)
    (z.square().sum() + ld.sum()).backward()
    close(x.grad, f["grad_x"], 1e-4, 1e-5)
    grads_close(ic, f["grads"])
    xb, ldb = ic(cu(f["z"]), torch.zeros(2, device="cuda"), True)
    close(xb, f["x_back"], 1e-4, 1e-4)
    close(ldb, f["logdet_back"], 1e-5, 1e-5)


def test_conv2dnorm_zeros(golden):
    from Flow import Conv2dNorm, Conv2dZeros
    m = golden("modules.pt")
    f = m["conv2dnorm"]
    cn = load_sd(Conv2dNorm(5, 7), f["sd"]).train()
    close(cn(cu(f["x"])), f["y"], 1e-5, 1e-5)
    cn0 = Conv2dNorm(5, 7).cuda().train()
    with torch.no_grad():
        cn0.conv.weight.copy_(f["sd"]["conv.weight"])
    close(cn0(cu(f["x"])), f["y_first"], 1e-4, 1e-5)
    close(cn0.norm_type.logs, f["sd"]["norm_type.logs"], 1e-4, 1e-5)
    f = m["conv2dnorm_1x1"]
    cn1 = Conv2dNorm(5, 7, kernel_size=[1, 1]).cuda().train()
    with torch.no_grad():
        cn1.conv.weight.copy_(f["sd"]["conv.weight"])
    close(cn1(cu(f["x"])), f["y"], 1e-4, 1e-5)
    f = m["conv2dzeros"]
    cz = load_sd(Conv2dZeros(5, 6), f["sd"])
    close(cz(cu(f["x"])), f["y"], 1e-5, 1e-5)


@pytest.mark.parametrize("clamp", ["realnvp", "glow", "softclamp", "none"])
@pytest.mark.parametrize("non_lin", ["relu", "leakyrelu"])
def test_affine_coupling(golden, clamp, non_lin, conv_precision):
    from Flow import AffineCoupling
    f = golden("modules.pt")["affine_%s_%s" % (clamp, non_lin)]
    # The fixture perturbs every parameter by N(0, 0.1): with the unbounded clamps (glow / softclamp / none, not the
    # reference's default) exp(log_scale) reaches 1e7 and multiplies any error of the coupling net by |log_scale|.
    # The split-precision convs (1e-5 relative) are therefore checked at 30x the fp32 tolerance there.
    k = 30.0 if (conv_precision == "bf16x3" and clamp != "realnvp") else 1.0
    ac = load_sd(AffineCoupling([2, 6, 4, 4], [2, 5, 4, 4], 16, non_lin, clamp), f["sd"]).train()
    x = cu(f["x"]).requires_grad_(True)
    c = cu(f["cond"]).requires_grad_(True)
    y, ld = ac(x, c, torch.zeros(2, device="cuda"), False)
    close(y, f["y"], 1e-5 * k, 1e-5)
    close(ld, f["logdet"], 1e-4, 1e-5)
    ((y * cu(f["wgt"])).sum() + (ld * cu(f["gld"])).sum()).backward()
    close(x.grad, f["grad_x"], 1e-4 * k, 1e-5)
    close(c.grad, f["grad_cond"], 1e-4 * k, 1e-5)
    grads_close(ac, f["grads"], 2e-3 * k, 2e-4 * k)
    xb, ldb = ac(cu(f["y"]), cu(f["cond"]), torch.zeros(2, device="cuda"), True)
    close(xb, f["x_back"], 1e-4 * k, 1e-5)
    close(ldb, f["logdet_back"], 1e-4, 1e-5)


@pytest.mark.parametrize("cond_on", [True, False])
@pytest.mark.parametrize("clampf", ["softplus", "exp"])
def test_split2d(golden, cond_on, clampf):
    from Flow import Split2d
    f = golden("modules.pt")["split2d_%s_%s" % ("cond" if cond_on else "uncond", clampf)]
    sp = load_sd(Split2d([2, 8, 4, 4], [2, 6, 4, 4], cond_on, clampf), f["sd"]).train()
    x = cu(f["x"]).requires_grad_(True)
    c = cu(f["cond"]).requires_grad_(True)
    z1, ld = sp(x, c, torch.zeros(2, device="cuda"), False)
    assert torch.equal(z1.detach().cpu(), f["z1"])
    close(ld, f["logdet"], 1e-4, 1e-5)
    ((z1 * cu(f["wgt"])).sum() + (ld * cu(f["gld"])).sum()).backward()
    close(x.grad, f["grad_x"], 1e-4, 1e-5)
    if cond_on:
        close(c.grad, f["grad_cond"], 1e-4, 1e-5)
    grads_close(sp, f["grads"])


def glow_ns(d):
    return Namespace(**d)


def test_glowstep(golden):
    from Flow import GlowStep
    from tests.golden_args import GLOW_DEFAULTS
    f = golden("glow.pt")["glowstep"]
    gs = load_sd(GlowStep([2, 8, 4, 4], [2, 6, 4, 4], glow_ns(GLOW_DEFAULTS)), f["sd"]).train()
    x = cu(f["x"]).requires_grad_(True)
    c = cu(f["cond"]).requires_grad_(True)
    y, ld = gs(x, c, torch.zeros(2, device="cuda"), False)
    close(y, f["y"], 1e-5, 1e-5)
    close(ld, f["logdet"], 1e-4, 1e-5)
    ((y * cu(f["wgt"])).sum() + (ld * cu(f["gld"])).sum()).backward()
    close(x.grad, f["grad_x"], 1e-4, 1e-5)
    close(c.grad, f["grad_cond"], 1e-4, 1e-5)
    grads_close(gs, f["grads"])
    xb, ldb = gs(cu(f["y"]), cu(f["cond"]), torch.zeros(2, device="cuda"), True)
    close(xb, f["x_back"], 1e-4, 1e-5)
    close(ldb, f["logdet_back"], 1e-4, 1e-5)


def test_glowstep_canonical_level0(golden):
    from Flow import GlowStep
    from tests.golden_args import GLOW_DEFAULTS
    f = golden("glowstep_canonical_l0.pt")
    a = dict(GLOW_DEFAULTS)
    a["n_units_affine"] = 256
    gs = load_sd(GlowStep([1, 4, 32, 32], [1, 16, 32, 32], glow_ns(a)), f["sd"]).train()
    x = cu(f["x"]).requires_grad_(True)
    c = cu(f["cond"]).requires_grad_(True)
    y, ld = gs(x, c, torch.zeros(1, device="cuda"), False)
    close(y, f["y"], 1e-4, 1e-4)
    close(ld, f["logdet"], 1e-4, 1e-4)
    # backward at the canonical width (Hd = 256, one 32x32 frame: the fused forward / backward kernels of the shallow
    # levels in 'mixed') against the oracle's autograd on the same weights -- the fixture pins the oracle's forward
    g = torch.Generator().manual_seed(5)
    wgt, gld = torch.randn(1, 4, 32, 32, generator=g), torch.randn(1, generator=g)
    ((y * cu(wgt)).sum() + (ld * cu(gld)).sum()).backward()
    sd = {k: (v.float() if v.dtype == torch.float16 else v).clone() for k, v in f["sd"].items()}
    for k, v in sd.items():
        if v.is_floating_point() and "initialized" not in k and k.split(".")[-1] not in ("p", "sign_s"):
            v.requires_grad_(True)
    xo, co = f["x"].clone().requires_grad_(True), f["cond"].clone().requires_grad_(True)
    yo, ldo = O.glowstep(sd, "", xo, co, torch.zeros(1), False, True, a["non_lin_glow"], a["clamp_type"])
    ((yo * wgt).sum() + (ldo * gld).sum()).backward()
    rel = lambda a_, b_: float((a_.detach().cpu() - b_).norm() / (b_.norm() + 1e-30))
    assert rel(x.grad, xo.grad) <= 5e-3 and rel(c.grad, co.grad) <= 5e-3
    named = dict(gs.named_parameters())
    n_checked = 0
    for k, v in sd.items():
        if v.requires_grad and v.grad is not None and k in named and named[k].grad is not None and float(v.grad.norm()) > 1e-12:
            assert rel(named[k].grad, v.grad) <= 5e-3, (k, rel(named[k].grad, v.grad))
            n_checked += 1
    assert n_checked >= 12


@pytest.mark.parametrize("name", ["listglow_L2K2", "listglow_L3K2_rgb_leaky_glowclamp", "listglow_uncond"])
def test_listglow(golden, name):
    from Flow import ListGlow
    f = golden("glow.pt")[name]
    args = glow_ns(f["args"])
    # (i) first training call: data dependent init
    flow = load_sd(ListGlow(f["x_size"], f["cond_sizes"], tuple(f["base_size"]), args), f["sd_fresh"]).train()
    z, nll = flow.log_prob(cu(f["x"]), [cu(c) for c in f["conds"]], cu(f["base_cond"]), 0, noise=cu(f["noise_init"]))
    close(z, f["z_init"], 1e-4, 1e-4)
    nll_rel(nll, f["nll_init"])
    sd_now = flow.state_dict()
    for k, v in f["sd_init"].items():
        if v.is_floating_point():
            close(sd_now[k], v, 1e-4, 1e-5)
        else:
            assert torch.equal(sd_now[k].cpu(), v), k
    # (ii) steady state + gradients
    flow = load_sd(ListGlow(f["x_size"], f["cond_sizes"], tuple(f["base_size"]), args), f["sd"]).train()
    conds = [cu(c).requires_grad_(True) for c in f["conds2"]]
    bc = cu(f["base_cond2"]).requires_grad_(True)
    z, nll = flow.log_prob(cu(f["x2"]), conds, bc, 0, noise=cu(f["noise2"]))
    close(z, f["z2"], 1e-4, 1e-4)
    nll_rel(nll, f["nll2"])
    nll.mean().backward()
    grads_close(flow, f["grads"], 3e-3, 3e-4)
    for c, g in zip(conds, f["grad_conds2"]):
        if c.numel():
            close(c.grad, g, 1e-3, 1e-5)
    if f["args"]["learn_prior"]:
        close(bc.grad, f["grad_base_cond2"], 1e-3, 1e-5)
    # (iii) reverse path with pinned draws
    flow.eval()
    xs = flow.sample(cu(f["z2"]), [cu(c) for c in f["conds2"]], cu(f["base_cond2"]), temperature=0.8,
                     eps_list=[cu(e) for e in f["sample_draws"]])
    close(xs, f["sample_from_z2"], 1e-3, 1e-4)


def test_listglow_time_batching_equals_per_step_calls(golden):
    """the driver's time-batched call (N = several 'timesteps' of B frames) == separate calls, frame by frame"""
    from Flow import ListGlow
    f = golden("glow.pt")["listglow_L2K2"]
    flow = load_sd(ListGlow(f["x_size"], f["cond_sizes"], tuple(f["base_size"]), glow_ns(f["args"])), f["sd"]).eval()
    g = torch.Generator().manual_seed(9)
    B, reps = f["x_size"][0], 3
    xs = [torch.rand(f["x_size"], generator=g) - 0.5 for _ in range(reps)]
    cs = [[torch.randn(c, generator=g) for c in f["cond_sizes"]] for _ in range(reps)]
    bs = [torch.randn(f["base_size"], generator=g) for _ in range(reps)]
    ns = [torch.rand(f["x_size"], generator=g) / 256 for _ in range(reps)]
    with torch.no_grad():
        sep = [flow.log_prob(cu(xs[i]), [cu(c) for c in cs[i]], cu(bs[i]), 0, noise=cu(ns[i]))[1] for i in range(reps)]
        allc = [torch.cat([cs[i][l] for i in range(reps)]) for l in range(len(f["cond_sizes"]))]
        tog = flow.log_prob(cu(torch.cat(xs)), [cu(c) for c in allc], cu(torch.cat(bs)), 0, noise=cu(torch.cat(ns)))[1]
    assert torch.equal(torch.cat(sep).cpu(), tog.cpu())


@pytest.mark.parametrize("name", ["small", "seq3_4x4", "sibling_8x8"])
def test_convlstm(golden, name):
    from Utils import ConvLSTM
    f = golden("convlstm.pt")[name]
    cin, hc, H, W, B, S = f["cfg"]
    m = load_sd(ConvLSTM(cin, hc, [3, 3], bias=True, peephole=True), f["sd"])
    x = cu(f["x"]).requires_grad_(True)
    h0 = cu(f["h0"]).requires_grad_(True)
    c0 = cu(f["c0"]).requires_grad_(True)
    out, ht, ct = m(x, h0, c0)
    close(out, f["out"], 1e-5, 1e-6)
    close(ht, f["ht"], 1e-5, 1e-6)
    close(ct, f["ct"], 1e-5, 1e-6)
    ((ht * cu(f["wh"])).sum() + (ct * cu(f["wc"])).sum() + out.sum() * 0.1).backward()
    close(x.grad, f["grad_x"], 1e-4, 1e-6)
    close(h0.grad, f["grad_h0"], 1e-4, 1e-6)
    close(c0.grad, f["grad_c0"], 1e-4, 1e-6)
    grads_close(m, {k: v for k, v in f["grads"].items() if "Wc" not in k}, 1e-3, 1e-4)
    _, htn, ctn = m(cu(f["x"]), None, None)
    close(htn, f["ht_none"], 1e-5, 1e-6)
    close(ctn, f["ct_none"], 1e-5, 1e-6)


@pytest.mark.parametrize("who,cin,hc", [("SRNN lstm_h", 256, 60), ("SRNN lstm_a", 316, 60), ("VRNN lstm", 384, 256),
                                        ("SRNN lstm_h with peepholes", 256, 60)])
def test_convlstm_at_the_sibling_models_sizes(who, cin, hc):
    """the SRNN / VRNN baselines drive the same ConvLSTM one frame at a time on 8x8 maps
    (SRNN/SRNN.py:161-171,210-240: in = 256 or 256 + h_dim, hidden 60; VRNN/VRNN.py:169-173,199-201: in = 256 + 128,
    hidden 256; defaults of main_srnn.py / main_vrnn.py).  Three recurrent steps with gradients at those channel counts,
    HIP module against the CPU oracle on the same weights (the golden fixture `sibling_8x8` pins the oracle on this shape
    class at reduced channel counts).  The last variant sets nonzero peephole tensors Wci / Wcf / Wco on the module
    and, through the state dict, in the oracle (as a reference CPU checkpoint that carries them would): the peephole
    terms of both gate kernels run; same bounds, and the Wc gradients themselves are not produced, so not compared."""
    from Utils import ConvLSTM
    torch.manual_seed(91)
    B, H, W, S = 3, 8, 8, 3
    m = ConvLSTM(cin, hc, [3, 3], bias=True, peephole=True).cuda()
    g = torch.Generator().manual_seed(92)
    if "peepholes" in who:
        gp = torch.Generator().manual_seed(93)
        for n in ("Wci", "Wcf", "Wco"):
            m.LSTMlayer.register_parameter(n, torch.nn.Parameter((0.5 * torch.randn(1, hc, H, W, generator=gp)).cuda(),
                                                                 requires_grad=False))
        assert all(t is not None for t in m.LSTMlayer._peephole_tensors(H, W, "cuda"))
    xs = [torch.randn(B, 1, cin, H, W, generator=g) for _ in range(S)]
    h0, c0 = torch.randn(B, hc, H, W, generator=g) * 0.5, torch.randn(B, hc, H, W, generator=g) * 0.5
    wh, wc = torch.randn(B, hc, H, W, generator=g), torch.randn(B, hc, H, W, generator=g)
    sd = {k: v.detach().cpu().clone().requires_grad_(v.dtype == torch.float32) for k, v in m.state_dict().items()}

    def run(step, leaf):
        x = [leaf(t) for t in xs]
        h, c = leaf(h0), leaf(c0)
        ht, ct = h, c
        for t in range(S):
            _, ht, ct = step(x[t], ht, ct)
        ((ht * wh.to(ht.device)).sum() + (ct * wc.to(ht.device)).sum()).backward()
        return ht, ct, x[0].grad, h.grad, c.grad
    got = run(lambda x, h, c: m(x, h, c), lambda t: t.clone().cuda().requires_grad_(True))
    want = run(lambda x, h, c: O.convlstm(sd, "", x, h, c), lambda t: t.clone().requires_grad_(True))
    for name, a, b in zip(["ht", "ct", "grad_x0", "grad_h0", "grad_c0"], got, want):
        close(a, b, 2e-4, 2e-5)
    conv = m.LSTMlayer.conv[0]
    close(conv.weight.grad, sd["LSTMlayer.conv.0.weight"].grad, 2e-3, 2e-4)
    close(conv.bias.grad, sd["LSTMlayer.conv.0.bias"].grad, 2e-3, 2e-4)


@pytest.mark.parametrize("name", ["plain", "smooth_resq", "overshoot_D2", "with_skip", "no_skipfeat"])
def test_rfn_loss_end_to_end(golden, name):
    from RFN import RFN
    f = golden("rfn_loss.pt")[name]
    args = Namespace(**f["args"])
    # first call from fresh weights: ActNorm data dependent init on the t=1 batch + BatchNorm running stats
    m = load_sd(RFN(args), f["sd_fresh"]).train()
    out = m.loss(cu(f["x"]), 0, draws=[t for _, t in f["draws_first"]])
    for a, b in zip(out, f["out_first"]):
        assert abs(float(a) - b) <= 1e-4 * abs(b) + 1e-4, (float(a), b)
    # steady state with gradients; bits/dim within 1e-4 relative (north_star)
    m = load_sd(RFN(args), f["sd"]).train()
    kl_fb, kl, nll = m.loss(cu(f["x"]), 0, draws=[t for _, t in f["draws"]])
    for a, b in zip((kl_fb, kl, nll), f["out"]):
        assert abs(float(a) - b) <= 1e-4 * abs(b) + 1e-5, (float(a), b)
    bpd = O.bits_per_dim(kl.detach().cpu(), nll.detach().cpu(), f["x"].shape[2:], f["T"] - 1)
    assert abs(bpd - f["bits_per_dim"]) <= 1e-4 * abs(f["bits_per_dim"])
    (nll + 0.3 * kl_fb).backward()
    grads_close(m, {k: v for k, v in f["grads"].items() if not k.startswith(("extractor.net.", "upscaler.net."))
                    and "LSTMlayer.Wc" not in k}, 5e-3, 5e-4)


@pytest.mark.parametrize("B,Cx,Hc,H,W,S", [(4, 24, 10, 2, 2, 5), (33, 6, 4, 4, 4, 3), (3, 5, 6, 2, 2, 4)])
def test_convlstm_sequence_node_equals_per_step_cells(B, Cx, Hc, H, W, S, conv_precision):
    """ConvLSTM.forward_steps (one autograd node, time-batched input projection and gradients) against S calls of the
    cell (Utils/modules.py:355-377 driven per frame by RFN_new.py:131-139): states and every gradient.  The third
    case has channel counts the dense kernels do not take and must fall back to the per-step cells."""
    from Utils import ConvLSTM
    torch.manual_seed(11)
    m = ConvLSTM(Cx, Hc, (3, 3), bias=True).cuda()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(S, B, Cx, H, W, generator=g).cuda()
    h0, c0 = torch.randn(B, Hc, H, W, generator=g).cuda(), torch.randn(B, Hc, H, W, generator=g).cuda()
    gw = [torch.randn(B, Hc, H, W, generator=g).cuda() for _ in range(S)]
    gcl = torch.randn(B, Hc, H, W, generator=g).cuda()

    def run(seq):
        xs, hh, cc = x.clone().requires_grad_(True), h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        if seq:
            hs, hl, cl = m.forward_steps(xs, hh, cc)
        else:
            hs, hl, cl = [], hh, cc
            for t in range(S):
                _, hl, cl = m(xs[t].unsqueeze(1), hl, cl)
                hs.append(hl)
        (sum((a * b).sum() for a, b in zip(hs, gw)) + (cl * gcl).sum()).backward()
        conv = m.LSTMlayer.conv[0]
        return [torch.stack(hs), cl, xs.grad, hh.grad, cc.grad, conv.weight.grad.clone(), conv.bias.grad.clone()]
    a, b = run(True), run(False)
    for name, u, v in zip(["h", "c_last", "gx", "gh0", "gc0", "gw", "gb"], a, b):
        err = float((u - v).abs().max() / (v.abs().max() + 1e-12))
        assert err < 5e-5, (name, err)


@pytest.mark.parametrize("S,B,C,H,W,act", [(3, 4, 6, 8, 8, "leakyrelu"), (5, 2, 16, 2, 2, "relu"), (2, 3, 5, 4, 6, "tanh"),
                                           (4, 3, 8, 1, 2, None)])
def test_fused_per_step_batchnorm_activation(S, B, C, H, W, act):
    """rfn_stepbn_* through run_time_batched: BatchNorm2d (training) with the statistics of each timestep's B samples,
    fused with the following activation, against S separate calls of the torch modules (what the reference's
    per-frame extractor / upscaler calls do, RFN_new.py:126-128): output, input / affine gradients, running statistics."""
    import copy
    import torch.nn as nn
    from Utils.modules import NormLayer, ActFun, run_time_batched
    torch.manual_seed(21)
    layers = [NormLayer(C, "batchnorm")]
    if act in ("relu", "leakyrelu"):
        layers.append(ActFun(act))
    elif act == "tanh":
        layers.append(nn.Tanh())
    seq = nn.Sequential(*layers).cuda().train()
    with torch.no_grad():
        seq[0].norm.weight.uniform_(0.5, 1.5)
        seq[0].norm.bias.uniform_(-0.5, 0.5)
    ref = copy.deepcopy(seq)
    g = torch.Generator().manual_seed(22)
    x = (torch.randn(S * B, C, H, W, generator=g) * 2 + 0.7).cuda()
    gy = torch.randn(S * B, C, H, W, generator=g).cuda()
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = run_time_batched(seq, xa, S)
    yb = torch.cat([ref(xb[t * B:(t + 1) * B]) for t in range(S)], 0)
    (ya * gy).sum().backward()
    (yb * gy).sum().backward()
    rel = lambda u, v: float((u - v).abs().max() / (v.abs().max() + 1e-12))
    assert rel(ya, yb) < 2e-5
    assert rel(xa.grad, xb.grad) < 1e-4
    assert rel(seq[0].norm.weight.grad, ref[0].norm.weight.grad) < 1e-4
    assert rel(seq[0].norm.bias.grad, ref[0].norm.bias.grad) < 1e-4
    assert rel(seq[0].norm.running_mean, ref[0].norm.running_mean) < 1e-5
    assert rel(seq[0].norm.running_var, ref[0].norm.running_var) < 1e-5
    assert int(seq[0].norm.num_batches_tracked) == int(ref[0].norm.num_batches_tracked)


def test_graph_captured_step_equals_eager_step():
    """Solver in hipGraph mode (fwd+bwd captured, replayed) produces the same loss and gradients as the eager step."""
    import __graft_entry__ as ge
    from RFN.trainer import Solver
    from RFN import RFN
    from rfn_hip import dist as rdist
    args = ge._tiny_args()
    for k, v in dict(n_bits=8, n_epochs=1, learning_rate=0.0, verbose=False, path="/gpurun_out/tmp/", patience_lr=1,
                     factor_lr=0.5, min_lr=0.0, patience_es=1, beta_max=0.5, beta_min=0.5, beta_steps=10,
                     choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=16,
                     preprocess_range="0.5", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                     n_conditions=2, scheduler_type="linear", use_validation_set=False).items():
        setattr(args, k, v)
    torch.manual_seed(3)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.model = RFN(args).cuda().train()
    s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
    s.optimizer = torch.optim.SGD(s.model.parameters(), lr=0.0)  # parameters stay fixed: both modes see the same model
    g = torch.Generator().manual_seed(4)
    B, T = args.batch_size, 4
    x = torch.rand(B, T, 1, 16, 16, generator=g).cuda()
    draws = []
    for _ in range(T - 1):
        draws += [torch.randn(B, args.z_dim, 4, 4, generator=g).cuda(), torch.randn(B, args.z_dim, 4, 4, generator=g).cuda(),
                  (torch.rand(B, 1, 16, 16, generator=g) / 256).cuda()]
    s.model.loss(s.preprocess(x), 0, draws=draws)  # data dependent init
    s.beta = 0.5
    kl_fb, kl, nll = s.model.loss(s.preprocess(x), 0, draws=draws)
    s.optimizer.zero_grad(set_to_none=True)
    (nll + 0.5 * kl_fb).backward()
    eager = {n: p.grad.detach().clone() for n, p in s.model.named_parameters() if p.grad is not None}
    eager_loss = float(nll + 0.5 * kl_fb)
    # drop every reference to the eager autograd graph: its AccumulateGrad nodes are bound to the default stream and
    # would drag that stream into the capture (the trainer never keeps a loss tensor across steps either)
    del kl_fb, kl, nll
    s.optimizer.zero_grad(set_to_none=True)
    assert s.capture_graph(x, static_draws=draws), getattr(s, "_graph_error", "")
    for _ in range(2):  # replay twice: gradients must be overwritten, not accumulated
        out = s.train_step(x)
    torch.cuda.synchronize()
    assert abs(float(out) - eager_loss) <= 1e-5 * abs(eager_loss)
    for n, p in s.model.named_parameters():
        if n in eager:
            torch.testing.assert_close(p.grad, eager[n], rtol=1e-4, atol=1e-5 * float(eager[n].abs().max()) + 1e-7,
                                       msg=lambda m: n + ": " + m)


def test_graph_replay_repacks_weights_updated_in_place():
    """a captured body that asks for a conv pack and a small-map pack (one PackBatch) and consumes both: the packs are
    part of the graph, so a replay after an in-place weight update computes with the new weights, as an eager run does"""
    from rfn_hip import ops as K
    g = torch.Generator().manual_seed(12)
    N, Cin, Cout, S = 4, 16, 32, 8
    x, xs = cu(torch.randn(N, Cin, S, S, generator=g)), cu(torch.randn(N, Cin, 2, 2, generator=g))
    w, ws = cu(torch.randn(Cout, Cin, 3, 3, generator=g) / 12), cu(torch.randn(Cout, Cin, 3, 3, generator=g) / 12)
    fp = K.fwd_prec(S, S)

    def body():
        with K.PackBatch() as pb:
            pc, pd = pb.conv(w, prec=fp), pb.dense(ws, 2, 2, False)
        return K.conv2d_raw(x, None, pc, Cout, 3, prec=fp), K.smallmap_dense(xs, pd, Cout)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    graph.replay()
    old = [o.clone() for o in out]
    w.mul_(-0.5).add_(0.03)
    ws.mul_(1.5).sub_(0.02)
    graph.replay()
    torch.cuda.synchronize()
    eager = body()
    ref = (F.conv2d(x.cpu().double(), w.cpu().double(), padding=1), F.conv2d(xs.cpu().double(), ws.cpu().double(), padding=1))
    for o, o_old, e, r in zip(out, old, eager, ref):
        close(o, e.cpu(), 1e-6, 0.0)               # the replay equals the eager run on the new weights
        close(o, r, 2e-5, 0.0)                     # ... which is the convolution with them (bf16x3 at worst)
        assert float((o - o_old).abs().max()) > 0.1 * float(r.abs().max())   # and not the old result


def test_graph_replays_are_reproducible_canonical_architecture():
    """canonical architecture (split-K / few-pixel kernels, multi-block torch reductions) at B=2, T=4 with pinned draws
    and lr=0: every replay of the captured step must reproduce the eager loss and gradients.  Guards the ROCm graph
    memset-node race (rfn_hip/__init__.py): with it, replays sporadically return stale / non-finite values."""
    import main_rfn
    from RFN.trainer import Solver
    from RFN import RFN
    from rfn_hip import dist as rdist
    B, T = 2, 4
    args = main_rfn.build_parser().parse_args(main_rfn.canonical_smmnist_argv(B, T))
    args.path = "/gpurun_out/tmp/"
    args.beta_min = args.beta_max = 0.5
    torch.manual_seed(5)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.model = RFN(args).cuda().train()
    s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
    s.optimizer = torch.optim.SGD(s.model.parameters(), lr=0.0)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(B, T, 1, 64, 64, generator=g).cuda()
    zshape = tuple(s.model.z_0.shape)
    draws = []
    for _ in range(T - 1):
        draws += [torch.randn(zshape, generator=g).cuda(), torch.randn(zshape, generator=g).cuda(),
                  (torch.rand(B, 1, 64, 64, generator=g) / 256).cuda()]
    s.model.loss(s.preprocess(x), 0, draws=draws)  # data dependent init
    kl_fb, kl, nll = s.model.loss(s.preprocess(x), 0, draws=draws)
    s.optimizer.zero_grad(set_to_none=True)
    (nll + 0.5 * kl_fb).backward()
    eager = {n: p.grad.detach().clone() for n, p in s.model.named_parameters() if p.grad is not None}
    eager_loss = float(nll + 0.5 * kl_fb)
    del kl_fb, kl, nll
    s.optimizer.zero_grad(set_to_none=True)
    assert s.capture_graph(x, static_draws=draws), getattr(s, "_graph_error", "")
    for r in range(8):
        out = s.train_step(x)
        torch.cuda.synchronize()
        assert abs(float(out) - eager_loss) <= 2e-5 * abs(eager_loss), (r, float(out), eager_loss)
        for n, p in s.model.named_parameters():
            if n in eager:
                torch.testing.assert_close(p.grad, eager[n], rtol=1e-3, atol=2e-4 * float(eager[n].abs().max()) + 1e-7,
                                           msg=lambda m: "replay %d %s: %s" % (r, n, m))


@pytest.mark.parametrize("Hd,N,C,Cc,S", [(64, 3, 8, 6, 8), (256, 70, 8, 12, 16), (512, 66, 4, 10, 16)])
def test_glowstep_hd64_gradients_vs_oracle(conv_precision, Hd, N, C, Cc, S):
    """hidden width 64 takes the fused data-gradient + activation-backward kernels (the golden fixtures use 16); the
    256 / 512 wide cases have enough pixels (>= 16384) for the weight-stationary 1x1 / 3x3 kernels, the implicit 3x3
    weight gradient and (512) two 256-channel output blocks."""
    from Flow import GlowStep
    from tests.golden_args import GLOW_DEFAULTS
    a = dict(GLOW_DEFAULTS)
    a["n_units_affine"] = Hd
    torch.manual_seed(12)
    gs = GlowStep([N, C, S, S], [N, Cc, S, S], glow_ns(a)).cuda().train()
    g = torch.Generator().manual_seed(13)
    x0 = torch.randn(N, C, S, S, generator=g)
    c0 = torch.randn(N, Cc, S, S, generator=g)
    gs(cu(x0), cu(c0), torch.zeros(N, device="cuda"), False)  # data dependent init
    with torch.no_grad():
        for prm in gs.parameters():
            prm.add_(0.05 * torch.randn(prm.shape, generator=g).cuda())
    x = cu(x0).requires_grad_(True)
    c = cu(c0).requires_grad_(True)
    y, ld = gs(x, c, torch.zeros(N, device="cuda"), False)
    wgt = torch.randn(y.shape, generator=g)
    gld = torch.randn(N, generator=g)
    ((y * cu(wgt)).sum() + (ld * cu(gld)).sum()).backward()
    # oracle on the same parameters
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in gs.state_dict().items()}
    xo = x0.clone().requires_grad_(True)
    co = c0.clone().requires_grad_(True)
    yo, ldo = O.glowstep(sd, "", xo, co, torch.zeros(N), False, True)
    ((yo * wgt).sum() + (ldo * gld).sum()).backward()
    close(y, yo.detach(), 1e-4, 1e-5)
    close(ld, ldo.detach(), 1e-4, 1e-5)
    if Hd <= 64:
        close(x.grad, xo.grad, 2e-3, 1e-5)
        close(c.grad, co.grad, 2e-3, 1e-5)
        for k, p in gs.named_parameters():
            ref = sd[k].grad
            torch.testing.assert_close(p.grad.cpu(), ref, rtol=3e-3, atol=3e-4 * float(ref.abs().max()) + 1e-6,
                                       msg=lambda m: k + ": " + m)
        return
    # Millions of hidden activations: a handful sit within the arithmetic's 1e-5 of the LeakyReLU kink and take the other
    # slope than the CPU run (checked: the outliers of the split-precision run are exactly the 3x3 neighbourhoods of
    # the sign flips against the fp32 kernels, which themselves agree with the oracle to 1e-6 everywhere).  The
    # derivative is discontinuous there, so gradients are compared in the L2 norm.
    l2 = lambda u, v: float((u.detach().cpu().double() - v.double()).norm() / (v.double().norm() + 1e-30))
    tol = 2e-5 if conv_precision == "f32" else 5e-3
    assert l2(x.grad, xo.grad) < tol
    assert l2(c.grad, co.grad) < tol
    for k, p in gs.named_parameters():
        assert l2(p.grad, sd[k].grad) < tol, (k, l2(p.grad, sd[k].grad))


def test_flow_bijection_single_level():
    """with L = 1 there is no Split2d re-sampling, so g(f(x)) = x (the reference's 'bijection check',
    RFN_new.py:437-439, asserted here)."""
    from Flow import ListGlow
    from tests.golden_args import GLOW_DEFAULTS
    a = dict(GLOW_DEFAULTS)
    a.update(L=1, K=3, n_units_affine=64)
    torch.manual_seed(5)
    flow = ListGlow([4, 3, 16, 16], [[4, 6, 8, 8]], (4, 12, 8, 8), glow_ns(a)).cuda().train()
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(4, 3, 16, 16, generator=g) - 0.5).cuda()
    cond = [torch.randn(4, 6, 8, 8, generator=g).cuda()]
    base = torch.randn(4, 12, 8, 8, generator=g).cuda()
    noise = torch.zeros_like(x)
    flow.log_prob(x, cond, base, 0, noise=noise)  # data dependent init
    with torch.no_grad():
        for prm in flow.parameters():
            prm.add_(0.05 * torch.randn(prm.shape, generator=g).cuda())
        z, nll = flow.log_prob(x, cond, base, 0, noise=noise)
        xb = flow.sample(z, cond, base, temperature=1.0)
    assert torch.isfinite(nll).all()
    close(xb, x.cpu(), 2e-4, 2e-5)


def test_canonical_size_properties():
    """BASELINE sizes (N = 32*19 = 608 frames, level-0 GlowStep 4ch 32x32, cond 16ch, Hd 256): reverse(forward(x)) = x,
    and the time-batched call equals the per-timestep calls (what the reference executes)."""
    from Flow import GlowStep
    from tests.golden_args import GLOW_DEFAULTS
    a = dict(GLOW_DEFAULTS)
    a["n_units_affine"] = 256
    torch.manual_seed(7)
    B, T1 = 32, 19
    gs = GlowStep([B, 4, 32, 32], [B, 16, 32, 32], glow_ns(a)).cuda().train()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B * T1, 4, 32, 32, generator=g).cuda()
    c = torch.randn(B * T1, 16, 32, 32, generator=g).cuda()
    with torch.no_grad():
        gs(x[:B], c[:B], torch.zeros(B, device="cuda"), False)  # init on the t = 1 batch
        for prm in gs.parameters():
            prm.add_(0.02 * torch.randn(prm.shape, generator=g).cuda())
        y, ld = gs(x, c, torch.zeros(B * T1, device="cuda"), False)
        xb, ldb = gs(y, c, ld.clone(), True)
        assert float((xb - x).abs().max()) < 2e-4 * float(x.abs().max())
        assert float(ldb.abs().max()) < 1e-4 * float(ld.abs().max()) + 1e-3
        ys = torch.cat([gs(x[t * B:(t + 1) * B], c[t * B:(t + 1) * B], torch.zeros(B, device="cuda"), False)[0]
                        for t in range(T1)])
        assert torch.equal(ys, y)  # no reduction crosses a frame in the forward kernels: bit identical


def test_generation_paths_run(golden):
    """predict / sample / reconstruct (RFN_new.py:256-494) through the reverse kernels: shapes, finiteness, and
    determinism of the conditioning frames."""
    from RFN import RFN
    f = golden("rfn_loss.pt")["plain"]
    m = load_sd(RFN(Namespace(**f["args"])), f["sd"]).eval()
    x = cu(f["x"])
    true_x, preds = m.predict(x, n_predictions=3, n_conditions=2)
    assert tuple(preds.shape) == (3,) + tuple(x[:, 0].shape) and torch.isfinite(preds).all()
    assert torch.equal(true_x[0], f["x"][:, 0])
    samples = m.sample(x, n_samples=2)
    assert tuple(samples.shape) == (2,) + tuple(x[:, 0].shape) and torch.isfinite(samples).all()
    recons, recons_flow = m.reconstruct(x)
    assert tuple(recons.shape) == (f["T"],) + tuple(x[:, 0].shape)
    assert torch.isfinite(recons).all() and torch.isfinite(recons_flow).all()


def test_canonical_rfn_loss_vs_oracle_T10(conv_precision):
    """north_star's bits/dim budget on the real thing: canonical architecture (K=10, L=5, Hd=256), B=2, T=10, pinned
    draws, every flow parameter perturbed by N(0, s^2) after the data dependent init; RFN.loss on the GPU against the
    CPU oracle, |Δ bits/dim| / |bits/dim| <= 1e-4 (rtol only).  s = 0.003 is a well-conditioned model (bits/dim ~ 50),
    s = 0.01 an ill-conditioned one (bits/dim ~ 1e11: the 9-step rollout explodes), at s = 0.1 the reference arithmetic
    itself overflows (the oracle returns nan), which is asserted rather than compared.
    'mixed' (the shipped arithmetic) and 'f32' must hold the budget everywhere; all-'bf16x3' only on the
    well-conditioned model -- two bf16 pieces per operand are 16 significant bits (tools/precision_study.py) and measure
    1e-4..5e-4 on the ill-conditioned one, which is why the forward pass does not use them.
    The GPU figure is the median of three evaluations of the same weights (bench.parity_check): in the ill-conditioned
    case the run-dependent order of the split-K float atomics alone moves bits/dim by 1e-5..8e-5, fp32 kernels included.
    This is the gate bench.py uses to choose its headline run."""
    import bench
    r = bench.parity_check(torch.device("cuda"), T=10, scales=(0.003, 0.01, 0.1))
    cases = {c["perturbation"]: c for c in r["cases"]}
    assert not cases[0.1]["oracle_finite"]
    assert cases[0.003]["rel_err"] <= 1e-4, (conv_precision, cases[0.003])
    if conv_precision != "bf16x3":
        assert cases[0.01]["rel_err"] <= 1e-4, (conv_precision, cases[0.01])


def _tiny_solver_args(path, B=2):
    import __graft_entry__ as ge
    args = ge._tiny_args()
    args.batch_size = B
    args.x_dim = [B, 1, 16, 16]
    args.condition_dim = [B, 1, 16, 16]
    for k, v in dict(n_bits=8, n_epochs=1, learning_rate=1e-3, verbose=False, path=path, patience_lr=1,
                     factor_lr=0.5, min_lr=0.0, patience_es=1, beta_max=0.5, beta_min=0.5, beta_steps=10,
                     choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=16,
                     preprocess_range="0.5", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                     n_conditions=2, scheduler_type="linear", use_validation_set=False).items():
        setattr(args, k, v)
    return args


def test_hip_adam_equals_torch_adam():
    """rfn_adam_step_f32 (all tensors in one launch) against torch.optim.Adam (RFN/trainer.py:96 builds it with defaults):
    five steps on tensors of awkward sizes, one of which has no gradient on two of the steps (its own step count), then the
    state dicts are swapped between the two implementations and both continue identically; weight decay covered once."""
    from rfn_hip.optim import HipAdam
    g = torch.Generator().manual_seed(3)
    shapes = [(1,), (7,), (33, 5), (4096,), (8192,), (8193,), (3, 100003), (64, 32, 3, 3)]
    for wd in (0.0, 0.01):
        pa = [torch.nn.Parameter(torch.randn(sh, generator=g).cuda()) for sh in shapes]
        pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
        oa = HipAdam(pa, lr=1e-2, weight_decay=wd)
        ob = torch.optim.Adam(pb, lr=1e-2, weight_decay=wd)

        def step(i, oa, ob, pa, pb):
            for j, (a, b) in enumerate(zip(pa, pb)):
                if j == 2 and i in (1, 3):
                    a.grad = b.grad = None
                    continue
                gr = (torch.randn(a.shape, generator=g) * (0.1 + j)).cuda()
                a.grad, b.grad = gr.clone(), gr.clone()
            if i == 3:
                for grp in list(oa.param_groups) + list(ob.param_groups):
                    grp["lr"] = 3e-3
            oa.step(); ob.step()
        for i in range(5):
            step(i, oa, ob, pa, pb)
        for a, b in zip(pa, pb):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=2e-6, atol=1e-7)
        sa, sb = oa.state_dict(), ob.state_dict()
        for k in sb["state"]:
            assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"])
            torch.testing.assert_close(sa["state"][k]["exp_avg"], sb["state"][k]["exp_avg"], rtol=2e-6, atol=1e-8)
            torch.testing.assert_close(sa["state"][k]["exp_avg_sq"], sb["state"][k]["exp_avg_sq"], rtol=2e-6, atol=1e-10)
        # checkpoints are interchangeable: continue each implementation from the other's state
        oa2, ob2 = HipAdam(pa, lr=3e-3, weight_decay=wd), torch.optim.Adam(pb, lr=3e-3, weight_decay=wd)
        oa2.load_state_dict(sb); ob2.load_state_dict(sa)
        for i in range(5, 8):
            step(i, oa2, ob2, pa, pb)
        for a, b in zip(pa, pb):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=4e-6, atol=1e-7)


def test_checkpoint_resume_round_trip(tmp_path, conv_precision):
    """Solver.checkpoint -> read_checkpoint (nothing executed from the file) -> Solver.load reproduces the model, the
    optimizer state and the bookkeeping: the same loss on the same batch and identical parameters after one more Adam
    step (reference: RFN/trainer.py:277-315)."""
    if conv_precision != "mixed":
        pytest.skip("arithmetic-independent host logic: run once")
    from RFN.trainer import Solver
    from RFN import RFN
    from rfn_hip import dist as rdist
    import os as _os
    rel = "/" + _os.path.relpath(str(tmp_path), _os.getcwd()) + "/"
    _os.makedirs(str(tmp_path / "model_folder"), exist_ok=True)

    def make():
        args = _tiny_solver_args(rel)
        s = Solver(args)
        s.device = torch.device("cuda")
        s.model = RFN(args).cuda().train()
        s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
        s.optimizer = Solver.make_optimizer(s.model.parameters(), 1e-3)
        return s
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 4, 1, 16, 16, generator=g).cuda()
    draws = []
    for _ in range(3):
        draws += [torch.randn(2, 4, 4, 4, generator=g).cuda(), torch.randn(2, 4, 4, 4, generator=g).cuda(),
                  (torch.rand(2, 1, 16, 16, generator=g) / 256).cuda()]
    torch.manual_seed(9)
    s = make()
    for _ in range(3):
        s.train_step(x)
    s.checkpoint("rfn.pt", 1, 12.5)
    ck = Solver.read_checkpoint(str(tmp_path / "model_folder" / "rfn.pt"))
    assert set(ck) >= {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "kl_loss", "recon_loss", "losses",
                       "plot_counter", "annealing_counter", "bits_per_dim", "args"}
    assert ck["args"].K == s.args.K and ck["annealing_counter"] == 3
    torch.manual_seed(10)          # a different initialisation: everything must come from the file
    r = make()
    epoch, loss = r.load(ck)
    assert epoch == 1 and loss == 12.5 and r.counter == 3 and len(r.bits) == 3
    with torch.no_grad():
        a = [float(v) for v in s.model.loss(s.preprocess(x), 0, draws=draws)]
        b = [float(v) for v in r.model.loss(r.preprocess(x), 0, draws=draws)]
    assert a == b
    torch.manual_seed(77)          # the step draws its own noise: same generator state for both
    s.train_step(x)
    torch.manual_seed(77)
    r.train_step(x)
    for (n, p), (_, q) in zip(s.model.named_parameters(), r.model.named_parameters()):
        # (weight gradients are summed with float atomics: equal up to summation order)
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-7, msg=lambda m: n + ": " + m)


def test_graphed_generation_equals_eager_generation(conv_precision, monkeypatch):
    """RFN.predict / RFN.sample replay one generation step per frame from a hipGraph (RFN._gen_step_graphed; the draws
    are inputs of the graph).  With the generator seeded identically the frames equal those of the eager launches
    (RFN_GEN_GRAPH=0) up to summation order, also after the weights changed (the graph is rebuilt: inverse matrices and
    weight packs are baked into it)."""
    if conv_precision != "mixed":
        pytest.skip("launch-mode logic: run once")
    import rfn_hip
    if not rfn_hip.graph_capture_safe():
        pytest.skip("hipGraph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before the HIP runtime starts")
    import __graft_entry__ as ge
    from RFN import RFN
    args = ge._tiny_args()
    torch.manual_seed(5)
    m = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(args.batch_size, 5, *args.x_dim[1:], generator=g) - 0.5).cuda()
    m.loss(x, 0)                       # data dependent init
    m.eval()

    def run(graph):
        monkeypatch.setenv("RFN_GEN_GRAPH", "1" if graph else "0")
        torch.manual_seed(11)
        _, pred = m.predict(x, 3, 2)
        torch.manual_seed(12)
        smp = m.sample(x, 3)
        return pred, smp

    for rnd in range(2):
        pe, se = run(False)
        pg, sg = run(True)
        assert getattr(m, "_gen_graph", None) is not None
        close(pg.cuda(), pe, 1e-4, 1e-5)
        close(sg.cuda(), se, 1e-4, 1e-5)
        with torch.no_grad():          # change the weights: the graph must follow
            for prm in m.flow.parameters():
                prm.add_(0.01 * torch.randn_like(prm))


def test_generation_follows_hipadam_updates(tmp_path, conv_precision, monkeypatch):
    """HipAdam updates parameters through a raw-pointer kernel launch; the generation caches
    (ListGlow._reverse_cache: inverse 1x1 matrices and weight packs; RFN._gen_graph: the captured per-frame hipGraph) are
    keyed on the parameters' version counters, so the optimizer must bump them.  predict -> train steps with HipAdam (the
    Solver's GPU optimizer) -> predict again: the cached / graphed frames must equal an uncached eager generation on the
    new weights, and must differ from the frames of the old weights."""
    if conv_precision != "mixed":
        pytest.skip("cache logic: run once")
    import rfn_hip
    import os as _os
    from RFN.trainer import Solver
    from RFN import RFN
    from rfn_hip import dist as rdist
    from rfn_hip.optim import HipAdam
    rel = "/" + _os.path.relpath(str(tmp_path), _os.getcwd()) + "/"
    args = _tiny_solver_args(rel)
    torch.manual_seed(31)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.model = RFN(args).cuda().train()
    s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
    s.optimizer = Solver.make_optimizer(s.model.parameters(), 2e-2)   # large steps: the frames must visibly move
    assert isinstance(s.optimizer, HipAdam)
    g = torch.Generator().manual_seed(32)
    xs = [torch.rand(2, 4, 1, 16, 16, generator=g).cuda() for _ in range(2)]
    x = s.preprocess(xs[0])
    s.train_step(xs[0])                # data dependent init + first update
    graph_ok = rfn_hip.graph_capture_safe()

    def gen(cached):
        monkeypatch.setenv("RFN_GEN_GRAPH", "1" if (cached and graph_ok) else "0")
        monkeypatch.setenv("RFN_GEN_CACHE", "1" if cached else "0")
        s.model.eval()
        torch.manual_seed(41)
        _, pred = s.model.predict(x, 2, 2)
        torch.manual_seed(42)
        smp = s.model.sample(x, 2)
        s.model.train()
        return pred.cuda().clone(), smp.cuda().clone()

    p0, s0 = gen(True)                 # fills the caches (and captures the generation graph) on the current weights
    v0 = [p._version for p in s.model.parameters()]
    for i in range(3):
        s.train_step(xs[i % 2])        # HipAdam: raw-pointer updates
    assert all(p._version > v for p, v in zip(s.model.parameters(), v0) if p.grad is not None)
    p1, s1 = gen(True)                 # must NOT reuse the stale inverse matrices / packs / graph
    pe, se = gen(False)                # uncached eager generation on the new weights
    close(p1, pe.cpu(), 1e-4, 1e-5)
    close(s1, se.cpu(), 1e-4, 1e-5)
    assert float((p1 - p0).abs().max()) > 1e-3 and float((s1 - s0).abs().max()) > 1e-3


def test_training_trajectory_split_precision_vs_fp32_mfma(tmp_path, conv_precision):
    """20 Adam steps on the tiny configuration: the loss trajectory of the shipped arithmetic ('mixed', and 'bf16x3') stays
    on the trajectory of the all-fp32-MFMA kernels -- same initial weights, same batches, same noise (the RNG is re-seeded
    before every step).  Parity over many optimizer steps, not just at one point: every per-step loss within
    2e-3 relative of the fp32 one (the gradients' own tolerance), the final parameters within 5e-3 (a quarter of the distance 20 Adam steps can cover)."""
    if conv_precision == "f32":
        pytest.skip("f32 is the reference trajectory of this test")
    from RFN.trainer import Solver
    from RFN import RFN
    from rfn_hip import dist as rdist
    from rfn_hip import ops
    import os as _os
    rel = "/" + _os.path.relpath(str(tmp_path), _os.getcwd()) + "/"
    g = torch.Generator().manual_seed(14)
    xs = [torch.rand(2, 4, 1, 16, 16, generator=g).cuda() for _ in range(4)]

    def run(prec):
        ops.CONV_PRECISION = prec
        torch.manual_seed(21)
        args = _tiny_solver_args(rel)
        s = Solver(args)
        s.device = torch.device("cuda")
        s.model = RFN(args).cuda().train()
        s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
        s.optimizer = Solver.make_optimizer(s.model.parameters(), 1e-3)
        for i in range(20):
            torch.manual_seed(100 + i)
            s.train_step(xs[i % 4])
        s.flush_log()
        return [float(v) for v in s.losses], {n: p.detach().clone() for n, p in s.model.named_parameters()}

    try:
        l_ref, p_ref = run("f32")
        l_sp, p_sp = run(conv_precision)
    finally:
        ops.CONV_PRECISION = conv_precision
    assert len(l_ref) == len(l_sp) == 20
    for a, b in zip(l_sp, l_ref):
        assert abs(a - b) <= 2e-3 * abs(b), (l_sp, l_ref)
    # Adam normalises every gradient component to a step of about lr = 1e-3 whatever its size: a component whose
    # gradient is near zero (the learnable initial states, dead hidden units, the scale direction of a conv weight in
    # front of a BatchNorm) can take the opposite step.  After 20 steps (0.02 of possible movement) no parameter may
    # have drifted by more than a quarter of that.
    for n, q in p_ref.items():
        assert float((p_sp[n] - q).abs().max()) <= 5e-3, n


def test_forward_pass_is_bit_reproducible(conv_precision):
    """no order-dependent float atomics in the forward pass.  The canonical architecture (all five
    flow levels, split-K convolutions at the deep ones, the per-frame log-det sums of the level nodes) evaluated three
    times on the same weights, inputs and noise gives bit-identical KL, NLL and per-frame flow log-likelihoods -- in
    training mode with gradients enabled (the path the bench and the parity check run) and under no_grad."""
    import main_rfn
    from RFN import RFN
    B, T = 2, 4
    args = main_rfn.build_parser().parse_args(main_rfn.canonical_smmnist_argv(B, T))
    torch.manual_seed(71)
    m = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(72)
    x = ((torch.rand(B, T, 1, 64, 64, generator=g) * 255).floor() / 256 - 0.5).cuda()
    draws = []
    for _ in range(T - 1):
        draws += [torch.randn(B, 56, 2, 2, generator=g).cuda(), torch.randn(B, 56, 2, 2, generator=g).cuda(),
                  (torch.rand(B, 1, 64, 64, generator=g) / 256).cuda()]
    with torch.no_grad():
        m.loss(x, 0, draws=draws)                       # data dependent ActNorm init
        gp = torch.Generator().manual_seed(73)
        for prm in m.flow.parameters():                 # (Conv2dZeros start at zero: make every layer matter)
            prm.add_(0.003 * torch.randn(prm.shape, generator=gp).cuda())
    # the three scalars are means over frames (a last-bit difference in one frame can vanish in them): also keep what
    # ListGlow.log_prob returned for every frame -- its latent z and the per-frame negative log-likelihood
    seen = []
    orig = m.flow.log_prob

    def spy(*a, **k):
        z, nll_f = orig(*a, **k)
        seen.append((z.detach().clone(), nll_f.detach().clone()))
        return z, nll_f
    m.flow.log_prob = spy
    outs = []
    for rep in range(3):
        kl_fb, kl, nll = m.loss(x, 0, draws=draws)
        outs.append((kl_fb.detach().clone(), kl.detach().clone(), nll.detach().clone()) + seen.pop())
    with torch.no_grad():
        for rep in range(2):
            kl_fb, kl, nll = m.loss(x, 0, draws=draws)
            outs.append((kl_fb.clone(), kl.clone(), nll.clone()) + seen.pop())
    # (the two modes may legitimately differ from each other: under no_grad the latent recurrence takes other launches)
    for lo, hi in ((0, 3), (3, 5)):
        for i in range(lo + 1, hi):
            for name, a, b in zip(("kl_fb", "kl", "nll", "flow z", "per-frame nll"), outs[i], outs[lo]):
                assert torch.equal(a, b), (name, i, lo, float((a - b).abs().max()))
    assert bool(torch.isfinite(outs[0][2]))


def test_training_trajectory_vs_oracle_adam(conv_precision):
    """the multi-step evidence for the shipped arithmetic against the ORACLE, not against another GPU
    arithmetic.  12 Adam steps on the tiny configuration: GPU (RFN.loss on the HIP kernels + HipAdam) and CPU (oracle
    rfn_loss + torch.optim.Adam), same post-init weights, same four batches, same pinned noise per step.
    Bounds: every per-step loss within 2e-3 relative; final parameters max drift <= 2e-3 and mean drift <= 3e-4 -- the
    bounds the round-2 GPU-vs-GPU test started from -- over the WELL-CONDITIONED components.  A component is
    ill-conditioned for Adam when its gradient is below the gradients' own arithmetic tolerance (elsewhere in this file:
    2e-4 of the tensor's largest gradient magnitude): Adam divides by sqrt(v), so such a component takes steps of size lr
    whose sign the arithmetic decides (measured round 2: `z_0x`, a learnable initial state whose gradient is ~1e-9,
    drifted 4.3e-4 on average).  Those components are held to the distance the steps can cover (steps x lr), nothing
    tighter is meaningful for them; they must be a minority (< 25 % of all components)."""
    if conv_precision != "mixed":
        pytest.skip("the shipped arithmetic (the CPU oracle needs ~8 s per step on the GPU box: one arithmetic, 12 steps)")
    import __graft_entry__ as ge
    from RFN import RFN
    from rfn_hip.optim import HipAdam
    lr, steps, T = 1e-3, 12, 4
    args = ge._tiny_args()
    torch.manual_seed(61)
    m = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(62)
    xs = [(torch.rand(args.batch_size, T, 1, 16, 16, generator=g) * 255).floor() / 256 - 0.5 for _ in range(4)]
    shapes = [(args.batch_size, args.z_dim, 4, 4)] * 2
    draws_all = []
    for _ in range(steps + 1):
        d = []
        for _ in range(T - 1):
            d += [torch.randn(*shapes[0], generator=g), torch.randn(*shapes[1], generator=g),
                  torch.rand(args.batch_size, 1, 16, 16, generator=g) / 256]
        draws_all.append(d)
    with torch.no_grad():
        m.loss(xs[0].cuda(), 0, draws=[d.cuda() for d in draws_all[-1]])      # data dependent ActNorm init
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    leaves = {}
    for k, v in sd.items():
        if v.is_floating_point() and "running_" not in k:
            v.requires_grad_(True)
            leaves[k] = v
    names = [n for n, _ in m.named_parameters()]
    assert all(n in leaves for n in names)
    opt_c = torch.optim.Adam([leaves[n] for n in names], lr=lr)
    opt_g = HipAdam(list(m.parameters()), lr=lr)
    cfg = vars(args)
    l_c, l_g = [], []
    for i in range(steps):
        x, d = xs[i % 4], draws_all[i]
        kl_fb, kl, nll = O.rfn_loss(sd, cfg, x, d, True)
        opt_c.zero_grad()
        (nll + 0.5 * kl_fb).backward()
        opt_c.step()
        l_c.append(float(nll + 0.5 * kl_fb))
        kl_fb, kl, nll = m.loss(x.cuda(), 0, draws=[t.cuda() for t in d])
        opt_g.zero_grad(set_to_none=True)
        (nll + 0.5 * kl_fb).backward()
        opt_g.step()
        l_g.append(float(nll + 0.5 * kl_fb))
    for a, b in zip(l_g, l_c):
        assert abs(a - b) <= 2e-3 * abs(b), (l_g, l_c)
    n_all = n_ill = 0
    for n, p in m.named_parameters():
        st = opt_c.state[leaves[n]]
        if not st:
            continue
        vhat = (st["exp_avg_sq"] / (1 - 0.999 ** steps)).sqrt()         # typical |gradient| per component
        ill = vhat <= 2e-4 * float(vhat.max())
        diff = (p.detach().cpu() - leaves[n].detach()).abs()
        n_all += diff.numel()
        n_ill += int(ill.sum())
        if bool((~ill).any()):
            assert float(diff[~ill].max()) <= 2e-3, (n, float(diff[~ill].max()))
            assert float(diff[~ill].mean()) <= 3e-4, (n, float(diff[~ill].mean()))
        if bool(ill.any()):
            assert float(diff[ill].max()) <= 1.05 * steps * lr, (n, float(diff[ill].max()))
    assert n_ill < 0.25 * n_all, (n_ill, n_all)


_DP_RFN_WORKER = r"""
import os, sys
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "recurrent-flows-msc_amd"))
import torch, torch.distributed as dist
from tests.test_hip_modules import _tiny_solver_args
from RFN.trainer import Solver
from RFN import RFN
from rfn_hip import dist as rdist
rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
torch.cuda.set_device(0)
if world > 1:
    dist.init_process_group("gloo")
B_glob, T = 4, 4
B = B_glob // world
g = torch.Generator().manual_seed(4)
X = torch.rand(B_glob, T, 1, 16, 16, generator=g)
init = {k: torch.randn(B_glob, *s, generator=g) * 0.1 for k, s in (("z_0", (4, 4, 4)), ("z_0x", (4, 4, 4)), ("h_0", (8, 4, 4)), ("c_0", (8, 4, 4)))}
draws_glob = []
for _ in range(T - 1):
    draws_glob += [torch.randn(B_glob, 4, 4, 4, generator=g), torch.randn(B_glob, 4, 4, 4, generator=g),
                   torch.rand(B_glob, 1, 16, 16, generator=g) / 256]
sl = slice(rank * B, (rank + 1) * B)
args = _tiny_solver_args("/gpurun_out/tmp/", B)
# the default BatchNorm of the extractor / upscaler, with the statistics of the GLOBAL batch (synchronised BatchNorm,
# rfn_hip.dist.set_sync_batchnorm; the bench keeps local statistics: a collective cannot live in its captured graph)
assert args.norm_type_features == "batchnorm"
rdist.set_sync_batchnorm(True)
torch.manual_seed(50 + rank)                      # different initial weights per rank: the broadcast must fix that
s = Solver(args)
s.device = torch.device("cuda")
s.model = RFN(args).cuda().train()
rdist.broadcast_module_state(s.model)
with torch.no_grad():
    for k, v in init.items():
        getattr(s.model, k).copy_(v[sl].cuda())   # rank r owns rows [rB, (r+1)B) of the batch-shaped initial states
s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
x = X[sl].cuda()
draws = [d[sl].cuda() for d in draws_glob]
xin = s.preprocess(x)
kl_fb, kl, nll = s.model.loss(xin, 0, draws=draws)          # first forward: data dependent ActNorm init (rank-local)
if world > 1:
    rdist.broadcast_module_state(s.model)                    # replicas take rank 0's init (Solver.train_step does this)
    kl_fb, kl, nll = s.model.loss(xin, 0, draws=draws)
(nll + 0.5 * kl_fb).backward()
s.reducer.finish()
torch.cuda.synchronize()
out = {"grads": {n: p.grad.detach().cpu() for n, p in s.model.named_parameters() if p.grad is not None},
       "state": {k: v.detach().cpu() for k, v in rdist.gather_sharded_state(s.model).items()},
       "loss": rdist.all_reduce_mean_scalars(nll.detach().cpu() if world > 1 else nll)[0]}
torch.save(out, sys.argv[2] + ".rank%d" % rank)
if world > 1:
    dist.destroy_process_group()
print("rank %d ok" % rank)
"""


_DP_TRAIN_WORKER = r"""
import os, sys
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "recurrent-flows-msc_amd"))
import torch
from tests.test_hip_modules import _tiny_solver_args
from RFN.trainer import Solver
args = _tiny_solver_args(sys.argv[2], 2)          # per-rank batch 2 -> global batch 4
args.synthetic_data, args.multigpu, args.digit_size, args.max_steps, args.n_epochs = True, True, 8, 2, 1
s = Solver(args)
s.build()                                          # process group (gloo, both ranks on this GPU), loaders, model, HipAdam
assert s.world == 2 and type(s.optimizer).__name__ == "HipAdam"
s.train()                                          # two steps, the end-of-epoch consensus, the checkpoint collective
print("rank %d trained, counter %d" % (s.rank, s.counter))
"""


def test_data_parallel_solver_train_and_resume(tmp_path, conv_precision):
    """ADVICE r2 (high / medium): a two-rank `Solver.train()` reaches the end of its epoch -- the loss / stop consensus
    (host scalars through the process group), the checkpoint collective -- and writes a file that describes ONE process
    on the global batch: the gathered rows of the sharded initial states AND of their Adam moments, the global batch size
    beside the per-rank args.  A single process then resumes it (`Solver.args_for_world`, `Solver.load`: the moments have
    their parameters' sizes, which HipAdam checks) and takes a step."""
    if conv_precision != "mixed":
        pytest.skip("arithmetic-independent protocol: run once")
    import subprocess, sys as _sys, os as _os
    from tests.conftest import ROOT
    from RFN.trainer import Solver
    script = tmp_path / "dp_train_worker.py"
    script.write_text(_DP_TRAIN_WORKER)
    rel = "/" + _os.path.relpath(str(tmp_path), _os.getcwd()) + "/"
    env = dict(_os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29751", WORLD_SIZE="2", OMP_NUM_THREADS="2",
               RFN_DIST_BACKEND="gloo", RFN_SINGLE_GPU="1")
    procs = [subprocess.Popen([_sys.executable, str(script), ROOT, rel], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=_os.getcwd()) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "rank %d trained, counter 2" % r in o, "rank %d failed:\n%s" % (r, o[-3000:])
    ckpt = Solver.read_checkpoint(str(tmp_path / "model_folder" / "rfn.pt"))
    assert ckpt["world_size"] == 2 and ckpt["global_batch_size"] == 4 and ckpt["args"].batch_size == 2
    sd, osd = ckpt["model_state_dict"], ckpt["optimizer_state_dict"]
    assert sd["h_0"].shape[0] == 4 and sd["z_0"].shape[0] == 4
    args1 = Solver.args_for_world(ckpt, 1)
    assert args1.batch_size == 4
    args1.multigpu = False
    s = Solver(args1)
    s.build()
    names = [n for n, _ in s.model.named_parameters()]
    assert tuple(osd["state"][names.index("h_0")]["exp_avg"].shape) == tuple(sd["h_0"].shape)   # gathered moments
    s.load(ckpt)
    for n, p in s.model.named_parameters():
        st = s.optimizer.state.get(p)
        if st:
            assert st["exp_avg"].shape == p.shape, n
    x = next(iter(s.train_loader))
    s.train_step(x.cuda())                          # HipAdam builds its table: sizes agree
    s.flush_log()
    assert s.counter == 3


def test_data_parallel_rfn_equals_single_process_global_batch(tmp_path, conv_precision):
    """two fresh processes (gloo, both on this GPU) shard a global batch of 4 sequences: after the first-step protocol of
    Solver.train_step (rank-0 ActNorm init broadcast) the averaged gradients of every shared parameter, the gradients
    of the sharded initial states (rows of rank r) and the mean loss equal a single process run on the global batch --
    except that the reference initialises ActNorm on the batch it sees, so the single process is given rank 0's
    post-init state.  The extractor / upscaler keep their default BatchNorm: the two ranks
    run it synchronised (global-batch statistics in the forward pass, rank-summed partial sums in the backward pass)."""
    if conv_precision != "mixed":
        pytest.skip("arithmetic-independent protocol: run once")
    import subprocess, sys as _sys, os as _os
    from tests.conftest import ROOT
    script = tmp_path / "dp_rfn_worker.py"
    script.write_text(_DP_RFN_WORKER)
    env = dict(_os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29741", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    out2 = str(tmp_path / "dp2")
    procs = [subprocess.Popen([_sys.executable, str(script), ROOT, out2], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "rank %d ok" % r in o, "rank %d failed:\n%s" % (r, o[-3000:])
    d0, d1 = torch.load(out2 + ".rank0", weights_only=True), torch.load(out2 + ".rank1", weights_only=True)
    # replicas agree on every shared gradient and on the gathered state
    for n, g0 in d0["grads"].items():
        if n not in ("z_0", "z_0x", "h_0", "c_0"):
            assert torch.equal(g0, d1["grads"][n]), n
    # single process on the global batch, started from the data-parallel run's post-init state
    from RFN import RFN
    args = _tiny_solver_args("/gpurun_out/tmp/", 4)
    assert args.norm_type_features == "batchnorm"
    m = RFN(args).cuda().train()
    # post-init ActNorm state of the data-parallel run, but the BatchNorm running statistics of BEFORE its steps (they do
    # not enter a training-mode forward; compared after this process took the same two forward passes)
    m.load_state_dict(d0["state"])
    g = torch.Generator().manual_seed(4)
    X = torch.rand(4, 4, 1, 16, 16, generator=g)
    for k, s_ in (("z_0", (4, 4, 4)), ("z_0x", (4, 4, 4)), ("h_0", (8, 4, 4)), ("c_0", (8, 4, 4))):
        torch.randn(4, *s_, generator=g)
    draws = []
    for _ in range(3):
        draws += [torch.randn(4, 4, 4, 4, generator=g).cuda(), torch.randn(4, 4, 4, 4, generator=g).cuda(),
                  (torch.rand(4, 1, 16, 16, generator=g) / 256).cuda()]
    xin = (X * 255 / 256 - 0.5).cuda()
    kl_fb, kl, nll = m.loss(xin, 0, draws=draws)
    (nll + 0.5 * kl_fb).backward()
    assert abs(float(nll) - d0["loss"]) <= 2e-5 * abs(float(nll))
    for n, p in m.named_parameters():
        if p.grad is None:
            continue
        ref = p.grad.detach().cpu()
        if n in ("z_0", "z_0x", "h_0", "c_0"):
            got = torch.cat([d0["grads"][n], d1["grads"][n]], 0)
        else:
            got = d0["grads"][n]
        torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-4 * float(ref.abs().max()) + 1e-7, msg=lambda s: n + ": " + s)


@pytest.mark.parametrize("name", ["plain", "smooth_resq_skip", "bair_like"])
def test_rfn_analysis_methods_vs_reference(golden, name):
    """RFN.reconstruct_elbo_gap / probability_future / param_analysis and the eval-mode loss on the GPU against the
    reference's outputs (tests/golden/rfn_analysis.pt: same weights, captured draws).  'bair_like' = C 3, overshooting
    D 2, skip conditions.  NLL / bits-per-dim quantities within 1e-4 relative."""
    from RFN import RFN
    f = golden("rfn_analysis.pt")[name]
    args = Namespace(**f["args"])
    m = load_sd(RFN(args), f["sd"]).eval()
    x = cu(f["x"])
    e = f["elbo_gap"]
    _, _, kld, nlls = m.reconstruct_elbo_gap(x, sample=False, draws=[t for _, t in e["draws"]])
    close(kld, e["kld"], 1e-4, 1e-5)
    close(nlls, e["nlls"], 1e-4, 1e-4)
    e = f["prob_future"]
    out = m.probability_future(x, e["n_conditions"], draws=[t for _, t in e["draws"]])
    close(out, e["out"], 1e-4, 1e-4)
    e = f["param_analysis"]
    out = m.param_analysis(x, e["n_predictions"], e["n_conditions"], draws=[t for _, t in e["draws"]])
    for a, b in zip(out, e["out"]):
        close(a, b, 1e-4, 1e-5)
    e = f["loss_eval"]
    out = m.loss(x, 0, draws=[t for _, t in e["draws"]])
    for a, b in zip(out, e["out"]):
        assert abs(float(a) - b) <= 1e-4 * abs(b) + 1e-5, (float(a), b)
    # sampling variants run and have the reference's shapes
    rec, rec_flow, _, _ = m.reconstruct_elbo_gap(x, sample=True)
    assert tuple(rec.shape) == (2, f["T"]) + tuple(x[:, 0].shape) and bool(torch.isfinite(rec_flow).all())


def test_evaluator_bpd_loop(golden):
    """Evaluator.get_loss (evaluation_metrics/error_metrics.py:370-417): the mean of per-batch bits/dim equals the
    oracle's restatement of that loop on the same batches and noise (eval mode), and compute_loss reproduces the
    reference's figure of the trainer fixture."""
    from RFN import RFN
    from RFN.trainer import Solver
    from evaluation_metrics import Evaluator
    args = _tiny_solver_args("/gpurun_out/tmp/")
    torch.manual_seed(3)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.model = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(8)
    batches = [torch.rand(2, 4, 1, 16, 16, generator=g) for _ in range(3)]
    with torch.no_grad():
        s.model.loss(s.preprocess(batches[0].cuda()), 0)       # data dependent init
    ev = Evaluator(s)
    gfix = golden("trainer.pt")["compute_loss"]
    b, k, n = ev.compute_loss(gfix["nll"], gfix["kl"], gfix["dims"], gfix["t"])
    assert abs(b - gfix["bits"]) <= 1e-6 * abs(gfix["bits"])
    # the loop itself against the ORACLE's restatement of error_metrics.py:370-417 (not against this
    # repo's own RFN.loss): eval mode, the same three batches, the noise of every batch pinned on both sides
    gd = torch.Generator().manual_seed(12)
    draws_list = []
    for xb in batches:
        d = []
        for _ in range(xb.shape[1] - 1):
            d += [torch.randn(2, args.z_dim, 4, 4, generator=gd), torch.randn(2, args.z_dim, 4, 4, generator=gd),
                  torch.rand(2, 1, 16, 16, generator=gd) / 256]
        draws_list.append(d)
    pending = [list(d) for d in draws_list]
    plain_loss = s.model.loss
    s.model.loss = lambda xin, logdet=0: plain_loss(xin, logdet, draws=[t.cuda() for t in pending.pop(0)])
    try:
        mean, std = ev.get_loss("rfn.pt", 1, loader=batches)
    finally:
        del s.model.loss
    assert std == -1 and not pending
    sd = {k: v.detach().cpu().clone() for k, v in s.model.state_dict().items()}
    ref = O.evaluator_get_loss(sd, vars(args), batches, draws_list, n_trained=args.n_frames, n_bits=args.n_bits)
    assert abs(float(mean) - float(ref)) <= 1e-4 * abs(float(ref)), (float(mean), float(ref))


@pytest.mark.parametrize("name", ["plain", "smooth_resq_skip", "bair_like"])
def test_rfn_generation_methods_vs_reference(golden, name):
    """RFN.predict / reconstruct / sample on the GPU (reverse Glow steps through the fused kernel where it applies)
    against the reference's outputs with the captured draws.  Autoregressive: a frame feeds the next one, tolerance 1e-4
    of the image range."""
    from RFN import RFN
    f = golden("rfn_analysis.pt")[name]
    args = Namespace(**f["args"])
    m = load_sd(RFN(args), f["sd"]).eval()
    x = cu(f["x"])
    e = f["predict"]
    tx, pr = m.predict(x, e["n_predictions"], e["n_conditions"], draws=[t for _, t in e["draws"]])
    assert torch.equal(tx, e["true_x"])
    close(pr, e["predictions"], 1e-4, 1e-5)
    e = f["reconstruct"]
    rc, rcf = m.reconstruct(x, draws=[t for _, t in e["draws"]])
    close(rc, e["recons"], 1e-4, 1e-5)
    close(rcf, e["recons_flow"], 1e-4, 1e-5)
    e = f["sample"]
    sm = m.sample(x, e["n_samples"], draws=[t for _, t in e["draws"]])
    close(sm, e["samples"], 1e-4, 1e-5)


@pytest.mark.parametrize("C,Cc,S", [(12, 32, 32), (24, 64, 16), (48, 128, 8), (96, 256, 4)])
def test_glowstep_bair_channel_counts(conv_precision, C, Cc, S):
    """BASELINE config 5 (BAIR: C = 3, L = 4 -> 12 / 24 / 48 / 96 channels per level, Hd = 256, skip conditions) at the
    full channel counts of every level: forward values and log-det against the CPU oracle, and the reverse step inverts
    the forward one (x -> y -> x, log-dets cancel).  Tolerances: 1e-4 of the tensor's range (forward), 2e-4 round trip."""
    from Flow import GlowStep
    from tests.golden_args import GLOW_DEFAULTS
    a = dict(GLOW_DEFAULTS)
    a["n_units_affine"] = 256
    N = 4
    torch.manual_seed(31)
    gs = GlowStep([N, C, S, S], [N, Cc, S, S], glow_ns(a)).cuda().train()
    g = torch.Generator().manual_seed(32)
    x0 = torch.randn(N, C, S, S, generator=g)
    c0 = torch.randn(N, Cc, S, S, generator=g)
    gs(cu(x0), cu(c0), torch.zeros(N, device="cuda"), False)  # data dependent init
    with torch.no_grad():
        for prm in gs.parameters():
            prm.add_(0.03 * torch.randn(prm.shape, generator=g).cuda())
    gs.eval()
    with torch.no_grad():
        y, ld = gs(cu(x0), cu(c0), torch.zeros(N, device="cuda"), False)
        sd = {k: v.detach().cpu().clone() for k, v in gs.state_dict().items()}
        yo, ldo = O.glowstep(sd, "", x0, c0, torch.zeros(N), False, False)
        close(y, yo, 1e-4, 1e-5)
        close(ld, ldo, 1e-4, 1e-4)
        xb, ldb = gs(y, cu(c0), ld.clone(), True)
        close(xb, x0, 2e-4, 2e-5)
        assert float(ldb.abs().max()) <= 2e-4 * float(ld.abs().max()) + 1e-3


@pytest.mark.parametrize("N,C,Cc,S,Hd,Kn,clamp", [(2, 4, 16, 32, 256, 3, "realnvp"), (3, 8, 32, 16, 256, 2, "glow"),
                                               (5, 16, 8, 8, 64, 3, "realnvp"), (4, 32, 16, 4, 64, 2, "softclamp"),
                                               (6, 64, 32, 2, 64, 3, "realnvp"), (3, 6, 0, 4, 64, 2, "none"),
                                               # K = 1: head launch, net, tail launch; backward without a shell launch
                                               (2, 4, 8, 4, 64, 1, "realnvp"),
                                               # the carried clamp-parameter gradients without condition channels
                                               (2, 6, 0, 4, 64, 3, "realnvp")])
def test_glow_level_node_equals_chain_of_step_nodes(conv_precision, N, C, Cc, S, Hd, Kn, clamp):
    """rfn_hip.ops.GlowLevelFn (the K steps of a level as one autograd node, shell work fused across step boundaries:
    rfn_glow_shell_fwd_f32 / rfn_glow_shell_bwd_f32) against K chained GlowStepFn nodes -- outputs, log-det and every
    gradient (input, shared condition, InvConv matrices, all step parameters).  The convolutions inside are the same
    kernels on both sides, so the tolerance is that of fp32 sums in a different order: 1e-5 / 1e-4 of the range."""
    from rfn_hip import ops as K
    g = torch.Generator().manual_seed(40 + C)
    Ch = C // 2
    rn = clamp == "realnvp"

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda().requires_grad_(True)

    x = leaf(N, C, S, S)
    cond = leaf(N, Cc, S, S)
    Wst = (torch.eye(C).expand(Kn, C, C) + 0.2 * torch.randn(Kn, C, C, generator=g)).cuda().requires_grad_(True)
    steps = []
    for _ in range(Kn):
        steps.append([leaf(1, C, 1, 1, scale=0.1), leaf(1, C, 1, 1, scale=0.1),                      # actnorm
                      leaf(Hd, Ch + Cc, 3, 3, scale=0.05), leaf(1, Hd, 1, 1, scale=0.1), leaf(1, Hd, 1, 1, scale=0.1),
                      leaf(Hd, Hd, 1, 1, scale=0.05), leaf(1, Hd, 1, 1, scale=0.1), leaf(1, Hd, 1, 1, scale=0.1),
                      leaf(C, Hd, 3, 3, scale=0.02), leaf(C, scale=0.1), leaf(C, 1, 1, scale=0.1),
                      leaf(Ch, 1, 1, scale=0.5) if rn else None, leaf(Ch, 1, 1, scale=0.1) if rn else None])
    act, ct = K.ACT["leakyrelu"], K.CLAMP[clamp]
    gout = torch.randn(N, C, S, S, generator=g).cuda()
    gdl = torch.randn(N, generator=g).cuda()
    leaves = [x, cond, Wst] + [t for st in steps for t in st if t is not None]

    def run(level):
        for t in leaves:
            t.grad = None
        if level:
            out, dl = K.GlowLevelFn.apply(x, cond, Wst, act, ct, None, *[t for st in steps for t in st])
        else:
            out, dl = x, 0
            for k in range(Kn):
                out, d = K.GlowStepFn.apply(out, cond, Wst[k], *steps[k], act, ct, None)
                dl = dl + d + steps[k][1].sum() * (S * S)  # the level node includes the ActNorm term H*W * sum logs
        ((out * gout).sum() + (dl * gdl).sum()).backward()
        return out.detach().clone(), dl.detach().clone(), [t.grad.detach().clone() for t in leaves]

    o_ref, d_ref, g_ref = run(False)
    o_lv, d_lv, g_lv = run(True)
    close(o_lv, o_ref.cpu(), 1e-5, 1e-6)
    close(d_lv, d_ref.cpu(), 1e-5, 1e-5)
    for a, b in zip(g_lv, g_ref):
        assert a.shape == b.shape
        close(a, b.cpu(), 1e-4, 1e-6)


@pytest.mark.parametrize("N,C,Cc,S,Kn,act", [(3, 4, 16, 32, 2, "relu"), (2, 8, 32, 16, 3, "leakyrelu")])
def test_fused_backward_chain_equals_unfused_backward(conv_precision, N, C, Cc, S, Kn, act, monkeypatch):
    """the level node with the fused coupling-net backward (rfn_coupling_po_bwd: one kernel from the forward kernel's
    activation masks, ActNorm gradients from the weight gradients) against the same node with RFN_COUPLING_PO_BWD=0 (two
    data-gradient kernels that read h1 / h2 and sum g*y themselves): every gradient -- input, condition, InvConv
    matrices, all 13 parameters of every step -- within the gradients' tolerance (the two paths use different split
    arithmetics: f16x3s vs bf16x3).  Covers the A/B switch the product keeps (switches multiply paths)."""
    if conv_precision != "mixed":
        pytest.skip("the fused kernels are the path of the 'mixed' arithmetic")
    from rfn_hip import ops as K
    g = torch.Generator().manual_seed(90 + C)
    Ch, Hd = C // 2, 256

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda().requires_grad_(True)

    x, cond = leaf(N, C, S, S), leaf(N, Cc, S, S)
    Wst = (torch.eye(C).expand(Kn, C, C) + 0.2 * torch.randn(Kn, C, C, generator=g)).cuda().requires_grad_(True)
    steps = []
    for _ in range(Kn):
        steps.append([leaf(1, C, 1, 1, scale=0.1), leaf(1, C, 1, 1, scale=0.1),
                      leaf(Hd, Ch + Cc, 3, 3, scale=0.05), leaf(1, Hd, 1, 1, scale=0.1), leaf(1, Hd, 1, 1, scale=0.1),
                      leaf(Hd, Hd, 1, 1, scale=0.05), leaf(1, Hd, 1, 1, scale=0.1), leaf(1, Hd, 1, 1, scale=0.1),
                      leaf(C, Hd, 3, 3, scale=0.02), leaf(C, scale=0.1), leaf(C, 1, 1, scale=0.1),
                      leaf(Ch, 1, 1, scale=0.5), leaf(Ch, 1, 1, scale=0.1)])
    plan = K.POPackPlan([(st[2].detach(), st[5].detach(), st[8].detach()) for st in steps])
    plan.run()
    assert all(b is not None for b in plan.bwd_bufs) and K.coupling_po_bwd_ok(N, C, S, S)
    packs = [K.StepPacks(po_fwd=plan.bufs[k], po_bwd=plan.bwd_bufs[k]) for k in range(Kn)]
    gout = torch.randn(N, C, S, S, generator=g).cuda()
    gdl = torch.randn(N, generator=g).cuda()
    leaves = [x, cond, Wst] + [t for st in steps for t in st]

    def run(fused):
        monkeypatch.setenv("RFN_COUPLING_PO_BWD", "1" if fused else "0")
        for t in leaves:
            t.grad = None
        out, dl = K.GlowLevelFn.apply(x, cond, Wst, K.ACT[act], K.CLAMP["realnvp"], packs, *[t for st in steps for t in st])
        ((out * gout).sum() + (dl * gdl).sum()).backward()
        return out.detach().clone(), [t.grad.detach().clone() for t in leaves]

    o0, g0 = run(False)
    o1, g1 = run(True)
    assert torch.equal(o0, o1)          # the forward pass is the same launches either way (and bit-reproducible)
    for a, b in zip(g1, g0):
        close(a, b.cpu(), 2e-3, 1e-7)


@pytest.mark.parametrize("C,Kn,hw", [(4, 10, 1024), (64, 3, 4), (24, 16, 64), (96, 2, 64), (6, 3, 16)])
def test_invconv_weights_kernel_equals_torch_algebra(conv_precision, C, Kn, hw, monkeypatch):
    """rfn_invconv_weights_{fwd,bwd}_f32 (InvConv.get_weight of the K steps of a level, glow_modules.py:178-207, in one
    launch each way) against the batched torch restatement of the same algebra: W, the log-det scalar, and the gradients
    of lower / upper / log_s for a random gW and scalar gradient."""
    if conv_precision != "mixed":
        pytest.skip("arithmetic-independent: run once")
    from Flow.glow import ListGlow
    from Flow.glow_modules import InvConv
    from types import SimpleNamespace
    torch.manual_seed(60 + C)
    ics = [InvConv(C, LU_decomposed=True).cuda() for _ in range(Kn)]
    with torch.no_grad():
        for ic in ics:  # away from the orthogonal init: generic triangular factors
            ic.lower.add_(0.3 * torch.randn_like(ic.lower)); ic.upper.add_(0.3 * torch.randn_like(ic.upper))
            ic.log_s.add_(0.2 * torch.randn_like(ic.log_s))
    steps = [SimpleNamespace(invconv=ic, flow_norm="actnorm") for ic in ics]
    g = torch.Generator().manual_seed(61)
    gW, gc = torch.randn(Kn, C, C, generator=g).cuda(), 1.7

    def run(kernel):
        monkeypatch.setenv("RFN_INVCONV_KERNEL", "1" if kernel else "0")
        for ic in ics:
            ic.zero_grad(set_to_none=True)
        W, c = ListGlow._batched_invconv(steps, hw)
        ((W * gW).sum() + gc * c).backward()
        return [W.detach().clone(), c.detach().clone()] + [p.grad.clone() for ic in ics for p in (ic.lower, ic.upper, ic.log_s)]
    ref, got = run(False), run(True)
    for a, b in zip(got, ref):
        close(a, b.cpu(), 2e-5, 1e-6)
    # structure: nothing leaks outside the triangles
    assert float(ics[0].lower.grad.triu().abs().max()) == 0.0 and float(ics[0].upper.grad.tril().abs().max()) == 0.0


def test_baseline_config_unconditional_glow_32x32(conv_precision):
    """BASELINE.json configs[1]: unconditional Glow on 32x32x3 images, K=8, L=3 (ListGlow with zero-channel conditions,
    make_conditional=False, learn_prior=False), Hd=256, at its real size: data dependent init + steady-state
    log-likelihood against the CPU oracle on the same weights and dequantisation noise (<= 1e-4 relative per sample),
    gradients flow, and sample() from the same z with pinned Split2d draws matches the oracle's."""
    from Flow import ListGlow
    from tests.golden_args import GLOW_DEFAULTS
    a = dict(GLOW_DEFAULTS, L=3, K=8, n_units_affine=256, make_conditional=False, learn_prior=False,
             non_lin_glow="leakyrelu")
    B, C, S = 4, 3, 32
    torch.manual_seed(51)
    conds_sz = [[B, 0, S >> (l + 1), S >> (l + 1)] for l in range(3)]
    flow = ListGlow([B, C, S, S], conds_sz, (B, 0, S >> 3, S >> 3), glow_ns(a)).cuda().train()
    g = torch.Generator().manual_seed(52)
    x = (torch.rand(B, C, S, S, generator=g) * 255).floor() / 256 - 0.5
    noise = torch.rand(B, C, S, S, generator=g) / 256
    conds = [torch.zeros(*sz) for sz in conds_sz]
    base = torch.zeros(B, 0, S >> 3, S >> 3)
    cc = [cu(c) for c in conds]
    flow.log_prob(cu(x), cc, cu(base), 0, noise=cu(noise))         # first call: ActNorm init
    with torch.no_grad():
        for prm in flow.parameters():
            prm.add_(0.01 * torch.randn(prm.shape, generator=g).cuda())
    z, nll = flow.log_prob(cu(x), cc, cu(base), 0, noise=cu(noise))
    sd = {k: v.detach().cpu().clone() for k, v in flow.state_dict().items()}
    with torch.no_grad():
        zo, nllo = O.listglow_log_prob(sd, "", a, x, conds, base, 0, noise, True)
    close(z, zo, 1e-4, 1e-4)
    nll_rel(nll, nllo)
    nll.mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in flow.parameters())
    flow.eval()
    with torch.no_grad():   # generation at this size (the Split2d levels draw fresh z2: not an inversion of log_prob)
        eps = [torch.randn(B, 6 * 2 ** l, S >> (l + 1), S >> (l + 1), generator=g) for l in (1, 0)]  # coarsest first
        xs = flow.sample(z.detach(), cc, cu(base), eps_list=[cu(e) for e in eps])
        xo = O.listglow_sample(sd, "", a, z.detach().cpu(), conds, base, eps_list=eps)
    close(xs, xo, 2e-4, 2e-5)


def test_baseline_config_bair_shaped_rfn(conv_precision):
    """BASELINE.json configs[4]: RFN on BAIR-shaped video -- C=3, 64x64, L=4, K=16, Hd=256, skip conditions in the flow
    (`with_skip`), overshooting D=2 -- one training loss at its real widths (B=2, T=3) against the CPU oracle with pinned
    draws: KL, NLL and bits/dim within 1e-4 relative; backward runs (grouped weight gradients with K = 16 groups)."""
    import main_rfn
    from RFN import RFN
    argv = ("--extractor_structure 32-32-pool-64 64-pool-128 128-pool-256 256-pool-512 "
            "--upscaler_structure 256 upsample-128-128 upsample-64-64 upsample-32-32 "
            "--prior_structure 256 256 --encoder_structure 256 256 --make_conditional --learn_prior "
            "--skip_connection_features --flow_norm actnorm --structure_scaler 2 --choose_data bair "
            "--n_units_affine 256 --n_units_prior 256 --temperature 0.7 --norm_type none --z_dim 32 --h_dim 128 "
            "--n_bits 8 --n_frames 3 --image_size 64 --K 16 --L 4 --D 2 --overshot_w 0.5 "
            "--x_dim 2 3 64 64 --condition_dim 2 3 64 64 --batch_size 2 "
            "--skip_connection_flow with_skip --no-upscaler_tanh --no-downscaler_tanh --synthetic_data").split()
    args = main_rfn.build_parser().parse_args(argv)
    B, T = 2, 3
    torch.manual_seed(61)
    m = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(62)
    x = (torch.rand(B, T, 3, 64, 64, generator=g) * 255).floor() / 256 - 0.5
    hu = 64 >> 4
    zshape = (B, args.z_dim, hu, hu)

    def draws():
        gg = torch.Generator().manual_seed(63)
        d = []
        for _ in range(T - 1):
            d += [torch.randn(zshape, generator=gg), torch.randn(zshape, generator=gg),
                  torch.rand(B, 3, 64, 64, generator=gg) / 256]
        for _ in range(8):                      # overshooting prior draws (more than needed is fine)
            d.append(torch.randn(zshape, generator=gg))
        return d
    with torch.no_grad():
        m.loss(cu(x), 0, draws=draws())       # data dependent init
        for prm in m.flow.parameters():
            prm.add_(0.003 * torch.randn(prm.shape, generator=g).cuda())
    kl_fb, kl, nll = m.loss(cu(x), 0, draws=draws())
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    want_grads = conv_precision == "mixed"     # the oracle's backward at these widths: once, for the shipped arithmetic
    leaves = {}
    if want_grads:
        for n_, _ in m.named_parameters():
            sd[n_].requires_grad_(True)
            leaves[n_] = sd[n_]
    with torch.set_grad_enabled(want_grads):
        r = O.rfn_loss(sd, vars(args), x, draws(), True)
    for a_, b_ in zip((kl_fb, kl, nll), r):
        assert abs(float(a_) - float(b_)) <= 1e-4 * abs(float(b_)) + 1e-5, (float(a_), float(b_))
    bpd = O.bits_per_dim(kl.detach().cpu(), nll.detach().cpu(), x.shape[2:], T - 1)
    bpd_o = O.bits_per_dim(r[1].detach(), r[2].detach(), x.shape[2:], T - 1)
    assert abs(bpd - bpd_o) <= 1e-4 * abs(bpd_o)
    (nll + 0.5 * kl_fb).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    assert sum(p.grad is not None for p in m.flow.parameters()) > 0
    if want_grads:
        # gradients at BAIR widths against the oracle, not only finite.  Norm-wise per tensor (at Hd = 256 on
        # 64x64 maps a handful of activations sit within the arithmetic's distance of the ReLU kink and flip, DESIGN.md
        # section 2): ||g - g_ref|| <= 5e-3 ||g_ref||, tensors whose reference gradient is numerically zero excepted
        (r[2] + 0.5 * r[0]).backward()
        errs = {}
        for n_, p in m.named_parameters():
            gref = leaves[n_].grad
            if gref is None or p.grad is None:
                continue
            nr = float(gref.norm())
            if nr < 1e-12:
                continue
            errs[n_] = float((p.grad.detach().cpu() - gref).norm()) / nr
        assert len(errs) > 500
        worst = max(errs, key=errs.get)
        ranked = sorted(errs.values())
        print("BAIR-width gradient errors: median %.2e  95%% %.2e  max %.2e (%s)" % (
            ranked[len(ranked) // 2], ranked[int(0.95 * len(ranked))], errs[worst], worst))
        # with only 4 frames in the batch one flipped activation is a visible share of a layer's gradient -- most of all
        # at the deepest level (4 frames x 16 pixels: measured worst 1.75e-2 on its last coupling net) -- so the typical
        # tensor must sit at the arithmetic's level (measured: median 1.3e-4, 95 % 1.4e-3) and the worst within 3e-2
        assert ranked[len(ranked) // 2] <= 1e-3 and ranked[int(0.95 * len(ranked))] <= 5e-3 and errs[worst] <= 3e-2, \
            (worst, errs[worst])
