"""The fused f16x3s coupling-net kernels (csrc/coupling_po.hip) at real magnitudes and at their size limits.

coupling_po_fwd_kernel (forward of the coupling net at flow levels 0-2 and BAIR level 0) and its BWD instantiation (the
data-gradient chain) compute on two fp16 pieces per operand after exact power-of-two scalings taken from the data:
one per convolution for the weights (max|w|), one per 128-pixel round for the image of conv1 (halo included), a
per-pixel running maximum for h1 (the conv2 partial sums are rescaled when quad 1 raises it) and a per-pixel maximum
over all 256 channels for h2.  test_hip_kernels feeds them unit-scale randn data only; here every scaling path is forced.

1. Stage-wise fp64 references.  Each stage is recomputed in fp64 on the CPU from what the GPU actually fed it: h1 from
   (z1 | cond), h2 from the GPU's h1, P from the GPU's h2 (its contract P[n, tap*C+co] = sum_c w3[co][c][tap] h2[c]),
   ga2 from go, ga1 from the GPU's ga2, and the four ActNorm gradients of rfn_coupling_po_bwd_finish from the GPU's
   ga1 / ga2 and fp64 weight gradients.  The activation branch of a reference is the one the GPU took (h > 0); it may
   differ from the fp64 pre-activation only inside the error band TOL * S of that element.
   Error measure: e_abs = max |y - y64| / S with S the fp64 sum of |a|*|b| of the element's dot product, plus |bias|,
   times exp(logs) of its channel (times |act'| for a gradient).  It does not punish conditioning the model creates.
   Floor model: x * 2^e = hi + lo with the scaled group maximum in [2^14, 2^15).  An element more than ~2^17 below its
   group maximum m has a subnormal fp16 lo piece, so its representation error is absolute, 2^-39 * m if fp16 subnormals
   survive the conversion and the MFMA (2^-28 * m if they were flushed), instead of 2^-22 relative.  In S every operand
   |x| of a product therefore counts as |x| + PHI * m with PHI = 2^-17 (the subnormal-preserving model): for the image
   of conv1 (m = the round's maximum, halo included) and for every weight (m = max|w| of the convolution).  conv2 and
   conv3 are per-pixel 1x1 products whose S always contains the element that set the h scale; no floor term there.
2. Magnitude scenarios (SCENARIOS), each with a CPU-side assertion that its inputs or the fp64 reference really are in
   the regime it names, over the four forward instantiations (NG, NP, W) = (3,2,32) (5,3,16) (9,5,8) (9,4,32) and the
   four backward ones (NG 1 at W 32 / 16, NG 2 at W 8 / 32), with ReLU and LeakyReLU.
3. Exact power-of-two equivariance, bit for bit: inputs and biases x 2^k, (w2, n2b) x 2^k, go x 2^k.
4. Forward and backward at the largest frame count each size predicate accepts (32-bit buffer offsets).

Measured on an MI355X, e_abs as the maximum over the instantiations of a scenario (forward h1 / h2 / P, backward
ga2 / ga1, the four ActNorm gradients of the finishing launch):
    actnorm_init           2.5e-7  2.4e-7  2.9e-8      w3_zero                2.6e-7  0 (exact)  0
    rescale_forced         3.0e-7  3.6e-7  4.0e-8      w3_1e-4                2.6e-7  2.9e-7  2.7e-8
    rescale_never          3.5e-7  2.6e-7  5.3e-8      go 1e-7, w3 1e-3       3.4e-7  2.6e-7  3.6e-8
    quad0_dead             2.8e-7  2.8e-7  3.5e-8      go 1e-9, w3 1e-4       2.8e-7  2.8e-7  2.7e-8
    zero_rounds            2.7e-7  2.7e-7  3.9e-8      go 1e4                 3.4e-7  2.8e-7  2.7e-8
    halo_spike             4.2e-7  2.3e-7  3.7e-8      hetero_cond            5.3e-7  2.8e-7  1.3e-7
    frames_of_round 2^10   2.4e-7  2.3e-7  3.9e-8      digit_background       4.0e-7  4.4e-7  4.5e-8
    frames_of_round 2^20   2.6e-7  2.3e-7  3.3e-8      size limit (8 frames)  2.9e-7  3.0e-7  --
Subnormal floor: conv1 outputs (zero ActNorm bias) whose whole image neighbourhood sits >= 2^19 below the round maximum
(digit_background, frames_of_round 2^20) show e_abs 1.4-2.4e-6 WITHOUT the floor term in S -- the 2^-19 relative error
of the subnormal-preserving model for values 2^-20 m, where flushed fp16 subnormals would leave ~2^-8 (and an fp32
rounding of the same references, without the split, 1-2e-8).  So fp16 subnormals survive the conversion and the MFMA
on gfx950, the floor is 2^-39 * m, and the test holds that (E_FLOOR <= 2^-17).  With the floor term those outputs stay
at the fp32-grade figures above.  TOL = 1e-6: about twice the largest of them.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PHI = 2.0 ** -17   # floor of the f16x3s split in units of the scale group's maximum (see the docstring)
TOL = 1e-6         # e_abs bound of every stage (fp32-grade)

# (C, Cc, S): the nets whose forward / backward run on the fused kernels
LEVELS = {"L0": (4, 16, 32), "L1": (8, 32, 16), "L2": (16, 64, 8), "BAIR0": (12, 64, 32)}
FRAMES = {32: 2, 16: 4, 8: 8}   # frames per scenario: 16 / 8 / 4 rounds
RELU, LEAKY = 1, 2


@pytest.fixture(autouse=True)
def mixed(monkeypatch):
    from rfn_hip import ops
    monkeypatch.setattr(ops, "CONV_PRECISION", "mixed")


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    assert torch.cuda.is_available(), "GPU tests need a device"
    return ops


def instance(C, Cc, S):
    """(NG, NP, W) of the forward kernel and (NG, W) of the backward kernel this net runs on"""
    return ((C // 2 + Cc + 7) // 8, (9 * C + 31) // 32, S), ((C + 7) // 8, S)


def test_levels_cover_every_instantiation():
    fwd = {instance(*lv)[0] for lv in LEVELS.values()}
    bwd = {instance(*lv)[1] for lv in LEVELS.values()}
    assert fwd == {(3, 2, 32), (5, 3, 16), (9, 5, 8), (9, 4, 32)}
    assert bwd == {(1, 32), (1, 16), (2, 8), (2, 32)}


# --------------------------------------------------------------------------------------------- fp64 references
def slope_of(act):
    return 0.0 if act == RELU else 0.2


def actf(act, y):
    return F.relu(y) if act == RELU else F.leaky_relu(y, 0.2)


def round_max(x):
    """per output pixel [N,1,S,S]: max |x| over the haloed image of its 128-pixel round, all channels (conv1's input
    scale group).  S >= 16: 128/S rows of one frame plus the row above and below; 8x8: two whole frames."""
    N, _, S, _ = x.shape
    rows = x.abs().amax(dim=(1, 3))   # [N, S]
    if S * S >= 128:
        R = 128 // S
        m = torch.empty(N, S, dtype=rows.dtype)
        for j in range(S // R):
            m[:, j * R:(j + 1) * R] = rows[:, max(j * R - 1, 0):min(j * R + R + 1, S)].amax(1, keepdim=True)
        return m.view(N, 1, S, 1).expand(N, 1, S, S)
    fpr = 128 // (S * S)
    m = rows.amax(1).view(N // fpr, fpr).amax(1).repeat_interleave(fpr)
    return m.view(N, 1, 1, 1).expand(N, 1, S, S)


def conv1_ref(x, w, phi=PHI):
    """fp64 3x3 convolution y = conv(x, w) and its S with the floor terms of the image (per round) and the weights:
    S = sum (|w| + phi max|w|) (|x| + phi m_round) over the taps inside the frame"""
    x, w = x.double(), w.double()
    ax, aw = x.abs(), w.abs()
    ones_x, ones_w = torch.ones_like(x), torch.ones_like(w)
    mw, mr = float(aw.max()), round_max(x)
    y = F.conv2d(x, w, padding=1)
    s = (F.conv2d(ax, aw, padding=1) + phi * mw * F.conv2d(ax, ones_w, padding=1)
         + phi * mr * (F.conv2d(ones_x, aw, padding=1) + phi * mw * F.conv2d(ones_x, ones_w, padding=1)))
    return y, s


def pix_ref(x, w2d, phi=PHI):
    """fp64 per-pixel product y[r] = sum_c w2d[r][c] x[c] and S = sum (|w| + phi max|w|) |x|"""
    x, w = x.double(), w2d.double()
    y = F.conv2d(x, w[:, :, None, None])
    s = F.conv2d(x.abs(), (w.abs() + phi * float(w.abs().max()))[:, :, None, None])
    return y, s


def ch(v):
    return v.double().view(1, -1, 1, 1)


def e_abs(y, ref, s):
    d = (y.detach().cpu().double() - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return math.inf
    return float((d / (s + 1e-300)).max())


def branch_like_gpu(y, h_gpu, s_tot, act):
    """the activation derivative the GPU took (h > 0: linear), allowed to differ from the fp64 pre-activation y only
    within the error band TOL * S of that element"""
    on = h_gpu.detach().cpu() > 0
    flips = on != (y > 0)
    assert not bool((flips & (y.abs() > TOL * s_tot)).any()), int(flips.sum())
    return torch.where(on, 1.0, slope_of(act)).double()


def stage_errors(d, g, act, bwd=True):
    """e_abs of every stage of the forward (h1, h2, P) and backward (ga2, ga1) kernels; inputs of each stage as the GPU
    fed them.  d: CPU inputs, g: GPU outputs (CPU copies)"""
    C = d["C"]
    Ch = C // 2
    e = {}
    xin = torch.cat((d["z"][:, :Ch], d["cond"]), 1)
    a1, s1 = conv1_ref(xin, d["w1"])
    ex1 = ch(d["n1l"].exp())
    y1, s1 = (a1 + ch(d["n1b"])) * ex1, (s1 + ch(d["n1b"]).abs()) * ex1
    d1 = branch_like_gpu(y1, g["h1"], s1, act)
    e["h1"] = e_abs(g["h1"], d1 * y1, s1)
    h1g = g["h1"].double()
    a2, s2 = pix_ref(h1g, d["w2"].view(256, 256))
    ex2 = ch(d["n2l"].exp())
    y2, s2 = (a2 + ch(d["n2b"])) * ex2, (s2 + ch(d["n2b"]).abs()) * ex2
    d2 = branch_like_gpu(y2, g["h2"], s2, act)
    e["h2"] = e_abs(g["h2"], d2 * y2, s2)
    w3t = d["w3"].permute(2, 3, 0, 1).reshape(9 * C, 256)   # row tap*C + co
    p, s3 = pix_ref(g["h2"], w3t)
    e["P"] = e_abs(g["P"], p, s3)
    if not bwd:
        return e
    gh2, sg2 = conv1_ref(d["go"], d["w3"].transpose(0, 1).flip(2, 3))   # conv3^T as a 3x3 convolution
    e["ga2"] = e_abs(g["ga2"], gh2 * d2 * ex2, sg2 * d2.abs() * ex2)
    gh1, sg1 = pix_ref(g["ga2"], d["w2"].view(256, 256).t())
    e["ga1"] = e_abs(g["ga1"], gh1 * d1 * ex1, sg1 * d1.abs() * ex1)
    return e


def finish_errors(K, d, g):
    """rfn_coupling_po_bwd_finish on the GPU's per-workgroup sums and fp64 weight gradients (rounded to fp32) against
    gnb = sum over pixels of ga, gnl = sum_k w gw + nb gnb in fp64"""
    C = d["C"]
    xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1).double()
    ga1, ga2 = g["ga1"].double(), g["ga2"].double()
    gw1 = torch.nn.grad.conv2d_weight(xin, tuple(d["w1"].shape), ga1, padding=1).float()
    gw2 = torch.nn.grad.conv2d_weight(g["h1"].double(), (256, 256, 1, 1), ga2).float()
    out = torch.empty((4, 256), device="cuda")
    t = [g["part_dev"], d["w1"].cuda(), gw1.cuda(), d["n1b"].cuda(), d["w2"].cuda(), gw2.cuda(), d["n2b"].cuda(), out]
    K.coupling_po_bwd_finish([t])
    torch.cuda.synchronize()
    out = out.cpu()
    e = {}
    for i, (ga, w, gw, nb) in enumerate(((ga1, d["w1"], gw1, d["n1b"]), (ga2, d["w2"], gw2, d["n2b"]))):
        w, gw, nb = w.double().view(256, -1), gw.double().view(256, -1), nb.double()
        gb, sb = ga.sum(dim=(0, 2, 3)), ga.abs().sum(dim=(0, 2, 3))
        gl, sl = (w * gw).sum(1) + nb * gb, (w * gw).abs().sum(1) + nb.abs() * sb
        e["gnb%d" % (i + 1)] = e_abs(out[2 * i], gb, sb)
        e["gnl%d" % (i + 1)] = e_abs(out[2 * i + 1], gl, sl)
    return e


def fp64_forward(d, act):
    """h1, h2 of the whole net in fp64 from the inputs alone (for the regime assertions)"""
    C = d["C"]
    xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1).double()
    h1 = actf(act, (F.conv2d(xin, d["w1"].double(), padding=1) + ch(d["n1b"])) * ch(d["n1l"].exp()))
    h2 = actf(act, (F.conv2d(h1, d["w2"].double()) + ch(d["n2b"])) * ch(d["n2l"].exp()))
    return h1, h2


def gpu_run(K, d, act, bwd=True):
    """forward (with masks) and backward of the fused kernels on inputs d; CPU copies of every output"""
    C = d["C"]
    dev = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
    plan = K.POPackPlan([(dev["w1"], dev["w2"], dev["w3"])])
    plan.run()
    h1, h2, P, masks = K.coupling_po_fwd(dev["z"], dev["cond"], plan.bufs[0], dev["n1b"], dev["n1l"], dev["n2b"],
                                         dev["n2l"], C, act, want_masks=True)
    out = {"h1": h1, "h2": h2, "P": P, "m1": masks[0], "m2": masks[1]}
    if bwd:
        ga2, ga1, part = K.coupling_po_bwd(dev["go"], plan.bwd_bufs[0], dev["n1l"], dev["n2l"], masks, act)
        out.update(ga2=ga2, ga1=ga1, part=part, part_dev=part)
    torch.cuda.synchronize()
    res = {k: (v.cpu() if k != "part_dev" else v) for k, v in out.items()}
    return res


# --------------------------------------------------------------------------------------------- scenarios
def base_net(C, Cc, S, N, seed, w3_scale=0.05):
    g = torch.Generator().manual_seed(seed)
    Cin = C // 2 + Cc
    return {
        "C": C, "g": g,
        "z": torch.randn(N, C, S, S, generator=g), "cond": torch.randn(N, Cc, S, S, generator=g),
        "w1": torch.randn(256, Cin, 3, 3, generator=g) * 0.05, "w2": torch.randn(256, 256, 1, 1, generator=g) * 0.05,
        "w3": torch.randn(C, 256, 3, 3, generator=g) * w3_scale,
        "n1b": torch.randn(256, generator=g) * 0.1, "n1l": torch.randn(256, generator=g) * 0.1,
        "n2b": torch.randn(256, generator=g) * 0.1, "n2l": torch.randn(256, generator=g) * 0.1,
        "go": torch.randn(N, C, S, S, generator=g),
    }


def log2_floor(t):
    """floor(log2 |t|) elementwise (-inf at 0)"""
    return torch.floor(torch.log2(t.abs().double()))


def blobs(N, Cn, S, g, n_blobs, amp):
    """sparse images: a few Gaussian blobs of amplitude ~amp on zero background"""
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    out = torch.zeros(N, Cn, S, S)
    for n in range(N):
        for _ in range(n_blobs):
            cy, cx = (torch.rand(2, generator=g) * S).tolist()
            r = 0.6 + 1.4 * float(torch.rand(1, generator=g))
            bump = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
            out[n] += bump * (amp * torch.randn(Cn, 1, 1, generator=g))
    return out


def sc_actnorm_init(C, Cc, S, act):
    """Sparse frames (constant background plus a few blobs, a third of the cond channels constant) and weight rows
    spread over six decades below max|w|; the ActNorm parameters come from the reference's data dependent init
    (bias = -mean, logs = log(1/(std+1e-6)), unbiased std) on the fp64 conv1 / conv2 outputs."""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 101 + S + C)
    g = d["g"]
    Ch = C // 2
    d["z"] = -0.5 + blobs(N, C, S, g, 2, 4.0)
    cond = blobs(N, Cc, S, g, 3, 12.0)
    nconst = Cc // 3
    cond[:, :nconst] = torch.randn(1, nconst, 1, 1, generator=g)
    d["cond"] = cond
    d["w1"] = d["w1"] * 10.0 ** (-6.0 * torch.rand(256, 1, 1, 1, generator=g))
    d["w2"] = d["w2"] * 10.0 ** (-6.0 * torch.rand(256, 1, 1, 1, generator=g))
    xin = torch.cat((d["z"][:, :Ch], d["cond"]), 1).double()

    def init(a):
        m, v = a.mean(dim=(0, 2, 3)), a.var(dim=(0, 2, 3), unbiased=True)
        return (-m).float(), torch.log(1.0 / (v.sqrt() + 1e-6)).float()
    a1 = F.conv2d(xin, d["w1"].double(), padding=1)
    d["n1b"], d["n1l"] = init(a1)
    h1 = actf(act, (a1 + ch(d["n1b"])) * ch(d["n1l"].exp()))
    d["n2b"], d["n2l"] = init(F.conv2d(h1, d["w2"].double()))

    def regime(d):
        ls = torch.cat((d["n1l"], d["n2l"]))
        assert float(ls.max()) >= 11.5 and float(ls.min()) <= 0.0 and float(ls.max() - ls.min()) >= 12.5, \
            (float(ls.min()), float(ls.max()))
    return d, regime


def _quad_gap(h):
    """per pixel: floor(log2) of the channel-128..255 maximum minus that of the channel-0..127 maximum"""
    return log2_floor(h[:, 128:].abs().amax(1)) - log2_floor(h[:, :128].abs().amax(1))


def sc_rescale(C, Cc, S, act, forced):
    """forced: the ActNorm logs of h1 channels 128-255 exceed those of 0-127 by 20 ln 2, so quad 1 raises every
    pixel's running exponent by at least 16 and the conv2 partial sums of quad 0 are rescaled by 2^-16 or less; h2's
    channels 0-127 lie 2^20 above 128-255.  reverse (forced=False): the opposite orderings -- quad 1 converts values far
    below the running scale and never rescales."""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 202 + S + C + forced)
    big, small = (slice(128, 256), slice(0, 128)) if forced else (slice(0, 128), slice(128, 256))
    d["n1l"][big] += 10 * math.log(2.0)
    d["n1l"][small] -= 10 * math.log(2.0)
    d["n2l"][small] += 10 * math.log(2.0)   # h2: the other half is the large one
    d["n2l"][big] -= 10 * math.log(2.0)

    def regime(d):
        h1, h2 = fp64_forward(d, act)
        gap1, gap2 = _quad_gap(h1), _quad_gap(h2)
        if forced:
            assert float(gap1.min()) >= 16 and float(gap2.max()) <= -16, (float(gap1.min()), float(gap2.max()))
        else:
            assert float(gap1.max()) <= -16 and float(gap2.min()) >= 16, (float(gap1.max()), float(gap2.min()))
    return d, regime


def sc_quad0_dead(C, Cc, S, act):
    """ReLU; channels 0-127 of h1 have very negative biases, so at the pixels of the weak half of each frame all of
    quad 0 is 0: the pixel's running exponent starts at the clamp (40) and quad 1 rescales from there"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 303 + S + C)
    amp = torch.ones(1, 1, 1, S)
    amp[..., S // 2:] = 0.05
    d["z"] = d["z"] * amp
    d["cond"] = d["cond"] * amp
    Ch = C // 2
    xin = torch.cat((d["z"][:, :Ch], d["cond"]), 1).double()
    a1 = F.conv2d(xin, d["w1"].double(), padding=1)
    weak = a1[:, :128, :, S // 2 + 1:].abs().amax(dim=(0, 2, 3))
    d["n1b"][:128] = -(2.0 * weak.float() + 0.05)

    def regime(d):
        h1, _ = fp64_forward(d, act)
        dead = h1[:, :128].abs().amax(1) == 0
        live1 = h1[:, 128:].abs().amax(1) > 0
        assert bool(dead.any()) and bool((~dead).any()) and bool((dead & live1).any())
        assert bool(dead[..., S // 2 + 1:].all())
    return d, regime


def sc_zero_rounds(C, Cc, S, act):
    """some rounds have an exactly zero image (z1 and cond, halo included) next to O(1) rounds; zero ActNorm biases,
    so h1 = h2 = 0 exactly there (the masks' "h <= 0 is off" against torch's relu / leaky_relu backward at 0)"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 404 + S + C)
    if S == 32:
        zero = (0, slice(8, 20))      # rows 8-19 of frame 0: round 3 (rows 12-15) and its halo rows 11 / 16
    elif S == 16:
        zero = (1, slice(0, S))       # frame 1 = rounds 2, 3
    else:
        zero = (slice(2, 4), slice(0, S))   # frames 2, 3 = round 1
    d["z"][zero[0], :, zero[1]] = 0.0
    d["cond"][zero[0], :, zero[1]] = 0.0
    d["n1b"].zero_()
    d["n2b"].zero_()

    def regime(d):
        xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1)
        m = round_max(xin)
        assert bool((m == 0).any()) and float(m.max()) >= 0.5
        h1, h2 = fp64_forward(d, act)
        z = (m == 0).expand_as(h1)
        assert bool((h1[z] == 0).all()) and bool((h2[z] == 0).all())
    return d, regime


def sc_halo_spike(C, Cc, S, act):
    """(32x32, 16x16) a round's interior is O(1) but the image row just below it -- its halo, the first row of the next
    round -- holds values 2^8 larger: the round's scale must come from the haloed image, or fp16 overflows"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 505 + S + C)
    R = 128 // S
    rows = list(range(R, S, 2 * R))   # the first row of every odd round
    for x in (d["z"], d["cond"]):
        x[:, :, rows] *= 256.0

    def regime(d):
        xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1).abs()
        for j in range(0, S // R, 2):   # even rounds: halo row (j+1)R against the interior
            inner = float(xin[:, :, j * R:(j + 1) * R].amax())
            halo = float(xin[:, :, (j + 1) * R].amax()) if (j + 1) * R < S else 0.0
            if halo:
                assert halo >= 2 ** 8 * inner * 0.5 and halo * 2.0 ** 14 / 2 ** math.floor(math.log2(inner)) > 65504
    return d, regime


def sc_frames_of_round(C, Cc, S, act, ratio_log2):
    """(8x8) a round holds two whole frames; the odd frame is 2^ratio_log2 smaller than the even one"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 606 + ratio_log2)
    for x in (d["z"], d["cond"]):
        x[1::2] *= 2.0 ** -ratio_log2
    d["go"][1::2] *= 2.0 ** -ratio_log2
    d["n1b"].zero_()   # the small frame's conv1 outputs carry only the convolution (the floor measurement below)

    def regime(d):
        xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1).abs()
        big, small = xin[0::2].amax(dim=(1, 2, 3)), xin[1::2].amax(dim=(1, 2, 3))
        assert bool((log2_floor(big) - log2_floor(small) >= ratio_log2 - 1).all())
    return d, regime


def sc_digit_background(C, Cc, S, act):
    """digit strokes (|x| >= 0.5) on a background 2^20 below them: inside every round some pixel neighbourhoods sit
    2^20 below the round maximum -- their lo pieces are fp16 subnormals (the floor of the model)"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 707 + S + C)
    bg = 2.0 ** -20
    yy = torch.arange(S).view(1, 1, S, 1).expand(N, 1, S, S)
    xx = torch.arange(S).view(1, 1, 1, S).expand(N, 1, S, S)
    digit = ((xx % 8) < 3) & (((yy + xx) % 5) < 3)   # strokes in every round, background columns between them
    for k in ("z", "cond"):
        x = d[k]
        d[k] = torch.where(digit, x.sign() * (0.5 + x.abs()), x * bg)
    d["go"] = torch.where(digit, d["go"], d["go"] * bg)
    d["n1b"].zero_()   # the background outputs of conv1 carry only the convolution (the floor measurement below)

    def regime(d):
        xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1).abs()
        nb = F.max_pool2d(xin.amax(1, keepdim=True), 3, 1, 1)   # 3x3 neighbourhood maximum
        low = nb <= 2.0 ** -19 * round_max(xin)
        assert bool(low.reshape(-1, 128).any(1).all())   # rounds are 128 consecutive (frame, pixel) positions
    return d, regime


def sc_zeros_w3(C, Cc, S, act, w3):
    """Conv2dZeros: w3 exactly 0 (as initialised) or ~w3"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 808 + S + C, w3_scale=w3)

    def regime(d):
        assert float(d["w3"].abs().max()) == 0.0 if w3 == 0 else float(d["w3"].abs().max()) < 10 * w3
    return d, regime


def sc_grad_scale(C, Cc, S, act, go, w3):
    """loss gradients at the scale bits/dim normalisation gives them (go ~1e-7 / 1e-9, small w3), and large ones"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 909 + S + C, w3_scale=w3)
    d["go"] = d["go"] * go

    def regime(d):
        m = float(d["go"].abs().max())
        assert go <= m <= 10 * go and float(d["w3"].abs().max()) < 10 * w3
    return d, regime


def sc_hetero_cond(C, Cc, S, act):
    """condition channels spanning 1e-4 .. 1e3, z1 O(1)"""
    N = FRAMES[S]
    d = base_net(C, Cc, S, N, 1010 + S + C)
    d["cond"] = d["cond"] * torch.logspace(-4, 3, Cc).view(1, Cc, 1, 1)

    def regime(d):
        m = d["cond"].abs().amax(dim=(0, 2, 3))
        assert float(m.min()) < 1e-3 and float(m.max()) > 1e3 / 2
    return d, regime


def _cases():
    out = []
    lv = list(LEVELS.items())
    for i, (name, (C, Cc, S)) in enumerate(lv):
        act = (RELU, LEAKY)[i % 2]
        other = LEAKY if act == RELU else RELU
        out += [("actnorm_init", name, act, lambda C=C, Cc=Cc, S=S, a=act: sc_actnorm_init(C, Cc, S, a))]
        out += [("rescale_forced", name, other, lambda C=C, Cc=Cc, S=S, a=other: sc_rescale(C, Cc, S, a, True))]
        out += [("rescale_never", name, act, lambda C=C, Cc=Cc, S=S, a=act: sc_rescale(C, Cc, S, a, False))]
        out += [("quad0_dead", name, RELU, lambda C=C, Cc=Cc, S=S: sc_quad0_dead(C, Cc, S, RELU))]
        for a in (RELU, LEAKY):
            out += [("zero_rounds", name, a, lambda C=C, Cc=Cc, S=S, a=a: sc_zero_rounds(C, Cc, S, a))]
        if S >= 16:
            out += [("halo_spike", name, act, lambda C=C, Cc=Cc, S=S, a=act: sc_halo_spike(C, Cc, S, a))]
        else:
            for r in (10, 20):
                out += [("frames_of_round_2^%d" % r, name, act,
                         lambda C=C, Cc=Cc, S=S, a=act, r=r: sc_frames_of_round(C, Cc, S, a, r))]
        out += [("digit_background", name, other, lambda C=C, Cc=Cc, S=S, a=other: sc_digit_background(C, Cc, S, a))]
        out += [("w3_zero", name, act, lambda C=C, Cc=Cc, S=S, a=act: sc_zeros_w3(C, Cc, S, a, 0.0))]
        out += [("w3_1e-4", name, other, lambda C=C, Cc=Cc, S=S, a=other: sc_zeros_w3(C, Cc, S, a, 1e-4))]
        for go, w3, a in ((1e-7, 1e-3, act), (1e-9, 1e-4, other), (1e4, 0.05, act)):
            out += [("go%g_w3%g" % (go, w3), name, a,
                     lambda C=C, Cc=Cc, S=S, a=a, go=go, w3=w3: sc_grad_scale(C, Cc, S, a, go, w3))]
        out += [("hetero_cond", name, act, lambda C=C, Cc=Cc, S=S, a=act: sc_hetero_cond(C, Cc, S, a))]
    return out


SCENARIOS = _cases()


@pytest.mark.parametrize("case", SCENARIOS, ids=lambda c: "%s-%s-%s" % (c[0], c[1], "relu" if c[2] == RELU else "leaky"))
def test_scenario_stagewise_vs_fp64(K, case):
    name, level, act, make = case
    C, Cc, S = LEVELS[level]
    d, regime = make()
    d.pop("g", None)
    regime(d)
    N = d["z"].shape[0]
    assert K.coupling_po_ok(N, C, Cc, 256, S, S, d["w1"], d["w3"], any_size=True) and K.coupling_po_bwd_ok(N, C, S, S)
    g = gpu_run(K, d, act)
    for k in ("h1", "h2", "P", "ga2", "ga1"):
        assert bool(torch.isfinite(g[k]).all()), (k, "non-finite")
    e = stage_errors(d, g, act)
    e.update(finish_errors(K, d, g))
    print("E_ABS %s %s %s %s" % (name, level, act, " ".join("%s=%.3g" % kv for kv in e.items())))
    if name == "w3_zero":   # Conv2dZeros at init: exactly zero, forward and backward
        for k in ("P", "ga2", "ga1"):
            assert bool((g[k] == 0).all()), k
        assert bool((g["part"] == 0).all())
    if name == "zero_rounds":   # the mask convention at h == 0 is torch's: relu'(0) = 0, leaky_relu'(0) = 0.2
        xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1)
        zmask = (round_max(xin) == 0).expand(N, 256, S, S)
        for h in ("h1", "h2"):
            assert bool((g[h][zmask] == 0).all()), h
        y = torch.zeros(8, dtype=torch.float64, requires_grad=True)
        actf(act, y).sum().backward()
        assert bool((y.grad == slope_of(act)).all())
        gh2 = F.conv_transpose2d(d["go"].double(), d["w3"].double(), padding=1)
        want = (gh2 * slope_of(act) * ch(d["n2l"].exp()))[zmask]
        assert torch.equal(g["ga2"][zmask] == 0, want == 0)
    if name.startswith("digit") or name == "frames_of_round_2^20":
        # the subnormal floor: conv1 outputs (zero ActNorm bias) whose image neighbourhood sits >= 2^19 below the round
        # maximum, measured against S without the floor term (2^-39 m errors of 2^-20 m values: <= 2^-19 if fp16
        # subnormals survive, ~2^-8 if they were flushed)
        xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1)
        nb = F.max_pool2d(xin.abs().amax(1, keepdim=True), 3, 1, 1)
        low = (nb <= 2.0 ** -19 * round_max(xin)).expand(N, 256, S, S)
        y0, s0 = conv1_ref(xin, d["w1"], phi=0.0)
        ex1 = ch(d["n1l"].exp())
        on = g["h1"] > 0
        ref = torch.where(on, (y0 + ch(d["n1b"])) * ex1, slope_of(act) * (y0 + ch(d["n1b"])) * ex1)
        dd = (g["h1"].double() - ref).abs() / ((s0 + ch(d["n1b"]).abs()) * ex1)
        e_floor = float(dd[low].max())
        print("E_FLOOR %s %s %.3g (n=%d)" % (name, level, e_floor, int(low.sum())))
        assert e_floor <= 2.0 ** -17, e_floor
    for k, v in e.items():
        assert v <= TOL, (k, v, e)


# --------------------------------------------------------------------------------------------- 3. equivariance
KS = (-40, -13, -1, 1, 7, 40)


def _biased_exp(t):
    """biased fp32 exponent of |t| (0 for 0)"""
    return (t.float().abs().view(torch.int32) >> 23) & 0xFF


def _assert_exponent_room(d, g, C):
    """Every scale of the kernels is 2^(141-E) with E = the biased exponent of a group maximum, clamped to [40, 250].
    Multiplying inputs by 2^k shifts each such E by k; with every non-zero group maximum at E in [81, 209] (values in
    [2^-46, 2^83)) E + k stays inside [41, 249] for |k| <= 40, so no clamp fires and every fp16 piece is unchanged.
    Groups that are exactly zero clamp to 40 in both runs and contribute zeros either way.  Every non-zero fp32 value
    the kernels store lies in [2^-80, 2^80], so after x 2^k (|k| <= 40) it is still a normal fp32 number and every
    rounding moves by exactly 2^k."""
    xin = torch.cat((d["z"][:, :C // 2], d["cond"]), 1)
    groups = [round_max(xin), round_max(d["go"]), g["h1"][:, :128].abs().amax(1), g["h1"].abs().amax(1),
              g["h2"].abs().amax(1), g["ga2"][:, :128].abs().amax(1), g["ga2"].abs().amax(1)]
    groups += [d[k].abs().max().view(1) for k in ("w1", "w2", "w3")]
    for m in groups:
        e = _biased_exp(m)
        assert bool(((e == 0) | ((e >= 81) & (e <= 209))).all()), (int(e[e > 0].min()), int(e.max()))
    for k in ("h1", "h2", "P", "ga2", "ga1", "part"):
        v = g[k].abs()
        v = v[v > 0]
        assert float(v.min()) >= 2.0 ** -80 and float(v.max()) <= 2.0 ** 80, k


def _scaled(d, keys, k):
    e = dict(d)
    for key in keys:
        e[key] = d[key] * 2.0 ** k
    return e


@pytest.mark.parametrize("level", list(LEVELS))
@pytest.mark.parametrize("act", [RELU, LEAKY], ids=["relu", "leaky"])
def test_power_of_two_equivariance_bit_exact(K, level, act):
    """every scale is an exact power of two taken from an exponent: scaling (z, cond, n1b, n2b) by 2^k scales h1, h2, P
    by exactly 2^k; scaling (w2, n2b) scales h2, P and leaves h1 alone; scaling go scales ga2, ga1 and the partial sums;
    the masks never change.  A missing or wrong rescale, or an unscale that does not match its scale, breaks these."""
    C, Cc, S = LEVELS[level]
    d = base_net(C, Cc, S, FRAMES[S], 1111 + S + C + act)
    d.pop("g")
    d["n1l"][128:] += 3.0   # the h1 rescale fires at every pixel (quad 1 raises the running exponent)
    g0 = gpu_run(K, d, act)
    _assert_exponent_room(d, g0, C)
    for k in KS:
        f = 2.0 ** k
        g = gpu_run(K, _scaled(d, ("z", "cond", "n1b", "n2b", "go"), k), act)
        for key in ("h1", "h2", "P", "ga2", "ga1", "part"):
            assert torch.equal(g[key], g0[key] * f), ("inputs", k, key)
        for key in ("m1", "m2"):
            assert torch.equal(g[key].view(torch.int32), g0[key].view(torch.int32)), ("inputs", k, key)
        g = gpu_run(K, _scaled(d, ("w2", "n2b"), k), act, bwd=False)
        assert torch.equal(g["h1"], g0["h1"]), ("w2", k)
        for key in ("h2", "P"):
            assert torch.equal(g[key], g0[key] * f), ("w2", k, key)
        for key in ("m1", "m2"):
            assert torch.equal(g[key].view(torch.int32), g0[key].view(torch.int32)), ("w2", k, key)


# --------------------------------------------------------------------------------------------- 4. size limit
def n_max(S):
    """largest frame count the fused kernels take on S x S maps: 32-bit byte offsets into [N, 256, S, S] fp32 tensors
    and whole 128-pixel rounds"""
    return max(n for n in range((1 << 32) // (1024 * S * S) - 2, (1 << 32) // (1024 * S * S) + 1)
               if n * 1024 * S * S < (1 << 32) and (n * S * S) % 128 == 0)


@pytest.mark.parametrize("level", list(LEVELS))
def test_size_limit_forward_backward(K, level):
    """forward and backward at the largest N the predicates accept (4095 / 16383 / 65534 frames of 32x32 / 16x16 / 8x8:
    4 GiB - 1 per hidden tensor), the first and last four frames against fp64; the next sizes are rejected by the
    predicates and never launched"""
    from rfn_hip import lib as L
    C, Cc, S = LEVELS[level]
    N = n_max(S)
    assert N == {32: 4095, 16: 16383, 8: 65534}[S]
    lib = L.load()
    w = base_net(C, Cc, S, 1, 1212 + S + C)
    assert lib.rfn_coupling_po_supported(N, C, Cc, 256, S, S) and lib.rfn_coupling_po_bwd_supported(N, C, S, S)
    assert K.coupling_po_ok(N, C, Cc, 256, S, S, w["w1"], w["w3"], any_size=True) and K.coupling_po_bwd_ok(N, C, S, S)
    for n in (N + 1, N + 2):
        assert not lib.rfn_coupling_po_supported(n, C, Cc, 256, S, S) and not lib.rfn_coupling_po_bwd_supported(n, C, S, S)
        assert not K.coupling_po_ok(n, C, Cc, 256, S, S, w["w1"], w["w3"], any_size=True)
        assert not K.coupling_po_bwd_ok(n, C, S, S)
    act = RELU if level in ("L0", "L2") else LEAKY
    gen = torch.Generator(device="cuda").manual_seed(13)
    z = torch.randn(N, C, S, S, device="cuda", generator=gen)
    cond = torch.randn(N, Cc, S, S, device="cuda", generator=gen)
    prm = {k: w[k].cuda() for k in ("w1", "w2", "w3", "n1b", "n1l", "n2b", "n2l")}
    plan = K.POPackPlan([(prm["w1"], prm["w2"], prm["w3"])])
    plan.run()
    h1, h2, P, masks = K.coupling_po_fwd(z, cond, plan.bufs[0], prm["n1b"], prm["n1l"], prm["n2b"], prm["n2l"], C, act,
                                         want_masks=True)
    torch.cuda.synchronize()
    ends = (slice(0, 4), slice(N - 4, N))
    cpu = [{"h1": h1[s].cpu(), "h2": h2[s].cpu(), "P": P[s].cpu(), "z": z[s].cpu(), "cond": cond[s].cpu()} for s in ends]
    del h1, h2, P, z, cond
    torch.cuda.empty_cache()
    go = torch.randn(N, C, S, S, device="cuda", generator=gen)
    ga2, ga1, part = K.coupling_po_bwd(go, plan.bwd_bufs[0], prm["n1l"], prm["n2l"], masks, act)
    torch.cuda.synchronize()
    for c, s in zip(cpu, ends):
        c.update(ga2=ga2[s].cpu(), ga1=ga1[s].cpu(), go=go[s].cpu())
    assert bool(torch.isfinite(part).all())
    del ga2, ga1, go, part, masks
    torch.cuda.empty_cache()
    worst = {}
    for c in cpu:
        d = {"C": C, "z": c["z"], "cond": c["cond"], "go": c["go"]}
        d.update({k: w[k] for k in ("w1", "w2", "w3", "n1b", "n1l", "n2b", "n2l")})
        e = stage_errors(d, c, act)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
    print("E_ABS size_limit %s N=%d %s" % (level, N, " ".join("%s=%.3g" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= TOL, (k, v, worst)
