"""Batch-norm flow steps with per-timestep statistics: what needs no GPU.

  * the closed-form running-statistics coefficients (rfn_hip.ops.bnflow_coef) against sequential updates;
  * the CPU route of Flow.glow_modules.BatchNormFlow with `steps = S` against S separate calls on the S slices
    (z, log-det, running buffers, gradients; float64);
  * ListGlow.log_prob takes `steps`;
  * the reference's fixture (tests/golden/make_golden_bnflow.py) loads with weights_only=True and holds what the GPU tests
    read.

`bnflow_ref` is the float64 restatement of the contract (include/rfn_hip.h, BatchNormFlow) that tests/test_bnflow.py holds
the kernels to; here it is checked against autograd on the reference's own expression, applied step by step."""
import inspect
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ("both_m03", "flow_m0", "b3_skip")
EPS = 1e-5


def load_fixture(name):
    """one configuration of rfn_bnflow.pt with the parameter-sized dicts of its part files put back"""
    e = dict(torch.load(os.path.join(GOLDEN, "rfn_bnflow.pt"), weights_only=True)[name])
    for part in e["parts"]:
        e.update(torch.load(os.path.join(GOLDEN, part), weights_only=True))
    return e


# ------------------------------------------------------------------------------------------------ float64 restatement
def bnflow_ref(x, lg, beta, S, eps=EPS):
    """training, forward: x [S*B, E] float64 -> z, mean [S, E], var [S, E], dl [S]"""
    B = x.shape[0] // S
    xs = x.view(S, B, -1)
    mean = xs.mean(1)
    var = (xs - mean[:, None]).pow(2).mean(1) + eps
    z = torch.exp(lg) * (xs - mean[:, None]) / var.sqrt()[:, None] + beta
    dl = (lg - 0.5 * torch.log(var)).sum(1)
    return z.reshape(x.shape), mean, var, dl


def bnflow_bwd_ref(x, lg, S, gz, gdl, eps=EPS):
    """the backward formulas of the contract -> gx, g_log_gamma, g_beta"""
    B = x.shape[0] // S
    xs, g = x.view(S, B, -1), gz.view(S, B, -1)
    mean = xs.mean(1, keepdim=True)
    var = (xs - mean).pow(2).mean(1, keepdim=True) + eps
    rstd = var.rsqrt()
    xh = (xs - mean) * rstd
    gp = g * torch.exp(lg)
    gx = rstd * (gp - gp.mean(1, keepdim=True) - xh * (gp * xh).mean(1, keepdim=True)) - gdl.view(S, 1, 1) * xh * rstd / B
    return gx.reshape(x.shape), (gp * xh).sum((0, 1)) + gdl.sum(), g.sum((0, 1))


def running_ref(r, stats, m):
    """S sequential updates r <- m r + (1 - m) stat_s"""
    for s in range(stats.shape[0]):
        r = m * r + (1 - m) * stats[s]
    return r


def apply_ref(x, lg, beta, rm, rv, reverse):
    dl = (lg - 0.5 * torch.log(rv)).sum()
    if not reverse:
        return torch.exp(lg) / rv.sqrt() * (x - rm) + beta, dl
    return (x - beta) * rv.sqrt() / torch.exp(lg) + rm, -dl


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("m", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("S", [1, 3, 19])
def test_closed_form_running_coefficients_equal_sequential_updates(S, m):
    from rfn_hip.ops import bnflow_coef
    g = torch.Generator().manual_seed(S)
    r0 = torch.randn(7, generator=g, dtype=torch.float64)
    stats = torch.randn(S, 7, generator=g, dtype=torch.float64)
    coef, decay = bnflow_coef(S, m)
    assert coef.dtype == torch.float64 and tuple(coef.shape) == (S,)
    got = decay * r0 + (coef[:, None] * stats).sum(0)
    torch.testing.assert_close(got, running_ref(r0, stats, m), rtol=1e-13, atol=1e-13)
    if m == 0.0:   # 0^0 = 1: "running = the last step's statistics", exactly
        assert decay == 0.0 and coef.tolist() == [0.0] * (S - 1) + [1.0]
    if m == 1.0:   # the buffers never move
        assert decay == 1.0 and coef.tolist() == [0.0] * S


def test_restated_backward_equals_autograd_of_the_step_wise_expression():
    g = torch.Generator().manual_seed(5)
    S, B, E = 3, 4, 10
    x = torch.randn(S * B, E, generator=g, dtype=torch.float64, requires_grad=True)
    lg = (0.2 * torch.randn(E, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = torch.randn(E, generator=g, dtype=torch.float64, requires_grad=True)
    gz = torch.randn(S * B, E, generator=g, dtype=torch.float64)
    gdl = torch.randn(S, generator=g, dtype=torch.float64)
    z, _, _, dl = bnflow_ref(x, lg, beta, S)
    ((z * gz).sum() + (dl * gdl).sum()).backward()
    gx, glg, gbeta = bnflow_bwd_ref(x.detach(), lg.detach(), S, gz, gdl)
    torch.testing.assert_close(gx, x.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(glg, lg.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(gbeta, beta.grad, rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize("m", [0.0, 0.3])
def test_cpu_route_with_steps_equals_separate_calls_on_the_slices(m):
    from Flow.glow_modules import BatchNormFlow
    g = torch.Generator().manual_seed(11)
    S, B, size = 3, 4, [4, 2, 3, 5]

    def make():
        bn = BatchNormFlow(size, momentum=m).double().train()
        gp = torch.Generator().manual_seed(12)
        with torch.no_grad():
            bn.log_gamma.copy_(0.3 * torch.randn(bn.log_gamma.shape, generator=gp, dtype=torch.float64))
            bn.beta.copy_(torch.randn(bn.beta.shape, generator=gp, dtype=torch.float64))
            bn.running_mean.copy_(torch.randn(bn.beta.shape, generator=gp, dtype=torch.float64))
            bn.running_var.copy_(torch.rand(bn.beta.shape, generator=gp, dtype=torch.float64) + 0.5)
        return bn
    x = torch.randn(S * B, *size[1:], generator=g, dtype=torch.float64) + 0.7
    w = torch.randn(x.shape, generator=g, dtype=torch.float64)
    wl = torch.randn(S * B, generator=g, dtype=torch.float64)
    ld0 = torch.randn(S * B, generator=g, dtype=torch.float64)

    one, xa = make(), x.clone().requires_grad_(True)
    z, ld = one(xa, ld0, reverse=False, steps=S)
    ((z * w).sum() + (ld * wl).sum()).backward()

    sep, xb = make(), x.clone().requires_grad_(True)
    zs, lds = [], []
    for s in range(S):   # what the reference does: one call per timestep
        zz, ll = sep(xb[s * B:(s + 1) * B], ld0[s * B:(s + 1) * B], reverse=False)
        zs.append(zz); lds.append(ll)
    z2, ld2 = torch.cat(zs), torch.cat(lds)
    ((z2 * w).sum() + (ld2 * wl).sum()).backward()

    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(z, z2, **tol)
    torch.testing.assert_close(ld, ld2, **tol)
    torch.testing.assert_close(one.running_mean, sep.running_mean, **tol)
    torch.testing.assert_close(one.running_var, sep.running_var, **tol)
    torch.testing.assert_close(xa.grad, xb.grad, **tol)
    torch.testing.assert_close(one.log_gamma.grad, sep.log_gamma.grad, **tol)
    torch.testing.assert_close(one.beta.grad, sep.beta.grad, **tol)
    # and both are the contract's restatement
    zr, mean, var, dl = bnflow_ref(x.view(S * B, -1), one.log_gamma.detach().view(-1), one.beta.detach().view(-1), S)
    torch.testing.assert_close(z.detach().view(S * B, -1), zr, **tol)
    torch.testing.assert_close((ld - ld0).detach(), dl.repeat_interleave(B), **tol)
    fresh = make()
    torch.testing.assert_close(one.running_var.view(-1), running_ref(fresh.running_var.view(-1), var, m), **tol)
    # update_running=False: same outputs, buffers untouched; the pooled statistics of all S*B rows are something else
    keep = make()
    z3, _ = keep(x, ld0, reverse=False, steps=S, update_running=False)
    torch.testing.assert_close(z3, z.detach(), **tol)
    assert torch.equal(keep.running_mean, fresh.running_mean) and torch.equal(keep.running_var, fresh.running_var)
    z4, _ = make()(x, ld0, reverse=False)
    assert float((z4 - z).detach().abs().max()) > 1e-3


def test_cpu_route_given_statistics_round_trip():
    from Flow.glow_modules import BatchNormFlow
    g = torch.Generator().manual_seed(21)
    bn = BatchNormFlow([3, 2, 2, 2], momentum=0.0).double().train()
    x = torch.randn(6, 2, 2, 2, generator=g, dtype=torch.float64)
    bn(x, None, reverse=False, steps=2)
    bn.eval()
    ld0 = torch.zeros(6, dtype=torch.float64)
    with torch.no_grad():
        z, ld = bn(x, ld0, reverse=False)
        xb, ldb = bn(z, ld, reverse=True)
    zr, dl = apply_ref(x.view(6, -1), bn.log_gamma.view(-1), bn.beta.view(-1), bn.running_mean.view(-1),
                       bn.running_var.view(-1), False)
    torch.testing.assert_close(z.view(6, -1), zr.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ld, dl.detach().expand(6), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(xb, x, rtol=1e-12, atol=1e-12)
    assert torch.equal(ldb, ld0)


def test_listglow_and_steps_take_the_step_count():
    from Flow.glow import GlowStep, ListGlow
    from Flow.glow_modules import BatchNormFlow, Conv2dNorm
    for fn in (ListGlow.log_prob, ListGlow.f, ListGlow._base_params, GlowStep.forward, BatchNormFlow.forward,
               Conv2dNorm.forward):
        p = inspect.signature(fn).parameters
        assert p["steps"].default == 1 and p["update_running"].default is True, fn


def test_batchnorm_step_keeps_the_reference_state_dict_keys():
    from argparse import Namespace
    from Flow.glow import GlowStep
    args = Namespace(flow_norm="batchnorm", flow_batchnorm_momentum=0.3, LU_decomposed=True, n_units_affine=8,
                     non_lin_glow="relu", clamp_type="realnvp")
    keys = set(GlowStep([2, 4, 2, 2], [2, 3, 2, 2], args).state_dict())
    assert {"norm.log_gamma", "norm.beta", "norm.running_mean", "norm.running_var"} <= keys
    assert not any("an_zero" in k or "_coef" in k for k in keys)


@pytest.mark.parametrize("name", CONFIGS)
def test_fixture_loads_and_has_its_keys(name):
    e = load_fixture(name)
    for k in ("args", "T", "x", "sd_fresh", "out_first", "draws_first", "sd", "out", "draws", "bits_per_dim", "grads",
              "grads64", "sd_after", "loss_eval", "predict"):
        assert k in e, k
    a = e["args"]
    B = a["batch_size"]
    assert a["flow_norm"] == "batchnorm" and B >= 3 and a["x_dim"][0] == B and a["condition_dim"][0] == B and e["T"] == 4
    assert tuple(e["x"].shape) == (B, 4, 1, 16, 16)
    assert {"both_m03": ("batchnorm", 0.3), "flow_m0": ("actnorm", 0.0), "b3_skip": ("actnorm", 0.5)}[name] == \
        (a["base_norm"], a["flow_batchnorm_momentum"])
    run = [k for k in e["sd_after"] if k.endswith("norm.running_var") and k.startswith("flow.glow_frame")]
    assert len(run) == a["L"] * a["K"]
    # the running statistics moved in the steady-state call (momentum < 1), the parameters did not
    assert all(not torch.equal(e["sd_after"][k], e["sd"][k]) for k in run)
    assert all(torch.equal(e["sd_after"][k], v) for k, v in e["sd"].items() if "running" not in k and "tracked" not in k)
    if a["base_norm"] == "batchnorm":
        nbt = [k for k in e["sd_after"] if k.startswith("flow.prior") and k.endswith("num_batches_tracked")]
        assert nbt and all(int(e["sd_after"][k]) == 2 * (e["T"] - 1) for k in nbt)   # T-1 per call, none for the init
    assert e["grads64"] and all(v.dtype == torch.float64 and v.shape == e["grads"][k].shape for k, v in e["grads64"].items())
    assert set(e["loss_eval"]) == {"draws", "out"} and {"draws", "true_x", "predictions"} <= set(e["predict"])
    assert all(os.path.getsize(os.path.join(GOLDEN, p)) < (1 << 20) for p in e["parts"] + ["rfn_bnflow.pt"])
