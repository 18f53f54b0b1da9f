"""`--flow_norm batchnorm` / `--base_norm batchnorm` end to end on the GPU against the REFERENCE's results
(tests/golden/rfn_bnflow.pt, made by tests/golden/make_golden_bnflow.py: same weights, captured draws).

The reference calls its flow once per timestep: every batch normalisation of the flow and of its prior net takes the
statistics of one timestep's B frames and updates its running statistics T-1 times per training call, in time order.
RFN.loss time-batches all B*(T-1) frames into one flow call and passes steps = T-1; statistics taken over the B*(T-1)
frames at once miss the loss and the running buffers, and one more running-statistics update by the data-initialising
call misses the buffers of 'both_m03' (momentum 0.3 keeps a trace of every update; BatchNorm2d counts them).

Tolerances: those of tests/test_hip_modules.py::test_rfn_loss_end_to_end and ::test_rfn_analysis_methods_vs_reference;
running buffers within 1e-5 of the largest reference value of the buffer.  The reference in float32 against itself in
float64 on these configurations: NLL 7e-8 relative, gradients 9e-7 of the largest component.

Two rules of this file's own, for tensors of which an invariance leaves (next to) nothing:
  * Gradients.  The bias of a convolution that a BatchNorm2d follows (the prior net under base_norm = batchnorm) has
    the gradient zero: the normalisation removes a constant.  `scale_shift` of a coupling whose output goes straight into
    a batch-norm step has next to none: a per-channel factor exp(shift) is normalised away and its log-det term is
    given back by the normalisation's, exactly but for eps inside var.  Either is computed as a difference of sums over
    N*H*W terms, and what float32 leaves is the rounding of those sums, which does not shrink with the remainder: the
    fixture holds the reference's own gradients of these tensors once more in float64 (`grads64`: same state, same
    draws), and the reference in float32 is 0.9e-6 .. 1.2e-5 off them where grads_close's atol, taken from the
    remainder, is 1.0e-6 .. 3.0e-6 (it is as far off, 1e-5 .. 3e-5, in the last step of a level, where nothing cancels
    and the atol is 1e-2 .. 2e-1).  So these tensors are held to the reference with grads_close's own rtol and atol PLUS
    twice the reference's own float32 rounding on tensors of that kind: E = the largest |grads - grads64| over the
    `scale_shift` tensors (respectively the conv biases) of the configuration that the invariance covers, and 2 E
    because two float32 computations that are each within E of the exact value are within 2 E of each other.  That is
    7.8e-6 .. 2.6e-5 for `scale_shift` values of 7e-5 .. 4e-3 (a zero gradient does not pass) and 2.7e-6 for the biases.
    Every other gradient is held by the plain rule.
  * A running mean after the FIRST call, where a Conv2dZeros still at zero makes a coupling the identity and the mean
    of a normalised, rotated tensor is 0: a mean of B values carries the rounding of their size, so the 1e-5 is taken
    of the larger of the buffer's largest value and the largest standard deviation sqrt(running_var) beside it.  After
    the steady-state call (sd_after) the rule is the plain one."""
from argparse import Namespace

import pytest
import torch

from oracle import rfn_oracle as O
from tests.test_bnflow_host import CONFIGS, load_fixture
from tests.test_hip_modules import close, cu, grads_close, load_sd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = load_fixture(name)
        return cache[name]
    return get


def running_close(m, sd_ref, mean_floor=False):
    """every running buffer of the flow and of its prior net; mean_floor: see the module docstring"""
    sd = m.state_dict()
    seen = 0
    for k, ref in sd_ref.items():
        if not k.startswith("flow."):
            continue
        if k.endswith(("running_mean", "running_var")):
            d = float((sd[k].detach().cpu().double() - ref.double()).abs().max())
            scale = float(ref.abs().max())
            if mean_floor and k.endswith("running_mean"):
                scale = max(scale, float(sd_ref[k[:-4] + "var"].max().sqrt()))
            assert d <= 1e-5 * scale, (k, d, scale)
            seen += 1
        elif k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(ref), (k, int(sd[k]), int(ref))
    assert seen > 0


def flow_grads_close(m, grads, grads64):
    """test_rfn_loss_end_to_end's gradient check; the tensors of which an invariance leaves next to nothing get the
    reference's own float32 rounding on top of the absolute tolerance (module docstring)"""
    from Flow.glow import GlowStep
    from Flow.glow_modules import Conv2dNorm
    frame = m.flow.glow_frame
    kinds = {"scale_shift": ["flow.glow_frame.%d.affine.scale_shift" % i for i in range(len(frame) - 1)
                             if isinstance(frame[i], GlowStep) and isinstance(frame[i + 1], GlowStep)
                             and frame[i + 1].flow_norm == "batchnorm"],
             "conv bias": ["flow.prior.%d.conv.bias" % i for i, mod in enumerate(m.flow.prior)
                           if isinstance(mod, Conv2dNorm) and mod.norm == "batchnorm"]}
    covered = [k for keys in kinds.values() for k in keys]
    grads = {k: v for k, v in grads.items() if not k.startswith(("extractor.net.", "upscaler.net."))
             and "LSTMlayer.Wc" not in k}
    assert kinds["scale_shift"] and all(k in grads and k in grads64 for k in covered)
    grads_close(m, {k: v for k, v in grads.items() if k not in covered}, 5e-3, 5e-4)
    named = dict(m.named_parameters())
    for kind, keys in kinds.items():
        if not keys:
            continue
        E = max(float((grads[k].double() - grads64[k]).abs().max()) for k in keys)
        for k in keys:
            got, ref = named[k].grad.detach().cpu(), grads[k]
            atol = 5e-4 * float(ref.abs().max()) + 1e-6 + 2.0 * E
            print("%s %s: max|ref| %.3e  |got - ref| %.3e  atol %.3e (reference float32 rounding E %.3e)" % (
                kind, k, float(ref.abs().max()), float((got - ref).abs().max()), atol, E))
            torch.testing.assert_close(got, ref, rtol=5e-3, atol=atol, msg=lambda s: k + ": " + s)


@pytest.mark.parametrize("name", CONFIGS)
def test_first_training_call_vs_reference(fixture, name):
    """from fresh weights: ActNorm init on the t = 1 batch (normalised with that batch's own statistics, running
    statistics untouched by it), then T-1 running-statistics updates"""
    from RFN import RFN
    f = fixture(name)
    m = load_sd(RFN(Namespace(**f["args"])), f["sd_fresh"]).train()
    out = m.loss(cu(f["x"]), 0, draws=[t for _, t in f["draws_first"]])
    for a, b in zip(out, f["out_first"]):
        assert abs(float(a.detach()) - b) <= 1e-4 * abs(b) + 1e-4, (float(a.detach()), b)
    # f["sd"] = the reference's state after this call (its parameters then perturbed; the buffers are as the call left them)
    running_close(m, f["sd"], mean_floor=True)


@pytest.mark.parametrize("name", CONFIGS)
def test_training_call_vs_reference(fixture, name):
    from RFN import RFN
    f = fixture(name)
    m = load_sd(RFN(Namespace(**f["args"])), f["sd"]).train()
    kl_fb, kl, nll = m.loss(cu(f["x"]), 0, draws=[t for _, t in f["draws"]])
    print("\n%s: nll %.6f (reference %.6f) kl %.6f (%.6f)" % (name, float(nll.detach()), f["out"][2],
                                                                float(kl.detach()), f["out"][1]))
    for a, b in zip((kl_fb, kl, nll), f["out"]):
        assert abs(float(a.detach()) - b) <= 1e-4 * abs(b) + 1e-5, (float(a.detach()), b)
    bpd = O.bits_per_dim(kl.detach().cpu(), nll.detach().cpu(), f["x"].shape[2:], f["T"] - 1)
    assert abs(bpd - f["bits_per_dim"]) <= 1e-4 * abs(f["bits_per_dim"])
    (nll + 0.3 * kl_fb).backward()
    flow_grads_close(m, f["grads"], f["grads64"])
    running_close(m, f["sd_after"])


@pytest.mark.parametrize("name", CONFIGS)
def test_eval_loss_and_predict_vs_reference(fixture, name):
    """eval mode: the given-statistics map (rfn_bnflow_apply_f32) forward in the loss, reverse in the generation"""
    from RFN import RFN
    f = fixture(name)
    m = load_sd(RFN(Namespace(**f["args"])), f["sd_after"]).eval()
    x = cu(f["x"])
    with torch.no_grad():
        e = f["loss_eval"]
        out = m.loss(x, 0, draws=[t for _, t in e["draws"]])
        for a, b in zip(out, e["out"]):
            assert abs(float(a) - b) <= 1e-4 * abs(b) + 1e-5, (float(a), b)
        e = f["predict"]
        tx, pr = m.predict(x, e["n_predictions"], e["n_conditions"], draws=[t for _, t in e["draws"]])
    assert torch.equal(tx.cpu(), e["true_x"])
    close(pr, e["predictions"], 1e-4, 1e-5)
    running_close(m, f["sd_after"])      # eval mode moves no buffer


def test_graph_captured_batchnorm_step_equals_eager_step(tmp_path):
    """Solver in hipGraph mode with flow_norm = base_norm = batchnorm: the captured step (BatchNormFlow kernels, the
    per-step BatchNorm2d of the prior net) replays to the eager loss, gradients and running statistics"""
    import __graft_entry__ as ge
    from RFN.trainer import Solver
    from RFN import RFN
    from rfn_hip import dist as rdist
    args = ge._tiny_args()
    B, T = 4, 4
    for k, v in dict(batch_size=B, x_dim=[B, 1, 16, 16], condition_dim=[B, 1, 16, 16], flow_norm="batchnorm",
                     base_norm="batchnorm", flow_batchnorm_momentum=0.0,
                     n_bits=8, n_epochs=1, learning_rate=0.0, verbose=False, path=str(tmp_path) + "/", patience_lr=1,
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
    assert any(n.endswith("norm.log_gamma") for n in eager)
    eager_loss = float(nll + 0.5 * kl_fb)
    # momentum 0: the running statistics of the flow are those of the last timestep, whatever came before
    eager_run = {k: v.detach().clone() for k, v in s.model.state_dict().items()
                 if k.startswith("flow.glow_frame") and "running" in k}
    del kl_fb, kl, nll
    s.optimizer.zero_grad(set_to_none=True)
    assert s.capture_graph(x, static_draws=draws), getattr(s, "_graph_error", "")
    for v in (v for k, v in s.model.state_dict().items() if k in eager_run):
        v.fill_(7.0)                                 # the replay itself has to write them
    for _ in range(2):  # replay twice: gradients must be overwritten, not accumulated
        out = s.train_step(x)
    torch.cuda.synchronize()
    assert abs(float(out) - eager_loss) <= 1e-5 * abs(eager_loss)
    for n, p in s.model.named_parameters():
        if n in eager:
            torch.testing.assert_close(p.grad, eager[n], rtol=1e-4, atol=1e-5 * float(eager[n].abs().max()) + 1e-7,
                                       msg=lambda m: n + ": " + m)
    sd = s.model.state_dict()
    for k, v in eager_run.items():
        torch.testing.assert_close(sd[k], v, rtol=1e-5, atol=1e-6, msg=lambda m: k + ": " + m)
