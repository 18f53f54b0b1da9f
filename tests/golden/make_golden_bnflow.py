#!/usr/bin/env python3
"""Generate tests/golden/rfn_bnflow.pt by running the REFERENCE implementation on the CPU with `--flow_norm batchnorm`
(and `--base_norm batchnorm`): the reference calls its flow once per timestep, so every batch normalisation of the flow
and of its prior net takes the statistics of one timestep's B frames and updates its running statistics T-1 times per
training call, in time order.

Test infrastructure only, in the manner of make_golden.py (whose CPU shims, RNG capture and helpers it imports): needs
the reference checkout (RFN_REFERENCE), writes tensors and plain Python scalars only.

Usage:  python tests/golden/make_golden_bnflow.py          (from the repo root)

Writes rfn_bnflow.pt (inputs, draws, results) and, per configuration, rfn_bnflow.<name>.init.pt (sd_fresh, sd) and
rfn_bnflow.<name>.step.pt (grads, sd_after).

Per configuration (tiny architecture of make_golden.rfn_args, T = 4, B >= 3: with two samples a per-pixel variance
reaches eps and the eval-mode likelihood is meaningless):
  sd_fresh, out_first, draws_first      the first training call (ActNorm init; running statistics updated T-1 times)
  sd, out, draws, bits_per_dim, grads   a steady-state training call after a parameter perturbation, loss nll + 0.3 kl_fb
  sd_after                              the state after it, running buffers included
  loss_eval, predict                    eval mode, from sd_after: loss(x) and predict(x, 2, 2), each with its draws
  grads64                               the steady-state call once more in float64 (same state, same draws): the gradients
                                        of every `scale_shift` and conv bias of the flow.  Where an invariance leaves
                                        next to nothing of such a gradient (tests/test_bnflow_modules.py), `grads` minus
                                        this is what float32 rounding does to the reference itself.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (CPU shims and RNG capture are installed on import)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {
    "both_m03": dict(batch_size=4, flow_norm="batchnorm", base_norm="batchnorm", flow_batchnorm_momentum=0.3),
    "flow_m0": dict(batch_size=4, flow_norm="batchnorm"),
    "b3_skip": dict(batch_size=3, flow_norm="batchnorm", flow_batchnorm_momentum=0.5, skip_connection_flow="with_skip"),
}
T = 4


def replay_grads(RFN, args, sd, x, draws, dtype):
    """the steady-state call of a fresh model in state `sd` with the recorded draws, in `dtype` -> {name: gradient}"""
    import torch.distributions.normal as tdn
    torch.set_default_dtype(dtype)
    try:
        m = RFN(args).train()
        with torch.no_grad():
            m.loss(x.to(dtype), 0)       # registers the ConvLSTM's lazily created peephole parameters
        m.load_state_dict(sd)
        m = m.to(dtype).train()
        q = [t for _, t in draws]

        def uniform_(self, *a, **k):
            return self.copy_(q.pop(0))
        tdn._standard_normal = lambda shape, dtype=None, device=None: q.pop(0).to(dtype)
        torch.Tensor.uniform_ = uniform_
        kl_fb, kl, nll = m.loss(x.to(dtype), 0)
        (nll + 0.3 * kl_fb).backward()
        assert not q, "draws left over"
        return G.grads_of(m)
    finally:
        tdn._standard_normal, torch.Tensor.uniform_ = G._orig_std_normal, G._orig_uniform_
        torch.set_default_dtype(torch.float32)


def gen_bnflow():
    import Utils.modules as um
    import Flow.glow as fg
    um.device = torch.device("cpu")
    fg.device = torch.device("cpu")
    from RFN.RFN_new import RFN
    g = torch.Generator().manual_seed(2025)
    fx = {}
    for name, kw in CONFIGS.items():
        torch.manual_seed(83)
        B = kw["batch_size"]
        args = G.rfn_args(x_dim=[B, 1, 16, 16], condition_dim=[B, 1, 16, 16], **kw)
        m = RFN(args)
        m.train()
        x = (torch.rand(B, T, 1, 16, 16, generator=g) * 255).floor() / 256 - 0.5
        sd_fresh = G.sd_clone(m)
        G.start_capture()
        out0 = m.loss(x, 0)
        d0 = G.stop_capture()
        G.randomize_(m, g, 0.02)
        sd = G.sd_clone(m)
        G.start_capture()
        kl_fb, kl, nll = m.loss(x, 0)
        d1 = G.stop_capture()
        (nll + 0.3 * kl_fb).backward()
        bpd = float((kl + nll).item() / (np.log(2.) * float(np.prod(x.shape[2:])) * (T - 1)))
        e = {"args": dict(vars(args)), "T": T, "x": x, "sd_fresh": sd_fresh,
             "out_first": [float(o) for o in out0], "draws_first": [(k, t) for k, t in d0],
             "sd": sd, "sd_after": G.sd_clone(m), "out": [float(kl_fb), float(kl), float(nll)],
             "draws": [(k, t) for k, t in d1], "bits_per_dim": bpd, "grads": G.grads_of(m)}
        m.eval()
        with torch.no_grad():
            G.start_capture()
            kl_fb, kl, nll = m.loss(x, 0)
            e["loss_eval"] = {"draws": [(k, t) for k, t in G.stop_capture()], "out": [float(kl_fb), float(kl), float(nll)]}
            G.start_capture()
            tx, pr = m.predict(x, 2, 2)
            e["predict"] = {"draws": [(k, t) for k, t in G.stop_capture()], "n_predictions": 2, "n_conditions": 2,
                            "true_x": tx.detach(), "predictions": pr.detach()}
        # (after everything that draws from the global generator: building the replay's models draws from it too)
        again = replay_grads(RFN, args, sd, x, d1, torch.float32)
        assert all(torch.equal(again[k], v) for k, v in e["grads"].items()), "the replay is not the recorded call"
        e["grads64"] = {k: v for k, v in replay_grads(RFN, args, sd, x, d1, torch.float64).items()
                        if k.startswith("flow.") and k.endswith(("affine.scale_shift", "conv.bias"))}
        # committed files stay under 1 MiB: the four parameter-sized dicts of a configuration go into two files of their
        # own, named in "parts" (tests/test_bnflow_host.py load_fixture puts them back)
        e["parts"] = ["rfn_bnflow.%s.%s.pt" % (name, p) for p in ("init", "step")]
        G.save(e["parts"][0], {k: e.pop(k) for k in ("sd_fresh", "sd")})
        G.save(e["parts"][1], {k: e.pop(k) for k in ("grads", "sd_after")})
        fx[name] = e
    G.save("rfn_bnflow.pt", fx)


if __name__ == "__main__":
    gen_bnflow()
