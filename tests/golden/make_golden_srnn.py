#!/usr/bin/env python3
"""Generate the fixtures of the SRNN baseline by running the REFERENCE implementation on the CPU: its mixture of
discretized logistics (Utils/discretize_logits.py) and its SRNN (SRNN/SRNN.py, SRNN/trainer.py, main_srnn.py).

Test infrastructure only, in the manner of make_golden_bnflow.py (make_golden's CPU shims and RNG capture are installed
on import): needs the reference checkout (RFN_REFERENCE), writes tensors, plain scalars and lists of names only.

Usage:  python tests/golden/make_golden_srnn.py [mol] [srnn]         (from the repo root)

mol.pt            {"cases": [names], "parts": {name: file}, "recipe": ...}; one file mol.<case>.pt per case with the
                  inputs x, l (float32), the reference's nll_pix and d(sum nll_pix)/dl evaluated in float64 on those
                  inputs ("nll_pix64", "dl64") and in float32 ("nll_pix32", "dl32"), and one draw of its sampler in
                  float32 with the recorded uniforms ("u_mix", "u_x", "sample32").
srnn.pt           {"flags": the parser of main_srnn.py, "checkpoint_keys", "preprocess", "compute_loss",
                  "configs": {name: {"args", "T", "seed", "keys", "shapes", "checksums", "parts"}}}
srnn.<name>.loss.pt   x, draws, out = (kl, nll) of the float32 training call, out64 and grads = the same call replayed
                      in float64 (gradients of a named handful of tensors, loss = nll + 0.3 kl), grads32_err = what the
                      float32 call's gradients miss them by (max error / max, per tensor)
srnn.<name>.gen.pt    predict(x, 2, 2) and reconstruct(x) in eval mode with their draws
Parameters are NOT stored: tests/srnn_state.fill_state(state_dict, seed) fills both sides.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (CPU shims and RNG capture are installed on import)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.srnn_state import describe, fill_state  # noqa: E402

from argparse import Namespace  # noqa: E402

import torch  # noqa: E402

MOL_CASES = {  # name: (N, C, M, H, W)
    "rgb_m10": (3, 3, 10, 5, 13),
    "gray_m10": (2, 1, 10, 24, 24),
    "gray_m1": (1, 1, 1, 4, 4),
    "rgb_m3": (2, 3, 3, 16, 16),
}
MOL_RECIPE = ("x = 2k/255 - 1, k random bytes, first row of each frame k = 0, last row k = 255; mixture logits 2 n; "
              "means x + 0.15 n; log-scales U(-8, -0.5); coefficients n; n ~ N(0,1)")


def mol_inputs(g, N, C, M, H, W):
    P = 3 if C == 3 else 2
    k = torch.randint(0, 256, (N, C, H, W), generator=g)
    k[:, :, 0] = 0
    k[:, :, -1] = 255
    x = 2.0 * k.float() / 255.0 - 1.0
    l = torch.empty(N, M * (1 + P * C), H, W)
    l[:, :M] = 2.0 * torch.randn(N, M, H, W, generator=g)
    for c in range(C):
        o = M + c * P * M
        l[:, o:o + M] = x[:, c:c + 1] + 0.15 * torch.randn(N, M, H, W, generator=g)
        l[:, o + M:o + 2 * M] = torch.rand(N, M, H, W, generator=g) * 7.5 - 8.0
        if P == 3:
            l[:, o + 2 * M:o + 3 * M] = torch.randn(N, M, H, W, generator=g)
    return x, l


def gen_mol():
    import Utils.discretize_logits as dl
    g = torch.Generator().manual_seed(1910)
    parts = {}
    for name, (N, C, M, H, W) in MOL_CASES.items():
        x, l = mol_inputs(g, N, C, M, H, W)
        fn = dl.discretized_mix_logistic_loss if C == 3 else dl.discretized_mix_logistic_loss_1d
        e = {"x": x, "l": l, "M": M}
        for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
            torch.set_default_dtype(dt)    # (the reference creates its zeros in the default dtype)
            try:
                lv = l.to(dt).clone().requires_grad_(True)
                nll = fn(x.to(dt), lv)
                nll.sum().backward()
            finally:
                torch.set_default_dtype(torch.float32)
            assert nll.shape == (N, H, W) and bool(torch.isfinite(nll).all()) and bool(torch.isfinite(lv.grad).all())
            e["nll_pix" + tag], e["dl" + tag] = nll.detach(), lv.grad.detach()
        G.start_capture()
        smp = (dl.sample_from_discretized_mix_logistic if C == 3 else dl.sample_from_discretized_mix_logistic_1d)(l, M)
        d = G.stop_capture()
        assert [k for k, _ in d] == ["uniform", "uniform"]
        e["u_mix"], e["u_x"], e["sample32"] = d[0][1], d[1][1], smp.detach()
        parts[name] = "mol.%s.pt" % name
        G.save(parts[name], e)
    G.save("mol.pt", {"cases": list(MOL_CASES), "parts": parts, "recipe": MOL_RECIPE})


# --------------------------------------------------------------------------------------------------------- SRNN
T, SEED = 4, 77
GRAD_NAMES = ("dec_mean.0.weight", "dec_mean.0.bias", "lstm_h.LSTMlayer.conv.0.weight", "lstm_h.LSTMlayer.conv.0.bias",
              "lstm_a.LSTMlayer.conv.0.weight", "lstm_a.LSTMlayer.conv.0.bias", "prior_mean.4.weight",
              "prior_std.4.weight", "enc_mean.4.weight", "enc_std.4.weight", "z_0", "z_0x", "h_0", "c_0", "a_0")


def srnn_args(**kw):
    B = 4
    a = dict(batch_size=B, x_dim=[B, 1, 32, 32], condition_dim=[B, 1, 32, 32], h_dim=8, a_dim=8, z_dim=4,
             loss_type="mol", n_logistics=3, norm_type="none", res_q=False, enable_smoothing=False, num_shots=0,
             overshot_w=1.0, n_bits=8, dequantize=True, preprocess_range="1.0")
    a.update(kw)
    return Namespace(**a)


# The gradient checks run without norm layers.  Through the batch norms over B = 4 samples the reference's OWN float32
# training call misses its float64 replay by 1 to 60 times the bound the tests hold the kernels to (rtol 2e-3 plus 2e-4
# of a tensor's maximum; 20 inputs tried, figures in DESIGN.md section 19), so a gradient comparison there measures the
# conditioning of the input, not a kernel.  "gray_mol_batchnorm" keeps the default norm for the losses and the
# generation paths (eval-mode statistics), without gradients.
SRNN_CONFIGS = {
    "gray_mol": dict(),
    "rgb_mol_resq_smooth": dict(x_dim=[4, 3, 32, 32], condition_dim=[4, 3, 32, 32], res_q=True, enable_smoothing=True),
    "gray_mol_shots2": dict(num_shots=2, overshot_w=0.5),
    "bernoulli_nonorm": dict(loss_type="bernoulli", norm_type="none"),
    "gray_mol_batchnorm": dict(norm_type="batchnorm"),
}
NO_GRADS = ("gray_mol_batchnorm",)


def parser_flags():
    """every flag of the reference's main_srnn.py: [{"flags", "dest", "default", "choices", "nargs", "type"}]"""
    import argparse
    import runpy
    import types
    stub = types.ModuleType("data_generators")
    for n in ("MovingMNIST", "PushDataset", "KTH"):
        setattr(stub, n, object)
    sys.modules["data_generators"] = stub
    import matplotlib
    matplotlib.use("Agg")

    class Captured(Exception):
        pass
    seen = []

    def parse_args(self, *a, **k):
        seen.append(self)
        raise Captured()
    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = parse_args
    try:
        runpy.run_path(os.path.join(G.REF, "main_srnn.py"), run_name="__main__")
    except Captured:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    out = []
    for a in seen[0]._actions:
        if a.dest == "help":
            continue
        out.append({"flags": list(a.option_strings), "dest": a.dest, "default": a.default,
                    "choices": None if a.choices is None else list(a.choices), "nargs": a.nargs,
                    "type": None if a.type is None else a.type.__name__, "const": a.const})
    return out


def trainer_facts():
    from SRNN.trainer import Solver
    base = dict(n_bits=8, n_epochs=1, learning_rate=1e-4, verbose=False, path="/tmp/", batch_size=2, patience_lr=1,
                factor_lr=0.5, min_lr=1e-5, patience_es=1, beta_max=1.0, beta_min=1e-4, beta_steps=100,
                choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=64,
                preprocess_range="1.0", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                n_conditions=2, use_validation_set=False)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 1, 8, 8, generator=g)
    pre = {}
    for nb in (5, 8):
        for rng in ("0.5", "1.0", "minmax"):
            a = dict(base)
            a.update(n_bits=nb, preprocess_range=rng)
            s = Solver(Namespace(**a))
            y = s.preprocess(x)
            pre["%d_%s" % (nb, rng)] = {"x": x, "y": y, "y_back": s.preprocess(y, reverse=True)}
    s = Solver(Namespace(**base))
    s.beta = 0.25
    nll, kl = torch.tensor(1234.5), torch.tensor(4.5)
    loss = s.compute_loss(nll, kl, torch.Size([1, 64, 64]), t=9)
    cl = {"nll": nll, "kl": kl, "beta": 0.25, "dims": [1, 64, 64], "t": 9, "loss": loss, "bits": s.bits[-1],
          "losses": s.losses[-1], "kl_loss": s.kl_loss[-1], "recon_loss": s.recon_loss[-1]}
    # the checkpoint's keys: the reference's checkpoint() on a stand-in model
    import tempfile
    s.model = torch.nn.Linear(2, 2)
    s.optimizer = torch.optim.Adam(s.model.parameters())
    s.counter = 0
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "model_folder"))
        s.path = d + "/"
        s.checkpoint("srnn.pt", 1, 0.5)
        keys = sorted(torch.load(os.path.join(d, "model_folder", "srnn.pt"), weights_only=False))
    return pre, cl, keys


def replay_grads64(SRNN, args, state, x, draws):
    """the recorded training call once more in float64: a fresh model in the same state, the same draws -> ((kl, nll),
    {name: gradient})"""
    import torch.distributions.normal as tdn
    torch.set_default_dtype(torch.float64)
    try:
        m = SRNN(args)
        m.load_state_dict(state)
        m = m.double().train()
        q = [t.double() for _, t in draws]
        tdn._standard_normal = lambda shape, dtype=None, device=None: q.pop(0)

        def uniform_(self, *a, **k):
            return self.copy_(q.pop(0))
        torch.Tensor.uniform_ = uniform_
        kl, nll = m.loss(x.double())
        (nll + 0.3 * kl).backward()
        assert not q, "draws left over"
        return (float(kl), float(nll)), G.grads_of(m)
    finally:
        tdn._standard_normal, torch.Tensor.uniform_ = G._orig_std_normal, G._orig_uniform_
        torch.set_default_dtype(torch.float32)


def gen_srnn():
    flags = parser_flags()
    pre, cl, ckpt_keys = trainer_facts()
    import Utils.modules as um
    um.device = torch.device("cpu")
    from SRNN.SRNN import SRNN
    cfgs = {}
    for name, kw in SRNN_CONFIGS.items():
        args = srnn_args(**kw)
        B, C, H, W = args.x_dim
        # The inputs are accepted by the reference's own precision: its float32 training call must agree with its float64
        # replay to a quarter of the bound the tests hold the kernels to (rtol 2e-3 plus 2e-4 of the tensor's maximum).
        for data_seed in range(2026, 2026 + 12):
            torch.manual_seed(87)
            g = torch.Generator().manual_seed(data_seed)
            m = SRNN(args)
            keys, shapes, _ = describe(m.state_dict())
            state = fill_state(m.state_dict(), SEED)
            m.load_state_dict(state)
            _, _, sums = describe(state)
            k = torch.randint(0, 256, (B, T, C, H, W), generator=g).float()
            # (td.Bernoulli validates its support: binary frames for that loss)
            x = 2.0 * k / 255.0 - 1.0 if args.loss_type == "mol" else (k >= 128).float()
            m.train()
            torch.manual_seed(data_seed)
            G.start_capture()
            kl, nll = m.loss(x)
            d = G.stop_capture()
            (nll + 0.3 * kl).backward()
            grads32 = {n: v for n, v in G.grads_of(m).items() if n in GRAD_NAMES}
            out64, grads64 = replay_grads64(SRNN, args, state, x, d)
            grads = {n: grads64[n].float() for n in grads32}
            assert all(bool(torch.isfinite(v).all()) for v in grads.values())
            err32 = {n: float((grads32[n].double() - grads64[n]).abs().max() / grads64[n].abs().max()) for n in grads32}
            worst = max(float(((grads32[n].double() - grads64[n]).abs() /
                               (2e-3 * grads64[n].abs() + 2e-4 * grads64[n].abs().max())).max()) for n in grads32)
            print(name, "data seed", data_seed, "float32 against float64: worst error / bound %.3f" % worst,
                  {n: "%.1e" % v for n, v in err32.items()})
            if worst <= 0.25 or name in NO_GRADS:
                break
        else:
            raise RuntimeError("no well-conditioned input found for " + name)
        print(name, "out32", float(kl), float(nll), "out64", out64)
        e = {"x": x, "draws": [(a, t) for a, t in d], "out": [float(kl), float(nll)], "out64": list(out64),
             "grads": {} if name in NO_GRADS else grads, "grads32_err": err32, "data_seed": data_seed}
        # generation from the SAME filled state in eval mode (the training call above moved the running statistics)
        m.load_state_dict(state, strict=False)
        m.eval()
        gen = {}
        with torch.no_grad():
            G.start_capture()
            tx, pr = m.predict(x, 2, 2)
            gen["predict"] = {"draws": [(a, t) for a, t in G.stop_capture()], "n_predictions": 2, "n_conditions": 2,
                              "true_x": tx.detach(), "predictions": pr.detach()}
            G.start_capture()
            rc = m.reconstruct(x)
            gen["reconstruct"] = {"draws": [(a, t) for a, t in G.stop_capture()], "recons": rc.detach()}
        parts = ["srnn.%s.%s.pt" % (name, p) for p in ("loss", "gen")]
        G.save(parts[0], e)
        G.save(parts[1], gen)
        cfgs[name] = {"args": dict(vars(args)), "T": T, "seed": SEED, "keys": keys, "shapes": shapes, "checksums": sums,
                      "parts": parts}
    G.save("srnn.pt", {"flags": flags, "checkpoint_keys": ckpt_keys, "preprocess": pre, "compute_loss": cl,
                       "configs": cfgs})


if __name__ == "__main__":
    which = sys.argv[1:] or ["mol", "srnn"]
    for w in which:
        {"mol": gen_mol, "srnn": gen_srnn}[w]()
