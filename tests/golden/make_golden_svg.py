#!/usr/bin/env python3
"""Generate the fixtures of the SVG baseline by running the REFERENCE implementation on the CPU: its SVG (SVG/SVG.py,
SVG/trainer.py, main_svg.py).

Test infrastructure only, in the manner of make_golden_vrnn.py (make_golden's CPU shims and RNG capture are installed on
import, make_golden_vrnn's helpers are reused): needs the reference checkout (RFN_REFERENCE), writes tensors, plain
scalars and lists of names only.  The reference's gaussian_lstm draws with Tensor.normal_(), which make_golden's capture
does not see: it is recorded (and replayed) here.  The reference's SVG reads args.variance, which its parser never
defines: the Namespace gets variance = 1.0.

Usage:  python tests/golden/make_golden_svg.py          (from the repo root)

svg.pt               {"flags": the parser of main_svg.py, "checkpoint_keys", "preprocess", "compute_loss",
                     "configs": {name: {"args", "T", "seed", "keys", "shapes", "checksums", "parts"}}}
svg.<name>.loss.pt   k (the frames as uint8; x = k / 255, or k >= 128 for "bernoulli": `frames`), draws, out = (kl, nll)
                     of the float32 training call, out64 and grads = the same call replayed in float64 (gradients of
                     GRAD_NAMES, loss = nll + 0.3 kl), grads_rel_l2_ref = per tensor the worst ||g - g64|| / ||g64|| of the
                     reference's own float32 calls (default arithmetic, four CPU arithmetics, 16 noisy calls),
                     grads32_ratio = the elementwise grads_close ratio of the default call (for the record), data_seed
svg.<name>.gen.pt    predict(x, 2, 1) and reconstruct(x) in eval mode with their draws (true_x is x[:, :1] and frame 0 of
                     the reconstruction is zero: neither is stored), gen_err64 = what the float32 frames miss the float64
                     replay by
svg_iw.<name>.pt     elbo_importance_weighting(x, K = 2) in eval mode: k, draws, ref32, and ref64 = the float64 replay
Parameters are NOT stored: tests/srnn_state.fill_state(state_dict, seed) fills both sides.

An input (one data seed per configuration, tried in order from 2026, twelve at most) is accepted when
  - every grads_rel_l2_ref is at most 5e-4 (the tests' bound per tensor is max(4 grads_rel_l2_ref, 2e-4)),
  - the reference's float32 generated frames lie within 2.5e-5 absolute of its float64 replay,
  - its float32 importance-weighted bound lies within 1e-4 relative of its float64 replay.
If no seed of twelve meets the first condition, the first seed that meets the other two is taken and the configuration
gets no gradient fixture (grads = {})."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (CPU shims and RNG capture are installed on import)
import make_golden_vrnn as V  # noqa: E402

from tests.srnn_state import describe, fill_state  # noqa: E402

from argparse import Namespace  # noqa: E402

import torch  # noqa: E402

T, SEED, IW_K = 3, 77, 2
GRAD_NAMES = ("encoder.c1.0.main.0.weight", "encoder.c5.0.weight", "decoder.upc1.0.weight", "decoder.out.1.weight",
              "frame_predictor.embed.weight", "frame_predictor.lstm.0.weight_ih", "frame_predictor.lstm.0.weight_hh",
              "frame_predictor.lstm.1.weight_ih", "frame_predictor.lstm.1.weight_hh", "frame_predictor.lstm.1.bias_ih",
              "posterior.lstm.0.weight_hh", "posterior.mu_net.weight", "posterior.std_net.0.weight", "prior.mu_net.weight")
GRAD_MAX_ELEMENTS = 70000
REL_L2_ACCEPT, GEN_ACCEPT, IW_ACCEPT = 5e-4, 2.5e-5, 1e-4


def svg_args(**kw):
    B = 4
    a = dict(batch_size=B, x_dim=[B, 1, 64, 64], condition_dim=[B, 1, 64, 64], c_features=8, h_dim=16, z_dim=4,
             posterior_rnn_layers=1, predictor_rnn_layers=2, prior_rnn_layers=1, loss_type="mse", n_conditions=1,
             n_predictions=2, preprocess_range="none", norm_type="batchnorm", dequantize=True, n_bits=8, variance=1.0)
    a.update(kw)
    return Namespace(**a)


SVG_CONFIGS = {
    "gray_mse": dict(),
    "rgb_mse": dict(x_dim=[4, 3, 64, 64], condition_dim=[4, 3, 64, 64]),
    "bernoulli": dict(loss_type="bernoulli"),
    "gaussian": dict(loss_type="gaussian"),
}


def frames(k, loss_type):
    """the float32 frames of the stored uint8 values (td.Bernoulli validates its support: binary frames for that loss)"""
    return (k >= 128).float() if loss_type == "bernoulli" else k.float() / 255.0


# ------------------------------------------------------------------------------------- Tensor.normal_ capture / replay
_orig_normal_ = torch.Tensor.normal_


def start_capture():
    G.start_capture()

    def rec(self, *a, **k):
        r = _orig_normal_(self, *a, **k)
        G._draws.append(("normal", r.detach().clone()))
        return r
    torch.Tensor.normal_ = rec


def stop_capture():
    torch.Tensor.normal_ = _orig_normal_
    return G.stop_capture()


class feed:
    """inside: Tensor.normal_() copies the next recorded draw"""

    def __init__(self, draws, dtype):
        self.q = [t.to(dtype) for _, t in draws]

    def __enter__(self):
        q = self.q

        def normal_(t, *a, **k):
            return t.copy_(q.pop(0))
        torch.Tensor.normal_ = normal_
        return self

    def __exit__(self, *exc):
        torch.Tensor.normal_ = _orig_normal_
        if exc[0] is None:
            assert not self.q, "draws left over"


def model64(SVG, args, state, train):
    """a fresh model of the reference in the same state, in float64 (call under the float64 default dtype)"""
    m = SVG(args)
    m.load_state_dict(state)
    m = m.double()
    return m.train() if train else m.eval()


class float64_default:
    def __enter__(self):
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(torch.float32)


def named_grads(m):
    g = {n: v for n, v in G.grads_of(m).items() if n in GRAD_NAMES}
    assert sorted(g) == sorted(GRAD_NAMES), sorted(set(GRAD_NAMES) - set(g))
    return g


def rel_l2(g, g64):
    return {n: float((g[n].double() - g64[n]).norm() / g64[n].norm()) for n in GRAD_NAMES}


def training_call(m, x, draws):
    m.zero_grad(set_to_none=True)
    with feed(draws, torch.float32):
        kl, nll = m.loss(x)
    (nll + 0.3 * kl).backward()
    return named_grads(m)


def float32_variants(m, x, draws, g64):
    """{variant: {tensor: r}} of the reference's float32 training call under the four CPU arithmetics of
    make_golden_vrnn.py (thread count, oneDNN on / off)"""
    out = {}
    try:
        for variant in V.FLOAT32_VARIANTS:
            torch.set_num_threads(1 if variant.startswith("1 ") else 4)
            with torch.backends.mkldnn.flags(enabled="no oneDNN" not in variant):
                out[variant] = rel_l2(training_call(m, x, draws), g64)
    finally:
        torch.set_num_threads(4)
    return out


def float32_noise_trials(m, x, draws, g64):
    """[{tensor: r}] of V.NOISE_TRIALS float32 training calls with one unit of float32 round-off (relative, Gaussian) of
    noise on the output of every convolution, deconvolution and Linear layer"""
    g = torch.Generator().manual_seed(4242)

    def hook(_m, _i, out):
        return out * (1.0 + V.NOISE_LEVEL * torch.randn(out.shape, generator=g))
    hooks = [mod.register_forward_hook(hook) for mod in m.modules()
             if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Linear))]
    try:
        return [rel_l2(training_call(m, x, draws), g64) for _ in range(V.NOISE_TRIALS)]
    finally:
        for h in hooks:
            h.remove()


def parser_flags():
    """every flag of the reference's main_svg.py: [{"flags", "dest", "default", "choices", "nargs", "type", "const"}]"""
    import argparse
    import runpy
    V._stub_data_generators()

    class Captured(Exception):
        pass
    seen = []

    def parse_args(self, *a, **k):
        seen.append(self)
        raise Captured()
    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = parse_args
    try:
        runpy.run_path(os.path.join(G.REF, "main_svg.py"), run_name="__main__")
    except Captured:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    return [{"flags": list(a.option_strings), "dest": a.dest, "default": a.default,
             "choices": None if a.choices is None else list(a.choices), "nargs": a.nargs,
             "type": None if a.type is None else a.type.__name__, "const": a.const}
            for a in seen[0]._actions if a.dest != "help"]


def trainer_facts():
    """preprocess / compute_loss / checkpoint keys of the reference's SVG Solver"""
    V._stub_data_generators()
    from SVG.trainer import Solver
    base = dict(n_bits=8, n_epochs=1, learning_rate=1e-4, verbose=False, path="/tmp/", batch_size=2, patience_lr=1,
                factor_lr=0.5, min_lr=1e-5, patience_es=1, beta_max=1.0, beta_min=1e-4, beta_steps=100,
                choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=64,
                preprocess_range="none", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                n_conditions=2, use_validation_set=False)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 1, 8, 8, generator=g)
    pre = {}
    for nb in (5, 8):
        for rng in ("0.5", "1.0", "minmax", "none"):
            s = Solver(Namespace(**dict(base, n_bits=nb, preprocess_range=rng)))
            y = s.preprocess(x)
            pre["%d_%s" % (nb, rng)] = {"x": x, "y": y, "y_back": s.preprocess(y, reverse=True)}
    s = Solver(Namespace(**base))
    s.beta = 0.25
    nll, kl = torch.tensor(1234.5), torch.tensor(4.5)
    loss = s.compute_loss(nll, kl, torch.Size([1, 64, 64]), t=9)
    cl = {"nll": nll, "kl": kl, "beta": 0.25, "dims": [1, 64, 64], "t": 9, "loss": loss, "bits": s.bits[-1],
          "losses": s.losses[-1], "kl_loss": s.kl_loss[-1], "recon_loss": s.recon_loss[-1]}
    import tempfile
    s.model = torch.nn.Linear(2, 2)
    s.optimizer = torch.optim.Adam(s.model.parameters())
    s.counter = 0
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "model_folder"))
        s.path = d + "/"
        s.checkpoint("svg.pt", 1, 0.5)
        keys = sorted(torch.load(os.path.join(d, "model_folder", "svg.pt"), weights_only=False))
    return pre, cl, keys


def one_seed(SVG, name, args, data_seed, full):
    """everything recorded for one data seed, and whether (gradients, the rest) meet the acceptance conditions.  A seed
    whose default float32 call already misses the gradient criterion is refused without the twenty other calls, unless
    `full` asks for them (until one seed meets the other two conditions: its figures are what DESIGN.md reports when no
    seed passes)"""
    B, C, H, W = args.x_dim
    torch.manual_seed(87)
    g = torch.Generator().manual_seed(data_seed)
    m = SVG(args)
    keys, shapes, _ = describe(m.state_dict())
    state = fill_state(m.state_dict(), SEED)
    m.load_state_dict(state)
    _, _, sums = describe(state)
    k = torch.randint(0, 256, (B, T, C, H, W), generator=g).to(torch.uint8)
    x = frames(k, args.loss_type)
    m.train()
    torch.manual_seed(data_seed)
    start_capture()
    kl, nll = m.loss(x)
    d = stop_capture()
    assert len(d) == 2 * (T - 1) and all(kind == "normal" and tuple(t.shape) == (B, args.z_dim) for kind, t in d)
    (nll + 0.3 * kl).backward()
    grads32 = named_grads(m)
    assert all(v.numel() <= GRAD_MAX_ELEMENTS for v in grads32.values())
    tracked = {n: int(v) for n, v in m.state_dict().items() if n.endswith("num_batches_tracked")}
    assert all(v == (2 * (T - 1) if n.startswith("encoder.") else T - 1) for n, v in tracked.items()), tracked
    with float64_default():
        m64 = model64(SVG, args, state, True)
        with feed(d, torch.float64):
            kl64, nll64 = m64.loss(x.double())
        (nll64 + 0.3 * kl64).backward()
        grads64 = named_grads(m64)
    assert all(bool(torch.isfinite(v).all()) for v in grads64.values())
    ratio = V._grad_ratio(grads32, grads64)
    rels = [rel_l2(grads32, grads64)]
    default_worst = max(rels[0].values())
    if full or default_worst <= REL_L2_ACCEPT:
        rels += list(float32_variants(m, x, d, grads64).values())
        rels += float32_noise_trials(m, x, d, grads64)
        assert len(rels) == 1 + 4 + V.NOISE_TRIALS
    worst = {n: max(r[n] for r in rels) for n in GRAD_NAMES}
    print(name, "data seed", data_seed, "float32 against float64, ||g - g64|| / ||g64||, worst of %d calls:" % len(rels),
          {n: "%.1e" % v for n, v in worst.items()}, "default call alone: worst %.1e;" % default_worst,
          "elementwise ratio of the default call %.3f" % ratio)
    grads_ok = len(rels) == 1 + 4 + V.NOISE_TRIALS and max(worst.values()) <= REL_L2_ACCEPT
    if not grads_ok and not full:
        return None, False, False
    # generation from the SAME filled state in eval mode (the training calls above moved the running statistics)
    m.load_state_dict(state, strict=False)
    m.eval()
    with torch.no_grad():
        start_capture()
        tx, pr = m.predict(x, 2, 1)
        dp = stop_capture()
        start_capture()
        rc = m.reconstruct(x)
        dr = stop_capture()
        torch.manual_seed(data_seed)
        start_capture()
        v32 = float(m.elbo_importance_weighting(x, IW_K))
        di = stop_capture()
    assert len(dp) == 2 and len(dr) == T - 1 and len(di) == 2 * IW_K * (T - 1)
    assert torch.equal(tx, x[:, :1].transpose(0, 1)) and float(rc[0].abs().max()) == 0.0
    with float64_default():
        m64 = model64(SVG, args, state, False)
        with torch.no_grad():
            with feed(dp, torch.float64):
                _, pr64 = m64.predict(x.double(), 2, 1)
            with feed(dr, torch.float64):
                rc64 = m64.reconstruct(x.double())
            with feed(di, torch.float64):
                v64 = float(m64.elbo_importance_weighting(x.double(), IW_K))
    gen_err = max(float((pr.double() - pr64).abs().max()), float((rc.double() - rc64).abs().max()))
    rel = abs(v32 - v64) / abs(v64)
    print(name, "data seed", data_seed, "generated frames: float32 against float64 %.2e;  bound K %d: float32 %.6f "
          "float64 %.6f relative %.2e" % (gen_err, IW_K, v32, v64, rel))
    rest_ok = gen_err <= GEN_ACCEPT and rel <= IW_ACCEPT
    rec = {"keys": keys, "shapes": shapes, "sums": sums,
           "loss": {"k": k, "draws": [(a, t) for a, t in d], "out": [float(kl), float(nll)],
                    "out64": [float(kl64), float(nll64)], "grads": {n: grads64[n].float() for n in GRAD_NAMES},
                    "grads_rel_l2_ref": worst, "grads_rel_l2_default": rels[0], "grads32_ratio": ratio,
                    "n_float32_calls": len(rels),
                    "data_seed": data_seed},
           "gen": {"predict": {"draws": [(a, t) for a, t in dp], "n_predictions": 2, "n_conditions": 1,
                               "predictions": pr.detach()},
                   "reconstruct": {"draws": [(a, t) for a, t in dr], "recons_from_1": rc[1:].detach().clone()},
                   "gen_err64": gen_err},
           "iw": {"config": name, "K": IW_K, "mode": "eval", "k": k, "draws": [(a, t) for a, t in di], "ref32": v32,
                  "ref64": v64, "data_seed": data_seed, "seed": SEED}}
    return rec, grads_ok, rest_ok


def gen():
    flags = parser_flags()
    pre, cl, ckpt_keys = trainer_facts()
    from SVG.SVG import SVG
    cfgs = {}
    for name, kw in SVG_CONFIGS.items():
        args = svg_args(**kw)
        fallback = None
        for data_seed in range(2026, 2026 + 12):
            rec, grads_ok, rest_ok = one_seed(SVG, name, args, data_seed, fallback is None)
            if rest_ok and fallback is None:
                fallback = rec
            if grads_ok and rest_ok:
                break
        else:
            if fallback is None:
                raise RuntimeError("no well-conditioned input found for " + name)
            print(name, "NO seed of twelve meets the gradient criterion: no gradient fixture")
            rec = fallback
            rec["loss"]["grads"] = {}
        parts = ["svg.%s.%s.pt" % (name, p) for p in ("loss", "gen")]
        G.save(parts[0], rec["loss"])
        G.save(parts[1], rec["gen"])
        G.save("svg_iw.%s.pt" % name, rec["iw"])
        cfgs[name] = {"args": dict(vars(args)), "T": T, "seed": SEED, "keys": rec["keys"], "shapes": rec["shapes"],
                      "checksums": rec["sums"], "parts": parts}
    G.save("svg.pt", {"flags": flags, "checkpoint_keys": ckpt_keys, "preprocess": pre, "compute_loss": cl,
                      "configs": cfgs, "grad_names": list(GRAD_NAMES)})


if __name__ == "__main__":
    gen()
