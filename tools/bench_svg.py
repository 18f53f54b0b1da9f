#!/usr/bin/env python3
"""Developer tool: cost of the SVG baseline's own kernels and where its training step goes.  Prints ONE JSON line and
writes the same line to --out (default profiles/svg_bench.json).  Profiler off.

  python tools/bench_svg.py [--B 100 --I 256 --H 256 --reps 5 --inner 100 --steps 5 --batch 100 --out ...]

(a) rfn_hip.ops.lstm_cell on the KERNEL route (csrc/lstm_cell.hip) against torch.nn.LSTMCell at [B, I] -> [B, H], float32:
    forward (under no_grad) and forward + backward through autograd (loss = sum h' u + sum c' v, gradients of x, h, c and
    the four parameters).  Median / min / max of --reps repetitions, the four variants alternated repetition by
    repetition; a repetition times --inner back-to-back calls between two events on the stream after two warm-up calls.
    The default route of rfn_hip.ops.lstm_cell follows the forward + backward figure.
(b) one eager training step of main_svg.py's default model (B = --batch, T = 10, 64x64 gray, mse): median of --steps steps
    after two warm-up steps, and the time by phase from device events around each phase of a restatement of SVG.loss that
    calls the model's own modules in the model's order (its (kl, nll) are checked against model.loss on the same draws):
    encoder, LSTM nets, heads + KL (mu_net, std_net, the sample, the KL), decoder, likelihood, backward, Adam.  The phases
    are serial on one stream, so their sum is the step but for the events' own cost.  Run once per route with
    RFN_LSTM_CELL=1 / 0 to see what the cell kernels do to the step (--reps 0 leaves (a) out, --steps 0 leaves (b) out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)

from bench_vrnn import summary, timer  # noqa: E402


def bench_cell(a):
    import torch
    from rfn_hip import ops as K
    B, I, H = a.B, a.I, a.H
    g = torch.Generator(device="cuda").manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    cell = torch.nn.LSTMCell(I, H).to("cuda")
    x, h, c, u, v = rn(B, I), rn(B, H), rn(B, H), rn(B, H), rn(B, H)
    params = [cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh]
    leaves = [t.clone().requires_grad_(True) for t in (x, h, c)]

    def kernel(x_, h_, c_):
        return K.lstm_cell(x_, h_, c_, *params, route="kernel")

    def module(x_, h_, c_):
        return cell(x_, (h_, c_))

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn(x, h, c)
        return run

    def both(fn):
        def run():
            for t in leaves + params:
                t.grad = None
            ho, co = fn(*leaves)
            ((ho * u).sum() + (co * v).sum()).backward()
        return run
    with torch.no_grad():
        hk, ck = kernel(x, h, c)
        ht, ct = module(x, h, c)
    agree = {"h": float((hk - ht).abs().max()), "c": float((ck - ct).abs().max())}
    timers = {"fwd": timer(fwd(kernel), a.inner), "torch_fwd": timer(fwd(module), a.inner),
              "fwd_bwd": timer(both(kernel), a.inner), "torch_fwd_bwd": timer(both(module), a.inner)}
    t = {k: [] for k in timers}
    for _ in range(a.reps):      # alternated: one repetition of each, then the next round
        for k, f in timers.items():
            t[k].append(f())
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"shape": {"B": B, "I": I, "H": H}, "us_per_call": {k: summary(v) for k, v in t.items()},
            "torch_over_kernel": {k: med["torch_" + k] / med[k] for k in ("fwd", "fwd_bwd")}, "agreement": agree,
            "kernel_not_slower_fwd_bwd": med["fwd_bwd"] <= med["torch_fwd_bwd"],
            "default_route_of_this_build": "kernel" if K.LSTM_CELL_KERNEL_DEFAULT else "torch"}


PHASES = ("encoder", "lstm_nets", "heads_kl", "decoder", "likelihood", "backward", "adam")


class Phases:
    """device events around the phases of one step; ms per phase after a synchronise"""

    def __init__(self):
        self.marks = []

    def __call__(self, name, fn):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.marks.append((name, e0, e1))
        return out

    def ms(self):
        import torch
        torch.cuda.synchronize()
        out = {p: 0.0 for p in PHASES}
        for name, e0, e1 in self.marks:
            out[name] += e0.elapsed_time(e1)
        return out


def loss_by_phase(m, x, eps, ph):
    """SVG.loss for loss_type "mse" with the model's own modules in the model's order, a phase name around each call"""
    import torch
    m._init_hidden(x.shape[0])
    eps = list(eps)
    nll, kl = 0, 0
    for i in range(1, x.shape[1]):
        h, skip = ph("encoder", lambda: m.encoder(x[:, i - 1]))
        h_target = ph("encoder", lambda: m.encoder(x[:, i])[0])
        hq = ph("lstm_nets", lambda: m.posterior._cells(h_target))
        hp = ph("lstm_nets", lambda: m.prior._cells(h))

        def heads():
            mu_q, lv_q = m.posterior.mu_net(hq), m.posterior.std_net(hq)
            mu_p, lv_p = m.prior.mu_net(hp), m.prior.std_net(hp)
            z = m.posterior.reparameterize(mu_q, lv_q, eps.pop(0))
            eps.pop(0)                        # (the prior's draw, made and dropped)
            return z, m.kl_criterion(mu_q, lv_q, mu_p, lv_p)
        z_t, kl_t = ph("heads_kl", heads)
        h_pred = ph("lstm_nets", lambda: m.frame_predictor(torch.cat([h, z_t], 1)))
        x_pred = ph("decoder", lambda: m.decoder([h_pred, skip]))
        nll = ph("likelihood", lambda: nll + m._nll_pixels(x_pred, x[:, i]))
        kl = kl + kl_t
    from Utils import batch_reduce
    return kl, ph("likelihood", lambda: batch_reduce(nll).mean())


def bench_step(a):
    import torch
    import main_svg
    from SVG import SVG
    from SVG.trainer import Solver
    args = main_svg.build_parser().parse_args([])
    assert (args.batch_size, args.n_frames, args.image_size, args.h_dim, args.z_dim, args.c_features, args.loss_type) == \
        (100, 10, 64, 256, 12, 256, "mse")
    B, T = a.batch, args.n_frames
    args.batch_size, args.x_dim, args.condition_dim = B, [B, 1, 64, 64], [B, 1, 64, 64]
    torch.manual_seed(1)
    m = SVG(args).to("cuda").train()
    opt = Solver.make_optimizer(m.parameters(), args.learning_rate)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randint(0, 256, (B, T, 1, 64, 64), generator=g, device="cuda").float() / 255.0
    eps = [torch.randn(B, args.z_dim, generator=g, device="cuda") for _ in range(2 * (T - 1))]

    def step(ph):
        kl, nll = loss_by_phase(m, x, eps, ph)
        opt.zero_grad(set_to_none=True)
        ph("backward", lambda: (nll + 1e-4 * kl).backward())
        ph("adam", opt.step)
        return kl, nll

    with torch.no_grad():    # the restatement is the model's loss
        m.eval()
        kl0, nll0 = m.loss(x, draws=list(eps))
        kl1, nll1 = loss_by_phase(m, x, eps, lambda name, fn: fn())
        m.train()
    same = {"kl_rel": abs(float(kl0) - float(kl1)) / abs(float(kl0)), "nll_rel": abs(float(nll0) - float(nll1)) / abs(float(nll0))}
    assert same["kl_rel"] <= 1e-4 and same["nll_rel"] <= 1e-4, same
    for _ in range(2):
        step(lambda name, fn: fn())
    torch.cuda.synchronize()
    whole, phases = [], {p: [] for p in PHASES}
    for _ in range(a.steps):
        ph = Phases()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(ph)
        e1.record()
        ms = ph.ms()
        whole.append(e0.elapsed_time(e1))
        for p in PHASES:
            phases[p].append(ms[p])
    med = {p: statistics.median(v) for p, v in phases.items()}
    from rfn_hip import ops as K
    return {"model": {"B": B, "T": T, "image": 64, "c_features": args.c_features, "h_dim": args.h_dim,
                      "z_dim": args.z_dim, "loss_type": "mse", "parameters": sum(p.numel() for p in m.parameters())},
            "lstm_cell_route": K.lstm_cell_route(x[:, 0, 0, 0]),
            "step_ms": summary(whole), "phase_ms": {p: summary(v) for p, v in phases.items()},
            "phase_share": {p: med[p] / sum(med.values()) for p in PHASES}, "restatement_against_model_loss": same,
            "peak_memory_GB": torch.cuda.max_memory_allocated() / 1e9}


def main(a):
    import torch
    assert torch.cuda.is_available(), "bench_svg.py needs a GPU"
    out = {"tool": "bench_svg", "device": torch.cuda.get_device_name(0),
           "protocol": "(a) median/min/max of %d alternated repetitions, each %d back-to-back calls between stream events, "
                       "two warm-up calls; (b) median/min/max of %d eager steps after two warm-up steps, phases from device "
                       "events; profiler off" % (a.reps, a.inner, a.steps),
           "lstm_cell": "not measured" if a.reps <= 0 else bench_cell(a)}
    out["train_step"] = "not measured" if a.steps <= 0 else bench_step(a)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=100)
    ap.add_argument("--I", type=int, default=256)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=100, help="B of the training step (main_svg.py's default is 100)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "svg_bench.json"))
    main(ap.parse_args())
