#!/usr/bin/env python3
"""Developer tool: cost of the VRNN baseline's own kernel and where its training step goes.  Prints ONE JSON line and
writes the same line to --out (default profiles/vrnn_bench.json).  Profiler off.

  python tools/bench_vrnn.py [--B 60 --Z 20 --reps 5 --inner 100 --steps 5 --out profiles/vrnn_bench.json]

(a) rfn_hip.ops.gauss_heads at [B, Z] (the step's diagonal Gaussians, csrc/gauss_heads.hip): forward (z_q, kl under
    no_grad) and forward + backward (loss = sum z_q w + sum kl u), against the same chain as float32 torch ops kept here
    (nn.Softplus, td.Normal, rsample by hand with the same eps, td.kl_divergence summed over the row).  Median / min / max
    of --reps repetitions, kernel and op chain alternated repetition by repetition; a repetition times --inner
    back-to-back calls between two events on the stream after two warm-up calls.  Both sides are launch-bound at this
    size: the figure is host enqueue time per call as much as device time, which is what a training step pays.
(b) one eager training step of main_vrnn.py's default model (B = 60, T = 10, 64x64 gray, mol): median of --steps steps
    after two warm-up steps, and the time by phase from device events around each phase of a restatement of VRNN.loss
    that calls the model's own modules in the model's order (its (kl, nll) are checked against model.loss on the same
    draws): phi_x_t, phi_z, ConvLSTM, heads (prior / enc convolutions, the four MLPs, gauss_heads), decoder, likelihood,
    backward, Adam.  The phases are serial on one stream, so their sum is the step but for the events' own cost."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def timer(fn, inner):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3   # microseconds per call
    return once


def bench_kernel(a):
    import torch
    import torch.distributions as td
    from rfn_hip import ops as K
    B, Z = a.B, a.Z
    g = torch.Generator(device="cuda").manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    q_loc, p_loc, eps = rn(B, Z), rn(B, Z), rn(B, Z)
    q_raw, p_raw = rn(B, Z) - 1.0, rn(B, Z) - 1.0
    w, u = rn(B, Z), rn(B)
    leaves = [t.clone().requires_grad_(True) for t in (q_loc, q_raw, p_loc, p_raw)]
    softplus = torch.nn.Softplus()

    def chain(ql, qr, pl, pr):
        qd, pd = td.Normal(ql, softplus(qr)), td.Normal(pl, softplus(pr))
        return qd.loc + qd.scale * eps, td.kl_divergence(qd, pd).sum(-1)

    def k_fwd():
        with torch.no_grad():
            K.gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=eps, want=("z_q", "kl"))

    def t_fwd():
        with torch.no_grad():
            chain(q_loc, q_raw, p_loc, p_raw)

    def both(fn):
        def run():
            for t in leaves:
                t.grad = None
            z, kl = fn(*leaves)
            ((z * w).sum() + (kl * u).sum()).backward()
        return run
    k_fb = both(lambda *l: K.gauss_heads(*l, eps_q=eps, want=("z_q", "kl")))
    t_fb = both(chain)
    # the two sides compute the same thing
    zk, klk = K.gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=eps, want=("z_q", "kl"))
    zt, klt = chain(q_loc, q_raw, p_loc, p_raw)
    agree = {"z_q": float((zk - zt).abs().max()), "kl_rel": float(((klk - klt).abs() / klt.abs()).max())}
    timers = {"fwd": timer(k_fwd, a.inner), "torch_fwd": timer(t_fwd, a.inner), "fwd_bwd": timer(k_fb, a.inner),
              "torch_fwd_bwd": timer(t_fb, a.inner)}
    t = {k: [] for k in timers}
    for _ in range(a.reps):      # alternated: one repetition of each, then the next round
        for k, f in timers.items():
            t[k].append(f())
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"shape": {"B": B, "Z": Z}, "us_per_call": {k: summary(v) for k, v in t.items()},
            "torch_over_kernel": {k: med["torch_" + k] / med[k] for k in ("fwd", "fwd_bwd")}, "agreement": agree}


PHASES = ("phi_x_t", "phi_z", "convlstm", "heads", "decoder", "likelihood", "backward", "adam")


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


def loss_by_phase(m, xt, eps, ph):
    """VRNN.loss for loss_type "mol" with the model's own modules in the model's order, a phase name around each call"""
    import torch
    from rfn_hip import ops as K
    b, t, c, h, w = xt.shape
    hprev, cprev, _, zxprev, _, kl_loss, nll_loss = m.get_inits()
    logits = []
    for i in range(1, t):
        xt_features = ph("phi_x_t", lambda: m.phi_x_t(xt[:, i]))
        ut = ph("phi_x_t", lambda: m.phi_x_t(xt[:, i - 1]))
        fz = ph("phi_z", lambda: m.phi_z(zxprev))
        _, ht, ct = ph("convlstm", lambda: m.lstm(torch.cat([ut, fz], 1).unsqueeze(1), hprev, cprev))

        def heads():
            p_loc, p_raw = m._prior_heads(ht)
            q_loc, q_raw = m._enc_heads(ht, xt_features)
            return K.gauss_heads(q_loc, q_raw, p_loc, p_raw, eps_q=eps[i - 1], want=("z_q", "kl"))
        zx_t, kl_t = ph("heads", heads)
        fz = ph("phi_z", lambda: m.phi_z(zx_t))
        logits.append(ph("decoder", lambda: m.dec_mean(m.dec(torch.cat([ht, fz], 1)))))
        zxprev, hprev, cprev = zx_t, ht, ct
        kl_loss = kl_loss + kl_t

    def likelihood():
        x_all = xt[:, 1:].transpose(0, 1).reshape((t - 1) * b, c, h, w)
        nll_steps = K.mol_nll(x_all.detach(), torch.cat(logits, 0), reduce="frame").view(t - 1, b)
        nll = 0
        for s in range(t - 1):
            nll = nll + nll_steps[s]
        return nll
    nll_loss = ph("likelihood", likelihood)
    return kl_loss.mean(), nll_loss.mean()


def bench_step(a):
    import torch
    import main_vrnn
    from VRNN import VRNN
    from VRNN.trainer import Solver
    args = main_vrnn.build_parser().parse_args([])
    assert (args.batch_size, args.n_frames, args.image_size, args.h_dim, args.z_dim, args.loss_type) == \
        (60, 10, 64, 256, 20, "mol")
    torch.manual_seed(1)
    m = VRNN(args).to("cuda").train()
    opt = Solver.make_optimizer(m.parameters(), args.learning_rate)
    B, T = args.batch_size, args.n_frames
    g = torch.Generator(device="cuda").manual_seed(2)
    xt = 2.0 * torch.randint(0, 256, (B, T, 1, 64, 64), generator=g, device="cuda").float() / 255.0 - 1.0
    eps = [torch.randn(B, args.z_dim, generator=g, device="cuda") for _ in range(T - 1)]

    def step(ph):
        kl, nll = loss_by_phase(m, xt, eps, ph)
        opt.zero_grad(set_to_none=True)
        ph("backward", lambda: (nll + 0.5 * kl).backward())
        ph("adam", opt.step)
        return kl, nll

    with torch.no_grad():    # the restatement is the model's loss
        m.eval()
        kl0, nll0 = m.loss(xt, draws=list(eps))
        kl1, nll1 = loss_by_phase(m, xt, eps, lambda name, fn: fn())
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
    return {"model": {"B": B, "T": T, "image": 64, "h_dim": args.h_dim, "z_dim": args.z_dim, "loss_type": "mol",
                      "norm_type": args.norm_type, "parameters": sum(p.numel() for p in m.parameters())},
            "step_ms": summary(whole), "phase_ms": {p: summary(v) for p, v in phases.items()},
            "phase_share": {p: med[p] / sum(med.values()) for p in PHASES}, "restatement_against_model_loss": same,
            "peak_memory_GB": torch.cuda.max_memory_allocated() / 1e9}


def main(a):
    import torch
    assert torch.cuda.is_available(), "bench_vrnn.py needs a GPU"
    out = {"tool": "bench_vrnn", "device": torch.cuda.get_device_name(0),
           "protocol": "(a) median/min/max of %d alternated repetitions, each %d back-to-back calls between stream events, "
                       "two warm-up calls; (b) median/min/max of %d eager steps after two warm-up steps, phases from device "
                       "events; profiler off" % (a.reps, a.inner, a.steps),
           "gauss_heads": bench_kernel(a)}
    print("gauss_heads: " + json.dumps(out["gauss_heads"]["us_per_call"]), file=sys.stderr, flush=True)
    out["train_step"] = "not measured" if a.steps <= 0 else bench_step(a)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=60)
    ap.add_argument("--Z", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "vrnn_bench.json"))
    main(ap.parse_args())
