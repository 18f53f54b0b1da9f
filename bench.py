#!/usr/bin/env python3
"""bench.py — RFN training-step throughput on synthetic SM-MNIST-shaped video (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...)

One "step" = one full training iteration of the hot path as RFN/trainer.py:233-250 of the reference runs it:
preprocess -> RFN.loss forward (extractor, ConvLSTM, latent recurrence, upscaler, time-batched Glow log_prob) ->
backward -> gradient all-reduce (N>1) -> Adam, on the canonical SM-MNIST configuration (RFN/default_rfn_job.sh) at
global batch 32, seq_len 20, fp32.  Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line.
Strong scaling: the global batch (32 sequences) is fixed and sharded over the ranks (north_star).

A plain run measures the headline arithmetic only (RFN_CONV_PRECISION, default `mixed`): set-up, warm-up, the K timed
steps and the JSON line.  `--full` adds what takes runs of its own: the other two arithmetics, the GPU-vs-oracle bits/dim
parity that picks the headline among them, the forward-only rate, the per-kernel roofline and the CPU baseline.
`--dump-outputs DIR` writes what the last timed step computed as DIR/*.npy (see dump_outputs).
"""
import argparse
import json
import os
# ROCm 7.2: with graph packet capture on, hipGraph memset nodes (PyTorch multi-block reductions zero their semaphores
# with one) race with neighbouring kernel nodes on replay; must be set before the HIP runtime initialises.
import sys
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
if "torch" not in sys.modules:  # the flag certainly precedes the HIP runtime: tell rfn_hip.graph_capture_safe()
    os.environ.setdefault("RFN_GRAPH_ENV_BEFORE_TORCH", "1")
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")  # (override: A/B runs of two builds)
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (no sparsity)
PEAK_HBM_GBS = 8000.0


def make_batch(B, T, seed, device):
    from data_generators import SyntheticMovingMNIST
    ds = SyntheticMovingMNIST(seq_len=T, seed=seed)
    return torch.stack([ds[i] for i in range(B)]).to(device)


def build_solver(B_local, T, device, lr=1e-4, argv=None):
    """`argv` (optional): another configuration than the canonical SM-MNIST one (tools/bench_config.py)"""
    import main_rfn
    from RFN.trainer import Solver
    from RFN import RFN
    from rfn_hip import dist as rdist
    args = main_rfn.build_parser().parse_args(argv if argv is not None else main_rfn.canonical_smmnist_argv(B_local, T))
    args.path = "/gpurun_out/bench_tmp/"
    s = Solver(args)
    s.device = device
    torch.manual_seed(0)
    s.model = RFN(args).to(device).train()
    rdist.broadcast_module_state(s.model)
    s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
    s.optimizer = Solver.make_optimizer(s.model.parameters(), lr)
    return s, args


def kernel_roofline(rec, steps):
    """`rec` = (name, meta, start, end) HIP-event pairs recorded on the launch stream around every librfn_hip launch
    of `steps` training steps (rfn_hip.lib.PROFILE); grouped by kernel symbol.  For the dominant kernel the achieved
    ALGORITHMIC byte rate (inputs read once + outputs written once + weights) and FLOP rate are reported against both
    roofs; `bound` names the roof it sits closer to."""
    def peak_of(sym):
        """MFMA roof of a kernel symbol: the fp32-MFMA kernels (csrc/conv.hip) against 157.3 TFLOP/s, every split kernel
        (bf16x3, f16x3s: three 16-bit MFMAs per fp32 product) against 2500 / 3"""
        f32k = sym.startswith("conv_mfma_kernel") or sym.startswith("wgrad_mfma_kernel")
        if sym.endswith(" x6"):  # bf16x6: six MFMAs per fp32 product
            return PEAK_BF16_MFMA_TFLOPS / 6.0
        return PEAK_F32_MFMA_TFLOPS if f32k else PEAK_BF16_MFMA_TFLOPS / 3.0
    groups, shapes = {}, {}
    for name, meta, e0, e1 in rec:
        ms = e0.elapsed_time(e1)
        key = meta[1] if meta else name
        g = groups.setdefault(key, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        g["calls"] += 1
        g["ms"] += ms
        if meta:
            g["flops"] += meta[2]
            g["bytes"] += meta[4]
            h = shapes.setdefault(str(meta[1]) + " | " + str(meta[3]), {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            h["calls"] += 1
            h["ms"] += ms
            h["flops"] += meta[2]
            h["bytes"] += meta[4]
    # the roofline line is per kernel TEMPLATE: epilogue variants ("+actbwd": run-time modes of one symbol) and the
    # tile instantiations of one template ("gemm_wgrad_b3_kernel<2,4,4,2,64>", "<4,2,2,3,64,1>", the grouped forms ...)
    # are one kernel as far as the question "where does the step's time go" is concerned -- rocprofv3 --stats lists
    # the instantiations separately, profiles/*_last_step_by_template.txt sums them the same way.  A different arithmetic
    # of the same template (" x6": six MFMAs per product) has another roof and stays apart.  The table keeps everything.
    def template_of(k):
        base = k.split("+")[0]
        return base.split("<")[0].strip() + (" x6" if base.endswith(" x6") else "")
    syms = {}
    for k, v in groups.items():
        g = syms.setdefault(template_of(k), {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        for f in g:
            g[f] += v[f]
    mfma = {k: v for k, v in syms.items() if v["flops"] > 0}  # (shell kernels carry bytes only)
    dom = max(mfma, key=lambda k: mfma[k]["ms"])
    d = mfma[dom]
    mfma_peak = peak_of(dom)
    b3 = mfma_peak != PEAK_F32_MFMA_TFLOPS
    tot_ms = sum(v["ms"] for v in groups.values())
    mfma_ms = sum(v["ms"] for v in mfma.values())
    mfma_fl = sum(v["flops"] for v in mfma.values())
    tf = d["flops"] / (d["ms"] * 1e-3) / 1e12
    gbs = d["bytes"] / (d["ms"] * 1e-3) / 1e9
    hbm_bound = gbs / PEAK_HBM_GBS >= tf / mfma_peak
    roof = {"bound": "hbm" if hbm_bound else "mfma", "kernel": dom,
            "achieved": gbs if hbm_bound else tf, "peak": PEAK_HBM_GBS if hbm_bound else mfma_peak,
            "unit": "GB/s" if hbm_bound else "TFLOP/s",
            "frac": gbs / PEAK_HBM_GBS if hbm_bound else tf / mfma_peak, "traffic": None,
            "launches_per_step": d["calls"] // steps, "avg_launch_us": 1e3 * d["ms"] / d["calls"],
            "bytes_per_launch": d["bytes"] / d["calls"], "flops_per_launch": d["flops"] / d["calls"],
            "hbm": {"achieved_GBps": gbs, "frac_of_8TBps": gbs / PEAK_HBM_GBS},
            "mfma": {"achieved_TFLOPs_fp32_equiv": tf, "peak_TFLOPs": mfma_peak, "frac": tf / mfma_peak,
                     "arithmetic": "split precision: 3 v_mfma_f32_32x32x16_{bf16,f16} per fp32 product, peak = 2500/3"
                     if b3 else "v_mfma_f32_32x32x2_f32"},
            "all_mfma_kernels": {"achieved_TFLOPs_fp32_equiv": mfma_fl / (mfma_ms * 1e-3) / 1e12,
                                 "ms_per_step": mfma_ms / steps, "flops_per_step": mfma_fl / steps},
            "hip_kernel_ms_per_step": tot_ms / steps}
    # the memory-bound shell around the convolutions (ActNorm / InvConv / coupling / epilogue-backward / gather-scatter /
    # ConvLSTM gates / latent step ...): aggregate algorithmic bytes over aggregate launch time, against the HBM roof
    sh = {}
    for name, meta, e0, e1 in rec:
        if meta and meta[0] == "shell":
            g = sh.setdefault(meta[1], {"calls": 0, "ms": 0.0, "bytes": 0.0})
            g["calls"] += 1
            g["ms"] += e0.elapsed_time(e1)
            g["bytes"] += meta[4]
    if sh:
        sb, sm, sc = (sum(v[k] for v in sh.values()) for k in ("bytes", "ms", "calls"))
        roof["shell"] = {"bound": "hbm", "achieved": sb / (sm * 1e-3) / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": sb / (sm * 1e-3) / 1e9 / PEAK_HBM_GBS, "ms_per_step": sm / steps,
                         "launches_per_step": sc // steps, "bytes_per_step": sb / steps,
                         "kernels": sorted(([k, v["calls"] // steps, round(v["ms"] / steps, 3),
                                             round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1)] for k, v in sh.items()),
                                           key=lambda r: -r[2])}
    # HBM traffic of the dominant kernel comes from separate rocprofv3 --pmc passes of this same workload (FETCH_SIZE /
    # WRITE_SIZE cannot be read from inside the process); the committed summary is attached when it is for this kernel
    try:
        with open(os.path.join(ROOT, "profiles", "r03_pmc_dominant_traffic.json")) as f:
            pmc = json.load(f)
        if pmc.get("kernel") and pmc["kernel"] in dom:
            # the figure belongs to the kernel source it was measured on: dropped (null + traffic_stale) when that file changed
            import hashlib
            src = pmc.get("source")
            cur = hashlib.sha256(open(os.path.join(ROOT, src), "rb").read()).hexdigest()[:16] if src else None
            if src and cur != pmc.get("source_sha16"):
                roof["traffic_stale"] = True
                raise ValueError("stale")
            roof["traffic"] = pmc["traffic_bytes_per_launch"]
            roof["traffic_source"] = ("profiles/r03_pmc_dominant_traffic.json (rocprofv3 --pmc FETCH_SIZE, WRITE_SIZE passes; "
                                      "mean over the launches of every instantiation of the template)")
    except (OSError, ValueError):
        pass
    table = sorted(([k, v["calls"] // steps, round(v["ms"] / steps, 3),
                     round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 2), round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1)]
                    for k, v in groups.items()), key=lambda r: -r[2])
    shape_rows = sorted(([k, v["calls"] // steps, round(v["ms"] / steps, 3),
                          round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 2),
                          round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1)] for k, v in shapes.items()),
                        key=lambda r: -r[2])
    return roof, {"kernels": table, "shapes": shape_rows}


def cpu_baseline(T_cpu=4, B_cpu=2):
    """the CPU port (oracle) timed on this box's host cores: forward + backward + Adam of the SAME canonical
    architecture on a bounded sample (B_cpu sequences x T_cpu frames)."""
    import main_rfn
    from RFN import RFN
    from oracle import rfn_oracle as O
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))  # the GPU box grants 16 host cores per GPU
    torch.set_num_threads(cores)
    print("[bench] cpu_baseline on %d host threads ..." % cores, file=sys.stderr, flush=True)
    args = main_rfn.build_parser().parse_args(main_rfn.canonical_smmnist_argv(B_cpu, T_cpu))
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in RFN(args).state_dict().items()}  # parameter container only (CPU)
    leaves = []
    for k, v in sd.items():
        if v.is_floating_point() and "running_" not in k:
            v.requires_grad_(True)
            leaves.append(v)
    opt = torch.optim.Adam(leaves, lr=1e-4)
    x = make_batch(B_cpu, T_cpu, 7, "cpu") * 255 / 256 - 0.5
    cfg = vars(args)
    O.rfn_loss(sd, cfg, x, None, True)  # warm-up = ActNorm init
    t0 = time.perf_counter()
    reps = 0
    while reps < 1 or (time.perf_counter() - t0 < 10.0 and reps < 8):
        kl_fb, kl, nll = O.rfn_loss(sd, cfg, x, None, True)
        opt.zero_grad()
        (nll + kl_fb).backward()
        opt.step()
        reps += 1
        print("[bench] cpu_baseline rep %d: %.1f s" % (reps, time.perf_counter() - t0), file=sys.stderr, flush=True)
    dt = (time.perf_counter() - t0) / reps
    return {"value": B_cpu * T_cpu / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "oracle (CPU restatement of the reference, torch fp32) fwd+bwd+Adam, canonical SM-MNIST model, "
                      "B=%d T=%d, mean of %d steps" % (B_cpu, T_cpu, reps)}


def parity_check(device, T=10, scales=(0.003, 0.01, 0.1)):
    """GPU loss vs CPU oracle on the canonical architecture, same weights and noise: B=2, T=10 (a 9-step rollout of the
    latent recurrence and 18 modeled frames through the 50-step flow), every flow parameter perturbed by N(0, s^2) for
    s = 0.003, 0.01 and 0.1 after the data dependent init (Conv2dZeros / realnvp scales start at exactly zero, which would make
    the coupling nets irrelevant to the result).  Returns the bits/dim of both sides per scale and the worst relative error
    over the scales at which the fp32 oracle is finite; the split-precision convolutions stay the headline only while
    that error is within north_star's 1e-4.  (`reproducible`: a second evaluation gave the same bits.)"""
    import main_rfn
    from RFN import RFN
    from oracle import rfn_oracle as O
    B = 2
    args = main_rfn.build_parser().parse_args(main_rfn.canonical_smmnist_argv(B, T))
    g = torch.Generator().manual_seed(2)
    x = make_batch(B, T, 11, "cpu") * 255 / 256 - 0.5
    draws = []
    for _ in range(T - 1):
        draws += [torch.randn(B, 56, 2, 2, generator=g), torch.randn(B, 56, 2, 2, generator=g),
                  torch.rand(B, 1, 64, 64, generator=g) / 256]
    res = {"B": B, "T": T, "cases": []}
    for s_ in scales:
        torch.manual_seed(1)
        m = RFN(args).to(device).train()
        with torch.no_grad():
            m.loss(x.to(device), 0, draws=draws)  # data dependent ActNorm init
            gp = torch.Generator().manual_seed(3)
            for prm in m.flow.parameters():
                prm.add_(s_ * torch.randn(prm.shape, generator=gp).to(device))
            # the forward pass has no order-dependent float atomics any more (round 3: split-K slices and per-frame
            # log-det partials are added in a fixed order, the feature convolutions left MIOpen's split-K kernels): ONE
            # evaluation is the figure of merit; a second one only feeds the `reproducible` flag
            gpu_runs = []
            for _ in range(2):
                kl_fb, kl, nll = m.loss(x.to(device), 0, draws=draws)
                gpu_runs.append(O.bits_per_dim(kl.cpu(), nll.cpu(), x.shape[2:], T - 1))
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        with torch.no_grad():
            r = O.rfn_loss(sd, vars(args), x, draws, True)
        bpd_ref = O.bits_per_dim(r[1], r[2], x.shape[2:], T - 1)
        finite = bpd_ref == bpd_ref and abs(bpd_ref) != float("inf")
        errs = [abs(v - bpd_ref) / abs(bpd_ref) for v in gpu_runs] if finite else None
        bpd_gpu = gpu_runs[0]
        res["cases"].append({"perturbation": s_, "bits_per_dim_gpu": bpd_gpu if bpd_gpu == bpd_gpu else None,
                             "bits_per_dim_oracle": bpd_ref if finite else None, "oracle_finite": finite,
                             "rel_err": max(errs) if finite else None,
                             "reproducible": gpu_runs[0] == gpu_runs[1] or gpu_runs[0] != gpu_runs[0]})
        del m
    # a perturbation at which the fp32 reference arithmetic itself overflows (0.1: the oracle returns nan) is no
    # parity point; it is reported and left out of the maximum
    res["rel_err"] = max(c["rel_err"] for c in res["cases"] if c["oracle_finite"])
    return res


DUMP_SAMPLE = 1 << 22  # elements kept of each flattened parameter-sized output (16 MB of fp32)


def dump_outputs(d, solver):
    """--dump-outputs: what the timed path handed its caller in its last step, as .npy files in `d`:
    step_scalars.npy (float64: loss / t, kl / t, nll / t, bits/dim; t = modeled frames, as Solver records them),
    params.npy and grads.npy (float32: every parameter after the step's Adam update and the gradient the step computed,
    flattened and concatenated in named_parameters order; a parameter without a gradient contributes zeros).  The
    canonical model has 36.5 M parameters, so both hold the same fixed sample of DUMP_SAMPLE positions (seed 0, sorted).
    The inputs are the same in every run with the same arguments; the outputs agree between runs to rounding, not bit for
    bit: the backward pass combines weight-gradient partial sums with float atomics, and the optimizer
    steps before the last one carry that rounding forward."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    params = [p for _, p in solver.model.named_parameters()]
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in params])
    n = flat_p.numel()
    if n > DUMP_SAMPLE:
        idx = torch.randint(n, (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
        idx = idx.to(flat_p.device)
        flat_p, flat_g = flat_p[idx], flat_g[idx]
    scalars = [solver.losses[-1], solver.kl_loss[-1], solver.recon_loss[-1], solver.bits[-1]]
    np.save(os.path.join(d, "step_scalars.npy"), np.array(scalars, dtype=np.float64))
    np.save(os.path.join(d, "params.npy"), flat_p.float().cpu().numpy())
    np.save(os.path.join(d, "grads.npy"), flat_g.float().cpu().numpy())


DTYPE_STR = {"mixed": "f32 (forward convolutions fp32-grade: fused scaled-fp16 split f16x3s / three-piece bf16x6 split; "
                      "gradient convolutions bf16x3 split MFMA; fp32 accumulate everywhere)",
             "bf16x3": "f32 (convolutions: bf16x3 split-precision MFMA, fp32 accumulate)",
             "f32": "f32 (convolutions: v_mfma_f32_32x32x2_f32)"}


def _run_child(extra, env):
    """one measurement in a fresh child process: hipGraph mode first, and if that child dies (a crash inside a graph
    capture cannot be caught in-process) once more in eager mode.  Returns (json dict | None, graph_fallback)."""
    import subprocess
    base = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child"] + extra
    rank = int(os.environ.get("RANK", 0))
    for attempt, more in enumerate(([], ["--no-graph"])):
        if "--no-graph" in sys.argv and attempt == 1:
            break
        r = subprocess.run(base + more, stdout=subprocess.PIPE, text=True, env=env)
        lines = [l for l in (r.stdout or "").splitlines() if l.startswith("{")]
        if r.returncode == 0 and (lines or rank != 0):
            return (json.loads(lines[-1]) if lines else {}), attempt == 1
        print("[bench] child attempt %d failed (rc=%s)%s" % (attempt, r.returncode, "; retrying eager" if attempt == 0 else ""),
              file=sys.stderr, flush=True)
    return None, True


def launch_ranks(n, argv=None, env=None, timeout=None, script=None):
    """`python bench.py --gpus N` outside a launcher (no WORLD_SIZE in the environment): this GPU-less parent starts the N
    ranks itself, one process per GPU, with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set the way
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` would set them (backend nccl =
    RCCL; RFN_DIST_BACKEND / RFN_SINGLE_GPU as documented in DESIGN.md section 8).  Each rank is this same script (its own
    supervisor + measurement child).  Rank 0's stdout (the ONE JSON line) is passed through; the exit code is the first
    non-zero exit code of any rank, and when one rank fails the others are terminated instead of waiting for a
    rendezvous that will never complete.  Nothing here initialises the GPU."""
    import socket
    import subprocess
    argv = list(sys.argv[1:]) if argv is None else list(argv)
    base_env = dict(os.environ if env is None else env)
    if "MASTER_PORT" not in base_env:
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
            sk.bind(("127.0.0.1", 0))
            base_env["MASTER_PORT"] = str(sk.getsockname()[1])
    base_env.setdefault("MASTER_ADDR", "127.0.0.1")
    base_env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool (RCCL peer buffers)
    procs = []
    for r in range(n):
        e = dict(base_env)
        e.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                  "GROUP_RANK": "0", "RFN_BENCH_SELF_LAUNCHED": "1"})
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + argv, env=e,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    rc, t0 = 0, time.time()
    live = set(range(n))
    while live:
        for r in sorted(live):
            c = procs[r].poll()
            if c is None:
                continue
            live.discard(r)
            if c != 0 and rc == 0:
                rc = c
                print("[bench] rank %d exited with code %d; stopping the other ranks" % (r, c), file=sys.stderr, flush=True)
        if live and (rc != 0 or (timeout is not None and time.time() - t0 > timeout)):
            rc = rc or 124
            for r in live:
                procs[r].terminate()
            for r in live:
                try:
                    procs[r].wait(timeout=20)
                except subprocess.TimeoutExpired:
                    procs[r].kill()
            break
        if live:
            time.sleep(0.2)
    out0 = procs[0].stdout.read() if procs[0].stdout else ""
    lines = [l for l in out0.splitlines() if l.startswith("{")]
    if rc == 0 and not lines:
        print("[bench] rank 0 printed no JSON line", file=sys.stderr, flush=True)
        rc = 1
    if lines:
        print(lines[-1], flush=True)
    return rc


def supervise():
    """The parent never touches the GPU.  It runs the measurement in a fresh child process for the headline arithmetic
    (RFN_CONV_PRECISION, default mixed) and prints ONE line.  With --full it runs every convolution arithmetic (mixed,
    bf16x3, f32), each in its own child, and the line holds all of them: the headline (`value`, `ms_per_step`, `dtype`)
    is then the first of (mixed, bf16x3) whose bits/dim parity against the oracle, measured in this same run (B=2, T=10,
    flow perturbed), is within north_star's 1e-4; otherwise the all-fp32-MFMA run."""
    import tempfile
    a = make_parser().parse_args()
    with tempfile.TemporaryDirectory(prefix="bench_dump_") as tmp:  # other arithmetics' --dump-outputs, until the
        return _supervise(a, tmp)                                     # headline is known


def _supervise(a, tmp):
    import shutil
    rank = int(os.environ.get("RANK", 0))
    first = os.environ.get("RFN_CONV_PRECISION", "mixed")
    order = [first] + [p for p in ("mixed", "bf16x3", "f32") if p != first]
    runs = {}
    world = int(os.environ.get("WORLD_SIZE", 1))
    for prec in order:
        # N > 1: the headline arithmetic only (its parity is established by the N = 1 run: same kernels, same shapes
        # per rank or smaller); three rendezvous per invocation would triple the driver's wall time for nothing
        if prec != first and (not a.full or os.environ.get("RFN_BENCH_ONE_PRECISION") == "1" or world > 1):
            break
        env = dict(os.environ)
        env["RFN_CONV_PRECISION"] = prec
        extra = [] if prec == first else ["--secondary"]
        if a.dump_outputs and prec != first:
            extra += ["--dump-outputs", os.path.join(tmp, prec)]
        out, fell_back = _run_child(extra, env)
        if out is None:
            if prec == first:
                return 1
            print("[bench] secondary precision run (%s) failed; omitted" % prec, file=sys.stderr, flush=True)
            continue
        out["graph_fallback"] = bool(fell_back)
        runs[prec] = out
    if rank != 0:
        return 0
    summary = {p: {"ms_per_step": r.get("ms_per_step"), "frames_per_s": r.get("value"),
                   "launch_mode": r.get("launch_mode"), "graph_fallback": r.get("graph_fallback"),
                   "parity_rel_err": (r.get("parity") or {}).get("rel_err"),
                   "bits_per_dim_last_step": r.get("bits_per_dim_last_step")} for p, r in runs.items()}
    head = None
    for p in ("mixed", "bf16x3"):
        err = ((runs.get(p) or {}).get("parity") or {}).get("rel_err")
        if err is not None and err <= 1e-4:
            head = p
            break
    if head is None:
        head = "f32" if "f32" in runs else first
    if world > 1:
        head = first
    if a.dump_outputs and head != first:   # the dumped outputs are the headline run's
        for f in os.listdir(os.path.join(tmp, head)):
            shutil.copy(os.path.join(tmp, head, f), os.path.join(a.dump_outputs, f))
    out = dict(runs[first])                     # roofline / cpu_baseline / kernel tables come from the primary run
    for k in ("value", "ms_per_step", "modeled_frames_per_s", "bits_per_dim_last_step", "launch_mode", "dtype",
              "graph_fallback", "parity"):
        if k in runs[head]:
            out[k] = runs[head][k]
    out["precision_runs"] = summary
    out["headline_precision"] = head
    print(json.dumps(out), flush=True)
    return 0


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32, help="GLOBAL batch (sequences)")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also the other arithmetics, parity vs the oracle, forward-only rate, roofline, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/*.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of a captured hipGraph step")
    ap.add_argument("--no-parity", action="store_true", help="skip the GPU-vs-oracle bits/dim check (profiling runs)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--secondary", action="store_true", help=argparse.SUPPRESS)  # second precision: timing + parity only
    return ap


def main():
    a = make_parser().parse_args()

    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    local = int(os.environ.get("LOCAL_RANK", 0))
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no fallback)"
    if os.environ.get("RFN_SINGLE_GPU"):
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        # RFN_DIST_BACKEND=gloo + RFN_SINGLE_GPU=1: rehearsal of the N>1 path on a one-GPU box (all ranks on cuda:0)
        import datetime
        dist.init_process_group(os.environ.get("RFN_DIST_BACKEND", "nccl"), timeout=datetime.timedelta(seconds=300))
    assert world == a.gpus or "--gpus" not in " ".join(sys.argv), \
        "--gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node equal to --gpus" % (a.gpus, world)
    assert a.batch % world == 0, "global batch must divide over ranks"
    B_local = a.batch // world

    solver, args = build_solver(B_local, a.frames, device)
    batches = [make_batch(B_local, a.frames, 100 + rank * 17 + i, device) for i in range(2)]

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    from rfn_hip import lib as rlib
    for i in range(max(a.warmup, 1)):
        solver.train_step(batches[i % 2])
    profile = a.full and rank == 0 and world == 1 and not a.no_roofline and not a.secondary
    rec = None
    if profile:
        # kernel roofline: HIP events on the launch stream around every librfn_hip launch of eager training steps
        # (identical kernels and shapes as the timed region; a captured graph cannot carry per-kernel events)
        barrier()
        rlib.PROFILE = []
        for i in range(2):
            solver.train_step(batches[i % 2])
        torch.cuda.synchronize()
        rec, rlib.PROFILE = rlib.PROFILE, None
    else:
        # same number of optimizer steps in every run, profiled or not, so that `bits_per_dim_last_step` is comparable
        # between the arithmetics of `precision_runs` (and between N = 1 and N > 1)
        for i in range(2):
            solver.train_step(batches[i % 2])
    graphed = False
    if not a.no_graph:
        graphed = solver.capture_graph(batches[0])
        if world > 1:  # all ranks must agree on the mode
            flag = torch.tensor([1 if graphed else 0], device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag) == 0 and graphed:
                solver._graph = None
                solver.reducer.add_hooks()
                graphed = False
        if rank == 0:
            print("[bench] hipGraph capture: %s %s" % ("ok" if graphed else "FAILED -> eager",
                                                      "" if graphed else getattr(solver, "_graph_error", "")),
                  file=sys.stderr, flush=True)
        if graphed:
            solver.train_step(batches[0])  # first replay outside the timed region
    barrier()
    t0 = time.perf_counter()
    trace = os.environ.get("RFN_BENCH_TRACE") == "1"
    for i in range(a.steps):
        solver.train_step(batches[i % 2])
        if trace:
            torch.cuda.synchronize()
            print("[bench] rank %d step %d done at +%.3f s" % (rank, i, time.perf_counter() - t0), file=sys.stderr, flush=True)
    barrier()
    dt = time.perf_counter() - t0
    solver.flush_log()
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, solver)
    if rank == 0:
        print("[bench] timed region done: %.1f ms/step (%s)" % (1e3 * dt / a.steps, "graph" if graphed else "eager"),
              file=sys.stderr, flush=True)
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    from rfn_hip import ops as _ops
    conv_precision = _ops.CONV_PRECISION
    ms_per_step = 1e3 * dt / a.steps
    frames_per_s = a.batch * a.frames * a.steps / dt
    bpd = solver.bits[-1]

    out = {"metric": "frames/sec, RFN SM-MNIST 64x64 train step (fwd+bwd+Adam)", "value": frames_per_s,
           "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_per_step,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": DTYPE_STR[conv_precision], "data": "synthetic",
           "config": {"workload": "RFN SM-MNIST 64x64 canonical (K=10 L=5 Hd=256 h=200 z=56), global_batch=%d, "
                                  "seq_len=%d, train step" % (a.batch, a.frames),
                      "global_batch": a.batch, "seq_len": a.frames, "parallelism": "dp%d" % world},
           "modeled_frames_per_s": a.batch * (a.frames - 1) * a.steps / dt, "bits_per_dim_last_step": bpd,
           "launch_mode": "hipGraph replay (fwd+bwd captured)" if graphed else "eager"}
    if a.full and rank == 0 and world == 1 and a.secondary and not a.no_parity:
        out["parity"] = parity_check(device)
    if a.full and rank == 0 and world == 1 and not a.secondary:
        # forward-only rate: RFN.loss under no_grad on the same batch, eager launches
        with torch.no_grad():
            xin = solver.preprocess(batches[0])
            solver.model.loss(xin, 0)
            torch.cuda.synchronize()
            tf0 = time.perf_counter()
            for _ in range(3):
                solver.model.loss(xin, 0)
            torch.cuda.synchronize()
            out["forward_only_frames_per_s"] = a.batch * a.frames * 3 / (time.perf_counter() - tf0)
        if profile:
            roof, table = kernel_roofline(rec, 2)
            out["roofline"] = roof
            os.makedirs(os.path.join(ROOT, "bench_out"), exist_ok=True)
            with open(os.path.join(ROOT, "bench_out", "bench_kernel_table.json"), "w") as f:
                json.dump({"columns": ["kernel", "launches_per_step", "ms_per_step", "TFLOP/s (fp32-equivalent)",
                                       "algorithmic GB/s"],
                           "rows": table["kernels"], "by_shape": table["shapes"]}, f, indent=1)
        if not a.no_parity:
            out["parity"] = parity_check(device)
        if not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def _gpus_arg(argv):
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            return int(argv[i + 1])
        if a.startswith("--gpus="):
            return int(a.split("=", 1)[1])
    return 1


if __name__ == "__main__":
    if "--child" in sys.argv or os.environ.get("RFN_BENCH_NO_SUPERVISOR") == "1":
        main()
    elif "WORLD_SIZE" not in os.environ and _gpus_arg(sys.argv[1:]) > 1:
        sys.exit(launch_ranks(_gpus_arg(sys.argv[1:])))   # the driver's `python bench.py --gpus N` form
    else:
        sys.exit(supervise())
