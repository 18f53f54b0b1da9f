"""GPU tests of the guard of the Adam step (rfn_grad_sumsq_f32 -> rfn_grad_guard_f32 -> rfn_adam_step_guarded_f32 through
rfn_hip.optim.HipAdam and the Solver): the global gradient norm against fp64, bit identity of an inert guard with the
plain step, clipping against torch's clip_grad_norm_ + Adam, the non-finite skip at every chunk position, no host read
on the steady path, the Solver in eager and hipGraph mode, and two ranks taking the same decision."""
import json
import math
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 8192
# numel 1, 3, 4 (one 16-byte vector), one element short of a chunk, a chunk, one over, two chunks and a tail (N-D), and
# (index 7) a view that is 4-byte but not 16-byte aligned: the scalar path of both kernels
SHAPES = [(1,), (3,), (2, 2), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), (3, 5463), (4097,)]
UNALIGNED = 7


def _unaligned(t):
    buf = torch.zeros(t.numel() + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def make_params(seed=3):
    g = torch.Generator().manual_seed(seed)
    assert 3 * 5463 == 2 * CHUNK + 5
    ps = []
    for j, sh in enumerate(SHAPES):
        t = torch.randn(sh, generator=g).cuda()
        ps.append(torch.nn.Parameter(_unaligned(t) if j == UNALIGNED else t))
    assert ps[UNALIGNED].data_ptr() % 16 == 4
    return ps


def clone_params(ps):
    return [torch.nn.Parameter(_unaligned(p.detach()) if j == UNALIGNED else p.detach().clone()) for j, p in enumerate(ps)]


def make_grads(seed):
    """host gradients randn * (0.1 + j), as test_hip_adam_equals_torch_adam draws them"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(sh, generator=g) * (0.1 + j) for j, sh in enumerate(SHAPES)]


def set_grads(ps, grads, skip=()):
    for j, (p, gr) in enumerate(zip(ps, grads)):
        if j in skip:
            p.grad = None
        else:
            p.grad = _unaligned(gr.cuda()) if j == UNALIGNED else gr.cuda()


def norm64(grads, skip=()):
    return math.sqrt(sum(float(g.double().pow(2).sum()) for j, g in enumerate(grads) if j not in skip))


def bits(x):
    return struct.pack("<f", x)


def steps_of(opt):
    return {k: float(v["step"]) for k, v in opt.state_dict()["state"].items()}


def test_gradient_norm_against_fp64():
    """|norm - fp64 norm| <= 1e-5 relative: <= 32 serial fp32 adds per lane, an 8-level tree and one rounding bound the
    error of the sum of squares by about 41 * 2^-24 = 2.4e-6 and that of its root by half of it; 1e-5 leaves a factor 8.
    The split into replicated and rank-local tensors does not move the norm (one process: nothing is all-reduced), and
    two launches on the same gradients give the same bits."""
    from rfn_hip.optim import HipAdam
    grads = make_grads(11)
    want = norm64(grads)
    got = []
    for local in ((), (3, 6)):
        ps = make_params()
        opt = HipAdam(ps, lr=1e-2, max_grad_norm=1e30, skip_nonfinite=True, rank_local=[ps[j] for j in local])
        set_grads(ps, grads)
        opt.step()
        a = opt.guard_stats()
        opt.step()
        b = opt.guard_stats()
        print("grad_norm", a["grad_norm"], "fp64", want, "rel", abs(a["grad_norm"] - want) / want)
        assert abs(a["grad_norm"] - want) <= 1e-5 * want
        assert bits(a["grad_norm"]) == bits(b["grad_norm"])
        assert a["scale"] == 1.0 and a["skipped_steps"] == 0
        got.append(a["grad_norm"])
    # both are one rounding of a double sum of the same fp32 partials, added in another order: one fp32 ulp at most
    assert abs(got[0] - got[1]) <= 2.0 ** -23 * want


def test_inert_guard_is_bit_identical_to_the_plain_step():
    from rfn_hip.optim import HipAdam
    for wd in (0.0, 0.01):
        pa = make_params()
        pb = clone_params(pa)
        oa = HipAdam(pa, lr=1e-2, weight_decay=wd, max_grad_norm=1e30, skip_nonfinite=True)
        ob = HipAdam(pb, lr=1e-2, weight_decay=wd)
        assert oa.guarded and not ob.guarded
        for i in range(5):
            grads = make_grads(20 + i)
            skip = (2,) if i in (1, 3) else ()     # one tensor without a gradient on two of the steps: its own count
            set_grads(pa, grads, skip)
            set_grads(pb, grads, skip)
            oa.step()
            ob.step()
        assert oa.guard_stats()["scale"] == 1.0 and oa.guard_stats()["skipped_steps"] == 0
        for a, b in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach())
            assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"])
            assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
        sa, sb = steps_of(oa), steps_of(ob)
        assert sa == sb and sa[2] == 3.0 and sa[0] == 5.0
        assert ob._gbuf is None and ob._guard is None      # guard off: nothing was allocated


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_clipping_equals_clip_grad_norm_then_adam(wd):
    """five steps clipped to half the first step's norm against CPU fp32 clip_grad_norm_ + torch.optim.Adam.  rtol 4e-6,
    atol 2e-7: twice the figures of test_hip_adam_equals_torch_adam, because the scale carries the norm's rounding
    (<= 1.2e-6 relative) into every gradient, and lr * steps = 5e-2 bounds what that can move."""
    from rfn_hip.optim import HipAdam
    all_grads = [make_grads(30 + i) for i in range(5)]
    max_norm = 0.5 * norm64(all_grads[0])
    pa = make_params()
    pb = [torch.nn.Parameter(p.detach().cpu().clone()) for p in pa]
    oa = HipAdam(pa, lr=1e-2, weight_decay=wd, max_grad_norm=max_norm)
    ob = torch.optim.Adam(pb, lr=1e-2, weight_decay=wd)
    for grads in all_grads:
        set_grads(pa, grads)
        for p, gr in zip(pb, grads):
            p.grad = gr.clone()
        oa.step()
        torch.nn.utils.clip_grad_norm_(pb, max_norm)
        ob.step()
        want = min(1.0, max_norm / (norm64(grads) + 1e-6))
        gs = oa.guard_stats()
        print("scale", gs["scale"], "fp64", want)
        assert want < 1.0 and abs(gs["scale"] - want) <= 1e-5 * want
    for j, (a, b) in enumerate(zip(pa, pb)):
        torch.testing.assert_close(a.detach().cpu(), b.detach(), rtol=4e-6, atol=2e-7, msg=lambda m: "tensor %d: %s" % (j, m))
        assert torch.equal(a.grad.cpu(), all_grads[-1][j])     # g itself is never written
    assert steps_of(oa) == {k: 5.0 for k in range(len(pa))}


# (tensor, flat positions, value): the first element of all, the last element of a chunk, a chunk of one element, the
# scalar path; two elements of 3e19 are finite but the sum of their squares is not an fp32 number
POISON = [(0, (0,), math.nan), (5, (CHUNK - 1,), math.inf), (5, (CHUNK,), -math.inf), (UNALIGNED, (5, 4000), 3e19)]


def test_non_finite_gradients_skip_the_step():
    from rfn_hip.optim import HipAdam
    pa = make_params()
    pb = clone_params(pa)                                   # the twin never sees a poisoned call
    oa = HipAdam(pa, lr=1e-2, skip_nonfinite=True)
    ob = HipAdam(pb, lr=1e-2, skip_nonfinite=True)
    first = make_grads(40)
    for ps, o in ((pa, oa), (pb, ob)):
        set_grads(ps, first)
        o.step()
    for n, (j, where, value) in enumerate(POISON):
        before = [(p.detach().clone(), oa.state[p]["exp_avg"].clone(), oa.state[p]["exp_avg_sq"].clone()) for p in pa]
        grads = make_grads(41 + n)
        for w in where:
            grads[j].view(-1)[w] = value
        set_grads(pa, grads)
        oa.step()
        gs = oa.guard_stats()
        assert gs["skipped_steps"] == n + 1, (n, gs)
        assert not math.isfinite(gs["grad_norm"]) or value == 3e19, (n, gs)
        for p, (p0, m0, v0) in zip(pa, before):
            assert torch.equal(p.detach(), p0) and torch.equal(oa.state[p]["exp_avg"], m0)
            assert torch.equal(oa.state[p]["exp_avg_sq"], v0)
        assert steps_of(oa) == {k: 1.0 for k in range(len(pa))}
    last = make_grads(50)
    for ps, o in ((pa, oa), (pb, ob)):
        set_grads(ps, last)
        o.step()
    for a, b in zip(pa, pb):                                # bias corrections of step 2 on both: the count did not advance
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
        assert bool(torch.isfinite(a).all())
    assert steps_of(oa) == steps_of(ob) == {k: 2.0 for k in range(len(pa))}
    assert oa.guard_stats()["skipped_steps"] == len(POISON) and ob.guard_stats()["skipped_steps"] == 0
    # a state dict written after skipped steps continues in torch.optim.Adam with the same counts
    ref = torch.optim.Adam([torch.nn.Parameter(p.detach().cpu().clone()) for p in pa], lr=1e-2)
    ref.load_state_dict(oa.state_dict())
    assert all(float(st["step"]) == 2.0 for st in ref.state.values())
    # the default: no guard, and the same NaN does poison the parameters
    pc = make_params()
    oc = HipAdam(pc, lr=1e-2)
    grads = make_grads(41)
    grads[0].view(-1)[0] = math.nan
    set_grads(pc, grads)
    oc.step()
    assert bool(torch.isnan(pc[0]).all()) and bool(torch.isfinite(pc[1]).all())


def test_steady_path_reads_nothing_from_the_device():
    """while the pointer table is unchanged (hipGraph mode: static gradient tensors) a guarded step must not synchronise"""
    from rfn_hip.optim import HipAdam
    ps = make_params()
    opt = HipAdam(ps, lr=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
    set_grads(ps, make_grads(60))
    opt.step()                                              # builds the table (reads are allowed there)
    probe = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                   # the mode is live: a host read is an error
            float(probe.sum())
        opt.step()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    gs = opt.guard_stats()
    assert gs["skipped_steps"] == 0 and gs["scale"] < 1.0 and steps_of(opt)[0] == 3.0


def _guarded_solver(tmp_path, seed):
    import os
    from RFN import RFN
    from RFN.trainer import Solver
    from rfn_hip import dist as rdist
    from rfn_hip.optim import HipAdam
    from tests.test_hip_modules import _tiny_solver_args
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = _tiny_solver_args(rel)
    args.grad_clip_norm, args.skip_nonfinite_steps = 1.0, True
    torch.manual_seed(seed)
    s = Solver(args)
    s.device = torch.device("cuda")
    s.model = RFN(args).cuda().train()
    s.reducer = rdist.GradBucketReducer(list(s.model.named_parameters()))
    s.optimizer = s.make_optimizer(s.model.parameters(), 1e-3, **s.guard_kwargs())
    assert isinstance(s.optimizer, HipAdam) and s.optimizer.guarded and s.optimizer.max_grad_norm == 1.0
    g = torch.Generator().manual_seed(seed + 1)
    clean = torch.rand(2, 4, 1, 16, 16, generator=g).cuda()
    bad = clean.clone()
    bad[1, 2, 0, 5, 7] = math.nan                           # one NaN pixel
    return s, clean, bad


def _snapshot(s):
    return [p.detach().clone() for p in s.model.parameters()]


def _flow_param(s):
    return next(p for p in s.model.flow.parameters() if p.grad is not None)


def test_solver_eager_skips_the_nan_batch(tmp_path):
    s, clean, bad = _guarded_solver(tmp_path, 61)
    s.train_step(clean)                                     # initialises ActNorm
    before = _snapshot(s)
    s.train_step(bad)
    assert all(torch.equal(p.detach(), q) for p, q in zip(s.model.parameters(), before))
    assert s.guard_stats()["skipped_steps"] == 1
    assert len(s.losses) == 1 and all(math.isfinite(v) for h in (s.losses, s.kl_loss, s.recon_loss, s.bits) for v in h)
    s.train_step(clean)
    gs = s.guard_stats()
    assert gs["skipped_steps"] == 1 and math.isfinite(gs["grad_norm"]) and 0.0 < gs["scale"] <= 1.0
    assert any(not torch.equal(p.detach(), q) for p, q in zip(s.model.parameters(), before))
    assert all(bool(torch.isfinite(p).all()) for p in s.model.parameters())
    assert len(s.losses) == 2 and all(math.isfinite(v) for v in s.losses + s.bits)
    assert float(s.optimizer.state[_flow_param(s)]["step"]) == 2.0


def test_solver_graph_mode_skips_the_nan_batch(tmp_path):
    import rfn_hip
    if not rfn_hip.graph_capture_safe():
        pytest.skip("hipGraph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before the HIP runtime starts")
    s, clean, bad = _guarded_solver(tmp_path, 71)
    s.train_step(clean)                                     # eager: initialises ActNorm
    assert s.capture_graph(clean), getattr(s, "_graph_error", "")
    s.train_step(clean)
    s.flush_log()
    assert len(s.losses) == 2
    before = _snapshot(s)
    s.train_step(bad)
    s.flush_log()                                           # the NaN replay appends nothing
    assert [len(h) for h in (s.losses, s.kl_loss, s.recon_loss, s.bits)] == [2, 2, 2, 2]
    assert all(torch.equal(p.detach(), q) for p, q in zip(s.model.parameters(), before))
    assert s.guard_stats()["skipped_steps"] == 1
    s.train_step(clean)
    s.flush_log()
    assert len(s.losses) == 3 and all(math.isfinite(v) for v in s.losses + s.bits)
    assert any(not torch.equal(p.detach(), q) for p, q in zip(s.model.parameters(), before))
    assert all(bool(torch.isfinite(p).all()) for p in s.model.parameters())
    gs = s.guard_stats()
    assert gs["skipped_steps"] == 1 and math.isfinite(gs["grad_norm"])
    assert float(s.optimizer.state[_flow_param(s)]["step"]) == 3.0


_DP_GUARD_WORKER = r"""
import json, math, os, struct, sys
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "recurrent-flows-msc_amd"))
import torch, torch.distributed as dist
from rfn_hip.optim import HipAdam
rank = int(os.environ["RANK"])
torch.cuda.set_device(0)
dist.init_process_group("gloo")
g = torch.Generator().manual_seed(7)                       # the replicated tensors: the same on both ranks
shapes = [(5,), (8193,), (30, 10)]
rep = [torch.nn.Parameter(torch.randn(sh, generator=g).cuda()) for sh in shapes]
rep_g = [torch.randn(sh, generator=g) * (1 + j) for j, sh in enumerate(shapes)]
gl = torch.Generator().manual_seed(100 + rank)             # the rank-local tensor: this rank's own
loc = torch.nn.Parameter(torch.randn(1000, generator=gl).cuda())
loc_g = torch.randn(1000, generator=gl) * 3
opt = HipAdam(rep + [loc], lr=1e-2, max_grad_norm=1.0, skip_nonfinite=True, rank_local=[loc])
def checksum(ps):
    return sum(int(p.detach().view(torch.int32).to(torch.int64).sum()) for p in ps)
out = {"rep_sq": sum(float(t.double().pow(2).sum()) for t in rep_g), "loc_sq": float(loc_g.double().pow(2).sum())}
for rnd in range(2):
    for p, t in zip(rep, rep_g):
        p.grad = t.cuda()
    loc.grad = loc_g.cuda()
    if rnd == 1 and rank == 1:
        loc.grad[17] = math.nan                            # only rank 1's local gradient is poisoned
    opt.step()
    gs = opt.guard_stats()
    out["round%d" % rnd] = {"norm_bits": struct.pack("<f", gs["grad_norm"]).hex(), "norm": gs["grad_norm"],
                            "scale": gs["scale"], "skipped": gs["skipped_steps"], "rep_sum": checksum(rep),
                            "loc_sum": checksum([loc])}
dist.destroy_process_group()
print("RESULT " + json.dumps(out))
"""


def test_two_ranks_take_the_same_decision(tmp_path):
    """gloo rehearsal on one GPU: the norm is that of one process on {replicated once, both rank-local tensors}, equal
    bit for bit on both ranks, so the clipped replicated parameters stay bit-equal; a NaN in one rank's local gradient
    makes both ranks skip."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    script = tmp_path / "dp_guard_worker.py"
    script.write_text(_DP_GUARD_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29771", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    res = []
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "RESULT " in o, "rank %d failed:\n%s" % (r, o[-3000:])
        res.append(json.loads(o[o.index("RESULT ") + 7:].splitlines()[0]))
    a, b = res
    assert a["rep_sq"] == b["rep_sq"] and a["loc_sq"] != b["loc_sq"]
    want = math.sqrt(a["rep_sq"] + a["loc_sq"] + b["loc_sq"])
    assert a["round0"]["norm_bits"] == b["round0"]["norm_bits"]
    assert abs(a["round0"]["norm"] - want) <= 1e-5 * want, (a["round0"]["norm"], want)
    assert a["round0"]["scale"] == b["round0"]["scale"] < 1.0
    assert a["round0"]["rep_sum"] == b["round0"]["rep_sum"] and a["round0"]["loc_sum"] != b["round0"]["loc_sum"]
    assert a["round0"]["skipped"] == b["round0"]["skipped"] == 0
    for r0, r1 in ((a["round0"], a["round1"]), (b["round0"], b["round1"])):
        assert r1["skipped"] == 1 and math.isnan(r1["norm"])
        assert r1["rep_sum"] == r0["rep_sum"] and r1["loc_sum"] == r0["loc_sum"]
