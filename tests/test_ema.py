"""GPU tests of the Polyak average of the weights inside the Adam launch: rfn_adam_ema_step_f32 called directly against a
float64 restatement of the definition and against rfn_adam_step_f32 on clones (p, m, v bit for bit) on both the 16-byte
and the scalar path, the per-tensor step count, the guarded route (skip and clip), rfn_param_swap_f32, the refusals of
the entry points, and a tiny Solver run: checkpoint, reload, ema_weights(), tools/export_ema.py, and nothing new at all
with the flag off."""
import ctypes
import math
import os

import pytest
import torch

from tests.test_ema_host import decay_at, load_export_ema, restate

pytestmark = pytest.mark.gpu

CHUNK = 8192
# one element, less than a 16-byte vector, exactly one, a vector tail, one chunk, one over, two chunks and a tail; then
# (P_OFF) a tensor whose p, g, m, v, ema are all views one float past a 16-byte boundary and (A_OFF) one where only the
# average is: both take the scalar loop
SIZES = [1, 3, 4, 255, CHUNK, CHUNK + 1, 20000, 4097, 1027]
P_OFF, A_OFF = 7, 8
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8


def _offset(t):
    buf = torch.zeros(t.numel() + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _place(t, j, kind):
    t = t.cuda()
    return _offset(t) if j == P_OFF or (j == A_OFF and kind == "ema") else t


class Tensors:
    """p, g, m, v (and the averages) of SIZES on the device, with the table, chunk list and pointer array of the entry
    points"""

    def __init__(self, seed, ema=True):
        from rfn_hip import lib as L
        g = torch.Generator().manual_seed(seed)
        host = [torch.randn(n, generator=g) for n in SIZES]
        self.p = [_place(t, j, "p") for j, t in enumerate(host)]
        self.g = [_place(torch.zeros(n), j, "g") for j, n in enumerate(SIZES)]
        self.m = [_place(torch.zeros(n), j, "m") for j, n in enumerate(SIZES)]
        self.v = [_place(torch.zeros(n), j, "v") for j, n in enumerate(SIZES)]
        self.ema = [_place(t, j, "ema") for j, t in enumerate(host)] if ema else None
        ent = (L.rfn_adam_entry * len(SIZES))()
        chunks = []
        for j, n in enumerate(SIZES):
            ent[j] = L.rfn_adam_entry(self.p[j].data_ptr(), self.g[j].data_ptr(), self.m[j].data_ptr(),
                                      self.v[j].data_ptr(), n, 0, 0)
            nck = (n + CHUNK - 1) // CHUNK
            chunks += [(j, c) for c in range(nck)]
        self.nck = len(chunks)
        self.tab = torch.frombuffer(ent, dtype=torch.uint8).cuda()
        self.chk = torch.tensor(chunks, dtype=torch.int32).reshape(-1).cuda()
        if ema:
            ptrs = (ctypes.c_void_p * len(SIZES))(*[a.data_ptr() for a in self.ema])
            self.ptrs = torch.frombuffer(ptrs, dtype=torch.uint8).cuda()

    def set_grads(self, seed):
        g = torch.Generator().manual_seed(seed)
        for j, n in enumerate(SIZES):
            self.g[j].copy_(torch.randn(n, generator=g) * (0.1 + j))

    def snapshot(self):
        return [[t.clone() for t in ts] for ts in (self.p, self.m, self.v) + ((self.ema,) if self.ema else ())]


def test_sizes_cover_both_paths():
    from rfn_hip import lib as L
    assert int(L.load().rfn_adam_chunk_elems()) == CHUNK
    t = Tensors(1)
    for j in range(len(SIZES)):
        aligned = [x[j].data_ptr() % 16 == 0 for x in (t.p, t.g, t.m, t.v, t.ema)]
        assert aligned == ([False] * 5 if j == P_OFF else [True] * 4 + [False] if j == A_OFF else [True] * 5)


def test_kernel_against_the_restatement_and_the_plain_kernel():
    """five steps.  p, m, v: the bits of rfn_adam_step_f32 on clones after every step.  ema: the float64 restatement fed
    the kernel's own float32 p sequence; after N steps |err| <= N * 2^-23 * M per element, M the largest |p|, |ema| the
    tensor has seen: each update is one rounded subtraction and one rounded fma (2^-24 relative each, of magnitudes
    <= M), and the recursion contracts (the old error is scaled by 1 - w <= 1)."""
    from rfn_hip import lib as L
    d = 0.999
    a, b = Tensors(3), Tensors(3, ema=False)
    ema64 = [e.double().cpu() for e in a.ema]
    M = [float(e.abs().max()) for e in a.ema]
    worst = 0.0
    for t in range(1, 6):
        a.set_grads(100 + t)
        b.set_grads(100 + t)
        L.call("rfn_adam_ema_step_f32", a.tab.data_ptr(), a.chk.data_ptr(), a.nck, LR, B1, B2, EPS, 0.0, t, d,
               a.ptrs.data_ptr())
        L.call("rfn_adam_step_f32", b.tab.data_ptr(), b.chk.data_ptr(), b.nck, LR, B1, B2, EPS, 0.0, t)
        for j in range(len(SIZES)):
            assert torch.equal(a.p[j], b.p[j]) and torch.equal(a.m[j], b.m[j]) and torch.equal(a.v[j], b.v[j]), (t, j)
            p = a.p[j].cpu()
            ema64[j] = restate(ema64[j], p, d, t)
            got = a.ema[j].cpu()
            M[j] = max(M[j], float(p.abs().max()), float(got.abs().max()))
            err = float((got.double() - ema64[j]).abs().max())
            bound = t * 2.0 ** -23 * M[j]
            worst = max(worst, err / bound)
            assert err <= bound, (t, j, err, bound)
            assert not torch.equal(got, p)                       # an average, not a copy
    print("largest err / bound:", worst)


def test_weight_decay_keeps_the_plain_bits_too():
    from rfn_hip import lib as L
    a, b = Tensors(4), Tensors(4, ema=False)
    for t in range(1, 3):
        a.set_grads(120 + t)
        b.set_grads(120 + t)
        L.call("rfn_adam_ema_step_f32", a.tab.data_ptr(), a.chk.data_ptr(), a.nck, LR, B1, B2, EPS, 0.01, t, 0.9,
               a.ptrs.data_ptr())
        L.call("rfn_adam_step_f32", b.tab.data_ptr(), b.chk.data_ptr(), b.nck, LR, B1, B2, EPS, 0.01, t)
    for j in range(len(SIZES)):
        assert torch.equal(a.p[j], b.p[j]) and torch.equal(a.m[j], b.m[j]) and torch.equal(a.v[j], b.v[j]), j


# ---- through rfn_hip.optim.HipAdam ------------------------------------------------------------------------------------
SHAPES = [(1,), (3,), (2, 2), (CHUNK + 1,), (3, 5463), (4097,)]
LATE = 2        # the tensor without a gradient on two of the steps
UNALIGNED = 5


def _params(seed=3):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for j, sh in enumerate(SHAPES):
        t = torch.randn(sh, generator=g).cuda()
        ps.append(torch.nn.Parameter(_offset(t.view(-1)).view(sh) if j == UNALIGNED else t))
    return ps


def _set_grads(ps, seed, skip=(), poison=None):
    g = torch.Generator().manual_seed(seed)
    for j, p in enumerate(ps):
        gr = torch.randn(p.shape, generator=g) * (0.1 + j)
        if poison is not None and j == poison[0]:
            gr.view(-1)[poison[1]] = poison[2]
        p.grad = None if j in skip else (_offset(gr.view(-1).cuda()).view(p.shape) if j == UNALIGNED else gr.cuda())


def _state(opt, ps):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(),
             opt.state[p]["ema"].clone()) for p in ps if opt.state[p]]


def test_hip_adam_rejects_a_bad_decay_and_keeps_no_state_when_off():
    from rfn_hip.optim import HipAdam
    for bad in (1.0, -0.1, math.nan):
        with pytest.raises(ValueError):
            HipAdam(_params(), lr=LR, ema_decay=bad)
    ps = _params()
    opt = HipAdam(ps, lr=LR)
    _set_grads(ps, 1)
    opt.step()
    assert all(sorted(opt.state[p]) == ["exp_avg", "exp_avg_sq", "step"] for p in ps)
    assert opt._ema is None
    with pytest.raises(RuntimeError):
        opt.swap_ema()


def test_each_tensor_decays_by_its_own_step_count():
    from rfn_hip.optim import HipAdam
    d = 0.999
    pa, pb = _params(), _params()
    oa, ob = HipAdam(pa, lr=LR, ema_decay=d), HipAdam(pb, lr=LR)
    ema64, own = {}, {j: 0 for j in range(len(SHAPES))}
    for i in range(5):
        skip = (LATE,) if i in (0, 3) else ()
        _set_grads(pa, 20 + i, skip)
        _set_grads(pb, 20 + i, skip)
        for j, p in enumerate(pa):                               # the average starts as the parameter before its first update
            if j not in skip and j not in ema64:
                ema64[j] = p.detach().double().cpu()
        oa.step()
        ob.step()
        for j, (a, b) in enumerate(zip(pa, pb)):
            assert torch.equal(a.detach(), b.detach())
            if j in skip:
                continue
            own[j] += 1
            assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"])
            ema64[j] = restate(ema64[j], a.detach().cpu(), d, own[j])
    assert own[LATE] == 3 and own[0] == 5
    steps = {k: float(v["step"]) for k, v in oa.state_dict()["state"].items()}
    assert steps[LATE] == 3.0 and steps[0] == 5.0
    for j, a in enumerate(pa):
        got = oa.state[a]["ema"]
        assert got.dtype == torch.float32 and got.shape == a.shape and got.data_ptr() != a.data_ptr()
        # (M of the bound above from the final values: Adam moves an element by about lr a step, 5 * lr covers the past)
        M = max(float(a.detach().abs().max()), float(got.abs().max()), float(ema64[j].abs().max())) + 5 * LR
        assert float((got.double().cpu() - ema64[j]).abs().max()) <= own[j] * 2.0 ** -23 * M, j
    # the late tensor's last step was its third, the launch's fifth: d_3 = 4/13 against d_5 = 6/15 is far outside
    a = pa[LATE]
    prev = (oa.state[a]["ema"].double().cpu() - (1 - decay_at(d, 3)) * a.detach().double().cpu()) / decay_at(d, 3)
    by_t = restate(prev, a.detach().cpu(), d, 5)
    assert float((oa.state[a]["ema"].double().cpu() - by_t).abs().max()) > 1e-4


def test_guarded_route_skips_and_clips():
    from rfn_hip.optim import HipAdam
    d = 0.999
    ps = _params()
    opt = HipAdam(ps, lr=LR, skip_nonfinite=True, ema_decay=d)
    ema64 = [p.detach().double().cpu() for p in ps]
    _set_grads(ps, 40)
    opt.step()
    ema64 = [restate(e, p.detach().cpu(), d, 1) for e, p in zip(ema64, ps)]
    before = _state(opt, ps)
    _set_grads(ps, 41, poison=(3, CHUNK, math.inf))
    opt.step()
    assert opt.guard_stats()["skipped_steps"] == 1
    for old, new in zip(before, _state(opt, ps)):
        assert all(torch.equal(x, y) for x, y in zip(old, new))  # p, m, v and ema keep their bits
    _set_grads(ps, 42)
    opt.step()
    assert opt.guard_stats()["skipped_steps"] == 1
    for j, p in enumerate(ps):
        got = opt.state[p]["ema"].double().cpu()
        M = max(float(p.detach().abs().max()), float(got.abs().max())) + 2 * LR
        want = restate(ema64[j], p.detach().cpu(), d, 2)         # n = 2: the skipped step is not counted
        wrong = restate(ema64[j], p.detach().cpu(), d, 3)
        assert float((got - want).abs().max()) <= 2 * 2.0 ** -23 * M, j
        assert float((got - wrong).abs().max()) > 2 * 2.0 ** -23 * M, j
        assert float(opt.state[p]["step"]) == 2.0
    # clipping: the bits of the guarded kernel without the average
    pa, pb = _params(5), _params(5)
    oa = HipAdam(pa, lr=LR, max_grad_norm=0.5, skip_nonfinite=True, ema_decay=d)
    ob = HipAdam(pb, lr=LR, max_grad_norm=0.5, skip_nonfinite=True)
    for i in range(3):
        _set_grads(pa, 50 + i)
        _set_grads(pb, 50 + i)
        oa.step()
        ob.step()
    assert oa.guard_stats()["scale"] < 1.0 and oa.guard_stats() == ob.guard_stats()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"])
        assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
        assert "ema" in oa.state[a] and "ema" not in ob.state[b]


def test_swap_exchanges_parameters_and_averages():
    from rfn_hip import lib as L
    from rfn_hip.optim import HipAdam
    ps = _params()
    opt = HipAdam(ps, lr=LR, ema_decay=0.9)
    _set_grads(ps, 60)
    opt.step()
    _set_grads(ps, 61, skip=(LATE,))                             # the last table lacks one tensor: the swap must not
    opt.step()
    raw = [p.detach().clone() for p in ps]
    avg = [opt.state[p]["ema"].clone() for p in ps]
    assert all(not torch.equal(r, a) for r, a in zip(raw, avg))
    versions = [p._version for p in ps]
    L.PROFILE = rec = []
    try:
        opt.swap_ema()
    finally:
        L.PROFILE = None
    assert [r[0] for r in rec] == ["rfn_param_swap_f32"]         # one launch
    assert all(torch.equal(p.detach(), a) for p, a in zip(ps, avg))
    assert all(torch.equal(opt.state[p]["ema"], r) for p, r in zip(ps, raw))
    assert all(p._version > v for p, v in zip(ps, versions))
    opt.swap_ema()
    assert all(torch.equal(p.detach(), r) for p, r in zip(ps, raw))
    assert all(torch.equal(opt.state[p]["ema"], a) for p, a in zip(ps, avg))
    # the state dict carries the average, and a state without one starts it from the loaded parameter
    sd = opt.state_dict()
    assert all(torch.equal(sd["state"][j]["ema"], avg[j]) for j in range(len(ps)))
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    other = HipAdam(qs, lr=LR, ema_decay=0.9)
    other.load_state_dict(sd)
    assert all(torch.equal(other.state[q]["ema"], a) for q, a in zip(qs, avg))
    sd = dict(sd, state={k: {n: x for n, x in st.items() if n != "ema"} for k, st in sd["state"].items()})
    other.load_state_dict(sd)
    assert all("ema" not in other.state[q] for q in qs)
    _set_grads(qs, 62)
    other.step()
    for q, r in zip(qs, raw):                                    # ema_1 = raw + (9/11) (p_1 - raw)
        want = restate(r.double().cpu(), q.detach().cpu(), 0.9, 3 if q is not qs[LATE] else 2)
        assert float((other.state[q]["ema"].double().cpu() - want).abs().max()) <= 2.0 ** -23 * (float(r.abs().max()) + LR)


def test_entry_points_refuse_a_null_average_and_a_bad_decay():
    from rfn_hip import lib as L
    lib = L.load()
    t = Tensors(7)
    t.set_grads(70)
    stats = torch.tensor([0.0, 1.0, 0.0], device="cuda")
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    before = t.snapshot()
    stream = torch.cuda.current_stream().cuda_stream
    common = (t.tab.data_ptr(), t.chk.data_ptr(), t.nck, LR, B1, B2, EPS, 0.0, 1)
    guard = (stats.data_ptr(), skipped.data_ptr())
    for decay, ptrs in ((0.9, None), (1.0, t.ptrs.data_ptr()), (-0.5, t.ptrs.data_ptr()), (math.nan, t.ptrs.data_ptr())):
        for rc in (lib.rfn_adam_ema_step_f32(*common, decay, ptrs, stream),
                   lib.rfn_adam_ema_step_guarded_f32(*common, *guard, decay, ptrs, stream)):
            assert rc != 0
            assert b"argument check failed" in lib.rfn_last_error()
    assert lib.rfn_param_swap_f32(t.tab.data_ptr(), t.chk.data_ptr(), t.nck, None, stream) != 0
    assert b"rfn_param_swap_f32" in lib.rfn_last_error()
    with pytest.raises(RuntimeError, match="ema"):
        L.call("rfn_adam_ema_step_f32", *common, 0.9, None)
    torch.cuda.synchronize()
    for old, new in zip(before, t.snapshot()):                   # nothing was launched
        assert all(torch.equal(x, y) for x, y in zip(old, new))
    # and the same arguments with a valid decay and array do run
    assert lib.rfn_adam_ema_step_f32(*common, 0.0, t.ptrs.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    for j in range(len(SIZES)):                                  # d = 0: w = 1, the average follows the parameter
        assert not torch.equal(t.p[j], before[0][j])
        assert float((t.ema[j] - t.p[j]).abs().max()) <= 2.0 ** -23 * float(t.p[j].abs().max())


# ---- a tiny Solver ---------------------------------------------------------------------------------------------------
def _recorded_train(s):
    from rfn_hip import lib as L
    L.PROFILE = rec = []
    try:
        s.train()
        torch.cuda.synchronize()
    finally:
        L.PROFILE = None
    return [r[0] for r in rec]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the same three steps with --ema_decay 0.9 (and a sheet) and without: trained once for the tests below"""
    from tests.test_sheet import _tiny_solver
    root = tmp_path_factory.mktemp("ema_runs")
    on = _tiny_solver(root / "on", "--ema_decay 0.9 --max_steps 3 --plot_every 1")
    on_calls = _recorded_train(on)
    off = _tiny_solver(root / "off", "--ema_decay 0 --max_steps 3")
    off_calls = _recorded_train(off)
    return {"root": root, "on": on, "on_calls": on_calls, "off": off, "off_calls": off_calls}


def _ckpt(s):
    from RFN.trainer import Solver
    return Solver.read_checkpoint(s.path + "model_folder/rfn.pt")


def test_solver_keeps_the_average_in_the_optimizer_state(runs):
    on, off = runs["on"], runs["off"]
    assert on.counter == off.counter == 3 and on.optimizer.ema_decay == 0.9
    assert len(on.optimizer.state) > 0
    for p, st in on.optimizer.state.items():
        assert st["ema"].shape == p.shape and st["ema"].dtype == torch.float32 and st["ema"].is_cuda
    assert any(not torch.equal(st["ema"], p.detach()) for p, st in on.optimizer.state.items())
    assert runs["on_calls"].count("rfn_adam_ema_step_f32") == 3 and "rfn_adam_step_f32" not in runs["on_calls"]
    assert runs["on_calls"].count("rfn_param_swap_f32") == 2     # the sheet: swapped in, drawn, swapped out
    assert os.listdir(on.path + "png_folder") == ["samples0.png"]
    a, b = _ckpt(on), _ckpt(off)
    assert list(a) == list(b)                                    # the average travels inside optimizer_state_dict
    for i, st in a["optimizer_state_dict"]["state"].items():
        p = list(on.model.parameters())[i]
        assert torch.equal(st["ema"], on.optimizer.state[p]["ema"].cpu())


def test_flag_off_records_no_new_launch_and_no_new_key(runs):
    off = runs["off"]
    assert runs["off_calls"].count("rfn_adam_step_f32") == 3
    assert not [c for c in runs["off_calls"] if "ema" in c or "swap" in c]
    assert all("ema" not in st for st in off.optimizer.state.values())
    assert all("ema" not in st for st in _ckpt(off)["optimizer_state_dict"]["state"].values())
    assert off.optimizer._ema is None and off.optimizer._swap is None


def test_load_restores_the_average_and_ema_weights_swaps(runs):
    from tests.test_sheet import _tiny_solver
    on = runs["on"]
    fresh = _tiny_solver(runs["root"] / "fresh", "--ema_decay 0.9 --max_steps 3")
    fresh.load(_ckpt(on))
    pairs = list(zip(fresh.model.parameters(), on.model.parameters()))
    for q, p in pairs:
        assert torch.equal(q.detach(), p.detach())
        assert ("ema" in fresh.optimizer.state[q]) == ("ema" in on.optimizer.state[p])
        if on.optimizer.state[p]:
            assert torch.equal(fresh.optimizer.state[q]["ema"], on.optimizer.state[p]["ema"])
    raw = [q.detach().clone() for q, _ in pairs]
    avg = [fresh.optimizer.state[q]["ema"].clone() if fresh.optimizer.state[q] else q.detach().clone() for q, _ in pairs]
    buffers = [b.clone() for b in fresh.model.buffers()]
    versions = [q._version for q, _ in pairs]
    with fresh.ema_weights():                                    # (before any step of this Solver: no Adam table yet)
        assert all(torch.equal(q.detach(), a) for (q, _), a in zip(pairs, avg))
        assert all(q._version > v for (q, _), v in zip(pairs, versions) if fresh.optimizer.state[q])
    assert all(torch.equal(q.detach(), r) for (q, _), r in zip(pairs, raw))
    assert all(torch.equal(fresh.optimizer.state[q]["ema"], a) for (q, _), a in zip(pairs, avg) if fresh.optimizer.state[q])
    assert all(torch.equal(b, c) for b, c in zip(fresh.model.buffers(), buffers))
    # a run without the flag drops the file's average instead of carrying it along unchanged
    plain = _tiny_solver(runs["root"] / "plain", "--max_steps 3")
    plain.load(_ckpt(on))
    assert all("ema" not in st for st in plain.optimizer.state.values())
    # load_ema_weights: the averages become the weights
    assert plain.load_ema_weights(_ckpt(on)) == len([1 for q, _ in pairs if fresh.optimizer.state[q]])
    assert all(torch.equal(p.detach(), a) for p, a in zip(plain.model.parameters(), avg))
    with pytest.raises(ValueError, match="no averaged weights"):
        plain.load_ema_weights(_ckpt(runs["off"]))


def test_export_ema_writes_a_run_the_solver_loads(runs):
    from tests.test_sheet import _tiny_solver
    X = load_export_ema()
    on = runs["on"]
    folder = os.path.dirname(on.path.rstrip("/")) + "/"
    X.main(["--folder_path", folder, "--experiment_names", "on"])
    assert sorted(os.listdir(folder + "on_ema/model_folder")) == sorted(os.listdir(folder + "on/model_folder"))
    from RFN.trainer import Solver
    src, out = _ckpt(on), Solver.read_checkpoint(folder + "on_ema/model_folder/rfn.pt")
    assert list(out) == list(src)
    # a parameter that two modules share is saved under both names, and both must hold the average
    keys = X.param_keys_of(on.model)
    assert len(keys) == len(list(on.model.parameters())) and any(len(k) > 1 for k in keys)
    emas = {k: st["ema"] for i, st in src["optimizer_state_dict"]["state"].items() for k in keys[i]}
    assert emas
    for k, v in out["model_state_dict"].items():
        assert torch.equal(v, emas[k] if k in emas else src["model_state_dict"][k]), k
    names = {k for ks in keys for k in ks}
    assert any(k not in names for k in out["model_state_dict"])  # the model has buffers, and they were kept
    s = _tiny_solver(runs["root"] / "from_export", "--max_steps 3")
    s.load(out)
    for (n, p) in s.model.named_parameters():
        assert torch.equal(p.detach().cpu(), emas[n] if n in emas else src["model_state_dict"][n])
    with pytest.raises(ValueError, match="no checkpoint with averaged weights"):
        X.export_folder(runs["off"].path + "model_folder", str(runs["root"] / "nothing"))
