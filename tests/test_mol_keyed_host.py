"""CPU tests of the mixture sampler's addressed uniforms (csrc/mol.hip: rfn_mol_sample_keyed / rfn_mol_keyed_uniforms;
DESIGN.md section 20) and of the host-side rules of evaluating srnn.pt.  The numpy restatement below
(mol_keyed_uniforms_ref) is the definition the GPU kernels are compared with in tests/test_mol_keyed.py; it is built on
the Philox4x64-10 restatement of tests/test_keyed_normal_host.py, which is checked against numpy's generator there.

  block j of pixel p = Philox4x64-10(key = (seed, (step << 32) | slot), counter = (j, p, seq, draw))
  slot 16: mixture uniforms, slot 17: colour uniforms (keyed_normal owns slots 0..7)
  uniform e of the pixel = 32-bit half e % 8 of block e / 8; halves: high w0, low w0, high w1, low w1, ...
  u = min(max((2 (half >> 9) + 1) 2^-24, 1e-5f), 1 - 1e-5f)       (all float32, all exact)
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rfn_hip import ops
from tests.test_keyed_normal_host import LO32, S32, U64, philox4x64_10_blocks

SLOT_MIX, SLOT_COLOUR = ops.MOL_KEYED_SLOT_MIX, ops.MOL_KEYED_SLOT_COLOUR   # 16 and 17: asserted below
U_LO = np.float32(1e-5)
U_HI = np.float32(1.0) - np.float32(1e-5)


# ---------------------------------------------------------------------------------------------- the restatement
def mol_key(seed, step, slot):
    return (int(seed), (int(step) << 32) | int(slot))


def mol_halves(seed, step, slot, seq, draw, pixels, n_blocks):
    """uint32 [len(pixels), 8 * n_blocks]: the 32-bit halves of blocks 0 .. n_blocks-1 of every pixel, in order"""
    pixels = np.asarray(pixels, dtype=U64)
    j = np.arange(n_blocks, dtype=U64)
    words = philox4x64_10_blocks(j[None, :], pixels[:, None], int(seq), int(draw), mol_key(seed, step, slot))
    w = np.stack(words, axis=2)                                   # [pixels, blocks, 4]
    halves = np.stack([w >> S32, w & LO32], axis=3)               # high half first
    return halves.reshape(len(pixels), n_blocks * 8).astype(np.uint32)


def mol_uniform(halves):
    u = (2 * (halves >> np.uint32(9)) + 1).astype(np.float32) * np.float32(2.0 ** -24)
    return np.minimum(np.maximum(u, U_LO), U_HI)


def mol_keyed_uniforms_ref(rows, B, HW, M, C, seed, step, first_seq=0, first_draw=0):
    """(u_mix float32 [rows, HW, M], u_x float32 [rows, HW, C]): row i is draw first_draw + i // B of sequence
    first_seq + i % B"""
    p = np.arange(HW)
    u_mix = np.empty((rows, HW, M), np.float32)
    u_x = np.empty((rows, HW, C), np.float32)
    for i in range(rows):
        seq, draw = first_seq + i % B, first_draw + i // B
        u_mix[i] = mol_uniform(mol_halves(seed, step, SLOT_MIX, seq, draw, p, (M + 7) // 8))[:, :M]
        u_x[i] = mol_uniform(mol_halves(seed, step, SLOT_COLOUR, seq, draw, p, 1))[:, :C]
    return u_mix, u_x


# ---------------------------------------------------------------------------------------------- the uniform map
def test_uniform_map_range_and_moments():
    """2^17 values per slot.  The unclamped map is uniform on the odd multiples of 2^-24: mean 1/2, variance 1/12 -
    2^-48/3; the clamp moves 1e-5 of the mass at each end by less than 1e-5, which changes neither beyond 1e-9.  The
    standard error of the mean of n = 2^18 values is 0.289 / 512 = 5.6e-4 and that of the variance 0.0745 / 512 =
    1.5e-4, so the bands of the issue (0.005 and 0.002) are 9 and 13 sigma wide."""
    n_pix = 1 << 14
    u = np.concatenate([mol_uniform(mol_halves(20261020, 3, slot, 5, 2, np.arange(n_pix), 1)).reshape(-1)
                        for slot in (SLOT_MIX, SLOT_COLOUR)]).astype(np.float64)
    assert u.size >= 100000
    print("min %.3e  1-max %.3e  mean %.6f  var %.6f" % (u.min(), 1 - u.max(), u.mean(), u.var()))
    assert u.min() >= float(U_LO) and u.max() <= float(U_HI)
    assert abs(u.mean() - 0.5) <= 0.005
    assert abs(u.var() - 1.0 / 12.0) <= 0.002
    # exactness: u and 1 - u are float32 numbers, and the clamp binds where it should
    h = np.array([0, 1 << 9, 0xffffffff, 167 << 9, 168 << 9, (1 << 23) - 1 << 9], dtype=np.uint32)
    got = mol_uniform(h)
    assert got[0] == U_LO and got[1] == U_LO and got[2] == U_HI      # 2^-24, 3 * 2^-24 and 1 - 2^-24 are clamped
    assert got[3] == np.float32(335 * 2.0 ** -24) and got[3] > U_LO  # the first numerator above 1e-5 * 2^24 = 167.8
    un = mol_uniform(mol_halves(1, 0, SLOT_MIX, 0, 0, np.arange(64), 2)).astype(np.float64)
    assert np.array_equal((1.0 - un).astype(np.float32).astype(np.float64), 1.0 - un)


def test_every_coordinate_of_the_address_changes_the_block():
    base = dict(seed=1, step=2, slot=SLOT_MIX, seq=4, draw=5, pixel=6, block=1)

    def block(a):
        return mol_halves(a["seed"], a["step"], a["slot"], a["seq"], a["draw"], [a["pixel"]], a["block"] + 1)[0, -8:]
    ref = block(base)
    for name in base:
        other = dict(base)
        other[name] = SLOT_COLOUR if name == "slot" else base[name] + 1
        assert not np.array_equal(ref, block(other)), name
    # a value does not depend on rows, B or which rows share the call
    a, ax = mol_keyed_uniforms_ref(6, 2, 9, 10, 3, 7, 1)
    b, bx = mol_keyed_uniforms_ref(2, 2, 9, 10, 3, 7, 1, first_draw=1)
    c, cx = mol_keyed_uniforms_ref(1, 1, 9, 10, 3, 7, 1, first_seq=1, first_draw=2)
    assert np.array_equal(a[2:4], b) and np.array_equal(ax[2:4], bx)
    assert np.array_equal(a[5:6], c) and np.array_equal(ax[5:6], cx)
    assert a.shape == (6, 9, 10) and ax.shape == (6, 9, 3)


def test_no_address_is_shared_with_keyed_normal():
    """an address is (key, counter).  keyed_normal: key (seed, (t << 32) | j) with j in 0..7, counter (q, 0, seq, draw);
    the sampler: key (seed, (t << 32) | 16 or 17), counter (j, p, seq, draw).  The slot words differ, so the keys do for
    every seed and step; spelled out over a grid of small addresses, where the counters do coincide"""
    assert (SLOT_MIX, SLOT_COLOUR) == (16, 17)
    assert min(SLOT_MIX, SLOT_COLOUR) >= ops.KEYED_NORMAL_MAX_SLOTS and max(SLOT_MIX, SLOT_COLOUR) < 1 << 32
    normal, mol = set(), set()
    for seed in (0, 1):
        for step in (0, 1, 16, 17):
            for seq in (0, 1):
                for draw in (0, 1):
                    for q in range(20):
                        normal.update((mol_key(seed, step, j), (q, 0, seq, draw)) for j in range(8))
                    for j in range(3):
                        mol.update((mol_key(seed, step, s), (j, p, seq, draw)) for s in (SLOT_MIX, SLOT_COLOUR)
                                   for p in range(4))
    assert len(mol) == 2 * 4 * 2 * 2 * 3 * 2 * 4 and not (normal & mol)
    assert {c for _, c in normal} & {c for _, c in mol}     # the counters alone would collide


# ---------------------------------------------------------------------------------------------- argument refusals
def test_ops_refuse_bad_arguments():
    l = torch.zeros(6, 30, 4, 4)
    with pytest.raises(RuntimeError, match="must be"):
        ops.mol_sample_keyed(torch.zeros(6, 30, 4), 2, 0, 0)
    with pytest.raises(RuntimeError, match="fit both"):
        ops.mol_sample_keyed(l, 2, 0, 0)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.mol_sample_keyed(torch.zeros(6, 31, 4, 4), 2, 0, 0, channels=3)
    with pytest.raises(ValueError, match="multiple of B"):
        ops.mol_sample_keyed(l, 4, 0, 0, channels=3)
    with pytest.raises(ValueError, match="multiple of B"):
        ops.mol_sample_keyed(l, 0, 0, 0, channels=3)
    with pytest.raises(ValueError, match="seed"):
        ops.mol_sample_keyed(l, 2, -1, 0, channels=3)
    with pytest.raises(ValueError, match="step"):
        ops.mol_sample_keyed(l, 2, 0, 1 << 31, channels=3)
    with pytest.raises(ValueError, match="first_draw"):
        ops.mol_sample_keyed(l, 2, 0, 0, first_draw=-1, channels=3)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.mol_sample_keyed(l, 2, 0, 0, channels=3)
    with pytest.raises(ValueError, match="rows, H, W"):
        ops.mol_keyed_uniforms((6, 4), 2, 10, 3, 0, 0)
    with pytest.raises(ValueError, match="channels"):
        ops.mol_keyed_uniforms((6, 4, 4), 2, 10, 2, 0, 0)
    with pytest.raises(ValueError, match="M >= 1"):
        ops.mol_keyed_uniforms((6, 4, 4), 2, 0, 3, 0, 0)
    with pytest.raises(ValueError, match="multiple of B"):
        ops.mol_keyed_uniforms((6, 4, 4), 5, 10, 3, 0, 0)
    with pytest.raises(ValueError, match="first_seq"):
        ops.mol_keyed_uniforms((6, 4, 4), 2, 10, 3, 0, 0, first_seq=1 << 63)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mol_keyed_uniforms(l, 2, 10, 3, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mol_keyed_uniforms((6, 4, 4), 2, 10, 3, 0, 0, device="cpu")


# ---------------------------------------------------------------------------------------------- srnn.pt on the host
def test_solver_class_of_srnn():
    from evaluation_metrics import eval_settings as E
    from SRNN.trainer import Solver
    assert E.solver_class("srnn.pt") is Solver
    for name in ("svg.pt", "vrnn.pt", "other.pt"):
        with pytest.raises(ValueError, match="baseline models") as e:
            E.solver_class(name)
        assert name in str(e.value)


def test_temperature_study_refuses_srnn(tmp_path):
    from evaluation_metrics import eval_settings as E
    ev, model = _stub_evaluator(n_frames=6, start_predictions=2, resample=2, draws_per_pass=2)
    with pytest.raises(ValueError, match="srnn.pt"):
        ev.get_eval_values_temperatures([0.5, 1.0], "srnn.pt", loader=[])
    assert model.calls == []
    # the driver refuses before any file is read (tmp_path holds no experiment)
    settings = E.parse_args(["--folder_path", str(tmp_path) + "/", "--experiment_names", "x", "--model_path", "srnn.pt",
                             "--test_temperature"])
    with pytest.raises(ValueError, match="srnn.pt"):
        E.main(settings)
    with pytest.raises(ValueError, match="baseline models"):
        ev.get_eval_values("vrnn.pt", loader=[])


class _StubSRNN(object):
    """records the Evaluator's calls; SRNN's signatures: loss(x) -> (kl, nll), one argument only"""

    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def predict(self, image, n_predictions, n_conditions):
        self.calls.append(("predict", n_predictions, n_conditions))
        return image[:, :n_conditions].transpose(0, 1), torch.zeros((n_predictions, image.shape[0]) + tuple(image.shape[2:]))

    def loss(self, x):
        self.calls.append(("loss", tuple(x.shape)))
        return torch.tensor(1.0), torch.tensor(2.0)

    def elbo_importance_weighting(self, x, K):
        self.calls.append(("iw", tuple(x.shape), K))
        return torch.tensor(float(np.log(2.0)) * 16 * 16 * (x.shape[1] - 1) * 3.0)


def _stub_evaluator(**settings):
    from evaluation_metrics import Evaluator
    model = _StubSRNN()
    # trained on 4 frames: the RFN branch would cut the loss's input to them
    solver = SimpleNamespace(model=model, args=SimpleNamespace(n_frames=4, n_conditions=2, batch_size=2),
                             device=torch.device("cpu"),
                             preprocess=lambda x, reverse=False: (x * 255).byte() if reverse else x)
    ev = Evaluator(solver, settings=SimpleNamespace(**settings))
    ev.eval_seq = lambda gt, pred: tuple(torch.zeros(gt.shape[:2]) for _ in range(3))
    return ev, model


def test_evaluator_routes_srnn_through_the_other_branches():
    batches = [torch.zeros(2, 6, 1, 16, 16) for _ in range(2)]
    ev, model = _stub_evaluator(n_frames=6, start_predictions=2, resample=2)
    assert ev.n_trained == 4 and ev.iw_samples == 20
    out = ev.get_eval_values("srnn.pt", loader=batches)
    # loss(image): one argument, the WHOLE sequence of 6 frames, not the 4 trained ones
    assert model.calls == [("predict", 4, 2), ("loss", (2, 6, 1, 16, 16))] * 4
    assert len(out) == 10 and tuple(out[0].shape) == (4, 4) and out[3] is None
    # compute_loss with the dims and t of `image`: (kl + nll) / (ln 2 * 256 * 5), kl / 5, nll / 5
    assert out[4].tolist() == pytest.approx([3.0 / (np.log(2.0) * 256 * 5)] * 2, rel=1e-6)
    assert out[5].tolist() == pytest.approx([0.2] * 2) and out[6].tolist() == pytest.approx([0.4] * 2)
    # get_loss: the importance-weighted bound on the trained frames with settings.iw_samples
    ev, model = _stub_evaluator(n_frames=6, start_predictions=2, resample=2, iw_samples=7)
    mean, std = ev.get_loss("srnn.pt", loss_resamples=1, loader=batches)
    assert model.calls == [("iw", (2, 4, 1, 16, 16), 7)] * 2
    assert float(mean) == pytest.approx(3.0, rel=1e-6) and std == -1
    ev, model = _stub_evaluator(n_frames=6, start_predictions=2)
    mean, std = ev.get_loss("srnn.pt", loss_resamples=2, loader=batches)
    assert [c[2] for c in model.calls] == [20] * 4 and float(std) == pytest.approx(0.0, abs=1e-6)
    with pytest.raises(ValueError, match="baseline models"):
        ev.get_loss("svg.pt", loader=batches)
