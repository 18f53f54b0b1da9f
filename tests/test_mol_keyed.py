"""rfn_hip.ops.mol_sample_keyed / mol_keyed_uniforms (csrc/mol.hip) on the GPU: the emitted
uniforms against the numpy restatement of tests/test_mol_keyed_host.py (exactly), the keyed sampler against mol_sample on
the emitted uniforms (bit for bit: both run one device function), independence of how the draws are split into calls
(bit for bit), and the float64 restatement tests/mol_ref.py under the bound and exclusion rule of
tests/test_mol.py::test_sample_against_float64 (error <= 1e-5 where the two best Gumbel scores differ by >= 1e-4, at most
1 % of the pixels left out).

Shapes: the logits of tests/golden/mol.*.pt, cycled to rows = 6 with B = 2 (three draws of two sequences) -- RGB M = 10
on 5x13 (a partial workgroup), gray M = 10 on 24x24 (three workgroups per frame, the last one partial; M = 10 uses 2 of
the 8 halves of its second Philox block), gray M = 1 on 4x4.

Measured on an MI355X, error against float64 / pixels left out:
  rgb_m10 1.4e-07 / 0.0000   gray_m10 2.1e-07 / 0.0000   gray_m1 5.8e-08 / 0.0000
"""
import numpy as np
import pytest
import torch

from tests import mol_ref as R
from tests.test_mol_host import load_case
from tests.test_mol_keyed_host import mol_keyed_uniforms_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("rgb_m10", "gray_m10", "gray_m1")
ROWS, B = 6, 2
SEED, STEP, FIRST_SEQ, FIRST_DRAW = 20261020, 7, 40, 3


@pytest.fixture(scope="module")
def ops():
    from rfn_hip import lib, ops as K
    assert torch.cuda.is_available(), "GPU tests need a device"
    lib.load()
    return K


@pytest.fixture(scope="module")
def cases(ops):
    """per case: the six rows of logits, the emitted uniforms and the keyed sample; computed once, left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            c = load_case(name)
            N, C, H, W = c["x"].shape
            l = c["l"][[i % N for i in range(ROWS)]].contiguous()
            ld = l.to(DEV)
            u_mix, u_x = ops.mol_keyed_uniforms(ld, B, c["M"], C, SEED, STEP, FIRST_SEQ, FIRST_DRAW)
            out = ops.mol_sample_keyed(ld, B, SEED, STEP, FIRST_SEQ, FIRST_DRAW, channels=C)
            cache[name] = dict(l=l, ld=ld, M=c["M"], C=C, H=H, W=W, u_mix=u_mix, u_x=u_x, out=out)
        return cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_uniforms_equal_the_host_restatement(ops, cases, name):
    c = cases(name)
    H, W, M, C = c["H"], c["W"], c["M"], c["C"]
    assert c["u_mix"].shape == (ROWS, H, W, M) and c["u_x"].shape == (ROWS, H, W, C)
    ref_mix, ref_x = mol_keyed_uniforms_ref(ROWS, B, H * W, M, C, SEED, STEP, FIRST_SEQ, FIRST_DRAW)
    assert np.array_equal(c["u_mix"].cpu().numpy().reshape(ROWS, H * W, M), ref_mix)
    assert np.array_equal(c["u_x"].cpu().numpy().reshape(ROWS, H * W, C), ref_x)
    # from a shape instead of the logits
    a, b = ops.mol_keyed_uniforms((ROWS, H, W), B, M, C, SEED, STEP, FIRST_SEQ, FIRST_DRAW, device=DEV)
    assert torch.equal(a, c["u_mix"]) and torch.equal(b, c["u_x"])


@pytest.mark.parametrize("name", CASES)
def test_keyed_sampler_is_mol_sample_on_the_emitted_uniforms(ops, cases, name):
    c = cases(name)
    assert c["out"].shape == (ROWS, c["C"], c["H"], c["W"])
    assert torch.equal(c["out"], ops.mol_sample(c["ld"], c["u_mix"], c["u_x"]))
    from Utils import DiscretizedMixtureLogits, DiscretizedMixtureLogits_1d
    lik = DiscretizedMixtureLogits if c["C"] == 3 else DiscretizedMixtureLogits_1d
    assert torch.equal(c["out"], lik(c["M"])(logits=c["ld"]).sample_keyed(B, SEED, STEP, FIRST_SEQ, FIRST_DRAW))


@pytest.mark.parametrize("name", CASES)
def test_rows_do_not_depend_on_the_call(ops, cases, name):
    c = cases(name)
    ld, C = c["ld"], c["C"]
    # rows 2..3 are draw FIRST_DRAW + 1 of both sequences
    part = ops.mol_sample_keyed(ld[2:4].contiguous(), B, SEED, STEP, FIRST_SEQ, FIRST_DRAW + 1, channels=C)
    assert torch.equal(part, c["out"][2:4])
    # row 5 alone: sequence FIRST_SEQ + 1, draw FIRST_DRAW + 2, as a batch of one
    one = ops.mol_sample_keyed(ld[5:6].contiguous(), 1, SEED, STEP, FIRST_SEQ + 1, FIRST_DRAW + 2, channels=C)
    assert torch.equal(one, c["out"][5:6])
    um, ux = ops.mol_keyed_uniforms(ld[5:6], 1, c["M"], C, SEED, STEP, FIRST_SEQ + 1, FIRST_DRAW + 2)
    assert torch.equal(um, c["u_mix"][5:6]) and torch.equal(ux, c["u_x"][5:6])
    # another step, another seed: other numbers
    assert not torch.equal(ops.mol_sample_keyed(ld, B, SEED, STEP + 1, FIRST_SEQ, FIRST_DRAW, channels=C), c["out"])
    assert not torch.equal(ops.mol_sample_keyed(ld, B, SEED + 1, STEP, FIRST_SEQ, FIRST_DRAW, channels=C), c["out"])


@pytest.mark.parametrize("name", CASES)
def test_keyed_sample_against_float64(ops, cases, name):
    c = cases(name)
    ref, gap = R.sample(c["l"].double(), c["u_mix"].cpu().double(), c["u_x"].cpu().double())
    out = c["out"].cpu()
    keep = (gap >= 1e-4).unsqueeze(1).expand_as(out)
    left_out = 1.0 - float(keep.float().mean())
    err = float((out.double() - ref)[keep].abs().max())
    print("%s: keyed sample error %.3e, pixels left out %.4f" % (name, err, left_out))
    assert left_out <= 0.01
    assert err <= 1e-5
    assert float(out.abs().max()) <= 1.0


def test_generator_untouched_and_capturable(ops, cases):
    c = cases("rgb_m10")
    ld, C = c["ld"], c["C"]
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    ops.mol_sample_keyed(ld, B, SEED, STEP, FIRST_SEQ, FIRST_DRAW, channels=C)
    ops.mol_keyed_uniforms(ld, B, c["M"], C, SEED, STEP, FIRST_SEQ, FIRST_DRAW)
    assert torch.equal(torch.cuda.get_rng_state(DEV), gpu_state) and torch.equal(torch.get_rng_state(), cpu_state)
    l_in = torch.zeros_like(ld)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.mol_sample_keyed(l_in, B, SEED, STEP, FIRST_SEQ, FIRST_DRAW, channels=C)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.mol_sample_keyed(l_in, B, SEED, STEP, FIRST_SEQ, FIRST_DRAW, channels=C)
    l_in.copy_(ld)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, c["out"])
