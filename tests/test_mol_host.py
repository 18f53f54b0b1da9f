"""The float64 restatement of the mixture of discretized logistics (tests/mol_ref.py, written from DESIGN.md section 19)
against the reference's own float64 results stored in tests/golden/mol*.pt, and the host-side shape checks of
rfn_hip.ops.  No GPU, no kernel."""
import os

import pytest
import torch

from tests import mol_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INDEX = torch.load(os.path.join(GOLD, "mol.pt"), weights_only=True)
CASES = INDEX["cases"]


def load_case(name):
    return torch.load(os.path.join(GOLD, INDEX["parts"][name]), weights_only=True)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_cases_are_the_issues():
    shapes = {n: (tuple(load_case(n)["x"].shape), load_case(n)["M"]) for n in CASES}
    assert shapes == {"rgb_m10": ((3, 3, 5, 13), 10), "gray_m10": ((2, 1, 24, 24), 10), "gray_m1": ((1, 1, 4, 4), 1),
                      "rgb_m3": ((2, 3, 16, 16), 3)}


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_float64(name):
    c = load_case(name)
    x, l = c["x"].double(), c["l"].double().requires_grad_(True)
    nll = R.nll_pix(x, l)
    nll.sum().backward()
    assert nll.shape == c["nll_pix64"].shape
    assert rel(nll.detach(), c["nll_pix64"]) <= 1e-12
    assert rel(l.grad, c["dl64"]) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_restatement_sampler_matches_reference(name):
    """the reference's sampler only runs in float32 (it draws into FloatTensors): the restatement in float32 on the same
    uniforms, where the component choice is not a near tie"""
    c = load_case(name)
    out, gap = R.sample(c["l"], c["u_mix"], c["u_x"])
    keep = (gap >= 1e-4).unsqueeze(1).expand_as(out)
    assert float((~keep).float().mean()) <= 0.01
    assert out.shape == c["sample32"].shape
    assert float((out - c["sample32"])[keep].abs().max()) <= 1e-5
    assert float(out.abs().max()) <= 1.0


def test_recipe_covers_every_branch():
    """what the issue says of the input recipe: every branch and the log-scale clamp are exercised, few pixels sit on
    the discontinuity"""
    c = load_case("rgb_m3")   # (16 rows: the two forced rows are 1/16 of the items each)
    x, l = c["x"].double(), c["l"].double()
    _, delta = R.items(x, l)
    xe = x.unsqueeze(2).expand_as(delta)
    left, right = xe < -0.999, xe > 0.999
    low = ~left & ~right & (delta <= R.THRESH)
    assert 0.03 < float(left.float().mean()) < 0.12 and 0.03 < float(right.float().mean()) < 0.12
    assert 0.25 < float(low.float().mean()) < 0.55
    _, par = R.split(l, 3)
    assert 0.08 < float((par[:, :, 1] < R.MIN_LOG_SCALE).float().mean()) < 0.2
    for n in CASES:
        c = load_case(n)
        assert float(R.near_threshold(c["x"].double(), c["l"].double()).float().mean()) <= 0.02


def test_shape_errors_need_no_device():
    from rfn_hip import ops
    x = torch.zeros(2, 3, 4, 4)
    assert ops.mol_dims(x, torch.zeros(2, 30, 4, 4)) == (2, 3, 3, 16)
    assert ops.mol_dims(x[:, :1], torch.zeros(2, 30, 4, 4)) == (2, 1, 10, 16)
    for bad in (torch.zeros(2, 31, 4, 4), torch.zeros(2, 30, 4, 5), torch.zeros(1, 30, 4, 4), torch.zeros(2, 0, 4, 4)):
        with pytest.raises(RuntimeError):
            ops.mol_dims(x, bad)
    with pytest.raises(RuntimeError):
        ops.mol_dims(torch.zeros(2, 2, 4, 4), torch.zeros(2, 20, 4, 4))
    with pytest.raises(RuntimeError, match="device"):
        ops.mol_nll(x, torch.zeros(2, 30, 4, 4))          # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="no gradient flows into x"):
        ops.mol_nll(x.clone().requires_grad_(True), torch.zeros(2, 30, 4, 4))
    with pytest.raises(RuntimeError, match="channels"):
        ops.mol_sample(torch.zeros(2, 30, 4, 4))          # 30 = 10*3 = 3*10: ambiguous
