"""GPU: a flow level that is handed the packs of ListGlow._packed_weights packs nothing itself.

The level node reads the StepPacks fields its route names (rfn_hip.ops.coupling_route) and packs a missing one on the
spot -- silently, inside the captured training step.  Here one GlowLevelFn forward + backward (K = 2) runs under
rfn_hip.lib.PROFILE for each route, and no recorded launch may be a weight pack.  (What the runs compute is compared
with fp64 by tests/test_hip_modules.py.)"""
from argparse import Namespace

import pytest
import torch

from tests.golden_args import GLOW_DEFAULTS
from tests.test_coupling_route_host import ACT, EXTRA, SHAPES

pytestmark = pytest.mark.gpu

PACK_LAUNCHES = ("rfn_pack_", "rfn_smallmap_pack_", "rfn_coupling_po_pack")

# case: (row of SHAPES, knob set to "0", what the knob changes of the row's 'mixed' / 'bf16x3' route)
# (no level of a ListGlow that the fused forward kernel takes lacks a fused backward instance -- C would have to be 10 --
# so the fused forward meets the "dgrad_act" chain through the backward kernel's knob)
CASES = {
    "fused": ("po_16x16", None, {}, {}),
    "fused_fwd_dgrad_act": ("po_16x16", "RFN_COUPLING_PO_BWD",
                            dict(masks=False, bwd_chain="dgrad_act", packs=("po_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad")), {}),
    "dense": ("dense_2x2", None, {}, {}),
    "dgrad_small": ("small_16x16", None, {}, {}),
    "generic": ("small_16x16", "RFN_DGRAD_SMALL", dict(dgrad1="conv"), dict(dgrad1="conv")),
}
# what each case is there for, in 'mixed': (fwd, conv1, bwd_chain, dgrad1)
INTENDED = {"fused": ("po", "conv", "po", "small"), "fused_fwd_dgrad_act": ("po", "conv", "dgrad_act", "small"),
            "dense": ("convs", "dense", "dgrad_act", "dense"), "dgrad_small": ("convs", "conv", "dgrad_act", "small"),
            "generic": ("convs", "conv", "dgrad_act", "conv")}


@pytest.mark.parametrize("prec", [None, "mixed", "bf16x3"])
@pytest.mark.parametrize("case", list(CASES))
def test_level_node_with_planned_packs_packs_nothing(monkeypatch, case, prec):
    from Flow import ListGlow
    from rfn_hip import lib as L
    from rfn_hip import ops as K
    row, knob, mixed, b3 = CASES[case]
    if prec is not None:
        monkeypatch.setattr(K, "CONV_PRECISION", prec)
    for name in ("RFN_COUPLING_PO", "RFN_COUPLING_PO_BWD", "RFN_SMALLMAP_GLOW", "RFN_DGRAD_SMALL"):
        monkeypatch.delenv(name, raising=False)
    if knob:
        monkeypatch.setenv(knob, "0")
    N, C, Cc, Hd, H, W, k1, k2, k3 = SHAPES[row]
    if K.CONV_PRECISION in ("mixed", "bf16x3"):   # (the default arithmetic is the environment's)
        want = EXTRA[K.CONV_PRECISION, row][0]._replace(**(mixed if K.CONV_PRECISION == "mixed" else b3))
        assert K.coupling_route(N, C, Cc, Hd, H, W, k1, k2, k3, ACT, True) == want
        if K.CONV_PRECISION == "mixed":
            assert (want.fwd, want.conv1, want.bwd_chain, want.dgrad1) == INTENDED[case]

    torch.manual_seed(3)
    args = Namespace(**dict(GLOW_DEFAULTS, learn_prior=False, L=1, K=2, n_units_affine=Hd))
    flow = ListGlow([N, C // 4, 2 * H, 2 * W], [[N, Cc, H, W]], (N, 4, H, W), args).cuda().train()
    x = (torch.rand(N, C // 4, 2 * H, 2 * W) - 0.5).cuda()
    cond = [torch.randn(N, Cc, H, W).cuda().requires_grad_(True)]
    flow.log_prob(x, cond, None, 0)   # data dependent init
    (_, steps, _), = flow._level_steps()
    z = K.squeeze2d_raw(x).requires_grad_(True)
    Wst, _ = flow._batched_invconv(steps, H * W)
    flat = [p for s in steps for p in (s.norm.bias, s.norm.logs, *s.affine.nn_params())]
    packs = flow._packed_weights(x.shape, cond)
    L.PROFILE = []
    try:
        out, dl = K.GlowLevelFn.apply(z, cond[0], Wst, ACT, K.CLAMP["realnvp"], [packs[s] for s in steps], *flat)
        (out.sum() + dl.sum()).backward()
        torch.cuda.synchronize()
    finally:
        rec, L.PROFILE = L.PROFILE, None
    names = [r[0] for r in rec]
    assert len(names) > 10 and any(n.startswith("rfn_glow_shell_bwd") for n in names)
    assert [n for n in names if n.startswith(PACK_LAUNCHES)] == []
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in flat if p is not None)
