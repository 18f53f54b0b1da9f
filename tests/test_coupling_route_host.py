"""CPU-only: the kernel route of a Glow step's coupling net (rfn_hip.ops.coupling_route) and the weight packs the flow
keeps for it (Flow.glow.plan_packs), pinned.

The expected routes are literals.  They were recorded before coupling_route existed, by evaluating the predicates
(coupling_po_ok, coupling_po_bwd_ok, smallmap_conv_ok, dgrad_small_ok, zeros_conv_uses_taps, fwd_prec, bwd_b3) the way
the four places that used to decide separately combined them: the forward chain, the backward chain, the reverse step and
the flow's pack list.  The library's *_supported queries answer without a device."""
import pytest

from rfn_hip.ops import CouplingRoute as R

PRECISIONS = ("mixed", "bf16x3", "f32")
FRAMES = (76, 608)   # local batches of 4 and 32 sequences of 20 frames
# the canonical flow (64x64x1 input, K=10, L=5, Hd=256): (C, condition channels, map side) per level
LEVELS = [(4, 16, 32), (8, 32, 16), (16, 64, 8), (32, 128, 4), (64, 256, 2)]
ACT = 1   # relu, the canonical flow's

# rows that make each branch flip: (N, C, Cc, Hd, H, W, k1, k2, k3)
SHAPES = {
    "k2_3": (76, 8, 32, 256, 16, 16, 3, 3, 3),          # conv2 not 1x1: no fused kernel either way
    "k2_1": (76, 8, 32, 256, 16, 16, 3, 1, 3),          # ... its 1x1 twin
    "hd64": (76, 8, 32, 64, 16, 16, 3, 1, 3),           # Hd != 256: unfused, Hd % 64 == 0: dgrad_act
    "hd96": (76, 8, 32, 96, 16, 16, 3, 1, 3),           # Hd % 64 != 0: epilogue chain, nothing deferred
    "map3x5": (76, 8, 32, 256, 3, 5, 3, 1, 3),          # H * W % 4 != 0: nothing deferred
    "wide_few_px": (254, 16, 64, 256, 8, 8, 3, 1, 3),   # C/2 + Cc > 40 below 128 * 128 pixels: the any_size policy
    "wide_many_px": (256, 16, 64, 256, 8, 8, 3, 1, 3),  # ... and at 128 * 128 pixels
    "dense_2x2": (2, 16, 8, 64, 2, 2, 3, 1, 3),
    "po_16x16": (2, 8, 32, 256, 16, 16, 3, 1, 3),
    "small_16x16": (2, 8, 4, 64, 16, 16, 3, 1, 3),
    "k1_1": (76, 8, 32, 256, 16, 16, 1, 1, 3),          # conv1 not 3x3
}

# fwd, fwd_prec, conv1, conv3, masks, bwd_chain, dgrad1, defer_wgrad, packs
R00 = R("po", "bf16x6", "conv", "taps", True, "po", "small", True,
        ("po_fwd", "po_bwd", "w1_dgrad"))
R01 = R("po", "bf16x6", "conv", "taps", False, None, None, False,
        ("po_fwd",))
R02 = R("convs", "bf16x6", "conv", "conv", False, "po", "small", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "po_bwd", "w1_dgrad"))
R03 = R("convs", "bf16x6", "conv", "conv", False, None, None, False,
        ("w1_fwd", "w2_fwd", "w3_fwd"))
R04 = R("po", "bf16x6", "conv", "conv", True, "po", "small", True,
        ("po_fwd", "po_bwd", "w1_dgrad"))
R05 = R("po", "bf16x6", "conv", "conv", False, None, None, False,
        ("po_fwd",))
R06 = R("convs", "bf16x6", "conv", "conv", False, "dgrad_act", "dense", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dense_dgrad"))
R07 = R("convs", "bf16x6", "conv", "conv", False, "dgrad_act", "conv", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R08 = R("convs", "bf16x3", "dense", "dense", False, "dgrad_act", "dense", True,
        ("w1_dense_fwd", "w2_fwd", "w3_dense_fwd", "w3_dgrad", "w2_dgrad", "w1_dense_dgrad"))
R09 = R("convs", "bf16x3", "dense", "dense", False, None, None, False,
        ("w1_dense_fwd", "w2_fwd", "w3_dense_fwd"))
R10 = R("convs", "bf16x3", "conv", "conv", False, None, None, False,
        ("w1_fwd", "w2_fwd", "w3_fwd"))
R11 = R("convs", "bf16x3", "conv", "taps", False, "dgrad_act", "small", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R12 = R("convs", "bf16x3", "conv", "taps", False, None, None, False,
        ("w1_fwd", "w2_fwd", "w3_fwd"))
R13 = R("convs", "bf16x3", "conv", "conv", False, "dgrad_act", "small", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R14 = R("convs", "bf16x3", "conv", "conv", False, "dgrad_act", "conv", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R15 = R("convs", "f32", "conv", "taps", False, "epilogue", "conv", False,
        ("w3_dgrad", "w2_dgrad", "w1_dgrad"))
R16 = R("convs", "f32", "conv", "taps", False, None, None, False,
        ())
R17 = R("convs", "f32", "conv", "taps", False, None, None, False,
        ("w1_fwd", "w2_fwd", "w3_fwd"))
R18 = R("convs", "f32", "conv", "conv", False, "epilogue", "conv", False,
        ("w3_dgrad", "w2_dgrad", "w1_dgrad"))
R19 = R("convs", "f32", "conv", "conv", False, None, None, False,
        ())
R20 = R("convs", "f32", "conv", "conv", False, None, None, False,
        ("w1_fwd", "w2_fwd", "w3_fwd"))
R21 = R("convs", "bf16x6", "conv", "taps", False, "dgrad_act", "small", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R22 = R("convs", "bf16x6", "conv", "taps", False, None, None, False,
        ("w1_fwd", "w2_fwd", "w3_fwd"))
R23 = R("convs", "bf16x6", "conv", "taps", False, "epilogue", "small", False,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R24 = R("convs", "bf16x6", "conv", "taps", False, "dgrad_act", "dense", False,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dense_dgrad"))
R25 = R("convs", "bf16x6", "conv", "taps", False, "dgrad_act", "conv", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R26 = R("convs", "bf16x3", "conv", "taps", False, "epilogue", "small", False,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))
R27 = R("convs", "bf16x3", "conv", "taps", False, "dgrad_act", "dense", False,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dense_dgrad"))
R28 = R("convs", "bf16x3", "conv", "taps", False, "dgrad_act", "conv", True,
        ("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))

CANONICAL = {   # (CONV_PRECISION, level, frames): routes with grad, without, in reverse
    ("mixed", 0, 76): (R00, R01, R01),
    ("mixed", 0, 608): (R00, R01, R01),
    ("mixed", 1, 76): (R00, R01, R01),
    ("mixed", 1, 608): (R00, R01, R01),
    ("mixed", 2, 76): (R02, R03, R03),
    ("mixed", 2, 608): (R04, R05, R05),
    ("mixed", 3, 76): (R06, R03, R03),
    ("mixed", 3, 608): (R07, R03, R03),
    ("mixed", 4, 76): (R08, R09, R10),
    ("mixed", 4, 608): (R08, R09, R10),
    ("bf16x3", 0, 76): (R11, R12, R12),
    ("bf16x3", 0, 608): (R11, R12, R12),
    ("bf16x3", 1, 76): (R11, R12, R12),
    ("bf16x3", 1, 608): (R11, R12, R12),
    ("bf16x3", 2, 76): (R13, R10, R10),
    ("bf16x3", 2, 608): (R13, R10, R10),
    ("bf16x3", 3, 76): (R08, R09, R10),
    ("bf16x3", 3, 608): (R14, R10, R10),
    ("bf16x3", 4, 76): (R08, R09, R10),
    ("bf16x3", 4, 608): (R08, R09, R10),
    ("f32", 0, 76): (R15, R16, R17),
    ("f32", 0, 608): (R15, R16, R17),
    ("f32", 1, 76): (R15, R16, R17),
    ("f32", 1, 608): (R15, R16, R17),
    ("f32", 2, 76): (R18, R19, R20),
    ("f32", 2, 608): (R18, R19, R20),
    ("f32", 3, 76): (R18, R19, R20),
    ("f32", 3, 608): (R18, R19, R20),
    ("f32", 4, 76): (R18, R19, R20),
    ("f32", 4, 608): (R18, R19, R20),
}

EXTRA = {   # (CONV_PRECISION, row of SHAPES): routes with grad, in reverse
    ("mixed", "k2_3"): (R21, R22),
    ("mixed", "k2_1"): (R00, R01),
    ("mixed", "hd64"): (R21, R22),
    ("mixed", "hd96"): (R23, R22),
    ("mixed", "map3x5"): (R24, R22),
    ("mixed", "wide_few_px"): (R02, R03),
    ("mixed", "wide_many_px"): (R04, R05),
    ("mixed", "dense_2x2"): (R08, R10),
    ("mixed", "po_16x16"): (R00, R01),
    ("mixed", "small_16x16"): (R21, R22),
    ("mixed", "k1_1"): (R25, R22),
    ("bf16x3", "k2_3"): (R11, R12),
    ("bf16x3", "k2_1"): (R11, R12),
    ("bf16x3", "hd64"): (R11, R12),
    ("bf16x3", "hd96"): (R26, R12),
    ("bf16x3", "map3x5"): (R27, R12),
    ("bf16x3", "wide_few_px"): (R13, R10),
    ("bf16x3", "wide_many_px"): (R13, R10),
    ("bf16x3", "dense_2x2"): (R08, R10),
    ("bf16x3", "po_16x16"): (R11, R12),
    ("bf16x3", "small_16x16"): (R11, R12),
    ("bf16x3", "k1_1"): (R28, R12),
    ("f32", "k2_3"): (R15, R17),
    ("f32", "k2_1"): (R15, R17),
    ("f32", "hd64"): (R15, R17),
    ("f32", "hd96"): (R15, R17),
    ("f32", "map3x5"): (R15, R17),
    ("f32", "wide_few_px"): (R18, R20),
    ("f32", "wide_many_px"): (R18, R20),
    ("f32", "dense_2x2"): (R18, R20),
    ("f32", "po_16x16"): (R15, R17),
    ("f32", "small_16x16"): (R15, R17),
    ("f32", "k1_1"): (R15, R17),
}

# route.packs that the pack plan does NOT build (every other row: none), grad rows:
#   'f32' has no pack plan at all (PackPlan packs split precision): every node packs its own data-gradient weights;
#   below 128 * 128 pixels the wide level is refused the fused forward kernel (policy), so its nets get no streams, while
#   the fused backward kernel would take the shape: the backward falls back to "dgrad_act" (whose packs the plan builds)
F32_MISSING = ("w3_dgrad", "w2_dgrad", "w1_dgrad")
MISSING = {("mixed", 2, 76): ("po_bwd",), ("mixed", "wide_few_px"): ("po_bwd",)}

# packs the plan builds and no route reads, canonical flow, grad rows (without grad: also the three w*_dgrad packs)
UNREAD = {
    ("mixed", 0): ("w2_dgrad", "w3_dgrad"), ("mixed", 1): ("w2_dgrad", "w3_dgrad"),
    ("mixed", 2, 76): ("w2_dgrad", "w3_dgrad"),   # (read after all: the "dgrad_act" fallback of MISSING)
    ("mixed", 2, 608): ("w2_dgrad", "w3_dgrad"),
    ("mixed", 3, 76): ("w1_dgrad",), ("mixed", 3, 608): (),
    ("mixed", 4): ("w1_fwd", "w1_dgrad", "w3_fwd"),
    ("bf16x3", 0): (), ("bf16x3", 1): (), ("bf16x3", 2): (),
    ("bf16x3", 3, 76): ("w1_fwd", "w1_dgrad", "w3_fwd"), ("bf16x3", 3, 608): (),
    ("bf16x3", 4): ("w1_fwd", "w1_dgrad", "w3_fwd"),
}


@pytest.fixture(scope="module")
def K():
    from rfn_hip import ops
    return ops


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for knob in ("RFN_COUPLING_PO", "RFN_COUPLING_PO_BWD", "RFN_SMALLMAP_GLOW", "RFN_DGRAD_SMALL"):
        monkeypatch.delenv(knob, raising=False)


@pytest.fixture(scope="module")
def flow_levels():
    """plan_packs' `levels` of the canonical model, read off its modules"""
    import main_rfn
    from RFN import RFN
    from rfn_hip import ops
    model = RFN(main_rfn.build_parser().parse_args(main_rfn.canonical_smmnist_argv(1, 2)))
    levels = []
    for _, steps, split in model.flow._level_steps():
        w = [[s.affine.net[i].conv.weight for i in (0, 2, 4)] for s in steps]
        Cc = int(w[0][0].shape[1]) - int(w[0][2].shape[0]) // 2
        levels.append((Cc, split is not None, [(int(w1.shape[0]), int(w1.shape[2]), int(w2.shape[2]), int(w3.shape[2]),
                                                ops.ACT[s.affine.non_lin], s.flow_norm != "batchnorm")
                                               for s, (w1, w2, w3) in zip(steps, w)]))
    return levels


def test_the_table_is_the_canonical_model(flow_levels):
    assert [(Cc, len(steps)) for Cc, _, steps in flow_levels] == [(Cc, 10) for _, Cc, _ in LEVELS]
    assert all(step == (256, 3, 1, 3, ACT, True) for _, _, steps in flow_levels for step in steps)
    assert [split for _, split, _ in flow_levels] == [True] * 4 + [False]


@pytest.mark.parametrize("prec", PRECISIONS)
def test_canonical_routes(K, monkeypatch, prec):
    monkeypatch.setattr(K, "CONV_PRECISION", prec)
    for l, (C, Cc, S) in enumerate(LEVELS):
        for N in FRAMES:
            got = tuple(K.coupling_route(N, C, Cc, 256, S, S, 3, 1, 3, ACT, grad, reverse=rev)
                        for grad, rev in ((True, False), (False, False), (False, True)))
            assert got == CANONICAL[prec, l, N], (prec, l, N)
            # (a reverse step has no backward whatever `grad` says)
            assert K.coupling_route(N, C, Cc, 256, S, S, 3, 1, 3, ACT, True, reverse=True) == got[2]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("row", list(SHAPES))
def test_branch_rows(K, monkeypatch, prec, row):
    monkeypatch.setattr(K, "CONV_PRECISION", prec)
    got = (K.coupling_route(*SHAPES[row], ACT, True), K.coupling_route(*SHAPES[row], ACT, False, reverse=True))
    assert got == EXTRA[prec, row]


def test_no_activation_means_no_masks(K, monkeypatch):
    monkeypatch.setattr(K, "CONV_PRECISION", "mixed")
    C, Cc, S = LEVELS[0]
    assert K.coupling_route(76, C, Cc, 256, S, S, 3, 1, 3, 0, True) == CANONICAL["mixed", 0, 76][0]._replace(masks=False)


def _plan_fields(conv, nets, dense, step, C, grad):
    fields = {f for s, f, _ in conv + dense if s == step}
    if step in nets:   # POPackPlan: a backward stream for at most 16 channels, refreshed under grad
        fields |= {"po_fwd"} | ({"po_bwd"} if C <= 16 and grad else set())
    return fields


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("grad", [True, False])
def test_the_plan_builds_what_the_canonical_routes_read(K, monkeypatch, flow_levels, prec, grad):
    from Flow.glow import plan_packs
    monkeypatch.setattr(K, "CONV_PRECISION", prec)
    for N in FRAMES:
        conv, nets, dense = plan_packs(N, 1, 64, 64, flow_levels, grad)
        if prec == "f32":   # (ListGlow._packed_weights does not get this far: no split precision, no plan)
            conv, nets, dense = [], [], []
        for l, (C, Cc, S) in enumerate(LEVELS):
            route = CANONICAL[prec, l, N][0 if grad else 1]
            for k in (0, 9):
                have = _plan_fields(conv, nets, dense, (l, k), C, grad)
                missing = tuple(f for f in route.packs if f not in have)
                want = (F32_MISSING if prec == "f32" else MISSING.get((prec, l, N), ())) if grad else ()
                assert missing == want, (prec, l, N, k)
                if prec != "f32":
                    unread = tuple(f for f in K.StepPacks._fields if f in have and f not in route.packs)
                    want = UNREAD.get((prec, l), UNREAD.get((prec, l, N)))
                    if not grad:
                        want = tuple(f for f in K.StepPacks._fields if f in want or f in F32_MISSING)
                    assert unread == want, (prec, l, N, k)


@pytest.mark.parametrize("prec", ["mixed", "bf16x3"])
@pytest.mark.parametrize("row", list(SHAPES))
def test_the_plan_builds_what_the_branch_rows_read(K, monkeypatch, prec, row):
    from Flow.glow import plan_packs
    monkeypatch.setattr(K, "CONV_PRECISION", prec)
    N, C, Cc, Hd, H, W, k1, k2, k3 = SHAPES[row]
    conv, nets, dense = plan_packs(N, C // 4, 2 * H, 2 * W, [(Cc, False, [(Hd, k1, k2, k3, ACT, True)])], True)
    have = _plan_fields(conv, nets, dense, (0, 0), C, True)
    assert tuple(f for f in EXTRA[prec, row][0].packs if f not in have) == MISSING.get((prec, row), ())


def test_plan_order_and_modes(K, monkeypatch):
    """launch order: per step w1, w2, w3, forward pack (where the forward is unfused and split precision) before
    data-gradient pack; forward packs in three planes (+4) where bf16x6 is the forward arithmetic, conv3 tap-expanded (2)
    for at most 8 outputs; a step that is no rfn_hip.ops node (BatchNorm flow) gets no fused streams"""
    from Flow.glow import plan_packs
    monkeypatch.setattr(K, "CONV_PRECISION", "mixed")
    step = (256, 3, 1, 3, ACT, True)
    conv, nets, dense = plan_packs(608, 1, 64, 64, [(16, True, [step, step[:5] + (False,)]), (32, False, [step])], True)
    dg = lambda s: [(s, "w%d_dgrad" % i, 1) for i in (1, 2, 3)]
    mixed01 = [((0, 1), "w1_fwd", 4), ((0, 1), "w1_dgrad", 1), ((0, 1), "w2_fwd", 4), ((0, 1), "w2_dgrad", 1),
               ((0, 1), "w3_fwd", 6), ((0, 1), "w3_dgrad", 1)]
    assert conv == dg((0, 0)) + mixed01 + dg((1, 0)) and nets == [(0, 0), (1, 0)] and dense == []
    monkeypatch.setattr(K, "CONV_PRECISION", "bf16x3")
    conv, nets, dense = plan_packs(76, 16, 8, 8, [(128, True, [step]), (256, False, [step])], True)
    assert nets == [] and [c[1:] for c in conv[:6]] == [("w1_fwd", 0), ("w1_dgrad", 1), ("w2_fwd", 0), ("w2_dgrad", 1),
                                                       ("w3_fwd", 0), ("w3_dgrad", 1)]
    assert dense == [((l, 0), f, (S, S, t)) for l, S in ((0, 4), (1, 2))
                     for f, t in (("w1_dense_fwd", False), ("w3_dense_fwd", False), ("w1_dense_dgrad", True))]
    assert plan_packs(76, 16, 8, 8, [(128, True, [step]), (256, False, [step])], False)[2] == [d for d in dense if not d[2][2]]


KNOBS = [   # knob, row, the fields it governs (packs follows them)
    ("RFN_COUPLING_PO", ("mixed", 0, 76), dict(fwd="convs", masks=False, packs=("w1_fwd", "w2_fwd", "w3_fwd", "po_bwd", "w1_dgrad"))),
    ("RFN_COUPLING_PO_BWD", ("mixed", 0, 76), dict(masks=False, bwd_chain="dgrad_act",
                                                   packs=("po_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))),
    ("RFN_SMALLMAP_GLOW", ("bf16x3", 4, 76), dict(conv1="conv", conv3="conv", dgrad1="conv",
                                                  packs=("w1_fwd", "w2_fwd", "w3_fwd", "w3_dgrad", "w2_dgrad", "w1_dgrad"))),
    ("RFN_DGRAD_SMALL", ("bf16x3", 1, 76), dict(dgrad1="conv")),
]


@pytest.mark.parametrize("knob,row,changes", KNOBS, ids=[k[0] for k in KNOBS])
def test_a_knob_changes_the_fields_it_governs(K, monkeypatch, knob, row, changes):
    """read on every call (no memoised route), and nothing else moves"""
    prec, l, N = row
    C, Cc, S = LEVELS[l]
    monkeypatch.setattr(K, "CONV_PRECISION", prec)
    assert K.coupling_route(N, C, Cc, 256, S, S, 3, 1, 3, ACT, True) == CANONICAL[row][0]
    monkeypatch.setenv(knob, "0")
    assert K.coupling_route(N, C, Cc, 256, S, S, 3, 1, 3, ACT, True) == CANONICAL[row][0]._replace(**changes)
    monkeypatch.delenv(knob)
    assert K.coupling_route(N, C, Cc, 256, S, S, 3, 1, 3, ACT, True) == CANONICAL[row][0]
