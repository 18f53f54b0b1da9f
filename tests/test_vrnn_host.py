"""Host side of the VRNN baseline against what tests/golden/make_golden_vrnn.py recorded from the reference: the parser of
main_vrnn.py, the state_dict of VRNN(args) (keys and shapes; constructed on the CPU, no kernel is called), the seeded
fill both sides share, the trainer's arithmetic (the package's VRNN Solver inherits SRNN's: the fixture holds the
REFERENCE's VRNN trainer), the checkpoint names, the refusals, and the argument checks of rfn_hip.ops.gauss_heads that
need no device."""
import os
from argparse import Namespace

import pytest
import torch

from tests.srnn_state import describe, fill_state

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX = torch.load(os.path.join(GOLD, "vrnn.pt"), weights_only=True)
CONFIGS = list(FX["configs"])

SOLVER_ARGS = dict(n_bits=8, n_epochs=1, learning_rate=1e-4, verbose=False, path="/tmp/", batch_size=2, patience_lr=1,
                   factor_lr=0.5, min_lr=1e-5, patience_es=1, beta_max=1.0, beta_min=1e-4, beta_steps=100,
                   choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=64,
                   preprocess_range="1.0", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                   n_conditions=2, use_validation_set=False)


def test_the_configurations_are_the_issues():
    assert CONFIGS == ["gray_mol", "rgb_mol", "bernoulli", "gray_mol_batchnorm"]
    c = FX["configs"]
    assert c["rgb_mol"]["args"]["x_dim"][1] == 3 and c["bernoulli"]["args"]["loss_type"] == "bernoulli"
    assert c["gray_mol_batchnorm"]["args"]["norm_type"] == "batchnorm"
    for name, c in FX["configs"].items():
        a = c["args"]
        assert (a["batch_size"], c["T"], a["x_dim"][2:], a["h_dim"], a["z_dim"], a["n_logistics"],
                a["preprocess_range"]) == (4, 4, [32, 32], 8, 4, 3, "1.0")
        assert a["norm_type"] == ("batchnorm" if name == "gray_mol_batchnorm" else "none")
        assert len(c["parts"]) == 2 and os.path.isfile(os.path.join(GOLD, "vrnn_iw.%s.pt" % name))


def test_parser_has_every_flag_of_the_reference():
    import main_vrnn
    p = main_vrnn.build_parser()
    own = {a.dest: a for a in p._actions}
    assert len(FX["flags"]) >= 30
    for f in FX["flags"]:
        flag = [a for a in p._actions if list(a.option_strings) == f["flags"]]
        assert len(flag) == 1, f["flags"]
        a = flag[0]
        assert a.dest == f["dest"] and a.default == f["default"] and a.nargs == f["nargs"] and a.const == f["const"], f
        assert (None if a.choices is None else list(a.choices)) == f["choices"], f
        assert (None if a.type is None else a.type.__name__) == f["type"], f
    ns = p.parse_args([])
    for f in FX["flags"]:
        assert getattr(ns, f["dest"]) == f["default"]
    assert (ns.num_workers, ns.factor_lr, ns.beta_min, ns.beta_steps, ns.h_dim) == (5, 0.7, 1e-6, 2000, 256)
    for extra in ("synthetic_data", "mnist_root", "data_root", "data_cache", "data_seed", "max_steps"):
        assert extra in own
    # exactly the reference's flags and the six additions: no smoothing or over-shooting flags
    assert {a.dest for a in p._actions} - {"help"} == {f["dest"] for f in FX["flags"]} | {
        "synthetic_data", "mnist_root", "data_root", "data_cache", "data_seed", "max_steps"}


@pytest.mark.parametrize("name", CONFIGS)
def test_state_dict_keys_and_shapes(name):
    from VRNN import VRNN
    c = FX["configs"][name]
    m = VRNN(Namespace(**c["args"]))
    keys, shapes, _ = describe(m.state_dict())
    assert keys == c["keys"]
    assert shapes == c["shapes"]
    # 60 without norm layers, 5 more per batch norm (12 of them); `variance` where there is no mixture
    assert len(keys) == {"gray_mol_batchnorm": 120, "bernoulli": 61}.get(name, 60)
    assert isinstance(m.enc_std[5], torch.nn.Softplus) and isinstance(m.prior_std[5], torch.nn.Softplus)
    state = fill_state(m.state_dict(), c["seed"])
    m.load_state_dict(state)                       # strict
    _, _, sums = describe(state)
    assert sums == pytest.approx(c["checksums"], rel=1e-12, abs=1e-12)


def test_exports_and_refusals():
    from SRNN.trainer import Solver as SRNNSolver
    from VRNN import VRNN
    from VRNN.trainer import Solver
    a = dict(FX["configs"]["gray_mol"]["args"])
    a.update(loss_type="gaussian", dequantize=False)
    with pytest.raises(ValueError, match="dequantize"):
        VRNN(Namespace(**a))
    with pytest.raises(NotImplementedError, match="VRNN.*multigpu"):
        Solver(Namespace(**dict(SOLVER_ARGS, multigpu=True)))
    s = Solver(Namespace(**SOLVER_ARGS))
    assert isinstance(s, SRNNSolver)
    assert s.checkpoint_names == ("vrnn.pt", "vrnn_best_model.pt") and s.scheduler_type == "plateau"
    assert not hasattr(s.args, "scheduler_type")
    assert isinstance(s.make_model.__self__, Solver) and Solver.make_model is not SRNNSolver.make_model
    with pytest.raises(NotImplementedError, match="VRNN"):
        s.capture_graph(None)
    with pytest.raises(NotImplementedError, match="VRNN"):
        s.plotter()
    m = VRNN(Namespace(**FX["configs"]["gray_mol"]["args"]))
    with pytest.raises(ValueError, match="K must be"):
        m.elbo_importance_weighting(torch.zeros(4, 2, 1, 32, 32), 0)


def test_trainer_arithmetic():
    """the reference's two trainers share preprocess and compute_loss: the inherited ones against the VRNN trainer's"""
    from VRNN.trainer import Solver
    assert sorted(FX["checkpoint_keys"]) == sorted(
        ["epoch", "model_state_dict", "optimizer_state_dict", "loss", "kl_loss", "recon_loss", "losses", "bits",
         "plot_counter", "annealing_counter", "args"])
    for key, e in FX["preprocess"].items():
        nb, rng = key.split("_")
        s = Solver(Namespace(**dict(SOLVER_ARGS, n_bits=int(nb), preprocess_range=rng)))
        y = s.preprocess(e["x"])
        assert torch.equal(y, e["y"]), key
        assert torch.equal(s.preprocess(y, reverse=True), e["y_back"]), key
    e = FX["compute_loss"]
    s = Solver(Namespace(**SOLVER_ARGS))
    s.beta = e["beta"]
    loss = s.compute_loss(e["nll"], e["kl"], torch.Size(e["dims"]), t=e["t"])
    assert float(loss) == pytest.approx(float(e["loss"]), rel=1e-6)
    for got, want in ((s.bits[-1], e["bits"]), (s.losses[-1], e["losses"]), (s.kl_loss[-1], e["kl_loss"]),
                      (s.recon_loss[-1], e["recon_loss"])):
        assert got == pytest.approx(want, rel=1e-6)


def test_gauss_heads_argument_refusals():
    """what rfn_hip.ops.gauss_heads refuses before it touches a device, and that there is no CPU path behind it"""
    from rfn_hip import ops
    t = torch.zeros(3, 5)
    assert ops.gauss_heads_check(t, t, t, t, t, t, ops.GAUSS_HEADS_OUTPUTS) == (3, 5)
    assert ops.gauss_heads_check(None, None, t, t, None, t, ("z_p", "p_scale", "logp")) == (3, 5)
    for want in ((), ("z_q", "z_q"), ("zq",)):
        with pytest.raises(ValueError, match="want"):
            ops.gauss_heads(t, t, t, t, t, t, want=want)
    with pytest.raises(ValueError, match="p_loc and p_raw"):
        ops.gauss_heads(t, t, None, t, t, t, want=("z_q",))
    with pytest.raises(ValueError, match="come together"):
        ops.gauss_heads(t, None, t, t, t, t, want=("z_p",))
    with pytest.raises(ValueError, match="eps_q without"):
        ops.gauss_heads(None, None, t, t, t, t, want=("z_p",))
    for want, kw in ((("z_q",), dict(eps_p=t)), (("logq",), dict(eps_p=t)), (("z_p",), dict(eps_q=t)),
                     (("logp",), dict(eps_q=t))):
        with pytest.raises(ValueError, match="needs eps_"):
            ops.gauss_heads(t, t, t, t, want=want, **kw)
    for want in (("kl",), ("q_scale",), ("z_q",)):
        with pytest.raises(ValueError, match="needs q_loc, q_raw"):
            ops.gauss_heads(None, None, t, t, None, t, want=want)
    with pytest.raises(ValueError, match="shape"):
        ops.gauss_heads(t, t, t, torch.zeros(3, 4), t, t, want=("kl",))
    with pytest.raises(ValueError, match=r"\[B, Z\]"):
        ops.gauss_heads(t[0], t[0], t[0], t[0], t[0], t[0], want=("kl",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gauss_heads(t, t, t, t, t, t, want=("kl",))
