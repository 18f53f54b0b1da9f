"""Host side of the SRNN baseline against what tests/golden/make_golden_srnn.py recorded from the reference: the parser of
main_srnn.py, the state_dict of SRNN(args) (keys and shapes; constructed on the CPU, no kernel is called), the seeded
fill both sides share, and the trainer's arithmetic."""
import os
from argparse import Namespace

import pytest
import torch

from tests.srnn_state import describe, fill_state

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX = torch.load(os.path.join(GOLD, "srnn.pt"), weights_only=True)
CONFIGS = list(FX["configs"])

SOLVER_ARGS = dict(n_bits=8, n_epochs=1, learning_rate=1e-4, verbose=False, path="/tmp/", batch_size=2, patience_lr=1,
                   factor_lr=0.5, min_lr=1e-5, patience_es=1, beta_max=1.0, beta_min=1e-4, beta_steps=100,
                   choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=64,
                   preprocess_range="1.0", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                   n_conditions=2, use_validation_set=False)


def test_the_configurations_are_the_issues():
    assert CONFIGS == ["gray_mol", "rgb_mol_resq_smooth", "gray_mol_shots2", "bernoulli_nonorm", "gray_mol_batchnorm"]
    c = FX["configs"]
    assert c["rgb_mol_resq_smooth"]["args"]["x_dim"][1] == 3 and c["rgb_mol_resq_smooth"]["args"]["res_q"]
    assert c["rgb_mol_resq_smooth"]["args"]["enable_smoothing"] and c["gray_mol_shots2"]["args"]["num_shots"] == 2
    assert (c["bernoulli_nonorm"]["args"]["loss_type"], c["bernoulli_nonorm"]["args"]["norm_type"]) == ("bernoulli", "none")
    assert c["gray_mol_batchnorm"]["args"]["norm_type"] == "batchnorm"
    for name, c in FX["configs"].items():
        a = c["args"]
        assert (a["batch_size"], c["T"], a["x_dim"][2:], a["h_dim"], a["a_dim"], a["z_dim"], a["n_logistics"]) == \
            (4, 4, [32, 32], 8, 8, 4, 3)


def test_parser_has_every_flag_of_the_reference():
    import main_srnn
    p = main_srnn.build_parser()
    own = {a.dest: a for a in p._actions}
    for f in FX["flags"]:
        flag = [a for a in p._actions if list(a.option_strings) == f["flags"]]
        assert len(flag) == 1, f["flags"]
        a = flag[0]
        assert a.dest == f["dest"] and a.default == f["default"] and a.nargs == f["nargs"] and a.const == f["const"], f
        assert (None if a.choices is None else list(a.choices)) == f["choices"], f
        assert (None if a.type is None else a.type.__name__) == f["type"], f
    # the defaults parse to the reference's values, and the package's own data flags are there
    ns = p.parse_args([])
    for f in FX["flags"]:
        assert getattr(ns, f["dest"]) == f["default"]
    for extra in ("synthetic_data", "mnist_root", "data_root", "data_cache", "data_seed", "max_steps"):
        assert extra in own


@pytest.mark.parametrize("name", CONFIGS)
def test_state_dict_keys_and_shapes(name):
    from SRNN import SRNN
    c = FX["configs"][name]
    m = SRNN(Namespace(**c["args"]))
    keys, shapes, _ = describe(m.state_dict())
    assert keys == c["keys"]
    assert shapes == c["shapes"]
    state = fill_state(m.state_dict(), c["seed"])
    m.load_state_dict(state)                       # strict
    _, _, sums = describe(state)
    assert sums == pytest.approx(c["checksums"], rel=1e-12, abs=1e-12)


def test_exports_and_refusals():
    import Utils
    from SRNN import SRNN
    from SRNN.trainer import Solver
    assert Utils.DiscretizedMixtureLogits(3).nr_mix == 3 and Utils.DiscretizedMixtureLogits_1d(3).nr_mix == 3
    with pytest.raises(RuntimeError, match="needs logits"):
        Utils.DiscretizedMixtureLogits(3)(logits=torch.zeros(1, 9, 4, 4))
    a = dict(FX["configs"]["gray_mol"]["args"])
    a.update(loss_type="gaussian", dequantize=False)
    with pytest.raises(ValueError, match="dequantize"):
        SRNN(Namespace(**a))
    with pytest.raises(NotImplementedError, match="multigpu"):
        Solver(Namespace(**dict(SOLVER_ARGS, multigpu=True)))
    s = Solver(Namespace(**SOLVER_ARGS))
    assert s.checkpoint_names == ("srnn.pt", "srnn_best_model.pt") and s.scheduler_type == "plateau"
    assert not hasattr(s.args, "scheduler_type")
    with pytest.raises(NotImplementedError):
        s.capture_graph(None)


def test_trainer_arithmetic():
    from SRNN.trainer import Solver
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
