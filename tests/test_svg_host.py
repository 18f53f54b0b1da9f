"""Host side of the SVG baseline against what tests/golden/make_golden_svg.py recorded from the reference: the parser of
main_svg.py (every flag of the reference with its default, plus --variance and the six additions), the state_dict of
SVG(args) (keys and shapes), the seeded fill both sides share, the trainer's arithmetic (the SVG trainer's own
`preprocess`, with its "none" range), the checkpoint names, the refusals, and the mirror itself on the CPU (the torch route
of rfn_hip.ops.lstm_cell) for gray_mse and bernoulli: the loss within 1e-5 relative of the fixture's float32 (kl, nll), the
predicted frames within 1e-5 absolute, and the running buffers moved as the reference moves them.  This pins the draw
order and the reference's quirks before any GPU run."""
import os
from argparse import Namespace

import pytest
import torch

from tests.srnn_state import describe, fill_state

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX = torch.load(os.path.join(GOLD, "svg.pt"), weights_only=True)
CONFIGS = list(FX["configs"])
ADDITIONS = {"synthetic_data", "mnist_root", "data_root", "data_cache", "data_seed", "max_steps"}

SOLVER_ARGS = dict(n_bits=8, n_epochs=1, learning_rate=1e-4, verbose=False, path="/tmp/", batch_size=2, patience_lr=1,
                   factor_lr=0.5, min_lr=1e-5, patience_es=1, beta_max=1.0, beta_min=1e-4, beta_steps=100,
                   choose_data="mnist", n_frames=4, digit_size=28, step_length=4, num_digits=2, image_size=64,
                   preprocess_range="none", preprocess_scale=255, num_workers=0, multigpu=False, n_predictions=2,
                   n_conditions=2, use_validation_set=False)


def frames(k, loss_type):
    """the float32 frames of a fixture's uint8 values, as make_golden_svg.frames"""
    return (k >= 128).float() if loss_type == "bernoulli" else k.float() / 255.0


def part(name, which):
    return torch.load(os.path.join(GOLD, "svg.%s.%s.pt" % (name, which)), weights_only=True)


def filled(name):
    from SVG import SVG
    c = FX["configs"][name]
    m = SVG(Namespace(**c["args"]))
    state = fill_state(m.state_dict(), c["seed"])
    m.load_state_dict(state)
    return m, state


def test_the_configurations_are_the_issues():
    assert CONFIGS == ["gray_mse", "rgb_mse", "bernoulli", "gaussian"]
    c = FX["configs"]
    assert c["rgb_mse"]["args"]["x_dim"][1] == 3
    assert [c[n]["args"]["loss_type"] for n in CONFIGS] == ["mse", "mse", "bernoulli", "gaussian"]
    biggest = max(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if not f.startswith("svg"))
    for name, c in FX["configs"].items():
        a = c["args"]
        assert (a["batch_size"], c["T"], a["x_dim"][2:], a["c_features"], a["h_dim"], a["z_dim"], a["preprocess_range"],
                a["variance"]) == (4, 3, [64, 64], 8, 16, 4, "none", 1.0)
        assert (a["posterior_rnn_layers"], a["predictor_rnn_layers"], a["prior_rnn_layers"]) == (1, 2, 1)
        files = c["parts"] + ["svg_iw.%s.pt" % name]
        assert len(c["parts"]) == 2
        for f in files:
            size = os.path.getsize(os.path.join(GOLD, f))
            assert size <= biggest and size <= 1 << 20, (f, size)
    assert len(FX["grad_names"]) == 14


def test_parser_has_every_flag_of_the_reference():
    import main_svg
    p = main_svg.build_parser()
    assert len(FX["flags"]) >= 35
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
    assert (ns.batch_size, ns.num_workers, ns.learning_rate, ns.preprocess_range, ns.beta_max, ns.z_dim, ns.c_features,
            ns.loss_type) == (100, 4, 0.001, "none", 0.0001, 12, 256, "mse")
    # the reference's parser has no --variance although its model reads args.variance: the one documented deviation
    assert "variance" not in {f["dest"] for f in FX["flags"]}
    var = [a for a in p._actions if a.dest == "variance"][0]
    assert var.default == 1.0 and var.type is float and "never defines" in var.help
    assert {a.dest for a in p._actions} - {"help"} == {f["dest"] for f in FX["flags"]} | ADDITIONS | {"variance"}


@pytest.mark.parametrize("name", CONFIGS)
def test_state_dict_keys_and_shapes(name):
    from SVG import SVG
    c = FX["configs"][name]
    m = SVG(Namespace(**c["args"]))
    keys, shapes, _ = describe(m.state_dict())
    assert keys == c["keys"]
    assert shapes == c["shapes"]
    assert "frame_predictor.lstm.1.weight_ih" in keys and "posterior.std_net.0.weight" in keys
    assert isinstance(m.frame_predictor.lstm[0], torch.nn.LSTMCell)      # the parameter holders stay
    state = fill_state(m.state_dict(), c["seed"])
    m.load_state_dict(state)                       # strict
    _, _, sums = describe(state)
    assert sums == pytest.approx(c["checksums"], rel=1e-12, abs=1e-12)
    for n in FX["grad_names"]:
        assert n in keys and state[n].numel() <= 70000, n


def test_exports_and_refusals():
    import sys
    import SVG  # noqa: F401
    S = sys.modules["SVG.SVG"]                    # (the package's `SVG` attribute is the class)
    from SRNN.trainer import Solver as SRNNSolver
    from SVG import SVG
    from SVG.trainer import Solver
    for n in ("vgg_layer", "Encoder", "Decoder", "lstm_svg", "gaussian_lstm", "SVG", "init_weights"):
        assert hasattr(S, n), n
    a = dict(FX["configs"]["gray_mse"]["args"])
    with pytest.raises(ValueError, match="undefined loss"):
        SVG(Namespace(**dict(a, loss_type="mol")))
    with pytest.raises(NotImplementedError, match="SVG.*multigpu"):
        Solver(Namespace(**dict(SOLVER_ARGS, multigpu=True)))
    s = Solver(Namespace(**SOLVER_ARGS))
    assert isinstance(s, SRNNSolver)
    assert s.checkpoint_names == ("svg.pt", "svg_best_model.pt") and s.scheduler_type == "plateau"
    assert isinstance(s.make_model.__self__, Solver) and Solver.make_model is not SRNNSolver.make_model
    with pytest.raises(NotImplementedError, match="SVG"):
        s.capture_graph(None)
    with pytest.raises(NotImplementedError, match="SVG"):
        s.plotter()
    m = SVG(Namespace(**a))
    with pytest.raises(ValueError, match="K must be"):
        m.elbo_importance_weighting(torch.zeros(4, 2, 1, 64, 64), 0)
    assert m.training
    with pytest.raises(RuntimeError, match="eval mode"):
        m.predict_draws(torch.zeros(4, 2, 1, 64, 64), 1, 1, 2, 5)
    m.eval()
    with pytest.raises(ValueError, match="n_draws"):
        m.predict_draws(torch.zeros(4, 2, 1, 64, 64), 1, 1, 0, 5)
    # the hidden state follows the parameters: batch_size rows by default, no device is named anywhere
    hid = m.frame_predictor.init_hidden()
    assert len(hid) == 2 and hid[0][0].shape == (4, 16) and hid[0][0].device == m.frame_predictor.embed.weight.device
    assert m.prior.init_hidden(rows=7)[0][1].shape == (7, 16)


def test_trainer_arithmetic():
    from SVG.trainer import Solver
    assert sorted(FX["checkpoint_keys"]) == sorted(
        ["epoch", "model_state_dict", "optimizer_state_dict", "loss", "kl_loss", "recon_loss", "losses", "bits",
         "plot_counter", "annealing_counter", "args"])
    assert len(FX["preprocess"]) == 8
    for key, e in FX["preprocess"].items():
        nb, rng = key.split("_")
        s = Solver(Namespace(**dict(SOLVER_ARGS, n_bits=int(nb), preprocess_range=rng)))
        y = s.preprocess(e["x"])
        assert torch.equal(y, e["y"]), key
        assert torch.equal(s.preprocess(y, reverse=True), e["y_back"]), key
    with pytest.raises(ValueError, match="Invalid preprocess"):
        Solver(Namespace(**dict(SOLVER_ARGS, preprocess_range="2.0"))).preprocess(torch.zeros(1))
    e = FX["compute_loss"]
    s = Solver(Namespace(**SOLVER_ARGS))
    s.beta = e["beta"]
    loss = s.compute_loss(e["nll"], e["kl"], torch.Size(e["dims"]), t=e["t"])
    assert float(loss) == pytest.approx(float(e["loss"]), rel=1e-6)
    for got, want in ((s.bits[-1], e["bits"]), (s.losses[-1], e["losses"]), (s.kl_loss[-1], e["kl_loss"]),
                      (s.recon_loss[-1], e["recon_loss"])):
        assert got == pytest.approx(want, rel=1e-6)


@pytest.mark.parametrize("name", ["gray_mse", "bernoulli"])
def test_the_mirror_on_the_cpu(name):
    """the torch route end to end: draw order, the two encoder calls per step, the reference's formulas"""
    m, state = filled(name)
    f, gen = part(name, "loss"), part(name, "gen")
    x = frames(f["k"], m.loss_type)
    T = x.shape[1]
    m.train()
    kl, nll = m.loss(x, draws=f["draws"])
    print("%s: kl %.6f (ref %.6f)  nll %.6f (ref %.6f)" % (name, float(kl.detach()), f["out"][0], float(nll.detach()), f["out"][1]))
    assert float(kl.detach()) == pytest.approx(f["out"][0], rel=1e-5)
    assert float(nll.detach()) == pytest.approx(f["out"][1], rel=1e-5)
    tracked = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
    assert len(tracked) == 21                                           # 11 batch norms in the encoder, 10 in the decoder
    for k, v in tracked.items():
        assert v == (2 * (T - 1) if k.startswith("encoder.") else T - 1), (k, v)
    with pytest.raises(RuntimeError, match="left over"):
        m.loss(x[:, :2], draws=f["draws"])
    m.load_state_dict(state)
    m.eval()
    p, r = gen["predict"], gen["reconstruct"]
    assert (p["n_predictions"], p["n_conditions"]) == (2, 1)
    with torch.no_grad():
        tx, pr = m.predict(x, 2, 1, draws=p["draws"])
        rc = m.reconstruct(x, draws=r["draws"])
    assert torch.equal(tx, x[:, :1].transpose(0, 1)) and pr.shape == p["predictions"].shape
    err = float((pr - p["predictions"]).abs().max())
    err_r = float((rc[1:] - r["recons_from_1"]).abs().max())
    print("%s: predicted frames differ by %.2e, reconstructed by %.2e" % (name, err, err_r))
    assert err <= 1e-5 and err_r <= 1e-5
    assert rc.shape[0] == T and float(rc[0].abs().max()) == 0.0
    with torch.no_grad():
        s = m.sample(x, 3)
    assert s.shape == (3,) + tuple(x[:, 0].shape) and float(s[0].abs().max()) == 0.0 and float(s[1].abs().max()) > 0.0
