"""CPU tests of the evaluation driver (evaluation_metrics/eval_settings.py) and of the host-side rules of the temperature
sweep: the parser's flags and defaults, the t<T> file-name rule, the refusal of the baseline models, the draws-per-pass
rule of Evaluator.get_eval_values_temperatures, and the row layout shared by ops.keyed_normal(tiles=K) and
RFN.predict_draws(temperatures=...)."""
from argparse import Namespace

import pytest
import torch

# the reference's flags with its defaults (evaluation_metrics/eval_settings.py:169-224 of the reference) ...
REFERENCE_DEFAULTS = dict(
    folder_path="./work1/s146996/", experiment_names=["rfn_bair_final"], label_names=["RFN-BAIR"], model_path=["rfn.pt"],
    use_validation_set=False, num_samples_to_plot=3, n_frames=30, start_predictions=5, temperatures=[0.7], resample=30,
    extra_plots=False, test_temperature=False, debug_mnist=True, calc_eval=True, debug_plot=True, n_conditions=5,
    eval_parameters=False, calc_fvd=False, fvd_predicts=13, eval_loss=False)
# ... and ours
OUR_DEFAULTS = dict(draws_per_pass=None, seed=0, lpips_weights=None, fvd_weights=None, max_batches=None)
BOOL_FLAGS = ("use_validation_set", "extra_plots", "test_temperature", "debug_mnist", "calc_eval", "debug_plot",
              "eval_parameters", "calc_fvd", "eval_loss")


def test_parser_flags_and_defaults():
    from evaluation_metrics import eval_settings as E
    got = vars(E.build_parser().parse_args([]))
    assert got == dict(REFERENCE_DEFAULTS, **OUR_DEFAULTS)
    for name in BOOL_FLAGS:                      # --flag / --no-flag pairs, as the reference's add_bool_arg
        assert getattr(E.build_parser().parse_args(["--" + name]), name) is True
        assert getattr(E.build_parser().parse_args(["--no-" + name]), name) is False
        with pytest.raises(SystemExit):
            E.build_parser().parse_args(["--" + name, "--no-" + name])
    s = E.parse_args("--temperatures 0.3 0.5 1 --experiment_names a b --model_path rfn.pt rfn.pt --draws_per_pass 8 "
                     "--seed 4 --lpips_weights /w --fvd_weights /a /b --max_batches 2 --resample 7".split())
    assert s.temperatures == [0.3, 0.5, 1.0] and all(isinstance(t, float) for t in s.temperatures)
    assert s.experiment_names == ["a", "b"] and s.model_path == ["rfn.pt", "rfn.pt"]
    assert (s.draws_per_pass, s.seed, s.max_batches, s.resample) == (8, 4, 2, 7)
    assert s.lpips_weights == "/w" and s.fvd_weights == ["/a", "/b"]     # one entry: the directory itself


def test_temperature_file_names():
    from evaluation_metrics import eval_settings as E
    assert E.temperature_file_name(0.7) == "t07evaluations.pt"
    assert E.temperature_file_name(1.0) == "t10evaluations.pt"
    assert E.temperature_file_name(0.001) == "t0001evaluations.pt"
    assert len(E.EVAL_KEYS) == 11 and len(E.FULL_KEYS) == 15
    d = E.eval_dict((torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 3), None, torch.zeros(1), torch.zeros(1),
                     torch.zeros(1), torch.ones(2, 3), torch.ones(2, 3), None), 0.7)
    assert tuple(d) == E.EVAL_KEYS and d["temperature"] == 0.7
    assert d["LPIPS_values"] is None and d["LPIPS_std_mean"] is None


def test_baseline_models_are_refused(tmp_path):
    from evaluation_metrics import eval_settings as E
    with pytest.raises(ValueError, match="baseline models"):
        E.solver_class("vrnn.pt")
    settings = E.parse_args(["--folder_path", str(tmp_path) + "/", "--experiment_names", "x", "--model_path", "vrnn.pt"])
    with pytest.raises(ValueError, match="vrnn.pt"):      # before any file is read
        E.main(settings)
    from RFN.trainer import Solver
    assert E.solver_class("rfn.pt") is Solver


def test_draws_per_temperature_rule():
    from evaluation_metrics import Evaluator
    P = Evaluator.draws_per_temperature
    assert [P(8, k) for k in (1, 2, 3, 6, 8, 9, 20)] == [8, 4, 2, 1, 1, 1, 1]
    assert P(4, 2) == 2 and P(1, 1) == 1 and P(48, 6) == 8
    for dpp in range(1, 20):
        for k in range(1, 12):
            assert P(dpp, k) == max(1, dpp // k)
    with pytest.raises(ValueError):
        P(0, 2)
    with pytest.raises(ValueError):
        P(4, 0)
    # the sweep needs the setting, and distinct temperatures
    solver = Namespace(model=None, args=Namespace(), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="draws_per_pass"):
        Evaluator(solver).get_eval_values_temperatures([0.5, 1.0])
    with pytest.raises(ValueError, match="duplicates"):
        Evaluator(solver, settings=Namespace(draws_per_pass=4)).get_eval_values_temperatures([0.5, 0.5])


def test_tiled_row_layout():
    """row (k * n_draws + r) * B + b, against the enumeration temperature-major, then draw-major, then sequence; the
    per-row temperature vector of RFN.predict_draws follows it"""
    from RFN import RFN
    from rfn_hip import ops
    for K, P, B in ((1, 1, 1), (2, 3, 2), (3, 2, 5), (6, 1, 4)):
        n = 0
        for k in range(K):
            for r in range(P):
                for b in range(B):
                    row = ops.keyed_normal_tiled_row(k, r, b, P, B)
                    assert row == n
                    assert row % (P * B) == r * B + b          # the untiled row whose values it repeats
                    n += 1
        assert n == K * P * B
        values = [0.25 * (k + 1) for k in range(K)]
        rows = RFN._temperature_rows(values, P, B, "cpu")
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (K * P * B,)
        for k in range(K):
            for r in range(P):
                for b in range(B):
                    assert float(rows[ops.keyed_normal_tiled_row(k, r, b, P, B)]) == values[k]


def test_temperature_lists_of_predict_draws():
    from RFN import RFN
    m = Namespace(temperature=0.7, kl_temperature=1)
    L = lambda t, kl: RFN._temperature_lists(m, t, kl)
    assert L([0.5, 1], None) == ([0.5, 1.0], [1.0, 1.0])
    assert L(None, (0.1, 0.2, 0.3)) == ([0.7] * 3, [0.1, 0.2, 0.3])
    assert L([2], [3]) == ([2.0], [3.0])
    with pytest.raises(ValueError, match="2 temperatures and 1 kl_temperatures"):
        L([1, 2], [1])
    with pytest.raises(ValueError, match="empty"):
        L([], None)
    with pytest.raises(TypeError, match="temperatures"):
        L(0.5, None)


def test_wrapper_argument_errors_on_the_host():
    """the checks of the two wrappers that need no device"""
    from rfn_hip import ops
    with pytest.raises(TypeError, match="tiles"):
        ops.keyed_normal([(4,)], 1, 1, 0, 0, device="cuda", tiles=2.0)
    with pytest.raises(ValueError, match="tiles"):
        ops.keyed_normal([(4,)], 1, 1, 0, 0, device="cuda", tiles=0)
    with pytest.raises(ValueError, match="must have 6 rows"):          # tiles * n_draws * B rows
        ops.keyed_normal(None, 1, 2, 0, 0, out=[torch.zeros(2, 4)], tiles=3)
    o, eps = torch.zeros(3, 4, 2, 2), torch.zeros(3, 2, 2, 2)
    with pytest.raises(TypeError, match="temperature"):
        ops.gauss_sample(o, eps, 0, 0, "0.7")
    with pytest.raises(TypeError, match="temperature tensor must be float32"):
        ops.gauss_sample(o, eps, 0, 0, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="temperature holds 2 values for 3 frames"):
        ops.gauss_sample(o, eps, 0, 0, torch.zeros(2))
