"""GPU tests of RFN.iw_log_weights / RFN.elbo_importance_weighting on the tiny model of
__graft_entry__._tiny_args(): agreement with the float64 restatement of tests/iw_ref.py fed the very noise tensors the
addressed generators produce, independence of how the chains are split into passes and calls, reproducibility, that
nothing of the model or of torch's generators changes, and the Evaluator's route."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests import iw_ref
from tests.test_predict_draws import close

pytestmark = pytest.mark.gpu

B, T, KC, SEED, FIRST_SEQ = 2, 4, 3, 9, 5
CONFIGS = {"default": {}, "res_q": {"res_q": True}, "smoothing": {"enable_smoothing": True},
           "with_skip": {"skip_connection_flow": "with_skip"}}


@pytest.fixture(scope="module", params=list(CONFIGS))
def case(request):
    """(model in eval mode after its data dependent init, args, batch, log weights of the reference call, the float64
    restatement's): computed once per configuration and left unchanged"""
    import __graft_entry__ as ge
    from RFN import RFN
    from rfn_hip import ops
    args = ge._tiny_args()
    for k, v in CONFIGS[request.param].items():
        setattr(args, k, v)
    torch.manual_seed(5)
    m = RFN(args).cuda().train()
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(B, T, *args.x_dim[1:], generator=g) - 0.5).cuda()
    m.loss(x, 0)
    m.eval()
    lw = m.iw_log_weights(x, KC, SEED, first_seq=FIRST_SEQ)
    # the restatement on the numbers of the defined addresses: eps_t slot 0 at step t, u_t slot 24 at step t
    z = tuple(m.z_0x.shape[1:])
    eps = [ops.keyed_normal([z], B, KC, SEED, t, FIRST_SEQ, 0, device="cuda")[0].view(KC, B, *z).cpu().double()
           for t in range(1, T)]
    u = ops.keyed_uniform(tuple(x.shape[2:]), B, KC, SEED, 1, n_steps=T - 1, slot=24, scale=2.0 ** -args.n_bits,
                          first_seq=FIRST_SEQ, device="cuda").view(T - 1, KC, B, *x.shape[2:]).cpu().double()
    ref = iw_ref.iw_log_weights_ref(iw_ref.state_dict64(m), vars(args), x.cpu().double(), eps, list(u))
    return m, args, x, lw, ref


def test_log_weights_and_bound_against_the_restatement(case):
    m, args, x, lw, ref = case
    assert lw.is_cuda and lw.dtype == torch.float64 and tuple(lw.shape) == (KC, B)
    print("log w  gpu %s\n       ref %s\n       max |diff| / max |ref| = %.3e" %
          (lw.cpu().tolist(), ref.tolist(), float((lw.cpu() - ref).abs().max() / ref.abs().max())))
    close(lw.float(), ref)
    assert float((lw[0] - lw[1]).abs().max()) > 1e-3          # the chains differ
    want = -iw_ref.iw_bound_ref(ref).mean()
    got = m.elbo_importance_weighting(x, KC, seed=SEED, first_seq=FIRST_SEQ)
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
    print("bound  gpu %.6f  ref %.6f" % (float(got), float(want)))
    close(got.float(), want)
    # K = 1 is the one-sample estimate: the mean of chain 0's weights
    one = m.elbo_importance_weighting(x, 1, seed=SEED, first_seq=FIRST_SEQ)
    close(one.float(), -ref[0].mean())
    assert float(got) <= float(-lw.mean()) + 1e-9 * abs(float(got))      # bound >= mean_k log w, as a loss: <=


def test_independent_of_passes_and_calls(case):
    m, args, x, lw, ref = case
    for P in (1, 2, 3, 7):
        close(m.iw_log_weights(x, KC, SEED, first_seq=FIRST_SEQ, chains_per_pass=P).float(), lw)
        close(m.elbo_importance_weighting(x, KC, seed=SEED, first_seq=FIRST_SEQ, chains_per_pass=P).float(),
              -iw_ref.iw_bound_ref(lw).mean())
    parts = [m.iw_log_weights(x, 1, SEED, first_seq=FIRST_SEQ, first_chain=0),
             m.iw_log_weights(x, 2, SEED, first_seq=FIRST_SEQ, first_chain=1)]
    close(torch.cat(parts, 0).float(), lw)
    # first_seq and seed change the result
    for other in (dict(seed=SEED, first_seq=FIRST_SEQ + 1), dict(seed=SEED + 1, first_seq=FIRST_SEQ)):
        assert float((m.iw_log_weights(x, KC, **other) - lw).abs().max()) > 1e-3


def test_reproducible_and_leaves_everything_as_it_was(case):
    m, args, x, lw, ref = case
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(123)
    cpu, gpu = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    again = m.iw_log_weights(x, KC, SEED, first_seq=FIRST_SEQ)
    assert torch.equal(again, lw)                     # the same bits, whatever torch's generator holds
    bound = m.elbo_importance_weighting(x, KC, seed=SEED, first_seq=FIRST_SEQ)
    assert torch.equal(bound, m.elbo_importance_weighting(x, KC, seed=SEED, first_seq=FIRST_SEQ))
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), gpu)
    after = m.state_dict()
    assert set(after) == set(state)
    for k, v in state.items():                        # parameters and buffers, running statistics included
        assert torch.equal(after[k], v), k
    assert not m.training and not lw.requires_grad
    m.train()
    try:
        for call in (lambda: m.iw_log_weights(x, KC, SEED), lambda: m.elbo_importance_weighting(x, KC)):
            with pytest.raises(RuntimeError, match="eval mode"):
                call()
    finally:
        m.eval()
    for k, v in state.items():
        assert torch.equal(m.state_dict()[k], v), k


def test_evaluator_get_loss(case):
    """get_loss with rfn_iw_samples = 3 over two synthetic batches is the mean of the per-batch values computed
    directly; unset, it is RFN.loss through compute_loss"""
    from evaluation_metrics import Evaluator
    m, args, x, lw, ref = case
    g = torch.Generator().manual_seed(17)
    batches = [torch.rand(B, T + 1, *args.x_dim[1:], generator=g) - 0.5 for _ in range(2)]
    solver = SimpleNamespace(model=m, args=SimpleNamespace(n_frames=T, n_conditions=2, choose_data="mnist"),
                             device=torch.device("cuda"), preprocess=lambda t, reverse=False: t)
    ev = Evaluator(solver, settings=SimpleNamespace(rfn_iw_samples=KC, seed=11, iw_chains_per_pass=2))
    mean, std = ev.get_loss("rfn.pt", loader=batches)
    dims = 1
    for d in args.x_dim[1:]:
        dims *= d
    per = []
    for i, b in enumerate(batches):
        v = m.elbo_importance_weighting(b[:, :T].cuda(), KC, seed=11, first_seq=i * B, chains_per_pass=2)
        per.append(float(v) / (math.log(2.0) * dims * (T - 1)))
    assert std == -1
    assert float(mean) == pytest.approx(float(torch.FloatTensor(per).mean()), rel=1e-6)
    assert abs(per[0] - per[1]) > 1e-6
    # unset: the ELBO path, from torch's generator
    plain = Evaluator(solver, settings=SimpleNamespace(seed=11))
    torch.manual_seed(4)
    elbo, _ = plain.get_loss("rfn.pt", loader=batches)
    torch.manual_seed(4)
    want = []
    for b in batches:
        with torch.no_grad():
            _, kl, nll = m.loss(b[:, :T].cuda(), 0)
        want.append(plain.compute_loss(nll=nll, kl=kl, dims=b.shape[2:], t=T - 1)[0])
    assert float(elbo) == float(torch.FloatTensor(want).mean())
