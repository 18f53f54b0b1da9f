#!/usr/bin/env python3
"""Generate the fixtures of SRNN.elbo_importance_weighting by running the REFERENCE implementation on the CPU
(SRNN/SRNN.py:482-579 of the reference, the bound its evaluator reports as the baselines' bits/dim).

Test infrastructure only, in the manner of make_golden_srnn.py (whose configurations, CPU shims and RNG capture are
used): needs the reference checkout (RFN_REFERENCE), writes tensors, plain scalars and lists of names only.

Usage:  python tests/golden/make_golden_srnn_iw.py          (from the repo root)

srnn_iw.<config>.pt   {"config", "K", "mode", "x", "draws", "ref32", "ref64", "data_seed", "seed"}: the input, the
                      recorded draws of the reference's float32 call in eval mode (per time step and inner sample:
                      encoder eps, prior eps), its value, and the same call replayed in float64 (same state, same
                      draws).  Parameters are NOT stored: tests/srnn_state.fill_state(state_dict, seed) fills both sides.

An input is accepted when the reference's own float32 value lies within 1e-4 relative of its float64 replay (the bound
tests/test_srnn.py holds losses to); data seeds are tried in order and the one taken is recorded.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (CPU shims and RNG capture are installed on import)
import make_golden_srnn as S  # noqa: E402

from tests.srnn_state import fill_state  # noqa: E402

import torch  # noqa: E402

IW_CONFIGS = {"gray_mol": 3, "rgb_mol_resq_smooth": 2, "bernoulli_nonorm": 2, "gray_mol_batchnorm": 2}   # name: K


def replay64(SRNN, args, state, x, draws, K):
    """the recorded call once more in float64: a fresh model in the same state, eval mode, the same draws"""
    import torch.distributions.normal as tdn
    torch.set_default_dtype(torch.float64)
    try:
        m = SRNN(args)
        m.load_state_dict(state)
        m = m.double().eval()
        q = [t.double() for _, t in draws]
        tdn._standard_normal = lambda shape, dtype=None, device=None: q.pop(0)

        def uniform_(self, *a, **k):
            return self.copy_(q.pop(0))
        torch.Tensor.uniform_ = uniform_
        with torch.no_grad():
            v = m.elbo_importance_weighting(x.double(), K)
        assert not q, "draws left over"
        return float(v)
    finally:
        tdn._standard_normal, torch.Tensor.uniform_ = G._orig_std_normal, G._orig_uniform_
        torch.set_default_dtype(torch.float32)


def gen():
    import Utils.modules as um
    um.device = torch.device("cpu")
    from SRNN.SRNN import SRNN
    for name, K in IW_CONFIGS.items():
        args = S.srnn_args(**S.SRNN_CONFIGS[name])
        B, C, H, W = args.x_dim
        for data_seed in range(2026, 2026 + 12):
            torch.manual_seed(87)
            g = torch.Generator().manual_seed(data_seed)
            m = SRNN(args)
            state = fill_state(m.state_dict(), S.SEED)
            m.load_state_dict(state)
            k = torch.randint(0, 256, (B, S.T, C, H, W), generator=g).float()
            x = 2.0 * k / 255.0 - 1.0 if args.loss_type == "mol" else (k >= 128).float()
            m.eval()
            torch.manual_seed(data_seed)
            with torch.no_grad():
                G.start_capture()
                v32 = float(m.elbo_importance_weighting(x, K))
                d = G.stop_capture()
            v64 = replay64(SRNN, args, state, x, d, K)
            rel = abs(v32 - v64) / abs(v64)
            print(name, "K", K, "data seed", data_seed, "float32 %.6f float64 %.6f relative %.2e" % (v32, v64, rel))
            if rel <= 1e-4:
                break
        else:
            raise RuntimeError("no input found for " + name)
        assert len(d) == 2 * K * (S.T - 1) and all(kind == "normal" for kind, _ in d)
        G.save("srnn_iw.%s.pt" % name, {"config": name, "K": K, "mode": "eval", "x": x, "draws": [(a, t) for a, t in d],
                                        "ref32": v32, "ref64": v64, "data_seed": data_seed, "seed": S.SEED})


if __name__ == "__main__":
    gen()
