"""developer probe: every librfn_hip launch of a small flow, in order, as `entry point <TAB> kind <TAB> label <TAB> shape
<TAB> flops <TAB> bytes` lines (all fields of the launch's profiling metadata: bench.py's per-kernel table is built
from them).  A ListGlow of L=3, K=2, Hd=256 on N=4 frames of 2x32x32 (level 0 takes the fused coupling kernels in
'mixed', level 1 is the wide level below the fused forward's pixel threshold, level 2 a small map) runs log_prob +
backward twice -- the first, data-initialising call walks the steps one by one, the second takes the level nodes -- and
then sample twice (the second reuses the generation cache).  Two builds that print the same lines launch the same
kernels on the same shapes in the same order: python tools/coupling_launches.py > a.txt with RFN_CONV_PRECISION = mixed
| bf16x3 | f32.  RFN_PKG_DIR selects another build of the package (A/B on the same box, as tools/bench_wgrad.py).

--dump FILE: after that, write what one more log_prob + backward and one more sample compute (z, nll, every parameter's
gradient, the sample) to FILE with torch.save, twice: on the flow as built ("init": Conv2dZeros weights are zero, so the
nets' inner gradients are) and with every parameter moved by seeded noise ("perturbed").  tools/coupling_compare.py
compares such files."""
import os, sys
from argparse import Namespace
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.environ.get("RFN_PKG_DIR") or os.path.join(ROOT, "recurrent-flows-msc_amd")):
    sys.path.insert(0, p)
import torch
from rfn_hip import lib as L
from Flow.glow import ListGlow

N, S, COND = 4, 32, [32, 64, 128]
args = Namespace(learn_prior=False, n_units_prior=16, make_conditional=True, base_norm="actnorm", non_lin_glow="relu",
                 split2d_act="softplus", L=3, K=2, n_bits=8, flow_norm="actnorm", flow_batchnorm_momentum=0.0,
                 LU_decomposed=True, n_units_affine=256, clamp_type="realnvp")
torch.manual_seed(0)
flow = ListGlow([N, 2, S, S], [[N, c, S >> (l + 1), S >> (l + 1)] for l, c in enumerate(COND)], [N, 8, 4, 4], args).cuda()
x = torch.rand(N, 2, S, S).cuda() - 0.5
cond = [torch.randn(N, c, S >> (l + 1), S >> (l + 1)).cuda() for l, c in enumerate(COND)]
L.PROFILE = []
for _ in range(2):
    flow.zero_grad(set_to_none=True)
    _, nll = flow.log_prob(x, cond, None)
    nll.sum().backward()
for _ in range(2):
    flow.sample(None, cond, None, num_samples=N)
torch.cuda.synchronize()
rec, L.PROFILE = L.PROFILE, None
for name, meta, _, _ in rec:
    kind, label, flops, shape, nbytes = ("-",) * 5 if meta is None else meta
    print("\t".join(str(v) for v in (name, kind, label, shape, flops, nbytes)))


def outputs():
    flow.zero_grad(set_to_none=True)
    torch.manual_seed(1)   # (the dequantisation draw and the sample's base draw)
    z, nll = flow.log_prob(x, cond, None)
    nll.sum().backward()
    out = {"z": z.detach(), "nll": nll.detach(), "sample": flow.sample(None, cond, None, num_samples=N)}
    out.update(("grad/" + n, p.grad.detach()) for n, p in flow.named_parameters() if p.grad is not None)
    return {k: v.cpu().clone() for k, v in out.items()}


if "--dump" in sys.argv:
    dump = {"init": outputs()}
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in flow.parameters():
            p.add_(0.03 * torch.randn(p.shape, generator=g).to(p.device))
    dump["perturbed"] = outputs()
    torch.save(dump, sys.argv[sys.argv.index("--dump") + 1])
