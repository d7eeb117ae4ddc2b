"""How far is a pseudo-point posterior from the exact one?  The 2-Wasserstein distance between their predictions at the same points,
as a function of the number of inducing points -- written against ``stheno_amd.torch``.

    python examples/sparse_posterior_distance.py [N] [N*]

``post_sparse(xs).w2(post_exact(xs))`` compares the two JOINT predictive distributions, means and full covariances: unlike ``kl`` it is
symmetric and stays finite where a predictive covariance is nearly singular.  The distance is
``sqrt(|dm|^2 + tr V1 + tr V2 - 2 |L2^T L1|_*)``; the nuclear norm is summed by a Newton-Schulz polar iteration on the fp64 GEMM
(``gpk_nuclear_norm``), from the two Cholesky factors -- no eigendecomposition.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, PseudoObs

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device("cuda")
dt = torch.float64
width = 60.0                                                   # the inputs spread over 60 length scales

gen = torch.Generator().manual_seed(0)
x = (width * torch.rand(n, generator=gen, dtype=dt)).sort().values.to(dev)[:, None]
y = torch.sin(x) + 0.3 * torch.randn(n, 1, generator=gen, dtype=dt).to(dev)
xs = torch.linspace(0.0, width, ns, dtype=dt, device=dev)[:, None]

with torch.no_grad():
    f = GP(EQ())
    exact = (f | (f(x, 0.09), y))(xs)
    to_prior = float(exact.w2(f(xs)))
    print(f"N = {n}, N* = {ns}: the exact posterior has moved {to_prior:.4f} from the prior")
    for m in (10, 20, 40, 60, 80, 120):
        z = torch.linspace(0.0, width, m, dtype=dt, device=dev)[:, None]
        sparse = (f | PseudoObs(f(z), f(x, 0.09), y))(xs)
        d = float(sparse.w2(exact))
        print(f"  {m:4d} inducing points: W2(sparse, exact) = {d:.3e}   ({d / to_prior:.1e} of the way from the prior)")
