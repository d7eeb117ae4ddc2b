"""Bayesian linear regression as a Gaussian process: ``f = slope * ScaleFn(lambda x: x) + intercept`` with ``slope, intercept = GP(1), GP(1)``
-- the reference's first modelling example, written against ``stheno_amd.torch``.

    python examples/bayesian_linear_regression.py [N]

A process times a function of the inputs is a process again (mean ``fn m``, kernel ``fn(x) k(x, y) fn(y)``); the kernel matrix of the
scaled summand is one launch of the fused kernel with a row and a column factor applied at the store, accumulated onto the
intercept's.  Conditioning on ``f`` gives the posteriors of the two random coefficients, read off at any input.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import GP, Measure, ScaleFn

n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
dev = torch.device("cuda")
dt = torch.float64

with Measure() as prior:
    slope, intercept = GP(1), GP(1)
    f = slope * ScaleFn(lambda x: x) + intercept      # (a bare function is refused: wrap it, or pass a callable object)

x = torch.linspace(0.0, 10.0, n, dtype=dt, device=dev)
gen = torch.Generator().manual_seed(0)
true_slope, true_intercept = (float(v) for v in torch.randn(2, generator=gen, dtype=dt))      # a draw from the prior of the coefficients
obs = true_slope * x[:, None] + true_intercept + 0.2 * torch.randn(n, 1, generator=gen, dtype=dt).to(dev)

with torch.no_grad():
    post = prior | (f(x, 0.04), obs)
    zero = torch.zeros(1, dtype=dt, device=dev)
    ms, vs = post(slope)(zero).marginals()
    mi, vi = post(intercept)(zero).marginals()
    evidence = float(f(x, 0.04).logpdf(obs))

print(f"log marginal likelihood: {evidence:.3f}")
print(f"true slope      {true_slope:8.4f}   predicted {float(ms):8.4f} +- {2 * float(vs) ** 0.5:.4f}")
print(f"true intercept  {true_intercept:8.4f}   predicted {float(mi):8.4f} +- {2 * float(vi) ** 0.5:.4f}")
