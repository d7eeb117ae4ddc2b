"""Batch Bayesian optimisation's inner step on the MI355X path: choose q = 8 candidates JOINTLY by maximising a Monte-Carlo
acquisition built from reparameterised joint posterior samples, ``mean + chol(cov) xi`` with fixed draws ``xi`` -- qUCB,
``E max_j (mean_j + sqrt(b pi / 2) |s_j - mean_j|)`` (Wilson et al., 2017).  Gradients w.r.t. the candidates flow through the full
posterior covariance and its Cholesky factor (``stheno_amd/autograd.py``: ``_PosteriorCovariance``, the factorisation's
vector-Jacobian product ``gpk_potrf_vjp``); ``examples/bayes_opt_ucb.py`` is the pointwise counterpart.

    python examples/bayes_opt_qucb.py [N] [samples]
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
num = int(sys.argv[2]) if len(sys.argv) > 2 else 128
q = 8
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
x = (torch.rand(n, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev)
y = torch.sin(2 * x[:, :1]) * torch.cos(x[:, 1:]) + 0.05 * torch.randn(n, 1, generator=g, dtype=torch.float64).to(dev)

f = GP(0.5 * EQ().stretch(0.7))                        # a fitted model (examples/learn_hyperparameters.py fits one)
post = f | (f(x, 0.05 ** 2), y)
xs = (torch.rand(q, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev).requires_grad_(True)
xi = torch.randn(q, num, generator=g, dtype=torch.float64).to(dev)      # fixed draws: the acquisition is a deterministic function of xs
opt = torch.optim.Adam([xs], lr=0.05)


def qucb(b=2.0):
    fdd = post(xs)
    s = fdd.sample(xi=xi)                              # (q, num): joint samples, differentiable in xs
    mean = fdd.mean
    return (mean + math.sqrt(b * math.pi / 2) * (s - mean).abs()).max(dim=0).values.mean()


print(f"acquisition before: {float(qucb().detach()):+.4f}", flush=True)
for it in range(41):
    opt.zero_grad()
    acq = qucb()
    (-acq).backward()
    opt.step()
    if it % 10 == 0:
        print(f"step {it:2d}  qUCB {float(acq.detach()):+.4f}", flush=True)
print(f"acquisition after:  {float(qucb().detach()):+.4f}")
print("proposed batch:", [[round(v, 3) for v in row] for row in xs.detach().tolist()])
