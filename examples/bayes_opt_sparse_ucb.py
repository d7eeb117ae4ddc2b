"""Bayesian optimisation's inner step on a PSEUDO-POINT surrogate: maximise the upper confidence bound ``mean + b * sqrt(var)`` of
``f | PseudoObs(f(z), f(x, noise), y)`` over the test inputs with Adam -- gradients w.r.t. ``xs`` flow through the posterior mean and
marginal variances of the sparse posterior (``stheno_amd/autograd.py``, ``_SparsePosteriorMarginals``).  With ``xs`` the only leaf the
backward touches nothing of size N: the surrogate's cost per step does not grow with the data.

    python examples/bayes_opt_sparse_ucb.py [N] [inducing points] [candidates]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, PseudoObs

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 256
c = int(sys.argv[3]) if len(sys.argv) > 3 else 64
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
x = (torch.rand(n, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev)
y = torch.sin(2 * x[:, :1]) * torch.cos(x[:, 1:]) + 0.05 * torch.randn(n, 1, generator=g, dtype=torch.float64).to(dev)
side = int(round(m ** 0.5))
grid = torch.linspace(-3, 3, side, dtype=torch.float64)
z = torch.cartesian_prod(grid, grid).to(dev)             # inducing inputs: a grid over the data's range

f = GP(0.5 * EQ().stretch(0.7))                        # a fitted model (examples/learn_hyperparameters.py sparse fits one)
post = f | PseudoObs(f(z), f(x, 0.05 ** 2), y)
xs = (torch.rand(c, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev).requires_grad_(True)
opt = torch.optim.Adam([xs], lr=0.05)


def ucb(b=2.0):
    mean, var = post(xs).marginals()
    return mean + b * torch.sqrt(var)


start = float(ucb().detach().mean())
for it in range(41):
    opt.zero_grad()
    acq = ucb()
    (-acq.sum()).backward()
    opt.step()
    if it % 10 == 0:
        print(f"step {it:2d}  mean UCB {float(acq.detach().mean()):+.4f}  best {float(acq.detach().max()):+.4f}", flush=True)
final = ucb().detach()
print(f"acquisition before the ascent {start:+.4f}, after {float(final.mean()):+.4f}")
print("proposed next input:", [round(v, 3) for v in xs.detach()[int(final.argmax())].tolist()])
