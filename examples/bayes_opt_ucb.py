"""Bayesian optimisation's inner step on the MI355X path: maximise the upper confidence bound ``mean + b * sqrt(var)`` of a fitted
posterior over the test inputs with Adam -- gradients w.r.t. ``xs`` flow through the posterior mean and marginal variances
(``stheno_amd/autograd.py``, ``_PosteriorMarginals``: the back-substitution with the transposed factor on the GPU).

    python examples/bayes_opt_ucb.py [N] [candidates]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
m = int(sys.argv[2]) if len(sys.argv) > 2 else 64
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
x = (torch.rand(n, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev)
y = torch.sin(2 * x[:, :1]) * torch.cos(x[:, 1:]) + 0.05 * torch.randn(n, 1, generator=g, dtype=torch.float64).to(dev)

f = GP(0.5 * EQ().stretch(0.7))                        # a fitted model (examples/learn_hyperparameters.py fits one)
post = f | (f(x, 0.05 ** 2), y)
xs = (torch.rand(m, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev).requires_grad_(True)
opt = torch.optim.Adam([xs], lr=0.05)


def ucb(b=2.0):
    mean, var = post(xs).marginals()
    return mean + b * torch.sqrt(var)


for it in range(41):
    opt.zero_grad()
    acq = ucb()
    (-acq.sum()).backward()
    opt.step()
    if it % 10 == 0:
        print(f"step {it:2d}  mean UCB {float(acq.detach().mean()):+.4f}  best {float(acq.detach().max()):+.4f}", flush=True)
best = int(ucb().detach().argmax())
print("proposed next input:", [round(v, 3) for v in xs.detach()[best].tolist()])
