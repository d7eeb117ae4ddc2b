"""A Bayesian-optimisation LOOP on the MI355X path: the loop of ``bayes_opt_ucb.py`` with the data set growing by one point per round
through ``obs = obs.append(...)`` -- the Cholesky factor of the observations is bordered by the new point (``gpk_potrf_border``,
O(N^2) per round) instead of rebuilt (O(N^3)).  Every round prints its time next to the time of conditioning on all the data from
scratch, and the largest difference of the two posteriors' means over the candidates.

    python examples/bayes_opt_append.py [N] [candidates] [rounds]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, Obs

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
m = int(sys.argv[2]) if len(sys.argv) > 2 else 64
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 8
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
noise = 0.05 ** 2


def objective(x):
    return torch.sin(2 * x[:, :1]) * torch.cos(x[:, 1:])


x = (torch.rand(n, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev)
y = objective(x) + 0.05 * torch.randn(n, 1, generator=g, dtype=torch.float64).to(dev)
f = GP(0.5 * EQ().stretch(0.7))                        # a fitted model (examples/learn_hyperparameters.py fits one)
obs = Obs(f(x, noise), y)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def propose(post):
    """A few Adam steps on the upper confidence bound over random candidates; the best one."""
    xs = (torch.rand(m, 2, generator=g, dtype=torch.float64) * 6 - 3).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([xs], lr=0.05)
    for _ in range(10):
        opt.zero_grad()
        mean, var = post(f)(xs).marginals()
        acq = mean + 2.0 * torch.sqrt(var)
        (-acq.sum()).backward()
        opt.step()
    return xs.detach()[int(acq.detach().argmax())][None, :], xs.detach()


post = f.measure | obs
post(f)(x[:m]).marginals()                             # (factorises the first N points: the factor every round grows)
for r in range(rounds):
    x_new, cand = propose(post)
    y_new = objective(x_new) + 0.05 * torch.randn(1, 1, generator=g, dtype=torch.float64).to(dev)
    x, y = torch.cat([x, x_new]), torch.cat([y, y_new])

    def grown():
        new = obs.append(f(x_new, noise), y_new)
        return new, (f.measure | new)(f)(cand).marginals()

    def from_scratch():
        return (f.measure | Obs(f(x, noise), y))(f)(cand).marginals()

    (obs, (mean, _)), t_append = timed(grown)
    (mean_ref, _), t_scratch = timed(from_scratch)
    post = f.measure | obs
    print(f"round {r}: N = {x.shape[0]}  y_new = {float(y_new):+.4f}  append {t_append:7.2f} ms   from scratch {t_scratch:7.2f} ms   "
          f"max |mean difference| {float((mean - mean_ref).abs().max()):.2e}", flush=True)
