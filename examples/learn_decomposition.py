"""Learning an additive decomposition -- trend + seasonal + line, observed through their noisy sum -- with the period among the learnt
quantities, then predicting the components (as ``examples/decompose_signal.py`` does with fixed hyper-parameters).

    python examples/learn_decomposition.py [N] [iterations]

The sum's kernel ``v1 * EQ().stretch(l) + v2 * EQ().periodic(p) + v3 * Linear()`` has its terms behind different input maps: the
periodic part sees ``(sin(2 pi x / p), cos(2 pi x / p))``, the others ``x``.  The log-density is differentiable all the same
(``stheno_amd/autograd.py``): the kernel matrix is built group by group into one buffer and factorised in place; the backward reduces
the one cotangent of ``K`` against each group's term table on that group's mapped inputs, and torch carries the input gradient of the
periodic group through the map to the period.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, B, Linear, Measure

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device("cuda")
dt = torch.float64
B.epsilon = 1e-8
true_period, true_noise = 2.0, 0.04

# a signal with a known decomposition
gen = torch.Generator().manual_seed(0)
x = (torch.rand(n, generator=gen, dtype=dt) * 10.0).sort().values.to(dev)
truth = [torch.sin(0.6 * x), 0.8 * torch.sin(2.0 * torch.pi * x / true_period), 0.3 * x]
truth = [t[:, None] for t in truth]
y = sum(truth) + true_noise**0.5 * torch.randn(n, 1, generator=gen, dtype=dt).to(dev)

start = dict(v1=1.0, l=2.0, v2=1.0, p=1.15 * true_period, v3=0.1, noise=0.1)        # (the period starts 15 % off)
raw = {k: torch.tensor(v, dtype=dt).log().requires_grad_(True) for k, v in start.items()}
opt = torch.optim.Adam(list(raw.values()), lr=5e-2)


def model(q):
    with Measure() as prior:
        f_trend = GP(q["v1"] * EQ().stretch(q["l"]))
        f_seasonal = GP(q["v2"] * EQ().periodic(q["p"]))
        f_line = GP(q["v3"] * Linear())
        f = f_trend + f_seasonal + f_line
    return prior, f, (f_trend, f_seasonal, f_line)


t0 = time.perf_counter()
for it in range(iters + 1):
    opt.zero_grad()
    q = {k: v.exp() for k, v in raw.items()}
    _, f, _ = model(q)
    loss = -f(x, q["noise"]).logpdf(y) / n
    loss.backward()
    opt.step()
    if it % max(iters // 5, 1) == 0:
        print(f"iter {it:4d}  -logpdf/N {float(loss.detach()):+.5f}  period {float(q['p'].detach()):.4f}  "
              f"noise {float(q['noise'].detach()):.4f}", flush=True)
torch.cuda.synchronize()
q = {k: v.detach().exp() for k, v in raw.items()}
print(f"N = {n}: {iters + 1} iterations in {time.perf_counter() - t0:.2f} s")
print(f"learnt period {float(q['p']):.4f}   (generating: {true_period})")
print(f"learnt noise  {float(q['noise']):.4f}   (generating: {true_noise})")

# the components under the learnt hyper-parameters: every posterior shares the one factor of the sum's kernel matrix
with torch.no_grad():
    prior, f, parts = model(q)
    post = prior | (f(x, q["noise"]), y)
    for name, p, t in zip(("trend", "seasonal", "line"), parts, truth):
        mean, var = post(p)(x).marginals()
        mean, var = mean.reshape(-1), var.reshape(-1)
        # (the trend and the line are identified only up to what the other can absorb; their sum is)
        rmse = (t[:, 0] - mean).pow(2).mean().sqrt()
        print(f"{name:9s} rmse {float(rmse):.4f}  mean posterior sd {float(var.clamp_min(0).sqrt().mean()):.4f}")
    total = sum(post(p)(x).mean.reshape(-1) for p in parts)
    resid = (sum(truth)[:, 0] - total).pow(2).mean().sqrt()
    print(f"sum of the components against the noise-free signal: rmse {float(resid):.4f}")
