"""Decomposing a signal into a smooth trend, short-range wiggles, a periodic part and a line -- four processes on one measure,
observed only through their noisy sum (the model of the reference's decomposition example, written against ``stheno_amd.torch``).

    python examples/decompose_signal.py [N]

The sum's kernel is ``EQ + RQ(0.1).stretch(0.5) + EQ().periodic(1.0) + Linear``: four groups of terms behind three different input
maps, evaluated group by group into one buffer by the fused kernel-matrix launch and factorised in place; every component's
posterior then shares that one factor.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, RQ, Linear, Measure

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda")
dt = torch.float64
noise = 0.05

with Measure() as prior:
    f_smooth = GP(EQ())
    f_wiggly = GP(RQ(1e-1).stretch(0.5))
    f_periodic = GP(EQ().periodic(1.0))
    f_linear = GP(Linear())
    f = f_smooth + f_wiggly + f_periodic + f_linear

# a signal with a known decomposition: a slow trend, short-range wiggles, a part of period one and a line
x = torch.linspace(0.0, 10.0, n, dtype=dt, device=dev)
gen = torch.Generator().manual_seed(0)
truth = [
    torch.sin(0.7 * x) + 0.5 * torch.cos(0.3 * x + 1.0),
    0.3 * torch.sin(6.1 * x + 0.4) * torch.exp(-0.5 * (x - 4.0) ** 2),
    0.8 * torch.cos(2.0 * torch.pi * x) + 0.4 * torch.sin(4.0 * torch.pi * x),
    0.3 * x - 1.0,
]
truth = [t[:, None] for t in truth]
y = sum(truth) + noise**0.5 * torch.randn(n, 1, generator=gen, dtype=dt).to(dev)

post = prior | (f(x, noise), y)
print(f"N = {n}: log-evidence of the sum {float(f(x, noise).logpdf(y)):.3f}")
total = 0.0
for name, p, t in zip(("smooth", "wiggly", "periodic", "linear"), (f_smooth, f_wiggly, f_periodic, f_linear), truth):
    mean, var = post(p)(x).marginals()
    mean, var = mean.reshape(-1), var.reshape(-1)
    inside = ((t[:, 0] - mean).abs() <= 2.0 * var.clamp_min(0).sqrt() + 1e-9).double().mean()
    rmse = (t[:, 0] - mean).pow(2).mean().sqrt()
    total = total + mean
    print(f"{name:9s} rmse {float(rmse):.4f}  mean posterior sd {float(var.clamp_min(0).sqrt().mean()):.4f}  "
          f"truth within two sd at {100 * float(inside):.1f} % of the inputs")
sum_mean = post(f)(x).mean.reshape(-1)
print(f"components add up to the posterior of the sum: max deviation {float((total - sum_mean).abs().max()):.2e}")
