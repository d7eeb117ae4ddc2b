"""Learning an additive model over input dimensions -- ``y = f1(x[:, 0]) + f2(x[:, 1:]) + noise`` -- with ``select``, then predicting
each component.

    python examples/learn_additive_dimensions.py [N] [iterations]

The sum's kernel ``v1 * EQ().stretch(l1).select(0) + v2 * Matern52().stretch(l2).select([1, 2])`` is two groups of terms behind two
input maps: each group sees its own columns of ``x``.  The kernel matrix is built group by group into one buffer (one fused launch
each) and factorised in place; the backward reduces the one cotangent of ``K`` against each group's term table on that group's columns.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, B, Matern52, Measure

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 150
dev = torch.device("cuda")
dt = torch.float64
B.epsilon = 1e-8
true_noise = 0.05

gen = torch.Generator().manual_seed(0)
x = (torch.rand(n, 3, generator=gen, dtype=dt) * 4.0 - 2.0).to(dev)
truth = [torch.sin(2.0 * x[:, :1]), 0.7 * torch.cos(x[:, 1:2] + 0.5 * x[:, 2:3])]
y = sum(truth) + true_noise**0.5 * torch.randn(n, 1, generator=gen, dtype=dt).to(dev)

start = dict(v1=1.0, l1=1.0, v2=1.0, l2=1.0, noise=0.2)
raw = {k: torch.tensor(v, dtype=dt).log().requires_grad_(True) for k, v in start.items()}
opt = torch.optim.Adam(list(raw.values()), lr=5e-2)


def model(q):
    with Measure() as prior:
        f1 = GP(q["v1"] * EQ().stretch(q["l1"])).select(0)
        f2 = GP(q["v2"] * Matern52().stretch(q["l2"])).select(1, 2)
        f = f1 + f2
    return prior, f, (f1, f2)


t0 = time.perf_counter()
for it in range(iters + 1):
    opt.zero_grad()
    q = {k: v.exp() for k, v in raw.items()}
    _, f, _ = model(q)
    loss = -f(x, q["noise"]).logpdf(y) / n
    loss.backward()
    opt.step()
    if it % max(iters // 5, 1) == 0:
        print(f"iter {it:4d}  -logpdf/N {float(loss.detach()):+.5f}  l1 {float(q['l1'].detach()):.3f}  l2 {float(q['l2'].detach()):.3f}  "
              f"noise {float(q['noise'].detach()):.4f}", flush=True)
torch.cuda.synchronize()
q = {k: v.detach().exp() for k, v in raw.items()}
print(f"N = {n}: {iters + 1} iterations in {time.perf_counter() - t0:.2f} s")
print(f"learnt noise {float(q['noise']):.4f}   (generating: {true_noise})")

# the components under the learnt hyper-parameters: both posteriors share the one factor of the sum's kernel matrix
with torch.no_grad():
    prior, f, parts = model(q)
    post = prior | (f(x, q["noise"]), y)
    for name, p, t in zip(("f1(x0)", "f2(x1, x2)"), parts, truth):
        mean, var = post(p)(x).marginals()
        mean, var = mean.reshape(-1), var.reshape(-1)
        # (each component is identified up to a constant the other can absorb: compare after centring)
        err = (t[:, 0] - t.mean()) - (mean - mean.mean())
        print(f"{name:11s} rmse {float(err.pow(2).mean().sqrt()):.4f}  mean posterior sd {float(var.clamp_min(0).sqrt().mean()):.4f}")
