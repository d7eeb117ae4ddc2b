"""Learning the lag between two sensors: ``g = f.shift(tau)`` -- the second sensor sees the signal ``tau`` later -- with both observed
through noise, and ``tau``, the variance and the length scale learnt from the joint log-density.

    python examples/learn_lag.py [N per sensor] [iterations]

The cross-covariance of ``g`` with ``f`` is ``k(x - tau, y)``: the kernel behind one map per argument.  The joint matrix of the two
sensors is assembled block by block in one buffer and factorised in place; the backward hands the shifted inputs their gradient from
every block they enter, and torch carries it through ``x - tau`` to the lag.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, B, Measure

n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 150
dev = torch.device("cuda")
dt = torch.float64
B.epsilon = 1e-8
true_lag, noise_a, noise_b = 0.7, 0.02, 0.05


def signal(t):
    return torch.sin(1.3 * t) + 0.5 * torch.sin(3.1 * t + 0.4)


gen = torch.Generator().manual_seed(0)
xa = (torch.rand(n, generator=gen, dtype=dt) * 12.0).sort().values
xb = (torch.rand(n, generator=gen, dtype=dt) * 12.0).sort().values
ya = (signal(xa) + noise_a**0.5 * torch.randn(n, generator=gen, dtype=dt))[:, None].to(dev)
yb = (signal(xb - true_lag) + noise_b**0.5 * torch.randn(n, generator=gen, dtype=dt))[:, None].to(dev)
xa, xb = xa.to(dev), xb.to(dev)

log_v = torch.tensor(1.0, dtype=dt).log().requires_grad_(True)
log_s = torch.tensor(1.0, dtype=dt).log().requires_grad_(True)
tau = torch.tensor(0.2, dtype=dt, requires_grad=True)
opt = torch.optim.Adam([log_v, log_s, tau], lr=3e-2)


def model():
    with Measure() as prior:
        f = GP(log_v.exp() * EQ().stretch(log_s.exp()))
        g = f.shift(tau)
    return prior, f, g


t0 = time.perf_counter()
for it in range(iters + 1):
    opt.zero_grad()
    prior, f, g = model()
    loss = -prior.logpdf((f(xa, noise_a), ya), (g(xb, noise_b), yb)) / (2 * n)
    loss.backward()
    opt.step()
    if it % max(iters // 5, 1) == 0:
        print(f"iter {it:4d}  -logpdf/N {float(loss.detach()):+.5f}  lag {float(tau.detach()):.4f}  "
              f"variance {float(log_v.detach().exp()):.3f}  scale {float(log_s.detach().exp()):.3f}", flush=True)
torch.cuda.synchronize()
print(f"N = 2 x {n}: {iters + 1} iterations in {time.perf_counter() - t0:.2f} s")
print(f"learnt lag {float(tau.detach()):.4f}   (generating: {true_lag})")
print(f"learnt variance {float(log_v.detach().exp()):.3f}, length scale {float(log_s.detach().exp()):.3f}")

# the first sensor's signal from the second sensor alone, under the learnt lag
with torch.no_grad():
    prior, f, g = model()
    mean = (f | (g(xb, noise_b), yb))(xa).mean.reshape(-1)
    print(f"f from the lagged sensor alone: rmse {float((mean - signal(xa)).pow(2).mean().sqrt()):.4f}")
