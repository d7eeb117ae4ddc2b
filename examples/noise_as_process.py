"""Noise as a process of its own: ``y = f + e`` with ``e = GP(v * Delta())`` -- the reference's idiom for observation noise, written
against ``stheno_amd.torch``.

    python examples/noise_as_process.py [N]

The noise variance is the variance of a kernel term like any other, so it is learnt through the same differentiable log-density as
the length scale; after conditioning on ``y(x)``, ``post(f)`` is the latent function and ``post(y)`` the noisy prediction.  ``Delta``
is a term kind of the fused kernel-matrix kernels: ``EQ + v * Delta`` is one launch.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, Delta, Measure

n = int(sys.argv[1]) if len(sys.argv) > 1 else 500
dev = torch.device("cuda")
dt = torch.float64

x = torch.linspace(0.0, 10.0, n, dtype=dt, device=dev)
gen = torch.Generator().manual_seed(0)
truth = torch.sin(x)[:, None]
obs = truth + 0.2 * torch.randn(n, 1, generator=gen, dtype=dt).to(dev)

log_v = torch.tensor(0.0, dtype=dt, requires_grad=True)        # log of the noise variance
log_l = torch.tensor(0.0, dtype=dt, requires_grad=True)        # log of the length scale


def model():
    with Measure() as prior:
        f = GP(EQ().stretch(log_l.exp()))
        e = GP(log_v.exp() * Delta())
        y = f + e
    return prior, f, y


opt = torch.optim.Adam([log_v, log_l], lr=0.1)
for step in range(60):
    opt.zero_grad()
    _, _, y = model()
    loss = -y(x).logpdf(obs)
    loss.backward()
    opt.step()
print(f"N = {n}: learnt noise variance {float(log_v.detach().exp()):.4f} (true 0.04), length scale {float(log_l.detach().exp()):.3f}, "
      f"log-evidence {-float(loss.detach()):.2f}")

with torch.no_grad():
    prior, f, y = model()
    post = prior | (y(x), obs)
    xs = ((x[:-1] + x[1:]) / 2)[::5]                                 # between the training inputs: Delta is 0 against all of them
    mean_f, var_f = post(f)(xs).marginals()
    mean_y, var_y = post(y)(xs).marginals()
rmse = (mean_f.reshape(-1) - torch.sin(xs)).pow(2).mean().sqrt()
print(f"latent f: rmse {float(rmse):.4f}, mean sd {float(var_f.clamp_min(0).sqrt().mean()):.4f}; "
      f"noisy y: mean sd {float(var_y.clamp_min(0).sqrt().mean()):.4f} "
      f"(variance larger by {float((var_y - var_f).mean()):.4f} = the noise variance)")
