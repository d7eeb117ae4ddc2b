"""Learn hyper-parameters from a predictive loss when values AND slopes are observed: the kernel's variance and length scale and
both noise levels are fitted by Adam on the held-out predictive log-loss of ``post(f)`` and ``post(df)`` -- gradients through a
posterior across processes (``autograd._BlockPosteriorMarginals``: the derivative blocks are reduced by ``gpk_kmat_diff_vjp``).

    python examples/learn_slope_predictions.py [STEPS]

``df = f.diff()`` is a process of the same measure; the training set holds a few values and more slopes, the held-out set values and
slopes at other inputs.  Every step conditions the prior on the training set and scores the held-out set under the posterior
marginals of ``f`` and of ``df``.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, Measure

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
dev = torch.device("cuda")
dt = torch.float64
gen = torch.Generator().manual_seed(0)


def truth(x):
    return torch.sin(2.0 * x) + 0.3 * x


def slope(x):
    return 2.0 * torch.cos(2.0 * x) + 0.3


def noisy(fn, x, sd):
    return (fn(x) + sd * torch.randn(x.shape[0], generator=gen, dtype=dt)).to(dev)


x_val, x_slope = torch.linspace(0.0, 5.0, 8, dtype=dt), torch.linspace(0.2, 4.8, 16, dtype=dt)
x_hold_val, x_hold_slope = torch.linspace(0.3, 4.7, 12, dtype=dt), torch.linspace(0.1, 4.9, 12, dtype=dt)
y_val, y_slope = noisy(truth, x_val, 0.05), noisy(slope, x_slope, 0.10)
y_hold_val, y_hold_slope = noisy(truth, x_hold_val, 0.05), noisy(slope, x_hold_slope, 0.10)
x_val, x_slope, x_hold_val, x_hold_slope = (t.to(dev) for t in (x_val, x_slope, x_hold_val, x_hold_slope))

# logarithms of the variance, the length scale and the two noise variances (deliberately far off)
params = [torch.tensor(v, dtype=dt, requires_grad=True) for v in (0.0, math.log(2.5), math.log(0.5), math.log(0.5))]
opt = torch.optim.Adam(params, lr=0.05)


def gaussian_nll(y, mean, var):
    return 0.5 * (torch.log(2 * math.pi * var) + (y - mean) ** 2 / var).sum()


def held_out_loss():
    lv, ll, ln_val, ln_slope = params
    with Measure() as prior:
        f = GP(torch.exp(lv) * EQ().stretch(torch.exp(ll)))
        df = f.diff()
    post = prior | ((f(x_val, torch.exp(ln_val)), y_val), (df(x_slope, torch.exp(ln_slope)), y_slope))
    mf, vf = post(f)(x_hold_val, torch.exp(ln_val)).marginals()
    md, vd = post(df)(x_hold_slope, torch.exp(ln_slope)).marginals()
    return gaussian_nll(y_hold_val, mf.reshape(-1), vf.reshape(-1)) + gaussian_nll(y_hold_slope, md.reshape(-1), vd.reshape(-1))


first = None
for step in range(steps):
    opt.zero_grad()
    loss = held_out_loss()
    loss.backward()
    opt.step()
    first = float(loss.detach()) if first is None else first
    if step % 10 == 0 or step == steps - 1:
        v, l, nv, nd = (float(torch.exp(p.detach())) for p in params)
        print(f"step {step:3d}  held-out loss {float(loss.detach()):9.3f}   variance {v:5.2f}  scale {l:5.2f}  noise sd {nv ** 0.5:5.3f} (values) "
              f"{nd ** 0.5:5.3f} (slopes)")
print(f"held-out loss {first:.3f} -> {float(held_out_loss().detach()):.3f}")
