"""Derivative observations: fit a function from a few values PLUS slopes, then predict the function and its slope with error bars --
``f.diff()`` of the reference (``stheno/model/gp.py:218``), written against ``stheno_amd.torch``.

    python examples/derivative_observations.py [N_VALUES [N_SLOPES]]

``df = f.diff()`` is a process of the same measure, jointly Gaussian with ``f``: it is observed like any other process
(``(df(x), slopes)``), and ``post(df)`` is the posterior of the slope.  Every block of the joint covariance -- ``cov(f, f)``,
``cov(df, f)``, ``cov(df, df)`` -- is one fused launch (``gpk_kmat`` / ``gpk_kmat_diff``) written straight into the matrix that is then
factorised in place.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, Measure

n_val = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n_slope = int(sys.argv[2]) if len(sys.argv) > 2 else 12
dev = torch.device("cuda")
dt = torch.float64
gen = torch.Generator().manual_seed(0)


def truth(x):
    return torch.sin(2.0 * x) + 0.3 * x


def slope(x):
    return 2.0 * torch.cos(2.0 * x) + 0.3


x_val = torch.linspace(0.0, 5.0, n_val, dtype=dt)
x_slope = torch.linspace(0.2, 4.8, n_slope, dtype=dt)
y_val = (truth(x_val) + 0.05 * torch.randn(n_val, generator=gen, dtype=dt)).to(dev)
y_slope = (slope(x_slope) + 0.10 * torch.randn(n_slope, generator=gen, dtype=dt)).to(dev)
x_val, x_slope = x_val.to(dev), x_slope.to(dev)
x_new = torch.linspace(0.0, 5.0, 11, dtype=dt, device=dev)

with Measure() as prior:
    f = GP(2.0 * EQ().stretch(0.8))
    df = f.diff()

with torch.no_grad():
    post_values_only = prior | (f(x_val, 0.05**2), y_val)
    post = prior | ((f(x_val, 0.05**2), y_val), (df(x_slope, 0.10**2), y_slope))
    lp = prior.logpdf((f(x_val, 0.05**2), y_val), (df(x_slope, 0.10**2), y_slope))
    m0, v0 = post_values_only(f)(x_new).marginals()
    mf, vf = post(f)(x_new).marginals()
    md, vd = post(df)(x_new).marginals()

print(f"{n_val} values and {n_slope} slopes; joint log-density {float(lp):.3f}")
print("    x    truth   f | values          f | values + slopes    slope   df | values + slopes")
for i in range(x_new.shape[0]):
    xi = x_new[i].cpu()
    print(f"{float(xi):5.2f}  {float(truth(xi)):7.3f}  {float(m0[i]):7.3f} +- {2 * float(v0[i].clamp_min(0).sqrt()):5.3f}"
          f"  {float(mf[i]):7.3f} +- {2 * float(vf[i].clamp_min(0).sqrt()):5.3f}"
          f"   {float(slope(xi)):7.3f}  {float(md[i]):7.3f} +- {2 * float(vd[i].clamp_min(0).sqrt()):5.3f}")
err0 = float((m0.cpu().ravel() - truth(x_new.cpu())).abs().max())
err1 = float((mf.cpu().ravel() - truth(x_new.cpu())).abs().max())
print(f"largest error of the mean: {err0:.3f} from the values alone, {err1:.3f} with the slopes")
