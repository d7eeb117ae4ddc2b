"""One kernel for a batch of small regression tasks, learnt on what it is wanted for: the held-out predictive log-loss of every task at
once -- the counterpart, for posterior predictions, of the batched ``logpdf`` learning.

    python examples/learn_shared_kernel_across_tasks.py [B] [N]

B tasks of N training and N / 4 held-out points each share ``v * EQ().stretch(l)`` and a noise level.  Every step conditions all B
posteriors in one batched launch sequence, evaluates the marginal predictive densities at the held-out inputs and back-propagates
through ``post(xs, noise).marginals()`` (``autograd._BatchedPosteriorMarginals``: one ``gpk_kmat_vjp_dense_batch`` launch per
reduction, whatever B is); the only host work is Adam on three scalars.
"""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, B   # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 64
n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
ns = n // 4
dev, dt = torch.device("cuda"), torch.float32
B.epsilon = 1e-6

g = torch.Generator().manual_seed(0)
freq = 0.6 + 0.8 * torch.rand((nb, 1, 1), generator=g, dtype=dt)             # every task its own function, one smoothness for all
phase = 6.28 * torch.rand((nb, 1, 1), generator=g, dtype=dt)


def task(points):
    x = 8 * torch.rand((nb, points, 1), generator=g, dtype=dt)
    return x.to(dev), (torch.sin(freq * x + phase) + 0.15 * torch.randn((nb, points, 1), generator=g, dtype=dt)).to(dev)


(x, y), (xs, ys) = task(n), task(ns)

log_var = torch.zeros((), requires_grad=True)
log_scale = torch.tensor(-1.0, requires_grad=True)
log_noise = torch.tensor(-1.0, requires_grad=True)
opt = torch.optim.Adam([log_var, log_scale, log_noise], lr=5e-2)


def held_out_log_loss():
    f = GP(log_var.exp() * EQ().stretch(log_scale.exp()))
    noise = log_noise.exp().to(device=dev, dtype=dt)
    mean, var = (f | (f(x, noise), y))(xs, noise).marginals()               # (B, N*) each: the predictive marginals of every task
    mean, var = mean.reshape(nb, ns), var.reshape(nb, ns)
    return 0.5 * (torch.log(2 * math.pi * var) + (ys[..., 0] - mean) ** 2 / var).mean()


t0 = time.perf_counter()
for it in range(41):
    opt.zero_grad()
    loss = held_out_log_loss()
    loss.backward()
    opt.step()
    if it in (0, 40):
        print(f"step {it:2d}  held-out log-loss per point {float(loss.detach()):+.4f}  variance {float(log_var.detach().exp()):.3f}  "
              f"scale {float(log_scale.detach().exp()):.3f}  noise {float(log_noise.detach().exp()):.4f}", flush=True)
torch.cuda.synchronize()
print(f"{nb} tasks x (N = {n}, N* = {ns}): 41 steps in {time.perf_counter() - t0:.2f} s")
