"""B restarts of hyper-parameter learning on one data set, in ONE batch: every restart has its own variance, length scale and noise
-- hyper-parameters given once per batch entry, as tensors of shape ``(B, 1, 1)`` -- and starts from its own initial length scale.

    python examples/learn_restarts.py [B] [N]

The data are shared: ``x.expand(B, N, 1)`` is a view with batch stride 0, nothing is copied.  One objective evaluation is one batched
launch sequence (kernel matrices of all restarts in one ``gpk_kmat_batch_terms`` launch, the batched factorisation, the solves); the
backward walks the batch and leaves restart b's gradient at index b of every per-batch parameter.  Adam sees ``B`` independent
problems in one tensor per hyper-parameter; the best restart is printed at the end.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, B as backend

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 16
n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
dev = torch.device("cuda")
dt = torch.float32
backend.epsilon = 1e-6           # the jitter the reference advises for fp32

g = torch.Generator().manual_seed(0)
x = (torch.rand(n, 1, generator=g, dtype=dt) * 10).to(dev)
y = torch.sin(x) + 0.3 * torch.cos(3 * x) + 0.2 * torch.randn(n, 1, generator=g, dtype=dt).to(dev)
xb = x.expand(nb, n, 1)                                          # shared by the restarts: batch stride 0, no copy
yb = y.expand(nb, n, 1).contiguous()

# one leaf per hyper-parameter, one entry per restart; the initial length scales are spread over two decades
log_var = torch.zeros((nb, 1, 1), dtype=dt, device=dev, requires_grad=True)
log_scale = torch.linspace(-2.3, 2.3, nb, dtype=dt, device=dev).reshape(nb, 1, 1).requires_grad_()
log_noise = torch.full((nb, 1), -1.0, dtype=dt, device=dev, requires_grad=True)
opt = torch.optim.Adam([log_var, log_scale, log_noise], lr=5e-2)


def objective():
    f = GP(log_var.exp() * EQ().stretch(log_scale.exp()))
    return -f(xb, log_noise.exp().expand(nb, n)).logpdf(yb) / n      # (B,): one objective per restart


t0 = time.perf_counter()
for it in range(101):
    opt.zero_grad()
    losses = objective()
    losses.sum().backward()                                          # restart b's gradient lands at index b of every leaf
    opt.step()
    if it % 20 == 0:
        best = int(losses.detach().argmin())
        print(f"iter {it:3d}  objective/N: best {float(losses.detach()[best]):+.5f} (restart {best}), worst {float(losses.detach().max()):+.5f}", flush=True)
torch.cuda.synchronize()
losses = objective().detach()
best = int(losses.argmin())
print(f"{nb} restarts x N={n}: 101 iterations in {time.perf_counter() - t0:.2f} s")
print(f"best restart {best} (initial scale {float(torch.linspace(-2.3, 2.3, nb)[best].exp()):.3f}): objective/N {float(losses[best]):+.5f}  "
      f"variance {float(log_var.detach()[best].exp()):.3f}  scale {float(log_scale.detach()[best].exp()):.3f}  "
      f"noise {float(log_noise.detach()[best].exp()):.4f}")
