"""A deep kernel: ``EQ().transform(net)`` with a small ``torch.nn`` feature map (3 -> 4 -> 2, ``tanh``), its weights learnt with the
variance and the noise through ``logpdf``.

    python examples/deep_kernel.py [N] [iterations]

The network runs in torch in front of the fused kernel-matrix launch -- O(N D) next to the O(N^3) factorisation -- and the backward
hands it the gradient of the log-density with respect to the features (``gpk_kmat_vjp_dense``), which torch carries to the weights.
The target depends on the inputs through one direction only, which an isotropic ``EQ`` on the raw inputs cannot exploit.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, B

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device("cuda")
dt = torch.float64
B.epsilon = 1e-8
true_noise = 0.02

gen = torch.Generator().manual_seed(0)
x = torch.rand(n + 200, 3, generator=gen, dtype=dt) * 4.0 - 2.0
u = x @ torch.tensor([1.0, -0.7, 0.4], dtype=dt)
y = (torch.sign(u) * u.abs().sqrt() + true_noise**0.5 * torch.randn(n + 200, generator=gen, dtype=dt))[:, None]
x, y, xt, yt = x[:n].to(dev), y[:n].to(dev), x[n:].to(dev), y[n:].to(dev)

torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Tanh(), torch.nn.Linear(4, 2, bias=False)).to(device=dev, dtype=dt)
raw = {k: torch.tensor(v, dtype=dt).log().requires_grad_(True) for k, v in dict(v=1.0, noise=0.1).items()}
opt = torch.optim.Adam(list(raw.values()) + list(net.parameters()), lr=3e-2)


def rmse(f, noise):
    with torch.no_grad():
        mean = (f | (f(x, noise), y))(xt).mean
        return float((mean - yt).pow(2).mean().sqrt())


with torch.no_grad():
    plain = GP(EQ())
    print(f"EQ on the raw inputs, noise {true_noise}: held-out rmse {rmse(plain, true_noise):.4f}")

t0 = time.perf_counter()
for it in range(iters + 1):
    opt.zero_grad()
    q = {k: v.exp() for k, v in raw.items()}
    f = GP(q["v"] * EQ().transform(net))
    loss = -f(x, q["noise"]).logpdf(y) / n
    loss.backward()
    opt.step()
    if it % max(iters // 5, 1) == 0:
        print(f"iter {it:4d}  -logpdf/N {float(loss.detach()):+.5f}  noise {float(q['noise'].detach()):.4f}", flush=True)
torch.cuda.synchronize()
q = {k: v.detach().exp() for k, v in raw.items()}
print(f"N = {n}: {iters + 1} iterations in {time.perf_counter() - t0:.2f} s")
print(f"learnt noise {float(q['noise']):.4f}   (generating: {true_noise})")
print(f"deep kernel: held-out rmse {rmse(GP(q['v'] * EQ().transform(net)), q['noise']):.4f}")
