"""A network whose amplitude and offset are Gaussian processes: ``f = (1 + a) * net + b`` -- the reference's GP-RNN example with a small
``tanh`` MLP in the place of the RNN, written against ``stheno_amd.torch``.

    python examples/gp_modulated_network.py [N] [STEPS]

``a`` and ``b`` are slowly varying processes with small variances: the network explains the shape of the signal, ``a`` modulates its
amplitude and ``b`` its offset.  Everything is learnt by Adam through ``f(x, noise).logpdf(y)``: the kernel of ``(1 + a) * net`` is
``net(x) k_a(x, y) net(y)``, one launch of the fused kernel with the network's values as row and column factors, and the gradient
reaches the network's parameters through those factors (and through the mean, which is ``net`` itself).  The posteriors of ``f``, ``a``
and ``b`` are then read off the conditioned measure.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

from stheno_amd.torch import EQ, GP, Measure

n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device("cuda")
dt = torch.float64

torch.manual_seed(0)
x = torch.linspace(0.0, 1.0, n, dtype=dt, device=dev)[:, None]
truth = (1.0 + 0.3 * torch.sin(2.0 * x)) * torch.sin(14.0 * x) + 0.3 * x
obs = truth + 0.1 * torch.randn(n, 1, dtype=dt, device=dev)

net = torch.nn.Sequential(torch.nn.Linear(1, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))
net.to(device=dev, dtype=dt)
log_la = torch.tensor(-1.0, dtype=dt, requires_grad=True)      # log length scales of a and b
log_lb = torch.tensor(-1.0, dtype=dt, requires_grad=True)
log_noise = torch.tensor(-3.0, dtype=dt, requires_grad=True)


def model():
    with Measure() as prior:
        a = GP(1e-2 * EQ().stretch(log_la.exp()))
        b = GP(1e-2 * EQ().stretch(log_lb.exp()))
        f = (1 + a) * net + b
    return prior, f, a, b


opt = torch.optim.Adam(list(net.parameters()) + [log_la, log_lb, log_noise], lr=5e-3)
for step in range(steps):
    opt.zero_grad()
    prior, f, a, b = model()
    loss = -f(x, log_noise.exp()).logpdf(obs)
    loss.backward()
    opt.step()
    if step % 50 == 0 or step == steps - 1:
        print(f"step {step:4d}  -logpdf {float(loss.detach()):10.3f}  noise {float(log_noise.exp().detach()):.4f}")

with torch.no_grad():
    prior, f, a, b = model()
    post = prior | (f(x, log_noise.exp()), obs)
    for name, p, ref in (("f", f, truth), ("a", a, None), ("b", b, None)):
        mean, lower, upper = post(p)(x).marginal_credible_bounds()
        line = f"posterior of {name}: mean in [{float(mean.min()):.3f}, {float(mean.max()):.3f}], widest 95% band {float((upper - lower).max()):.3f}"
        if ref is not None:
            line += f", rmse against the truth {float(((mean.reshape(-1) - ref.reshape(-1)) ** 2).mean().sqrt()):.4f}"
        print(line)
