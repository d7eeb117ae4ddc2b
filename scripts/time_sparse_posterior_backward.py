"""Forward / backward times of the pseudo-point posterior marginals under learnable quantities at cfg5's shape (VFE, EQ, N = 200000,
D = 8, M = 4096, fp32, N* = 2048; the jitter at the fp32 setting 1e-6), for three losses -- the mean only, the marginal variances only,
UCB -- with the variance, the length scale and the noise learnable; then UCB with ``xs`` alone, and the additional cost of ``d/dz`` and of
``d/dx`` on top of the hyper-parameters.  Each case reports ``torch.cuda.max_memory_allocated`` over one forward + backward.

    python scripts/time_sparse_posterior_backward.py [N] [M] [N*]

Prints one JSON line.  ``forward_ms`` is conditioning + prediction (a new model every step, as in a learning loop: the M x N work of
``PseudoObs`` is part of it), ``predict_ms`` the prediction alone on a conditioned model.  Every timing is the median of five repetitions
after one warm-up, bracketed by device events."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
ns = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
d = 8
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
x0 = torch.randn(n, d, generator=g, dtype=torch.float32).to(dev)
y = torch.randn(n, 1, generator=g, dtype=torch.float32).to(dev)
z0 = torch.randn(m, d, generator=torch.Generator().manual_seed(2), dtype=torch.float32).to(dev)
xs0 = torch.randn(ns, d, generator=torch.Generator().manual_seed(1), dtype=torch.float32).to(dev)
st.B.epsilon = 1e-6


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def case(loss, leaves):
    """``leaves``: which of "hyper", "xs", "z", "x" require a gradient."""
    hyper = "hyper" in leaves
    lv = torch.zeros((), dtype=torch.float64, requires_grad=hyper)
    ls = torch.zeros((), dtype=torch.float64, requires_grad=hyper)         # (cfg5: unit variance, unit length scale)
    ln = torch.tensor(np.log(0.1), dtype=torch.float32, device=dev, requires_grad=hyper)
    xs = xs0.clone().requires_grad_("xs" in leaves)
    z = z0.clone().requires_grad_("z" in leaves)
    x = x0.clone().requires_grad_("x" in leaves)
    state = {}

    def condition():
        f = st.GP(torch.exp(lv) * st.EQ().stretch(torch.exp(ls)))
        state["post"] = f | st.PseudoObs(f(z), f(x, torch.exp(ln)), y)
        state["post"](xs0[:1]).mean                       # (the rules are lazy: conditioning happens at the first look-up)

    def predict():
        fdd = state["post"](xs)
        if loss == "mean":
            state["l"] = fdd.mean.sum()
        elif loss == "var":
            state["l"] = fdd.var_diag.sum()
        else:
            mean, var = fdd.marginals()
            state["l"] = (mean + 2.0 * torch.sqrt(var)).sum()

    def forward():
        condition()
        predict()

    def backward():
        state["l"].backward()

    forward()
    backward()                                            # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fwd, pred, bwd = [], [], []
    for _ in range(5):
        fwd.append(timed(forward))
        pred.append(timed(predict))
        bwd.append(timed(backward))
    return {"forward_ms": round(float(np.median(fwd)), 3), "predict_ms": round(float(np.median(pred)), 3),
            "backward_ms": round(float(np.median(bwd)), 3), "peak_mib": round(torch.cuda.max_memory_allocated() / 2**20, 1)}


res = {"n": n, "m": m, "ns": ns, "dtype": "float32", "kernel": f"EQ, D = {d}", "method": "vfe"}
for loss in ("mean", "var", "ucb"):
    res[loss] = case(loss, ("hyper",))
res["ucb_xs_only"] = case("ucb", ("xs",))
res["ucb_hyper_z"] = case("ucb", ("hyper", "z"))
res["ucb_hyper_x"] = case("ucb", ("hyper", "x"))
res["extra_dz_ms"] = round(res["ucb_hyper_z"]["backward_ms"] - res["ucb"]["backward_ms"], 3)
res["extra_dx_ms"] = round(res["ucb_hyper_x"]["backward_ms"] - res["ucb"]["backward_ms"], 3)
print(json.dumps(res), flush=True)
