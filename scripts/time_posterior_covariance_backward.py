"""Forward / backward times of the JOINT posterior covariance under learnable quantities (``post(xs, noise)``: a sample loss with
fixed draws, an entropy loss), beside the marginal-variance backward of the same run, the ``gpk_potrf_vjp`` launch alone at n = 2048
and the peak memory of each case.  EQ, D = 8, fp64; default shape cfg2's (N = 16384, N* = 2048).

    python scripts/time_posterior_covariance_backward.py [N] [N*] [out.json]

Prints one JSON line (and writes it to ``out.json`` when given).  Every timing is the median of five repetitions after one warm-up,
bracketed by device events; records, no thresholds."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402
from stheno_amd.matrix import Chol  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
dev = torch.device("cuda")
rng = np.random.default_rng(0)
x = torch.tensor(rng.standard_normal((n, 8)), device=dev)
y = torch.tensor(rng.standard_normal((n, 1)), device=dev)
xs0 = rng.standard_normal((ns, 8))
xi = torch.tensor(rng.standard_normal((ns, 4)), device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def case(loss):
    lv = torch.zeros((), dtype=torch.float64, requires_grad=True)
    ls = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    xs = torch.tensor(xs0, device=dev, requires_grad=True)
    state = {}

    def forward():
        f = st.GP(torch.exp(lv) * st.EQ().stretch(torch.exp(ls)))
        fdd = (f | (f(x, 0.1), y))(xs, 0.05)
        if loss == "marginal_variance":
            state["l"] = fdd.var_diag.sum()
        elif loss == "sample":
            s = fdd.sample(xi=xi)
            state["l"] = (s * s).sum()
        else:
            state["l"] = fdd.entropy()

    forward()
    state["l"].backward()                                # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fwd, bwd = [], []
    for _ in range(5):
        fwd.append(timed(forward))
        bwd.append(timed(lambda: state["l"].backward()))
    return {"forward_ms": round(float(np.median(fwd)), 3), "backward_ms": round(float(np.median(bwd)), 3),
            "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}


res = {"n": n, "ns": ns, "dtype": "float64", "kernel": "EQ, D = 8", "gpk_version": int(st.ops.get_backend().lib.gpk_version())}
for loss in ("marginal_variance", "sample", "entropy"):
    res[loss] = case(loss)
    torch.cuda.empty_cache()

# the Cholesky VJP alone, n = 2048
m = 2048
a = torch.randn((m, m + 8), dtype=torch.float64, device=dev) / (m + 8) ** 0.5
chol = Chol.factor_(a @ a.T + 0.5 * torch.eye(m, dtype=torch.float64, device=dev))
lbar = torch.randn((m, m), dtype=torch.float64, device=dev)
chol.potrf_vjp(lbar)
torch.cuda.synchronize()
res["potrf_vjp_n2048_ms"] = round(float(np.median([timed(lambda: chol.potrf_vjp(lbar)) for _ in range(5)])), 3)
line = json.dumps(res)
print(line, flush=True)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as fh:
        fh.write(line + "\n")
