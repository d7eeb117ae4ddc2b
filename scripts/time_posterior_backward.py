"""Forward / backward times of the posterior marginals under learnable quantities at cfg2's shape (EQ, N = 16384, D = 8, fp64,
N* = 2048), for three losses -- the mean only, the marginal variances only, UCB with d/dxs -- and an A/B of the transposed solve
``L^{-T} V`` (gpk_trsm_lower_t) against the explicit-inverse route (gpk_trtri_lower + one triangular GEMM).

    python scripts/time_posterior_backward.py [N] [N*]

Prints one JSON line.  Every timing is the median of five repetitions after one warm-up, bracketed by device events."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402
from stheno_amd import ops  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
dev = torch.device("cuda")
rng = np.random.default_rng(0)
x = torch.tensor(rng.standard_normal((n, 8)), device=dev)
y = torch.tensor(rng.standard_normal((n, 1)), device=dev)
xs0 = rng.standard_normal((ns, 8))


def median_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def case(loss):
    lv = torch.zeros((), dtype=torch.float64, requires_grad=True)
    ls = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    xs = torch.tensor(xs0, device=dev, requires_grad=(loss == "ucb"))
    state = {}

    def forward():
        f = st.GP(torch.exp(lv) * st.EQ().stretch(torch.exp(ls)))
        post = f | (f(x, 0.1), y)
        fdd = post(xs)
        if loss == "mean":
            state["l"] = fdd.mean.sum()
        elif loss == "var":
            state["l"] = fdd.var_diag.sum()
        else:
            mean, var = fdd.marginals()
            state["l"] = (mean + 2.0 * torch.sqrt(var)).sum()

    def backward():
        state["l"].backward()

    def both():
        forward()
        backward()

    both()
    t_fwd = median_ms(forward)
    fwd_times, bwd_times = [], []
    for _ in range(5):
        forward()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        backward()
        b.record()
        torch.cuda.synchronize()
        bwd_times.append(a.elapsed_time(b))
    return {"forward_ms": round(t_fwd, 3), "backward_ms": round(float(np.median(bwd_times)), 3)}


res = {"n": n, "ns": ns, "dtype": "float64", "kernel": "EQ, D = 8"}
for loss in ("mean", "var", "ucb"):
    res[loss] = case(loss)

# A/B: L^{-T} V by back-substitution vs by the explicit inverse
be = ops.get_backend()
f = st.GP(st.EQ())
K = f(x, 0.1).var
chol = K.chol()
V = torch.randn((n, ns), dtype=torch.float64, device=dev)
t_trsm = median_ms(lambda: chol.solve_t(V))
sb, dsb = chol._blocks(n)


def via_inverse():
    W = be.trtri(chol.l, dsb, sb)                               # L^{-1}, N^3/3 flops
    return be.gemm(W, V, a_kmajor=False, b_kmajor=False)        # (L^{-1})^T V


t_inv = median_ms(via_inverse)
ref = via_inverse()
err = float((chol.solve_t(V) - ref).abs().max() / ref.abs().max())
res["solve_t_ab"] = {"trsm_lower_t_ms": round(t_trsm, 3), "trtri_plus_gemm_ms": round(t_inv, 3), "max_rel_diff": err}
print(json.dumps(res), flush=True)
