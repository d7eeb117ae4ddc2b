"""Forward / backward times of posterior marginals ACROSS processes under learnable quantities: values and slopes observed together
(N = 8192 + 8192, D = 2, fp64, ``f ~ v EQ().stretch(l) + v2 Matern52()``), ``post(f)`` predicted at N* = 2048 with a UCB loss; the
variance, the length scale and both noises learnable, then the test inputs as well.  And the ``gpk_kmat_diff_vjp`` launch alone (all
three modes) next to ``gpk_kmat_vjp_dense`` on the same 8192 x 8192 cotangent and the same term table.

    python scripts/time_block_posterior_backward.py [N_VALUES] [N_SLOPES] [N*]

Prints one JSON line.  ``forward_ms`` is conditioning + prediction (a new model every step, as in a learning loop).  Every timing is
the median of five repetitions after one warm-up, bracketed by device events."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402
from stheno_amd import ops  # noqa: E402

n1 = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
n2 = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
ns = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
d = 2
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
x1, x2, xs0 = (torch.rand(k, d, generator=g, dtype=torch.float64).mul(6.0).to(dev) for k in (n1, n2, ns))
y1 = (torch.sin(2.0 * x1[:, :1]) * torch.cos(x1[:, 1:]) + 0.1 * torch.randn(n1, 1, generator=g, dtype=torch.float64).to(dev))
y2 = (-torch.sin(2.0 * x2[:, :1]) * torch.sin(x2[:, 1:]) + 0.1 * torch.randn(n2, 1, generator=g, dtype=torch.float64).to(dev))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    return round(float(np.median([timed(fn) for _ in range(reps)])), 3)


def case(leaves):
    hyper = "hyper" in leaves
    lv, ll, ln1, ln2 = (torch.tensor(v, dtype=torch.float64, requires_grad=hyper) for v in (0.2, -0.3, np.log(0.01), np.log(0.02)))
    xs = xs0.clone().requires_grad_("xs" in leaves)
    state = {}

    def forward():
        with st.Measure() as prior:
            f = st.GP(torch.exp(lv) * st.EQ().stretch(torch.exp(ll)) + 0.5 * st.Matern52())
            df = f.diff(1)
        post = prior | ((f(x1, torch.exp(ln1)), y1), (df(x2, torch.exp(ln2)), y2))
        mean, var = post(f)(xs).marginals()
        state["l"] = (mean + 2.0 * torch.sqrt(var)).sum()

    def backward():
        state["l"].backward()

    forward()
    backward()                                            # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fwd, bwd = [], []
    for _ in range(5):
        fwd.append(timed(forward))
        bwd.append(timed(backward))
    return {"forward_ms": round(float(np.median(fwd)), 3), "backward_ms": round(float(np.median(bwd)), 3),
            "peak_mib": round(torch.cuda.max_memory_allocated() / 2**20, 1)}


res = {"n_values": n1, "n_slopes": n2, "ns": ns, "dtype": "float64", "kernel": f"EQ + Matern52, D = {d}"}
res["ucb_hyper"] = case(("hyper",))
res["ucb_hyper_xs"] = case(("hyper", "xs"))

# the launches alone, on the same cotangent
be = ops.get_backend()
terms = ops.KTerms([("eq", 1.2, 0.75), ("matern52", 0.5, 1.0)])
cot = torch.randn(n1, n2, generator=g, dtype=torch.float64).to(dev)
launch = {"n": n1, "m": n2, "cotangent_mib": round(cot.numel() * 8 / 2**20, 1)}
launch["kmat_vjp_dense_ms"] = median(lambda: be.kmat_vjp_dense(terms, x1, x2, cot))
for name, (a, b) in (("dx", (1, None)), ("dy", (None, 1)), ("dxy", (1, 1))):
    launch[f"kmat_diff_vjp_{name}_ms"] = median(lambda: be.kmat_diff_vjp(terms, x1, x2, a, b, cot))
launch["kmat_vjp_dense_gradx_ms"] = median(lambda: be.kmat_vjp_dense(terms, x1, x2, cot, want_gradx=True))
launch["kmat_diff_vjp_dx_gradx_ms"] = median(lambda: be.kmat_diff_vjp(terms, x1, x2, 1, None, cot, want_gradx=True))
res["launch"] = launch
print(json.dumps(res), flush=True)
