"""Forward / backward times of ``logpdf`` under a kernel whose terms sit behind DIFFERENT input maps, beside the single-group path.

    python scripts/time_map_groups_backward.py [N]

N = 16384, D = 1, fp64.  The kernel is the trend + seasonal + line model of ``examples/learn_decomposition.py`` with a second seasonal
part, so that it has three groups: ``v1 EQ.stretch(l) + v3 Linear`` (inputs as they are), ``v2 EQ.periodic(p)`` and
``v4 EQ.periodic(p2)``.  Three cases: every hyper-parameter learnable (the periods too: the explicit cotangent, one
``gpk_kmat_vjp_dense`` pass per group with the input gradient), variances and scalar scales only (one ``gpk_kmat_vjp`` pass per group),
and a single ``v EQ.stretch(l)`` group -- the path every sum of primitives takes.  An extra group costs one O(N^2) kernel-matrix launch
forward and one O(N^2) reduction backward beside the O(N^3) factorisation and inverse.

Prints one JSON line.  Every timing is the median of five repetitions after one warm-up, bracketed by device events."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
dev = torch.device("cuda")
rng = np.random.default_rng(0)
x = torch.tensor(np.sort(rng.uniform(0.0, 50.0, (n, 1)), axis=0), device=dev)
y = torch.tensor(rng.standard_normal((n, 1)), device=dev)


def case(groups, learn_maps):
    def leaf(v, grad=True):
        return torch.tensor(v, dtype=torch.float64, requires_grad=grad)

    v1, l, v2, v3, v4 = leaf(1.0), leaf(2.0), leaf(0.7), leaf(0.1), leaf(0.4)
    p, p2 = leaf(2.0, learn_maps), leaf(7.0, learn_maps)
    state = {}

    def forward():
        k = v1 * st.EQ().stretch(l)
        if groups == 3:
            k = k + v3 * st.Linear() + v2 * st.EQ().periodic(p) + v4 * st.EQ().periodic(p2)
        state["l"] = st.GP(k)(x, 0.1).logpdf(y)

    def both():
        forward()
        state["l"].backward()

    both()                                                       # warm-up
    torch.cuda.synchronize()
    fwd, bwd = [], []
    for _ in range(5):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        forward()
        b.record()
        state["l"].backward()
        c.record()
        torch.cuda.synchronize()
        fwd.append(a.elapsed_time(b))
        bwd.append(b.elapsed_time(c))
    return {"forward_ms": round(float(np.median(fwd)), 3), "backward_ms": round(float(np.median(bwd)), 3)}


res = {"n": n, "d": 1, "dtype": "float64",
       "three_groups_learnable_maps": case(3, True),
       "three_groups_fixed_maps": case(3, False),
       "one_group_eq": case(1, False)}
print(json.dumps(res), flush=True)
