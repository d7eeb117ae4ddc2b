"""Times of the 2-Wasserstein distance ``Normal.w2`` between two kernel-matrix covariances on the same points
(``1.3 EQ(0.9) + 0.1 I`` and ``0.8 EQ(1.7) + 0.5 Linear + 0.2 I``, D = 2, different means), n = 2048 and 4096, fp64 and fp32:

* ``entry_ms``: ``gpk_nuclear_norm`` alone (``HipBackend.nuclear_norm`` on ``M = L_o^T L_s``, default step count) and the TFLOP/s it
  achieves, counting ``3 n^3`` per step;
* ``w2_ms``: the whole ``p.w2(q)`` from two dense covariances -- two factorisations, the GEMM for ``M``, the entry, the traces;
* ``host_eigh_ms``: the same distance by the reference's formula, two dense eigendecompositions (``numpy.linalg.eigh``) in fp64 on the
  host, timed once -- there is no other GPU implementation to compare with;
* ``rel_err``: ``|w2^2 - host w2^2|`` relative to ``|dm|^2 + tr V1 + tr V2``.

    python scripts/time_w2.py [out.json] [n ...]

Prints one JSON line per case (and writes all of them to ``out.json`` when given).  GPU timings are medians of five repetitions after
one warm-up, bracketed by device events; records, no thresholds."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402
from stheno_amd import ops  # noqa: E402

dev = torch.device("cuda")
sizes = [int(a) for a in sys.argv[2:]] or [2048, 4096]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median5(fn):
    fn()
    torch.cuda.synchronize()
    return float(np.median([timed(fn) for _ in range(5)]))


def sym_root(a):
    w, q = np.linalg.eigh(a)
    return (q * np.sqrt(np.clip(w, 0.0, None))) @ q.T


lines = []
for n in sizes:
    rng = np.random.default_rng(n)
    x = rng.uniform(-2.0, 2.0, (n, 2))
    sq = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    v1 = 1.3 * np.exp(-0.5 * sq / 0.9 ** 2) + 0.1 * np.eye(n)
    v2 = 0.8 * np.exp(-0.5 * sq / 1.7 ** 2) + 0.5 * (x @ x.T) + 0.2 * np.eye(n)
    m1, m2 = rng.standard_normal((n, 1)), rng.standard_normal((n, 1)) + 0.3
    t0 = time.perf_counter()
    r = sym_root(v1)
    host = float(((m1 - m2) ** 2).sum() + np.trace(v1) + np.trace(v2) - 2 * np.trace(sym_root(r @ v2 @ r)))
    host_ms = (time.perf_counter() - t0) * 1e3
    scale = float(((m1 - m2) ** 2).sum() + np.trace(v1) + np.trace(v2))
    print(f"# n={n}: host formula {host_ms:.0f} ms", flush=True)
    for dtype in (torch.float64, torch.float32):
        st.B.epsilon = 1e-6 if dtype == torch.float32 else 1e-12
        t = lambda a: torch.as_tensor(a, dtype=dtype, device=dev)      # noqa: E731
        tm1, tv1, tm2, tv2 = t(m1), t(v1), t(m2), t(v2)
        be = ops.get_backend()
        p, q = st.Normal(tm1, tv1), st.Normal(tm2, tv2)
        mat = be.gemm(q.var.chol().lower(), p.var.chol().lower(), a_kmajor=False, b_kmajor=False, tri_k=True)
        iters = ops.NUCLEAR_ITERS_F64 if dtype == torch.float64 else ops.NUCLEAR_ITERS_F32
        entry_ms = median5(lambda: be.nuclear_norm(mat))
        w2_ms = median5(lambda: st.Normal(tm1, tv1).w2(st.Normal(tm2, tv2)))
        got = float(st.Normal(tm1, tv1).w2(st.Normal(tm2, tv2))) ** 2
        res = {"n": n, "dtype": str(dtype).replace("torch.", ""), "iters": iters, "entry_ms": round(entry_ms, 3),
               "entry_tflops": round(3.0 * n ** 3 * iters / (entry_ms * 1e-3) / 1e12, 2), "w2_ms": round(w2_ms, 3),
               "host_eigh_ms": round(host_ms, 1), "rel_err": float(f"{abs(got - host) / scale:.3e}"),
               "gpk_version": int(be.lib.gpk_version())}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del p, q, mat, tm1, tv1, tm2, tv2
        torch.cuda.empty_cache()
st.B.epsilon = 1e-12
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
