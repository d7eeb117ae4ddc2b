"""Times of the gradients through BATCHED posterior means and marginal variances (``autograd._BatchedPosteriorMarginals``) beside the
only spelling the parent commit has: the same loss computed entry by entry through the unbatched ``_PosteriorMarginals``.

    python scripts/time_batch_posterior_backward.py [--reps 5] [--shapes big,small]

Shapes: "big" = 512 x (N = 2048, N* = 256, D = 3) in fp32 (``B.epsilon = 1e-6``), "small" = 16 x (N = 512, N* = 64, D = 3) in fp64.
Model: ``v * EQ().stretch(l)`` with leaf ``v``, ``l`` shared by the batch, scalar noise.  Losses: the mean only, the marginal variances
only, and a UCB ``sum(mean + 2 sqrt(var))`` with ``xs.requires_grad_()`` (so ``d/dxs`` is part of the backward).

  (a) per loss: forward (with the graph) and backward of ONE batched evaluation against a walk over the entries, each an unbatched
      evaluation with its own forward and backward; peak memory of either;
  (b) the new launch alone, ``gpk_kmat_vjp_dense_batch`` with ``gradx``, against B calls of ``gpk_kmat_vjp_dense`` on the same
      cotangents: the cross shape (N x N*) and the square one (N x N).

Method: every candidate is warmed up once, then the candidates ALTERNATE for ``--reps`` rounds; forward and backward are bracketed by
device events (the walk: one pair per entry and phase, read after the round's one synchronisation and summed).  Reported: the median
over the rounds and the smallest and largest round (the spread).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402
from stheno_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", default="big,small")
args = ap.parse_args()

assert torch.cuda.is_available(), "a timing needs the GPU: there is no fallback"
dev = torch.device("cuda")
SHAPES = {"big": (512, 2048, 256, 3, torch.float32, 1e-6), "small": (16, 512, 64, 3, torch.float64, 1e-12)}
NOISE = 0.1


def event():
    return torch.cuda.Event(enable_timing=True)


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def loss_of(kind, mean, var):
    if kind == "mean":
        return mean.sum()
    if kind == "var":
        return var.sum()
    return (mean + 2.0 * torch.sqrt(var)).sum()


def leaves(dtype):
    return [torch.tensor(a, dtype=dtype, device=dev, requires_grad=True) for a in (1.3, 0.9)]


def batched(kind, x, y, xs):
    """One batched evaluation: ``(forward ms, backward ms)``."""
    v, l = leaves(x.dtype)
    q = xs.clone().requires_grad_(kind == "ucb")
    e = [event() for _ in range(4)]
    e[0].record()
    f = st.GP(v * st.EQ().stretch(l))
    mean, var = (f | (f(x, NOISE), y))(q).marginals()
    total = loss_of(kind, mean, var)
    e[1].record()
    e[2].record()
    total.backward()
    e[3].record()
    torch.cuda.synchronize()
    assert v.grad is not None and (kind != "ucb" or q.grad is not None)
    return e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3])


def walk(kind, x, y, xs):
    """The same loss entry by entry, each an unbatched evaluation (what the parent commit can do): ``(forward ms, backward ms)``."""
    v, l = leaves(x.dtype)
    q = xs.clone().requires_grad_(kind == "ucb")
    marks = []
    for b in range(x.shape[0]):
        e = [event() for _ in range(4)]
        e[0].record()
        f = st.GP(v * st.EQ().stretch(l))
        mean, var = (f | (f(x[b], NOISE), y[b]))(q[b]).marginals()
        total = loss_of(kind, mean, var)
        e[1].record()
        e[2].record()
        total.backward()
        e[3].record()
        marks.append(e)
    torch.cuda.synchronize()
    return sum(e[0].elapsed_time(e[1]) for e in marks), sum(e[2].elapsed_time(e[3]) for e in marks)


def compare(cands):
    """``cands``: name -> callable returning a tuple of times.  One warm-up each, alternating rounds; per name: stats per time, peak MB."""
    peak = {}
    for name, fn in cands.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    times = {name: [] for name in cands}
    for _ in range(args.reps):
        for name, fn in cands.items():
            times[name].append(fn())
    return times, peak


out = {"reps": args.reps}
for shape in args.shapes.split(","):
    B, n, ns, d, dtype, eps = SHAPES[shape]
    st.B.epsilon = eps
    g = torch.Generator(device="cpu").manual_seed(0)
    x, xs = (torch.randn((B, k, d), generator=g, dtype=dtype).to(dev) for k in (n, ns))
    y = torch.randn((B, n, 1), generator=g, dtype=dtype).to(dev)
    res = {}
    for kind in ("mean", "var", "ucb"):
        times, peak = compare({"batched": lambda: batched(kind, x, y, xs), "walk": lambda: walk(kind, x, y, xs)})
        r = {}
        for name, t in times.items():
            r[name] = {"forward": stats([a for a, _ in t]), "backward": stats([b for _, b in t]), "peak_mb": peak[name]}
        r["backward_batched_over_walk"] = round(r["batched"]["backward"]["median_ms"] / r["walk"]["backward"]["median_ms"], 4)
        r["forward_batched_over_walk"] = round(r["batched"]["forward"]["median_ms"] / r["walk"]["forward"]["median_ms"], 4)
        res[kind] = r
    # (b) the launch alone
    be = ops.get_backend()
    terms = ops.KTerms([("eq", 1.3, 0.9)])
    for name, (y_in, m) in {"cross": (xs, ns), "square": (x, n)}.items():
        cot = torch.randn((B, n, m), dtype=dtype, device=dev)

        def one(fn):
            a, b = event(), event()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            return (a.elapsed_time(b),)

        def loop():
            for e in range(B):
                be.kmat_vjp_dense(terms, x[e], y_in[e], cot[e], want_gradx=True)

        times, _ = compare({"one_launch": lambda: one(lambda: be.kmat_vjp_dense_batch(terms, x, y_in, cot, want_gradx=True)),
                            "b_launches": lambda: one(loop)})
        r = {k: stats([a for (a,) in t]) for k, t in times.items()}
        r["one_over_b"] = round(r["one_launch"]["median_ms"] / r["b_launches"]["median_ms"], 4)
        res["launch_" + name] = r
        del cot
    out[shape] = res
    del x, xs, y
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
