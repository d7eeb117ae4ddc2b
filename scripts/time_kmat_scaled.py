"""Times of the kernel-matrix launch with a row and a column factor (``gpk_kmat_scaled``) beside what it replaces and what it must not
disturb.

    python scripts/time_kmat_scaled.py [--parent-lib PATH/libgpk.so] [--reps 9] [--inner 10] [--out FILE.json]

Shapes: N = 16384, D = 8 in fp64 and N = 32768, D = 4 in fp32; the lower triangle with a noise term on the diagonal, as the log-density
builds it.  EQ kernel.

  (a) ``gpk_kmat`` of this library against the PARENT commit's (``--parent-lib``): its code is meant to be unchanged -- the ratio is
      judged against the run-to-run spread (the parent timed twice: ``parent``, ``parent_again``), and the output bits are compared;
  (b) ``gpk_kmat_scaled`` with both scales;
  (c) ``gpk_kmat`` followed by the two multiplications in torch, in place (what (b) replaces: three passes over the matrix);
  (d) the two-group sum ``fn k_a fn + k_b``: one ``gpk_kmat`` and one accumulating ``gpk_kmat_scaled`` into ONE buffer, against the same
      sum through an N x N temporary for the scaled summand -- with the peak device memory of each;
  (e) N = 8192, fp64: forward + backward of ``logpdf`` under ``(1 + a) * net + b`` (the scaled group's explicit-cotangent passes and the
      ``G_r`` buffer) beside the plain two-group sum ``a + b``.

Method: every candidate of a comparison is warmed up, then the candidates ALTERNATE for ``--reps`` rounds; a round times ``--inner``
back-to-back calls between two device events and records the time per call.  Reported: the median over the rounds and the smallest
and largest round.  Prints one JSON line (and writes it to ``--out``)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd as st  # noqa: E402
from stheno_amd import _native, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "a timing needs the GPU: there is no fallback"
dev = torch.device("cuda")
lib = _native.load()
parent = None
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.gpk_kmat.restype, parent.gpk_kmat.argtypes = _native.SIGNATURES["gpk_kmat"]
    parent.gpk_version.restype = ctypes.c_int

ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())      # noqa: E731
NOISE = 0.1


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def plain(which, x, out, scale=1.0, accumulate=0, noise=NOISE):
    """``gpk_kmat`` of library ``which``: EQ, lower triangle, noise on the diagonal; x (n, d), out (n, n)."""
    n, d = x.shape
    kinds, var, ils = (ctypes.c_int * 1)(_native.K_EQ), (ctypes.c_double * 1)(1.0), (ctypes.c_double * 1)(1.0 / scale)
    code = which.gpk_kmat(ops._dtype_id(x), kinds, var, ils, None, 1, ptr(x), n, d, 0, ptr(x), n, d, 0, d, ptr(out), n, 0, 1, 1, 1, noise,
                          None, 0, accumulate, stream())
    assert code == 0, code


def scaled(x, rs, cs, out, accumulate=0, noise=NOISE):
    n, d = x.shape
    kinds, var, ils = (ctypes.c_int * 1)(_native.K_EQ), (ctypes.c_double * 1)(1.0), (ctypes.c_double * 1)(1.0)
    code = lib.gpk_kmat_scaled(ops._dtype_id(x), kinds, var, ils, None, 1, ptr(x), n, d, 0, ptr(x), n, d, 0, d, ptr(rs), 0, ptr(cs), 0,
                               ptr(out), n, 0, 1, 1, 1, noise, None, 0, accumulate, stream())
    assert code == 0, code


def plain_then_torch(x, s, out):
    plain(lib, x, out, noise=0.0)
    out.mul_(s[:, None]).mul_(s[None, :])
    torch.diagonal(out).add_(NOISE)


def sum_fused(x, s, out):
    plain(lib, x, out, scale=2.0)
    scaled(x, s, s, out, accumulate=1, noise=0.0)


def sum_through_temporary(x, s, out):
    plain(lib, x, out, scale=2.0)
    tmp = torch.empty_like(out)
    plain(lib, x, tmp, noise=0.0)
    tmp.mul_(s[:, None]).mul_(s[None, :])
    out.add_(tmp)


def compare(candidates, inner):
    """``candidates``: name -> callable.  Alternating rounds; ms per call: median, min, max."""
    for fn in candidates.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in candidates}
    for _ in range(args.reps):
        for name, fn in candidates.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / inner)
    return {name: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for name, t in times.items()}


def ratio(res, a, b):
    return round(res[a]["median_ms"] / res[b]["median_ms"], 4)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)


out = {"reps": args.reps, "inner": args.inner, "library_version": lib.gpk_version(),
       "parent_version": parent.gpk_version() if parent is not None else None}

for name, (n, d, dtype) in {"n16384_d8_f64": (16384, 8, torch.float64), "n32768_d4_f32": (32768, 4, torch.float32)}.items():
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn((n, d), generator=g, dtype=dtype).to(dev)
    s = torch.randn((n,), generator=g, dtype=dtype).to(dev)
    buf = torch.empty((n, n), dtype=dtype, device=dev)
    cands = {}
    if parent is not None:
        cands["a_kmat_parent"] = lambda: plain(parent, x, buf)
    cands["a_kmat_this_commit"] = lambda: plain(lib, x, buf)
    if parent is not None:
        cands["a_kmat_parent_again"] = lambda: plain(parent, x, buf)
    cands["b_kmat_scaled"] = lambda: scaled(x, s, s, buf)
    cands["c_kmat_then_two_torch_multiplications"] = lambda: plain_then_torch(x, s, buf)
    res = compare(cands, args.inner)
    if parent is not None:
        res["this_commit_over_parent"] = ratio(res, "a_kmat_this_commit", "a_kmat_parent")
        res["parent_again_over_parent"] = ratio(res, "a_kmat_parent_again", "a_kmat_parent")
        ref = torch.empty_like(buf)
        plain(parent, x, ref)
        plain(lib, x, buf)
        torch.cuda.synchronize()
        res["a_outputs_equal"] = bool(torch.equal(torch.tril(ref), torch.tril(buf)))
        del ref
    res["scaled_over_plain"] = ratio(res, "b_kmat_scaled", "a_kmat_this_commit")
    res["scaled_over_plain_then_torch"] = ratio(res, "b_kmat_scaled", "c_kmat_then_two_torch_multiplications")
    sums = compare({"d_sum_fused": lambda: sum_fused(x, s, buf), "d_sum_through_temporary": lambda: sum_through_temporary(x, s, buf)}, max(args.inner // 2, 1))
    sums["fused_over_temporary"] = ratio(sums, "d_sum_fused", "d_sum_through_temporary")
    sums["peak_mib_fused"] = peak_mib(lambda: sum_fused(x, s, buf))
    sums["peak_mib_through_temporary"] = peak_mib(lambda: sum_through_temporary(x, s, buf))
    res.update(sums)
    out[name] = res
    del x, s, buf
    torch.cuda.empty_cache()

# (e): forward + backward of the log-density at N = 8192, fp64
n = 8192
g = torch.Generator(device="cpu").manual_seed(1)
x = torch.rand((n, 1), generator=g, dtype=torch.float64).to(dev)
y = torch.randn((n, 1), generator=g, dtype=torch.float64).to(dev)
net = torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)).to(device=dev, dtype=torch.float64)
l_a = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
l_b = torch.tensor(0.2, dtype=torch.float64, requires_grad=True)


def step(scaled_model):
    with st.Measure():
        a, b = st.GP(1e-2 * st.EQ().stretch(l_a)), st.GP(1e-2 * st.EQ().stretch(l_b))
        f = (1 + a) * net + b if scaled_model else a + b
    f(x, NOISE).logpdf(y).backward()


res = compare({"e_scaled_model_forward_backward": lambda: step(True), "e_plain_two_group_forward_backward": lambda: step(False)}, 1)
res["scaled_over_plain"] = ratio(res, "e_scaled_model_forward_backward", "e_plain_two_group_forward_backward")
out["n8192_f64_logpdf_backward"] = res
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
