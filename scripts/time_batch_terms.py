"""Times of the kernel-matrix launch with one term table per batch entry (``gpk_kmat_batch_terms``) beside what it replaces and what it
must not disturb.

    python scripts/time_batch_terms.py [--parent-lib PATH/libgpk.so] [--reps 9] [--inner 20]

Shapes: "cfg4" = 512 matrices of N = 2048, D = 3 (the batched benchmark workload), "cfg2" = one matrix of N = 16384, D = 8; the lower
triangle with a noise term on the diagonal, as the log-density builds it.  EQ kernel.

  (a) one per-batch launch against a loop of 512 unbatched ``gpk_kmat`` launches into views of one buffer -- the only spelling of 512
      different parameter sets without the new entry (cfg4, fp32);
  (b) one per-batch launch against the shared-parameter ``gpk_kmat`` launch of the PARENT commit's library (``--parent-lib``; cfg4, fp32);
  (c) the shared-parameter ``gpk_kmat`` of this library against the parent's, fp32 and fp64, cfg2 and cfg4: its code is meant to be
      unchanged;
  (d) the forward ``logpdf`` of the 512-entry model with per-batch parameters beside the shared-parameter one (fp32).

Method: every candidate of a comparison is warmed up, then the candidates ALTERNATE for ``--reps`` rounds; a round times ``--inner``
back-to-back launches between two device events (for (a) and (d): one pass) and records the time per launch.  Reported: the median
over the rounds, and the smallest and largest round (the spread).  The parent library is timed as TWO candidates (``parent``,
``parent_again``): the ratio of those two is the run-to-run spread every other ratio is to be judged against.  Prints one JSON line."""
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
ap.add_argument("--inner", type=int, default=20)
args = ap.parse_args()

assert torch.cuda.is_available(), "a timing needs the GPU: there is no fallback"
dev = torch.device("cuda")
lib = _native.load()
parent = None
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.gpk_kmat.restype, parent.gpk_kmat.argtypes = _native.SIGNATURES["gpk_kmat"]
    parent.gpk_version.restype = ctypes.c_int

ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
NOISE = 0.1


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def shared_launch(which, x, out, variance=1.0, scale=1.0):
    """``gpk_kmat`` of library ``which``: EQ, lower triangle, noise on the diagonal; x (B, n, d), out (B, n, n)."""
    B, n, d = x.shape
    kinds, var, ils = (ctypes.c_int * 1)(_native.K_EQ), (ctypes.c_double * 1)(variance), (ctypes.c_double * 1)(1.0 / scale)
    code = which.gpk_kmat(ops._dtype_id(x), kinds, var, ils, None, 1, ptr(x), n, d, n * d, ptr(x), n, d, n * d, d,
                          ptr(out), n, n * n, B, 1, 1, NOISE, None, 0, 0, stream())
    assert code == 0, code


def batch_launch(x, out, var, ils):
    B, n, d = x.shape
    kinds = (ctypes.c_int * 1)(_native.K_EQ)
    code = lib.gpk_kmat_batch_terms(ops._dtype_id(x), kinds, ptr(var), ptr(ils), None, 1, 1, ptr(x), n, d, n * d, ptr(x), n, d, n * d, d,
                                    ptr(out), n, n * n, B, 1, 1, NOISE, None, 0, 0, stream())
    assert code == 0, code


def loop_launch(x, out, variances, scales):
    for b in range(x.shape[0]):
        shared_launch(lib, x[b:b + 1], out[b:b + 1], variances[b], scales[b])


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


def inputs(B, n, d, dtype):
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn((B, n, d), generator=g, dtype=dtype).to(dev)
    return x, torch.empty((B, n, n), dtype=dtype, device=dev)


out = {"reps": args.reps, "inner": args.inner, "library_version": lib.gpk_version(),
       "parent_version": parent.gpk_version() if parent is not None else None}

# (a), (b): cfg4, fp32
B, n, d = 512, 2048, 3
x, buf = inputs(B, n, d, torch.float32)
scales = np.linspace(0.2, 3.0, B)
variances = np.linspace(0.5, 2.0, B)
var_t = torch.tensor(variances, dtype=torch.float64, device=dev).reshape(B, 1).contiguous()
ils_t = (1.0 / torch.tensor(scales, dtype=torch.float64, device=dev)).reshape(B, 1).contiguous()
cands = {"per_batch": lambda: batch_launch(x, buf, var_t, ils_t), "loop_of_512_unbatched": lambda: loop_launch(x, buf, variances, scales)}
res = compare(cands, 1)
res["per_batch_over_loop"] = ratio(res, "per_batch", "loop_of_512_unbatched")
out["a_cfg4_f32_per_batch_vs_loop"] = res
# the same numbers from both spellings (entry by entry: the same element program on the same parameters)
ref = torch.empty_like(buf)
batch_launch(x, buf, var_t, ils_t)
loop_launch(x, ref, variances, scales)
torch.cuda.synchronize()
out["a_outputs_equal"] = bool(torch.equal(torch.tril(buf), torch.tril(ref)))

if parent is not None:
    cands = {"parent": lambda: shared_launch(parent, x, buf), "per_batch": lambda: batch_launch(x, buf, var_t, ils_t),
             "parent_again": lambda: shared_launch(parent, x, buf), "shared_this_commit": lambda: shared_launch(lib, x, buf)}
    res = compare(cands, args.inner)
    res["per_batch_over_parent"] = ratio(res, "per_batch", "parent")
    res["parent_again_over_parent"] = ratio(res, "parent_again", "parent")
    out["b_cfg4_f32_per_batch_vs_parent_shared"] = res
    # (c)
    for name, (B2, n2, d2) in {"cfg4": (512, 2048, 3), "cfg2": (1, 16384, 8)}.items():
        for dtype in (torch.float32, torch.float64):
            x2, buf2 = inputs(B2, n2, d2, dtype)
            cands = {"parent": lambda: shared_launch(parent, x2, buf2), "this_commit": lambda: shared_launch(lib, x2, buf2),
                     "parent_again": lambda: shared_launch(parent, x2, buf2)}
            res = compare(cands, args.inner)
            res["this_commit_over_parent"] = ratio(res, "this_commit", "parent")
            res["parent_again_over_parent"] = ratio(res, "parent_again", "parent")
            a_ref, b_ref = torch.empty_like(buf2), torch.empty_like(buf2)
            shared_launch(parent, x2, a_ref)
            shared_launch(lib, x2, b_ref)
            torch.cuda.synchronize()
            res["outputs_equal"] = bool(torch.equal(torch.tril(a_ref), torch.tril(b_ref)))
            out[f"c_{name}_{'f32' if dtype == torch.float32 else 'f64'}_shared_vs_parent"] = res
            del x2, buf2, a_ref, b_ref

# (d): the forward logpdf, fp32
del buf, ref
B, n, d = 512, 2048, 3
st.B.epsilon = 1e-6
y = torch.randn((B, n, 1), dtype=torch.float32, device=dev)
v_pb = torch.tensor(variances, dtype=torch.float32, device=dev).reshape(B, 1, 1)
l_pb = torch.tensor(scales, dtype=torch.float32, device=dev).reshape(B, 1, 1)
f_pb, f_sh = st.GP(v_pb * st.EQ().stretch(l_pb)), st.GP(1.0 * st.EQ().stretch(1.0))
state = {}


def logpdf(f):
    with torch.no_grad():
        state["lp"] = f(x, NOISE).logpdf(y)


res = compare({"per_batch_model": lambda: logpdf(f_pb), "shared_model": lambda: logpdf(f_sh)}, 1)
res["per_batch_over_shared"] = ratio(res, "per_batch_model", "shared_model")
res["gps_per_second_per_batch"] = round(B / (res["per_batch_model"]["median_ms"] * 1e-3), 1)
out["d_cfg4_f32_forward_logpdf"] = res
print(json.dumps(out), flush=True)
