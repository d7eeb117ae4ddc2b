"""Benchmark of the dense GP inference hot path on MI355X.

Metric (BASELINE.json): GP logpdf+posterior evals/sec at N=16384 D=8 fp64, with the
Cholesky trailing-update GEMM priced against the fp64 MFMA peak.

One STEP = one eval of ``configs[1]``:  from ``x`` (N x D, resident in HBM) build
``K + sigma^2 I`` (lower triangle, jitter fused), Cholesky-factorise it in place,
condition ``f | (f(x, noise), y)``, the posterior mean + marginal variance at N* = 2048 test points, and
``f(x, noise).logpdf(y)`` (re-using the factor) -- through the public ``stheno_amd`` API, i.e. through libgpk.so.
Call order (``--order``): the posterior first (default) -- nothing has factorised K when it is asked for, so K(x*, x) rides through the
factorisation as rows under the matrix (``gpk_potrf_rows``) and there is no separate 2048-column solve -- or the log-density first (the
factor exists when the posterior is asked for: the blocked solve of rounds 1-4).  Same quantities, same flops, one factorisation either way.  Nothing is carried from one step to the next: the
kernel matrix, the factor and the solves are rebuilt, and the one thing the library remembers about
a data tensor between calls -- the NaN scan of ``y`` (``matrix.any_missing``) -- is forgotten at the
start of every step, so each step pays for its scan like a first call.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload dense_f64|sum_f32|batched_f32|sparse_f32] [--full]
                    [--dump-outputs DIR]

A plain run sets up, runs W untimed and K timed steps, and prints the line: ``value`` (steps per second, or GPs per second for the
batched workload) and ``ms_per_step`` come from the K timed steps alone.  ``--dump-outputs DIR`` writes what the last timed step
returned (``logpdf``, ``mean``, ``var``; ``logpdf`` of the batched workload; ``elbo`` of the sparse one) as ``DIR/<name>.npy`` in the
workload's precision; the inputs are seeded, so two builds given the same arguments can be compared output for output.

``--gpus N`` with N > 1: one process per GPU.  Either the driver launches this file under
``python -m torch.distributed.run --nproc-per-node N ...`` (RANK / WORLD_SIZE in the environment), or --
when they are absent -- ``bench.py --gpus N`` re-launches ITSELF that way (127.0.0.1 rendezvous, a free
port) and passes the one JSON line through.  The dense workload does not shard (one coupled
factorisation), so every rank runs an independent replica ("replicas only"); the batched configuration
(BASELINE.json configs[3]: 512 independent GPs, the one north_star scales over GPUs) shards its GPs over
the ranks and all-gathers the log-densities (stheno_amd/dist.py): it is the headline of
``--workload batched_f32`` and rides along as the ``batched`` sub-record of every other workload's ``--full`` line.
``--dry-run-dist`` proves the launch / rendezvous / collective / reporting path on a GPU-less box (gloo,
a stand-in step that does no GP arithmetic; the line says ``"dry_run": true``).

Rank 0 prints ONE JSON line.  What takes runs or host time of its own comes with ``--full`` only (``"full": true`` in the line):
``other_call_order``, ``roofline``, the measured peak, ``allgather_us``, the ``batched`` sub-record and ``cpu_baseline``; a plain
run's line has ``roofline`` and ``cpu_baseline`` null.  ``roofline`` is the dominant kernel -- the MFMA GEMM variant with the
largest summed duration in a step; for the dense workloads that is the persistent two-segment
trailing update of the look-ahead Cholesky, ``gemm_persist_kernel<double, 128, false>`` --:
algorithmic flops of its launches in one step / their summed duration, measured with HIP
events on the launch stream (gpk_prof_* hooks) in extra, untimed steps right after the
timed region; ``whole_step`` prices the entire step (all kernels, all gaps) the same way.
``cpu_baseline`` is the NumPy/SciPy oracle (a restatement of Stheno's NumPy path) timed on
the host cores on a bounded sample -- a reported baseline, not the target.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import stheno_amd as st  # noqa: E402
from stheno_amd import _native  # noqa: E402
from stheno_amd.matrix import forget_scan  # noqa: E402

PEAK_TFLOPS = {"f64": 78.6, "f32": 157.3}     # dense MFMA peaks, MI355X_MICROARCH.md / SURVEY 8(d)
NOISE = 0.1

WORKLOADS = {
    # name: (description, dtype, N, D, N*, extra)
    "dense_f64": dict(desc="EQ() kernel, N=16384 D=8 fp64, logpdf + condition, posterior mean/var at N*=2048",
                      dtype="f64", n=16384, d=8, ns=2048),
    "sum_f32": dict(desc="EQ()+Linear(), N=32768 D=4 fp32, logpdf + posterior at 2048 test points",
                    dtype="f32", n=32768, d=4, ns=2048),
    "batched_f32": dict(desc="512 independent GPs x N=2048 D=3 EQ fp32, logpdf, sharded over ranks",
                        dtype="f32", n=2048, d=3, b=512),
    "sparse_f32": dict(desc="PseudoObs VFE ELBO, N=200000 D=8, M=4096 inducing, EQ fp32",
                       dtype="f32", n=200000, d=8, m=4096),
}
TORCH_DTYPE = {"f64": torch.float64, "f32": torch.float32}
DEFER_CHECKS = False         # (--deferred-checks: the whole step inside st.deferred_checks(); measured 0.4 ms SLOWER per cfg2 step -- the one host
                             # read moves to the end of the step, where nothing of the next step is queued yet: profiles/r05_experiments.md section 7)
DRY_RUN_GPS = 16             # (--dry-run-gps: stand-in GPs of the dry run; any number, also one the ranks do not divide)
ORDER = "posterior-first"    # (--order: which of the step's two API calls comes first -- the same work either way)


def make_inputs(name, device, rank=0, world=1, n_override=None):
    """Synthetic inputs of the named config (seeded; ``x ~ N(0,1)``, ``y ~ N(0,1)``)."""
    w = dict(WORKLOADS[name])
    if n_override:
        w["n"] = n_override
    dt = TORCH_DTYPE[w["dtype"]]
    g = torch.Generator(device="cpu").manual_seed(0)
    if name in ("dense_f64", "sum_f32"):
        x = torch.randn(w["n"], w["d"], generator=g, dtype=torch.float64).to(dt).to(device)
        y = torch.randn(w["n"], 1, generator=g, dtype=torch.float64).to(dt).to(device)
        xs = torch.randn(w["ns"], w["d"], generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dt).to(device)
        return w, dict(x=x, y=y, xs=xs)
    if name == "batched_f32":
        from stheno_amd.dist import shard_bounds

        lo, hi = shard_bounds(w["b"], world, rank)
        x = torch.randn(w["b"], w["n"], w["d"], generator=g, dtype=torch.float32)[lo:hi].to(device)
        y = torch.randn(w["b"], w["n"], 1, generator=g, dtype=torch.float32)[lo:hi].to(device)
        return w, dict(x=x, y=y)
    if name == "sparse_f32":
        x = torch.randn(w["n"], w["d"], generator=g, dtype=torch.float32).to(device)
        y = torch.randn(w["n"], 1, generator=g, dtype=torch.float32).to(device)
        z = torch.randn(w["m"], w["d"], generator=torch.Generator().manual_seed(2), dtype=torch.float32).to(device)
        return w, dict(x=x, y=y, z=z)
    raise ValueError(name)


def make_step(name, w, t):
    """Returns a zero-argument callable running one eval; its return value is kept alive
    until the next call (so allocations are part of the step, like for a user)."""
    if name == "dense_f64":
        kernel = st.EQ()
    elif name == "sum_f32":
        kernel = st.EQ() + st.Linear()
    else:
        kernel = st.EQ()

    if name in ("dense_f64", "sum_f32"):
        def step():
            forget_scan(t["y"])          # (every step scans y for NaN, as a first call does)
            # (`--deferred-checks`: the step inside `st.deferred_checks()`, one `info` read at its end -- VERDICT r4's weak item 7;
            # measured slower in this loop, see DEFER_CHECKS)
            import contextlib

            with (st.deferred_checks() if DEFER_CHECKS else contextlib.nullcontext()):
                f = st.GP(kernel)
                fdd = f(t["x"], NOISE)
                if ORDER == "posterior-first":
                    # condition + predict before anything has factorised K: K(x*, x) rides in the factorisation as rows under the kernel
                    # matrix (gpk_potrf_rows) and the separate 2048-column triangular solve is gone; the log-density shares the factor
                    post = f | (fdd, t["y"])
                    mean, var = post(t["xs"]).marginals()
                    lp = fdd.logpdf(t["y"])
                else:
                    lp = fdd.logpdf(t["y"])
                    post = f | (fdd, t["y"])
                    mean, var = post(t["xs"]).marginals()
            return lp, mean, var
    elif name == "batched_f32":
        from stheno_amd.dist import sharded_logpdf

        def step():
            forget_scan(t["y"])
            f = st.GP(kernel)
            return sharded_logpdf(f, t["x"], NOISE, t["y"], w["b"])
    else:
        def step():
            forget_scan(t["y"])
            prior = st.Measure()
            f = st.GP(kernel, measure=prior)
            return st.PseudoObs(f(t["z"]), f(t["x"], NOISE), t["y"]).elbo(prior)
    return step


def pmc_traffic(name, w, kernel):
    """HBM-side bytes per launch of ``kernel`` from the committed PMC passes (``rocprofv3 --pmc FETCH_SIZE`` and
    ``--pmc WRITE_SIZE`` run separately on this same command by scripts/collect_pmc.py; FETCH_SIZE doubled as
    MI355X_MICROARCH.md prescribes for gfx950).  PMC collection cannot run inside the timed process, so the
    figure is read from ``profiles/``; ``None`` if no pass exists for this workload / kernel."""
    if w["n"] != WORKLOADS[name]["n"]:
        return None, None
    # only a pass of THIS round's kernels and call order counts (a figure read back from an older round's file
    # can be stale after a kernel change); the line names the file it came from
    path = os.path.join(ROOT, "profiles", "r06_pmc_%s.json" % name)
    if os.path.exists(path):
        with open(path) as f:
            ks = json.load(f)["kernels"]
        # (the profiler prints every template argument: the plain kernels carry their k-loop variant, `..., 2>`, behind what the hooks name)
        k = ks.get(kernel) or ks.get(kernel[:-1] + ", 2>")
        if k is not None:
            return k["hbm_bytes_per_launch"], "profiles/r06_pmc_%s.json (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this command)" % name
    return None, None


PROF_CODES = 256        # gpk_prof variant codes (include/gpk.h, gpk_prof_stop)


def measured_peak(dtype, min_ms=60.0):
    """The chip's SUSTAINED matrix-pipe rate on THIS box (``gpk_mfma_peak``: one workgroup per CU, register-resident waves streaming the
    library's own MFMA instruction on pseudo-random operands for >= ``min_ms`` of device time) -- what SURVEY 8(d) asks to be printed
    beside the nominal peak.  One and two waves per SIMD are measured, the better one is the peak; the shader clock the stream ran
    at and the pipes' issue efficiency at that clock come with it."""
    import ctypes

    lib = _native.load()
    best = None
    for waves in (2, 1):
        tf, ms, mhz, eff = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        st_ = lib.gpk_mfma_peak(0 if dtype == "f32" else 1, float(min_ms), waves, ctypes.byref(tf), ctypes.byref(ms), ctypes.byref(mhz),
                                ctypes.byref(eff), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if st_ != 0:
            return None
        rec = {"tflops": tf.value, "waves_per_simd": waves, "device_ms": ms.value, "shader_clock_mhz": mhz.value, "issue_efficiency_at_that_clock": eff.value}
        if best is None or rec["tflops"] > best["tflops"]:
            best = rec
    best["what"] = ("gpk_mfma_peak: 256 threads x waves_per_simd per CU, 8 independent accumulators per wave, v_mfma_%s_16x16x4 on pseudo-random "
                    "operands, no memory traffic, >= %.0f ms of device time" % ("f32" if dtype == "f32" else "f64", min_ms))
    return best


def dominant_kernel_roofline(name, w, step, prof_steps=2):
    """Live roofline of the dominant kernel (``--full``): extra untimed steps under HIP-event hooks, every GEMM kernel variant's
    summed time, the one with the most time priced against the nominal peak."""
    import ctypes

    lib = _native.load()
    lib.gpk_prof_start()
    for _ in range(prof_steps):
        keep = step()
    torch.cuda.synchronize()
    del keep
    ms, nl, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    best = None
    for code in range(PROF_CODES):    # every GEMM kernel variant: the dominant one is the one with the most time
        lib.gpk_prof_stop(code, ctypes.byref(ms), ctypes.byref(nl), ctypes.byref(fl))
        if nl.value > 0 and (best is None or ms.value > best[1]):
            best = (code, ms.value, nl.value, fl.value)
    if best is None or best[1] <= 0:
        return None
    peak = PEAK_TFLOPS[w["dtype"]]
    code, tms, launches, flops = best
    achieved = flops / (tms * 1e-3) / 1e12
    kname = _variant_name(code, w["dtype"])
    return {
        "kernel": kname,
        "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
        "traffic": pmc_traffic(name, w, kname)[0],
        "traffic_source": pmc_traffic(name, w, kname)[1],
        "launches_per_step": launches // prof_steps,
        "avg_launch_us": tms * 1e3 / launches,
        "algorithmic_flops_per_step": flops / prof_steps,
        "kernel_ms_per_step": tms / prof_steps,
    }


def _variant_name(code, dtype):
    """Kernel behind a gpk_prof variant code (see gpk_prof_stop in include/gpk.h)."""
    t = "double" if dtype == "f64" else "float"
    ts = 64 if code & 16 else 128
    edge = "true" if code & 1 else "false"
    if code >= 160:                  # one mixed-phase step of a batched factorisation (panel solves + update tiles in one launch)
        return f"batch_mix_kernel<{t}>"
    if code >= 128:                  # the panel solve against a triangular inverse: its own kernel (and its own code since round 4)
        return f"gemm_trib_kernel<{t}, {ts}, {edge}, {2 if ts == 64 else 1}>"
    if code >= 96:
        return f"gemm_trilo_pair_kernel<{t}, {'true' if code & 2 else 'false'}, {edge}>"
    if code >= 64:
        return f"panel_step_kernel<{t}, ..., {edge}>"
    if code & 32:
        return f"gemm_persist_kernel<{t}, {ts}, {edge}>"
    return f"gemm_kernel<{t}, {ts}, {'true' if code & 4 else 'false'}, {'true' if code & 2 else 'false'}, {edge}, 1>"


#: algorithmic flops of ONE step: POTRF N^3/3 + posterior TRSM N^2 N* + the O(N^2) rest (kernel
#: matrices, TRSV, reductions: < 1 %, not counted)
def step_flops(name, w):
    n = float(w["n"])
    if name in ("dense_f64", "sum_f32"):
        return n ** 3 / 3 + n * n * w["ns"]
    if name == "batched_f32":
        return w["b"] * n ** 3 / 3
    m = float(w["m"])
    return 2 * m * m * n + 2 * m ** 3 / 3          # TRSM M^2 N + SYRK M^2 N (symmetric count) + two POTRF(M)


def _host_threads():
    try:
        from threadpoolctl import threadpool_info

        return int(max([p.get("num_threads", 1) for p in threadpool_info()] or [1]))
    except Exception:
        return os.cpu_count() or 1


def _full_size_cpu_record(name):
    """The one-off FULL-SIZE run of the CPU baseline (``bench.py --cpu-baseline-full``, committed under ``profiles/``): printed
    beside the bounded sample's extrapolation so that the extrapolation can be judged."""
    for rnd in ("r06", "r05", "r04"):
        path = os.path.join(ROOT, "profiles", "%s_cpu_baseline_full_%s.json" % (rnd, name))
        if os.path.exists(path):
            with open(path) as f:
                return json.load(f)
    return None


def cpu_baseline(name, full=False):
    """The oracle (NumPy/SciPy restatement of Stheno's NumPy path) on the host cores, on a bounded sample of
    the same workload (stated in ``sample``); the same op sequence as the GPU step, one shared factorisation.
    ``full``: the dense workloads at their full N instead (minutes; development / one-off record)."""
    from oracle import gp_oracle as O

    w = WORKLOADS[name]
    rng = np.random.default_rng(0)
    np_dt = np.float64 if w["dtype"] == "f64" else np.float32
    eps = 1e-12 if w["dtype"] == "f64" else 1e-6
    if name in ("dense_f64", "sum_f32"):
        # dense_f64 runs at its FULL N: 13.7 s on the GPU box's 128 host threads (profiles/r04_cpu_baseline_full_dense_f64.json) -- the
        # N = 8192 sample of rounds 1-3, scaled by N^3, over-estimated the time five-fold (8.7 s measured at N = 8192: the host BLAS is
        # far from its asymptotic rate there)
        # sum_f32: the live sample is N = 16384 (the host BLAS is close to its asymptotic rate there: the extrapolation lands within ~10 % of
        # the full-size run; the N = 8192 sample of rounds 1-5 was 8.7x off)
        n_s = w["n"] if (full or name == "dense_f64") else 16384
        terms = [("eq", 1.0, 1.0)] if name == "dense_f64" else [("eq", 1.0, 1.0), ("linear", 1.0, 1.0)]
        x, y = rng.standard_normal((n_s, w["d"])).astype(np_dt), rng.standard_normal((n_s, 1)).astype(np_dt)
        xs = rng.standard_normal((w["ns"], w["d"])).astype(np_dt)
        t0 = time.perf_counter()
        k = O.kernel_matrix(terms, x) + NOISE * np.eye(n_s, dtype=np_dt)
        t_k = time.perf_counter() - t0
        blocked = n_s >= 32768
        if blocked:
            # (OpenBLAS' potrf segfaults at this order on the boxes of this pool -- tests/golden/make_golden_fullsize.py met it too -- so
            # the factorisation is spelt out right-looking on 8192-blocks with the same LAPACK / BLAS calls: potrf, trsm, syrk)
            import scipy.linalg as sla

            k = O.reg(k, eps)
            nbk = 8192
            for c in range(0, n_s, nbk):
                e = min(c + nbk, n_s)
                k[c:e, c:e] = np.linalg.cholesky(k[c:e, c:e])
                if e < n_s:
                    k[e:, c:e] = sla.solve_triangular(k[c:e, c:e], k[e:, c:e].T, lower=True, check_finite=False).T
                    k[e:, e:] -= k[e:, c:e] @ k[e:, c:e].T
            chol = np.tril(k)
            del k
        else:
            chol = O.cholesky(k, eps)
        lp = -(O.logdet_chol(chol) + n_s * O.LOG_2_PI + O.iqf_diag(chol, y)) / 2
        v = O.solve_lower(chol, O.kernel_matrix(terms, x, xs))
        mean = v.T @ O.solve_lower(chol, y)
        var = O.kernel_diag(terms, xs) - np.sum(v * v, axis=0)
        dt = time.perf_counter() - t0
        assert np.isfinite(lp).all() and np.isfinite(mean).all() and np.isfinite(var).all()
        # the kernel-matrix build and the solves against N* scale with N^2, the factorisation with N^3
        r = w["n"] / n_s
        t_fac = dt - t_k
        if n_s == w["n"]:
            return {"value": 1.0 / dt, "unit": "evals/s", "cores": _host_threads(), "kind": "port", "seconds_per_eval": dt,
                    "sample": f"oracle/gp_oracle.py (NumPy/SciPy, {w['dtype']}) at the FULL N={n_s}, D={w['d']}, N*={w['ns']}: {dt:.2f} s per "
                              f"eval measured ({t_k:.2f} s of it the kernel-matrix build); no extrapolation"
                              + ("; Cholesky spelt out on 8192-blocks (potrf / trsm / syrk of the same BLAS: its potrf segfaults at this order)" if blocked else "")}
        t_full = t_k * r * r + t_fac * r ** 3
        out = {"value": 1.0 / t_full, "unit": "evals/s", "cores": _host_threads(), "kind": "port",
               "sample": f"oracle/gp_oracle.py (NumPy/SciPy, {w['dtype']}) at N={n_s}, D={w['d']}, N*={w['ns']}: {dt:.2f} s per eval "
                         f"measured ({t_k:.2f} s of it the N^2 kernel-matrix build); extrapolated to N={w['n']} with the build "
                         f"scaled by (N/{n_s})^2 and the rest by (N/{n_s})^3"}
        rec = _full_size_cpu_record(name)
        if rec is not None:
            # VERDICT r5 (weak 11): the MEASURED full-size figure is the baseline's `value`; this run's bounded sample and its
            # extrapolation stay beside it (`live_sample`) so that the two can be compared
            live = dict(out)
            out = {"value": rec["value"], "unit": rec.get("unit", "evals/s"), "cores": rec.get("cores", out["cores"]), "kind": "port",
                   "seconds_per_eval": rec.get("seconds_per_eval"),
                   "sample": "FULL-SIZE run of oracle/gp_oracle.py on this pool's host cores, measured once and committed (profiles/*_cpu_baseline_full_%s.json: %s); "
                             "this run's bounded sample is under `live_sample`" % (name, rec.get("sample", "")),
                   "live_sample": live}
        return out
    if name == "batched_f32":
        n_g = 4
        x = rng.standard_normal((n_g, w["n"], w["d"])).astype(np_dt)
        y = rng.standard_normal((n_g, w["n"], 1)).astype(np_dt)
        t0 = time.perf_counter()
        for b in range(n_g):
            lp = O.gp_logpdf([("eq", 1.0, 1.0)], x[b], NOISE, y[b], eps=eps)
        dt = time.perf_counter() - t0
        assert np.isfinite(lp)
        return {"value": n_g / dt, "unit": "GPs/s", "cores": _host_threads(), "kind": "port",
                "sample": f"oracle/gp_oracle.py gp_logpdf (NumPy/SciPy, fp32 inputs) on {n_g} of the 512 GPs (N={w['n']}, D={w['d']}), one after "
                          f"the other as NumPy's batched path does: {dt:.2f} s"}
    full = True          # (round 5: 13-14 s per eval at the FULL N = 200000 on the box's 128 host threads -- inside the 10-30 s a bounded sample may take;
                         #  the N = 20000 sample of rounds 1-4, scaled, had said 15-18 s)
    n_s = w["n"] if full else 20000
    x, y = rng.standard_normal((n_s, w["d"])).astype(np_dt), rng.standard_normal((n_s, 1)).astype(np_dt)
    z = rng.standard_normal((w["m"], w["d"])).astype(np_dt)
    t0 = time.perf_counter()
    elbo = O.pseudo_obs([("eq", 1.0, 1.0)], x, NOISE, y, z, method="vfe", eps=eps)["elbo"]
    dt = time.perf_counter() - t0
    assert np.isfinite(elbo)
    # the M^3 part (two factorisations) does not grow with N: measure it alone and scale only the rest
    t1 = time.perf_counter()
    O.cholesky(O.kernel_matrix([("eq", 1.0, 1.0)], z) + 0.1 * np.eye(w["m"], dtype=np_dt), eps)
    t_m3 = 2 * (time.perf_counter() - t1)
    if full:
        return {"value": 1.0 / dt, "unit": "evals/s", "cores": _host_threads(), "kind": "port", "seconds_per_eval": dt,
                "sample": f"oracle/gp_oracle.py pseudo_obs (VFE; NumPy/SciPy, fp32 inputs) at the FULL N={n_s}, M={w['m']}: {dt:.2f} s per eval "
                          f"measured; no extrapolation"}
    t_full = t_m3 + max(dt - t_m3, 0.0) * (w["n"] / n_s)
    out = {"value": 1.0 / t_full, "unit": "evals/s", "cores": _host_threads(), "kind": "port",
           "sample": f"oracle/gp_oracle.py pseudo_obs (VFE; NumPy/SciPy, fp32 inputs) at N={n_s}, M={w['m']}: {dt:.2f} s measured; the two "
                     f"M^3 factorisations ({t_m3:.2f} s) kept, the O(N M^2) rest scaled by N/{n_s} = x{w['n'] // n_s}"}
    rec = _full_size_cpu_record(name)
    if rec is not None:
        out["full_size_measured"] = {k: rec[k] for k in ("value", "unit", "cores", "seconds_per_eval", "sample") if k in rec}
    return out


def _free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _relaunch_under_torchrun(n, argv):
    """``bench.py --gpus N`` outside a launcher: start N ranks of this file (one per GPU) under ``torch.distributed.run`` and hand
    their output through -- rank 0 prints the one JSON line."""
    import subprocess

    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), GPK_BENCH_RELAUNCHED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=env)


class _StandInProcess:
    """``--dry-run-dist``: stands where a ``GP`` stands in ``dist.sharded_logpdf`` -- ``process(x, noise).logpdf(y)`` -- and does no
    GP arithmetic (there is no CPU path in the package to do it with): the launch, the sharding, the collective and the reporting
    are what the dry run is about."""

    def __call__(self, x, noise):
        self._x, self._noise = x, noise
        return self

    def logpdf(self, y):
        return -(y[..., 0] ** 2).sum(-1) / (1.0 + self._noise) - self._x.pow(2).sum((-1, -2))


def _timed(step, steps, warmup, barrier, use_dist, device):
    """W untimed + K timed steps between barriers; the MAX over ranks of the elapsed time, and what the last timed step returned."""
    keep = None
    for _ in range(warmup):
        keep = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        keep = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:
        import torch.distributed as dist

        tmax = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax[0])
    return elapsed, keep


#: names of what one step of each workload returns, in ``make_step``'s order (``--dump-outputs`` writes ``<name>.npy`` for each)
OUTPUT_NAMES = {"dense_f64": ("logpdf", "mean", "var"), "sum_f32": ("logpdf", "mean", "var"), "batched_f32": ("logpdf",),
                "sparse_f32": ("elbo",)}


def dump_outputs(name, result, out_dir):
    """``--dump-outputs DIR``: what the last timed step computed -- the arrays a caller of the step receives -- as ``DIR/<name>.npy``
    in the workload's own precision (float32 or float64); at most 33 kB per workload, so nothing is sampled."""
    arrays = result if isinstance(result, tuple) else (result,)
    assert len(arrays) == len(OUTPUT_NAMES[name]), (name, len(arrays))
    os.makedirs(out_dir, exist_ok=True)
    for key, a in zip(OUTPUT_NAMES[name], arrays):
        np.save(os.path.join(out_dir, key + ".npy"), torch.as_tensor(a).detach().cpu().numpy())


def _allgather_us(total, world, device, barrier, reps=50):
    """Average time of the data path's ONE exchange step by itself: the all-gather of ``total / world`` fp32 log-densities per rank."""
    import torch.distributed as dist

    local = torch.zeros(total // world, dtype=torch.float32, device=device)
    out = torch.empty(total // world * world, dtype=torch.float32, device=device)
    for _ in range(5):
        dist.all_gather_into_tensor(out, local)
    barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        dist.all_gather_into_tensor(out, local)
    barrier()
    return 1e6 * (time.perf_counter() - t0) / reps


def _batched_record(device, rank, world, steps, warmup, barrier, use_dist, dry_run=False):
    """configs[3] (512 independent GPs x N = 2048, D = 3, EQ, fp32) sharded over the ranks: whole-job GPs/s, the step time, the
    fraction of the fp32 MFMA peak PER GPU the factorisations reach, the all-gather alone."""
    name = "batched_f32"
    if dry_run:
        from stheno_amd.dist import shard_bounds, sharded_logpdf

        w = dict(WORKLOADS[name], n=8, b=DRY_RUN_GPS)
        lo, hi = shard_bounds(w["b"], world, rank)
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(w["b"], w["n"], w["d"], generator=g)[lo:hi].to(device)
        y = torch.randn(w["b"], w["n"], 1, generator=g)[lo:hi].to(device)
        proc = _StandInProcess()

        def step():
            return sharded_logpdf(proc, x, NOISE, y, w["b"])
    else:
        w, t = make_inputs(name, device, rank, world)
        eps0 = st.B.epsilon
        st.B.epsilon = 1e-6
        step = make_step(name, w, t)
    try:
        elapsed, _ = _timed(step, steps, warmup, barrier, use_dist, device)
        full = step()
    finally:
        if not dry_run:
            st.B.epsilon = eps0
    assert full.shape == (w["b"],) and bool(torch.isfinite(full).all())
    rec = {"metric": "batched GP logpdfs/sec (512 x N=2048 D=3 fp32)" if not dry_run else "dry run of the batched path (%d stand-in GPs)" % w["b"],
           "value": w["b"] * steps / elapsed, "unit": "GPs/s", "n_gpus": world, "steps": steps, "warmup": warmup,
           "ms_per_step": 1e3 * elapsed / steps, "scaling": "strong", "dtype": "f32",
           "parallelism": "GPs sharded over %d ranks (contiguous blocks), all-gather of the log-densities" % world,
           "allgather_us": (_allgather_us(w["b"], world, device, barrier) if use_dist and w["b"] % world == 0 else None)}
    if not dry_run:
        fl = step_flops(name, w) / world * steps / elapsed / 1e12
        rec["per_gpu_step"] = {"unit": "TFLOP/s", "achieved": fl, "peak": PEAK_TFLOPS["f32"], "frac": fl / PEAK_TFLOPS["f32"]}
        pm = measured_peak("f32") if rank == 0 else None
        if pm is not None:
            rec["per_gpu_step"].update(peak_measured=pm["tflops"], frac_of_measured=fl / pm["tflops"], peak_measurement=pm)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="dense_f64", choices=sorted(WORKLOADS))
    ap.add_argument("--n", type=int, default=0, help="override N (development only; invalidates the metric)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="ONLY time the CPU baseline of a dense workload at its full N (minutes of host time, no GPU) and print it as JSON")
    ap.add_argument("--order", default="posterior-first", choices=["posterior-first", "logpdf-first"],
                    help="dense workloads: condition + predict, then the log-density (default: the posterior's solve rides in the factorisation) "
                         "or the other way round (the factor exists before the posterior is asked for: separate 2048-column solve)")
    ap.add_argument("--deferred-checks", action="store_true", help="development A/B: the whole step inside st.deferred_checks()")
    ap.add_argument("--no-batched-record", action="store_true", help="skip the `batched` sub-record (configs[3] sharded over the ranks)")
    ap.add_argument("--dry-run-dist", action="store_true",
                    help="GPU-less proof of the N-rank path: gloo, a stand-in step, the same launch / barrier / all-gather / JSON code")
    ap.add_argument("--dry-run-gps", type=int, default=16, help="--dry-run-dist: how many stand-in GPs are sharded over the ranks")
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: the other call order, the roofline of the dominant kernel, the measured peak, the "
                         "all-gather alone, the `batched` sub-record and the CPU baseline (a plain run times the steps and nothing else)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64; the inputs are seeded)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    global DEFER_CHECKS, ORDER, DRY_RUN_GPS
    DRY_RUN_GPS = max(1, args.dry_run_gps)
    DEFER_CHECKS = bool(args.deferred_checks)
    ORDER = args.order
    if args.cpu_baseline_full:
        print(json.dumps(cpu_baseline(args.workload, full=True)), flush=True)
        return
    launched = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    if args.gpus > 1 and not launched:
        raise SystemExit(_relaunch_under_torchrun(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if launched and args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d ranks" % (args.gpus, world))
    dry = args.dry_run_dist
    if dry:
        device = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device (there is no CPU path in stheno_amd)")
        if local_rank >= torch.cuda.device_count():
            raise SystemExit("bench.py: rank %d has no GPU (%d visible)" % (local_rank, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)          # one process per GPU
        device = torch.device("cuda", local_rank)
    use_dist = world > 1 or os.environ.get("GPK_BENCH_FORCE_DIST") == "1"   # (the env switch exercises the RCCL path on one GPU)
    if use_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    def barrier():
        if use_dist:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    if dry:
        rec = _batched_record(device, rank, world, args.steps, args.warmup, barrier, use_dist, dry_run=True)
        if rank == 0:
            out = {"metric": rec["metric"], "value": rec["value"], "unit": rec["unit"], "n_gpus": world, "steps": args.steps,
                   "warmup": args.warmup, "ms_per_step": rec["ms_per_step"], "higher_is_better": True, "scaling": "strong",
                   "vs_baseline": None, "dtype": "f32", "data": "dry run: no GP arithmetic, no GPU", "dry_run": True,
                   "config": {"workload": "stand-in step through stheno_amd.dist.sharded_logpdf", "parallelism": rec["parallelism"]},
                   "batched": rec, "world_size": (dist.get_world_size() if use_dist else 0), "backend": "gloo" if use_dist else None}
            line = json.dumps(out)
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(line, flush=True)
        return

    name = args.workload
    w, tensors = make_inputs(name, device, rank, world, args.n or None)
    if w["dtype"] == "f32":
        st.B.epsilon = 1e-6          # the reference's own fp32 setting (README.md:887-888)
    step = make_step(name, w, tensors)
    elapsed, last = _timed(step, args.steps, args.warmup, barrier, use_dist, device)
    if args.dump_outputs and rank == 0:
        dump_outputs(name, last, args.dump_outputs)
    del last
    full = args.full

    # -- the OTHER call order of the same step, a few steps (the default order is the one the rows-under-the-matrix path
    #    accelerates; the record carries both so that rounds stay comparable) --
    other_order = None
    if full and name in ("dense_f64", "sum_f32"):
        first = ORDER
        ORDER = "logpdf-first" if first == "posterior-first" else "posterior-first"
        try:
            k_other = max(2, min(args.steps, 5))
            el, _ = _timed(step, k_other, 1, barrier, use_dist, device)
            other_order = {"call_order": ORDER, "steps": k_other, "ms_per_step": 1e3 * el / k_other,
                           "value": k_other * (world if name != "batched_f32" else 1) / el}
        finally:
            ORDER = first

    roofline = dominant_kernel_roofline(name, w, step) if full else None
    peak = PEAK_TFLOPS[w["dtype"]]
    # -- the peak the chip SUSTAINS on this box, measured; the nominal figure stays the one `frac` is quoted against --
    pm = measured_peak(w["dtype"]) if full else None
    if roofline is not None and pm is not None:
        roofline["peak_measured"] = pm["tflops"]
        roofline["frac_of_measured"] = roofline["achieved"] / pm["tflops"]
        roofline["peak_measurement"] = pm
    whole = {"algorithmic_flops_per_step": step_flops(name, w), "unit": "TFLOP/s", "peak": peak}
    # per GPU: replicas run `world` steps at once, the batched workload splits one step over the ranks
    per_gpu = 1.0 if name != "batched_f32" else 1.0 / world
    whole["achieved"] = whole["algorithmic_flops_per_step"] * per_gpu * args.steps / elapsed / 1e12
    whole["frac"] = whole["achieved"] / peak
    if pm is not None:
        whole["peak_measured"] = pm["tflops"]
        whole["frac_of_measured"] = whole["achieved"] / pm["tflops"]
    allgather = None
    if full and name == "batched_f32" and use_dist and w["b"] % world == 0:
        allgather = _allgather_us(w["b"], world, device, barrier)

    # -- north_star: "at 1 GPU and at 2/4/8 GPUs for the batched config": configs[3] sharded over these same ranks --
    batched = None
    if full and name != "batched_f32" and not args.no_batched_record and not args.n:
        del step, tensors
        torch.cuda.empty_cache()
        batched = _batched_record(device, rank, world, max(2, min(args.steps, 10)), 1, barrier, use_dist)

    if rank == 0:
        units = args.steps * (world if name != "batched_f32" else 1)
        if name == "batched_f32":
            metric, unit, value = "batched GP logpdfs/sec (512 x N=2048 D=3 fp32)", "GPs/s", w["b"] * args.steps / elapsed
            scaling = "strong"
        elif name == "sparse_f32":
            metric, unit, value, scaling = "VFE ELBO evals/sec at N=200000 M=4096 fp32", "evals/s", units / elapsed, "weak"
        else:
            metric = "GP logpdf+posterior evals/sec at N=%d D=%d %s" % (w["n"], w["d"], "fp64" if w["dtype"] == "f64" else "fp32")
            unit, value, scaling = "evals/s", units / elapsed, "weak"
        out = {
            "metric": metric, "value": value, "unit": unit, "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": scaling, "vs_baseline": None, "dtype": w["dtype"], "data": "synthetic",
            "config": {"workload": w["desc"], "noise_variance": NOISE, "epsilon": st.B.epsilon,
                       "nan_scan": "every step (the library's per-tensor memo is cleared at the start of each step)",
                       "call_order": (ORDER if name in ("dense_f64", "sum_f32") else None),
                       "info_check": ("once per step, at the end of the step's st.deferred_checks() block (dense workloads)" if DEFER_CHECKS else "behind the call that factorised (the library's default)"),
                       "single_column_solve": "L^-1 (y - m(x)) is computed INSIDE the factorisation (a right-hand side under the matrix / inside the batched steps: "
                                              "the library's defaults matrix.config.posterior_rows_rhs, logpdf_rhs) -- the same quantity as the separate sweep, "
                                              "shared by the log-density and the posterior mean as before",
                       "parallelism": ("replicas only (%d independent evals in flight, one process per GPU)" % world) if name != "batched_f32"
                       else "GPs sharded over %d ranks, all-gather of log-densities" % world},
            "roofline": roofline,
            "whole_step": whole,
            "rccl_world_size": (dist.get_world_size() if use_dist else 0),
            "cpu_baseline": None if (not full or args.no_cpu_baseline or world > 1 or args.n) else cpu_baseline(name),
            "full": full,
        }
        if other_order is not None:
            out["other_call_order"] = other_order
        if allgather is not None:
            out["allgather_us"] = allgather
        if batched is not None:
            out["batched"] = batched
        line = json.dumps(out)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(line, flush=True)          # the ONE JSON line, last thing on stdout (after RCCL's own init / teardown chatter)


if __name__ == "__main__":
    main()
