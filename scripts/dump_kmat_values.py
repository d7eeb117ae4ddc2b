"""What the kernel-matrix entries of ``libgpk.so`` compute, launch shape by launch shape, as raw values in one ``.npz``: what a change
of ``gpk_kmat.hip`` / ``gpk_kdiff.hip`` / ``gpk_vjp.hip`` or of their shared headers that is meant to move code, not results, must
leave equal BIT FOR BIT.  Needs the GPU.

    python scripts/dump_kmat_values.py OUT.npz            # dump
    python scripts/dump_kmat_values.py A.npz B.npz        # compare two dumps (exit status 1 when an entry differs)

Run it on one machine with the library built at the two commits (the script uses the package of the tree it lies in) and compare.
``HipBackend.kmat``, ``kmat_diff``, ``kdiag``, ``kmat_vjp`` and ``kmat_vjp_dense`` for d = 1, 3, 8 (the row-band kernels with 1, 4 and
8 staged dimensions) and 9 (the chunked one-tile kernels), fp32 and fp64, a single-term program, an 8-term table and a table with RQ
and Delta; full, lower and rectangular matrices at ``97 x 259`` (partial tiles, several column tiles), a batch of 3, accumulation into
a padded view.  Then the shapes whose launch plan gives a workgroup several column tiles -- the two of ``tests/test_diff_gpu.py``
(1536 x 97 x 259 / 600 walked 3 tiles at a time, 640 lower triangles of 300 / 600 on the compact grid) and the lower triangle of one
``16384 x 16384`` matrix at d = 8 -- for which the dump holds a wrap-around int64 sum of the bit patterns and every 9973rd value."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stheno_amd import ops  # noqa: E402

DTYPES = {"f64": torch.float64, "f32": torch.float32}
SINGLE = ([("eq", 1.3, 0.9)], None)
TABLE8 = ([("eq", 1.0, 0.8), ("matern32", 0.7, 1.3), ("matern52", 0.5, 0.6), ("linear", 0.3, 1.7), ("const", 0.2, 1.0), ("rq", 0.9, 1.1),
           ("eq", 0.4, 2.1), ("matern52", 0.6, 1.9)], [None, None, None, None, None, 0.7, None, None])
RQ_DELTA = ([("rq", 1.1, 0.9), ("delta", 0.5, 1.0), ("matern12", 0.8, 1.4)], [1.6, 1e-6, None])
TABLES = {"single": SINGLE, "table8": TABLE8, "rq+delta": RQ_DELTA}
DIFF_TABLES = {"single": SINGLE, "table8": TABLE8, "rq": ([("rq", 1.1, 0.9), ("eq", 0.5, 1.2)], [1.6, None])}      # (Delta and Matern12 have no derivative)
N, M = 97, 259
DEV = "cuda"


def t(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=DTYPES[dtype], device=DEV)


def points(rng, shape, d):
    x = rng.standard_normal(tuple(shape) + (d,)) / np.sqrt(d)
    x.reshape(-1, d)[::5] = x.reshape(-1, d)[0]       # coincident points: the Delta term and the diagonal of the symmetric cases
    return x


def raw(v):
    return np.ascontiguousarray(v.detach().cpu().numpy())


def digest(v):
    """Wrap-around int64 sum of the bit patterns and a strided sample of a large result."""
    flat = v.contiguous().reshape(-1)
    if flat.element_size() == 4 and flat.numel() % 2:
        flat = torch.cat([flat, flat.new_zeros(1)])
    return np.concatenate([raw(flat.view(torch.int64).sum()).reshape(1), raw(flat[::9973].double()).view(np.int64)])


def small_cases(be, out, dtype, d):
    rng = np.random.default_rng(100 + d)
    x, y = t(points(rng, (N,), d), dtype), t(points(rng, (M,), d), dtype)
    xb, yb = t(points(rng, (3, N), d), dtype), t(points(rng, (3, M), d), dtype)
    dv = t((np.arange(N) % 16) / 8.0, dtype)
    base = t(np.arange(N * (M + 5)).reshape(N, M + 5) % 7 - 3, dtype)
    for name, (terms, shapes) in TABLES.items():
        kt, key = ops.KTerms(terms, shapes), f"{dtype}/d{d}/{name}"
        out[f"kmat/{key}/full"] = raw(be.kmat(kt, x, diag_add=0.25, diag_vec=dv))
        out[f"kmat/{key}/lower"] = raw(be.kmat(kt, x, lower=True, diag_add=0.25, diag_vec=dv, out=torch.zeros((N, N), dtype=x.dtype, device=DEV)))
        out[f"kmat/{key}/rect"] = raw(be.kmat(kt, x, y))
        out[f"kmat/{key}/batch3"] = raw(be.kmat(kt, xb, yb))
        acc = base.clone()
        be.kmat(kt, x, y, out=acc[:, 2:M + 2], accumulate=True)
        out[f"kmat/{key}/accumulate"] = raw(acc)
        out[f"kdiag/{key}"] = raw(be.kdiag(kt, xb))
        # the two gradient kernels: a symmetric "inverse", three weight columns; a dense cotangent with every option
        kinv = t(rng.standard_normal((N, N)), dtype)
        S, tr, dg = be.kmat_vjp(kt, x, kinv, t(rng.standard_normal((N, 3)), dtype), [0.7, -0.2, 1.1])
        out[f"vjp/{key}/S"], out[f"vjp/{key}/trace"], out[f"vjp/{key}/diag"] = raw(S), raw(tr), raw(dg)
        S, cs, gx = be.kmat_vjp_dense(kt, x, y, t(rng.standard_normal((N, M)), dtype), t(rng.uniform(0.5, 1.5, M), dtype),
                                      t(rng.standard_normal(N), dtype), t(rng.standard_normal(M), dtype), want_colsum=True, want_gradx=d <= 8)
        out[f"vjp_dense/{key}/S"], out[f"vjp_dense/{key}/colsum"] = raw(S), raw(cs)
        if gx is not None:
            out[f"vjp_dense/{key}/gradx"] = raw(gx)
    a, b = d - 1, 0
    for name, (terms, shapes) in DIFF_TABLES.items():
        kt, key = ops.KTerms(terms, shapes), f"{dtype}/d{d}/{name}"
        out[f"kmat_diff/{key}/full"] = raw(be.kmat_diff(kt, x, None, a, a, diag_add=0.25, diag_vec=dv))
        out[f"kmat_diff/{key}/lower"] = raw(be.kmat_diff(kt, x, None, a, a, lower=True, diag_add=0.25, diag_vec=dv,
                                                         out=torch.zeros((N, N), dtype=x.dtype, device=DEV)))
        for mode, dims in (("dx", (a, None)), ("dy", (None, b)), ("dxy", (a, b))):
            out[f"kmat_diff/{key}/rect-{mode}"] = raw(be.kmat_diff(kt, x, y, *dims))
        out[f"kmat_diff/{key}/batch3"] = raw(be.kmat_diff(kt, xb, yb, a, b))
        acc = base.clone()
        be.kmat_diff(kt, x, y, a, b, out=acc[:, 2:M + 2], accumulate=True)
        out[f"kmat_diff/{key}/accumulate"] = raw(acc)


def large_cases(be, out, dtype):
    rng = np.random.default_rng(7)
    kt = ops.KTerms(*TABLE8)
    rep = lambda v, batch: v[torch.arange(batch, device=DEV) % 3].contiguous()     # noqa: E731
    m, n = (259, 300) if dtype == "f64" else (600, 600)
    xb, yb, xs = t(points(rng, (3, N), 3), dtype), t(points(rng, (3, m), 3), dtype), t(points(rng, (3, n), 3), dtype)
    dv = t((np.arange(3 * n).reshape(3, n) % 16) / 8.0, dtype)
    out[f"walk/{dtype}/kmat_diff"] = digest(be.kmat_diff(kt, rep(xb, 1536), rep(yb, 1536), 2, 0))
    out[f"walk/{dtype}/kmat"] = digest(be.kmat(kt, rep(xb, 1536), rep(yb, 1536)))
    for fn, dims in ((be.kmat_diff, (None, 2, 2)), (be.kmat, ())):
        res = fn(kt, rep(xs, 640), *dims, lower=True, diag_add=0.25, diag_vec=rep(dv, 640), out=torch.zeros((640, n, n), dtype=xs.dtype, device=DEV))
        out[f"compact/{dtype}/{fn.__name__}"] = digest(res)
    big = t(points(rng, (16384,), 8), dtype)
    for name, (terms, shapes) in (("single", SINGLE), ("table8", TABLE8)):
        res = be.kmat(ops.KTerms(terms, shapes), big, lower=True, diag_add=0.1, out=torch.zeros((16384, 16384), dtype=big.dtype, device=DEV))
        out[f"n16384/{dtype}/kmat/{name}"] = digest(res)
        del res
    res = be.kmat_diff(kt, big, None, 7, 7, lower=True, diag_add=0.1, out=torch.zeros((16384, 16384), dtype=big.dtype, device=DEV))
    out[f"n16384/{dtype}/kmat_diff/table8"] = digest(res)


def dump(path):
    be, out = ops.HipBackend(), {}
    for dtype in DTYPES:
        for d in (1, 3, 8, 9):
            small_cases(be, out, dtype, d)
        large_cases(be, out, dtype)
    torch.cuda.synchronize()
    np.savez(path, **{k.replace("/", "|"): v for k, v in out.items()})
    print(f"{len(out)} arrays -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        if a[name].shape != b[name].shape or a[name].dtype != b[name].dtype or a[name].tobytes() != b[name].tobytes():
            bad.append(name)
    print(f"{len(a.files)} / {len(b.files)} arrays, {len(bad)} differ" + "".join(f"\n  {n}" for n in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2:
        dump(sys.argv[1])
    elif len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
