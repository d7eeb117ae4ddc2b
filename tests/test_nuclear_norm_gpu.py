"""``gpk_nuclear_norm``, the sum of the singular values by the Newton-Schulz polar iteration on the MFMA GEMM, through the C entry and
through ``HipBackend.nuclear_norm``, against ``numpy.linalg.svd`` in fp64 on the CPU (of the matrix as rounded to the working dtype,
so that the error is the entry's own).  Orders on both sides of the 16-element pitch of the workspace, the 32-tile of the glue
kernels and the 128-tile of the GEMM.  Matrices: ``L2^T L1`` from the Cholesky factors of two kernel matrices with noise 0.1 (what
``Normal.w2`` feeds) and Gaussian random matrices.

Bounds on ``|got - ref| / ref`` at the default step counts (60 / 40): 1e-12 in fp64, 1e-5 in fp32.  An emulation of the iteration in
NumPy with every product rounded to the working dtype stayed below 7e-16 / 6e-8 of ``tr V1 + tr V2``, of which the nuclear norm is a
quarter to a half; the factor of a few hundred on top is for the GEMM's different summation order and nothing else."""
import ctypes

import numpy as np
import pytest
import torch

from stheno_amd import _native, ops

from .test_w2_host import kernel_pair

pytestmark = pytest.mark.gpu

ORDERS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 127, 128, 129, 200, 257]
TOL = {torch.float64: 1e-12, torch.float32: 1e-5}
NP = {torch.float64: np.float64, torch.float32: np.float32}
_REF = {}


def _ceil16(n):
    return (n + 15) // 16 * 16


def _matrix(kind, n, seed=0):
    if kind == "chol":
        _, v1, _, v2 = kernel_pair(n, 0.1, seed=100 + n + seed)
        return np.linalg.cholesky(v2).T @ np.linalg.cholesky(v1)
    return np.random.default_rng(200 + n + seed).standard_normal((n, n))


def _reference(kind, n, dtype, seed=0):
    """``(matrix rounded to dtype, as fp64; its nuclear norm by the SVD)``, computed once per case."""
    key = (kind, n, dtype, seed)
    if key not in _REF:
        m = _matrix(kind, n, seed).astype(NP[dtype]).astype(np.float64)
        _REF[key] = (m, float(np.linalg.svd(m, compute_uv=False).sum()))
    return _REF[key]


def _strided(mats, dtype, ld, sm, offset, fill):
    """``mats`` (B, n, n) placed in a buffer filled with ``fill``: row stride ``ld``, batch stride ``sm``, starting ``offset`` elements
    into the storage.  Returns ``(buffer, view)``."""
    b, n, _ = mats.shape
    buf = torch.full((offset + b * sm + 7,), fill, dtype=dtype, device="cuda")
    view = buf.as_strided((b, n, n), (sm, ld, 1), offset)
    view.copy_(torch.as_tensor(mats, dtype=dtype))
    return buf, view


def _call(lib, m, n, ld, sm, batch, iters, out, ws, dtype=None):
    did = (_native.GPK_F32 if (m is not None and m.dtype == torch.float32) else _native.GPK_F64) if dtype is None else dtype
    ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())      # noqa: E731
    return lib.gpk_nuclear_norm(did, ptr(m), n, ld, sm, batch, iters, ptr(out), ptr(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _entry(lib, view, iters=None, poison=True):
    """The C entry on a (B, n, n) strided view; the workspace is filled with NaN first (its contents must not matter)."""
    b, n, _ = view.shape
    dtype = view.dtype
    if iters is None:
        iters = ops.NUCLEAR_ITERS_F64 if dtype == torch.float64 else ops.NUCLEAR_ITERS_F32
    ws = torch.full((int(lib.gpk_nuclear_norm_ws_elems(n, b)),), float("nan") if poison else 0.0, dtype=dtype, device="cuda")
    out = torch.full((b + 2,), -7.0, dtype=dtype, device="cuda")
    assert _call(lib, view, n, view.stride(1), view.stride(0), b, iters, out, ws) == 0
    assert bool((out[b:] == -7.0).all()), "the call wrote past its `batch` outputs"
    return out[:b].clone()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["chol", "gauss"])
@pytest.mark.parametrize("n", ORDERS)
def test_against_the_svd(hip_backend, dtype, kind, n):
    m, ref = _reference(kind, n, dtype)
    got_be = float(hip_backend.nuclear_norm(torch.as_tensor(m, dtype=dtype, device="cuda")))
    _, view = _strided(m[None], dtype, n + 5, n * (n + 5), 0, float("nan"))
    got_c = float(_entry(hip_backend.lib, view)[0])
    err_be, err_c = abs(got_be - ref) / ref, abs(got_c - ref) / ref
    print(f"nuclear_norm {kind} n={n} {dtype}: backend err {err_be:.3e}, C entry err {err_c:.3e}")
    assert np.isfinite(got_be) and np.isfinite(got_c)
    assert err_be <= TOL[dtype] and err_c <= TOL[dtype], (err_be, err_c)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 17, 33, 129, 200])
def test_layouts_padding_and_repeats(hip_backend, dtype, batch, wide, n):
    """Padded row strides, a batch stride beyond ``n * ld``, a storage offset that breaks the 16-byte alignment; NaN in every element
    outside the n x n blocks changes no bit; the input is left as it was; two calls in a row agree bit for bit."""
    lib = hip_backend.lib
    ld = _ceil16(n) + 16 if wide else n + 5
    sm = n * ld + 13
    cases = [_reference("chol" if b % 2 == 0 else "gauss", n, dtype, seed=b) for b in range(batch)]
    mats = np.stack([c[0] for c in cases])
    buf_nan, view_nan = _strided(mats, dtype, ld, sm, 3, float("nan"))
    buf_clean, view_clean = _strided(mats, dtype, ld, sm, 3, 0.0)
    before = buf_nan.clone()
    got = _entry(lib, view_nan)
    again = _entry(lib, view_nan, poison=False)
    clean = _entry(lib, view_clean)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, again), "a repeated call differs"
    assert torch.equal(got, clean), "NaN in the padding changed the result"
    assert torch.equal(buf_nan.view(torch.int64 if dtype == torch.float64 else torch.int32),
                       before.view(torch.int64 if dtype == torch.float64 else torch.int32)), "the input was written to"
    for b, (_, ref) in enumerate(cases):
        assert abs(float(got[b]) - ref) / ref <= TOL[dtype]
    # the backend on the same strided view (batch stride and row stride as they are): one launch sequence for the batch
    be = hip_backend.nuclear_norm(view_nan if batch > 1 else view_nan[0])
    assert tuple(be.shape) == ((batch,) if batch > 1 else ())
    assert torch.equal(be.reshape(-1), got)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_exact_cases(hip_backend, dtype):
    n = 40
    tol = TOL[dtype]
    dev = dict(dtype=dtype, device="cuda")
    assert float(hip_backend.nuclear_norm(torch.zeros((n, n), **dev))) == 0.0
    assert abs(float(hip_backend.nuclear_norm(torch.eye(n, **dev))) - n) <= tol * n
    q, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((n, n)))
    m = (-2.5 * q).astype(NP[dtype]).astype(np.float64)
    ref = float(np.linalg.svd(m, compute_uv=False).sum())
    got = float(hip_backend.nuclear_norm(torch.as_tensor(m, **dev)))
    assert abs(ref - 2.5 * n) <= 1e-5 * n and abs(got - ref) <= tol * ref
    # rank deficient: two equal rows and a zero row -- the singular values at zero stay there and cost nothing
    r = np.random.default_rng(6).standard_normal((20, 20)).astype(NP[dtype]).astype(np.float64)
    r[7] = r[3]
    r[11] = 0.0
    ref = float(np.linalg.svd(r, compute_uv=False).sum())
    got = float(hip_backend.nuclear_norm(torch.as_tensor(r, **dev)))
    print(f"nuclear_norm rank-deficient {dtype}: err {abs(got - ref) / ref:.3e}")
    assert np.isfinite(got) and abs(got - ref) <= tol * ref
    # a batch with a zero entry in it
    both = torch.stack([torch.zeros((20, 20), **dev), torch.as_tensor(r, **dev)])
    out = hip_backend.nuclear_norm(both)
    assert float(out[0]) == 0.0 and abs(float(out[1]) - ref) <= tol * ref


def test_ill_conditioned_pair_meets_the_parity_bar(hip_backend):
    """One noise-free pair (n = 200, fp64, jitter 1e-12: the smallest singular value is about 1e-14 of the Frobenius norm).  The error
    of ``2 |M|_*`` relative to ``tr V1 + tr V2`` is printed per step count; the default count must meet the project's parity bar."""
    n = 200
    _, v1, _, v2 = kernel_pair(n, 0.0, seed=9)
    jit = 1e-12 * np.eye(n)
    m = np.linalg.cholesky(v2 + jit).T @ np.linalg.cholesky(v1 + jit)
    ref = float(np.linalg.svd(m, compute_uv=False).sum())
    scale = float(np.trace(v1) + np.trace(v2))
    mt = torch.as_tensor(m, device="cuda")
    errs = {k: 2 * abs(float(hip_backend.nuclear_norm(mt, iters=k)) - ref) / scale for k in (20, 30, 40, 50, 60)}
    print("nuclear_norm noise-free pair, error of 2 |M|_* relative to tr V1 + tr V2:", {k: f"{e:.2e}" for k, e in errs.items()})
    default = 2 * abs(float(hip_backend.nuclear_norm(mt)) - ref) / scale
    assert ops.NUCLEAR_ITERS_F64 == 60 and default == errs[60]
    assert default <= 1e-6, errs


def test_workspace_size_argument_codes_and_version(hip_backend):
    lib = hip_backend.lib
    assert lib.gpk_version() >= 111
    # three 200 x 208 matrices, ceil(200 / 32) = 7 partial sums and the norm, per entry
    assert lib.gpk_nuclear_norm_ws_elems(200, 3) == 3 * (3 * 200 * 208 + 7 + 1)
    assert lib.gpk_nuclear_norm_ws_elems(0, 3) == 0 and lib.gpk_nuclear_norm_ws_elems(-4, 1) == 0 and lib.gpk_nuclear_norm_ws_elems(5, 0) == 0
    n = 20
    m = torch.eye(n, dtype=torch.float64, device="cuda")
    out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty((int(lib.gpk_nuclear_norm_ws_elems(n, 2)),), dtype=torch.float64, device="cuda")
    ok = dict(m=m, n=n, ld=n, sm=0, batch=2, iters=5, out=out, ws=ws)

    def code(**kw):
        a = dict(ok, **kw)
        return _call(lib, a["m"], a["n"], a["ld"], a["sm"], a["batch"], a["iters"], a["out"], a["ws"], a.get("dtype"))

    assert code(dtype=7) == -1
    assert code(n=0) == 0 and code(n=-3) == 0 and code(batch=0) == 0
    assert code(n=0, m=None, out=None, ws=None) == 0       # (an empty problem reads nothing)
    assert code(m=None) == -2
    assert code(n=(1 << 20) + 1, ld=1 << 21) == -3
    assert code(ld=n - 1) == -4
    assert code(sm=-1) == -5
    assert code(batch=65536) == -6
    assert code(iters=0) == -7 and code(iters=-2) == -7
    assert code(out=None) == -8
    assert code(ws=None) == -9
    assert bool((out == -7.0).all()), "a refused call wrote to out"
    assert code(iters=60) == 0                              # sm = 0: one matrix shared by the two entries
    assert abs(float(out[0]) - n) <= 1e-12 * n and float(out[0]) == float(out[1])
