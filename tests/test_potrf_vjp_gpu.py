"""``gpk_potrf_vjp``, the vector-Jacobian product of the Cholesky factorisation, through the C entry and through
``HipBackend.potrf_vjp``, against torch autograd through ``torch.linalg.cholesky`` in fp64 on the CPU (symmetrised).  Matrices: the
``a a^T + 0.5 I`` recipe of ``tests/test_posterior_grad_gpu.py::_factor``; orders one short of, on and one past the 128 diagonal
block / GEMM tile, and a ragged larger one.  The bounds are the project's own for the transposed solves on the same matrices."""
import ctypes

import pytest
import torch

from stheno_amd import _native, ops

from .test_posterior_grad_gpu import _factor

pytestmark = pytest.mark.gpu

ORDERS = [1, 127, 128, 129, 257, 1000]
TOL = {torch.float64: 1e-9, torch.float32: 2e-3}
_REF = {}


def _lbar(n, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.tril(torch.randn((n, n), dtype=torch.float64, generator=g))


def _reference(n):
    """``(spd, lbar, abar)`` in fp64 on the CPU, computed once per order: ``abar`` = the symmetrised gradient of
    ``sum(lbar * cholesky(spd))``."""
    if n not in _REF:
        g = torch.Generator(device="cuda").manual_seed(n)
        a = torch.randn((n, n + 8), dtype=torch.float64, device="cuda", generator=g) / (n + 8) ** 0.5
        spd = (a @ a.T + 0.5 * torch.eye(n, dtype=torch.float64, device="cuda")).cpu()
        lbar = _lbar(n, n)
        leaf = spd.clone().requires_grad_(True)
        (torch.linalg.cholesky(leaf) * lbar).sum().backward()
        _REF[n] = (spd, lbar, 0.5 * (leaf.grad + leaf.grad.T))
    return _REF[n]


def _chol_of(n, dtype, pad=0):
    """The factor of ``_reference(n)``'s matrix (the seed of ``_factor`` is the order)."""
    chol, _ = _factor(n, dtype, pad=pad, seed=n)
    return chol


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _call(lib, l, n, ld, dsb, sb, lbar, ldlb, abar, lda, ws, dtype=None):
    did = (_native.GPK_F32 if (l is not None and l.dtype == torch.float32) else _native.GPK_F64) if dtype is None else dtype
    ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())      # noqa: E731
    return lib.gpk_potrf_vjp(did, ptr(l), n, ld, ptr(dsb), sb, ptr(lbar), ldlb, ptr(abar), lda, ptr(ws),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", ORDERS)
def test_backend_against_torch_autograd(hip_backend, dtype, n):
    _, lbar, ref = _reference(n)
    chol = _chol_of(n, dtype)
    got = chol.potrf_vjp(lbar.to(dtype).cuda())
    err = _err(got, ref)
    print(f"potrf_vjp n={n} {dtype}: err {err:.3e}")
    assert tuple(got.shape) == (n, n)
    assert torch.equal(got, got.T), "abar is not symmetric bit for bit"
    assert err <= TOL[dtype], err


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [127, 129, 257])
def test_strict_upper_triangles_are_not_read_and_calls_repeat(hip_backend, dtype, n):
    _, lbar, ref = _reference(n)
    chol = _chol_of(n, dtype)
    sb, dsb = chol._blocks(n)
    lb = lbar.to(dtype).cuda()
    clean = hip_backend.potrf_vjp(chol.lower(), dsb, sb, lb)
    again = hip_backend.potrf_vjp(chol.l, dsb, sb, lb)
    assert torch.equal(clean, again), "a repeated call differs"
    upper = torch.triu(torch.ones((n, n), dtype=torch.bool, device="cuda"), 1)
    l_nan, lb_nan = chol.l.clone(), lb.clone()
    l_nan[upper] = float("nan")
    lb_nan[upper] = float("nan")
    got = hip_backend.potrf_vjp(l_nan, dsb, sb, lb_nan)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, clean), "NaN above the diagonals changed the result"
    assert _err(got, ref) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [129, 1000])
def test_c_entry_padded_and_offset_views(hip_backend, dtype, n):
    """Padded ``ld`` / ``ldlb`` / ``lda`` and views that start inside a larger buffer: the result is the contiguous call's, and a
    sentinel everywhere outside the n x n view of ``abar`` stays."""
    lib = hip_backend.lib
    _, lbar, ref = _reference(n)
    chol = _chol_of(n, dtype, pad=24)                      # (ld = n + 24)
    sb, dsb = chol._blocks(n)
    assert chol.l.stride(0) == n + 24
    lbuf = torch.full((n + 3, n + 7), float("nan"), dtype=dtype, device="cuda")
    lb = lbuf[2: 2 + n, 5: 5 + n]
    lb.copy_(lbar.to(dtype))
    abuf = torch.full((n + 4, n + 9), -7.0, dtype=dtype, device="cuda")
    ab = abuf[3: 3 + n, 1: 1 + n]
    ws = torch.empty((int(lib.gpk_potrf_vjp_ws_elems(n, sb)),), dtype=dtype, device="cuda")
    assert _call(lib, chol.l, n, chol.l.stride(0), dsb, sb, lb, lb.stride(0), ab, ab.stride(0), ws) == 0
    first = ab.clone()
    assert _call(lib, chol.l, n, chol.l.stride(0), dsb, sb, lb, lb.stride(0), ab, ab.stride(0), ws) == 0
    assert torch.equal(ab, first), "a repeated call differs"
    assert torch.equal(ab, ab.T)
    assert _err(ab, ref) <= TOL[dtype]
    outside = torch.ones_like(abuf, dtype=torch.bool)
    outside[3: 3 + n, 1: 1 + n] = False
    assert bool((abuf[outside] == -7.0).all()), "the call wrote outside the n x n view of abar"
    assert bool(torch.isnan(lbuf[0]).all()) and bool(torch.isnan(lbuf[:, :5]).all()), "the call wrote into lbar's buffer"
    # the same through the backend on contiguous operands
    assert torch.equal(hip_backend.potrf_vjp(chol.l, dsb, sb, lb.contiguous()), first)


def test_argument_codes_and_version(hip_backend):
    lib = hip_backend.lib
    assert lib.gpk_version() >= 110
    n = 130
    chol = _chol_of(129, torch.float64)
    sb, dsb = chol._blocks(129)
    l = torch.eye(n, dtype=torch.float64, device="cuda")
    lb = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    ab = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    ws = torch.empty((int(lib.gpk_potrf_vjp_ws_elems(n, 128)),), dtype=torch.float64, device="cuda")
    assert lib.gpk_potrf_vjp_ws_elems(n, 128) == 3 * n * 144 + 128 * n
    assert lib.gpk_potrf_vjp_ws_elems(0, 128) == 0 and lib.gpk_potrf_vjp_ws_elems(n, 100) == 0
    ok = dict(l=l, n=n, ld=n, dsb=dsb, sb=128, lbar=lb, ldlb=n, abar=ab, lda=n, ws=ws)

    def code(**kw):
        a = dict(ok, **kw)
        return _call(lib, a["l"], a["n"], a["ld"], a["dsb"], a["sb"], a["lbar"], a["ldlb"], a["abar"], a["lda"], a["ws"], a.get("dtype"))

    assert code(dtype=7) == -1
    assert code(n=0) == 0 and code(n=-3) == 0
    assert code(n=0, l=None, dsb=None, lbar=None, abar=None, ws=None) == 0       # (an empty problem reads nothing)
    assert code(l=None) == -2
    assert code(n=(1 << 20) + 1, ld=1 << 21, ldlb=1 << 21, lda=1 << 21) == -3
    assert code(ld=n - 1) == -4
    assert code(dsb=None) == -5
    for bad in (0, 64, 100, 192, 8192):
        assert code(sb=bad) == -6
    assert code(lbar=None) == -7
    assert code(ldlb=n - 1) == -8
    assert code(abar=None) == -9
    assert code(lda=n - 1) == -10
    assert code(ws=None) == -11
    assert bool((ab == 0).all()), "a refused call wrote to abar"
