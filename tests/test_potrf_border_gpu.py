"""``gpk_potrf_border`` (``include/gpk.h``) element by element on the device: the new rows of the factor, the whitened residual, the
128 x 128 diagonal-block inverses, what must not be written, reproducibility, ``info`` and the argument checks.

Matrices: ``A = k(x) + 0.1 I`` with ``EQ + Linear`` on ``x ~ 0.6 N(0, 1)``, D = 3, evaluated in fp64 on the host and rounded to the
dtype; ``L11`` from the existing ``potrf_``, ``V = L11^{-1} K12`` from the existing solve (``Chol.solve``: the GEMV sweep up to 8
columns, the blocked GEMM solve above).

Yardstick: with ``L`` a computed factor, ``rho = max over the new rows of |A - L L^T|_ij / (eps (|L| |L|^T)_ij)`` in ``longdouble``.
``rho0`` is that ratio for the factor the existing ``potrf_`` gives for the whole bordered matrix in the same run, ``BOUND[dtype]`` is
twice the worst ``rho0`` over the cases below on an MI355X (profiles/README.md, "Factor append"; twice: a border and a panel add in
different orders), never above ``n + q + 1`` -- Higham's gamma_{n+q+1} in units of eps, what ANY order of summation guarantees."""
import ctypes

import numpy as np
import pytest
import torch

from stheno_amd import matrix, ops

pytestmark = pytest.mark.gpu

#: twice the worst rho0 measured on an MI355X over SHAPES and LAYOUTS -- 20.211 in fp64, 20.414 in fp32, both at (n, q) = (130, 127)
#: (profiles/README.md, "Factor append", lists every case)
BOUND = {torch.float64: 2 * 20.211, torch.float32: 2 * 20.414}

SHAPES = [(1, 1), (127, 1), (128, 1), (130, 126), (130, 127), (200, 128), (384, 64), (1000, 5), (1000, 9), (4133, 16)]
LAYOUTS = [(130, 127, "ld"), (200, 128, "cap")]      # ld = n + q + 4 VEC;  a cap x cap buffer with cap > n + q
SENTINEL = 777.0


def _bordered(n, q, seed=0):
    rng = np.random.default_rng(1000 * n + q + seed)
    x = 0.6 * rng.standard_normal((n + q, 3))
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2) + x @ x.T + 0.1 * np.eye(n + q), rng


def _ratios(a, l_ld, rows, eps):
    """|A - L L^T| / (eps |L| |L|^T) on `rows`, in longdouble, zero above the diagonal; L (longdouble) lower triangular."""
    lr = l_ld[rows]
    num = np.abs(a[rows].astype(np.longdouble) - lr @ l_ld.T)
    den = eps * (np.abs(lr) @ np.abs(l_ld).T)
    mask = np.arange(l_ld.shape[0])[None, :] <= np.asarray(rows)[:, None]
    return np.where(mask, num / np.where(mask, den, 1), 0)


def _rho(a, l_ld, rows, eps):
    return float(np.max(_ratios(a, l_ld, rows, eps)))


def _run(be, n, q, dtype, layout=None, rhs=True, spoil=None):
    """One call of the entry on a fresh buffer.  Returns a dict of what went in and what came out (host copies)."""
    dev = torch.device("cuda")
    a64, rng = _bordered(n, q)
    if spoil is not None:
        a64[n + spoil, n + spoil] = 1e-3 * a64[n + spoil, n + spoil]
    a = torch.as_tensor(a64, dtype=dtype, device=dev)
    m = n + q
    vec = 2 if dtype == torch.float64 else 4
    rows, ld = (m, m)
    if layout == "ld":
        ld = m + 4 * vec
    elif layout == "cap":
        rows = ld = (m + 127) // 128 * 128 + 128
    buf = torch.full((rows, ld), SENTINEL, dtype=dtype, device=dev)
    buf[:n, :n] = torch.where(torch.ones(n, n, dtype=torch.bool, device=dev).tril(), a[:n, :n], buf[:n, :n])
    dinv11, info11 = be.potrf_(buf[:n, :n])
    assert int(info11[0]) == 0
    chol = matrix.Chol(buf[:n, :n], dinv11, info11)
    v = chol.solve(a[:n, n:].contiguous())
    buf[n:m, n:m] = torch.where(torch.ones(q, q, dtype=torch.bool, device=dev).tril(), a[n:, n:], buf[n:m, n:m])
    nblk, keep = (m + 127) // 128, n // 128
    dinv = torch.full((1, nblk, 128, 128), SENTINEL, dtype=dtype, device=dev)
    dinv[0, : dinv11.shape[1]] = dinv11[0]
    w1 = r2 = r2_in = None
    if rhs:
        r = torch.as_tensor(rng.standard_normal((m, 1)), dtype=dtype, device=dev)
        w1 = chol.solve(r[:n]).reshape(-1).contiguous()
        r2_in = r[n:, 0].clone()
        r2 = r2_in.clone()
    before_rows, before_dinv, before_buf = buf[:n].clone(), dinv[0, :keep].clone(), buf.clone()
    info = be.potrf_border(buf, n, q, v, dinv, w1, r2)
    torch.cuda.synchronize()
    return dict(a=a.cpu().numpy(), buf=buf.cpu().numpy(), before_buf=before_buf.cpu().numpy(), dinv=dinv[0].cpu().numpy(), info=int(info[0]),
                rows_same=torch.equal(buf[:n], before_rows), dinv_same=torch.equal(dinv[0, :keep], before_dinv), v=v.cpu().numpy(),
                w1=None if w1 is None else w1.cpu().numpy(), r2_in=None if r2 is None else r2_in.cpu().numpy(),
                w2=None if r2 is None else r2.cpu().numpy(), keep=keep, nblk=nblk)


_yardstick = {}


def _rho0(be, n, q, dtype):
    """rho of the new rows for the factor the EXISTING potrf_ gives for the whole bordered matrix (computed once per case)."""
    key = (n, q, dtype)
    if key not in _yardstick:
        a64, _ = _bordered(n, q)
        a = torch.as_tensor(a64, dtype=dtype, device="cuda")
        l = a.clone()
        _, info = be.potrf_(l)
        assert int(info[0]) == 0
        ld = np.longdouble
        _yardstick[key] = _rho(a.cpu().numpy(), np.tril(l.cpu().numpy()).astype(ld), np.arange(n, n + q), float(torch.finfo(dtype).eps))
    return _yardstick[key]


def _check(be, n, q, dtype, layout=None):
    eps = float(torch.finfo(dtype).eps)
    ld = np.longdouble
    m = n + q
    out = _run(be, n, q, dtype, layout)
    assert out["info"] == 0
    bound = min(BOUND[dtype], m + 1)
    lt = np.tril(out["buf"][:m, :m]).astype(ld)
    part = _ratios(out["a"], lt, np.arange(n, m), eps)
    rho = float(part.max())
    rho0 = _rho0(be, n, q, dtype)
    print(f"potrf_border {str(dtype)[6:]} n={n} q={q} layout={layout}: rho={rho:.3f} rho0={rho0:.3f} bound={bound:.3f}")
    print(f"    of which columns < n (L21 = V^T: the solve's residual): {float(part[:, :n].max()):.3f}; columns >= n (L22): "
          f"{float(part[:, n:].max()):.3f}")
    # what must not be written: the old rows (their sentinel-filled upper triangle and padding included), the new rows' padding
    # columns, the rows behind the grown factor, the blocks of dinv below n / 128
    assert out["rows_same"] and out["dinv_same"]
    assert np.array_equal(out["buf"][n:m, m:], out["before_buf"][n:m, m:]) and np.array_equal(out["buf"][m:], out["before_buf"][m:])
    assert np.array_equal(out["buf"][n:m, :n], out["v"].T)          # L21 is V^T, bit for bit
    # the whitened residual of the new rows
    l21, l22 = lt[n:, :n], lt[n:, n:]
    inv22 = np.linalg.inv(l22.astype(np.float64)).astype(ld)
    for _ in range(2):                                              # (two Newton steps: the inverse to longdouble accuracy)
        inv22 = inv22 + inv22 @ (np.eye(q, dtype=ld) - l22 @ inv22)
    w1, r2 = out["w1"].astype(ld), out["r2_in"].astype(ld)
    want = inv22 @ (r2 - l21 @ w1)
    tol = bound * eps * (np.abs(inv22) @ (np.abs(r2) + np.abs(l21) @ np.abs(w1)))
    err = np.abs(out["w2"].astype(ld) - want)
    print(f"    w2: worst error / tolerance = {float(np.max(err / tol)):.3f}")
    # the diagonal-block inverses of the grown factor, identity-padded
    worst = 0.0
    for g in range(out["keep"], out["nblk"]):
        blk = np.eye(128, dtype=ld)
        nv = min(128, m - 128 * g)
        blk[:nv, :nv] = lt[128 * g : 128 * g + nv, 128 * g : 128 * g + nv]
        d = out["dinv"][g].astype(ld)
        res, scale = np.abs(d @ blk - np.eye(128, dtype=ld)), eps * (np.abs(d) @ np.abs(blk))
        assert np.all(res[scale == 0] == 0) and np.all(np.triu(d, 1) == 0)
        worst = max(worst, float(np.max(res[scale > 0] / scale[scale > 0])))
        assert np.array_equal(d[nv:, nv:], np.eye(128 - nv, dtype=ld)) and np.all(d[nv:, :nv] == 0)
    print(f"    dinv: worst |D L - I| / (eps |D| |L|) = {worst:.3f}")
    assert rho <= bound, (rho, rho0, bound)
    assert np.all(err <= tol), float(np.max(err / tol))
    assert worst <= bound, (worst, bound)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,q", SHAPES)
def test_border_contract(hip_backend, n, q, dtype):
    _check(hip_backend, n, q, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,q,layout", LAYOUTS)
def test_border_contract_in_padded_buffers(hip_backend, n, q, layout, dtype):
    _check(hip_backend, n, q, dtype, layout)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_two_calls_write_the_same_bits(hip_backend, dtype):
    a, b = (_run(hip_backend, 1000, 9, dtype) for _ in range(2))
    assert np.array_equal(a["buf"], b["buf"]) and np.array_equal(a["dinv"], b["dinv"]) and np.array_equal(a["w2"], b["w2"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,q,row", [(130, 40, 17), (200, 128, 0), (127, 1, 0)])
def test_a_non_positive_pivot_reports_its_order(hip_backend, n, q, row, dtype):
    # K22[row][row] a thousandth of its value: far below what the rows before it explain of it, so the pivot is negative whatever
    # the rounding
    out = _run(hip_backend, n, q, dtype, rhs=False, spoil=row)
    assert out["info"] == n + row + 1
    assert out["rows_same"] and out["dinv_same"]


def test_without_a_residual_the_factor_is_the_same(hip_backend):
    a, b = _run(hip_backend, 384, 64, torch.float64), _run(hip_backend, 384, 64, torch.float64, rhs=False)
    assert np.array_equal(a["buf"], b["buf"]) and np.array_equal(a["dinv"], b["dinv"])


def test_version_workspace_and_argument_errors(hip_backend):
    lib = hip_backend.lib
    assert lib.gpk_version() >= 112
    assert lib.gpk_potrf_border_ws_elems(1000, 9) > 0
    assert lib.gpk_potrf_border_ws_elems(0, 9) == 0 and lib.gpk_potrf_border_ws_elems(10, 0) == 0 and lib.gpk_potrf_border_ws_elems(10, 129) == 0
    n, q = 20, 4
    t = torch.zeros((n + q, n + q), dtype=torch.float64, device="cuda")
    info = torch.zeros((1,), dtype=torch.int32, device="cuda")
    p, null = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(0)
    ip = ctypes.c_void_p(info.data_ptr())
    good = dict(dtype=1, a=p, n=n, q=q, ld=n + q, v=p, ldv=q, dinv=p, w1=p, r2=p, info=ip, ws=p)

    def call(**kw):
        g = dict(good, **kw)
        return lib.gpk_potrf_border(g["dtype"], g["a"], g["n"], g["q"], g["ld"], g["v"], g["ldv"], g["dinv"], g["w1"], g["r2"], g["info"], g["ws"], null)

    assert call(dtype=7) == -1
    assert call(a=null) == -2
    assert call(n=0) == -3
    assert call(q=0) == -4 and call(q=129, ld=n + 129) == -4
    assert call(ld=n + q - 1) == -5
    assert call(v=null) == -6
    assert call(ldv=q - 1) == -7
    assert call(dinv=null) == -8
    assert call(w1=null) == -9
    assert call(r2=null) == -10
    assert call(info=null) == -11
    assert call(ws=null) == -12
    torch.cuda.synchronize()
    assert not t.any() and int(info[0]) == 0            # (nothing was launched)
