"""``gpk_kmat_scaled`` element by element: ``out (+)= rs_i cs_j k(x_i, y_j)`` through ``HipBackend.kmat_scaled`` and through the C entry,
in fp64 and fp32, against the value contract of ``include/gpk.h``: with ``K`` from ``HipBackend.kmat`` on the same arguments, every
element outside the diagonal of a non-accumulating launch has the BITS of ``(K * rs[:, None]) * cs[None, :]`` formed by torch in the
launch's dtype (NaN patterns equal); an element that receives an addition ``a`` (the diagonal of a symmetric launch, every element of an
accumulating one) lies within ``eps (|v| + |a|)`` of ``v + a`` -- the one rounding a fused multiply-add saves.

Shapes ``(n, m, d)`` -- tile rows are 32, ``TN`` columns per tile (128 in fp64, 256 in fp32: 64 lanes x one 16-byte store): the
smallest launch; one short of and one past both tile edges at the staged widths 4 and 8; a ragged last column tile; the one-tile kernel
with two and three dimension chunks; the compact lower-triangle grid; a batch large enough that a workgroup walks two column tiles with
the next tile's column factors in flight.  Term tables from ``tests/vjp_reference.TERMSETS`` so that every program is launched."""
import ctypes

import numpy as np
import pytest
import torch

from stheno_amd import _native, ops

from . import vjp_reference as R

pytestmark = pytest.mark.gpu

DTYPES = {"float64": torch.float64, "float32": torch.float32}
TN = {"float64": 128, "float32": 256}
EPS = {"float64": 2.0 ** -52, "float32": 2.0 ** -23}
INT = {"float64": torch.int64, "float32": torch.int32}
NAN = float("nan")
SENTINEL = -12345.0

TERMS = {"eq": R.TERMSETS["eq"], "eq_linear": R.TERMSETS["eq"] + R.TERMSETS["linear"], "matern32": R.TERMSETS["matern32"],
         "rq": R.TERMSETS["rq9"], "mix8": R.TERMSETS["mix8"], "mix8rq": R.TERMSETS["mix8rq"]}


def _shapes(dtype):
    tn = TN[dtype]
    return [(1, 1, 1), (31, tn - 1, 3), (33, tn + 1, 8), (65, 2 * tn + 3, 2), (33, tn + 1, 9), (33, tn + 1, 17)]


def _kterms(name):
    return ops.KTerms(*R.split_terms(TERMS[name]))


def _points(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.6 * torch.randn(shape, generator=g, dtype=torch.float64)).to(DTYPES[dtype]).cuda()


def _scale(shape, dtype, seed, nan=False):
    """Mixed signs, one exact 0 and, where asked, one NaN per vector."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(shape, generator=g, dtype=torch.float64).to(DTYPES[dtype])
    n = shape[-1]
    s[..., n // 3] = 0.0
    if nan and n > 2:
        s[..., (2 * n) // 3] = NAN
    return s.cuda()


def _expect(K, rs, cs):
    """``(K * rs[:, None]) * cs[None, :]`` by torch, in K's dtype; scales are ``(..., n)`` / ``(..., m)`` or None."""
    out = K
    if rs is not None:
        out = out * rs.unsqueeze(-1)
    if cs is not None:
        out = out * cs.unsqueeze(-2)
    return out


def _same_bits(got, ref, dtype, what):
    assert got.shape == ref.shape, what
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN patterns differ"
    a, b = torch.where(gn, 0, got.contiguous().view(INT[dtype])), torch.where(rn, 0, ref.contiguous().view(INT[dtype]))
    bad = int((a != b).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} elements differ in their bits"


def _within_one_rounding(got, v, a, dtype, what):
    """``|got - (v + a)| <= eps (|v| + |a|)`` in extended precision."""
    g, v, a = (np.asarray(t.detach().cpu().numpy(), dtype=np.longdouble) for t in (got, v, a))
    ok = np.isfinite(v)
    assert np.array_equal(np.isnan(g), np.isnan(v + a)), f"{what}: NaN patterns differ"
    dev, bar = np.abs(g - (v + a))[ok], (np.longdouble(EPS[dtype]) * (np.abs(v) + np.abs(a)))[ok]
    worst = float(np.max(dev / np.where(bar > 0, bar, 1))) if dev.size else 0.0
    print(f"{what}: worst |got - (v + a)| / (eps (|v| + |a|)) = {worst:.3f}")
    assert bool(np.all(dev <= bar)), (what, worst)


# ---- every program on every shape ------------------------------------------------------------
@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("shape", range(6))
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_scaled_launch_has_the_bits_of_the_two_multiplications(hip_backend, dtype, shape, terms):
    n, m, d = _shapes(dtype)[shape]
    kt = _kterms(terms)
    x, y = _points((n, d), dtype, 1), _points((m, d), dtype, 2)
    nan = shape == 2
    rs, cs = _scale((n,), dtype, 3, nan), _scale((m,), dtype, 4, nan)
    K = hip_backend.kmat(kt, x, y)
    for what, r, c in (("both", rs, cs), ("row only", rs, None), ("column only", None, cs), ("both NULL", None, None)):
        got = hip_backend.kmat_scaled(kt, x, y, r, c)
        _same_bits(got, _expect(K, r, c), dtype, f"{terms} {n}x{m}x{d} {what}")
    if nan:
        got = hip_backend.kmat_scaled(kt, x, y, rs, cs)
        bad = torch.isnan(got)
        assert bool(bad[(2 * n) // 3].all()) and bool(bad[:, (2 * m) // 3].all())
        keep = torch.ones_like(bad)
        keep[(2 * n) // 3], keep[:, (2 * m) // 3] = False, False
        assert not bool(bad[keep].any()), "a NaN scale reaches its row or column only"
    zero = hip_backend.kmat_scaled(kt, x, y, rs, cs)[n // 3]
    assert bool(((zero == 0) | torch.isnan(zero)).all()), "a zero scale gives exact zeros"


@pytest.mark.parametrize("terms", ["eq", "matern32", "mix8rq"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_accumulate_onto_a_prefilled_buffer(hip_backend, dtype, terms):
    n, m, d = _shapes(dtype)[3]
    kt = _kterms(terms)
    x, y = _points((n, d), dtype, 5), _points((m, d), dtype, 6)
    rs, cs = _scale((n,), dtype, 7), _scale((m,), dtype, 8)
    prev = _points((n, m), dtype, 9)
    out = prev.clone()
    res = hip_backend.kmat_scaled(kt, x, y, rs, cs, out=out, accumulate=True)
    assert res.data_ptr() == out.data_ptr()
    _within_one_rounding(out, _expect(hip_backend.kmat(kt, x, y), rs, cs), prev, dtype, f"accumulate {terms}")


# ---- the compact lower-triangle grid ------------------------------------------------------------
@pytest.mark.parametrize("terms", ["eq", "eq_linear", "mix8"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_symmetric_lower_only_with_diagonal_additions(hip_backend, dtype, terms):
    tn = TN[dtype]
    n, d = 3 * tn + 5, 4
    kt = _kterms(terms)
    x = _points((n, d), dtype, 11)
    s = _scale((n,), dtype, 12)
    dvec = _points((n,), dtype, 13).abs()
    dadd = 0.375
    out = torch.full((n, n), SENTINEL, dtype=DTYPES[dtype], device="cuda")
    hip_backend.kmat_scaled(kt, x, None, s, s, lower=True, diag_add=dadd, diag_vec=dvec, out=out)
    v = _expect(hip_backend.kmat(kt, x, None), s, s)
    rows, cols = torch.arange(n, device="cuda")[:, None], torch.arange(n, device="cuda")[None, :]
    written = (cols // tn) * tn <= (rows // 32) * 32 + 31            # tiles that touch the lower triangle
    off = written & (rows != cols)
    _same_bits(out[off], v[off], dtype, f"lower {terms}: elements off the diagonal")
    assert bool((out[~written] == SENTINEL).all()), "tiles above the diagonal stay untouched"
    # (the two additions, diag_add then diag_vec[i], as one `a` with |a| = |diag_add| + |diag_vec[i]|)
    g, vd, a = (np.asarray(t.cpu().numpy(), dtype=np.longdouble) for t in (torch.diagonal(out), torch.diagonal(v), dvec))
    dev, bar = np.abs(g - (vd + dadd + a)), np.longdouble(EPS[dtype]) * (np.abs(vd) + dadd + np.abs(a))
    print(f"lower {terms}: worst diagonal deviation / bar = {float(np.max(dev / bar)):.3f}")
    assert bool(np.all(dev <= bar))


# ---- a batch whose workgroups walk two column tiles ------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_large_batch_per_entry_and_shared_scales(hip_backend, dtype):
    tn = TN[dtype]
    B, n, m, d = 1536, 33, 2 * tn + 1, 3
    kt = _kterms("eq")
    x, y = _points((B, n, d), dtype, 21), _points((B, m, d), dtype, 22)
    K = hip_backend.kmat(kt, x, y)
    rs, cs = _scale((B, n), dtype, 23), _scale((B, m), dtype, 24)
    got = hip_backend.kmat_scaled(kt, x, y, rs, cs)
    _same_bits(got, _expect(K, rs, cs), dtype, "per-entry scales")
    del got
    got = hip_backend.kmat_scaled(kt, x, y, rs[7], cs[5])        # one vector shared by the batch: s_rs = s_cs = 0
    _same_bits(got, (K * rs[7][None, :, None]) * cs[5][None, None, :], dtype, "shared scales")


# ---- layouts ------------------------------------------------------------
def _carve(t, pad=3):
    """``t`` as a view into a NaN-filled buffer, ``pad`` elements more along every axis, offset by one."""
    buf = torch.full(tuple(s + pad for s in t.shape), NAN, dtype=t.dtype, device="cuda")
    view = buf[tuple(slice(1, 1 + s) for s in t.shape)]
    view.copy_(t)
    return view


@pytest.mark.parametrize("terms", ["eq", "mix8"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_offset_views_padded_rows_and_carved_inputs(hip_backend, dtype, terms):
    tn = TN[dtype]
    n, m, d = 65, 2 * tn + 3, 3
    kt = _kterms(terms)
    x, y = _points((n, d), dtype, 31), _points((m, d), dtype, 32)
    rs, cs = _scale((n,), dtype, 33), _scale((m,), dtype, 34)
    ref = _expect(hip_backend.kmat(kt, x, y), rs, cs)
    xc, yc = _carve(x), _carve(y)
    rc, cc = _carve(rs), _carve(cs)
    assert xc.stride(0) == d + 3 and rc.data_ptr() % 16 != 0
    # a view at an odd element offset (the scalar store path) with a padded leading dimension, in a sentinel-filled buffer
    big = torch.full((n + 4, m + 9), SENTINEL, dtype=DTYPES[dtype], device="cuda")
    view = big[2:2 + n, 5:5 + m]
    assert (view.data_ptr() % 16) != 0 and view.stride(0) == m + 9
    hip_backend.kmat_scaled(kt, xc, yc, rc, cc, out=view)
    _same_bits(view, ref, dtype, f"offset view {terms}")
    assert not bool(torch.isnan(view).any()), "no NaN from outside the carved inputs reaches the view"
    view.fill_(SENTINEL)
    assert bool((big == SENTINEL).all()), "nothing outside the view changed"
    # an aligned view with a padded leading dimension (the vector store path)
    pad = torch.full((n, m + 16 - m % 16 + 16), SENTINEL, dtype=DTYPES[dtype], device="cuda")
    hip_backend.kmat_scaled(kt, xc, yc, rc, cc, out=pad[:, :m])
    _same_bits(pad[:, :m], ref, dtype, f"padded rows {terms}")
    assert bool((pad[:, m:] == SENTINEL).all())


# ---- the C entry ------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _call(lib, dtype, kinds, var, ils, shapes, nt, x, n, y, m, d, rs, s_rs, cs, s_cs, out, batch=1, lower=0, symmetric=0, diag_add=0.0,
          diag_vec=None, accumulate=0):
    arr = lambda typ, v: None if v is None else (typ * max(len(v), 1))(*v)      # noqa: E731
    return lib.gpk_kmat_scaled(_native.GPK_F64 if dtype == "float64" else _native.GPK_F32, arr(ctypes.c_int, kinds),
                               arr(ctypes.c_double, var), arr(ctypes.c_double, ils), arr(ctypes.c_double, shapes), nt,
                               _p(x), n, d, n * d, _p(y), m, d, m * d, d, _p(rs), s_rs, _p(cs), s_cs, _p(out), m, n * m, batch, lower,
                               symmetric, diag_add, _p(diag_vec), n, accumulate, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_c_entry_values_and_argument_codes(hip_backend, dtype):
    lib = hip_backend.lib
    assert lib.gpk_version() >= 109
    tn = TN[dtype]
    B, n, m, d = 2, 33, tn + 1, 3
    x, y = _points((B, n, d), dtype, 41), _points((B, m, d), dtype, 42)
    rs, cs = _scale((B, n), dtype, 43), _scale((m,), dtype, 44)        # per-entry rows, shared columns
    kt = _kterms("rq")
    out = torch.full((B, n, m), SENTINEL, dtype=DTYPES[dtype], device="cuda")
    eq, rq = _native.K_EQ, _native.K_RQ
    args = dict(x=x, n=n, y=y, m=m, d=d, rs=rs, s_rs=n, cs=cs, s_cs=0, out=out, batch=B)
    assert _call(lib, dtype, [rq], [0.75], [1.0], [9.0], 1, **args) == 0
    _same_bits(out, _expect(hip_backend.kmat(kt, x, y), rs, cs[None].expand(B, m)), dtype, "C entry")
    both_null = dict(args, rs=None, cs=None, s_rs=0, s_cs=0)
    assert _call(lib, dtype, [rq], [0.75], [1.0], [9.0], 1, **both_null) == 0
    _same_bits(out, hip_backend.kmat(kt, x, y), dtype, "C entry, both NULL")
    # gpk_kmat's codes, unchanged: they stand for arguments in front of the four new ones
    assert _call(lib, dtype, [eq] * 9, [1.0] * 9, [1.0] * 9, None, 9, **args) == -4
    assert _call(lib, dtype, [99], [1.0], [1.0], None, 1, **args) == -1
    assert _call(lib, dtype, [rq], [1.0], [1.0], None, 1, **args) == -1
    assert _call(lib, dtype, [rq], [1.0], [1.0], [0.0], 1, **args) == -5
    assert _call(lib, dtype, [eq], [1.0], [1.0], None, 1, **dict(args, batch=65536)) == -6
    assert _call(lib, dtype, [eq], [1.0], [1.0], None, 1, **dict(args, d=-1)) == -13
    # an empty problem returns 0 and writes nothing
    out.fill_(SENTINEL)
    for empty in (dict(n=0), dict(m=0), dict(batch=0)):
        assert _call(lib, dtype, [eq], [1.0], [1.0], None, 1, **dict(args, **empty)) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
