"""The kernel-gradient kernels (``gpk_kmat_vjp``, ``gpk_kmat_vjp_dense``, with and without shaped terms; ``stheno_amd/csrc/gpk_vjp.hip``) called
directly through ``HipBackend.kmat_vjp`` / ``kmat_vjp_dense`` and compared element by element with the extended-precision reference of
``tests/vjp_reference.py``, in fp64 and fp32, at the tile, chunk and dimension edges.

Acceptance, for every output element: ``|got - ref| <= c * eps(dtype) * absum``, with ``absum`` the sum of the absolute values of what is
added up for the element.  ``c`` (``BOUND``) is twice the worst figure measured with these cases on an MI355X (``profiles/README.md``,
"Kernel-gradient kernels, element by element") and never above 50, the figure the native self-test uses norm-wise.
``tests/test_vjp_reference_host.py`` shows, for every case here, that losing a tile, a partial tile, a partial chunk of input dimensions,
a column of A or a term moves an output by more than four times the bound at c = 50."""
import ctypes

import numpy as np
import pytest
import torch

from stheno_amd import _native, ops

from . import vjp_reference as R

pytestmark = pytest.mark.gpu

CAP = 50
#: twice the worst |got - ref| / (eps absum) measured per output and dtype
BOUND = {
    ("logdensity", "S", "float64"): 0.63, ("logdensity", "S", "float32"): 1.04,             # measured 0.312, 0.517
    ("logdensity", "trace", "float64"): 0.75, ("logdensity", "trace", "float32"): 0.65,     # 0.374, 0.322
    ("logdensity", "diag", "float64"): 1.05, ("logdensity", "diag", "float32"): 2.0,        # 0.523, 0.995
    ("dense", "S", "float64"): 1.8, ("dense", "S", "float32"): 2.87,                        # 0.899, 1.434
    ("dense", "colsum", "float64"): 3.82, ("dense", "colsum", "float32"): 3.9,              # 1.906, 1.948
    ("dense", "gradx", "float64"): 1.62, ("dense", "gradx", "float32"): 1.43,               # 0.808, 0.712
}
assert max(BOUND.values()) <= CAP
DTYPES = {"float64": torch.float64, "float32": torch.float32}


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.array(a), dtype=DTYPES[dtype], device="cuda")


def _kterms(terms):
    return ops.KTerms(*R.split_terms(terms))


def run_logdensity(be, case, dtype):
    """Worst ratio per output of one case: ``{output: max |got - ref| / (eps absum)}``."""
    inp, ref = R.reference(case)
    n = case["n"]
    kinv = np.array(inp["kinv"])
    if case.get("nan_upper"):
        kinv[np.triu_indices(n, 1)] = np.nan            # the strict upper triangle is not read
    if case.get("ldk_pad"):
        buf = torch.full((n, n + 7), float("nan"), dtype=DTYPES[dtype], device="cuda")
        kv = buf[:, :n]
        kv.copy_(_dev(kinv, dtype))
        assert kv.stride(0) > n
    else:
        kv = _dev(kinv, dtype)
    S, tr, dg = be.kmat_vjp(_kterms(inp["terms"]), _dev(inp["x"], dtype), kv, _dev(inp["alpha"], dtype), [float(v) for v in inp["g"]])
    got = {"S": S, "trace": tr, "diag": dg}
    out = {}
    for k, (val, ab) in ref.items():
        g = got[k].cpu().numpy()
        assert g.shape == np.shape(val), (k, g.shape, np.shape(val))
        out[k] = float(np.max(R.ratios(g, val, ab, dtype)))
    return out


def run_dense(be, case, dtype):
    inp, ref = R.reference(case)
    n, m = case["n"], case["m"]
    x = _dev(inp["x"], dtype)
    y = x if case.get("y_is_x") else _dev(inp["y"], dtype)
    if case.get("padded"):
        buf = torch.full((n, m + 5), float("nan"), dtype=DTYPES[dtype], device="cuda")
        g = buf[:, :m]
        g.copy_(_dev(inp["g"], dtype))
        assert g.stride(0) == m + 5
    else:
        g = _dev(inp["g"], dtype)
    S, colsum, gradx = be.kmat_vjp_dense(_kterms(inp["terms"]), x, y, g, _dev(inp["colscale"], dtype), _dev(inp["w"], dtype),
                                         _dev(inp["b"], dtype), want_colsum=case["colsum"], want_gradx=case["gradx"])
    assert (colsum is not None) == case["colsum"] and (gradx is not None) == case["gradx"]
    got = {"S": S, "colsum": colsum, "gradx": gradx}
    out = {}
    for k, (val, ab) in ref.items():
        if got[k] is None:
            continue
        gk = got[k].cpu().numpy()
        assert gk.shape == np.shape(val), (k, gk.shape, np.shape(val))
        out[k] = float(np.max(R.ratios(gk, val, ab, dtype)))
    if any(len(t) > 3 for t in inp["terms"]):
        third = S.cpu().numpy()[:, 2]
        assert all(v == 0 for v, t in zip(third, inp["terms"]) if len(t) == 3), third       # kinds without a shape
    return out


def _accept(case, dtype, worst):
    print(f"{case['form']} {case['id']} {dtype}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BOUND[(case["form"], k, dtype)], (k, v)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", R.LOGDENSITY_CASES, ids=lambda c: c["id"])
def test_logdensity_form_element_by_element(hip_backend, case, dtype):
    _accept(case, dtype, run_logdensity(hip_backend, case, dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", [c for c in R.DENSE_CASES if c is not R.MULTI_TILE_CHUNK], ids=lambda c: c["id"])
def test_dense_form_element_by_element(hip_backend, case, dtype):
    _accept(case, dtype, run_dense(hip_backend, case, dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_dense_form_with_two_tiles_per_chunk(hip_backend, dtype):
    """33 x 65 tiles: two tiles per chunk (the loop the ELBO gradient at n = 200000, m = 4096 runs 64 times per workgroup), a last chunk
    of one tile, a last row tile of one row and a last column tile 4 wide."""
    case = R.MULTI_TILE_CHUNK
    rt, nc = ctypes.c_int64(), ctypes.c_int64()
    assert hip_backend.lib.gpk_kmat_vjp_dense_grid(case["n"], case["m"], ctypes.byref(rt), ctypes.byref(nc)) == 0
    ctiles = -(-case["m"] // R.TILE)
    assert rt.value == -(-case["n"] // R.TILE) and nc.value < ctiles, "chunks hold one tile: the case no longer covers the chunk loop"
    assert case["colsum"] and case["gradx"]
    _accept(case, dtype, run_dense(hip_backend, case, dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gradx_past_eight_dimensions_is_refused(hip_backend, dtype):
    x, y = torch.zeros((5, 9), dtype=DTYPES[dtype], device="cuda"), torch.zeros((7, 9), dtype=DTYPES[dtype], device="cuda")
    g = torch.ones((5, 7), dtype=DTYPES[dtype], device="cuda")
    with pytest.raises(RuntimeError, match="gpk_kmat_vjp_dense"):
        hip_backend.kmat_vjp_dense(ops.KTerms([("eq", 1.0, 1.0)]), x, y, g, want_gradx=True)
    S, _, gx = hip_backend.kmat_vjp_dense(ops.KTerms([("eq", 1.0, 1.0)]), x, y, g, want_gradx=False)
    assert gx is None and float(S[0, 0]) == 35.0


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_unshaped_terms_take_the_two_wide_rows_whatever_shapes_holds(hip_backend, dtype):
    """The launchers choose the instantiation from the term table, not from ``shapes``: with kinds that have no shape parameter a junk
    ``shapes`` array and ``NULL`` write the same bits into partial rows of ``2 * GPK_MAX_TERMS + 1`` elements, and nothing behind them
    (``partial`` is sized for the 3-wide rows and prefilled, so a launch of the shaped kernels would show in its tail)."""
    lib, T = hip_backend.lib, DTYPES[dtype]
    terms = ops.KTerms([("eq", 0.8, 1.1), ("linear", 0.5, 2.0)])
    kinds, var, ils, nt = terms.c_arrays()
    junk = (ctypes.c_double * 2)(7.0, 7.0)
    dt = _native.GPK_F64 if T == torch.float64 else _native.GPK_F32
    n = m = 65
    d, W2, W3, sentinel = 3, 2 * _native.MAX_TERMS + 1, 3 * _native.MAX_TERMS + 1, -12345.0
    rng = np.random.default_rng(11)
    x, y = (torch.as_tensor(rng.standard_normal((k, d)), dtype=T, device="cuda") for k in (n, m))
    kinv, g = (torch.as_tensor(rng.standard_normal(sh), dtype=T, device="cuda") for sh in ((n, n), (n, m)))
    alpha = torch.as_tensor(rng.standard_normal((n, 1)), dtype=T, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bits = lambda t: t.cpu().view(torch.int64 if T == torch.float64 else torch.int32)   # noqa: E731
    one = (ctypes.c_double * 1)(1.0)

    # log-density form: two 64-row tiles, 3 blocks of the lower triangle
    rows = int(lib.gpk_kmat_vjp_blocks(n))
    assert rows == 3
    got = []
    for sh in (junk, None):
        partial = torch.full((rows * W3,), sentinel, dtype=T, device="cuda")
        diag_g = torch.empty((n,), dtype=T, device="cuda")
        assert lib.gpk_kmat_vjp(dt, kinds, ils, sh, nt, p(x), n, d, d, p(kinv), n, p(alpha), 1, 1, one, p(partial), p(diag_g), stream) == 0
        assert bool((partial[rows * W2:] == sentinel).all()), "something was written behind the 2-wide rows"
        head = partial[: rows * W2].reshape(rows, W2)
        assert bool((head[:, : 2 * nt] != sentinel).all()) and bool((head[:, W2 - 1] != sentinel).all())     # sums and trace were written
        got.append((bits(partial), bits(diag_g)))
    assert all(torch.equal(a, b) for a, b in zip(*got))

    # explicit-cotangent form: 2 row tiles x 2 chunks
    rt, nc = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gpk_kmat_vjp_dense_grid(n, m, ctypes.byref(rt), ctypes.byref(nc)) == 0
    rt, nc = rt.value, nc.value
    assert (rt, nc) == (2, 2)
    rows = rt * nc
    got = []
    for sh in (junk, None):
        partial = torch.full((rows * W3,), sentinel, dtype=T, device="cuda")
        colsum = torch.full((rt, m), sentinel, dtype=T, device="cuda")
        gradx = torch.full((nc, n, d), sentinel, dtype=T, device="cuda")
        assert lib.gpk_kmat_vjp_dense(dt, kinds, var, ils, sh, nt, p(x), n, d, p(y), m, d, d, p(g), m, None, None, None,
                                      p(partial), p(colsum), p(gradx), stream) == 0
        assert bool((partial[rows * W2:] == sentinel).all()), "something was written behind the 2-wide rows"
        assert bool((partial[: rows * W2] != sentinel).all()) and bool((colsum != sentinel).all()) and bool((gradx != sentinel).all())
        got.append((bits(partial), bits(colsum), bits(gradx)))
    assert all(torch.equal(a, b) for a, b in zip(*got))
