"""The VJP of a derivative block (``gpk_kmat_diff_vjp``; ``stheno_amd/csrc/gpk_vjp.hip``) called directly through
``HipBackend.kmat_diff_vjp`` and compared element by element with the extended-precision reference of ``tests/diff_vjp_reference.py``, in
fp64 and fp32, at the tile, chunk and dimension edges, in all four modes.

Acceptance, for every output element: ``|got - ref| <= c * eps(dtype) * absum``, with ``absum`` the sum of the absolute values of what is
added up for the element.  ``c`` (``BOUND``) is twice the worst figure measured with these cases on an MI355X (``profiles/README.md``,
"Derivative-block gradient kernel, element by element") and never above 50, the project's cap.  ``tests/test_diff_vjp_host.py`` shows, for
every case here, that losing the last tile, a partial tile, a chunk of input dimensions, a term or the ``[a == b]`` addend moves an output
by more than four times the bound at c = 50."""
import ctypes

import numpy as np
import pytest
import torch

from stheno_amd import ops

from . import diff_vjp_reference as R

pytestmark = pytest.mark.gpu

CAP = 50
#: twice the worst |got - ref| / (eps absum) measured per output and dtype
BOUND = {
    ("S", "float64"): 2.29, ("S", "float32"): 2.07,                 # measured 1.142, 1.033
    ("gradx", "float64"): 4.44, ("gradx", "float32"): 6.92,         # 2.219, 3.457
}
assert max(BOUND.values()) <= CAP
DTYPES = {"float64": torch.float64, "float32": torch.float32}


def _dev(a, dtype):
    return torch.as_tensor(np.array(a), dtype=DTYPES[dtype], device="cuda")


def run_case(be, case, dtype):
    """Worst ratio per output of one case: ``{output: max |got - ref| / (eps absum)}``."""
    inp, ref = R.reference(case, dtype)
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
    want_gx = ref["gradx"] is not None
    S, gradx = be.kmat_diff_vjp(ops.KTerms(inp["terms"], inp["shapes"]), x, y, inp["a"], inp["b"], g, want_gradx=want_gx)
    assert (gradx is not None) == want_gx
    out = {}
    for k, got in (("S", S), ("gradx", gradx)):
        if got is None:
            continue
        val, ab = ref[k]
        gk = got.cpu().numpy()
        assert gk.shape == np.shape(val), (k, gk.shape, np.shape(val))
        out[k] = float(np.max(R.ratios(gk, val, ab, dtype)))
    third = S.cpu().numpy()[:, 2] if S.shape[1] == 3 else None
    if inp["shapes"] is None:
        assert third is None                                                   # no shaped term: the two-wide rows
    else:
        assert all(v == 0 for v, al in zip(third, inp["shapes"]) if al is None), third       # kinds without a shape: exactly 0
    return out


def _accept(case, dtype, worst):
    print(f"diff_vjp {case['id']} {dtype}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BOUND[(k, dtype)], (k, v)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", [c for c in R.CASES if c is not R.MULTI_TILE_CHUNK], ids=lambda c: c["id"])
def test_element_by_element(hip_backend, case, dtype):
    _accept(case, dtype, run_case(hip_backend, case, dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_two_tiles_per_chunk(hip_backend, dtype):
    """33 x 65 tiles: two tiles per chunk, a last chunk of one tile, a last row tile of one row and a last column tile 4 wide."""
    case = R.MULTI_TILE_CHUNK
    rt, nc = ctypes.c_int64(), ctypes.c_int64()
    assert hip_backend.lib.gpk_kmat_vjp_dense_grid(case["n"], case["m"], ctypes.byref(rt), ctypes.byref(nc)) == 0
    assert rt.value == -(-case["n"] // R.TILE) and nc.value < -(-case["m"] // R.TILE), "chunks hold one tile: the case no longer covers the chunk loop"
    _accept(case, dtype, run_case(hip_backend, case, dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_coincident_points_add_exactly_zero_for_matern32(hip_backend, dtype):
    """``y`` the same tensor as ``x``: on the diagonal Matern32's ``1 / s`` is taken as 0 and ``D_a = 0``, so a cotangent that lives on
    the diagonal alone gives exact zeros in the one-sided modes and off the diagonal of the mixed block."""
    x = _dev(R.round32(np.random.default_rng(5).uniform(-1, 1, (70, 3))), dtype)
    g = torch.eye(70, dtype=DTYPES[dtype], device="cuda")
    terms = ops.KTerms(*R.TABLES["matern32"])
    for a, b, gx in ((1, None, True), (None, 2, True), (0, 2, False)):
        S, gradx = hip_backend.kmat_diff_vjp(terms, x, x, a, b, g, want_gradx=gx)
        assert not bool(S.any()), (a, b, S)
        assert gradx is None or bool(torch.isfinite(gradx).all())
    S, _ = hip_backend.kmat_diff_vjp(terms, x, x, 1, 1, g)
    c = 1.0 / 1.25 ** 2
    assert abs(float(S[0, 0]) - 70 * 3.0 * c) <= 1e-5 * 70 * 3.0 * c          # -2 c kappa'(0) = 3 c on each of the 70 diagonal entries


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_refusals(hip_backend, dtype):
    x, y = torch.zeros((5, 9), dtype=DTYPES[dtype], device="cuda"), torch.zeros((7, 9), dtype=DTYPES[dtype], device="cuda")
    g = torch.ones((5, 7), dtype=DTYPES[dtype], device="cuda")
    eq = ops.KTerms([("eq", 1.0, 1.0)])
    with pytest.raises(RuntimeError, match="gpk_kmat_diff_vjp failed with status -19"):
        hip_backend.kmat_diff_vjp(eq, x, y, 0, None, g, want_gradx=True)                     # d > 8
    with pytest.raises(RuntimeError, match="gpk_kmat_diff_vjp failed with status -19"):
        hip_backend.kmat_diff_vjp(eq, x[:, :3], y[:, :3], 0, 1, g, want_gradx=True)          # the mixed block
    with pytest.raises(RuntimeError, match="gpk_kmat_diff_vjp failed with status -2"):
        hip_backend.kmat_diff_vjp(ops.KTerms([("matern12", 1.0, 1.0)]), x, y, 0, None, g)
    S, gx = hip_backend.kmat_diff_vjp(eq, x, y, 8, 8, g)
    assert gx is None and float(S[0, 0]) == 35.0 and float(S[0, 1]) == 35.0              # coincident: beta = c dbeta/dc = -2 c kappa'(0) = 1
