"""Derivative blocks of the kernel matrix on the MI355X: ``HipBackend.kmat_diff`` (``gpk_kmat_diff``) element by element against the
longdouble reference of ``tests/diff_reference.py``, and ``f.diff(dim)`` end to end on the HIP backend.

Shapes are the smallest at which the tiling can go wrong: tiles are 32 rows by 128 (fp64) / 256 (fp32) columns, so ``(33, 65)`` has a
second row band and partial tiles, ``(97, 259)`` a second column tile in both dtypes (the band walk's double-buffered Y staging);
``d <= 8`` takes the row-band kernel, ``d = 9`` the chunked one-tile kernel (the switch the release library offers; the native
self-test, ``gpk_selftest --diff``, forces each through the development knob as well).  A workgroup walks more than one column tile,
and the lower triangle goes onto the compact 1-D grid, only when the launch is large: the two cases at the end reach both with batches.

Value bound: ``|got - ref| <= C eps absum`` element by element, ``absum`` as defined in ``tests/diff_reference.py``; ``C`` =
``VALUE_BOUND`` is twice the worst ratio measured with these cases on an MI355X (``profiles/README.md``, "Derivative kernel").  Inputs
are fp32-representable, so one reference serves both dtypes."""
import functools

import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import ops

from . import diff_reference as D

pytestmark = pytest.mark.gpu

DTYPES = {"float64": torch.float64, "float32": torch.float32}
#: twice the worst |got - ref| / (eps absum) measured over every case of this file (profiles/README.md, "Derivative kernel")
VALUE_BOUND = {"float64": 4.50, "float32": 4.60}                                            # measured 2.249, 2.298
SHAPES = [(1, 1), (33, 65), (97, 259)]
DIMS = [1, 3, 8, 9]
MODES = {"dx": lambda a, b: (a, None), "dy": lambda a, b: (None, b), "dxy": lambda a, b: (a, b)}


def dev(a, dtype):
    return None if a is None else torch.as_tensor(np.array(a, dtype=np.float64), dtype=DTYPES[dtype], device="cuda")


def r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def dimsets(d):
    return [(0, 0)] if d == 1 else [(0, 0), (d - 1, 0), (0, d - 1), (d - 1, d - 1)]


@functools.lru_cache(maxsize=None)
def case(name, n, m, d, a, b, coincident=False, seed=0):
    """Inputs (fp32-representable) and the reference of one case, computed once for both dtypes and never modified."""
    x, y = (r32(v) for v in D.inputs(n, m, d, seed=seed))
    if coincident:
        y[::3] = x[(np.arange(0, m, 3) * 7) % n]
    ref = D.diff_matrices(*D.TABLES[name], x, y, a, b)
    for v in (x, y) + tuple(w for pair in ref.values() for w in pair):
        v.setflags(write=False)
    return x, y, ref


def accept(what, got, val, ab, dtype):
    """The figure is printed, then asserted."""
    g = got.double().cpu().numpy()
    assert g.shape == np.shape(val), (what, g.shape, np.shape(val))
    w = float(np.max(D.ratios(g, val, ab, dtype)))
    print(f"{what} {dtype}: worst |got - ref| / (eps absum) = {w:.3f}")
    assert w <= VALUE_BOUND[dtype], (what, w)
    return w


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", list(D.TABLES))
def test_values(hip_backend, name, d, dtype):
    kt = ops.KTerms(*D.TABLES[name])
    for n, m in SHAPES:
        for a, b in dimsets(d):
            x, y, ref = case(name, n, m, d, a, b)
            tx, ty = dev(x, dtype), dev(y, dtype)
            for mode, dims in MODES.items():
                got = hip_backend.kmat_diff(kt, tx, ty, *dims(a, b))
                accept(f"kmat_diff {name} {mode} {n}x{m} d{d} dims ({a}, {b})", got, *ref[mode], dtype)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9], ids=["d3-row-band", "d9-tile"])
@pytest.mark.parametrize("name", ["eq", "matern32", "rq0.7"])
def test_coincident_points(hip_backend, name, d, dtype):
    """``y`` holds rows of ``x``: the one-sided blocks of a stationary table are exactly 0 there, the mixed block is the ``elwise``
    constant (same dimension) or exactly 0 (different dimensions), nothing is NaN -- Matern32's ``kappa''`` is singular at distance 0."""
    n, m = 33, 65
    terms, shapes = D.TABLES[name]
    kt = ops.KTerms(terms, shapes)
    cols = np.arange(0, m, 3)
    rows = (cols * 7) % n
    const = float(D.elwise_constant(terms))
    for a, b in [(d - 1, d - 1), (0, d - 1)]:
        x, y, ref = case(name, n, m, d, a, b, coincident=True)
        tx, ty = dev(x, dtype), dev(y, dtype)
        for mode, dims in MODES.items():
            got = hip_backend.kmat_diff(kt, tx, ty, *dims(a, b))
            assert not bool(torch.isnan(got).any()), (mode, a, b)
            accept(f"kmat_diff {name} {mode} coincident d{d} dims ({a}, {b})", got, *ref[mode], dtype)
            at = got.double().cpu().numpy()[rows, cols]
            if mode != "dxy" or a != b:
                assert np.all(at == 0.0), (mode, a, b, at)
            else:
                assert np.max(np.abs(at - const)) <= VALUE_BOUND[dtype] * float(D.EPS[dtype]) * abs(const), (at, const)
    k = {"eq": st.EQ(), "matern32": st.Matern32(), "rq0.7": st.RQ(0.7)}[name].stretch(terms[0][2]) * terms[0][1]
    el = k.diff(d - 1).elwise(dev(case(name, n, m, d, 0, 0)[0], dtype))
    assert el.shape == (n, 1) and float((el.double() - const).abs().max()) <= 4 * float(D.EPS[dtype]) * abs(const)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9], ids=["d3-row-band", "d9-tile"])
def test_nan_inputs(hip_backend, d, dtype):
    n, m, a, b = 33, 65, d - 1, 0
    x, y, ref = case("all8", n, m, d, a, b)
    kt = ops.KTerms(*D.TABLES["all8"])
    xn, yn = np.array(x), np.array(y)
    xn[7, 1 if d > 1 else 0] = np.nan
    yn[40, 0] = np.nan
    for mode, dims in MODES.items():
        got = hip_backend.kmat_diff(kt, dev(xn, dtype), dev(yn, dtype), *dims(a, b))
        nan = torch.isnan(got).cpu().numpy()
        want = np.zeros((n, m), dtype=bool)
        want[7, :] = True
        want[:, 40] = True
        assert np.array_equal(nan, want), mode
        keep = ~want
        val, ab = ref[mode]
        w = float(np.max(D.ratios(got.double().cpu().numpy()[keep], val[keep], ab[keep], dtype)))
        assert w <= VALUE_BOUND[dtype], (mode, w)


# ---------------------------------------------------------------------------------------------
# the options gpk_kmat_diff shares with gpk_kmat
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9], ids=["d3-row-band", "d9-tile"])
def test_symmetric_lower_only_with_diagonal_additions(hip_backend, d, dtype):
    n, a = 130, d - 1
    x, _, _ = case("all8", n, 1, d, a, a)
    kt = ops.KTerms(*D.TABLES["all8"])
    val, ab = D.diff_matrices(*D.TABLES["all8"], x, x, a, a)["dxy"]
    dv = (np.arange(n) % 16) / 8.0
    val, ab = val + np.diag(0.25 + dv), ab + np.diag(0.25 + dv)
    tx = dev(x, dtype)
    full = hip_backend.kmat_diff(kt, tx, None, a, a, diag_add=0.25, diag_vec=dev(dv, dtype))
    accept(f"kmat_diff all8 symmetric {n} d{d}", full, val, ab, dtype)
    low = hip_backend.kmat_diff(kt, tx, None, a, a, lower=True, diag_add=0.25, diag_vec=dev(dv, dtype))
    assert torch.equal(torch.tril(low), torch.tril(full))
    # the full matrix against its own transpose, element by element (the diagonal additions are on the diagonal only)
    g = full.double().cpu().numpy()
    w = float(np.max(D.ratios(g, g.T.astype(D.LD), ab, dtype)))
    print(f"kmat_diff all8 symmetric {n} d{d} {dtype}: worst |full - full^T| / (eps absum) = {w:.3f}")
    assert w <= VALUE_BOUND[dtype], w
    # two different dimensions are not symmetric: refused by the library, with the `symmetric` argument's number
    if d > 1:
        with pytest.raises(RuntimeError, match="status -23"):
            hip_backend.kmat_diff(kt, tx, None, 0, a)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9], ids=["d3-row-band", "d9-tile"])
def test_accumulate_strided_view_and_batch(hip_backend, d, dtype):
    n, m, a, b = 33, 65, d - 1, 0
    x, y, ref = case("all8", n, m, d, a, b)
    kt = ops.KTerms(*D.TABLES["all8"])
    tx, ty = dev(x, dtype), dev(y, dtype)
    for mode, dims in MODES.items():
        val, ab = ref[mode]
        # accumulate into what is there
        base = (np.arange(n * m).reshape(n, m) % 7 - 3).astype(np.float64)
        acc = dev(base, dtype)
        hip_backend.kmat_diff(kt, tx, ty, *dims(a, b), out=acc, accumulate=True)
        accept(f"kmat_diff all8 {mode} accumulate d{d}", acc, val + base, ab + np.abs(base), dtype)
        # a view with an odd offset (73 elements) and an odd leading dimension (71): the pointer is off the 16-byte grid and
        # `ld % VEC != 0` in both dtypes -- the scalar store path; the rest of the buffer stays untouched
        buf = torch.full((n + 2, m + 6), -7.0, dtype=DTYPES[dtype], device="cuda")
        view = buf[1:n + 1, 2:m + 2]
        out = hip_backend.kmat_diff(kt, tx, ty, *dims(a, b), out=view)
        assert out.data_ptr() == view.data_ptr() and out.stride(0) == 71 and view.storage_offset() == 73
        accept(f"kmat_diff all8 {mode} strided view d{d}", view, val, ab, dtype)
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[1:n + 1, 2:m + 2] = False
        assert bool((buf[mask] == -7.0).all())
    # a batch of 3 with batch strides: inputs and output are the leading rows of taller buffers
    xb, yb = (r32(v) for v in D.inputs(n, m, d, seed=1, batch=3))
    refs = [D.diff_matrices(*D.TABLES["all8"], xb[i], yb[i], a, b)["dxy"] for i in range(3)]
    wide = torch.zeros((3, n + 4, m), dtype=DTYPES[dtype], device="cuda")
    xw = torch.full((3, n + 2, d), float("nan"), dtype=DTYPES[dtype], device="cuda")
    yw = torch.full((3, m + 3, d), float("nan"), dtype=DTYPES[dtype], device="cuda")
    xw[:, :n], yw[:, :m] = dev(xb, dtype), dev(yb, dtype)
    assert xw[:, :n].stride(0) == (n + 2) * d and yw[:, :m].stride(0) == (m + 3) * d
    got = hip_backend.kmat_diff(kt, xw[:, :n], yw[:, :m], a, b, out=wide[:, :n])
    assert got.data_ptr() == wide.data_ptr() and bool((wide[:, n:] == 0).all())
    accept(f"kmat_diff all8 dxy batch=3 d{d}", got, np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs]), dtype)


def test_error_codes(hip_backend):
    """The argument codes of ``include/gpk.h`` as the binding reports them (the codes themselves: ``tests/test_diff_host.py``, no device)."""
    x = dev(np.zeros((4, 3)), "float64")
    eq = ops.KTerms([("eq", 1.0, 1.0)])
    for dims, code in (((3, 0), -7), ((None, None), -7), ((0, 3), -8)):
        with pytest.raises(RuntimeError, match=f"status {code}$"):
            hip_backend.kmat_diff(eq, x, x, *dims)
    for terms, shapes in (([("matern12", 1.0, 1.0)], None), ([("eq", 1.0, 1.0), ("delta", 1.0, 1.0)], [None, 1e-6])):
        with pytest.raises(RuntimeError, match="status -2$"):
            hip_backend.kmat_diff(ops.KTerms(terms, shapes), x, x, 0, 0)
    with pytest.raises(RuntimeError, match="status -23$"):
        hip_backend.kmat_diff(eq, x, x, 0, None, lower=True)


# ---------------------------------------------------------------------------------------------
# launch plans with more than one column tile per workgroup: the launcher gives a workgroup CT > 1 tiles only once the grid holds 6144
# workgroups without them, so these cases are batches of many small matrices whose entries repeat three different ones.  They are
# compared bit for bit with the same three matrices launched as a batch of 3 (CT = 1, one tile per pass: the path of every case
# above); tests/test_kmat_plan.py asserts that the launcher's arithmetic gives these shapes the plans named here.
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def three(n, m, d):
    """Three fp32-representable input pairs, never modified."""
    xb, yb = (r32(v) for v in D.inputs(n, m, d, seed=2, batch=3))
    xb.setflags(write=False)
    yb.setflags(write=False)
    return xb, yb


def repeated(a, batch, dtype):
    """A batch whose entry ``b`` is entry ``b % 3`` of ``a``."""
    return dev(a, dtype)[torch.arange(batch, device="cuda") % 3].contiguous()


@pytest.mark.parametrize("dtype,m", [("float64", 259), ("float32", 600)])
def test_walk_of_several_column_tiles(hip_backend, dtype, m):
    """``gy * batch = 4 * 1536 = 6144``: CT = 8, and the workgroup walks the 3 column tiles of its band, the last one ragged -- the
    double-buffered Y staging with the next tile's fetch under this tile's arithmetic."""
    n, d, a, b, batch = 97, 3, 2, 0, 1536
    xb, yb = three(n, m, d)
    kt = ops.KTerms(*D.TABLES["all8"])
    small = hip_backend.kmat_diff(kt, dev(xb, dtype), dev(yb, dtype), a, b)
    refs = [D.diff_matrices(*D.TABLES["all8"], xb[i], yb[i], a, b)["dxy"] for i in range(3)]
    accept(f"kmat_diff all8 dxy batch=3 {n}x{m} d{d}", small, np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs]), dtype)
    got = hip_backend.kmat_diff(kt, repeated(xb, batch, dtype), repeated(yb, batch, dtype), a, b)
    assert got.shape == (batch, n, m)
    assert bool((got.reshape(batch // 3, 3, n, m) == small).all())


@pytest.mark.parametrize("dtype,n", [("float64", 300), ("float32", 600)])
def test_compact_grid_with_two_tiles_per_workgroup(hip_backend, dtype, n):
    """Lower triangle of a batch of 640 symmetric blocks: CT = 8 and 4 leave fewer than 6144 workgroups, CT = 2 does not, and two column
    chunks per row band put the launch on the compact 1-D grid (8 / 16 row bands per chunk).  Against the lower triangle of the full
    matrices of a batch of 3."""
    d, a, batch = 3, 2, 640
    xb, _ = three(n, 1, d)
    kt = ops.KTerms(*D.TABLES["all8"])
    dv = (np.arange(3 * n).reshape(3, n) % 16) / 8.0
    full = hip_backend.kmat_diff(kt, dev(xb, dtype), None, a, a, diag_add=0.25, diag_vec=dev(dv, dtype))
    low = hip_backend.kmat_diff(kt, repeated(xb, batch, dtype), None, a, a, lower=True, diag_add=0.25, diag_vec=repeated(dv, batch, dtype))
    assert low.shape == (batch, n, n)
    upper = torch.ones((n, n), dtype=torch.bool, device="cuda").triu(1)
    for r in range(3):
        assert bool(((low[r::3] == full[r]) | upper).all()), r


# ---------------------------------------------------------------------------------------------
# end to end: values and slopes observed jointly (the case of tests/test_diff_host.py) on the HIP backend
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol,eps", [("float64", 1e-6, 1e-12), ("float32", 1e-3, 1e-6)])
def test_values_and_slopes_jointly(hip_backend, dtype, tol, eps):
    old = st.B.epsilon
    st.B.epsilon = eps             # (fp32: the jitter the README prescribes for that dtype)
    try:
        ref = D.joint_reference(*D.joint_data(), eps, dtype)
        D.check_joint(ref, *D.joint_model(), lambda a: dev(a, dtype), tol)
    finally:
        st.B.epsilon = old


def test_block_matrix_of_a_process_and_its_derivative_in_lower_mode(hip_backend):
    xf, xd, _, _, _ = D.joint_data()
    prior, f, d0, d1 = D.joint_model()
    with prior:
        joint = st.cross(f, d1)
    k = prior.kernels[joint]
    inp = (f(dev(xf, "float64")), d1(dev(xd, "float64")))
    full = k.pairwise(inp)
    low = k.pairwise(inp, lower=True)
    assert full.shape == (55, 55) and torch.equal(torch.tril(low), torch.tril(full))
    want = D.joint_reference(*D.joint_data(), 0.0)["K"] - D.NOISE * np.eye(55)
    assert float(np.max(np.abs(full.cpu().numpy() - want))) <= 1e-12 * float(np.max(np.abs(want)))
