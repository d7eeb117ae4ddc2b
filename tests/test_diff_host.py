"""Host logic of derivative processes, ``f.diff(dim)``: the closed forms of the derivative blocks (``tests/diff_reference.py``) pinned
against torch double-backward, the reference's ``test_derivative``, a joint model of values and slopes against dense NumPy, the kernel
algebra of ``DiffKernel`` / ``DiffMean``, every refusal, the learnable-hyper-parameter guard and the argument codes of
``gpk_kmat_diff`` -- which need no GPU: the entry checks every argument before an empty problem returns.  The derivative blocks
themselves come from the NumPy ``kmat_diff`` of ``stheno_amd.ops._HostDelta`` here; on the MI355X: ``tests/test_diff_gpu.py``."""
import ctypes

import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import _native, kernels as K
from stheno_amd.torch import EQ, Delta, Linear, Matern12, Matern32, Matern52

from . import diff_reference as D
from .conftest import T


def np_(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------
# the closed forms against torch autograd (fp64 double-backward), one kind at a time
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eq", "matern32", "rq0.7", "eq+linear+const", "all8", "matern52"])
def test_closed_forms_against_torch_double_backward(name):
    terms, shapes = D.TABLES[name] if name in D.TABLES else ([("matern52", 0.75, 1.5)], None)
    x, y = D.inputs(7, 5, 3, seed=3)
    worst = 0.0
    for a, b in [(0, 0), (2, 0), (1, 2)]:
        ref = D.diff_matrices(terms, shapes, x, y, a, b)
        tx, ty = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, y))
        k = D.torch_kernel(terms, shapes, tx, ty)
        got = {k_: np.zeros((7, 5)) for k_ in ref}
        for i in range(7):
            for j in range(5):
                gx, gy = torch.autograd.grad(k[i, j], (tx, ty), create_graph=True)
                got["dx"][i, j], got["dy"][i, j] = float(gx[i, a].detach()), float(gy[j, b].detach())
                got["dxy"][i, j] = float(torch.autograd.grad(gx[i, a], ty, retain_graph=True)[0][j, b])
        for key, (val, ab) in ref.items():
            err = float(np.max(np.abs(got[key] - val) / ab))
            worst = max(worst, err)
            assert err <= 1e-12, (name, key, a, b, err)
    print(f"{name}: worst |closed form - autograd| / absum = {worst:.2e}")


def test_host_kmat_diff_matches_the_reference(oracle_backend):
    """The NumPy ``kmat_diff`` the CPU tests run on, all three modes, against the longdouble reference; coincident points included."""
    from stheno_amd import ops

    x, y = D.inputs(9, 11, 3, seed=5)
    y[3], y[7] = x[2], x[8]
    for name, (terms, shapes) in D.TABLES.items():
        kt = ops.KTerms(terms, shapes)
        ref = D.diff_matrices(terms, shapes, x, y, 2, 1)
        for key, dims in (("dx", (2, None)), ("dy", (None, 1)), ("dxy", (2, 1))):
            got = np_(ops.get_backend().kmat_diff(kt, T(x), T(y), *dims))
            assert not np.isnan(got).any()
            assert float(np.max(D.ratios(got, *ref[key], "float64"))) <= 8.0, (name, key)


# ---------------------------------------------------------------------------------------------
# the reference's test_derivative (tests/model/test_model.py:510-530)
# ---------------------------------------------------------------------------------------------
def test_derivative_as_in_the_reference(oracle_backend):
    p = st.GP(lambda x: x**2, EQ())
    assert str(p.diff(1)) == "GP(d(1) <lambda>, d(1) EQ())"

    dp = p.diff()
    x = torch.linspace(0, 1, 100, dtype=torch.float64)
    y = 2 * x
    x_check = torch.linspace(0.2, 0.8, 100, dtype=torch.float64)

    post = p.measure | (p(x), y)
    mean = np_(post(dp)(x_check).mean)
    assert mean.shape == (100, 1) and np.max(np.abs(mean - 2.0)) <= 1e-4

    zero = torch.tensor(0.0, dtype=torch.float64)
    post = p.measure | ((p(zero), zero), (dp(x), y))
    mean = np_(post(p)(x_check).mean)
    assert np.max(np.abs(mean - np_(x_check)[:, None] ** 2)) <= 1e-4


# ---------------------------------------------------------------------------------------------
# values and slopes observed jointly, D = 2, against dense NumPy
# ---------------------------------------------------------------------------------------------
def test_values_and_slopes_jointly_against_numpy(oracle_backend):
    ref = D.joint_reference(*D.joint_data(), st.B.epsilon)
    D.check_joint(ref, *D.joint_model(), T, 1e-8)


# ---------------------------------------------------------------------------------------------
# algebra
# ---------------------------------------------------------------------------------------------
def test_kernel_algebra(oracle_backend):
    k = 1.3 * EQ().stretch(0.7) + 0.5 * Matern52()
    with st.Measure() as m:
        f = st.GP(k)
        g = st.GP(Matern32())
        da, db = f.diff(0), f.diff(1)
    kab = m.kernels[da, db]
    assert isinstance(kab, K.DiffKernel) and kab.k is m.kernels[f] and (kab.dim_x, kab.dim_y) == (0, 1)
    kba = m.kernels[db, da]
    assert isinstance(kba, K.DiffKernel) and (kba.dim_x, kba.dim_y) == (1, 0)
    r = reversed(kab)
    assert isinstance(r, K.DiffKernel) and (r.dim_x, r.dim_y) == (1, 0) and r.k is kab.k
    kfa = m.kernels[f, da]
    assert isinstance(kfa, K.DiffKernel) and (kfa.dim_x, kfa.dim_y) == (None, 0)
    assert (m.kernels[da, f].dim_x, m.kernels[da, f].dim_y) == (0, None)
    assert m.kernels[da].terms() is None and repr(EQ().diff(1)) == "d(1) EQ()" and repr(EQ().diff(0, None)) == "d(0, None) EQ()"
    assert EQ().diff(None, None).terms() is not None              # nothing differentiated: the kernel itself
    # an independent process: no cross-covariance
    assert isinstance(m.kernels[da, g], K.ZeroKernel) and isinstance(m.kernels[g, da], K.ZeroKernel)
    assert isinstance(K.ZeroKernel().diff(0), K.ZeroKernel)
    # values: pairwise of the three kinds of block against the reference, elwise = the diagonal of pairwise
    terms, shapes = k.terms(), k.shapes()
    x, y = D.inputs(6, 4, 2, seed=9)
    ref = D.diff_matrices(terms, shapes, x, y, 0, 1)
    for kern, key in ((kab, "dxy"), (m.kernels[da, f], "dx"), (m.kernels[f, db], "dy")):
        assert float(np.max(D.ratios(np_(kern.pairwise(T(x), T(y))), *ref[key], "float64"))) <= 8.0
    for kern in (m.kernels[da], kab, m.kernels[da, f], (EQ() + 2.0 * Linear().stretch(2.0)).diff(1), (EQ() + Linear()).diff(None, 1),
                 (EQ() + Linear()).diff(1, None)):
        full = np_(kern.pairwise(T(x), T(x)))
        np.testing.assert_allclose(np_(kern.elwise(T(x)))[:, 0], np.diag(full), rtol=0, atol=1e-14)
    # (f + g).diff() and (2 f).diff()
    with st.Measure() as m2:
        f = st.GP(EQ())
        g = st.GP(Matern52().stretch(2.0))
        ds, d2 = (f + g).diff(0), (2.0 * f).diff(0)
    x1 = np.linspace(-1, 1, 5)[:, None]
    want = D.diff_matrices([("eq", 1.0, 1.0), ("matern52", 1.0, 2.0)], None, x1, x1, 0, 0)
    np.testing.assert_allclose(np_(m2.kernels[ds].pairwise(T(x1))), np.asarray(want["dxy"][0], dtype=np.float64), rtol=0, atol=1e-13)
    np.testing.assert_allclose(np_(m2.kernels[ds, g].pairwise(T(x1), T(x1))),
                               np.asarray(D.diff_matrices([("matern52", 1.0, 2.0)], None, x1, x1, 0, 0)["dx"][0], dtype=np.float64), rtol=0, atol=1e-13)
    want = D.diff_matrices([("eq", 1.0, 1.0)], None, x1, x1, 0, 0)
    np.testing.assert_allclose(np_(m2.kernels[d2].pairwise(T(x1))), 4 * np.asarray(want["dxy"][0], dtype=np.float64), rtol=0, atol=1e-13)
    np.testing.assert_allclose(np_(m2.kernels[d2, f].pairwise(T(x1), T(x1))), 2 * np.asarray(want["dx"][0], dtype=np.float64), rtol=0, atol=1e-13)
    # exports
    import stheno_amd

    assert stheno_amd.DiffKernel is K.DiffKernel and st.DiffKernel is K.DiffKernel and st.DiffMean is K.DiffMean


def test_per_dimension_length_scales(oracle_backend):
    scales = np.array([0.5, 2.0, 1.25])
    k = (1.5 * EQ() + 0.5 * Matern32()).stretch(scales)
    x, y = D.inputs(6, 5, 3, seed=4)
    terms = [("eq", 1.5, 1.0), ("matern32", 0.5, 1.0)]
    ref = D.diff_matrices(terms, None, x / scales, y / scales, 2, 0)
    for dims, key, factor in (((2, 0), "dxy", 1 / (scales[2] * scales[0])), ((2, None), "dx", 1 / scales[2]), ((None, 0), "dy", 1 / scales[0])):
        got = np_(k.diff(*dims).pairwise(T(x), T(y)))
        val, ab = ref[key]
        assert float(np.max(D.ratios(got, val * factor, ab * factor, "float64"))) <= 16.0, key
    d = k.diff(1)
    np.testing.assert_allclose(np_(d.elwise(T(x)))[:, 0], np.diag(np_(d.pairwise(T(x)))), rtol=1e-14)
    assert float(d.elwise(T(x))[0, 0]) == pytest.approx((1.5 * 1 + 0.5 * 3) / scales[1] ** 2, rel=1e-14)


def test_means(oracle_backend):
    x = T(np.linspace(0.5, 2.0, 7)[:, None] * np.array([[1.0, 2.0]]))
    assert isinstance(K.ZeroMean().diff(0), K.ZeroMean) and isinstance(K.OneMean().diff(1), K.ZeroMean)
    m = K.FunctionMean(lambda x: (x[:, :1] ** 2) * x[:, 1:]) * 3.0 + K.OneMean()
    d0, d1 = m.diff(0), m.diff(1)
    xn = np_(x)
    np.testing.assert_allclose(np_(d0(x))[:, 0], 3 * 2 * xn[:, 0] * xn[:, 1], rtol=1e-14)
    np.testing.assert_allclose(np_(d1(x))[:, 0], 3 * xn[:, 0] ** 2, rtol=1e-14)
    assert repr(K.FunctionMean(lambda x: x).diff(1)) == "d(1) <lambda>"
    with torch.no_grad():                                       # autograd inside, whatever the caller's mode
        np.testing.assert_allclose(np_(d1(x))[:, 0], 3 * xn[:, 0] ** 2, rtol=1e-14)
    assert float(K.FunctionMean(lambda x: torch.ones(x.shape[0], 1, dtype=x.dtype)).diff(0)(x).abs().max()) == 0.0
    with pytest.raises(NotImplementedError, match="second"):
        d0.diff(0)
    with pytest.raises(ValueError, match="dimension"):
        K.FunctionMean(lambda x: x[:, :1]).diff(2)(x)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(oracle_backend):
    f = st.GP(EQ())
    with pytest.raises(NotImplementedError, match="second derivatives"):
        f.diff().diff()
    with pytest.raises(NotImplementedError, match="second derivatives"):
        EQ().diff(0, None).diff(1, None)
    for k in (Matern12(), EQ() + 0.1 * Delta(), 2.0 * Matern12().stretch(3.0)):
        with pytest.raises(NotImplementedError, match="not differentiable"):
            k.diff(0)
    with pytest.raises(NotImplementedError, match="periodic"):
        EQ().periodic(2.0).diff(0)
    with pytest.raises(NotImplementedError, match="different input maps"):
        (EQ().stretch([1.0, 2.0]) + EQ()).diff(0)
    x = T(np.linspace(0, 1, 5))
    post = f | (f(x, 0.1), T(np.zeros(5)))
    with pytest.raises(NotImplementedError, match="posterior"):
        post.kernel.diff(0)
    with pytest.raises(NotImplementedError, match="posterior"):
        post.diff()
    with pytest.raises(NotImplementedError):
        K.SubspaceKernel(EQ(), EQ(), x, None).diff(0)
    with pytest.raises(ValueError, match="dimension"):
        EQ().diff(-1)
    with pytest.raises(ValueError, match="dimension"):
        EQ().diff(3).pairwise(T(np.zeros((4, 2))))
    with pytest.raises(TypeError):
        EQ().diff()


def test_learnable_hyperparameters_behind_a_derivative_are_refused_not_detached(oracle_backend):
    v = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    x, y = T(np.linspace(0, 1, 9)), T(np.sin(np.linspace(0, 1, 9)))
    with st.Measure() as prior:
        f = st.GP(v * EQ())
        df = f.diff()
    with pytest.raises(NotImplementedError, match="cut off from the autograd graph"):
        df(x, 0.1).logpdf(y)
    with pytest.raises(NotImplementedError, match="cut off from the autograd graph"):
        prior.logpdf((f(x, 0.1), y), (df(x, 0.1), y))
    with torch.no_grad():
        lp = df(x, 0.1).logpdf(y)
        lpj = prior.logpdf((f(x, 0.1), y), (df(x, 0.1), y))
    assert np.isfinite(float(lp)) and np.isfinite(float(lpj)) and not lp.requires_grad
    ref = D.diff_matrices([("eq", 1.3, 1.0)], None, np_(x)[:, None], np_(x)[:, None], 0, 0)["dxy"][0]
    Kd = np.asarray(ref, dtype=np.float64) + (0.1 + st.B.epsilon) * np.eye(9)
    L = np.linalg.cholesky(Kd)
    w = np.linalg.solve(L, np_(y))
    assert float(lp) == pytest.approx(-0.5 * (2 * np.log(np.diag(L)).sum() + 9 * np.log(2 * np.pi) + w @ w), rel=1e-9)


def test_a_learnable_mean_behind_a_derivative_stays_in_the_graph(oracle_backend):
    """``DiffMean`` differentiates with ``create_graph`` while a graph is recorded: the slope of ``a x^2`` is ``2 a x`` WITH its dependence
    on ``a``, so ``logpdf`` sees a residual that requires a gradient and refuses -- it never returns a detached value."""
    a = torch.tensor(1.5, dtype=torch.float64, requires_grad=True)
    x = T(np.linspace(0.1, 1.0, 7))
    dm = K.FunctionMean(lambda x: a * x**2).diff(0)
    out = dm(x)
    assert out.requires_grad
    (g,) = torch.autograd.grad(out.sum(), a)
    assert float(g) == pytest.approx(float(2 * x.sum()), rel=1e-14)
    with torch.no_grad():
        assert not dm(x).requires_grad
    df = st.GP(lambda x: a * x**2, EQ()).diff()
    with pytest.raises(NotImplementedError, match="cut off from the autograd graph"):
        df(x, 0.1).logpdf(T(np.zeros(7)))
    with torch.no_grad():
        assert np.isfinite(float(df(x, 0.1).logpdf(T(np.zeros(7)))))


def test_diff_after_conditioning_names_the_reason(oracle_backend):
    """A posterior conditioned before ``f.diff()`` cannot take the derivative: ``f.diff()`` itself works (the prior has it), the lookup
    under that posterior refuses with the reason, a posterior conditioned afterwards has it; no other refusal is swallowed."""
    x, y = T(np.linspace(0, 1, 6)), T(np.sin(np.linspace(0, 1, 6)))
    f = st.GP(EQ())
    early = f.measure | (f(x, 0.1), y)
    df = f.diff()
    assert isinstance(df.kernel, K.DiffKernel)
    with pytest.raises(K.PosteriorDerivativeError, match="conditioned before"):
        early(df)
    late = f.measure | (f(x, 0.1), y)
    assert late(df)(x).mean.shape == (6, 1)
    g = st.GP(Matern12())
    keep = g.measure | (g(x, 0.1), y)            # a live posterior must not turn the kernel's own refusal into a silent skip
    with pytest.raises(NotImplementedError, match="not differentiable"):
        g.diff()
    assert keep is not None


# ---------------------------------------------------------------------------------------------
# C ABI: version, binding, argument codes (no device: every argument is checked before an empty problem returns)
# ---------------------------------------------------------------------------------------------
def _call(lib, kinds, shapes, dim_x, dim_y, *, d=3, n=0, lower=0, symmetric=0, nterms=None, dtype=_native.GPK_F64):
    nt = len(kinds) if nterms is None else nterms
    ck = (ctypes.c_int * max(len(kinds), 1))(*kinds)
    one = (ctypes.c_double * max(len(kinds), 1))(*([1.0] * max(len(kinds), 1)))
    sh = None if shapes is None else (ctypes.c_double * len(shapes))(*shapes)
    return lib.gpk_kmat_diff(dtype, ck, one, one, sh, nt, dim_x, dim_y, None, n, d, 0, None, n, d, 0, d, None, max(n, 1), 0, 1, lower, symmetric,
                             0.0, None, 0, 0, None)


def test_abi_version_binding_and_argument_codes():
    lib = _native.load()
    assert lib.gpk_version() >= 105
    assert "gpk_kmat_diff" in _native.SIGNATURES and len(_native.SIGNATURES["gpk_kmat_diff"][1]) == len(_native.SIGNATURES["gpk_kmat"][1]) + 2
    N = _native
    ok = [N.K_EQ, N.K_MATERN32, N.K_MATERN52, N.K_LINEAR, N.K_CONST]
    assert _call(lib, ok, None, 0, 0) == 0 and _call(lib, ok, None, 2, -1) == 0 and _call(lib, ok, None, -1, 1) == 0
    assert _call(lib, ok, None, 1, 1, lower=1, symmetric=1) == 0
    assert _call(lib, [N.K_RQ], [0.7], 0, 0) == 0 and _call(lib, [], None, 0, 0) == 0
    assert _call(lib, ok, None, 0, 0, dtype=7) == -1
    for bad in (N.K_MATERN12, N.K_DELTA, 8, -1):
        assert _call(lib, [N.K_EQ, bad], [0.0, 1e-6], 0, 0) == -2
    assert _call(lib, [N.K_RQ], None, 0, 0) == -1 and _call(lib, [N.K_RQ], [0.0], 0, 0) == -5       # (the `shapes` rules of gpk_kmat) and _call(lib, [N.K_EQ, N.K_RQ], [0.0, -1.0], 0, 0) == -5
    assert _call(lib, ok, None, 0, 0, nterms=9) == -6 and _call(lib, ok, None, 0, 0, nterms=-1) == -6
    assert _call(lib, ok, None, 3, 0) == -7 and _call(lib, ok, None, -2, 0) == -7 and _call(lib, ok, None, -1, -1) == -7
    assert _call(lib, ok, None, 0, 3) == -8 and _call(lib, ok, None, 0, -2) == -8
    assert _call(lib, ok, None, 0, 0, d=-1) == -17
    for dims in ((0, 1), (0, -1), (-1, 0)):
        assert _call(lib, ok, None, *dims, symmetric=1) == -23 and _call(lib, ok, None, *dims, lower=1) == -23
    assert _call(lib, ok, None, 0, 0, n=2**31) == -10
