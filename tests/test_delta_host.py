"""Host logic of the ``Delta`` kernel (``"delta"`` term kind): the term algebra with its epsilon, descriptor validation, the values
a backend without the HIP kernels computes (the ``"delta"`` terms are added in NumPy by ``stheno_amd.ops``), noise as a process of
its own -- ``y = f + GP(s2 * Delta())`` against ``f(x, s2)`` -- and the argument codes of the C ABI, which need no GPU: the launchers
check their term tables before they touch the device.  Values on the MI355X: ``tests/test_delta_gpu.py``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import _native, autograd, kernels as K, learnable, ops
from stheno_amd.torch import EQ, RQ, Delta, Matern52

from . import delta_reference as D
from .conftest import ROOT, T


def np_(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------
# algebra
# ---------------------------------------------------------------------------------------------
def test_delta_term_algebra():
    k = Delta()
    assert repr(k) == "Delta(1e-06)" and repr(Delta(1e-3)) == "Delta(0.001)"
    assert k.terms() == [("delta", 1.0, 1.0)] and k.shapes() == [1e-6] and k.tensor_shapes() == [1e-6] and k.stationary
    assert reversed(k) is k
    # equal epsilons merge, different ones stay two terms
    s = Delta() + Delta()
    assert s.terms() == [("delta", 2.0, 1.0)] and s.shapes() == [1e-6]
    s = Delta(1e-6) + Delta(1e-3)
    assert s.terms() == [("delta", 1.0, 1.0), ("delta", 1.0, 1.0)] and s.shapes() == [1e-6, 1e-3]
    s = 2 * Delta() + Delta()
    assert s.terms() == [("delta", 3.0, 1.0)] and s.shapes() == [1e-6]
    # ... and never with another kind or another scale
    s = EQ() + 0.1 * Delta() + RQ(2.0) + Delta().stretch(2.0)
    assert [t[0] for t in s.terms()] == ["eq", "delta", "rq", "delta"] and s.shapes() == [None, 1e-6, 2.0, 1e-6]
    # stretch: scalar -> the term's scale; per dimension -> an input map in front of the same term
    s = (0.5 * Delta(1e-4)).stretch(4.0)
    assert s.terms() == [("delta", 0.5, 4.0)] and s.shapes() == [1e-4]
    v = Delta().stretch([0.5, 2.0])
    assert isinstance(v, K.InputScaled) and v.input_scaled_view()[0].terms() == [("delta", 1.0, 1.0)]
    # a learnable variance is a learnable hyper-parameter like any other; epsilon never is
    var = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    assert learnable.kernel_requires_grad(var * Delta()) and not learnable.kernel_requires_grad(0.1 * Delta())
    assert (var * Delta()).tensor_terms()[0][1].requires_grad
    assert "Delta" in st.__all__ if hasattr(st, "__all__") else hasattr(st, "Delta")
    import stheno_amd

    assert stheno_amd.Delta is Delta


def test_bad_and_learnable_epsilon_are_refused():
    for bad in (0.0, -1e-6, torch.tensor(-1.0)):
        with pytest.raises(ValueError, match="positive"):
            Delta(bad)
    with pytest.raises(ValueError, match="not learnable"):
        Delta(torch.tensor(1e-6, dtype=torch.float64, requires_grad=True))
    assert Delta(torch.tensor(1e-3)).shapes() == [pytest.approx(1e-3)]        # a plain tensor is a number
    # the autograd packing refuses one that got past the constructor
    e = torch.tensor(1e-6, dtype=torch.float64, requires_grad=True)
    with pytest.raises(ValueError, match="not learnable"):
        autograd._pack([("delta", 1.0, 1.0, e)])
    a = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
    assert len(autograd._pack([("rq", 1.0, 1.0, a)])[1]) == 3


def test_kterms_validate_epsilon():
    t = ops.KTerms([("eq", 1.0, 2.0), ("delta", 0.1, 1.0)], [None, 1e-6])
    assert t.shapes == [None, 1e-6] and list(t.c_shapes()) == [0.0, 1e-6]
    assert ops.KTerms([("eq", 1.0, 1.0)]).c_shapes() is None           # no shaped term: the library gets NULL
    assert list(t.c_arrays()[0]) == [_native.K_EQ, _native.K_DELTA] and _native.K_DELTA == 7
    assert "delta" in ops._SHAPED and "delta" not in ops._LEARNABLE_SHAPE
    for bad in ([0.0], [-1e-6], [None], None):
        with pytest.raises(ValueError, match=r"positive shape parameter \(epsilon\)"):
            ops.KTerms([("delta", 1.0, 1.0)], bad)


def test_epsilon_gradient_is_none_and_variance_gradient_is_s1():
    S = torch.tensor([[2.0, 3.0, 5.0], [7.0, 0.0, 0.0]], dtype=torch.float64)
    meta = [(torch.device("cpu"), torch.float64)] * 6
    gr = autograd._param_grads(("rq", "delta"), ([1.5, 0.5], [1.0, 2.0], [2.0, 1e-6]), S, meta)
    assert float(gr[0]) == 2.0 and float(gr[1]) == 7.0            # d/dv_t = S1_t
    assert float(gr[3]) == 0.0                                    # d/dscale of Delta: -2 v S2 / l with S2 = 0
    assert float(gr[4]) == 1.5 * 5.0 and gr[5] is None            # d/dalpha of RQ; None for Delta's epsilon


# ---------------------------------------------------------------------------------------------
# values through a backend without the HIP kernels
# ---------------------------------------------------------------------------------------------
TERMSETS = {
    "delta": D.DELTA1,
    "stretched+const": D.DELTA_STRETCHED,
    "eq+matern52+delta": ([("eq", 1.25, 2.0), ("matern52", 0.75, 1.0), ("delta", 0.5, 1.0)], [None, None, D.EPSILON]),
}


def _kernel(terms, shapes):
    prim = {"eq": EQ, "matern52": Matern52, "const": st.OneKernel}
    k = None
    for (kind, var, scale), shp in zip(terms, shapes):
        p = Delta(shp) if kind == "delta" else prim[kind]()
        p = var * (p.stretch(scale) if scale != 1.0 else p)
        k = p if k is None else k + p
    return k


@pytest.mark.parametrize("name", list(TERMSETS))
@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (33, 65, 3), (40, None, 2)])
def test_oracle_backend_matrix_equals_the_reference(oracle_backend, name, n, m, d):
    terms, shapes = TERMSETS[name]
    x, y = (None if a is None else np.array(a) for a in D.value_case(n, m, d))       # (private copies: torch wants writable memory)
    D.check_inputs(terms, shapes, x, y)
    k = _kernel(terms, shapes)
    assert k.terms() == terms and k.shapes() == shapes
    ref = np.asarray(D.kernel_matrix(terms, shapes, x, y), dtype=np.float64)
    got = np_(k.pairwise(T(x), None if y is None else T(y)))
    assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 1e-14 * np.max(np.abs(ref))
    if name == "delta":
        assert np.array_equal(got, ref)
    diag = np_(k.elwise(T(x)))[:, 0]
    assert np.allclose(diag, sum(v for _, v, _ in terms), rtol=0, atol=1e-15)
    if y is None:        # the diagonal additions, the lower triangle, a caller's view, accumulation
        dv = np.arange(n) / 8.0
        buf = torch.full((n, n + 4), -7.0, dtype=torch.float64)
        out = k.pairwise(T(x), lower=True, diag_add=0.25, diag_vec=T(dv), out=buf[:, :n])
        assert out.data_ptr() == buf.data_ptr() and bool((buf[:, n:] == -7.0).all())
        assert np.allclose(np.tril(np_(buf[:, :n])), np.tril(ref + np.diag(0.25 + dv)), rtol=0, atol=1e-14)
        acc = torch.ones((n, n), dtype=torch.float64)
        ops.get_backend().kmat(ops.KTerms(terms, shapes), T(x), None, out=acc, accumulate=True)
        assert np.allclose(np_(acc), 1.0 + ref, rtol=0, atol=1e-14)


def test_nan_inputs_stay_nan_and_per_dimension_stretch(oracle_backend):
    x, y = (np.array(a) for a in D.value_case(33, 65, 3))
    xn = x.copy()
    xn[7, 1] = np.nan
    got = np_((1.5 * Delta()).pairwise(T(xn), T(y)))
    assert np.isnan(got[7]).all() and not np.isnan(np.delete(got, 7, axis=0)).any()
    # per-dimension power-of-two scales: Delta sees x / l
    scales = np.array([0.5, 2.0, 4.0])
    ref = np.asarray(D.kernel_matrix(*D.DELTA1, x / scales, y / scales), dtype=np.float64)
    D.check_inputs(*D.DELTA1, x / scales, y / scales)
    assert np.array_equal(np_((1.5 * Delta()).stretch(scales).pairwise(T(x), T(y))), ref)
    # a coarse epsilon joins points a fine one keeps apart
    a, b = np.array([[0.0], [0.25]]), np.array([[0.0]])
    assert np_(Delta(1e-6).pairwise(T(a), T(b))).ravel().tolist() == [1.0, 0.0]
    assert np_(Delta(0.1).pairwise(T(a), T(b))).ravel().tolist() == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------
# noise as a process of its own
# ---------------------------------------------------------------------------------------------
def _data(n=48, ns=9, seed=5):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.permutation(4 * n)[:n] / 8.0)[:, None]             # distinct eighths
    xs = (rng.permutation(4 * n)[:ns] + 0.5)[:, None] / 8.0            # distinct, and none of them a training input
    y = np.sin(x) + 0.3 * rng.standard_normal((n, 1))
    return x, xs, y


def test_noise_process_identities(oracle_backend):
    x, xs, y = _data()
    s2 = 0.1
    with st.Measure() as prior:
        f = st.GP(EQ())
        e = st.GP(s2 * Delta())
        yp = f + e
    lp_process = float(yp(T(x)).logpdf(T(y)))
    lp_noise = float(f(T(x), s2).logpdf(T(y)))
    assert abs(lp_process - lp_noise) <= 1e-10 * abs(lp_noise)
    post = prior | (yp(T(x)), T(y))
    mean, var = post(f)(T(xs)).marginals()
    post_n = f | (f(T(x), s2), T(y))
    mean_n, var_n = post_n(T(xs)).marginals()
    assert np.max(np.abs(np_(mean) - np_(mean_n))) <= 1e-9 * np.max(np.abs(np_(mean_n)))
    assert np.max(np.abs(np_(var) - np_(var_n))) <= 1e-9 * np.max(np.abs(np_(var_n)))
    # the noisy prediction at new inputs carries the noise variance on top; the cross-covariance of e with f is zero
    _, var_y = post(yp)(T(xs)).marginals()
    assert np.max(np.abs(np_(var_y) - np_(var) - s2)) <= 1e-9
    assert float(prior.kernels[f, e].pairwise(T(x), T(x)).abs().max()) == 0.0
    kfy = np_(prior.kernels[yp, e].pairwise(T(x[:5]), T(x[:7])))
    assert np.array_equal(kfy, s2 * np.eye(5, 7))


def test_delta_variance_is_learnable_like_a_noise(oracle_backend):
    x, _, y = _data(n=40)
    v = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    nz = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    sc = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
    sc_n = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
    with st.Measure():
        f = st.GP(EQ().stretch(sc))
        lp = (f + st.GP(v * Delta()))(T(x)).logpdf(T(y))
    assert lp.requires_grad
    lp.backward()
    lp_n = st.GP(EQ().stretch(sc_n))(T(x), nz).logpdf(T(y))
    lp_n.backward()
    assert abs(float(v.grad) - float(nz.grad)) <= 1e-8 * abs(float(nz.grad))
    assert abs(float(sc.grad) - float(sc_n.grad)) <= 1e-8 * abs(float(sc_n.grad))


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def test_abi_codes_of_the_delta_kind():
    with open(os.path.join(ROOT, "include", "gpk.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert re.search(r"#define\s+GPK_K_DELTA\s+7\b", text)
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__ as g

        g.build()
    lib = _native.load()
    assert lib.gpk_version() >= 103
    # the term tables are checked before anything is launched: null device pointers are never read
    kind = (ctypes.c_int * 1)(_native.K_DELTA)
    one = (ctypes.c_double * 1)(1.0)
    eps, bad, neg = ((ctypes.c_double * 1)(v) for v in (1e-6, 0.0, -1e-6))
    n, m, d = 4, 5, 2
    for dt in (_native.GPK_F64, _native.GPK_F32):
        kmat_tail = (None, n, d, 0, None, m, d, 0, d, None, m, 0, 1, 0, 0, 0.0, None, 0, 0, None)
        kdiag_tail = (None, n, d, 0, d, None, n, 1, None)
        vjp_tail = (None, n, d, d, None, n, None, 1, 1, one, None, None, None)
        dense_tail = (None, n, d, None, m, d, d, None, m, None, None, None, None, None, None, None)
        # a Delta term and no shapes array at all: no epsilon was given
        assert lib.gpk_kmat(dt, kind, one, one, None, 1, *kmat_tail) == -1
        assert lib.gpk_kdiag(dt, kind, one, one, None, 1, *kdiag_tail) == -1
        assert lib.gpk_kmat_vjp(dt, kind, one, None, 1, *vjp_tail) == -1
        assert lib.gpk_kmat_vjp_dense(dt, kind, one, one, None, 1, *dense_tail) == -1
        for b in (bad, neg):
            assert lib.gpk_kmat(dt, kind, one, one, b, 1, *kmat_tail) == -5
            assert lib.gpk_kdiag(dt, kind, one, one, b, 1, *kdiag_tail) == -5
            assert lib.gpk_kmat_vjp(dt, kind, one, b, 1, *vjp_tail) == -5
            assert lib.gpk_kmat_vjp_dense(dt, kind, one, one, b, 1, *dense_tail) == -5
        # an empty problem is fine whatever the table says (nothing to do), as for every other kind
        assert lib.gpk_kmat(dt, kind, one, one, eps, 1, None, 0, d, 0, None, m, d, 0, d, None, m, 0, 1, 0, 0, 0.0, None, 0, 0, None) == 0
