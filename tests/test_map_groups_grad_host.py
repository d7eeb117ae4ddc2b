"""Learning sums of kernels behind DIFFERENT input maps: the host logic of the per-group differentiable paths (log-density of one
process, joint log-density of several, posterior marginals, the predictive density by the chain rule) on a test-only NumPy backend --
``OracleBackend`` extended here by the rational-quadratic kind, the sums for shape parameters, the transposed solve and a record of
the backend calls.  References, models and tolerances: ``tests/map_groups_cases.py``."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import kernels as K, ops
from stheno_amd.torch import EQ, RQ, Linear

from . import map_groups_cases as C
from .conftest import OracleBackend, _np


def _profile(kind, q, shape):
    """``(kappa, d kappa / dq, d kappa / d shape)`` of a term kind at ``q`` (the squared scaled distance; the scaled dot product for
    ``linear``)."""
    if kind == "eq":
        k = np.exp(-0.5 * q)
        return k, -0.5 * k, None
    if kind == "rq":
        b = 1.0 + q / (2.0 * shape)
        k = np.exp(-shape * np.log(b))
        return k, -0.5 * k / b, k * (-np.log(b) + (q / (2.0 * shape)) / b)
    if kind == "linear":
        return q, np.ones_like(q), None
    if kind == "const":
        return np.ones_like(q), np.zeros_like(q), None
    raise NotImplementedError(kind)


def _q(kind, a, b, scale):
    return (a @ b.T if kind == "linear" else C.d2(a, b)) / scale**2


class GroupsOracle(OracleBackend):
    """``OracleBackend`` with the ``"rq"`` kind (values, the third column of the sums, input gradients), distances by direct
    differences, ``tri_solve_t_`` -- and ``calls``, the names of the kernel-matrix launches and reductions in the order they were made."""

    def __init__(self):
        self.calls = []

    def count(self, name):
        return self.calls.count(name)

    def _shapes(self, terms):
        return terms.shapes if terms.shapes is not None else [None] * len(terms)

    def kmat(self, terms, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        self.calls.append("kmat")
        if x.dim() != 2:
            return super().kmat(terms, x, y, lower=lower, diag_add=diag_add, diag_vec=diag_vec, out=out, accumulate=accumulate)
        a = _np(x)
        b = a if y is None else _np(y)
        k = np.zeros((a.shape[0], b.shape[0]))
        for (kind, v, s), shp in zip(terms.terms, self._shapes(terms)):
            k += v * _profile(kind, _q(kind, a, b, s), shp)[0]
        if y is None:
            k[np.diag_indices(a.shape[0])] += diag_add
            if diag_vec is not None:
                k[np.diag_indices(a.shape[0])] += _np(diag_vec)
        res = self._t(k, x)
        if out is not None:
            out.copy_(out + res if accumulate else res)
            return out
        return res

    def kdiag(self, terms, x):
        a = _np(x)
        d = np.zeros(a.shape[:-1])
        for kind, v, s in terms.terms:
            d += v * ((a * a).sum(-1) / s**2 if kind == "linear" else 1.0)
        return self._t(d, x)

    def tri_solve_t_(self, l, dinv_sb, sb, b):
        L = np.tril(_np(l))
        b.copy_(self._t(np.linalg.solve(L.T, _np(b)), b))
        return b

    def _dense(self, terms, x, y, Ge, want_colsum, want_gradx):
        xs, ys = _np(x), _np(y)
        ns = 3 if terms.shapes is not None else 2
        S, kfull, gx = np.zeros((len(terms), ns)), np.zeros_like(Ge), np.zeros_like(xs)
        for t, ((kind, var, scale), shp) in enumerate(zip(terms.terms, self._shapes(terms))):
            q = _q(kind, xs, ys, scale)
            k, dk, da = _profile(kind, q, shp)
            S[t, 0], S[t, 1] = np.sum(Ge * k), np.sum(Ge * dk * q)
            if da is not None:
                S[t, 2] = np.sum(Ge * da)
            kfull += var * k
            if kind == "linear":
                gx += (Ge * var / scale**2) @ ys
            elif kind != "const":
                coef = Ge * var * dk * 2 / scale**2
                gx += coef.sum(1)[:, None] * xs - coef @ ys
        return (self._t(S, x), self._t((Ge * kfull).sum(0), x) if want_colsum else None, self._t(gx, x) if want_gradx else None)

    def kmat_vjp_dense(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        self.calls.append("kmat_vjp_dense")
        Ge = _np(g).copy()
        if colscale is not None:
            Ge = Ge * _np(colscale)[None, :]
        if w is not None:
            Ge = Ge + _np(w)[:, None] * _np(b)[None, :]
        return self._dense(terms, x, y, Ge, want_colsum, want_gradx)

    def kmat_vjp(self, terms, x, kinv, alpha, g):
        self.calls.append("kmat_vjp")
        ki = np.tril(_np(kinv)) + np.tril(_np(kinv), -1).T
        A, gv = _np(alpha), np.asarray(g, dtype=np.float64)
        G = 0.5 * ((A * gv) @ A.T - gv.sum() * ki)
        S, _, _ = self._dense(terms, x, x, G, False, False)
        return S, self._t(np.trace(G), x), self._t(np.diag(G).copy(), x)


@pytest.fixture()
def be():
    backend = GroupsOracle()
    prev = ops.set_backend(backend)
    old = st.B.epsilon
    st.B.epsilon = C.EPS
    yield backend
    st.B.epsilon = old
    ops.set_backend(prev)


def T(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


# ---------------------------------------------------------------------------------------------
# 1, 2: the log-density of one process
# ---------------------------------------------------------------------------------------------
def test_logpdf_of_three_groups_all_gradients(be):
    x, _, y, _ = C.data()
    ref = C.logpdf_reference()
    k, t = C.three_group_kernel()
    assert len(K._map_groups(k)) == 3 and k.input_scaled_view() is None
    tx, ty, noise = T(x, True), T(y, True), T(C.NOISE, True)
    lp = st.GP(k)(tx, noise).logpdf(ty)
    assert lp.requires_grad
    C.assert_value("logpdf", float(lp), ref["value"])
    lp.backward()
    C.assert_close("hyper-parameters", C.hyper_grads(t), ref["hyper"])
    C.assert_close("noise", float(noise.grad), ref["noise"])
    C.assert_close("y", ty.grad.numpy(), ref["y"])
    C.assert_close("x", tx.grad.numpy(), ref["x"])
    # the explicit cotangent once, every group's sums and input gradient out of ONE dense pass; the plain group's inputs move with x
    assert (be.count("kmat"), be.count("kmat_vjp"), be.count("kmat_vjp_dense")) == (3, 0, 3)


def test_logpdf_of_three_groups_without_learnable_maps(be):
    x, _, y, _ = C.data()
    ref = C.logpdf_reference()
    k, t = C.three_group_kernel(learn=C.PLAIN)
    ty, noise = T(y, True), T(C.NOISE, True)
    lp = st.GP(k)(T(x), noise).logpdf(ty)
    C.assert_value("logpdf", float(lp), ref["value"])
    lp.backward()
    pick = [C.NAMES.index(n) for n in C.PLAIN]
    C.assert_close("variances and scalar scales", C.hyper_grads(t, C.PLAIN), ref["hyper"][pick])
    C.assert_close("noise", float(noise.grad), ref["noise"])
    C.assert_close("y", ty.grad.numpy(), ref["y"])
    assert t["period"].grad is None and t["l"].grad is None and t["alpha"].grad is None
    # no mapped input carries a gradient: the implicit form, one pass over K^{-1} per group, no explicit cotangent
    assert (be.count("kmat"), be.count("kmat_vjp"), be.count("kmat_vjp_dense")) == (3, 3, 0)


# ---------------------------------------------------------------------------------------------
# 3: one group takes the launches it took
# ---------------------------------------------------------------------------------------------
def test_one_group_issues_the_same_backend_calls(be):
    x, _, y, _ = C.data()
    v, s = T(1.2, True), T(0.9, True)
    lp = st.GP(v * EQ().stretch(s))(T(x), C.NOISE).logpdf(T(y))
    lp.backward()
    assert be.calls == ["kmat", "kmat_vjp"]
    assert v.grad is not None and s.grad is not None
    # ... behind a map with a learnable parameter, or with inputs that move: the implicit pass, then the input gradient from the
    # explicit cotangent
    for make in (lambda: (st.GP(1.2 * EQ().periodic(T(3.1, True))), T(x)),
                 lambda: (st.GP(1.2 * EQ().stretch(T([0.8, 1.7], True))), T(x)),
                 lambda: (st.GP(1.2 * EQ().stretch(0.9)), T(x, True))):
        del be.calls[:]
        f, tx = make()
        f(tx, C.NOISE).logpdf(T(y)).backward()
        assert be.calls == ["kmat", "kmat_vjp", "kmat_vjp_dense"]


# ---------------------------------------------------------------------------------------------
# 4: several processes observed jointly
# ---------------------------------------------------------------------------------------------
def test_joint_logpdf_of_a_sum_process_and_its_periodic_part(be):
    x, _, y, _ = C.data()
    ref = C.joint_reference()
    prior, f, f2, t = C.joint_model()
    lp = prior.logpdf((f(T(x[:C.NA]), C.NOISE), T(y[:C.NA])), (f2(T(x[C.NA:]), C.NOISE_B), T(y[C.NA:])))
    assert lp.requires_grad
    C.assert_value("joint logpdf", float(lp), ref["value"])
    lp.backward()
    C.assert_close("hyper-parameters", np.array([float(t[n].grad) for n in C.JOINT_NAMES]), ref["hyper"])
    # blocks (f, f): two groups, (f2, f): one, (f2, f2): one -- plus the mirror pass of the off-diagonal block for its column inputs
    assert be.count("kmat_vjp_dense") == 5 and be.count("kmat_vjp") == 0


# ---------------------------------------------------------------------------------------------
# 5: posterior marginals
# ---------------------------------------------------------------------------------------------
def test_posterior_marginals_of_three_groups(be):
    x, xs, y, _ = C.data()
    ref = C.marginals_reference()
    k, t = C.three_group_kernel()
    f = st.GP(k)
    tx, txs = T(x, True), T(xs, True)
    post = f | (f(tx, C.NOISE), T(y))
    fdd = post(txs)
    loss = fdd.mean.sum() + fdd.var_diag.sum()
    assert loss.requires_grad
    C.assert_value("loss", float(loss), ref["value"])
    loss.backward()
    C.assert_close("hyper-parameters", C.hyper_grads(t), ref["hyper"])
    C.assert_close("x", tx.grad.numpy(), ref["x"])
    C.assert_close("xs", txs.grad.numpy(), ref["xs"])


# ---------------------------------------------------------------------------------------------
# 6: the predictive density, by the chain rule of two prior densities
# ---------------------------------------------------------------------------------------------
def test_predictive_logpdf_under_learnable_maps(be):
    x, xs, y, ys = C.data()
    ref = C.predictive_reference()
    k, t = C.three_group_kernel()
    f = st.GP(k)
    lp = (f | (f(T(x), C.NOISE), T(y)))(T(xs), C.NOISE).logpdf(T(ys))
    assert lp.requires_grad
    C.assert_value("predictive logpdf", float(lp), ref["value"])
    lp.backward()
    C.assert_close("hyper-parameters", C.hyper_grads(t), ref["hyper"])


# ---------------------------------------------------------------------------------------------
# 7: what stays refused
# ---------------------------------------------------------------------------------------------
def test_refusals_that_stay(be):
    rng = np.random.default_rng(7)
    p = T(3.1, True)
    k = 1.2 * EQ().stretch(0.9) + 0.7 * EQ().periodic(p)
    # a batch of data sets under a multi-map kernel
    xb, yb = T(rng.uniform(-2, 2, (2, 12, 2))), T(rng.standard_normal((2, 12, 1)))
    with pytest.raises(NotImplementedError, match="outside the differentiable paths"):
        st.GP(k)(xb, 0.1).logpdf(yb)
    # the pseudo-point bound of a multi-map kernel
    x, z, y = T(rng.uniform(-2, 2, (12, 2))), T(rng.uniform(-2, 2, (5, 2))), T(rng.standard_normal((12, 1)))
    f = st.GP(k)
    elbo = st.PseudoObs(f(z), f(x, 0.1), y).elbo(f.measure)
    assert not elbo.requires_grad                     # (not built: a value without a graph, as before)
    # a periodic group with five input dimensions under a learnable period: ten dimensions behind the map
    x5, y5 = T(rng.standard_normal((12, 5))), T(rng.standard_normal((12, 1)))
    del be.calls[:]
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        st.GP(0.7 * EQ().periodic(p))(x5, 0.1).logpdf(y5)
    assert be.calls == []                             # (refused before anything is launched)


def test_the_limits_hold_per_group(be):
    """Eight input dimensions behind a map that passes a gradient on, eight terms: per group, refused before anything is launched."""
    rng = np.random.default_rng(8)
    p = T(3.1, True)
    x5, y5 = T(rng.standard_normal((12, 5))), T(rng.standard_normal((12, 1)))
    k = 1.2 * EQ().stretch(0.9) + 0.7 * EQ().periodic(p)
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        st.GP(k)(x5, 0.1).logpdf(y5)
    f = st.GP(k)
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        (f | (f(x5, 0.1), y5))(x5).mean
    assert be.calls == []
    # (a learnable variance alone needs no input gradient: any dimension, in every group)
    v = T(1.0, True)
    lp = st.GP(v * EQ().stretch(0.9) + 0.7 * EQ().periodic(3.1))(x5, 0.1).logpdf(y5)
    lp.backward()
    assert v.grad is not None
    # nine terms in one of two groups
    del be.calls[:]
    many = sum((RQ(0.1 * (i + 1)) for i in range(1, 9)), RQ(0.1)) + 0.7 * EQ().periodic(p)
    with pytest.raises(ValueError, match="at most 8"):
        st.GP(many)(x5[:, :2], 0.1).logpdf(y5)
    assert be.calls == []
