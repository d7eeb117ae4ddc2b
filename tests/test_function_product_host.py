"""Processes times functions, ``f * fn``: the host logic (kernel and mean algebra, the group walk with its scaled launches, the measure's
product rule, the differentiable log-density and the refusals) on the stock test-only oracle backend, with the backend calls recorded.
Models, references and bars: ``tests/function_product_cases.py``."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import kernels as K, ops
from stheno_amd.torch import EQ, RQ, Matern32

from oracle import gp_oracle as O

from . import function_product_cases as F
from . import map_groups_cases as C
from .conftest import OracleBackend, _np


class Recorder(ops._HostDelta):
    """The stock oracle backend behind the package's own host wrapper, with ``calls``: ``(name, out argument, accumulate, result)`` of
    every kernel-matrix call."""

    def __init__(self):
        super().__init__(OracleBackend())
        self.calls = []

    def kmat(self, terms, x, y=None, **kw):
        res = super().kmat(terms, x, y, **kw)
        self.calls.append(("kmat", kw.get("out"), bool(kw.get("accumulate")), res))
        return res

    def kmat_scaled(self, terms, x, y, row_scale, col_scale, **kw):
        res = super().kmat_scaled(terms, x, y, row_scale, col_scale, **kw)
        self.calls.append(("kmat_scaled", kw.get("out"), bool(kw.get("accumulate")), res))
        return res

    def kmat_vjp(self, *a, **kw):
        self.calls.append(("kmat_vjp", None, False, None))
        return self._inner.kmat_vjp(*a, **kw)

    def kmat_vjp_dense(self, *a, **kw):
        self.calls.append(("kmat_vjp_dense", None, False, None))
        return super().kmat_vjp_dense(*a, **kw)

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture()
def be():
    rec = Recorder()
    prev = ops.set_backend(rec)
    yield rec
    ops.set_backend(prev)


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


# ---- Bayesian linear regression against weight space ------------------------------------------------------------
def test_blr_posteriors_and_evidence_match_weight_space(be):
    x, y, xs = F.blr_data()
    w, cov, pm, pv, lml = F.blr_reference(x, y, xs)
    prior, slope, intercept, f = F.blr_model()
    C.assert_value("log marginal likelihood", float(f(T(x), F.NOISE).logpdf(T(y)[:, None])), lml)
    post = prior | (f(T(x), F.NOISE), T(y)[:, None])
    for name, p, i in (("slope", slope, 0), ("intercept", intercept, 1)):
        fdd = post(p)(T([0.0]))
        C.assert_value(f"{name} mean", float(fdd.mean), w[i])
        C.assert_value(f"{name} variance", float(_np(fdd.var.mat)[0, 0]), cov[i, i])
    mean, var = post(f)(T(xs)).marginals()
    C.assert_close("predictive mean", _np(mean).ravel(), pm)
    C.assert_close("predictive variances", _np(var).ravel(), pv)
    lo, hi = post(f)(T(xs)).marginal_credible_bounds()[1:]
    assert bool((lo < hi).all())


def test_blr_sample_and_joint_conditioning(be):
    x, y, xs = F.blr_data()
    w, cov, *_ = F.blr_reference(x, y, xs)
    prior, slope, intercept, f = F.blr_model()
    s = f(T(x), F.NOISE).sample(3, generator=torch.Generator().manual_seed(0))
    assert tuple(s.shape) == (len(x), 3) and bool(torch.isfinite(s).all())
    # the data and one exact observation of the intercept, jointly: the slope's posterior is the one-weight regression on y - c
    c = -2.0
    post = prior | ((f(T(x), F.NOISE), T(y)[:, None]), (intercept(T([0.0])), T([[c]])))
    a = x @ x / F.NOISE + 1.0
    C.assert_value("slope | intercept", float(post(slope)(T([0.0])).mean), (x @ (y - c)) / F.NOISE / a)
    C.assert_value("slope variance | intercept", float(_np(post(slope)(T([0.0])).var.mat)[0, 0]), 1.0 / a)


# ---- values of the algebra against the oracle ------------------------------------------------------------
def _data(n=23, d=2, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)), rng.standard_normal((7, d))


def _fn(x):
    return torch.sin(x[..., 0]) + 0.5 * x[..., 1]


FN = st.ScaleFn(_fn)        # (a bare function is refused by GP.__mul__, as before: the wrapped function multiplies a process)


def _fn_np(x):
    return np.sin(x[..., 0]) + 0.5 * x[..., 1]


TERMS = [("eq", 1.3, 0.8), ("matern32", 0.4, 1.1)]


def _kernel():
    return 1.3 * EQ().stretch(0.8) + 0.4 * Matern32().stretch(1.1)


def test_variance_cross_blocks_and_diagonal(be):
    x, xs = _data()
    Kxx, s = O.kernel_matrix(TERMS, x, x), _fn_np(x)
    with st.Measure():
        f = st.GP(_kernel())
        g = f * FN
        both = st.cross(f, g)
    C.assert_close("var", _np(g(T(x)).var.mat), np.outer(s, s) * Kxx)
    C.assert_close("var_diag", _np(g(T(x)).var_diag), s * s * np.diag(Kxx))
    mi = K.MultiInput([(f, T(x)), (g, T(x))])
    blocks = _np(both.kernel.pairwise(mi))
    n = len(x)
    C.assert_close("cov(f, f fn)", blocks[:n, n:], Kxx * s[None, :])
    C.assert_close("cov(f fn, f)", blocks[n:, :n], Kxx * s[:, None])
    C.assert_close("cov(f fn, f fn)", blocks[n:, n:], np.outer(s, s) * Kxx)
    C.assert_close("k(x, xs)", _np(g.kernel.pairwise(T(x), T(xs))), s[:, None] * O.kernel_matrix(TERMS, x, xs) * _fn_np(xs)[None, :])


def test_batch_module_orders_and_products(be):
    rng = np.random.default_rng(9)
    xb = rng.standard_normal((3, 11, 2))
    sb = _fn_np(xb)
    f = st.GP(_kernel())
    ref = np.stack([np.outer(sb[i], sb[i]) * O.kernel_matrix(TERMS, xb[i], xb[i]) for i in range(3)])
    C.assert_close("batch (3, N, 2)", _np((f * FN)(T(xb)).var.mat), ref)

    class Mod(torch.nn.Module):
        def forward(self, x):
            return _fn(x)[..., None]           # (..., N, 1) is accepted too

    x, _ = _data()
    s, Kxx = _fn_np(x), O.kernel_matrix(TERMS, x, x)
    C.assert_close("nn.Module", _np((f * Mod())(T(x)).var.mat), np.outer(s, s) * Kxx)
    C.assert_close("fn * f", _np((FN * f)(T(x)).var.mat), np.outer(s, s) * Kxx)
    fn2 = st.ScaleFn(lambda x: torch.cos(x[..., 1]))
    s2 = s * np.cos(x[:, 1])
    prod = (f * FN) * fn2
    assert isinstance(prod.kernel, K.FnScaled) and not isinstance(prod.kernel.k, K.FnScaled)
    C.assert_close("(f fn1) fn2", _np(prod(T(x)).var.mat), np.outer(s2, s2) * Kxx)
    scaled = 3.0 * (f * FN)
    assert isinstance(scaled.kernel, K.FnScaled)             # c * (k * fn) stays a scaled group
    C.assert_close("c (f fn)", _np(scaled(T(x)).var.mat), 9.0 * np.outer(s, s) * Kxx)
    m = st.GP(lambda x: x[..., :1] ** 2, EQ()) * FN
    C.assert_close("mean", _np(m(T(x)).mean).ravel(), x[:, 0] ** 2 * s)
    assert isinstance((st.GP(EQ()) * FN).mean, K.ZeroMean)
    with pytest.raises(ValueError, match=r"\(23, 2\)"):
        (f * st.ScaleFn(lambda x: x))(T(x)).var.mat                    # (N, 2) for (N, 2) inputs: neither (N,) nor (N, 1)


def test_reversed_exchanges_the_functions(be):
    x, xs = _data()
    fa, fb = K.ScaleFn(_fn), K.ScaleFn(lambda x: torch.cos(x[..., 1]))
    k = K._fn_scaled(_kernel(), fa, fb)
    assert not k.symmetric and reversed(k).fx is fb and reversed(k).fy is fa
    C.assert_close("reversed", _np(reversed(k).pairwise(T(xs), T(x))), _np(k.pairwise(T(x), T(xs))).T)
    sym = _kernel() * _fn
    assert sym.symmetric and reversed(sym) is sym


def test_sum_is_one_kmat_and_one_accumulating_scaled_launch(be):
    x, _ = _data()
    s = _fn_np(x)
    with st.Measure():
        f = st.GP(_kernel()) * FN + st.GP(0.7 * EQ())
    be.calls.clear()
    got = f(T(x), 0.1).var.mat
    assert be.names() == ["kmat_scaled", "kmat"] or be.names() == ["kmat", "kmat_scaled"]
    first, second = be.calls
    assert first[1] is None and not first[2]
    assert second[2] and second[1] is first[3], "the second launch accumulates onto the buffer the first returned"
    ref = np.outer(s, s) * O.kernel_matrix(TERMS, x, x) + 0.7 * O.kernel_matrix([("eq", 1.0, 1.0)], x, x) + 0.1 * np.eye(len(x))
    C.assert_close("fn k_a fn + k_b + noise", np.tril(_np(got)), np.tril(ref))
    # k_b first: the plain group writes (with the unscaled noise), the scaled group adds
    with st.Measure():
        g = st.GP(0.7 * EQ()) + st.GP(_kernel()) * FN
    be.calls.clear()
    C.assert_close("k_b + fn k_a fn + noise", np.tril(_np(g(T(x), 0.1).var.mat)), np.tril(ref))
    assert be.names() == ["kmat", "kmat_scaled"] and be.calls[1][2] and be.calls[1][1] is be.calls[0][3]


def test_out_views_keep_their_meaning(be):
    x, xs = _data()
    k = (_kernel() * _fn) + 0.7 * EQ()
    big = torch.full((40, 40), -7.0, dtype=torch.float64)
    k.pairwise(T(x), T(xs), out=big[3:26, 5:12])
    ref = _fn_np(x)[:, None] * O.kernel_matrix(TERMS, x, xs) * _fn_np(xs)[None, :] + 0.7 * O.kernel_matrix([("eq", 1.0, 1.0)], x, xs)
    C.assert_close("view", _np(big[3:26, 5:12]), ref)
    big[3:26, 5:12] = -7.0
    assert bool((big == -7.0).all())


# ---- refusals ------------------------------------------------------------
def test_refusals_of_the_algebra(be):
    k = _kernel() * _fn
    for op in (lambda: k.diff(0), lambda: k.shift(1.0), lambda: k.stretch(2.0), lambda: k.stretch([1.0, 2.0]), lambda: k.select(0),
               lambda: k.transform(lambda x: x), lambda: k.periodic(1.0), lambda: (k + EQ()).shift(1.0), lambda: (2.0 * k).diff(0)):
        with pytest.raises(NotImplementedError, match="function-scaled"):
            op()
    f = st.GP(lambda x: x[..., :1], EQ())
    g = f * FN
    for op in (lambda: g.diff(0), lambda: g.shift(1.0), lambda: g.mean.diff(0), lambda: g.mean.shift(1.0)):
        with pytest.raises(NotImplementedError, match="function-scaled"):
            op()
    assert isinstance(f.shift(1.0) * FN, st.GP)                 # mapping first and scaling then works
    with pytest.raises(NotImplementedError, match="products of processes"):
        f * f
    with pytest.raises(NotImplementedError, match="wrap the function"):      # a bare function: refused as before, with the way out
        f * _fn
    for op in (lambda: RQ(1.0) * EQ(), lambda: EQ().periodic(1.0) * EQ()):
        with pytest.raises(NotImplementedError, match="products of kernels"):
            op()
    v = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64).reshape(3, 1, 1)
    xb = T(np.random.default_rng(0).standard_normal((3, 5, 2)))
    be.calls.clear()
    with pytest.raises(NotImplementedError, match="per-batch hyper-parameters"):
        (st.GP(v * EQ()) * FN)(xb).var.mat
    assert be.calls == []


def _learnable_model():
    w = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    fn = st.ScaleFn(lambda x: w * x[..., 0])
    with st.Measure() as prior:
        a, b = st.GP(EQ()), st.GP(0.5 * EQ())
        f = a * fn + b
    return prior, a, b, f


def _learnable_cases():
    rng = np.random.default_rng(1)
    x, xs, y = T(rng.standard_normal((9, 1))), T(rng.standard_normal((4, 1))), T(rng.standard_normal((9, 1)))
    xb, yb = T(rng.standard_normal((2, 9, 1))), T(rng.standard_normal((2, 9, 1)))

    def inputs(prior, a, b, f):
        return f(x.clone().requires_grad_(True), 0.1).logpdf(y)

    def batch(prior, a, b, f):
        return f(xb, 0.1).logpdf(yb)

    def joint(prior, a, b, f):
        return prior.logpdf((f(x, 0.1), y), (b(xs, 0.1), y[:4]))

    def bound(prior, a, b, f):
        return st.PseudoObs(f(xs), f(x, 0.1), y).elbo(prior)

    def post_mean(prior, a, b, f):
        return (prior | (f(x, 0.1), y))(f)(xs).mean

    def post_var(prior, a, b, f):
        return (prior | (f(x, 0.1), y))(a)(xs).var_diag

    def predictive(prior, a, b, f):
        return (prior | (f(x, 0.1), y))(f)(xs, 0.1).logpdf(y[:4])

    return [inputs, batch, joint, bound, post_mean, post_var, predictive]


@pytest.mark.parametrize("case", _learnable_cases(), ids=lambda c: c.__name__)
def test_learnable_cases_outside_the_logpdf_are_refused_before_any_launch(be, case):
    model = _learnable_model()
    be.calls.clear()
    with pytest.raises(NotImplementedError, match="(?s)function-scaled.*cut off from the autograd graph"):
        case(*model)
    assert be.calls == []
    with torch.no_grad():
        val = case(*_learnable_model())
    assert bool(torch.isfinite(torch.as_tensor(val)).all())


# ---- learning ------------------------------------------------------------
def test_modulated_network_gradients_match_finite_differences(be):
    x, y = F.modulated_data(60)
    p = F.net_params()
    ref, fd = F.fd_reference(p, F.NET_NAMES, x, y)
    net = F.TanhNet(p, "cpu")
    f, a, b, prior, t = F.modulated_model(p, net, "cpu")
    be.calls.clear()
    lp = f(T(x), t["noise"]).logpdf(T(y)[:, None])
    assert be.names() == ["kmat_scaled", "kmat"]
    C.assert_value("logpdf", float(lp.detach()), ref)
    lp.backward()
    # the scaled group: one pass for the per-term sums, one for the column sums behind the function; the plain group: one pass
    assert be.names()[2:] == ["kmat_vjp_dense", "kmat_vjp_dense", "kmat_vjp_dense"]
    C.assert_close("d logpdf / d (l_a, l_b, v_a, v_b, noise, net)", F.net_grads(t, net), fd)


def test_gradient_of_a_parameter_inside_the_function_where_it_vanishes(be):
    x, y = F.modulated_data(60, with_zero=True)
    assert (x == 0.0).sum() == 1
    p = dict(F.net_params(), w=np.array(0.8))
    names = ["l_a", "l_b", "v_a", "v_b", "noise", "w"]
    ref, fd = F.fd_reference(p, names, x, y, fn=F.linear_np)
    w = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
    f, a, b, prior, t = F.modulated_model(p, lambda x: w * x[:, 0], "cpu")      # (wrapped there)
    lp = f(T(x), t["noise"]).logpdf(T(y)[:, None])
    C.assert_value("logpdf", float(lp.detach()), ref)
    lp.backward()
    got = np.array([float(t[k].grad) for k in names[:-1]] + [float(w.grad)])
    C.assert_close("d logpdf / d (l_a, l_b, v_a, v_b, noise, w)", got, fd)


def test_nothing_learnable_runs_the_plain_path(be):
    x, y, _ = F.blr_data()
    prior, slope, intercept, f = F.blr_model()
    be.calls.clear()
    lp = f(T(x), F.NOISE).logpdf(T(y)[:, None])          # grad mode on, nothing learnable: a plain value
    assert not lp.requires_grad and "kmat_vjp_dense" not in be.names()
