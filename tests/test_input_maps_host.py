"""Input maps for kernels, means and processes -- ``shift`` / ``select`` / ``transform``, their composition, the scalar stretch in front of
them and the view with one map per argument: the host logic on a test-only NumPy backend (``OracleBackend`` with distances by direct
differences, the transposed solve and a record of the backend calls).  Models, references and tolerances: ``tests/input_maps_cases.py``.

One departure from the wording of the composition check: a symmetric shift of a STATIONARY kernel returns the kernel itself, and for
``EQ`` the two orders ``shift(0.5).stretch(2.0)`` and ``stretch(2.0).shift(0.5)`` are the same function (``k`` depends on ``x - y`` only).
Both spellings of ``EQ`` are held to NumPy; that the order matters is shown on ``Linear``, where it does."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import kernels as K, ops
from stheno_amd.matrix import KernelDense
from stheno_amd.torch import EQ, Linear, Matern52

from . import input_maps_cases as C
from .conftest import OracleBackend
from .test_posterior_grad_host import TransposedSolveOracle


class MapsOracle(TransposedSolveOracle):
    """``TransposedSolveOracle`` (Matern kernels exact on the diagonal, ``tri_solve_t_``) for unbatched inputs, ``OracleBackend`` for
    batched ones -- and ``calls``, the names of the kernel-matrix launches and reductions in the order the host logic made them."""

    def __init__(self):
        self.calls = []

    def kmat(self, terms, x, y=None, **kw):
        self.calls.append("kmat")
        if x.dim() != 2:
            return OracleBackend.kmat(self, terms, x, y, **kw)
        return super().kmat(terms, x, y, **kw)

    def kdiag(self, terms, x):
        self.calls.append("kdiag")
        return super().kdiag(terms, x)

    def kmat_vjp_dense(self, *args, **kw):
        self.calls.append("kmat_vjp_dense")
        return super().kmat_vjp_dense(*args, **kw)

    def kmat_vjp(self, terms, x, kinv, alpha, g):
        self.calls.append("kmat_vjp")
        n = len(self.calls)
        out = super().kmat_vjp(terms, x, kinv, alpha, g)
        del self.calls[n:]          # (the parent class reduces through `kmat_vjp_dense`: not a call the host logic made)
        return out


@pytest.fixture()
def be():
    backend = MapsOracle()
    prev = ops.set_backend(backend)
    old = st.B.epsilon
    st.B.epsilon = C.EPS
    yield backend
    st.B.epsilon = old
    ops.set_backend(prev)


def T(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


# ---------------------------------------------------------------------------------------------
# 1: values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_values_against_numpy(be, case):
    d = C.data()
    name, k, ref = C.value_cases()[case]
    x, xs = d["x"], d["xs"]
    C.assert_matrix(f"{name}: k(x, xs)", k.pairwise(T(x), T(xs)), ref(x, xs))
    C.assert_matrix(f"{name}: k(x)", k.pairwise(T(x)), ref(x, x))
    C.assert_matrix(f"{name}: elwise", k.elwise(T(x))[:, 0], C.diag_np(ref, x))
    low = k.pairwise(T(x), lower=True, diag_add=0.25)
    C.assert_matrix(f"{name}: lower triangle with the diagonal", torch.tril(low), np.tril(ref(x, x) + 0.25 * np.eye(C.N)))


def test_values_of_a_batch(be):
    xb = C.data()["xbatch"]
    _, k, ref = C.value_cases()[0]
    got = k.pairwise(T(xb))
    assert tuple(got.shape) == (4, 50, 50)
    for b in range(4):
        C.assert_matrix(f"batch entry {b}", got[b], ref(xb[b], xb[b]))
    C.assert_matrix("batched elwise", k.elwise(T(xb))[..., 0], np.stack([C.diag_np(ref, xb[b]) for b in range(4)]))


def test_one_dimensional_inputs_are_upranked_and_dimensions_checked(be):
    x1 = C.data()["xa"][:, 0]
    C.assert_matrix("select(0) of (N,) inputs", EQ().select(0).pairwise(T(x1)), C.eq_np(x1[:, None], x1[:, None]))
    with pytest.raises(ValueError, match="inputs have 1 dimensions, the kernel selects dimension 2"):
        EQ().select([0, 2]).pairwise(T(x1))
    with pytest.raises(ValueError, match="the shift has 3 entries"):
        Linear().shift(list(C.SHIFT_C)).pairwise(T(x1))
    with pytest.raises(ValueError):
        EQ().select(-1)


# ---------------------------------------------------------------------------------------------
# 2: composition order
# ---------------------------------------------------------------------------------------------
def test_composition_order(be):
    x = C.data()["x"]
    for k in (EQ().shift(0.5).stretch(2.0), EQ().stretch(2.0).shift(0.5)):        # (stationary: one function, see the docstring)
        C.assert_matrix("EQ, either order", k.pairwise(T(x)), C.eq_np(x / 2 - 0.5, x / 2 - 0.5))
    a, b = Linear().shift(0.5).stretch(2.0), Linear().stretch(2.0).shift(0.5)
    ra, rb = C.lin_np(x / 2 - 0.5, x / 2 - 0.5), C.lin_np((x - 0.5) / 2, (x - 0.5) / 2)
    C.assert_matrix("shift, then stretch: k(x / 2 - 0.5)", a.pairwise(T(x)), ra)
    C.assert_matrix("stretch, then shift: k((x - 0.5) / 2)", b.pairwise(T(x)), rb)
    assert np.max(np.abs(ra - rb)) > 0.1
    # a later select acts first; a stretch in front of a selection is folded into the term table (no map of its own)
    c = Linear().shift(0.5).select(0)
    C.assert_matrix("k(x[:, [0]] - c)", c.pairwise(T(x)), C.lin_np(x[:, [0]] - 0.5, x[:, [0]] - 0.5))
    folded = EQ().select(0).stretch(2.0)
    (kern, mx, my), = K._map_groups(folded)
    assert isinstance(mx, K._SelectMap) and mx is my and kern.terms() == [("eq", 1.0, 2.0)]
    (kern, mx, my), = K._map_groups(Linear().shift(0.5).stretch(2.0))
    assert [type(m) for m in mx.maps] == [K._StretchMap, K._ShiftMap] and kern.terms() == [("linear", 1.0, 1.0)]


# ---------------------------------------------------------------------------------------------
# 3: one map per argument
# ---------------------------------------------------------------------------------------------
def test_two_argument_forms(be):
    d = C.data()
    x, xs = d["x"], d["xs"]
    c = np.array(C.SHIFT_C)
    w = np.array([[0.5, -1.0], [0.2, 0.3], [-0.7, 0.1]])
    fn = lambda a: torch.tanh(a @ T(w))                                         # noqa: E731
    cases = [
        (Linear().shift(list(C.SHIFT_C), 0), T(xs), lambda a, b: C.lin_np(a - c, b), lambda a, b: C.lin_np(a, b - c)),
        (EQ().select([0], None), T(xs[:, [1]]), lambda a, b: C.eq_np(a[:, [0]], b), None),
        (Matern52().transform(fn, None), T(xs[:, :2]), lambda a, b: C.m52_np(np.tanh(a @ w), b), None),
        (Linear().stretch(2.0, 1), T(xs), lambda a, b: C.lin_np(a / 2, b), lambda a, b: C.lin_np(a, b / 2)),
    ]
    for k, y, ref, ref_rev in cases:
        yn = y.numpy()
        assert not k.symmetric and k.terms() is None
        C.assert_matrix("k(map(x), y)", k.pairwise(T(x), y), ref(x, yn))
        r = reversed(k)
        assert r is not k and reversed(r).symmetric is False
        C.assert_matrix("reversed: the maps change places", r.pairwise(y, T(x)), ref(x, yn).T)
        if ref_rev is not None:
            C.assert_matrix("reversed, closed form", r.pairwise(T(x), y), ref_rev(x, yn))
        with pytest.raises(NotImplementedError, match="same map in both arguments"):
            k.elwise(T(x))
    k = Linear().shift(list(C.SHIFT_C), 0)
    full = k.pairwise(T(x))
    ref = C.lin_np(x - c, x)
    C.assert_matrix("the symmetric spelling is the full block", full, ref)
    assert np.max(np.abs(ref - ref.T)) > 0.1
    for kw in (dict(lower=True), dict(diag_add=0.1), dict(diag_vec=T(np.ones(C.N)))):
        with pytest.raises(ValueError, match="not symmetric"):
            k.pairwise(T(x), **kw)
    # sums and scalings of such kernels reverse group by group
    s = 2.0 * k + EQ()
    C.assert_matrix("reversed sum", reversed(s).pairwise(T(x), T(xs)), 2.0 * C.lin_np(x, xs - c) + C.eq_np(x, xs))
    assert reversed(2.0 * EQ().select(0) + EQ()) is not None and reversed(EQ().select(0)).symmetric


# ---------------------------------------------------------------------------------------------
# 4: algebra and grouping
# ---------------------------------------------------------------------------------------------
def test_algebra_and_grouping(be):
    k = 1.2 * EQ().stretch(0.9)
    assert k.shift(0.5) is k and k.shift(T(0.5, True)) is k
    assert Linear().shift(0.5) is not None and not Linear().shift(0.5).stationary
    assert EQ().select(0).stationary and not EQ().transform(torch.tanh).stationary
    assert EQ().transform(torch.tanh).shift(0.5).terms() is None                # (not stationary: the shift stays)
    assert len(K._map_groups(EQ().transform(torch.tanh).shift(0.5))[0][1].maps) == 2
    a, _ = C.model_a()
    assert len(K._map_groups(a)) == 3 and a.input_scaled_view() is None and a.terms() is None
    one = EQ().select(0) + Matern52().select(0)
    assert len(K._map_groups(one)) == 1 and one.input_scaled_view() is not None
    assert len(K._map_groups(EQ().select(0) + Matern52().select(1))) == 2
    assert len(K._map_groups(EQ().shift(0.5, 0) + Matern52().shift(0.5, 0))) == 1
    assert len(K._map_groups(EQ().shift(0.5, 0) + Matern52().shift(0, 0.5))) == 2
    fn, fn2 = (lambda x: torch.tanh(x)), (lambda x: torch.tanh(x))
    assert len(K._map_groups(EQ().transform(fn) + Matern52().transform(fn))) == 1
    assert len(K._map_groups(EQ().transform(fn) + Matern52().transform(fn2))) == 2
    assert K._TransformMap(fn).stamp() is None
    tau = T(0.4, True)
    assert len(K._map_groups(Linear().shift(tau) + EQ().shift(tau, tau) + Linear().shift(T(0.4, True)))) == 2
    # distribution over sums and scalings; None / 0 / 1 leave an argument as it is
    assert (EQ() + Linear()).select(0).input_scaled_view()[0].terms() == [("eq", 1.0, 1.0), ("linear", 1.0, 1.0)]
    assert Linear().shift(0, 0).terms() is not None and Linear().stretch(1, 1).terms() is not None
    assert Linear().select(None, None).terms() is not None and Linear().transform(None, None).terms() is not None
    for bad in (K.DiffKernel(EQ(), 0, 0), ):
        with pytest.raises(NotImplementedError, match="input maps"):
            bad.select(0)


def _logpdf_calls(be, kernel, x, y):
    del be.calls[:]
    v = T(1.3, True)
    lp = st.GP(v * kernel)(T(x), C.NOISE).logpdf(T(y))
    lp.backward()
    return list(be.calls), float(lp), float(v.grad)


def test_plain_kernel_issues_the_calls_it_always_did(be):
    """Without maps nothing changes: ``1.0 * EQ()`` is a sum of primitives and its log-density and gradient take one kernel-matrix
    launch and one implicit reduction.  (Passes before and after input maps existed.)"""
    d = C.data()
    assert (1.0 * EQ()).terms() == [("eq", 1.0, 1.0)]
    calls, _, _ = _logpdf_calls(be, 1.0 * EQ(), d["x"], d["y"])
    assert calls == ["kmat", "kmat_vjp"]


def test_mapped_spelling_issues_the_same_calls(be):
    d = C.data()
    plain = _logpdf_calls(be, 1.0 * EQ(), d["x"], d["y"])
    mapped = _logpdf_calls(be, 1.0 * EQ().select([0, 1, 2]), d["x"], d["y"])
    assert mapped[0] == plain[0] == ["kmat", "kmat_vjp"]
    assert abs(mapped[1] - plain[1]) <= 1e-12 * abs(plain[1]) and abs(mapped[2] - plain[2]) <= 1e-12 * abs(plain[2])
    f = st.GP(EQ().select([0, 2]))
    var = f(T(d["x"]), 0.1).var
    assert isinstance(var, KernelDense) and var._mat is None                    # lazy: built lower-only, factorised in place


# ---------------------------------------------------------------------------------------------
# 5: means
# ---------------------------------------------------------------------------------------------
def test_means(be):
    x = C.data()["x"]
    m = K.FunctionMean(lambda a: (a ** 2).sum(-1, keepdim=True) + a[..., :1])
    mn = lambda a: (a ** 2).sum(-1, keepdims=True) + a[..., :1]                # noqa: E731
    c = np.array(C.SHIFT_C)
    w = np.array([[0.5, -1.0], [0.2, 0.3], [-0.7, 0.1]])
    C.assert_matrix("shift", m.shift(list(C.SHIFT_C))(T(x)), mn(x - c))
    C.assert_matrix("stretch", m.stretch(2.0)(T(x)), mn(x / 2))
    C.assert_matrix("stretch by a vector", m.stretch([1.0, 2.0, 4.0])(T(x)), mn(x / np.array([1.0, 2.0, 4.0])))
    C.assert_matrix("select", m.select([0, 2])(T(x)), mn(x[:, [0, 2]]))
    C.assert_matrix("transform", m.transform(lambda a: torch.tanh(a @ T(w)))(T(x)), mn(np.tanh(x @ w)))
    C.assert_matrix("a later map acts first", m.shift(0.5).select(1)(T(x)), mn(x[:, [1]] - 0.5))
    C.assert_matrix("sums and scalings", (2.0 * m + 1.0).shift(0.5)(T(x)), 2.0 * mn(x - 0.5) + 1.0)
    for const in (K.ZeroMean(), K.OneMean()):
        assert const.shift(0.5) is const and const.stretch(2.0) is const and const.select(0) is const
        assert const.transform(torch.tanh) is const
    assert isinstance((2.0 * K.OneMean()).shift(0.5).m, K.OneMean)
    with pytest.raises(NotImplementedError, match="derivative mean"):
        m.diff(0).shift(0.5)
    with pytest.raises(NotImplementedError, match="derivatives behind the input map"):
        m.shift(0.5).diff(0)
    tau = T(0.4, True)
    m.shift(tau)(T(x)).sum().backward()
    assert tau.grad is not None


# ---------------------------------------------------------------------------------------------
# 6: processes
# ---------------------------------------------------------------------------------------------
def test_lag_model_kernels(be):
    d = C.data()
    v, s, tau = C.B_P0
    prior, f, g, _ = C.model_b(learn=False)
    xa, xb = d["xa"], d["xb"]
    ks = prior.kernels
    C.assert_matrix("kernels[g]", ks[g].pairwise(T(xb)), C.eq_np(xb - tau, xb - tau, s, v))
    C.assert_matrix("kernels[g, f]", ks[g, f].pairwise(T(xb), T(xa)), C.eq_np(xb - tau, xa, s, v))
    C.assert_matrix("kernels[f, g]", ks[f, g].pairwise(T(xa), T(xb)), C.eq_np(xa, xb - tau, s, v))
    fdd = prior(st.cross(f, g)((f(T(xa)), g(T(xb)))))
    C.assert_matrix("the joint matrix", fdd.var.mat, C.b_matrix(C.B_P0))
    # the shifted mean
    with st.Measure():
        h = st.GP(lambda a: a ** 2, EQ())
        hs = h.shift(0.4)
    C.assert_matrix("mean of the shifted process", hs.mean(T(xa)), (xa - 0.4) ** 2)


def test_select_stretch_transform_of_processes(be):
    d = C.data()
    x3, x1 = d["x"][:40], d["xa"][:30]
    with st.Measure() as prior:
        f = st.GP(1.2 * Matern52().stretch(0.9))
        h = f.select(0)
        u = f.stretch(2.0)
        t = f.transform(lambda a: torch.tanh(a))
        h12 = st.GP(EQ()).select(1, 2)

    def k(a, b):
        return C.m52_np(a, b, 0.9, 1.2)

    fdd = prior(st.cross(h, f)((h(T(x3)), f(T(x1)))))
    ref = np.block([[k(x3[:, [0]], x3[:, [0]]), k(x3[:, [0]], x1)], [k(x1, x3[:, [0]]), k(x1, x1)]])
    C.assert_matrix("f.select(0) at 3-D inputs beside f at 1-D inputs", fdd.var.mat, ref)
    ks = prior.kernels
    C.assert_matrix("cov(f.stretch(2), f)", ks[u, f].pairwise(T(x1), T(x1)), k(x1 / 2, x1))
    C.assert_matrix("cov(f, f.stretch(2))", ks[f, u].pairwise(T(x1), T(x1)), k(x1, x1 / 2))
    C.assert_matrix("var(f.stretch(2))", ks[u].pairwise(T(x1)), k(x1 / 2, x1 / 2))
    C.assert_matrix("cov(f.transform, f)", ks[t, f].pairwise(T(x1), T(x1)), k(np.tanh(x1), x1))
    C.assert_matrix("cov(f.transform, f.stretch)", ks[t, u].pairwise(T(x1), T(x1)), k(np.tanh(x1), x1 / 2))
    C.assert_matrix("select(1, 2)", h12.kernel.pairwise(T(x3)), C.eq_np(x3[:, 1:], x3[:, 1:]))


def test_lag_model_posterior(be):
    d = C.data()
    ref = C.b_posterior_reference()
    prior, f, g, _ = C.model_b(learn=False)
    post = f | (g(T(d["xb"]), C.NOISE_B), T(d["yb"]))
    fdd = post(T(d["xt"]))
    C.assert_close("posterior mean of f given the lagged sensor", fdd.mean[:, 0].numpy(), ref["mean"])
    C.assert_close("posterior variances", fdd.var_diag.numpy(), ref["var"])


def test_a_posterior_conditioned_earlier_refuses_the_mapped_process(be):
    d = C.data()
    with st.Measure() as prior:
        f = st.GP(EQ())
    post = prior | (f(T(d["xa"]), 0.1), T(d["ya"]))
    g = f.shift(0.4)
    assert g.kernel is f.kernel                                                 # (registered in the prior all the same)
    with pytest.raises(K.PosteriorInputMapError, match="conditioned before the mapped process was created"):
        post(g)
    df = f.diff(0)
    with pytest.raises(K.PosteriorDerivativeError, match="conditioned before the derivative process was created"):
        post(df)
    later = prior | (f(T(d["xa"]), 0.1), T(d["ya"]))
    assert later(g)(T(d["xt"])).mean.shape == (C.NS, 1)


# ---------------------------------------------------------------------------------------------
# 7: gradients
# ---------------------------------------------------------------------------------------------
def test_additive_logpdf_gradients(be):
    d = C.data()
    ref = C.a_logpdf_reference()
    k, t = C.model_a()
    tx = T(d["x"], True)
    fdd = st.GP(k)(tx, C.NOISE)
    lp = fdd.logpdf(T(d["y"]))
    assert lp.requires_grad
    C.assert_value("logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    C.assert_close("hyper-parameters", [float(t[n].grad) for n in C.A_NAMES], ref["hyper"])
    C.assert_close("x", C.picked(tx.grad), ref["x"])
    assert be.calls.count("kmat") == 3 and be.calls.count("kmat_vjp_dense") == 3       # one launch and one reduction per group


def test_additive_posterior_marginal_gradients(be):
    d = C.data()
    ref = C.a_marginals_reference()
    k, t = C.model_a()
    f = st.GP(k)
    tx = T(d["x"], True)
    fdd = (f | (f(tx, C.NOISE_MARGINALS), T(d["y"])))(T(d["xs"]))
    loss = fdd.mean.sum() + fdd.var_diag.sum()
    assert loss.requires_grad
    C.assert_value("loss", float(loss.detach()), ref["value"])
    loss.backward()
    C.assert_close("hyper-parameters", [float(t[n].grad) for n in C.A_NAMES], ref["hyper"])
    C.assert_close("x", C.picked(tx.grad), ref["x"])


def test_lag_joint_logpdf_gradients(be):
    d = C.data()
    ref = C.b_joint_reference()
    prior, f, g, t = C.model_b()
    lp = prior.logpdf((f(T(d["xa"]), C.NOISE), T(d["ya"])), (g(T(d["xb"]), C.NOISE_B), T(d["yb"])))
    assert lp.requires_grad
    C.assert_value("joint logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    C.assert_close("(v, s, tau)", [float(t[n].grad) for n in C.B_NAMES], ref["hyper"])


def test_deep_kernel_logpdf_gradients(be):
    d = C.data()
    ref = C.c_logpdf_reference()
    k, v, fn = C.model_c()
    lp = st.GP(k)(T(d["x"]), C.NOISE).logpdf(T(d["y"]))
    assert lp.requires_grad
    C.assert_value("logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    C.assert_close("variance and the 24 network entries", np.concatenate([[float(v.grad)], fn.grads()]), ref["params"])


def test_deep_kernel_bound_gradients(be):
    d = C.data()
    ref = C.c_elbo_reference()
    k, v, fn = C.model_c(learn=("w2",), w2_scale=C.W2_BOUND)
    f = st.GP(k)
    z = T(d["z"], True)
    elbo = st.PseudoObs(f(z), f(T(d["x"]), C.NOISE), T(d["y"])).elbo(f.measure)
    assert elbo.requires_grad
    C.assert_value("bound", float(elbo.detach()), ref["value"])
    elbo.backward()
    got = np.concatenate([[float(v.grad)], fn.w2.grad.numpy().ravel(), z.grad.numpy().ravel()])
    C.assert_close("variance, W2 and the inducing inputs", got, ref["params"])


# ---------------------------------------------------------------------------------------------
# 8: refusals and loudness
# ---------------------------------------------------------------------------------------------
def test_refusals(be):
    fn = lambda a: torch.tanh(a)                                                # noqa: E731
    for k in (EQ().select(0), Linear().shift(0.5), EQ().transform(fn), Linear().shift(0.5, 0)):
        with pytest.raises(NotImplementedError, match="derivatives behind the input map"):
            k.diff(0)
        with pytest.raises(NotImplementedError, match="periodic is implemented for sums of primitive kernels"):
            k.periodic(2.0)
    with pytest.raises(NotImplementedError, match="two-argument stretch takes scalars"):
        EQ().stretch([1.0, 2.0], 1)
    with pytest.raises(NotImplementedError, match="two-argument stretch takes scalars"):
        EQ().stretch(1.0, T([1.0, 2.0]))
    d = C.data()
    with st.Measure() as prior:
        f = st.GP(EQ())
    post = prior | (f(T(d["xa"]), 0.1), T(d["ya"]))
    for op in (lambda k: k.shift(0.5, 0), lambda k: k.select(0), lambda k: k.transform(fn), lambda k: k.stretch(2.0, 1)):
        with pytest.raises(NotImplementedError, match="posterior kernels"):
            op(post.kernels[f])
    with pytest.raises(NotImplementedError, match="posterior means"):
        post.means[f].shift(0.5)
    with pytest.raises(NotImplementedError, match="input maps"):
        st.cross(f, f).kernel.select(0)


def test_nine_features_with_learnable_inputs_are_refused_before_any_launch(be):
    d = C.data()
    w = T(np.random.default_rng(3).standard_normal((3, 9)))
    k = EQ().transform(lambda a: a @ w)
    del be.calls[:]
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        st.GP(k)(T(d["x"], True), C.NOISE).logpdf(T(d["y"]))
    assert be.calls == []
    lp = st.GP(T(1.0, True) * k)(T(d["x"]), C.NOISE).logpdf(T(d["y"]))           # (a learnable variance alone: any dimension)
    assert lp.requires_grad
    with torch.no_grad():
        lp0 = st.GP(k)(T(d["x"], True), C.NOISE).logpdf(T(d["y"]))
    ref = C.logpdf_np(C.eq_np(d["x"] @ w.numpy(), d["x"] @ w.numpy()) + (C.NOISE + C.EPS) * np.eye(C.N), d["y"])
    assert not lp0.requires_grad
    C.assert_value("the refused call under no_grad", float(lp0), ref)


def test_transform_learnability_rule(be):
    d = C.data()
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Tanh(), torch.nn.Linear(4, 2)).double()
    m = K._TransformMap(net)
    assert m.requires_grad                          # (never evaluated: unknown counts as learnable)
    m(T(d["x"]))
    assert m.requires_grad                          # (probed: the parameters require a gradient)
    for p in net.parameters():
        p.requires_grad_(False)
    assert not m.requires_grad
    assert m._probe.shape == (1, 3) and m._probe.untyped_storage().nbytes() == 3 * 8       # one row of its own, not the input's storage

    class Closing(torch.nn.Module):                 # a module whose forward closes over a learnable tensor that is no parameter
        def __init__(self):
            super().__init__()
            self.w = T(np.eye(3), True)

        def forward(self, a):
            return a @ self.w

    hidden = K._TransformMap(Closing())
    hidden(T(d["xbatch"]))
    assert hidden.requires_grad and hidden._probe.shape == (1, 3)
    w = T(np.eye(3), True)
    closure = K._TransformMap(lambda a: a @ w)
    assert closure.requires_grad                    # (never evaluated: unknown counts as learnable)
    closure(T(d["x"]))
    assert closure.requires_grad                    # (probed: the output of the first row requires a gradient)
    fixed = K._TransformMap(lambda a: torch.tanh(a))
    fixed(T(d["x"]))
    assert not fixed.requires_grad
    from stheno_amd import learnable as ag
    frozen = EQ().transform(net)
    frozen.pairwise(T(d["x"]))
    assert ag.kernel_requires_grad(frozen) is False
    assert ag.kernel_requires_grad(Linear().shift(T(0.4, True)))
    assert not ag.kernel_requires_grad(Linear().shift(0.4))


def test_learnable_lag_under_a_pseudo_point_posterior_is_loud(be):
    d = C.data()
    prior, f, g, t = C.model_b()
    obs = st.PseudoObs(f(T(d["xt"][:8])), f(T(d["xa"]), C.NOISE), T(d["ya"]))
    post = prior | obs
    with pytest.raises(NotImplementedError, match="cut off from the autograd graph"):
        post(g)(T(d["xb"]), C.NOISE_B).logpdf(T(d["yb"]))
    with torch.no_grad():
        lp = post(g)(T(d["xb"]), C.NOISE_B).logpdf(T(d["yb"]))
    assert np.isfinite(float(lp)) and not lp.requires_grad


def test_bound_over_a_mapped_process_is_loud(be):
    """Inducing points on ``f``, data on ``g = f.shift(tau)`` with a learnable lag: the lag sits in the data's kernel and the
    cross-kernel only, outside the differentiable bound -- refused, not returned without a graph."""
    d = C.data()
    prior, f, g, t = C.model_b()
    t["v"].requires_grad_(False), t["s"].requires_grad_(False)
    obs = st.PseudoObs(f(T(d["xt"][:8])), g(T(d["xb"]), C.NOISE_B), T(d["yb"]))
    with pytest.raises(NotImplementedError, match="gradients of the bound are implemented for noise-free inducing points of the observed"):
        obs.elbo(prior)
    with torch.no_grad():
        value = obs.elbo(prior)
    assert np.isfinite(float(value)) and not value.requires_grad
    # nothing learnable behind the map: a value, as before
    prior, f, g, _ = C.model_b(learn=False)
    value = st.PseudoObs(f(T(d["xt"][:8])), g(T(d["xb"]), C.NOISE_B), T(d["yb"])).elbo(prior)
    assert np.isfinite(float(value)) and not value.requires_grad


# ---------------------------------------------------------------------------------------------
# kernels that carry their own map: the two-argument stretch, processes, and scaled sums inside a multi-process matrix
# ---------------------------------------------------------------------------------------------
def test_stretch_of_processes_with_a_bare_periodic_or_per_dimension_kernel(be):
    d = C.data()
    x = d["x"][:40, :2]
    ls = np.array([0.8, 1.7])
    cases = [
        (EQ().periodic(3.1), lambda a, b: C.eq_np(C.pmap(a, 3.1), C.pmap(b, 3.1))),
        (EQ().stretch([0.8, 1.7]), lambda a, b: C.eq_np(a / ls, b / ls)),
    ]
    for k, ref in cases:
        C.assert_matrix("k.stretch(2, 1)", k.stretch(2.0, 1).pairwise(T(x), T(x)), ref(x / 2, x))
        C.assert_matrix("k.stretch(1, 2)", k.stretch(1, 2.0).pairwise(T(x), T(x)), ref(x, x / 2))
        with st.Measure() as prior:
            f = st.GP(k)
            u = f.stretch(2.0)
        ks = prior.kernels
        C.assert_matrix("cov(f.stretch(2), f)", ks[u, f].pairwise(T(x), T(x)), ref(x / 2, x))
        C.assert_matrix("cov(f, f.stretch(2))", ks[f, u].pairwise(T(x), T(x)), ref(x, x / 2))
        fdd = prior(st.cross(u, f)((u(T(x)), f(T(x)))))
        C.assert_matrix("the joint matrix", fdd.var.mat, np.block([[ref(x / 2, x / 2), ref(x / 2, x)], [ref(x, x / 2), ref(x, x)]]))
    # the one-argument stretch of these kernels is what it was
    assert isinstance(EQ().periodic(3.1).stretch(2.0), K.Periodic) and isinstance(EQ().stretch([0.8, 1.7]).stretch(2.0), K.InputScaled)
    with st.Measure():
        f = st.GP(EQ())
        with pytest.raises(NotImplementedError, match="one length scale per input dimension"):
            f.stretch([1.0, 2.0])


def test_scaled_sum_behind_different_maps_inside_a_multi_process_matrix(be):
    """``h = 2 (f1 + f2)`` with ``f1`` behind per-dimension scales and ``f2`` periodic: the kernel of ``h`` is a ``Scaled`` around a sum
    that has no common map.  Its blocks go group by group into the multi-process matrix."""
    d = C.data()
    x, y = d["x"][:30, :2], d["y"][:30]
    ls = np.array([1.0, 2.0])

    def k1(a, b):
        return C.eq_np(a / ls, b / ls)

    def k2(a, b):
        return C.eq_np(C.pmap(a, 3.0), C.pmap(b, 3.0))

    k = 2.0 * (EQ().stretch([1.0, 2.0]) + EQ().periodic(3.0))
    assert k.input_scaled_view() is None and len(K._map_groups(k)) == 2
    buf = torch.full((34, 33), float("nan"), dtype=torch.float64)
    view = buf[2:32, 1:31]
    del be.calls[:]
    K._eval_into(k, T(x), T(x), view)
    assert be.calls == ["kmat", "kmat"]
    C.assert_matrix("the block", view, 2.0 * (k1(x, x) + k2(x, x)))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[2:32, 1:31] = False
    assert bool(torch.isnan(buf[outside]).all())
    C.assert_matrix("without a view: the product, as always", k.pairwise(T(x), T(x)), 2.0 * (k1(x, x) + k2(x, x)))
    with st.Measure() as prior:
        f1, f2 = st.GP(EQ().stretch([1.0, 2.0])), st.GP(EQ().periodic(3.0))
        h = 2.0 * (f1 + f2)
    fdd = prior(st.cross(h, f1)((h(T(x)), f1(T(x)))))
    ref = np.block([[4.0 * (k1(x, x) + k2(x, x)), 2.0 * k1(x, x)], [2.0 * k1(x, x), k1(x, x)]])
    C.assert_matrix("the joint matrix", fdd.var.mat, ref)
    lp = prior.logpdf((h(T(x), 0.1), T(y)), (f1(T(x), 0.1), T(y)))
    C.assert_value("joint logpdf", float(lp), C.logpdf_np(ref + (0.1 + C.EPS) * np.eye(60), np.concatenate([y, y])))
