"""Rational-quadratic terms and periodic kernels on the fused kernel-matrix path (MI355X).

The reference is closed-form NumPy in fp64, written out here (the test suite's CPU backend does not know ``"rq"``):
``RQ_alpha(q) = (1 + q / (2 alpha))^(-alpha)``, ``q = |x - y|^2 / scale^2``, and ``k.periodic(p)`` is ``k`` on
``(sin(2 pi x / p), cos(2 pi x / p))``.  Values are held to the project's parity bar -- 1e-6 of the largest entry in fp64, 1e-3 in
fp32 (the element-by-element figure against an 80-bit reference belongs to the native self-test, ``gpk_selftest --rq``); gradients
to the tolerances of ``tests/test_autograd.py`` / ``tests/test_posterior_grad_gpu.py``: 1e-6 of ``max(|reference|, 1)`` against
central finite differences of the closed form.

Shapes sit at the kernel's seams: the 32-row tile and its 8 rows per wave (N = 1, 33, 130), partial and several 64 x VEC column
tiles (M = 7, 64, 257), every dimension chunk (D = 1, 3, 8 -> DC = 1, 4, 8; D = 2 in the gradient cases), the vector-store switch
(``ld = m + 4``), the dedicated program against the term table.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl
import torch

import stheno_amd.torch as st
from stheno_amd import _native, ops
from stheno_amd.torch import EQ, RQ, Linear

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-6, torch.float32: 1e-3}
DTYPES = [torch.float64, torch.float32]
ALPHAS = (0.1, 1.0, 50.0)
SCALES = (0.5, 3.0)


# ---------------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------------
def d2(a, b):
    return ((a[..., :, None, :] - b[..., None, :, :]) ** 2).sum(-1)


def rq_np(a, b, alpha, scale, var=1.0):
    return var * np.exp(-alpha * np.log1p(d2(a, b) / scale**2 / (2 * alpha)))


def eq_np(a, b, scale=1.0, var=1.0):
    return var * np.exp(-0.5 * d2(a, b) / scale**2)


def lin_np(a, b, var=1.0):
    return var * (a @ np.swapaxes(b, -1, -2))


def pmap(x, p):
    a = 2 * np.pi * x / p
    return np.concatenate([np.sin(a), np.cos(a)], axis=-1)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def close(got, ref, dtype):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= TOL[dtype] * np.max(np.abs(ref)), np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def inputs(n, m, d, dtype, seed=0):
    rng = np.random.default_rng(seed + 1000 * n + 10 * m + d)
    x = rng.standard_normal((n, d)).astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)
    y = rng.standard_normal((m, d)).astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)
    return x, y


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("m", [7, 64, 257])
@pytest.mark.parametrize("n", [1, 33, 130])
def test_rq_single_term_values(hip_backend, n, m, d, dtype):
    x, y = inputs(n, m, d, dtype)
    for alpha in ALPHAS:
        for scale in SCALES:
            k = 1.3 * RQ(alpha).stretch(scale)
            close(k.pairwise(dev(x, dtype), dev(y, dtype)), rq_np(x, y, alpha, scale, 1.3), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("n,m", [(1, 7), (33, 64), (130, 257)])
def test_rq_in_a_sum_takes_the_term_table(hip_backend, n, m, d, dtype):
    x, y = inputs(n, m, d, dtype, seed=1)
    for alpha in ALPHAS:
        for scale in SCALES:
            k = 0.7 * RQ(alpha).stretch(scale) + 1.1 * EQ().stretch(1.4) + 0.3 * Linear()
            assert [t[0] for t in k.terms()] == ["rq", "eq", "linear"] and k.shapes() == [alpha, None, None]
            ref = rq_np(x, y, alpha, scale, 0.7) + eq_np(x, y, 1.4, 1.1) + lin_np(x, y, 0.3)
            close(k.pairwise(dev(x, dtype), dev(y, dtype)), ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("generic", [False, True], ids=["own-program", "term-table"])
@pytest.mark.parametrize("n,d", [(33, 1), (130, 3), (257, 8)])
def test_rq_symmetric_lower_and_diagonal(hip_backend, n, d, generic, dtype):
    x, _ = inputs(n, 1, d, dtype, seed=2)
    alpha, scale = 1.0, 0.5
    k = 0.9 * RQ(alpha).stretch(scale)
    ref = rq_np(x, x, alpha, scale, 0.9)
    if generic:
        k = k + 0.2 * Linear()
        ref = ref + lin_np(x, x, 0.2)
    tx = dev(x, dtype)
    dv = np.linspace(0.1, 0.7, n)
    close(k.pairwise(tx), ref, dtype)
    full = k.pairwise(tx, diag_add=0.25, diag_vec=dev(dv, dtype))
    close(full, ref + np.diag(0.25 + dv), dtype)
    low = k.pairwise(tx, lower=True, diag_add=0.25, diag_vec=dev(dv, dtype))
    close(torch.tril(low), np.tril(ref + np.diag(0.25 + dv)), dtype)
    assert torch.equal(torch.tril(low), torch.tril(full))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,m,d", [(33, 64, 3), (130, 257, 8)])
def test_rq_out_view_accumulate_and_batch(hip_backend, n, m, d, dtype):
    x, y = inputs(n, m, d, dtype, seed=3)
    alpha, scale = 0.1, 3.0
    k = RQ(alpha).stretch(scale)
    ref = rq_np(x, y, alpha, scale)
    tx, ty = dev(x, dtype), dev(y, dtype)
    # a strided view: ld = m + 4 elements (rows off the 16-byte grid for fp64 odd m -> the scalar store path), padding untouched
    buf = torch.full((n, m + 4), -7.0, dtype=dtype, device="cuda")
    out = k.pairwise(tx, ty, out=buf[:, :m])
    assert out.data_ptr() == buf.data_ptr()
    close(buf[:, :m], ref, dtype)
    assert bool((buf[:, m:] == -7.0).all())
    # accumulate into what is there
    base = np.random.default_rng(5).standard_normal((n, m))
    acc = dev(base, dtype)
    hip_backend.kmat(ops.KTerms(k.terms(), k.shapes()), tx, ty, out=acc, accumulate=True)
    close(acc, base.astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64) + ref, dtype)
    # a batch of two
    x2, y2 = inputs(n, m, d, dtype, seed=4)
    xb, yb = np.stack([x, x2]), np.stack([y, y2])
    close(k.pairwise(dev(xb, dtype), dev(yb, dtype)), np.stack([ref, rq_np(x2, y2, alpha, scale)]), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_rq_elwise_duplicates_and_nan(hip_backend, dtype):
    n, m, d = 130, 257, 3
    x, y = inputs(n, m, d, dtype, seed=6)
    y[5] = x[40]                                   # a row of y equal to a row of x
    v = torch.tensor(1.3, dtype=dtype)
    # (the last one goes through the term table: a constant term beside the RQ term)
    for k, want in ((1.3 * RQ(0.1).stretch(0.5), v), (1.3 * RQ(50.0).stretch(3.0), v),
                    (1.3 * RQ(1.0) + 0.25 * st.OneKernel(), v + torch.tensor(0.25, dtype=dtype))):
        tx, ty = dev(x, dtype), dev(y, dtype)
        kxy = k.pairwise(tx, ty)
        assert float(kxy[40, 5]) == float(want), "k(x, x) must be exactly the variance"
        kxx = k.pairwise(tx)
        assert torch.equal(torch.diagonal(kxx), k.elwise(tx)[:, 0])
        xn = x.copy()
        xn[33, 1] = np.nan
        kn = k.pairwise(dev(xn, dtype), ty)
        assert bool(torch.isnan(kn[33]).all()) and not bool(torch.isnan(kn[:33]).any()) and not bool(torch.isnan(kn[34:]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_kmat_s_without_rq_terms_is_bit_identical_to_kmat(hip_backend, dtype):
    n, d = 130, 3
    x = dev(inputs(n, 1, d, dtype, seed=7)[0], dtype)
    terms = ops.KTerms([("eq", 0.8, 1.1)])
    want = hip_backend.kmat(terms, x, None, diag_add=0.1)
    got = torch.empty_like(want)
    kinds, var, ils, nt = terms.c_arrays()
    shapes = (ctypes.c_double * 1)(7.0)            # ignored: EQ has no shape parameter
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for sh in (shapes, None):
        got.fill_(-1.0)
        code = hip_backend.lib.gpk_kmat(_native.GPK_F64 if dtype == torch.float64 else _native.GPK_F32, kinds, var, ils, sh, nt,
                                        p(x), n, d, 0, p(x), n, d, 0, d, p(got), got.stride(0), 0, 1, 0, 1, 0.1, None, 0, 0,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == 0
        assert torch.equal(got, want)
    # ... and an RQ term without a shapes array is an argument error, not a silent alpha
    rq = (ctypes.c_int * 1)(_native.K_RQ)
    code = hip_backend.lib.gpk_kmat(_native.GPK_F64 if dtype == torch.float64 else _native.GPK_F32, rq, var, ils, None, 1, p(x), n, d, 0,
                                    p(x), n, d, 0, d, p(got), got.stride(0), 0, 1, 0, 1, 0.1, None, 0, 0,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code < 0


# ---------------------------------------------------------------------------------------------
# gradients (fp64) against central finite differences of the closed form
# ---------------------------------------------------------------------------------------------
EPS = 1e-10
N, NS, M = 130, 33, 33


def fd_grad(fun, p, h=1e-6):
    g = np.zeros_like(p)
    for i in range(p.size):
        e = np.zeros_like(p)
        e.flat[i] = h
        g.flat[i] = (fun(p + e) - fun(p - e)) / (2 * h)
    return g


def kern_np(a, b, v, s, alpha, period):
    """``v * RQ(alpha).stretch(s)``, behind the periodic map when ``period`` is given."""
    if period is not None:
        a, b = pmap(a, period), pmap(b, period)
    return rq_np(a, b, alpha, s, v)


def logpdf_np(k, y):
    l = np.linalg.cholesky(k)
    w = sl.solve_triangular(l, y, lower=True)
    return float(-0.5 * (2 * np.sum(np.log(np.diag(l))) + len(y) * np.log(2 * np.pi) + np.sum(w * w)))


def elbo_np(kf, x, z, y, noise):
    m = z.shape[0]
    l_z = np.linalg.cholesky(kf(z, z) + EPS * np.eye(m))
    v = sl.solve_triangular(l_z, kf(z, x), lower=True)
    a = np.eye(m) + (v / noise) @ v.T
    l_a = np.linalg.cholesky(a + EPS * np.eye(m))
    u = sl.solve_triangular(l_a, (v / noise) @ y, lower=True)
    kd = np.array([kf(x[i:i + 1], x[i:i + 1])[0, 0] for i in range(x.shape[0])])
    trace = np.sum((kd - (v * v).sum(0)) / noise)
    return float(-0.5 * (x.shape[0] * np.log(2 * np.pi * noise) + 2 * np.sum(np.log(np.diag(l_a))) + np.sum(y[:, 0] ** 2) / noise
                         - np.sum(u**2) + trace))


def post_np(kf, x, y, xs, noise):
    k = kf(x, x) + (noise + EPS) * np.eye(x.shape[0])
    l = np.linalg.cholesky(k)
    v = sl.solve_triangular(l, kf(x, xs), lower=True)
    w = sl.solve_triangular(l, y, lower=True)
    kd = np.array([kf(xs[i:i + 1], xs[i:i + 1])[0, 0] for i in range(xs.shape[0])])
    return (v.T @ w)[:, 0], kd - (v * v).sum(0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(42)
    x = rng.uniform(-2.0, 2.0, (N, 2))
    xs = rng.uniform(-2.0, 2.0, (NS, 2))
    z = rng.uniform(-2.0, 2.0, (M, 2))
    y = np.sin(x[:, :1]) + 0.3 * rng.standard_normal((N, 1))
    return x, xs, z, y


P0 = dict(v=1.2, s=0.9, alpha=0.8, period=3.1)
NOISE = 0.3


def torch_model(x, periodic, grad_x):
    par = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in P0.items()}
    k = par["v"] * RQ(par["alpha"]).stretch(par["s"])
    if periodic:
        k = k.periodic(par["period"])
    tx = torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=grad_x)
    return st.GP(k), par, tx


def check_grads(objective_np, par, tx, x, periodic):
    """``objective_np(v, s, alpha, period, x)``: the closed form; the autograd gradients sit in ``par`` / ``tx``."""
    names = ["v", "s", "alpha"] + (["period"] if periodic else [])
    p0 = np.array([P0[k] for k in names])

    def of_params(p):
        kw = dict(zip(names, p))
        return objective_np(kw["v"], kw["s"], kw["alpha"], kw.get("period"), x)

    ref = fd_grad(of_params, p0)
    got = np.array([float(par[k].grad) for k in names])
    print("hyper-parameters", names, "autograd", got, "finite differences", ref)
    assert np.max(np.abs(got - ref)) <= 1e-6 * max(np.max(np.abs(ref)), 1.0), (got, ref)
    if tx.grad is not None:
        refx = fd_grad(lambda xx: objective_np(P0["v"], P0["s"], P0["alpha"], P0["period"] if periodic else None, xx.reshape(x.shape)),
                       x.copy().ravel()).reshape(x.shape)
        gotx = tx.grad.cpu().numpy()
        print("inputs: worst deviation", np.max(np.abs(gotx - refx)), "largest entry", np.max(np.abs(refx)))
        assert np.max(np.abs(gotx - refx)) <= 1e-6 * max(np.max(np.abs(refx)), 1.0)


@pytest.fixture()
def eps():
    old = st.B.epsilon
    st.B.epsilon = EPS
    yield
    st.B.epsilon = old


@pytest.mark.parametrize("periodic", [False, True], ids=["rq", "rq-periodic"])
def test_logpdf_gradients(hip_backend, eps, data, periodic):
    x, _, _, y = data
    f, par, tx = torch_model(x, periodic, grad_x=True)

    def obj(v, s, alpha, period, xx):
        return logpdf_np(kern_np(xx, xx, v, s, alpha, period) + (NOISE + EPS) * np.eye(N), y)

    lp = f(tx, NOISE).logpdf(dev(y))
    want = obj(P0["v"], P0["s"], P0["alpha"], P0["period"] if periodic else None, x)
    assert lp.requires_grad and abs(float(lp) - want) <= 1e-6 * abs(want)
    lp.backward()
    check_grads(obj, par, tx, x, periodic)


@pytest.mark.parametrize("periodic", [False, True], ids=["rq", "rq-periodic"])
def test_vfe_elbo_gradients(hip_backend, eps, data, periodic):
    x, _, z, y = data
    f, par, tx = torch_model(x, periodic, grad_x=True)

    def obj(v, s, alpha, period, xx):
        return elbo_np(lambda a, b: kern_np(a, b, v, s, alpha, period), xx, z, y, NOISE)

    obs = st.PseudoObs(f(dev(z)), f(tx, NOISE), dev(y))
    elbo = obs.elbo(f.measure)
    want = obj(P0["v"], P0["s"], P0["alpha"], P0["period"] if periodic else None, x)
    assert elbo.requires_grad and abs(float(elbo) - want) <= 1e-6 * abs(want)
    elbo.backward()
    check_grads(obj, par, tx, x, periodic)


@pytest.mark.parametrize("periodic", [False, True], ids=["rq", "rq-periodic"])
def test_posterior_marginal_gradients(hip_backend, eps, data, periodic):
    x, xs, _, y = data
    f, par, tx = torch_model(x, periodic, grad_x=True)

    def obj(v, s, alpha, period, xx):
        mu, var = post_np(lambda a, b: kern_np(a, b, v, s, alpha, period), xx, y, xs, NOISE)
        return float(mu.sum() + var.sum())

    post = f | (f(tx, NOISE), dev(y))
    fdd = post(dev(xs))
    loss = fdd.mean.sum() + fdd.var_diag.sum()
    want = obj(P0["v"], P0["s"], P0["alpha"], P0["period"] if periodic else None, x)
    assert loss.requires_grad and abs(float(loss) - want) <= 1e-6 * abs(want)
    loss.backward()
    check_grads(obj, par, tx, x, periodic)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def test_periodic_gp_condition_and_predict(hip_backend, eps):
    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(0.0, 20.0, N))[:, None]
    xs = np.linspace(0.0, 20.0, NS)[:, None]
    y = np.sin(2 * np.pi * x / 5.0) + 0.2 * rng.standard_normal((N, 1))

    def kf(a, b):
        return eq_np(pmap(a, 5.0), pmap(b, 5.0))

    f = st.GP(EQ().periodic(5.0))
    fdd = f(dev(x), 0.1)
    lp = float(fdd.logpdf(dev(y)))
    post = f | (fdd, dev(y))
    mean, var = post(dev(xs)).marginals()
    ref_lp = logpdf_np(kf(x, x) + (0.1 + EPS) * np.eye(N), y)
    ref_mean, ref_var = post_np(kf, x, y, xs, 0.1)
    assert abs(lp - ref_lp) <= 1e-6 * abs(ref_lp)
    close(mean.reshape(-1), ref_mean, torch.float64)
    close(var.reshape(-1), ref_var, torch.float64)
    # ... and exactly periodic: the prediction one period on is the same prediction
    mean2, _ = post(dev(xs + 5.0)).marginals()
    close(mean2.reshape(-1), ref_mean, torch.float64)


def test_decomposition_components_add_up(hip_backend, eps):
    rng = np.random.default_rng(4)
    x = np.sort(rng.uniform(0.0, 10.0, N))[:, None]
    xs = np.linspace(0.0, 10.0, NS)[:, None]
    y = np.sin(x) + 0.1 * x + 0.2 * rng.standard_normal((N, 1))
    with st.Measure() as prior:
        f_smooth = st.GP(EQ())
        f_wiggly = st.GP(RQ(1e-1).stretch(0.5))
        f_periodic = st.GP(EQ().periodic(1.0))
        f_linear = st.GP(Linear())
        f = f_smooth + f_wiggly + f_periodic + f_linear
    post = prior | (f(dev(x), 0.05), dev(y))
    txs = dev(xs)
    total = post(f)(txs).mean
    parts = [post(p)(txs).mean for p in (f_smooth, f_wiggly, f_periodic, f_linear)]
    assert all(float(p.abs().max()) > 0 for p in parts)
    assert float((sum(parts) - total).abs().max()) <= 1e-8 * float(total.abs().max())
    # the sum's kernel against the closed form: four groups of terms behind three different input maps, one buffer
    ref = eq_np(x, x) + rq_np(x, x, 1e-1, 0.5) + eq_np(pmap(x, 1.0), pmap(x, 1.0)) + lin_np(x, x)
    close(f.kernel.pairwise(dev(x)), ref, torch.float64)
