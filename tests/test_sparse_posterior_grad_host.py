"""Gradients through the mean and the marginal variances of a pseudo-point posterior ``f | PseudoObs(f(z), f(x, noise), y)`` (VFE,
FITC, DTC; ``.mean``, ``.var_diag``, ``.marginals()``, ``.marginal_credible_bounds()``; ``autograd._SparsePosteriorMarginals``) -- the
host logic on a test-only NumPy backend: ``OracleBackend`` with distances by direct differences (the Matern kernels are exact on the
diagonal), the rational-quadratic kind with the sums for its shape parameter, and the transposed solve.  Reference:
``tests/sparse_posterior_reference.py``, a dense fp64 torch formula differentiated by torch autograd.

Acceptance, the project's own (``tests/test_posterior_grad_gpu.py``, ``test_elbo_gradients_host_logic``): the forward values agree with
the reference to 1e-9 of the largest entry BEFORE any gradient is compared; gradients ``max |got - ref| <= tol max(max |ref|, 1)`` with
``tol = 5e-6`` for the host logic.  The inducing inputs are a jittered grid over the data's range; at these cases the reference's own
gradients move by about 1e-9 (relative, same norm) when the jitter goes from 1e-12 to 1e-10 --
``test_reference_is_stable_under_the_jitter`` holds it to a tenth of the tolerance, here and at the shapes of the GPU tests."""
import math

import numpy as np
import pytest
import torch

import stheno_amd as st
from stheno_amd import ops

from . import sparse_posterior_reference as R
from .conftest import OracleBackend, _np

KINDS = {"eq": st.EQ, "matern12": st.Matern12, "matern52": st.Matern52, "linear": st.Linear}
OBS = {"vfe": st.PseudoObs, "fitc": st.PseudoObsFITC, "dtc": st.PseudoObsDTC}
N, M, NS = 90, 12, 17
TOL = 5e-6


def _profile(kind, q, shape):
    """``(kappa, d kappa / dq, d kappa / d shape)`` at ``q`` (the squared scaled distance; the scaled dot product for ``linear``)."""
    if kind == "eq":
        k = np.exp(-0.5 * q)
        return k, -0.5 * k, None
    if kind == "matern12":
        r = np.sqrt(q)
        k = np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            return k, np.where(r > 0, -0.5 * k / r, 0.0), None
    if kind == "matern52":
        s = np.sqrt(5 * q)
        return (1 + s + s * s / 3) * np.exp(-s), -(5.0 / 6.0) * (1 + s) * np.exp(-s), None
    if kind == "rq":
        b = 1.0 + q / (2.0 * shape)
        k = np.exp(-shape * np.log(b))
        return k, -0.5 * k / b, k * (-np.log(b) + (q / (2.0 * shape)) / b)
    if kind == "linear":
        return q, np.ones_like(q), None
    raise NotImplementedError(kind)


def _q(kind, a, b, scale):
    return (a @ b.T if kind == "linear" else ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)) / scale**2


class SparseOracle(OracleBackend):
    """``OracleBackend`` with distances by direct differences, the ``"rq"`` kind (values, the third column of the sums, input
    gradients) and ``tri_solve_t_`` -- and ``calls``, the names of the launches in the order the host logic made them."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _shapes(terms):
        return terms.shapes if terms.shapes is not None else [None] * len(terms)

    def kmat(self, terms, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        self.calls.append("kmat")
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
        self.calls.append("tri_solve_t_")
        L = np.tril(_np(l))
        b.copy_(self._t(np.linalg.solve(L.T, _np(b)), b))
        return b

    def gemm(self, a, b, **kw):
        self.calls.append("gemm")
        return super().gemm(a, b, **kw)

    def kmat_vjp_dense(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        self.calls.append("kmat_vjp_dense")
        Ge = _np(g).copy()
        if colscale is not None:
            Ge = Ge * _np(colscale)[None, :]
        if w is not None:
            Ge = Ge + _np(w)[:, None] * _np(b)[None, :]
        xs, ys = _np(x), _np(y)
        ns = 3 if terms.shapes is not None else 2
        S, kfull, gx = np.zeros((len(terms), ns)), np.zeros_like(Ge), np.zeros_like(xs)
        for t, ((kind, var, scale), shp) in enumerate(zip(terms.terms, self._shapes(terms))):
            q = _q(kind, xs, ys, scale)
            k, dk, da = _profile(kind, q, shp)
            S[t, 0] = np.sum(Ge * k)
            S[t, 1] = np.sum(Ge * (-0.5 * np.sqrt(q) * k if kind == "matern12" else dk * q))
            if da is not None:
                S[t, 2] = np.sum(Ge * da)
            kfull += var * k
            if kind == "linear":
                gx += (Ge * var / scale**2) @ ys
            else:
                coef = Ge * var * dk * 2 / scale**2
                gx += coef.sum(1)[:, None] * xs - coef @ ys
        return (self._t(S, x), self._t((Ge * kfull).sum(0), x) if want_colsum else None, self._t(gx, x) if want_gradx else None)


@pytest.fixture()
def be():
    backend = SparseOracle()
    prev = ops.set_backend(backend)
    yield backend
    ops.set_backend(prev)


def inducing_grid(rng, m, d, span=2.0):
    """``m`` inducing inputs spread over ``[-span, span]^d``: a grid along the first dimension, Kronecker sequences (multiples of
    sqrt(2), sqrt(3), ... modulo one) along the others, jittered -- well separated, so that ``K_z`` is well conditioned."""
    t = (np.arange(m) + 0.5) / m
    cols = [t] + [np.mod(0.5 + (np.arange(m) + 1) * math.sqrt(prime), 1.0) for prime in (2, 3, 5, 7, 11, 13, 17, 19)[: d - 1]]
    return span * (2.0 * np.stack(cols, axis=1) - 1.0) + 0.02 * rng.standard_normal((m, d))


def make_case(kinds, *, d=2, n=N, m=M, ns=NS, imap=None, per_point=False, seed=0, rq_alpha=False, span=2.0):
    rng = np.random.default_rng(seed)
    p = dict(x=rng.uniform(-span, span, (n, d)), z=inducing_grid(rng, m, d, span), xs=rng.uniform(-span, span, (ns, d)),
             y=rng.standard_normal((n, 1)),
             lv=np.log(rng.uniform(0.5, 1.5, len(kinds))), ls=np.log(rng.uniform(0.9, 1.5, len(kinds))), c=np.array(0.3),
             lnoise=np.log(rng.uniform(0.1, 0.3, n)) if per_point else np.array(np.log(0.2)))
    if rq_alpha:
        p["la"] = np.log(rng.uniform(0.8, 2.0, len(kinds)))
    if imap == "ard":
        p["map"] = np.log(rng.uniform(0.8, 1.5, d))
    elif imap == "periodic":
        p["map"] = np.log(np.array(3.1))
    return p, rng.uniform(0.5, 1.5, ns)


def leaves(p, names, dtype=torch.float64, dev="cpu"):
    return {k: torch.tensor(v, dtype=dtype, device=dev, requires_grad=k in names) for k, v in p.items()}


def build(P, kinds, method, imap=None, mean_fn=True):
    """The model under test from the leaves ``P``: ``(f, obs, post)``."""
    vs, ss = torch.exp(P["lv"]), torch.exp(P["ls"])
    prims = [st.RQ(torch.exp(P["la"][i])) if k == "rq" else KINDS[k]() for i, k in enumerate(kinds)]
    kernel = sum(vs[i] * prims[i].stretch(ss[i]) for i in range(len(kinds)))
    if imap == "ard":
        kernel = kernel.stretch(torch.exp(P["map"]))
    elif imap == "periodic":
        kernel = kernel.periodic(torch.exp(P["map"]))
    c = P["c"]
    f = st.GP((lambda t: c * torch.ones((t.shape[0], 1), dtype=t.dtype, device=t.device)), kernel) if mean_fn else st.GP(kernel)
    obs = OBS[method](f(P["z"]), f(P["x"], torch.exp(P["lnoise"])), P["y"])
    return f, obs, f | obs


def evaluate(post, xs, call, pred_noise):
    fdd = post(xs, 0.05) if pred_noise else post(xs)
    if call == "bounds":
        m, lo, hi = fdd.marginal_credible_bounds()
        return m, ((hi - lo) / (2 * 1.96)) ** 2
    if call == "mean":
        return fdd.mean[:, 0], None
    if call == "var":
        return None, fdd.var_diag
    return fdd.marginals()


def reference(p, names, kinds, method, imap, mean_fn, pred_noise, eps):
    Q = leaves(p, names)
    alphas = torch.exp(Q["la"]) if "la" in Q else [None] * len(kinds)
    mean_c = Q["c"] if mean_fn else torch.zeros((), dtype=torch.float64)
    rm, rv = R.sparse_posterior_t(method, kinds, torch.exp(Q["lv"]), torch.exp(Q["ls"]), alphas, Q["x"], Q["z"], Q["xs"], Q["y"],
                                  torch.exp(Q["lnoise"]), mean_c, eps, R.input_map(imap, torch.exp(Q["map"]) if imap else None))
    return Q, rm, (rv + 0.05 if pred_noise else rv)


def check_values(name, got, ref, vtol=1e-9):
    err = float((got.detach().double().cpu() - ref.detach()).abs().max() / ref.detach().abs().max())
    print(f"value {name}: err {err:.3e}")
    assert err <= vtol, (name, err)


def check_grads(P, Q, names, tol):
    for k in names:
        got, ref = P[k].grad, Q[k].grad
        if ref is None or not bool(ref.abs().max() > 0):
            continue                       # (e.g. the mean's constant under a variance-only loss)
        assert got is not None, f"no gradient reached {k}"
        err = float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1.0))
        print(f"grad {k}: err {err:.3e} (max |ref| {float(ref.abs().max()):.3e})")
        assert err <= tol, (k, err, got, ref)


def run_case(kinds, loss, method, *, imap=None, per_point=False, pred_noise=False, mean_fn=True, call="auto", d=2, seed=0, tol=TOL,
             n=N, m=M, ns=NS, dev="cpu", dtype=torch.float64, fixed=(), vtol=1e-9, span=2.0):
    p, wts_np = make_case(kinds, d=d, n=n, m=m, ns=ns, imap=imap, per_point=per_point, seed=seed, rq_alpha="rq" in kinds, span=span)
    names = [k for k in p if k not in fixed and (mean_fn or k != "c")]
    P = leaves(p, names, dtype, dev)
    _, _, post = build(P, kinds, method, imap, mean_fn)
    mean, var = evaluate(post, P["xs"], call, pred_noise)
    with torch.no_grad():                          # an identically built model without gradients: the same values
        plain = evaluate(build(leaves(p, (), dtype, dev), kinds, method, imap, mean_fn)[2], torch.tensor(p["xs"], dtype=dtype, device=dev),
                         call, pred_noise)
    Q, rm, rv = reference(p, names, kinds, method, imap, mean_fn, pred_noise, st.B.epsilon)
    for name, a, b, ref in (("mean", mean, plain[0], rm), ("var", var, plain[1], rv)):
        if a is not None:
            assert a.requires_grad and not b.requires_grad
            check_values(name + " against no_grad", a, b.double().cpu(), 1e-9 if dtype == torch.float64 else 1e-4)
            check_values(name, a, ref, vtol)
    wts = torch.tensor(wts_np, dtype=dtype, device=dev)
    R.loss_of(loss, mean, var, wts).backward()
    R.loss_of(loss, rm, rv, wts.double().cpu()).backward()
    check_grads(P, Q, names, tol)
    return P


@pytest.mark.parametrize("method", ["vfe", "fitc", "dtc"])
@pytest.mark.parametrize("loss", ["mean", "var", "ucb"])
def test_methods_and_losses(be, method, loss):
    run_case(("eq",), loss, method, seed=1)


@pytest.mark.parametrize("method", ["vfe", "fitc"])
@pytest.mark.parametrize("kinds", [("eq", "linear"), ("matern52", "matern12"), ("rq",)])
def test_kernels(be, kinds, method):
    run_case(kinds, "ucb", method, seed=2)


@pytest.mark.parametrize("method", ["vfe", "fitc"])
@pytest.mark.parametrize("imap,d", [("ard", 3), ("periodic", 1)])
def test_input_maps(be, imap, d, method):
    run_case(("eq",), "ucb", method, imap=imap, d=d, seed=3)


@pytest.mark.parametrize("method", ["vfe", "fitc"])
def test_per_point_noise_and_zero_mean(be, method):
    run_case(("eq", "linear"), "ucb", method, per_point=True, mean_fn=False, seed=4)


@pytest.mark.parametrize("call", ["mean", "var", "bounds", "auto"])
def test_every_entry_point_with_predictive_noise(be, call):
    loss = {"mean": "mean", "var": "var", "bounds": "ucb", "auto": "ucb"}[call]
    run_case(("matern52",), loss, "vfe", call=call, pred_noise=True, seed=5)


def test_mean_only_loss_takes_no_many_column_solve_and_no_gemm(be):
    """``gs = 0``: the cotangent behind Sigma has rank two -- single-column solves and rank-one passes, nothing of order M^2 N."""
    p, wts = make_case(("eq",), seed=6)
    P = leaves(p, list(p))
    _, _, post = build(P, ("eq",), "vfe")
    mean, var = post(P["xs"]).marginals()
    del be.calls[:]
    (mean * torch.tensor(wts)).sum().backward()
    assert be.calls.count("gemm") == 0, be.calls
    assert P["z"].grad is not None and var.requires_grad


@pytest.mark.parametrize("method", ["vfe", "fitc"])
def test_test_inputs_as_the_only_leaf_touch_nothing_of_the_data_size(be, method):
    """An acquisition ascent over ``xs`` on a fitted surrogate: the right gradient, and no kernel matrix against the data in the backward."""
    p, wts = make_case(("eq", "linear"), seed=10)
    run_case(("eq", "linear"), "ucb", method, seed=10, fixed=[k for k in p if k != "xs"])
    P = leaves(p, ["xs"])
    mean, var = build(P, ("eq", "linear"), method)[2](P["xs"]).marginals()
    del be.calls[:]
    R.loss_of("ucb", mean, var, torch.tensor(wts)).backward()
    assert be.calls.count("kmat") == 0 and be.calls.count("gemm") == 0 and be.calls.count("kmat_vjp_dense") == 1, be.calls


def test_marginals_run_one_forward_for_mean_and_variance(be):
    p, _ = make_case(("eq",), seed=6)
    P = leaves(p, list(p))
    _, _, post = build(P, ("eq",), "vfe")
    fdd = post(P["xs"])
    del be.calls[:]
    mean, var = fdd.marginals()
    assert mean.grad_fn is not None and var.grad_fn is not None
    assert be.calls.count("kmat") == 1, be.calls           # k(z, xs) once: one forward serves the mean and the variance
    del be.calls[:]
    (mean.sum() + var.sum()).backward()
    assert be.calls.count("kmat") == 1, be.calls           # ... and one backward: k(z, x) evaluated again, once


def test_dtc_gives_the_gradients_of_vfe(be):
    a = run_case(("eq", "linear"), "ucb", "vfe", seed=7)
    b = run_case(("eq", "linear"), "ucb", "dtc", seed=7)
    for k in a:
        assert torch.equal(a[k].grad, b[k].grad), k


def test_nothing_learnable_keeps_the_plain_path(be):
    p, _ = make_case(("eq",), seed=8)
    for mean_fn in (True, False):
        P = leaves(p, ())
        _, _, post = build(P, ("eq",), "vfe", mean_fn=mean_fn)
        mean, var = post(P["xs"]).marginals()
        assert mean.grad_fn is None and var.grad_fn is None and not mean.requires_grad and not var.requires_grad
    P = leaves(p, list(p))
    with torch.no_grad():
        _, _, post = build(P, ("eq",), "fitc")
        mean, var = post(P["xs"]).marginals()
        assert not post(P["xs"]).mean.requires_grad
    assert not mean.requires_grad and not var.requires_grad


@pytest.mark.parametrize("order", ["elbo_first", "mean_first"])
def test_bound_and_prediction_in_either_order_carry_gradients(be, order):
    p, _ = make_case(("eq",), seed=9)
    P = leaves(p, list(p))
    f, obs, post = build(P, ("eq",), "vfe")
    if order == "elbo_first":
        elbo = obs.elbo(f.measure)
        mean = post(P["xs"]).mean
    else:
        mean = post(P["xs"]).mean
        elbo = obs.elbo(f.measure)
    assert elbo.requires_grad and mean.requires_grad
    (elbo + mean.sum()).backward()
    for k in ("lv", "ls", "lnoise", "z", "y"):
        assert P[k].grad is not None and bool(torch.isfinite(P[k].grad).all()), k


def test_inputs_above_eight_dimensions_refuse_input_gradients(be):
    rng = np.random.default_rng(2)
    x, z = torch.tensor(rng.standard_normal((30, 9))), torch.tensor(rng.standard_normal((5, 9)))
    xs = torch.tensor(rng.standard_normal((5, 9)), requires_grad=True)
    y = torch.tensor(rng.standard_normal((30, 1)))
    f = st.GP(st.EQ())
    post = f | st.PseudoObs(f(z), f(x, 0.1), y)
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        post(xs).mean


def test_log_density_under_a_pseudo_point_posterior_still_refuses(be):
    rng = np.random.default_rng(3)
    x, y = torch.tensor(rng.standard_normal((30, 2))), torch.tensor(rng.standard_normal((30, 1)))
    v = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    f = st.GP(v * st.EQ())
    sparse_post = f | st.PseudoObs(f(x[:4]), f(x[:9], 0.1), y[:9])
    with pytest.raises(NotImplementedError):
        sparse_post(x[9:14], 0.1).logpdf(y[9:14])


#: the shapes of ``tests/test_sparse_posterior_grad_gpu.py``: the smallest at which the 64 x 64 tiles of ``gpk_kmat_vjp_dense`` and the
#: blocked solves can go wrong.  ``span``: the inputs fill ``[-span, span]^d``, wide enough for the inducing inputs to sit about a length
#: scale and a half apart (condition number of ``K_z``: 160, 240 and 100).
GPU_CASES = {
    "partial_tiles": dict(n=200, m=70, ns=45, d=3, imap="ard", span=3.0, seed=11),         # partial row and column tiles, M no multiple of 128
    "m_multiple_of_128": dict(n=300, m=128, ns=64, d=2, span=9.0, seed=12),
    "fp32": dict(n=1000, m=128, ns=64, d=2, span=9.0, seed=13),
}


def _reference_moves(kinds, method, tol, **shape):
    """How far the reference's own gradients move when the jitter goes from 1e-12 to 1e-10, in the tolerance's norm."""
    grads = []
    for eps in (1e-12, 1e-10):
        p, wts = make_case(kinds, **shape)
        Q, rm, rv = reference(p, list(p), kinds, method, shape.get("imap"), True, False, eps)
        R.loss_of("ucb", rm, rv, torch.tensor(wts)).backward()
        grads.append({k: Q[k].grad for k in p})
    return max(float((grads[0][k] - grads[1][k]).abs().max() / grads[1][k].abs().max().clamp_min(1.0)) for k in grads[0])


@pytest.mark.parametrize("method", ["vfe", "fitc"])
def test_reference_is_stable_under_the_jitter(method):
    """The reference's own gradients at 1e-12 and at 1e-10 of jitter: within a tenth of the tolerance, here and at the GPU cases."""
    assert _reference_moves(("matern52", "matern12"), method, TOL, seed=2) <= TOL / 10
    for name, shape in GPU_CASES.items():
        assert _reference_moves(("eq",), method, 1e-6, **shape) <= (1e-3 if name == "fp32" else 1e-6) / 10, name
