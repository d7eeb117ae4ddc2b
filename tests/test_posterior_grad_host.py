"""Gradients through the posterior mean and marginal variances of an exact posterior ``f | (f(x, noise), y)`` (``.mean``,
``.var_diag``, ``.marginals()``, ``.marginal_credible_bounds()``; ``autograd._PosteriorMarginals``) -- the host logic on the test-only
oracle backend, extended here by the transposed solve in NumPy (and distances by direct differences, so that the Matern kernels are
exact on the diagonal).  Checked against torch autograd through a pure-torch dense formula (``torch.linalg.cholesky``) and against
central finite differences."""
import numpy as np
import pytest
import torch

import stheno_amd as st
from stheno_amd import ops
from stheno_amd.matrix import config

from .conftest import OracleBackend, _np

KINDS = {"eq": st.EQ, "matern12": st.Matern12, "matern52": st.Matern52, "linear": st.Linear}


def _kappa_np(kind, a, b):
    if kind == "linear":
        return a @ b.T
    q = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    if kind == "eq":
        return np.exp(-0.5 * q)
    r = np.sqrt(q)
    if kind == "matern12":
        return np.exp(-r)
    s = np.sqrt(5.0) * r
    return (1 + s + s * s / 3) * np.exp(-s)


class TransposedSolveOracle(OracleBackend):
    """``OracleBackend`` plus ``tri_solve_t_`` (``L^{-T} b``) in NumPy; kernel matrices and the symmetric reduction from direct
    differences."""

    def tri_solve_t_(self, l, dinv_sb, sb, b):
        L = np.tril(_np(l))
        b.copy_(self._t(np.linalg.solve(L.T, _np(b)), b))
        return b

    def kmat(self, terms, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        a = _np(x)
        bb = a if y is None else _np(y)
        k = np.zeros((a.shape[0], bb.shape[0]))
        for kind, v, s in terms.terms:
            k += v * _kappa_np(kind, a / s, bb / s)
        if y is None:
            k[np.diag_indices(a.shape[0])] += diag_add
            if diag_vec is not None:
                k[np.diag_indices(a.shape[0])] += _np(diag_vec)
        res = self._t(k, x)
        if out is not None:
            out.copy_(out + res if accumulate else res)
            return out
        return res

    def kmat_vjp(self, terms, x, kinv, alpha, g):
        ki = np.tril(_np(kinv)) + np.tril(_np(kinv), -1).T
        A, gv = _np(alpha), np.asarray(g, dtype=np.float64)
        G = 0.5 * ((A * gv) @ A.T - gv.sum() * ki)
        S, _, _ = self.kmat_vjp_dense(terms, x, x, self._t(G, x))
        return S, self._t(np.trace(G), x), self._t(np.diag(G).copy(), x)


@pytest.fixture()
def tsolve_backend():
    prev = ops.set_backend(TransposedSolveOracle())
    yield
    ops.set_backend(prev)


# ---- the pure-torch dense formula -------------------------------------------------------------------------------------------
def _kmat_t(kinds, vs, ss, a, b):
    out = 0
    for kind, v, s in zip(kinds, vs, ss):
        if kind == "linear":
            k = (a @ b.T) / (s * s)
        else:
            q = (((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / (s * s)).clamp_min(1e-300)
            if kind == "eq":
                k = torch.exp(-0.5 * q)
            elif kind == "matern12":
                k = torch.exp(-torch.sqrt(q))
            else:
                r = torch.sqrt(5.0 * q)
                k = (1 + r + r * r / 3) * torch.exp(-r)
        out = out + v * k
    return out


def _posterior_t(kinds, vs, ss, x, y, xs, noise, mean_c, ard):
    if ard is not None:
        x, xs = x / ard, xs / ard
    n = x.shape[0]
    K = _kmat_t(kinds, vs, ss, x, x) + torch.diag(noise.expand(n)) + config.epsilon * torch.eye(n, dtype=x.dtype, device=x.device)
    L = torch.linalg.cholesky(K)
    kxs = _kmat_t(kinds, vs, ss, x, xs)
    sol = torch.cholesky_solve(torch.cat([y - mean_c, kxs], dim=1), L)
    mean = mean_c + kxs.T @ sol[:, :1]
    kd = sum(v * ((xs * xs).sum(-1) / (s * s) if kind == "linear" else torch.ones(xs.shape[0], dtype=xs.dtype, device=xs.device))
             for kind, v, s in zip(kinds, vs, ss))
    return mean[:, 0], kd - (kxs * sol[:, 1:]).sum(0)


def _loss(kind, mean, var, wts):
    if kind == "mean":
        return (mean * wts).sum()
    if kind == "var":
        return (var * wts).sum()
    return ((mean + 2.0 * torch.sqrt(var)) * wts).sum()          # UCB


def run_case(kinds, loss, *, ard=False, per_point=False, pred_noise=False, mean_fn=True, call="auto", dev="cpu",
             dtype=torch.float64, n=30, ns=7, d=3, seed=0, tol=1e-8, fd=False):
    rng = np.random.default_rng(seed)
    p = dict(x=rng.standard_normal((n, d)), xs=rng.standard_normal((ns, d)), y=rng.standard_normal((n, 1)),
             lv=np.log(rng.uniform(0.5, 1.5, len(kinds))), ls=np.log(rng.uniform(0.8, 1.6, len(kinds))),
             ard=np.log(rng.uniform(0.8, 1.5, d)), c=np.array(0.3),
             lnoise=np.log(rng.uniform(0.1, 0.3, n)) if per_point else np.array(np.log(0.2)))
    wts_np = rng.uniform(0.5, 1.5, ns)
    names = ["x", "xs", "y", "lv", "ls", "lnoise"] + (["ard"] if ard else []) + (["c"] if mean_fn else [])

    def leaves(values, dt=dtype):
        return {k: torch.tensor(values[k], dtype=dt, device=dev, requires_grad=k in names) for k in values}

    def ours(P, grad=True):
        vs, ss = torch.exp(P["lv"]), torch.exp(P["ls"])
        kernel = sum(vs[i] * KINDS[k]().stretch(ss[i]) for i, k in enumerate(kinds))
        if ard:
            kernel = kernel.stretch(torch.exp(P["ard"]))
        c = P["c"]
        f = st.GP((lambda z: c * torch.ones((z.shape[0], 1), dtype=z.dtype, device=z.device)), kernel) if mean_fn else st.GP(kernel)
        post = f | (f(P["x"], torch.exp(P["lnoise"])), P["y"])
        fdd = post(P["xs"], 0.05) if pred_noise else post(P["xs"])
        with torch.set_grad_enabled(grad):
            if call == "bounds":
                m, lo, hi = fdd.marginal_credible_bounds()
                return m, ((hi - lo) / (2 * 1.96)) ** 2
            if call == "mean":
                return fdd.mean[:, 0], None
            if call == "var":
                return None, fdd.var_diag
            return fdd.marginals()

    P = leaves(p)
    wts = torch.tensor(wts_np, dtype=dtype, device=dev)
    mean, var = ours(P)
    with torch.no_grad():
        plain = ours(leaves(p), grad=False)
    for a, b in zip((mean, var), plain):          # the values are the plain path's, bit for bit
        if a is not None:
            assert torch.equal(a.detach(), b), (a, b)
    _loss(loss, mean, var, wts).backward()

    Q = leaves(p, torch.float64)                 # (the reference in fp64 whatever the path's precision)
    mean_c = Q["c"] if mean_fn else torch.zeros((), dtype=torch.float64, device=dev)
    vtol = 1e-9 if dtype == torch.float64 else 1e-3
    rm, rv = _posterior_t(kinds, torch.exp(Q["lv"]), torch.exp(Q["ls"]), Q["x"], Q["y"], Q["xs"], torch.exp(Q["lnoise"]), mean_c,
                          torch.exp(Q["ard"]) if ard else None)
    if pred_noise:
        rv = rv + 0.05
    if mean is not None:
        assert torch.allclose(mean.detach().double(), rm.detach(), rtol=vtol, atol=vtol)
    if var is not None:
        assert torch.allclose(var.detach().double(), rv.detach(), rtol=vtol, atol=vtol)
    _loss(loss, rm, rv, wts.double()).backward()
    for k in names:
        got, ref = P[k].grad, Q[k].grad
        if ref is None or not bool(ref.abs().max() > 0):
            continue                       # (e.g. the mean's constant under a variance-only loss)
        assert got is not None, f"no gradient reached {k}"
        err = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1.0))
        assert err <= tol, (k, err, got, ref)
    if fd:                                 # central finite differences of the values the path computes
        for k in ("lv", "ls", "lnoise"):
            base = p[k]
            flat = np.atleast_1d(base).astype(np.float64)
            for i in range(min(flat.size, 2)):
                vals = []
                for h in (1e-6, -1e-6):
                    q = dict(p)
                    pert = flat.copy()
                    pert[i] += h
                    q[k] = pert.reshape(np.shape(base))
                    with torch.no_grad():
                        m2, v2 = ours(leaves(q), grad=False)
                    vals.append(float(_loss(loss, m2, v2, wts)))
                fdv = (vals[0] - vals[1]) / 2e-6
                g = float(P[k].grad.reshape(-1)[i])
                assert abs(g - fdv) <= 1e-5 * max(abs(fdv), 1.0), (k, i, g, fdv)


KERNELS = [("eq",), ("eq", "linear"), ("matern52", "matern12")]


@pytest.mark.parametrize("kinds", KERNELS)
@pytest.mark.parametrize("loss", ["mean", "var", "ucb"])
def test_posterior_marginal_gradients_host_logic(tsolve_backend, kinds, loss):
    run_case(kinds, loss, fd=True)


@pytest.mark.parametrize("loss", ["mean", "ucb"])
def test_per_dimension_scales_per_point_noise_host_logic(tsolve_backend, loss):
    run_case(("eq", "linear"), loss, ard=True, per_point=True, seed=3)


@pytest.mark.parametrize("call", ["mean", "var", "bounds"])
def test_every_entry_point_and_predictive_noise_host_logic(tsolve_backend, call):
    loss = {"mean": "mean", "var": "var", "bounds": "ucb"}[call]
    run_case(("matern52",), loss, call=call, pred_noise=True, seed=5)


def test_zero_mean_host_logic(tsolve_backend):
    run_case(("eq",), "ucb", mean_fn=False, seed=7)


def test_nothing_learnable_keeps_the_plain_path(tsolve_backend):
    """Without a learnable quantity the posterior marginals come from the plain path: no autograd node."""
    rng = np.random.default_rng(1)
    x, y, xs = (torch.tensor(a) for a in (rng.standard_normal((20, 2)), rng.standard_normal((20, 1)), rng.standard_normal((5, 2))))
    f = st.GP(st.EQ())
    mean, var = (f | (f(x, 0.1), y))(xs).marginals()
    assert mean.grad_fn is None and var.grad_fn is None


def test_inputs_above_eight_dimensions_refuse_input_gradients(tsolve_backend):
    rng = np.random.default_rng(2)
    x = torch.tensor(rng.standard_normal((20, 9)))
    xs = torch.tensor(rng.standard_normal((5, 9)), requires_grad=True)
    y = torch.tensor(rng.standard_normal((20, 1)))
    f = st.GP(st.EQ())
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        (f | (f(x, 0.1), y))(xs).mean
