"""Gradients through posteriors ACROSS processes (``autograd._BlockPosteriorMarginals``): the models both test modules run, a dense
torch fp64 reference of each, the comparison, and the NumPy backend of the host module.  Not collected by pytest.

The reference writes every kernel in torch (``diff_reference.torch_kernel``), takes the derivative blocks by autograd of that kernel
(``torch.func.grad`` per pair of points, ``vmap`` over the pairs), forms the posterior mean and the marginal variances with
``torch.linalg`` and takes its gradients by ``backward``.  ``torch_kernel`` differentiates through ``sqrt(q)``, which is not finite at
``q = 0``: in a block of a set of points with itself the pairs ``(x_i, x_i)`` -- and only those -- are evaluated with the second point
displaced by ``DISPLACE`` in every coordinate.  That moves a diagonal entry by O(DISPLACE^2) relative (the profiles are even in the
distance: 5e-11 here), and autograd's own cancellation in the Matern profile's slope, eps / s, stays at 1e-11; displacing whole
blocks, or a smaller displacement, puts errors of 1e-8 and more into K, which its condition number carries past the tolerance.

Models (D = 2 except for the decomposition, which is D = 1):

    decomposition   f = f1 + f2, f1 ~ v1 EQ().stretch(l), f2 ~ v2 EQ().periodic(p); f observed, f1 predicted
    two_observed    f ~ v1 EQ().stretch(l1), g ~ v2 Matern52().stretch(l2) independent; f at x1 and f + g at x2 observed, g predicted
    values_slopes   f ~ v EQ().stretch(l) + v2 Matern52() + v3 RQ(alpha); f at x1 and f.diff(1) at x2 observed, f predicted
    slope           the same f, observed at x1; f.diff(0) predicted (the cross block is one-sided)
    pred_noise      values_slopes with predictive noise: post(f)(xs, 0.05)

Every case's loss is a weighted UCB, ``sum w (mean + 2 sqrt(var))``, and ``xs`` requires a gradient.  Tolerances: the project's,
``1e-6 max(max |ref|, 1)`` in fp64 and ``1e-3`` in fp32."""
import math

import numpy as np
import torch
from torch.func import grad, vmap

import stheno_amd as st
from stheno_amd.matrix import config

from . import diff_reference as D
from .conftest import OracleBackend, _np

HOST_SIZES = dict(n1=40, n2=25, ns=17)
GPU_SIZES = dict(n1=70, n2=61, ns=65)          # across the 64-tile and 128-block edges
DISPLACE = 3e-6
PRED_NOISE = 0.05


# ---- the NumPy backend of the host module ---------------------------------------------------------------------------------------
def _profile_np(kind, q, alpha):
    """``(kappa, kappa', d kappa / d alpha)`` at ``q``."""
    zero = np.zeros_like(q)
    if kind == "eq":
        k = np.exp(-0.5 * q)
        return k, -0.5 * k, zero
    if kind == "matern32":
        s = np.sqrt(3 * q)
        return (1 + s) * np.exp(-s), -1.5 * np.exp(-s), zero
    if kind == "matern52":
        s = np.sqrt(5 * q)
        return (1 + s + s * s / 3) * np.exp(-s), -(5.0 / 6.0) * (1 + s) * np.exp(-s), zero
    if kind == "rq":
        u = q / (2 * alpha)
        k = np.exp(-alpha * np.log1p(u))
        return k, -0.5 * k / (1 + u), k * (u / (1 + u) - np.log1p(u))
    if kind == "linear":
        return q, np.ones_like(q), zero
    if kind == "const":
        return np.ones_like(q), zero, zero
    raise ValueError(kind)


class BlockOracle(OracleBackend):
    """``OracleBackend`` with the solve with the transposed factor, and with kernel matrices, diagonals and the explicit-cotangent
    reduction from direct differences for every kind the models use (the rational quadratic included); the derivative blocks and their
    VJP come from ``ops._HostDelta``, which wraps every backend that is not the HIP one."""

    def tri_solve_t_(self, l, dinv_sb, sb, b):
        b.copy_(self._t(np.linalg.solve(np.tril(_np(l)).T, _np(b)), b))
        return b

    @staticmethod
    def _q(kind, a, b, scale):
        return (a @ b.T if kind == "linear" else ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)) / scale ** 2

    def kmat(self, terms, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        a = _np(x)
        b = a if y is None else _np(y)
        k = np.zeros((a.shape[0], b.shape[0]))
        for (kind, v, s), al in zip(terms.terms, terms.shapes or [None] * len(terms)):
            k += v * _profile_np(kind, self._q(kind, a, b, s), al)[0]
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
        return self._t(sum(v * ((a * a).sum(-1) / s ** 2 if kind == "linear" else np.ones(a.shape[0])) for kind, v, s in terms.terms), x)

    def kmat_vjp_dense(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        assert colscale is None and w is None and b is None and not want_colsum
        a, c, G = _np(x), _np(y), _np(g)
        S = np.zeros((len(terms), 2 if terms.shapes is None else 3))
        gx = np.zeros_like(a)
        for t, ((kind, v, s), al) in enumerate(zip(terms.terms, terms.shapes or [None] * len(terms))):
            q = self._q(kind, a, c, s)
            k, dk, da = _profile_np(kind, q, al)
            S[t, 0], S[t, 1] = (G * k).sum(), (G * dk * q).sum()
            if kind == "rq":
                S[t, 2] = (G * da).sum()
            if kind == "linear":
                gx += (G * v / s ** 2) @ c
            elif kind != "const":
                coef = G * v * dk * 2 / s ** 2
                gx += coef.sum(1)[:, None] * a - coef @ c
        return self._t(S, x), None, (self._t(gx, x) if want_gradx else None)


# ---- the reference's kernels ---------------------------------------------------------------------------------------------------
def kernel_block(terms, shapes, x, y, a=None, b=None, coincident=False):
    """``D^(a, b) k(x, y)`` (n, m) in torch fp64, differentiable with respect to everything in ``terms`` / ``shapes`` and the inputs."""
    if a is None and b is None and not coincident:
        return D.torch_kernel(terms, shapes, x, y)
    k = lambda xi, yj: D.torch_kernel(terms, shapes, xi[None], yj[None])[0, 0]      # noqa: E731
    if a is None and b is None:
        fn = k
    elif a is not None:
        fn = lambda xi, yj: grad(k, 0)(xi, yj)[a]                                   # noqa: E731
        if b is not None:
            fn_a = fn
            fn = lambda xi, yj: grad(fn_a, 1)(xi, yj)[b]                            # noqa: E731
    else:
        fn = lambda xi, yj: grad(k, 1)(xi, yj)[b]                                   # noqa: E731
    if not coincident:
        return vmap(vmap(fn, (None, 0)), (0, None))(x, y)
    shift = DISPLACE * torch.eye(x.shape[0], dtype=x.dtype)[:, :, None]              # (n, n, 1): the pairs (x_i, x_i) alone
    return vmap(vmap(lambda xi, yj, e: fn(xi, yj + e), (None, 0, 0)), (0, None, 0))(x, y, shift)


def dense_posterior(K, C, r, kss, noise):
    """Mean minus the prior mean and marginal variance from the dense pieces: ``K`` (N, N) without noise, ``C`` (N, N*), ``r`` (N, 1),
    ``kss`` (N*,) the prior variances, ``noise`` (N,)."""
    n = K.shape[0]
    L = torch.linalg.cholesky(K + torch.diag(noise) + config.epsilon * torch.eye(n, dtype=K.dtype))
    sol = torch.cholesky_solve(torch.cat([r, C], dim=1), L)
    return (C.T @ sol[:, :1])[:, 0], kss - (C * sol[:, 1:]).sum(0)


def _data(case, sizes):
    rng = np.random.default_rng({"decomposition": 1, "two_observed": 2, "values_slopes": 3, "slope": 4, "pred_noise": 5}[case])
    n1, n2, ns = sizes["n1"], sizes["n2"], sizes["ns"]
    d = 1 if case == "decomposition" else 2
    x1, x2, xs = (rng.uniform(-1.5, 1.5, (k, d)) for k in (n1, n2, ns))
    fn = lambda z: np.sin(2.0 * z[:, :1]) * (np.cos(z[:, 1:2]) if d == 2 else 1.0)      # noqa: E731
    y1 = fn(x1) + 0.1 * rng.standard_normal((n1, 1))
    y2 = (-np.sin(2.0 * x2[:, :1]) * np.sin(x2[:, 1:2]) if d == 2 else fn(x2)) + 0.1 * rng.standard_normal((n2, 1))
    return dict(x1=x1, x2=x2, xs=xs, y1=y1, y2=y2, w=rng.uniform(0.5, 1.5, ns))


#: hyper-parameters per case, as logarithms (the leaves the gradients are asked for)
HYPER = {
    "decomposition": dict(lv1=math.log(1.2), ll=math.log(0.8), lv2=math.log(0.6), lp=math.log(1.7), ln1=math.log(0.15)),
    "two_observed": dict(lv1=math.log(1.1), ll1=math.log(0.9), lv2=math.log(0.7), ll2=math.log(1.3), ln1=math.log(0.12), ln2=math.log(0.2)),
    "values_slopes": dict(lv=math.log(1.3), ll=math.log(0.8), lv2=math.log(0.5), lv3=math.log(0.4), la=math.log(0.9), ln1=math.log(0.1),
                          ln2=math.log(0.15)),
}
HYPER["slope"] = {k: v for k, v in HYPER["values_slopes"].items() if k != "ln2"}
HYPER["pred_noise"] = HYPER["values_slopes"]
CASES = list(HYPER)
#: which data tensors a case uses, and which of them are leaves
USES = {"decomposition": ("x1", "y1", "xs"), "two_observed": ("x1", "x2", "y1", "y2", "xs"), "values_slopes": ("x1", "x2", "y1", "y2", "xs"),
        "slope": ("x1", "y1", "xs"), "pred_noise": ("x1", "x2", "y1", "y2", "xs")}
DATA_LEAVES = ("y1", "y2", "xs")


def leaves(case, sizes, dtype=torch.float64, dev="cpu"):
    """The tensors of a case: hyper-parameters as fp64 scalars on the host, the data in ``dtype`` on ``dev``; every hyper-parameter,
    every ``y`` and ``xs`` require a gradient."""
    data = _data(case, sizes)
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in HYPER[case].items()}
    for k in USES[case]:
        P[k] = torch.tensor(data[k], dtype=dtype, device=dev, requires_grad=k in DATA_LEAVES)
    P["w"] = torch.tensor(data["w"], dtype=dtype, device=dev)
    return P


def _three_terms(P):
    e = torch.exp
    return ([("eq", e(P["lv"]), e(P["ll"])), ("matern52", e(P["lv2"]), 1.0), ("rq", e(P["lv3"]), 1.0)], [None, None, e(P["la"])])


def ours(case, P):
    """``(mean (N*,), marginal variance (N*,))`` of the case through the package."""
    e = torch.exp
    with st.Measure() as prior:
        if case == "decomposition":
            f1 = st.GP(e(P["lv1"]) * st.EQ().stretch(e(P["ll"])))
            f2 = st.GP(e(P["lv2"]) * st.EQ().periodic(e(P["lp"])))
            f = f1 + f2
            obs, target = (f(P["x1"], e(P["ln1"])), P["y1"]), f1
        elif case == "two_observed":
            f = st.GP(e(P["lv1"]) * st.EQ().stretch(e(P["ll1"])))
            g = st.GP(e(P["lv2"]) * st.Matern52().stretch(e(P["ll2"])))
            h = f + g
            obs, target = ((f(P["x1"], e(P["ln1"])), P["y1"]), (h(P["x2"], e(P["ln2"])), P["y2"])), g
        else:
            f = st.GP(e(P["lv"]) * st.EQ().stretch(e(P["ll"])) + e(P["lv2"]) * st.Matern52() + e(P["lv3"]) * st.RQ(e(P["la"])))
            if case == "slope":
                target = f.diff(0)
                obs = (f(P["x1"], e(P["ln1"])), P["y1"])
            else:
                df = f.diff(1)
                obs, target = ((f(P["x1"], e(P["ln1"])), P["y1"]), (df(P["x2"], e(P["ln2"])), P["y2"])), f
    post = prior | obs
    fdd = post(target)(P["xs"], PRED_NOISE) if case == "pred_noise" else post(target)(P["xs"])
    mean, var = fdd.marginals()
    return mean.reshape(-1), var.reshape(-1)


def reference(case, Q):
    """The same in dense torch fp64 (``Q``: fp64 leaves on the host)."""
    e = torch.exp
    x1, xs = Q["x1"], Q["xs"]
    n1 = x1.shape[0]
    if case == "decomposition":
        t1 = ([("eq", e(Q["lv1"]), e(Q["ll"]))], None)
        t2 = ([("eq", e(Q["lv2"]), 1.0)], None)
        emb = lambda z: torch.cat([torch.sin(2 * math.pi * z / e(Q["lp"])), torch.cos(2 * math.pi * z / e(Q["lp"]))], dim=-1)      # noqa: E731
        K = kernel_block(*t1, x1, x1, coincident=True) + kernel_block(*t2, emb(x1), emb(x1), coincident=True)
        C = kernel_block(*t1, x1, xs)
        mean, var = dense_posterior(K, C, Q["y1"], e(Q["lv1"]).expand(xs.shape[0]), e(Q["ln1"]).expand(n1))
    elif case == "two_observed":
        x2 = Q["x2"]
        tf = ([("eq", e(Q["lv1"]), e(Q["ll1"]))], None)
        tg = ([("matern52", e(Q["lv2"]), e(Q["ll2"]))], None)
        K21 = kernel_block(*tf, x2, x1)
        K = torch.cat([torch.cat([kernel_block(*tf, x1, x1, coincident=True), K21.T], dim=1),
                       torch.cat([K21, kernel_block(*tf, x2, x2, coincident=True) + kernel_block(*tg, x2, x2, coincident=True)], dim=1)])
        C = torch.cat([torch.zeros((n1, xs.shape[0]), dtype=torch.float64), kernel_block(*tg, x2, xs)])
        noise = torch.cat([e(Q["ln1"]).expand(n1), e(Q["ln2"]).expand(x2.shape[0])])
        mean, var = dense_posterior(K, C, torch.cat([Q["y1"], Q["y2"]]), e(Q["lv2"]).expand(xs.shape[0]), noise)
    elif case == "slope":
        t = _three_terms(Q)
        K = kernel_block(*t, x1, x1, coincident=True)
        C = kernel_block(*t, x1, xs, None, 0)                          # cov(f(x1), d0 f(xs))
        kss = sum(v / (s * s) * {"eq": 1.0, "matern52": 5.0 / 3.0, "rq": 1.0}[kind] for kind, v, s in t[0])
        mean, var = dense_posterior(K, C, Q["y1"], kss.expand(xs.shape[0]), e(Q["ln1"]).expand(n1))
    else:
        x2 = Q["x2"]
        t = _three_terms(Q)
        K21 = kernel_block(*t, x2, x1, 1, None)                        # cov(d1 f(x2), f(x1))
        K = torch.cat([torch.cat([kernel_block(*t, x1, x1, coincident=True), K21.T], dim=1),
                       torch.cat([K21, kernel_block(*t, x2, x2, 1, 1, coincident=True)], dim=1)])
        C = torch.cat([kernel_block(*t, x1, xs), kernel_block(*t, x2, xs, 1, None)])
        noise = torch.cat([e(Q["ln1"]).expand(n1), e(Q["ln2"]).expand(x2.shape[0])])
        kss = sum(v for _, v, _ in t[0])
        mean, var = dense_posterior(K, C, torch.cat([Q["y1"], Q["y2"]]), kss.expand(xs.shape[0]), noise)
        if case == "pred_noise":
            var = var + PRED_NOISE
    return mean, var


def loss(mean, var, w):
    return ((mean + 2.0 * torch.sqrt(var)) * w).sum()


def check_case(case, sizes, dtype=torch.float64, dev="cpu"):
    """Values and every gradient of a case against the reference; under ``torch.no_grad()`` the values are the same bits."""
    tol = 1e-6 if dtype == torch.float64 else 1e-3
    P = leaves(case, sizes, dtype, dev)
    mean, var = ours(case, P)
    with torch.no_grad():
        plain = ours(case, leaves(case, sizes, dtype, dev))
    for got, same in zip((mean, var), plain):
        assert torch.equal(got.detach(), same), "the values differ from the plain path's"
    loss(mean, var, P["w"]).backward()
    Q = leaves(case, sizes)
    rm, rv = reference(case, Q)
    loss(rm, rv, Q["w"]).backward()

    def err(got, ref):
        return float((got.detach().double().cpu() - ref.detach()).abs().max() / ref.detach().abs().max().clamp_min(1.0))

    report = {"mean": err(mean, rm), "var": err(var, rv)}
    assert report["mean"] <= tol and report["var"] <= tol, report
    for k in list(HYPER[case]) + [d for d in DATA_LEAVES if d in USES[case]]:
        assert Q[k].grad is not None and bool(Q[k].grad.abs().max() > 0), k
        assert P[k].grad is not None, f"no gradient reached {k}"
        report[k] = err(P[k].grad, Q[k].grad)
    print(case, str(dtype), " ".join(f"{k} {v:.1e}" for k, v in report.items()))
    bad = {k: v for k, v in report.items() if not v <= tol}
    assert not bad, bad
