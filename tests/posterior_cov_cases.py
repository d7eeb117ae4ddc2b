"""Cases shared by ``test_posterior_cov_grad_host.py`` and ``test_posterior_cov_grad_gpu.py``: losses built from the JOINT posterior
covariance of an exact posterior ``f | (f(x, noise), y)`` -- ``post(xs).var`` as a dense matrix, reparameterised samples with fixed
draws, the entropy -- against torch autograd through a dense fp64 formula of the same posterior (``torch.linalg.cholesky``)."""
import math

import numpy as np
import torch

import stheno_amd as st
from stheno_amd.matrix import config

from .test_posterior_grad_host import KINDS, _kmat_t

TWO_GROUP = "two_group"          # v1 * EQ().stretch([l1, l2]) + v2 * EQ().periodic(p)
PRED_NOISE = 0.05
NUM = 4


def _period_map(x, p):
    a = (2.0 * math.pi) * x / p
    return torch.cat([torch.sin(a), torch.cos(a)], dim=-1)


def _kernel_t(kinds, Q, a, b):
    """The kernel matrix in torch (fp64), for the reference."""
    vs = torch.exp(Q["lv"])
    if kinds == TWO_GROUP:
        l12, p = torch.exp(Q["l12"]), torch.exp(Q["lp"])
        one = torch.ones((), dtype=a.dtype, device=a.device)
        return (_kmat_t(("eq",), vs[:1], [one], a / l12, b / l12) + _kmat_t(("eq",), vs[1:], [one], _period_map(a, p), _period_map(b, p)))
    return _kmat_t(kinds, vs, torch.exp(Q["ls"]), a, b)


def reference(kinds, Q, pred_noise):
    """``(mean (N*,), covariance (N*, N*))`` of the posterior at ``xs`` (plus the predictive noise), dense, inside the graph of ``Q``."""
    x, xs, y = Q["x"], Q["xs"], Q["y"]
    n, ns = x.shape[0], xs.shape[0]
    eye = lambda m: torch.eye(m, dtype=x.dtype, device=x.device)      # noqa: E731
    K = _kernel_t(kinds, Q, x, x) + torch.diag(torch.exp(Q["lnoise"]).expand(n)) + config.epsilon * eye(n)
    L = torch.linalg.cholesky(K)
    kxs = _kernel_t(kinds, Q, x, xs)
    sol = torch.cholesky_solve(torch.cat([y - Q["c"], kxs], dim=1), L)
    mean = Q["c"] + kxs.T @ sol[:, :1]
    cov = _kernel_t(kinds, Q, xs, xs) - kxs.T @ sol[:, 1:]
    if pred_noise:
        cov = cov + torch.exp(Q["lpn"]) * eye(ns)
    return mean[:, 0], cov


def loss_of(kind, mean, cov, fixed):
    """The three losses on a dense ``(mean, cov)`` (the reference side)."""
    ns = cov.shape[0]
    if kind == "var":
        return (fixed["G0"] * cov).sum()
    jit = config.epsilon * torch.eye(ns, dtype=cov.dtype, device=cov.device)
    if kind == "sample":
        s = mean[:, None] + torch.linalg.cholesky(cov + jit) @ fixed["xi"]
        return (fixed["W"] * s).sum() + 0.5 * (s * s).sum()
    return (torch.logdet(cov + jit) + ns * (math.log(2 * math.pi) + 1)) / 2


def make(kinds, *, n=30, ns=7, d=3, per_point=False, seed=0):
    rng = np.random.default_rng(seed)
    nk = 2 if kinds == TWO_GROUP else len(kinds)
    if kinds == TWO_GROUP:
        d = 2
    p = dict(x=rng.standard_normal((n, d)), xs=rng.standard_normal((ns, d)), y=rng.standard_normal((n, 1)),
             lv=np.log(rng.uniform(0.5, 1.5, nk)), ls=np.log(rng.uniform(0.8, 1.6, nk)), c=np.array(0.3),
             lnoise=np.log(rng.uniform(0.1, 0.3, n)) if per_point else np.array(np.log(0.2)), lpn=np.array(np.log(PRED_NOISE)),
             l12=np.log(rng.uniform(0.8, 1.5, 2)), lp=np.array(np.log(2.5)))
    fixed = dict(G0=rng.standard_normal((ns, ns)), xi=rng.standard_normal((ns, NUM)), W=rng.standard_normal((ns, NUM)))
    return p, fixed


def names_of(kinds, pred_noise):
    names = ["x", "xs", "y", "lv", "lnoise", "c"] + (["l12", "lp"] if kinds == TWO_GROUP else ["ls"])
    return names + (["lpn"] if pred_noise else [])


def leaves(p, names, dtype, dev):
    return {k: torch.tensor(p[k], dtype=dtype, device=dev, requires_grad=k in names) for k in p}


def process(kinds, P):
    vs = torch.exp(P["lv"])
    if kinds == TWO_GROUP:
        kernel = vs[0] * st.EQ().stretch(torch.exp(P["l12"])) + vs[1] * st.EQ().periodic(torch.exp(P["lp"]))
    else:
        ss = torch.exp(P["ls"])
        kernel = sum(vs[i] * KINDS[k]().stretch(ss[i]) for i, k in enumerate(kinds))
    c = P["c"]
    return st.GP((lambda z: c * torch.ones((z.shape[0], 1), dtype=z.dtype, device=z.device)), kernel)


def ours(kinds, P, loss, fixed, pred_noise, *, prime=None):
    """``(loss value, the dense covariance the path returned)``.  ``prime(fdd_obs, y)``: something to run on the observations before the
    posterior is asked (a log-density that leaves its factor behind)."""
    f = process(kinds, P)
    obs = f(P["x"], torch.exp(P["lnoise"]))
    if prime is not None:
        prime(obs, P["y"])
    post = f | (obs, P["y"])
    fdd = post(P["xs"], torch.exp(P["lpn"])) if pred_noise else post(P["xs"])
    if loss == "var":
        cov = fdd.var.mat
        return (fixed["G0"] * cov).sum(), cov
    if loss == "sample":
        s = fdd.sample(xi=fixed["xi"])
        assert tuple(s.shape) == (P["xs"].shape[0], NUM)
        return (fixed["W"] * s).sum() + 0.5 * (s * s).sum(), None
    return fdd.entropy(), None


def run_case(kinds, loss, *, pred_noise=None, per_point=False, dev="cpu", dtype=torch.float64, n=30, ns=7, d=3, seed=0, tol=1e-6,
             clamp=False):
    """Gradients of ``loss`` with respect to every leaf against the dense reference: ``max |got - ref| / max |ref| <= tol`` per leaf
    (``clamp``: the denominator is at least 1, as ``test_posterior_grad_host.run_case`` has it for fp32).  The covariance under grad
    has the bits of the same call under ``torch.no_grad()``."""
    pred_noise = (loss != "var") if pred_noise is None else pred_noise
    p, fixed_np = make(kinds, n=n, ns=ns, d=d, per_point=per_point, seed=seed)
    names = names_of(kinds, pred_noise)
    P = leaves(p, names, dtype, dev)
    fixed = {k: torch.tensor(v, dtype=dtype, device=dev) for k, v in fixed_np.items()}
    val, cov = ours(kinds, P, loss, fixed, pred_noise)
    assert val.requires_grad, "the loss is cut off from the graph"
    if cov is not None:
        with torch.no_grad():
            _, plain = ours(kinds, leaves(p, (), dtype, dev), loss, fixed, pred_noise)
        assert torch.equal(cov.detach(), plain), "the covariance under grad differs from the call under no_grad"
    val.backward()

    Q = leaves(p, names, torch.float64, dev)
    fixed64 = {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in fixed_np.items()}
    rm, rc = reference(kinds, Q, pred_noise)
    ref_val = loss_of(loss, rm, rc, fixed64)
    vtol = 1e-9 if dtype == torch.float64 else 1e-3
    v_, r_ = float(val.detach()), float(ref_val.detach())
    assert abs(v_ - r_) <= vtol * max(abs(r_), 1.0), (v_, r_)
    ref_val.backward()
    errs = {}
    for k in names:
        got, ref = P[k].grad, Q[k].grad
        if ref is None or not bool(ref.abs().max() > 0):
            continue                       # (y and the mean's constant under a loss of the covariance alone)
        assert got is not None, f"no gradient reached {k}"
        den = ref.abs().max().clamp_min(1.0) if clamp else ref.abs().max()
        errs[k] = float((got.double() - ref).abs().max() / den)
    print(f"posterior covariance gradients {kinds} {loss} n={n} ns={ns} {dtype}: " + " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= tol, (k, e, P[k].grad, Q[k].grad)
    return {k: P[k].grad.clone() for k in names if P[k].grad is not None}
