"""Models, references and the checker of the gradients through BATCHED posterior means and marginal variances
(``autograd._BatchedPosteriorMarginals``), shared by ``tests/test_batch_posterior_grad_host.py`` (the NumPy test backend) and
``tests/test_batch_posterior_grad_gpu.py`` (``libgpk``).  Not collected by pytest.

The reference is torch autograd through a pure-torch dense fp64 formula, entry by entry: ``test_posterior_grad_host._posterior_t`` for
the sums of EQ / Matern / Linear terms it knows, and the same formula on an explicit kernel function for what it does not (RQ, sums
behind different input maps, a periodic map)."""
import math

import numpy as np
import torch

import stheno_amd as st
from stheno_amd.matrix import config

from .test_posterior_grad_host import KINDS, _loss, _posterior_t


def _q(a, b, s):
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / (s * s)


def _dense_posterior(kfun, kdiag, x, y, xs, noise, mean_c):
    """``_posterior_t`` on a kernel given as functions: ``kfun(a, b)`` the matrix, ``kdiag(a)`` its diagonal."""
    n = x.shape[0]
    K = kfun(x, x) + torch.diag(noise.expand(n)) + config.epsilon * torch.eye(n, dtype=x.dtype, device=x.device)
    L = torch.linalg.cholesky(K)
    kxs = kfun(x, xs)
    sol = torch.cholesky_solve(torch.cat([y - mean_c, kxs], dim=1), L)
    return (mean_c + kxs.T @ sol[:, :1])[:, 0], kdiag(xs) - (kxs * sol[:, 1:]).sum(0)


def _ones(a):
    return torch.ones(a.shape[0], dtype=a.dtype, device=a.device)


#: model -> (the kernel from the leaves, the reference posterior of one entry from the leaves); ``kinds`` models are built in ``run_case``
def _rq_kernel(P):
    return torch.exp(P["lv"][0]) * st.RQ(torch.exp(P["la"])).stretch(torch.exp(P["ls"][0])) + torch.exp(P["lv"][1]) * st.EQ().stretch(torch.exp(P["ls"][1]))


def _rq_ref(Q, x, y, xs, noise, c):
    v, s, al = torch.exp(Q["lv"]), torch.exp(Q["ls"]), torch.exp(Q["la"])
    kfun = lambda a, b: v[0] * (1 + _q(a, b, s[0]) / (2 * al)) ** (-al) + v[1] * torch.exp(-0.5 * _q(a, b, s[1]))      # noqa: E731
    return _dense_posterior(kfun, lambda a: (v[0] + v[1]) * _ones(a), x, y, xs, noise, c)


def _two_kernel(P):
    return torch.exp(P["lv"][0]) * st.EQ().stretch(torch.exp(P["ard"])) + torch.exp(P["lv"][1]) * st.Matern52().stretch(torch.exp(P["ls"][1]))


def _m52(q):
    r = torch.sqrt(5.0 * q.clamp_min(1e-300))
    return (1 + r + r * r / 3) * torch.exp(-r)


def _two_ref(Q, x, y, xs, noise, c):
    v, s, ard = torch.exp(Q["lv"]), torch.exp(Q["ls"]), torch.exp(Q["ard"])
    kfun = lambda a, b: v[0] * torch.exp(-0.5 * _q(a / ard, b / ard, 1.0)) + v[1] * _m52(_q(a, b, s[1]))      # noqa: E731
    return _dense_posterior(kfun, lambda a: (v[0] + v[1]) * _ones(a), x, y, xs, noise, c)


def _period_kernel(P):
    return torch.exp(P["lv"][0]) * st.EQ().stretch(torch.exp(P["ls"][0])).periodic(torch.exp(P["lp"])) + torch.exp(P["lv"][1]) * st.EQ().stretch(torch.exp(P["ls"][1]))


def _period_ref(Q, x, y, xs, noise, c):
    v, s, p = torch.exp(Q["lv"]), torch.exp(Q["ls"]), torch.exp(Q["lp"])
    u = lambda a: torch.cat([torch.sin(2 * math.pi * a / p), torch.cos(2 * math.pi * a / p)], dim=-1)      # noqa: E731
    kfun = lambda a, b: v[0] * torch.exp(-0.5 * _q(u(a), u(b), s[0])) + v[1] * torch.exp(-0.5 * _q(a, b, s[1]))      # noqa: E731
    return _dense_posterior(kfun, lambda a: (v[0] + v[1]) * _ones(a), x, y, xs, noise, c)


MODELS = {"rq": (_rq_kernel, _rq_ref, ("la",)), "two_groups": (_two_kernel, _two_ref, ("ard",)), "period": (_period_kernel, _period_ref, ("lp",))}


def values(kinds, nb, n, ns, d, per_point, seed):
    rng = np.random.default_rng(seed)
    nk = 2 if isinstance(kinds, str) else len(kinds)
    return dict(x=rng.standard_normal((nb, n, d)), xs=rng.standard_normal((nb, ns, d)), y=rng.standard_normal((nb, n, 1)),
                lv=np.log(rng.uniform(0.5, 1.5, nk)), ls=np.log(rng.uniform(0.8, 1.6, nk)), ard=np.log(rng.uniform(0.8, 1.5, d)),
                la=np.array(np.log(1.7)), lp=np.array(np.log(2.5)), c=np.array(0.3),
                lnoise=np.log(rng.uniform(0.1, 0.3, (nb, n))) if per_point else np.array(np.log(0.2))), rng.uniform(0.5, 1.5, (nb, ns))


def run_case(kinds, loss, *, nb=3, n=12, ns=5, d=2, ard=False, per_point=False, pred_noise=False, mean_fn=True, call="auto", shared_x=False,
             logpdf_first=False, dev="cpu", dtype=torch.float64, seed=0, tol=1e-8, fd=False, repeat=False):
    """One model (``kinds``: a tuple of primitive kinds, or a key of ``MODELS``) and one loss (mean / var / ucb): the values against the
    ``torch.no_grad()`` plain path bit for bit, the values and every leaf's gradient against the fp64 reference entry by entry
    (relative to the largest reference entry, ``tol``), ``fd``: the hyper-parameters and the noise against central differences.
    Returns the leaves (their ``.grad`` filled)."""
    p, wts_np = values(kinds, nb, n, ns, d, per_point, seed)
    named = isinstance(kinds, str)
    names = ["x", "xs", "y", "lv", "ls", "lnoise"] + (["ard"] if ard else []) + (["c"] if mean_fn else []) + (list(MODELS[kinds][2]) if named else [])

    def leaves(vals, dt=dtype):
        return {k: torch.tensor(vals[k], dtype=dt, device=dev, requires_grad=k in names) for k in vals}

    def ours(P, grad=True):
        if named:
            kernel = MODELS[kinds][0](P)
        else:
            vs, ss = torch.exp(P["lv"]), torch.exp(P["ls"])
            kernel = sum(vs[i] * KINDS[k]().stretch(ss[i]) for i, k in enumerate(kinds))
            if ard:
                kernel = kernel.stretch(torch.exp(P["ard"]))
        c = P["c"]
        f = st.GP((lambda z: c * torch.ones(tuple(z.shape[:-1]) + (1,), dtype=z.dtype, device=z.device)), kernel) if mean_fn else st.GP(kernel)
        x = P["x"][:1].expand(nb, n, d) if shared_x else P["x"]
        obs = f(x, torch.exp(P["lnoise"]))
        if logpdf_first:
            with torch.no_grad():
                obs.logpdf(P["y"])                  # (leaves the factor and the whitened residual with the observations)
        post = f | (obs, P["y"])
        fdd = post(P["xs"], 0.05) if pred_noise else post(P["xs"])
        with torch.set_grad_enabled(grad):
            if call == "bounds":
                m, lo, hi = fdd.marginal_credible_bounds()
                return m.reshape(nb, ns), ((hi - lo) / (2 * 1.96)).reshape(nb, ns) ** 2
            if call == "mean":
                return fdd.mean[..., 0], None
            if call == "var":
                return None, fdd.var_diag.reshape(nb, ns)
            m, v = fdd.marginals()
            return m.reshape(nb, ns), v.reshape(nb, ns)

    P = leaves(p)
    wts = torch.tensor(wts_np, dtype=dtype, device=dev)
    mean, var = ours(P)
    with torch.no_grad():
        plain = ours(leaves(p), grad=False)
    for a, b in zip((mean, var), plain):          # the values are the plain path's, bit for bit
        if a is not None:
            assert a.requires_grad and torch.equal(a.detach(), b), (a, b)
    total = _loss(loss, mean, var, wts)
    total.backward(retain_graph=repeat)
    if repeat:                                    # a repeated backward is bit-identical
        first = {k: P[k].grad.clone() for k in names if P[k].grad is not None}
        for k in first:
            P[k].grad = None
        total.backward()
        for k, g in first.items():
            assert torch.equal(g, P[k].grad), k

    Q = leaves(p, torch.float64)                 # (the reference in fp64 whatever the path's precision)
    mean_c = Q["c"] if mean_fn else torch.zeros((), dtype=torch.float64, device=dev)
    vtol = 1e-9 if dtype == torch.float64 else 1e-3
    noise = torch.exp(Q["lnoise"])
    rms, rvs = [], []
    for b in range(nb):
        xb = Q["x"][0] if shared_x else Q["x"][b]
        nz = noise[b] if per_point else noise
        if named:
            rm, rv = MODELS[kinds][1](Q, xb, Q["y"][b], Q["xs"][b], nz, mean_c)
        else:
            rm, rv = _posterior_t(kinds, torch.exp(Q["lv"]), torch.exp(Q["ls"]), xb, Q["y"][b], Q["xs"][b], nz, mean_c,
                                  torch.exp(Q["ard"]) if ard else None)
        rms.append(rm)
        rvs.append(rv + 0.05 if pred_noise else rv)
    rm, rv = torch.stack(rms), torch.stack(rvs)
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
        print(f"{kinds} {loss} {k}: {err:.2e}")
        assert err <= tol, (k, err, got, ref)
    if fd:                                 # central finite differences of the values the path computes
        for k in ("lv", "ls", "lnoise"):
            base = p[k]
            flat = np.atleast_1d(base).astype(np.float64).reshape(-1)
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
    return P
