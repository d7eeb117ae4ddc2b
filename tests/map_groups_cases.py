"""Shared by ``test_map_groups_grad_host.py`` and ``test_map_groups_grad_gpu.py``: the models, the closed forms in NumPy and the
finite-difference references for gradients of sums of kernels behind DIFFERENT input maps.

The reference everywhere is central finite differences (h = 1e-6) of a NumPy closed form -- the method of
``tests/test_rq_periodic_gpu.py`` -- and the bar ``|autograd - fd| <= 1e-6 max(max|fd|, 1)``; values are held to 1e-6 relative.  For
the model below the finite differences at h = 1e-6 and h = 1e-5 agree to 3e-9 over the hyper-parameters and to 2e-8 over the inputs (the
condition number of K is 3e2), so the reference alone stays far inside the bar.

Three groups:  1.2 EQ.stretch(0.9) + 0.3 Linear  (inputs as they are),  0.7 EQ.periodic(3.1),  0.5 RQ(0.8).stretch([0.8, 1.7]).
Every reference is computed once per process (``functools.lru_cache``) and never written to."""
import functools

import numpy as np
import scipy.linalg as sl
import torch

import stheno_amd.torch as st
from stheno_amd.torch import EQ, RQ, Linear

EPS = 1e-10
N, NS = 130, 33
NA, NB = 70, 60
NOISE, NOISE_B = 0.3, 0.2
H = 1e-6

#: the nine hyper-parameters of the three-group kernel, in the order of the finite-difference vector
NAMES = ["v_eq", "s_eq", "v_lin", "v_per", "period", "v_rq", "l0", "l1", "alpha"]
P0 = np.array([1.2, 0.9, 0.3, 0.7, 3.1, 0.5, 0.8, 1.7, 0.8])
#: ... and those that sit in front of no input map (variances and the scalar scale)
PLAIN = ["v_eq", "s_eq", "v_lin", "v_per", "v_rq"]

JOINT_NAMES = ["v1", "s1", "v2", "period"]
JOINT_P0 = np.array([1.2, 0.9, 0.7, 3.1])


# ---------------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------------
def d2(a, b):
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def eq_np(a, b, scale=1.0, var=1.0):
    return var * np.exp(-0.5 * d2(a, b) / scale**2)


def rq_np(a, b, alpha, var=1.0):
    return var * np.exp(-alpha * np.log1p(d2(a, b) / (2 * alpha)))


def pmap(x, p):
    a = 2 * np.pi * x / p
    return np.concatenate([np.sin(a), np.cos(a)], axis=-1)


def kern3_np(p, a, b):
    """The three-group kernel at the hyper-parameters ``p`` (in the order of ``NAMES``)."""
    v_eq, s_eq, v_lin, v_per, period, v_rq, l0, l1, alpha = p
    ls = np.array([l0, l1])
    return (eq_np(a, b, s_eq, v_eq) + v_lin * (a @ b.T) + eq_np(pmap(a, period), pmap(b, period), 1.0, v_per)
            + rq_np(a / ls, b / ls, alpha, v_rq))


def logpdf_np(k, y):
    l = np.linalg.cholesky(k)
    w = sl.solve_triangular(l, y, lower=True)
    return float(-0.5 * (2 * np.sum(np.log(np.diag(l))) + len(y) * np.log(2 * np.pi) + np.sum(w * w)))


def post_np(kf, x, y, xs, noise):
    k = kf(x, x) + (noise + EPS) * np.eye(x.shape[0])
    l = np.linalg.cholesky(k)
    v = sl.solve_triangular(l, kf(x, xs), lower=True)
    w = sl.solve_triangular(l, y, lower=True)
    kd = np.array([kf(xs[i:i + 1], xs[i:i + 1])[0, 0] for i in range(xs.shape[0])])
    return (v.T @ w)[:, 0], kd - (v * v).sum(0)


def fd_grad(fun, p, h=H):
    g = np.zeros_like(p)
    for i in range(p.size):
        e = np.zeros_like(p)
        e.flat[i] = h
        g.flat[i] = (fun(p + e) - fun(p - e)) / (2 * h)
    return g


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(42)
    x = rng.uniform(-2.0, 2.0, (N, 2))
    xs = rng.uniform(-2.0, 2.0, (NS, 2))
    y = np.sin(x[:, :1]) + 0.3 * rng.standard_normal((N, 1))
    ys = np.sin(xs[:, :1]) + 0.3 * rng.standard_normal((NS, 1))
    for a in (x, xs, y, ys):
        a.setflags(write=False)
    return x, xs, y, ys


# ---------------------------------------------------------------------------------------------
# objectives in NumPy and their references (each once)
# ---------------------------------------------------------------------------------------------
def logpdf_obj(p, x, y, noise):
    return logpdf_np(kern3_np(p, x, x) + (noise + EPS) * np.eye(x.shape[0]), y)


@functools.lru_cache(maxsize=None)
def logpdf_reference():
    x, _, y, _ = data()
    return dict(
        value=logpdf_obj(P0, x, y, NOISE),
        hyper=fd_grad(lambda p: logpdf_obj(p, x, y, NOISE), P0.copy()),
        noise=fd_grad(lambda s: logpdf_obj(P0, x, y, s[0]), np.array([NOISE]))[0],
        y=fd_grad(lambda yy: logpdf_obj(P0, x, yy.reshape(y.shape), NOISE), y.copy().ravel()).reshape(y.shape),
        x=fd_grad(lambda xx: logpdf_obj(P0, xx.reshape(x.shape), y, NOISE), x.copy().ravel()).reshape(x.shape),
    )


def marginals_obj(p, x, y, xs):
    mu, var = post_np(lambda a, b: kern3_np(p, a, b), x, y, xs, NOISE)
    return float(mu.sum() + var.sum())


@functools.lru_cache(maxsize=None)
def marginals_reference():
    x, xs, y, _ = data()
    return dict(
        value=marginals_obj(P0, x, y, xs),
        hyper=fd_grad(lambda p: marginals_obj(p, x, y, xs), P0.copy()),
        x=fd_grad(lambda xx: marginals_obj(P0, xx.reshape(x.shape), y, xs), x.copy().ravel()).reshape(x.shape),
        xs=fd_grad(lambda xx: marginals_obj(P0, x, y, xx.reshape(xs.shape)), xs.copy().ravel()).reshape(xs.shape),
    )


def joint_obj(p):
    """Dense block covariance of ``(f(xa) + noise, f2(xb) + noise_b)`` with ``f = f1 + f2``."""
    v1, s1, v2, period = p
    x, _, y, _ = data()
    xa, xb = x[:NA], x[NA:]

    def k2(a, b):
        return eq_np(pmap(a, period), pmap(b, period), 1.0, v2)

    top = np.concatenate([eq_np(xa, xa, s1, v1) + k2(xa, xa) + (NOISE + EPS) * np.eye(NA), k2(xa, xb)], axis=1)
    bot = np.concatenate([k2(xb, xa), k2(xb, xb) + (NOISE_B + EPS) * np.eye(NB)], axis=1)
    return logpdf_np(np.concatenate([top, bot], axis=0), y)


@functools.lru_cache(maxsize=None)
def joint_reference():
    return dict(value=joint_obj(JOINT_P0), hyper=fd_grad(joint_obj, JOINT_P0.copy()))


def predictive_obj(p):
    """``log p(ys | y)`` at ``xs`` as the density of the Gaussian conditional (noise and jitter on both diagonals, as the model adds
    them)."""
    x, xs, y, ys = data()
    kxx = kern3_np(p, x, x) + (NOISE + EPS) * np.eye(N)
    kxs = kern3_np(p, x, xs)
    l = np.linalg.cholesky(kxx)
    v = sl.solve_triangular(l, kxs, lower=True)
    w = sl.solve_triangular(l, y, lower=True)
    return logpdf_np(kern3_np(p, xs, xs) + (NOISE + EPS) * np.eye(NS) - v.T @ v, ys - v.T @ w)


@functools.lru_cache(maxsize=None)
def predictive_reference():
    return dict(value=predictive_obj(P0), hyper=fd_grad(predictive_obj, P0.copy()))


# ---------------------------------------------------------------------------------------------
# the same models in the package
# ---------------------------------------------------------------------------------------------
def three_group_kernel(learn=NAMES, dtype=torch.float64):
    """``(kernel, leaves)``: ``leaves`` maps the names of ``NAMES`` to the tensors behind them (``l0`` / ``l1`` are entries of
    ``leaves["l"]``); those named in ``learn`` require a gradient."""
    val = dict(zip(NAMES, P0))

    def leaf(name, value):
        return torch.tensor(value, dtype=dtype, requires_grad=name in learn)

    t = {k: leaf(k, val[k]) for k in NAMES if k not in ("l0", "l1")}
    t["l"] = leaf("l0", [val["l0"], val["l1"]])
    k = (t["v_eq"] * EQ().stretch(t["s_eq"]) + t["v_lin"] * Linear() + t["v_per"] * EQ().periodic(t["period"])
         + t["v_rq"] * RQ(t["alpha"]).stretch(t["l"]))
    return k, t


def hyper_grads(t, names=NAMES):
    out = []
    for name in names:
        if name in ("l0", "l1"):
            out.append(float(t["l"].grad[int(name[1])]))
        else:
            out.append(float(t[name].grad))
    return np.array(out)


def joint_model(dtype=torch.float64):
    t = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in zip(JOINT_NAMES, JOINT_P0)}
    with st.Measure() as prior:
        f1 = st.GP(t["v1"] * EQ().stretch(t["s1"]))
        f2 = st.GP(t["v2"] * EQ().periodic(t["period"]))
        f = f1 + f2
    return prior, f, f2, t


def assert_close(what, got, ref, tol=1e-6):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    dev, scale = float(np.max(np.abs(got - ref))), max(float(np.max(np.abs(ref))), 1.0)
    print(f"{what}: worst deviation {dev:.3e}, largest reference entry {float(np.max(np.abs(ref))):.3e}, bar {tol * scale:.3e}")
    assert dev <= tol * scale, (what, dev, tol * scale)


def assert_value(what, got, ref, tol=1e-6):
    print(f"{what}: {got!r} against {ref!r}")
    assert abs(got - ref) <= tol * abs(ref), (what, got, ref)


# ---------------------------------------------------------------------------------------------
# end to end: a short version of ``examples/learn_decomposition.py``
# ---------------------------------------------------------------------------------------------
FIT_N, FIT_STEPS, FIT_PERIOD, FIT_SEED = 300, 60, 2.0, 0


def fit_decomposition(device):
    """Trend + seasonal + noise in one dimension, fitted by Adam on the log-density of ``v1 EQ.stretch(l) + v2 EQ.periodic(p) + v3
    Linear`` with learnable noise, from a period 15 % off.  Returns ``(losses, learnt period)``.  (With this seed the run on the test
    suite's CPU backend ends 0.2 % from the generating period.)"""
    import math

    rng = np.random.default_rng(FIT_SEED)
    x = np.sort(rng.uniform(0.0, 10.0, FIT_N))[:, None]
    y = 0.3 * x + np.sin(0.6 * x) + 0.8 * np.sin(2 * np.pi * x / FIT_PERIOD) + 0.2 * rng.standard_normal((FIT_N, 1))
    tx, ty = torch.tensor(x, device=device), torch.tensor(y, device=device)
    start = dict(v1=1.0, l=2.0, v2=1.0, p=1.15 * FIT_PERIOD, v3=0.1, noise=0.1)
    raw = {k: torch.tensor(math.log(v), dtype=torch.float64, requires_grad=True) for k, v in start.items()}
    opt = torch.optim.Adam(list(raw.values()), lr=0.05)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        q = {k: torch.exp(v) for k, v in raw.items()}
        k = q["v1"] * EQ().stretch(q["l"]) + q["v2"] * EQ().periodic(q["p"]) + q["v3"] * Linear()
        loss = -st.GP(k)(tx, q["noise"].to(device)).logpdf(ty)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, float(torch.exp(raw["p"].detach()))
