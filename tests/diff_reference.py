"""Extended-precision reference for the derivative blocks of a kernel matrix (``gpk_kmat_diff``, ``DiffKernel``), the term tables and
the inputs of the derivative tests.  Not collected by pytest.

``diff_matrices(terms, shapes, x, y, a, b, dtype)`` evaluates, in ``np.longdouble`` and on the inputs as rounded to ``dtype``, the
closed forms of ``include/gpk.h``.  A stationary term is ``v kappa(q)``, ``q = c |x - y|^2``, ``c = 1 / scale^2``, ``D_a = x[a] - y[a]``:

    d/dx_a = 2 c v kappa'(q) D_a        d/dy_b = -2 c v kappa'(q) D_b
    d^2/dx_a dy_b = v (-4 c^2 kappa''(q) D_a D_b - 2 c kappa'(q) [a == b])

    eq        kappa' = -kappa / 2                   kappa'' = kappa / 4
    rq        kappa' = -(1 + u)^(-alpha - 1) / 2    kappa'' = (alpha + 1) / (4 alpha) (1 + u)^(-alpha - 2),   u = q / (2 alpha)
    matern52  kappa' = -(5/6) (1 + s) e^(-s)        kappa'' = (25/12) e^(-s),      s = sqrt(5 q)
    matern32  kappa' = -(3/2) e^(-s)                kappa'' = 9 / (4 s) e^(-s),    s = sqrt(3 q);  kappa'' D_a D_b = 0 at s = 0
    linear (c v <x, y>):  c v y[a],  c v x[b],  c v [a == b];      const: 0

It returns ``{"dx": (value, absum), "dy": ..., "dxy": ...}`` with

    absum = sum_t |v_t| (|first addend| + |second addend|) (1 + |argument of the term's exponential|)

-- the addends being ``4 c^2 kappa'' D_a D_b`` and ``2 c kappa' [a == b]`` of the mixed block (the single product of a one-sided block
counts as the first), the argument ``q / 2``, ``s``, or ``(alpha + 1) log1p(u)`` / ``(alpha + 2) log1p(u)`` (the larger one where both
powers are used; 0 for linear).  ``eps * absum`` stays an honest unit of an element's rounding error where the two addends of the
mixed block cancel (EQ at ``c D_a^2 = 1``).

``joint_data`` / ``joint_reference`` / ``joint_model`` / ``check_joint``: the joint model of values and slopes both test modules run, its
dense NumPy reference and the comparison.  ``kernel_value`` is the plain kernel in longdouble (for joint covariances); ``torch_kernel`` the same kernel written in torch fp64,
which the host test differentiates twice to pin the closed forms.
"""
import numpy as np

LD = np.longdouble
EPS = {"float64": LD(2.0) ** -52, "float32": LD(2.0) ** -23}

# term tables of the value tests: (terms, shapes)
EQ1 = ([("eq", 1.5, 0.75)], None)
M32 = ([("matern32", 0.75, 1.25)], None)
RQ07 = ([("rq", 1.25, 1.5)], [0.7])
EQ_LIN_CONST = ([("eq", 1.0, 1.5), ("linear", 0.5, 2.0), ("const", 0.25, 1.0)], None)
ALL8 = ([("eq", 1.0, 1.0), ("matern32", 0.5, 2.0), ("matern52", 0.75, 1.5), ("rq", 1.25, 0.75), ("linear", 0.25, 4.0), ("const", 2.0, 1.0),
         ("eq", 0.5, 3.0), ("rq", 0.375, 2.5)],
        [None, None, None, 0.7, None, None, None, 3.0])
TABLES = {"eq": EQ1, "matern32": M32, "rq0.7": RQ07, "eq+linear+const": EQ_LIN_CONST, "all8": ALL8}


def rounded(a, dtype):
    """``a`` as the dtype under test holds it, in longdouble."""
    a = np.asarray(a, dtype=np.float64)
    if dtype == "float32":
        a = a.astype(np.float32).astype(np.float64)
    return a.astype(LD)


def _profile(kind, q, alpha):
    """``(kappa, kappa', kappa'' [None for matern32: singular], |argument of the exponential|)`` at ``q`` (longdouble)."""
    if kind == "eq":
        k = np.exp(-q / 2)
        return k, -k / 2, k / 4, q / 2
    if kind == "rq":
        al = LD(alpha)
        l = np.log1p(q / (2 * al))
        return np.exp(-al * l), -np.exp(-(al + 1) * l) / 2, (al + 1) / (4 * al) * np.exp(-(al + 2) * l), (al + 2) * l
    if kind == "matern52":
        s = np.sqrt(5 * q)
        e = np.exp(-s)
        return (1 + s + s * s / 3) * e, -LD(5) / 6 * (1 + s) * e, LD(25) / 12 * e, s
    if kind == "matern32":
        s = np.sqrt(3 * q)
        e = np.exp(-s)
        return (1 + s) * e, -LD(3) / 2 * e, None, s
    raise ValueError(f"no derivative for kind {kind!r}")


def _diffs(x, y):
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    df = x[..., :, None, :] - y[..., None, :, :]
    r2 = np.zeros(df.shape[:-1], dtype=LD)
    for c in range(df.shape[-1]):
        r2 += df[..., c] * df[..., c]
    return x, y, df, r2


def ils2_of(scale):
    inv = 1.0 / float(scale)          # the double the binding hands over
    return LD(inv) * LD(inv)


def kernel_value(terms, shapes, x, y):
    x, y, _, r2 = _diffs(x, y)
    shapes = shapes or [None] * len(terms)
    out = np.zeros_like(r2)
    for (kind, v, scale), alpha in zip(terms, shapes):
        c = ils2_of(scale)
        if kind == "const":
            out += LD(v)
        elif kind == "linear":
            out += LD(v) * c * np.einsum("...ic,...jc->...ij", x, y)
        else:
            out += LD(v) * _profile(kind, c * r2, alpha)[0]
    return out


def diff_matrices(terms, shapes, x, y, a, b, dtype="float64"):
    """The three derivative blocks for the dimension ``a`` of ``x`` and ``b`` of ``y``; see the module docstring."""
    x, y, df, r2 = _diffs(rounded(x, dtype), rounded(y, dtype))
    da, db = df[..., a], df[..., b]
    same = 1 if a == b else 0
    shapes = shapes or [None] * len(terms)
    zero = np.zeros_like(r2)
    val = {k: zero.copy() for k in ("dx", "dy", "dxy")}
    ab = {k: zero.copy() for k in ("dx", "dy", "dxy")}
    for (kind, v, scale), alpha in zip(terms, shapes):
        v, c = LD(v), ils2_of(scale)
        if kind == "const":
            continue
        if kind == "linear":
            t = {"dx": c * v * (y[..., None, :, a] + zero), "dy": c * v * (x[..., :, None, b] + zero), "dxy": c * v * same + zero}
            for k in t:
                val[k] += t[k]
                ab[k] += np.abs(t[k])
            continue
        q = c * r2
        _, k1, k2, arg = _profile(kind, q, alpha)
        if k2 is None:        # matern32: kappa'' D_a D_b = 9 / 4 e^(-s) D_a D_b / s, 0 at s = 0
            s = np.sqrt(3 * q)
            pos = s > 0
            k2dd = LD(9) / 4 * np.exp(-s) * np.where(pos, da * db / np.where(pos, s, 1), np.where(np.isnan(s), s, 0))
        else:
            k2dd = k2 * da * db
        w = 1 + arg
        val["dx"] += 2 * c * v * k1 * da
        ab["dx"] += np.abs(2 * c * v * k1 * da) * w
        val["dy"] += -2 * c * v * k1 * db
        ab["dy"] += np.abs(2 * c * v * k1 * db) * w
        val["dxy"] += v * (-4 * c * c * k2dd - 2 * c * k1 * same)
        ab["dxy"] += np.abs(v) * (np.abs(4 * c * c * k2dd) + np.abs(2 * c * k1 * same)) * w
    return {k: (val[k], ab[k]) for k in val}


def elwise_constant(terms):
    """``d^2 k / dx_a dy_a`` at coincident points: ``sum_t v_t c_t {eq 1, rq 1, matern32 3, matern52 5/3, linear 1, const 0}``."""
    f = {"eq": 1, "rq": 1, "matern32": 3, "matern52": LD(5) / 3, "linear": 1, "const": 0}
    return sum(LD(v) * ils2_of(scale) * f[kind] for kind, v, scale in terms)


def ratios(got, ref, absum, dtype):
    """``|got - ref| / (eps absum)`` element by element; where nothing is added up (absum = 0) the value has to be exactly 0: +inf if not."""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(absum > 0, err / (EPS[dtype] * np.where(absum > 0, absum, 1)), np.where(err == 0, 0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


def inputs(n, m, d, seed=0, batch=None):
    """Standard-normal inputs scaled so that squared distances stay of order 1 in every dimension count."""
    rng = np.random.default_rng(1000 * seed + 100 * d + n + m)
    lead = () if batch is None else (batch,)
    x = rng.standard_normal(lead + (n, d)) / np.sqrt(d)
    y = rng.standard_normal(lead + (m, d)) / np.sqrt(d)
    return x, y


def torch_kernel(terms, shapes, x, y):
    """The plain kernel ``sum_t v_t kappa_t`` written out in torch (fp64 tensors), differentiable twice: the matern square roots are
    taken of ``q + tiny`` so that the graph stays finite; used away from coincident points only."""
    import torch

    shapes = shapes or [None] * len(terms)
    df = x[:, None, :] - y[None, :, :]
    r2 = (df * df).sum(-1)
    out = torch.zeros_like(r2)
    for (kind, v, scale), alpha in zip(terms, shapes):
        c = (1.0 / scale) ** 2
        q = c * r2
        if kind == "const":
            out = out + v
        elif kind == "linear":
            out = out + v * c * (x @ y.T)
        elif kind == "eq":
            out = out + v * torch.exp(-q / 2)
        elif kind == "rq":
            out = out + v * (1 + q / (2 * alpha)) ** (-alpha)
        elif kind == "matern32":
            s = torch.sqrt(3 * q)
            out = out + v * (1 + s) * torch.exp(-s)
        elif kind == "matern52":
            s = torch.sqrt(5 * q)
            out = out + v * (1 + s + s * s / 3) * torch.exp(-s)
        else:
            raise ValueError(kind)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# values and slopes observed jointly (D = 2): f = GP(1.3 EQ().stretch(0.7) + 0.5 Matern52()), f at 30 points, f.diff(1) at 25, noise 0.05
# ---------------------------------------------------------------------------------------------------------------------------------
JOINT_TERMS = ([("eq", 1.3, 0.7), ("matern52", 0.5, 1.0)], None)
NOISE = 0.05


def joint_data():
    rng = np.random.default_rng(42)
    xf, xd, xs = rng.uniform(-1.5, 1.5, (30, 2)), rng.uniform(-1.5, 1.5, (25, 2)), rng.uniform(-1.5, 1.5, (20, 2))
    yf = np.sin(xf[:, :1]) * np.cos(xf[:, 1:]) + 0.1 * rng.standard_normal((30, 1))
    yd = -np.sin(xd[:, :1]) * np.sin(xd[:, 1:]) + 0.1 * rng.standard_normal((25, 1))       # (slopes in dimension 1)
    return xf, xd, xs, yf, yd


def joint_reference(xf, xd, xs, yf, yd, eps, dtype="float64"):
    """Posterior mean / marginal variance of ``f`` and ``f.diff(0)`` at ``xs`` and the joint log-density of ``(f(xf), f.diff(1)(xd))``
    with noise ``NOISE`` and jitter ``eps``, dense, in longdouble-assembled blocks."""
    t, s = JOINT_TERMS
    r = lambda v: np.asarray(rounded(v, dtype), dtype=np.float64)
    xf, xd, xs = r(xf), r(xd), r(xs)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    Kff = f64(kernel_value(t, s, xf, xf))
    Kfd = f64(diff_matrices(t, s, xf, xd, 1, 1)["dy"][0])              # cov(f(xf), d1 f(xd))
    Kdd = f64(diff_matrices(t, s, xd, xd, 1, 1)["dxy"][0])
    K = np.block([[Kff, Kfd], [Kfd.T, Kdd]]) + (NOISE + eps) * np.eye(55)
    y = np.concatenate([r(yf), r(yd)])
    L = np.linalg.cholesky(K)
    w = np.linalg.solve(L, y)
    lp = float(-0.5 * (2 * np.sum(np.log(np.diag(L))) + 55 * np.log(2 * np.pi) + np.sum(w * w)))
    out = {"logpdf": lp, "K": K}
    # f at xs
    c = np.concatenate([f64(kernel_value(t, s, xs, xf)), f64(diff_matrices(t, s, xs, xd, 1, 1)["dy"][0])], axis=1)
    v = np.linalg.solve(L, c.T)
    out["f"] = ((v.T @ w)[:, 0], float(t[0][1] + t[1][1]) - np.sum(v * v, axis=0))
    # d0 f at xs: cov(d0 f(xs), f(xf)) = dx block, cov(d0 f(xs), d1 f(xd)) = mixed block
    c = np.concatenate([f64(diff_matrices(t, s, xs, xf, 0, 0)["dx"][0]), f64(diff_matrices(t, s, xs, xd, 0, 1)["dxy"][0])], axis=1)
    v = np.linalg.solve(L, c.T)
    out["d0f"] = ((v.T @ w)[:, 0], float(elwise_constant(t)) - np.sum(v * v, axis=0))
    return out


def joint_model():
    import stheno_amd.torch as st
    from stheno_amd.torch import EQ, Matern52

    with st.Measure() as prior:
        f = st.GP(1.3 * EQ().stretch(0.7) + 0.5 * Matern52())
        d0, d1 = f.diff(0), f.diff(1)
    return prior, f, d0, d1


def check_joint(ref, prior, f, d0, d1, t, tol):
    xf, xd, xs, yf, yd = joint_data()
    obs = ((f(t(xf), NOISE), t(yf)), (d1(t(xd), NOISE), t(yd)))
    lp = float(prior.logpdf(*obs))
    print("joint logpdf", lp, "numpy", ref["logpdf"])
    assert abs(lp - ref["logpdf"]) <= tol * abs(ref["logpdf"])
    post = prior | obs
    for name, p in (("f", f), ("d0f", d0)):
        mean, var = (a.detach().cpu().numpy().ravel().astype(np.float64) for a in post(p)(t(xs)).marginals())
        rm, rv = ref[name]
        em, ev = np.max(np.abs(mean - rm)) / np.max(np.abs(rm)), np.max(np.abs(var - rv)) / np.max(np.abs(rv))
        print(f"{name}: mean {em:.2e}, variance {ev:.2e} (relative to the largest entry)")
        assert em <= tol and ev <= tol, (name, em, ev)
