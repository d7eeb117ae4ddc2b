"""Extended-precision reference for kernels with a ``"delta"`` term, the inputs of the Delta tests and the input condition they
all rest on.  Not collected by pytest.

``kernel_matrix(terms, shapes, x, y)`` is ``sum_t v_t kappa_t(q_t)``, ``q_t = |x_i - y_j|^2 / scale_t^2`` in ``np.longdouble`` for the
kinds ``eq``, ``matern12``, ``matern32``, ``matern52``, ``const``, ``rq`` and ``delta`` (``1`` where ``q < epsilon``, else ``0``; NaN where
``q`` is NaN), together with ``absum = sum_t |v_t kappa_t| (1 + |arg_t|)``, ``arg_t`` the argument of the term's exponential
(``q / 2``, ``sqrt(c q)``, ``alpha log1p(q / (2 alpha))``; 0 for ``const`` and ``delta``): the unit ``include/gpk.h`` states the accuracy
of the fused kernel-matrix kernels in.

The kernel-gradient reference of ``tests/vjp_reference.py`` is extended by linearity: every output of ``gpk_kmat_vjp`` /
``gpk_kmat_vjp_dense`` is a sum over terms, so the reference of a term list with Delta terms is that module's reference of the other
terms plus the Delta terms' own contribution from the formulas in ``include/gpk.h`` -- ``S1_t = sum G kappa_t``, ``S2_t = S3_t = 0``,
``v_t kappa_t`` in ``colsum``, nothing in ``gradx``.

Input condition.  A Delta value flips where ``q`` crosses ``epsilon``, and no tolerance may hide a flipped element, so no pair of
points of a value test may have ``q`` in ``[epsilon / 4, 4 epsilon]``.  Points are therefore drawn (with repetition) from a small pool
of distinct points whose coordinates are small integers over 4: ``q`` is exactly 0 for a repeated point and at least ``1 / (16 s^2)``
otherwise, computed without rounding in fp32 and fp64 for power-of-two scales ``s``.  ``check_inputs`` asserts the condition and that
at least 5 % of the elements off the diagonal are 1.
"""
import functools

import numpy as np

from . import vjp_reference as R

LD = np.longdouble
EPSILON = 1e-6          # Delta's default


def _q(x, y, scale):
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    r2 = np.zeros(x.shape[:-1] + (y.shape[-2],), dtype=LD)
    for c in range(x.shape[-1]):
        df = x[..., :, None, c] - y[..., None, :, c]
        r2 += df * df
    return r2 * R.ils2_of(scale)


def delta_kappa(q, epsilon):
    q = np.asarray(q, dtype=LD)
    return np.where(np.isnan(q), q, np.where(q < LD(epsilon), LD(1), LD(0)))


def _kappa_arg(kind, q, shape):
    """``(kappa, |argument of the exponential|)``."""
    if kind == "delta":
        return delta_kappa(q, shape), np.zeros_like(q)
    if kind == "const":
        return np.ones_like(q), np.zeros_like(q)
    if kind == "eq":
        return np.exp(-q / 2), q / 2
    if kind == "rq":
        a = LD(shape)
        arg = a * np.log1p(q / (2 * a))
        return np.exp(-arg), arg
    c = {"matern12": 1, "matern32": 3, "matern52": 5}[kind]
    s = np.sqrt(c * q)
    poly = {"matern12": 1, "matern32": 1 + s, "matern52": 1 + s + s * s / 3}[kind]
    return poly * np.exp(-s), s


def kernel_matrix(terms, shapes, x, y=None, *, with_absum=False):
    """``k(x, y)`` (``y is None``: ``k(x, x)``) in longdouble; ``with_absum``: ``(k, absum)``."""
    y = x if y is None else y
    shapes = [None] * len(terms) if shapes is None else shapes
    k = ab = None
    for (kind, var, scale), shp in zip(terms, shapes):
        kap, arg = _kappa_arg(kind, _q(x, y, scale), shp)
        t = LD(var) * kap
        k = t if k is None else k + t
        a = np.abs(t) * (1 + arg)
        ab = a if ab is None else ab + a
    return (k, ab) if with_absum else k


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def points(rng, n, d, pool=10, span=8):
    """``n`` points drawn with repetition from ``pool`` distinct points with coordinates in ``{-span, ..., span} / 4``."""
    cand = rng.integers(-span, span + 1, (4 * pool + 8, d))
    cand = cand[np.sort(np.unique(cand, axis=0, return_index=True)[1])][:pool]
    assert cand.shape[0] >= 2
    return cand[rng.integers(0, cand.shape[0], n)].astype(np.float64) / 4.0, cand.astype(np.float64) / 4.0


def check_inputs(terms, shapes, x, y=None, *, need_ones=True):
    """The input condition of every value test, asserted on the host: for every delta term no ``q`` in ``[eps / 4, 4 eps]``, and at
    least 5 % of the elements with ``i != j`` equal to 1 (when there are any such elements)."""
    sym = y is None
    y = x if sym else y
    for (kind, _, scale), eps in zip(terms, shapes or [None] * len(terms)):
        if kind != "delta":
            continue
        q = _q(x, y, scale)
        q = q[~np.isnan(q)]
        assert not np.any((q >= LD(eps) / 4) & (q <= 4 * LD(eps))), "a pair of points sits at Delta's threshold"
        if need_ones:
            n, m = np.shape(x)[-2], np.shape(y)[-2]
            off = ~np.eye(n, m, dtype=bool)
            k = delta_kappa(_q(x, y, scale), eps)[..., off]
            if k.size:
                assert np.mean(k == 1) >= 0.05, f"only {np.mean(k == 1):.3f} of the off-diagonal elements are 1"


@functools.lru_cache(maxsize=None)
def value_case(n, m, d, seed=0, batch=None):
    """``(x, y)`` of a value test (``m`` None: symmetric, ``y`` is None); ``batch``: stacked independent draws from one pool.
    Read-only arrays, made once per process."""
    rng = np.random.default_rng(10000 * seed + 100 * n + 10 * (m or 0) + d)
    reps = batch or 1
    xs, ys = [], []
    for _ in range(reps):
        x, pool = points(rng, n, d)
        xs.append(x)
        if m is not None:
            ys.append(pool[rng.integers(0, pool.shape[0], m)])
    x = np.stack(xs) if batch else xs[0]
    y = None if m is None else (np.stack(ys) if batch else ys[0])
    if m == 1 and n == 1 and not batch:
        y = x.copy()
    for a in (x, y):
        if a is not None:
            a.setflags(write=False)
    return x, y


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel-gradient kernels with a Delta term
# ---------------------------------------------------------------------------------------------------------------------------------
def _shaped(terms, shapes):
    """``[(kind, var, scale)]`` + shapes -> the 3- / 4-tuples of ``tests/vjp_reference.py`` without the delta terms, their positions,
    and the delta terms ``(position, var, scale, epsilon)``."""
    rest, keep, delta = [], [], []
    for i, ((kind, var, scale), shp) in enumerate(zip(terms, shapes)):
        if kind == "delta":
            delta.append((i, var, scale, shp))
        else:
            rest.append((kind, var, scale) if shp is None else (kind, var, scale, shp))
            keep.append(i)
    return rest, keep, delta


def _place(nt, keep, S_rest, Sa_rest):
    S, Sa = np.zeros((nt, 3), dtype=LD), np.zeros((nt, 3), dtype=LD)
    if keep:
        S[keep, : S_rest.shape[1]] = S_rest
        Sa[keep, : Sa_rest.shape[1]] = Sa_rest
    return S, Sa


def vjp_logdensity(terms, shapes, x, kinv, alpha, g):
    """Reference of ``HipBackend.kmat_vjp`` for terms that include Delta: ``{"S": (nt, 3), "trace": (), "diag": (n,)}`` as
    ``(value, absum)``; a Delta row is ``(sum_ij G_ij kappa_ij, 0, 0)`` with ``G`` symmetrised from the lower triangle of ``kinv``."""
    rest, keep, delta = _shaped(terms, shapes)
    ref = R.logdensity(rest, x, kinv, alpha, g)
    S, Sa = _place(len(terms), keep, *ref["S"])
    kl = np.tril(np.asarray(kinv, dtype=LD))
    ks = kl + np.tril(kl, -1).T
    A, gv = np.asarray(alpha, dtype=LD), np.asarray(g, dtype=LD)
    aa, aab = np.zeros_like(ks), np.zeros_like(ks)
    for c in range(A.shape[1]):
        p = gv[c] * A[:, c, None] * A[None, :, c]
        aa += p
        aab += np.abs(p)
    G, Ga = (aa - gv.sum() * ks) / 2, (aab + np.abs(gv.sum() * ks)) / 2
    for i, _, scale, eps in delta:
        k = delta_kappa(_q(x, x, scale), eps)
        S[i, 0], Sa[i, 0] = (G * k).sum(), (Ga * k).sum()
    return {"S": (S, Sa), "trace": ref["trace"], "diag": ref["diag"]}


def vjp_dense(terms, shapes, x, y, g, colscale=None, w=None, b=None):
    """Reference of ``HipBackend.kmat_vjp_dense`` for terms that include Delta: a Delta row of ``S`` is ``(sum Geff kappa, 0, 0)``,
    ``colsum`` gains ``sum_i Geff_ij v kappa_ij``, ``gradx`` nothing."""
    rest, keep, delta = _shaped(terms, shapes)
    ref = R.dense(rest, x, y, g, colscale, w, b)
    S, Sa = _place(len(terms), keep, *ref["S"])
    Ge = np.asarray(g, dtype=LD)
    if colscale is not None:
        Ge = Ge * np.asarray(colscale, dtype=LD)[None, :]
    Ga = np.abs(Ge)
    if w is not None:
        wb = np.asarray(w, dtype=LD)[:, None] * np.asarray(b, dtype=LD)[None, :]
        Ge, Ga = Ge + wb, Ga + np.abs(wb)
    cs, csa = np.array(ref["colsum"][0]), np.array(ref["colsum"][1])
    for i, var, scale, eps in delta:
        k = delta_kappa(_q(x, y, scale), eps)
        S[i, 0], Sa[i, 0] = (Ge * k).sum(), (Ga * k).sum()
        cs += (Ge * LD(var) * k).sum(0)
        csa += (Ga * np.abs(LD(var)) * k).sum(0)
    return {"S": (S, Sa), "colsum": (cs, csa), "gradx": ref["gradx"]}


#: the mixed sum of the value tests: parameters that fp32 holds exactly (1 / scale^2 and 1 / (2 alpha) too)
MIX4 = ([("eq", 1.25, 2.0), ("matern52", 0.75, 1.0), ("rq", 1.5, 2.0), ("delta", 0.5, 1.0)], [None, None, 2.0, EPSILON])
DELTA1 = ([("delta", 1.5, 1.0)], [EPSILON])
#: stretched Delta beside a constant: power-of-two scales keep q exact
DELTA_STRETCHED = ([("delta", 1.5, 0.5), ("const", 0.25, 1.0)], [EPSILON, None])
#: the kernel-gradient tests: Delta beside EQ and RQ
VJP3 = ([("eq", 1.25, 2.0), ("rq", 0.75, 1.0), ("delta", 0.5, 1.0)], [None, 2.0, EPSILON])


@functools.lru_cache(maxsize=None)
def vjp_case(form, n, m, d, cot="scaled+rank1"):
    """Inputs and reference of a kernel-gradient case with ``VJP3``: ``(inputs, reference)``, made once per process."""
    rng = np.random.default_rng(7 + 1000 * n + 10 * (m or 0) + d)
    terms, shapes = VJP3
    x, pool = points(rng, n, d, span=4)
    if form == "logdensity":
        C = 3
        kinv = R.round32(rng.standard_normal((n, n)) + 4.0 * np.eye(n))
        alpha = R.round32(rng.standard_normal((n, C)))
        gv = rng.integers(1, 13, C) / 8.0 * np.array([1.0, 1.0, -1.0])
        inp = dict(x=x, kinv=kinv, alpha=alpha, g=gv)
        check_inputs(terms, shapes, x)
        return inp, vjp_logdensity(terms, shapes, x, kinv, alpha, gv)
    y = pool[rng.integers(0, pool.shape[0], m)]
    g = R.round32(rng.standard_normal((n, m)))
    cs = R.round32(rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m)) if "scaled" in cot else None
    w = R.round32(rng.standard_normal(n)) if "rank1" in cot else None
    b = R.round32(rng.standard_normal(m)) if "rank1" in cot else None
    check_inputs(terms, shapes, x, y)
    return dict(x=x, y=y, g=g, colscale=cs, w=w, b=b), vjp_dense(terms, shapes, x, y, g, cs, w, b)
