"""Extended-precision reference of the two kernel-gradient operations (``gpk_kmat_vjp`` / ``gpk_kmat_vjp_dense``, with and without
shaped terms), the cases both test modules run, and the inputs of each case.  Not collected by pytest.

The reference is written from the formulas in ``include/gpk.h`` in ``np.longdouble`` and works in blocks of at most 256 rows.  For
every output element it returns the value and ``absum``: the sum of the absolute values of everything the kernels add up for that
element, so that ``eps * absum`` is the natural unit of an element's rounding error however much the terms cancel.  "Everything added
up" follows the kernels' own addition chains where those are longer than the formula suggests:

* ``G_ij = (sum_c g_c a_ic a_jc - sum(g) kinv_ij) / 2`` counts ``(sum_c |g_c a_ic a_jc| + |sum(g) kinv_ij|) / 2``;
* ``Geff_ij = g_ij colscale_j + w_i b_j`` counts ``|g_ij colscale_j| + |w_i b_j|``;
* the linear kind's ``<x, y>`` counts ``sum_c |x_c y_c|``;
* RQ's ``d kappa / d alpha = kappa (u / (1 + u) - log1p(u))`` counts ``kappa (u / (1 + u) + log1p(u))``;
* ``gradx_i = sum_j Geff_ij [cS_ij (x_i - y_j) + cL_ij y_j]`` is evaluated by the kernel as ``(sum_j Geff cS) x_i + sum_j Geff (cL - cS)
  y_j`` and counts ``|Geff| (|cS| (|x_i| + |y_j|) + |cL| |y_j|)``.

Conventions (``gpk.h`` and the kernels): squared distances from direct differences; the linear kind uses ``<x, y> / scale^2``;
``kappa'`` of Matern-1/2 is 0 at q = 0; only the lower triangle of ``kinv`` is read and mirrored; ``1 / scale^2`` is the square of the
double ``1 / scale`` the binding hands over.

Every reference function can be restricted to one part of the sum (``rows`` / ``cols``: a range of pairs; ``only_col``: one column of A;
``only_term``: one term) or to the leading ``ndims`` input dimensions.  By linearity, the reference with a contribution removed is the
full reference minus the reference restricted to that contribution; the discrimination test uses this.
"""
import zlib

import numpy as np

LD = np.longdouble
BLOCK = 256
TILE = 64
DCHUNK = 8

EPS = {"float64": LD(2.0) ** -52, "float32": LD(2.0) ** -23}


def round32(a):
    """fp64 values that fp32 represents exactly: one reference then serves both dtypes."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def ils2_of(scale):
    inv = 1.0 / float(scale)
    return LD(inv) * LD(inv)


def kappa_all(kind, q, alpha=None):
    """``(kappa, kappa' q, kappa', d kappa / d alpha, |.|-sum of d kappa / d alpha)`` at ``q`` (longdouble array)."""
    q = np.asarray(q, dtype=LD)
    zero = np.zeros_like(q)
    if kind == "eq":
        k = np.exp(-q / 2)
        dk = -k / 2
        return k, dk * q, dk, zero, zero
    if kind == "matern12":
        r = np.sqrt(q)
        k = np.exp(-r)
        pos = r > 0
        dk = np.where(pos, -k / (2 * np.where(pos, r, 1)), 0)      # singular at 0: reported as 0
        return k, -r * k / 2, dk, zero, zero
    if kind == "matern32":
        s = np.sqrt(3 * q)
        e = np.exp(-s)
        dk = -LD(3) / 2 * e
        return (1 + s) * e, dk * q, dk, zero, zero
    if kind == "matern52":
        s = np.sqrt(5 * q)
        e = np.exp(-s)
        dk = -LD(5) / 6 * (1 + s) * e
        return (1 + s + s * s / 3) * e, dk * q, dk, zero, zero
    if kind == "linear":
        return q, q, np.ones_like(q), zero, zero
    if kind == "const":
        return np.ones_like(q), zero, zero, zero, zero
    if kind == "rq":
        a = LD(alpha)
        u = q / (2 * a)
        lg = np.log1p(u)
        k = np.exp(-a * lg)
        dk = -k / (2 * (1 + u))
        return k, dk * q, dk, k * (u / (1 + u) - lg), k * (u / (1 + u) + lg)
    raise ValueError(kind)


def split_terms(terms):
    """``[(kind, variance, scale[, alpha])]`` -> ``[(kind, variance, scale)]`` and the shapes list (``None`` without any rq term)."""
    plain = [tuple(t[:3]) for t in terms]
    shapes = [t[3] if len(t) > 3 else None for t in terms]
    return plain, (shapes if any(s is not None for s in shapes) else None)


def _pairs(xa, ya, nd, inner=True):
    """Squared distances, inner products and sums of |x_c y_c| of two point blocks over the first ``nd`` dimensions (``inner``: whether
    a linear term needs the latter two)."""
    r2 = np.zeros((xa.shape[0], ya.shape[0]), dtype=LD)
    dot = np.zeros_like(r2) if inner else None
    adot = np.zeros_like(r2) if inner else None
    for c in range(nd):
        a, b = xa[:, c, None], ya[None, :, c]
        df = a - b
        r2 += df * df
        if inner:
            p = a * b
            dot += p
            adot += np.abs(p)
    return r2, dot, adot


def _rng(r, n):
    return (0, n) if r is None else (max(r[0], 0), min(r[1], n))


def _term_values(term, r2, dot, adot):
    kind, var, scale = term[:3]
    il2 = ils2_of(scale)
    q = (dot if kind == "linear" else r2) * il2
    k, dkq, dk, da, ada = kappa_all(kind, q, term[3] if len(term) > 3 else None)
    kab = adot * il2 if kind == "linear" else np.abs(k)
    return LD(var), il2, k, dkq, dk, da, ada, kab


def logdensity(terms, x, kinv, alpha, g, *, rows=None, cols=None, ndims=None, only_col=None, only_term=None):
    """Reference of ``HipBackend.kmat_vjp``: ``{"S": (nt, 2 | 3), "trace": (), "diag": (n,)}``, each a ``(value, absum)`` pair."""
    x, kinv, A = (np.asarray(a, dtype=LD) for a in (x, kinv, alpha))
    g = np.asarray(g, dtype=LD)
    n, d = x.shape
    nd = d if ndims is None else ndims
    nt = len(terms)
    ns = 3 if split_terms(terms)[1] is not None else 2
    s = g.sum() if only_col is None else LD(0)
    gcols = range(A.shape[1]) if only_col is None else [only_col]
    S, Sa = np.zeros((nt, ns), dtype=LD), np.zeros((nt, ns), dtype=LD)
    tr, tra = LD(0), LD(0)
    dg, dga = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    (r0, r1), (c0, c1) = _rng(rows, n), _rng(cols, n)
    for i0 in range(r0, r1, BLOCK):
        i1 = min(i0 + BLOCK, r1)
        j1 = min(i1, c1)
        if j1 <= c0:
            continue
        ii, jj = np.arange(i0, i1)[:, None], np.arange(c0, j1)[None, :]
        low = jj <= ii
        kl = np.where(low, kinv[i0:i1, c0:j1], 0)        # the strict upper triangle is not read
        aa, aab = np.zeros(kl.shape, dtype=LD), np.zeros(kl.shape, dtype=LD)
        for c in gcols:
            p = g[c] * A[i0:i1, c, None] * A[None, c0:j1, c]
            aa += p
            aab += np.abs(p)
        G = np.where(low, (aa - s * kl) / 2, 0)
        Ga = np.where(low, (aab + np.abs(s * kl)) / 2, 0)
        on = jj == ii
        if only_term is None:
            tr += G[on].sum()
            tra += Ga[on].sum()
            di = np.arange(max(i0, c0), j1)
            dg[di] = G[di - i0, di - c0]
            dga[di] = Ga[di - i0, di - c0]
        W = np.where(on, 1, 2) * G       # symmetry: off-diagonal entries count twice
        Wa = np.where(on, 1, 2) * Ga
        r2, dot, adot = _pairs(x[i0:i1], x[c0:j1], nd, any(t[0] == "linear" for t in terms))
        for t, term in enumerate(terms):
            if only_term is not None and t != only_term:
                continue
            _, _, k, dkq, _, da, ada, kab = _term_values(term, r2, dot, adot)
            S[t, 0] += (W * k).sum()
            Sa[t, 0] += (Wa * kab).sum()
            S[t, 1] += (W * dkq).sum()
            Sa[t, 1] += (Wa * (kab if term[0] == "linear" else np.abs(dkq))).sum()
            if ns == 3:
                S[t, 2] += (W * da).sum()
                Sa[t, 2] += (Wa * ada).sum()
    return {"S": (S, Sa), "trace": (tr, tra), "diag": (dg, dga)}


def dense(terms, x, y, g, colscale=None, w=None, b=None, *, rows=None, cols=None, ndims=None, only_term=None):
    """Reference of ``HipBackend.kmat_vjp_dense``: ``{"S": (nt, 2 | 3), "colsum": (m,), "gradx": (n, d)}`` as ``(value, absum)``."""
    x, y, g = (np.asarray(a, dtype=LD) for a in (x, y, g))
    n, d = x.shape
    m = y.shape[0]
    nd = d if ndims is None else ndims
    nt = len(terms)
    ns = 3 if split_terms(terms)[1] is not None else 2
    S, Sa = np.zeros((nt, ns), dtype=LD), np.zeros((nt, ns), dtype=LD)
    cs, csa = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
    gx, gxa = np.zeros((n, d), dtype=LD), np.zeros((n, d), dtype=LD)
    (r0, r1), (c0, c1) = _rng(rows, n), _rng(cols, m)
    if c1 <= c0:
        r1 = r0
    yc = y[c0:c1]
    linear = any(t[0] == "linear" for t in terms)
    for i0 in range(r0, r1, BLOCK):
        i1 = min(i0 + BLOCK, r1)
        Ge = g[i0:i1, c0:c1]
        if colscale is not None:
            Ge = Ge * np.asarray(colscale, dtype=LD)[None, c0:c1]
        Ga = np.abs(Ge)
        if w is not None:
            wb = np.asarray(w, dtype=LD)[i0:i1, None] * np.asarray(b, dtype=LD)[None, c0:c1]
            Ge = Ge + wb
            Ga = Ga + np.abs(wb)
        r2, dot, adot = _pairs(x[i0:i1], yc, nd, linear)
        kf, kfa = np.zeros_like(r2), np.zeros_like(r2)
        cS, cSa, cL, cLa = (np.zeros_like(r2) for _ in range(4))
        for t, term in enumerate(terms):
            if only_term is not None and t != only_term:
                continue
            var, il2, k, dkq, dk, da, ada, kab = _term_values(term, r2, dot, adot)
            S[t, 0] += (Ge * k).sum()
            Sa[t, 0] += (Ga * kab).sum()
            S[t, 1] += (Ge * dkq).sum()
            Sa[t, 1] += (Ga * (kab if term[0] == "linear" else np.abs(dkq))).sum()
            if ns == 3:
                S[t, 2] += (Ge * da).sum()
                Sa[t, 2] += (Ga * ada).sum()
            kf += var * k
            kfa += np.abs(var) * kab
            if term[0] == "linear":
                cL += var * il2
                cLa += np.abs(var * il2)
            else:
                cS += 2 * var * il2 * dk
                cSa += np.abs(2 * var * il2 * dk)
        cs[c0:c1] += (Ge * kf).sum(0)
        csa[c0:c1] += (Ga * kfa).sum(0)
        E, Ea = Ge * cS, Ga * cSa
        if linear:
            F, Fa = Ge * cL, Ga * cLa
        for c in range(nd):
            xi, yj = x[i0:i1, c, None], yc[None, :, c]
            gx[i0:i1, c] += (E * (xi - yj)).sum(1)
            gxa[i0:i1, c] += (Ea * (np.abs(xi) + np.abs(yj))).sum(1)
            if linear:
                gx[i0:i1, c] += (F * yj).sum(1)
                gxa[i0:i1, c] += (Fa * np.abs(yj)).sum(1)
    return {"S": (S, Sa), "colsum": (cs, csa), "gradx": (gx, gxa)}


def difference(full, part):
    """``full - part``, element by element: the reference with the contribution ``part`` removed (values only)."""
    return {k: full[k][0] - part[k][0] for k in full}


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
# variances are fp32 numbers; 1 / scale^2 is one too (0.8 -> 1.5625, 1.6 -> 0.390625), so a term's parameters are the same numbers
# in both dtypes (all but alpha = 0.4, which the fp32 launch rounds: 0.2 eps of kappa at the largest u)
ALONE = {
    "eq": [("eq", 1.25, 0.8)],
    "matern12": [("matern12", 0.75, 1.0)],
    "matern32": [("matern32", 1.5, 0.8)],
    "matern52": [("matern52", 0.5, 1.6)],
    "linear": [("linear", 0.75, 2.0)],
    "const": [("const", 1.25, 1.0)],
    "rq0.4": [("rq", 1.5, 0.8, 0.4)],
    "rq9": [("rq", 0.75, 1.0, 9.0)],
}
MIX8 = [("eq", 1.25, 0.8), ("matern12", 0.75, 1.0), ("matern32", 1.5, 1.6), ("matern52", 0.5, 2.0), ("linear", 0.75, 2.0),
        ("const", 0.25, 1.0), ("eq", 0.5, 4.0), ("matern52", 2.0, 0.8)]
MIX8RQ = [("rq", 1.5, 0.8, 0.4), ("matern12", 0.75, 1.0), ("matern32", 1.5, 1.6), ("linear", 0.75, 2.0), ("rq", 0.75, 1.0, 9.0),
          ("const", 0.25, 1.0), ("eq", 0.5, 4.0), ("matern52", 2.0, 0.8)]
TERMSETS = dict(ALONE, mix8=MIX8, mix8rq=MIX8RQ, rq_eq_rq=[("rq", 1.5, 0.8, 0.4), ("eq", 1.25, 1.0), ("rq", 0.75, 1.6, 9.0)],
                materns_rq=[("matern12", 0.75, 1.0), ("matern32", 1.5, 0.8), ("matern52", 0.5, 1.6), ("rq", 1.5, 0.8, 0.4)],
                eq_matern52=[("eq", 1.25, 0.8), ("matern52", 0.5, 1.6)], matern32_rq=[("matern32", 1.5, 0.8), ("rq", 0.75, 1.0, 9.0)],
                matern12_matern52=[("matern12", 0.75, 1.0), ("matern52", 0.5, 0.8)])


def _ld_case(n, C, d, terms, **flags):
    name = f"n{n}-C{C}-d{d}-{terms}" + "".join(f"-{k}" for k in sorted(flags))
    return dict(form="logdensity", id=name, n=n, C=C, d=d, terms=terms, **flags)


def _logdensity_cases():
    cs = []
    # every kind alone, at rotating sizes
    for (n, C, d), t in zip([(65, 3, 8), (129, 1, 9), (63, 8, 1), (200, 3, 17), (64, 1, 8), (65, 8, 8), (129, 3, 1), (200, 1, 8)],
                            ALONE):
        cs.append(_ld_case(n, C, d, t))
    # n through the tile edges (1000: 16 tile rows, 136 workgroups)
    for n, C, d, t in [(1, 1, 8, "eq"), (1, 8, 17, "mix8rq"), (63, 3, 9, "mix8"), (64, 8, 17, "mix8rq"), (65, 1, 1, "mix8"),
                       (129, 8, 8, "eq_matern52"), (200, 8, 9, "mix8rq"), (200, 1, 1, "mix8"), (1000, 3, 9, "eq"),
                       (1000, 8, 1, "matern32_rq"), (1000, 1, 17, "linear")]:
        cs.append(_ld_case(n, C, d, t))
    # C x d with all eight terms in one call
    for i, (C, d) in enumerate((C, d) for C in (1, 3, 8) for d in (1, 8, 9, 17)):
        cs.append(_ld_case(130, C, d, "mix8rq" if i % 2 else "mix8"))
    # sum(g) = 0, strides, memory that is not read, coincident points
    cs.append(_ld_case(129, 3, 8, "eq_matern52", zero_sum=True))
    cs.append(_ld_case(65, 3, 9, "mix8", ldk_pad=True))
    cs.append(_ld_case(129, 8, 8, "mix8rq", nan_upper=True))
    cs.append(_ld_case(200, 3, 17, "matern32_rq", ldk_pad=True, nan_upper=True))
    cs.append(_ld_case(1, 1, 8, "rq9", ldk_pad=True))
    cs.append(_ld_case(200, 3, 3, "materns_rq", coincident=True))
    cs.append(_ld_case(200, 8, 9, "materns_rq", coincident=True, nan_upper=True))
    return cs


def _dn_case(n, m, d, terms, cot="plain", colsum=True, gradx=True, **flags):
    name = f"n{n}-m{m}-d{d}-{terms}-{cot}-" + ("c" if colsum else "") + ("x" if gradx else "") + "".join(f"-{k}" for k in sorted(flags))
    return dict(form="dense", id=name, n=n, m=m, d=d, terms=terms, cot=cot, colsum=colsum, gradx=gradx, **flags)


SHAPES = [(1, 1), (63, 65), (64, 64), (65, 129), (130, 1000)]
MULTI_TILE_CHUNK = _dn_case(2049, 4100, 2, "eq", "scaled+rank1", True, True)


def _dense_cases():
    cs = []
    # every shape with a positive cotangent (S free of cancellation), then with a signed one under the other options
    for (n, m), d, t in zip(SHAPES, (3, 8, 1, 3, 8), ("eq_matern52", "mix8", "matern32", "mix8", "eq_matern52")):
        cs.append(_dn_case(n, m, d, t, "plain", positive=True))
    for (n, m), d, t, cot in zip(SHAPES, (1, 3, 8, 8, 3), ("mix8", "eq", "mix8", "matern12_matern52", "mix8"),
                                 ("scaled+rank1", "scaled", "rank1", "scaled+rank1", "scaled+rank1")):
        cs.append(_dn_case(n, m, d, t, cot))
    # outputs requested x cotangent options (the kernel's barriers differ between the former)
    for i, (c, gx) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        for j, cot in enumerate(("plain", "scaled", "rank1", "scaled+rank1")):
            if (i + j) % 2 == 0 or (c and gx):
                cs.append(_dn_case(65, 129, (1, 3, 8)[(i + j) % 3], "mix8" if j % 2 else "eq_matern52", cot, c, gx))
    # d past one staged chunk (no gradx), every kind alone
    for d, t in [(9, "mix8"), (20, "mix8"), (9, "eq"), (20, "matern52"), (9, "linear")]:
        cs.append(_dn_case(63, 65, d, t, "scaled+rank1", True, False))
    for (d, gx), t in zip([(1, True), (3, True), (8, True), (20, False), (9, False), (8, True), (3, True), (1, True)], ALONE):
        cs.append(_dn_case(65, 129, d, t, "scaled", True, gx))
    # padded cotangent, y is x, rq
    cs.append(_dn_case(65, 129, 3, "mix8", "scaled+rank1", padded=True))
    cs.append(_dn_case(130, 1000, 8, "eq", "plain", padded=True, positive=True))
    cs.append(_dn_case(1, 1, 1, "matern12", "plain", padded=True))
    cs.append(_dn_case(200, 200, 3, "matern12_matern52", "scaled+rank1", y_is_x=True))
    cs.append(_dn_case(65, 65, 8, "matern12_matern52", "plain", y_is_x=True, positive=True))
    cs.append(_dn_case(65, 129, 3, "rq_eq_rq", "scaled+rank1"))
    cs.append(_dn_case(130, 1000, 8, "mix8rq", "plain", positive=True))
    cs.append(_dn_case(63, 65, 9, "mix8rq", "scaled", True, False))
    cs.append(_dn_case(64, 64, 1, "rq_eq_rq", "rank1", False, True))
    cs.append(MULTI_TILE_CHUNK)
    return cs


LOGDENSITY_CASES = _logdensity_cases()
DENSE_CASES = _dense_cases()


def make_inputs(case):
    """The inputs of a case: fp64 arrays holding fp32 numbers, points scaled so that q <= 12 for the term of the smallest scale."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    terms = TERMSETS[case["terms"]]
    n, d = case["n"], case["d"]
    side = min(t[2] for t in terms) * np.sqrt(12.0 / d)

    def points(k):
        return round32(rng.uniform(-0.5, 0.5, (k, d)) * side)

    x = points(n)
    if case["form"] == "logdensity":
        if case.get("coincident"):
            x[n - 20:] = x[:20]
        C = case["C"]
        kinv = round32(rng.standard_normal((n, n)) + 4.0 * np.eye(n))
        alpha = round32(rng.standard_normal((n, C)))
        if case.get("zero_sum"):
            gv = np.array([1.5, -0.5, -1.0])[:C]
            assert gv.sum() == 0 and len(gv) == C
        else:
            gv = rng.integers(1, 13, C) / 8.0 * np.where(np.arange(C) % 3 == 2, -1.0, 1.0)       # eighths: the sum is exact
        return dict(terms=terms, x=x, kinv=kinv, alpha=alpha, g=gv)
    m = case["m"]
    y = x if case.get("y_is_x") else points(m)
    g = round32(rng.uniform(0.5, 1.5, (n, m)) if case.get("positive") else rng.standard_normal((n, m)))
    cot = case["cot"]
    colscale = round32(rng.uniform(0.5, 2.0, m) * (1 if case.get("positive") else rng.choice([-1.0, 1.0], m))) if "scaled" in cot else None
    w = round32(rng.standard_normal(n)) if "rank1" in cot else None
    b = round32(rng.standard_normal(m)) if "rank1" in cot else None
    return dict(terms=terms, x=x, y=y, g=g, colscale=colscale, w=w, b=b)


_CACHE = {}


def reference(case):
    """``(inputs, reference)`` of a case, computed once per process and shared (read-only) by every test that needs it."""
    if case["id"] not in _CACHE:
        inp = make_inputs(case)
        if case["form"] == "logdensity":
            ref = logdensity(inp["terms"], inp["x"], inp["kinv"], inp["alpha"], inp["g"])
        else:
            ref = dense(inp["terms"], inp["x"], inp["y"], inp["g"], inp["colscale"], inp["w"], inp["b"])
        for v in inp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        for val, ab in ref.values():
            for a in (val, ab):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _CACHE[case["id"]] = (inp, ref)
    return _CACHE[case["id"]]


def ratios(got, ref, absum, dtype):
    """``|got - ref| / (eps * absum)`` element by element; an element nothing is added up for (absum = 0) has to be exactly 0: +inf if not."""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    ref, absum = np.asarray(ref, dtype=LD), np.asarray(absum, dtype=LD)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(absum > 0, err / (EPS[dtype] * np.where(absum > 0, absum, 1)), np.where(err == 0, 0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)
