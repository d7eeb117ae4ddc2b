"""Extended-precision reference of the VJP of a derivative block (``gpk_kmat_diff_vjp`` / ``HipBackend.kmat_diff_vjp``), the cases both
test modules run, and the inputs of each case.  Not collected by pytest.  Built on the profiles and term tables of
``tests/diff_reference.py``, in the style of ``tests/vjp_reference.py``.

With ``g`` the cotangent of the block ``sum_t v_t beta_t`` that ``gpk_kmat_diff`` writes for ``(a, b)`` (``None``: not differentiated in
that argument), ``c = 1 / scale^2``, ``q = c |x - y|^2``, ``D_a = x[a] - y[a]`` (``include/gpk.h``):

    d/dx_a          beta = 2 c kappa' D_a                                   c dbeta/dc = 2 c D_a (kappa' + q kappa'')
    d/dy_b          the same with -D_b
    d^2/dx_a dy_b   beta = -4 c^2 kappa'' D_a D_b - 2 c kappa' [a == b]
                    c dbeta/dc = -4 c^2 D_a D_b (2 kappa'' + q kappa''') - 2 c [a == b] (kappa' + q kappa'')
    linear          beta = c y[a] | c x[b] | c [a == b],  c dbeta/dc = beta;      const: 0

    S[t] = (sum g beta_t,  sum g c dbeta_t/dc,  sum g dbeta_t/dalpha_t [tables with an rq term; 0 for the other kinds])
    gradx[i, e] = sum_j g_ij sum_t v_t dbeta_t/dx_i[e]        (one-sided blocks, d <= 8)
        d/dx_a:  4 c^2 kappa'' D_a D_e + 2 c kappa' [e == a];    d/dy_b: the negative with b;    linear: 0 | c [e == b]

Every output comes with ``absum``, the sum of the absolute values of everything added up for it: the two addends of the mixed block
separately, ``kappa'`` and ``q kappa''`` (``2 kappa''`` and ``q kappa'''``) separately, rq's ``(alpha + k) u / (alpha (1 + u))`` and
``log1p(u)`` separately, and ``D_e`` of ``gradx`` as ``|x_e| + |y_e|`` (the kernel multiplies the row's sum by ``x_e`` and subtracts the
``y_e`` products).  ``eps * absum`` is then the unit of an element's rounding error however much the addends cancel.

The inputs hold fp32 numbers, so one reference serves both dtypes wherever the term table's parameters are fp32 numbers too; where they
are not (``1 / 0.75^2``, ``alpha = 0.7``), the reference is evaluated on the parameters as the dtype under test holds them (the library
converts ``inv_ls^2``, the variance and alpha to the dtype of the launch).

A reference can be restricted to part of the sum (``rows`` / ``cols``: a range of pairs, ``only_term``: one term, ``only_same``: the
``[a == b]`` addend alone) or to the leading ``ndims`` input dimensions of the squared distance; by linearity the reference with a
contribution removed is the full one minus the restricted one (``tests/test_diff_vjp_host.py``).
"""
import zlib

import numpy as np

from . import diff_reference as D

LD = np.longdouble
EPS = D.EPS
TILE = 64
DCHUNK = 8
BLOCK = 256


def round32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _as_held(v, dtype):
    """A parameter as the launch of ``dtype`` holds it (``None``: as given), in longdouble."""
    v = float(v)
    return LD(np.float32(v)) if dtype == "float32" else LD(v)


def _c_of(scale, dtype):
    inv = 1.0 / float(scale)              # the double the binding hands over; the library squares it in double
    return _as_held(inv * inv, dtype)


def params_are_fp32(terms, shapes):
    shapes = shapes or [None] * len(terms)
    return all(np.float32(v) == v and np.float32((1.0 / s) ** 2) == (1.0 / s) ** 2 and (al is None or np.float32(al) == al)
               for (_, v, s), al in zip(terms, shapes))


def profile(kind, q, alpha):
    """``kappa', kappa'', q kappa'', q kappa''', dkappa'/dalpha, dkappa''/dalpha`` and the |.|-sums of the last two at ``q``
    (longdouble); matern32's ``1 / s`` is 0 where ``s`` is not positive."""
    zero = np.zeros_like(q)
    if kind == "eq":
        k = np.exp(-q / 2)
        return -k / 2, k / 4, q * k / 4, -q * k / 8, zero, zero, zero, zero
    if kind == "matern52":
        s = np.sqrt(5 * q)
        e = np.exp(-s)
        return -LD(5) / 6 * (1 + s) * e, LD(25) / 12 * e, LD(25) / 12 * q * e, -LD(25) / 24 * s * e, zero, zero, zero, zero
    if kind == "matern32":
        s = np.sqrt(3 * q)
        e = np.exp(-s)
        pos = s > 0
        inv = np.where(pos, 1 / np.where(pos, s, 1), 0)
        return -LD(3) / 2 * e, LD(9) / 4 * e * inv, LD(3) / 4 * s * e, -LD(9) / 8 * (1 + s) * inv * e, zero, zero, zero, zero
    if kind == "rq":
        al = LD(alpha)
        u = q / (2 * al)
        lg = np.log1p(u)
        p1, p2, p3 = (np.exp(-(al + k) * lg) for k in (1, 2, 3))
        w = u / (al * (1 + u))
        r2c = (al + 1) / (4 * al)
        k1a, k1aa = -p1 / 2 * ((al + 1) * w - lg), p1 / 2 * ((al + 1) * w + lg)
        k2a = r2c * p2 * ((al + 2) * w - lg) - p2 / (4 * al * al)
        k2aa = r2c * p2 * ((al + 2) * w + lg) + p2 / (4 * al * al)
        return -p1 / 2, r2c * p2, q * r2c * p2, -(al + 1) * (al + 2) / (8 * al * al) * q * p3, k1a, k2a, k1aa, k2aa
    raise ValueError(f"no derivative for kind {kind!r}")


def _rng(r, n):
    return (0, n) if r is None else (max(r[0], 0), min(r[1], n))


def diff_vjp(terms, shapes, x, y, a, b, g, dtype=None, *, rows=None, cols=None, ndims=None, only_term=None, only_same=False):
    """``{"S": (value, absum), "gradx": (value, absum) or None}``; see the module docstring."""
    x, y, g = (np.asarray(v, dtype=LD) for v in (x, y, g))
    n, d = x.shape
    m = y.shape[0]
    nd = d if ndims is None else ndims
    nt = len(terms)
    shapes = shapes or [None] * nt
    ns = 3 if any(s is not None for s in shapes) else 2
    mixed = a is not None and b is not None
    same = mixed and a == b
    sel = a if b is None else b
    S, Sa = np.zeros((nt, ns), dtype=LD), np.zeros((nt, ns), dtype=LD)
    want_gx = not mixed and d <= DCHUNK
    gx, gxa = (np.zeros((n, d), dtype=LD), np.zeros((n, d), dtype=LD)) if want_gx else (None, None)
    (r0, r1), (c0, c1) = _rng(rows, n), _rng(cols, m)
    if c1 <= c0:
        r1 = r0
    yc = y[c0:c1]
    for i0 in range(r0, r1, BLOCK):
        i1 = min(i0 + BLOCK, r1)
        xr = x[i0:i1]
        G = g[i0:i1, c0:c1]
        Ga = np.abs(G)
        r2 = np.zeros(G.shape, dtype=LD)
        for e in range(nd):
            df = xr[:, e, None] - yc[None, :, e]
            r2 += df * df
        da = xr[:, a, None] - yc[None, :, a] if a is not None else None
        db = xr[:, b, None] - yc[None, :, b] if b is not None else None
        sd = None if mixed else (da if b is None else -db)
        cD, cDa, cS, cSa = (np.zeros(G.shape, dtype=LD) for _ in range(4))
        for t, ((kind, v, scale), al) in enumerate(zip(terms, shapes)):
            if (only_term is not None and t != only_term) or kind == "const":
                continue
            v, c = _as_held(v, dtype), _c_of(scale, dtype)
            if kind == "linear":
                if b is None:
                    be = c * yc[None, :, a] + 0 * r2
                elif a is None:
                    be = c * xr[:, b, None] + 0 * r2
                else:
                    be = c * (1 if same else 0) + 0 * r2
                if only_same and not mixed:
                    continue
                S[t, 0] += (G * be).sum()
                S[t, 1] += (G * be).sum()
                Sa[t, 0] += (Ga * np.abs(be)).sum()
                Sa[t, 1] += (Ga * np.abs(be)).sum()
                if a is None:
                    cS += v * c
                    cSa += np.abs(v * c)
                continue
            al = None if al is None else _as_held(al, dtype)
            k1, k2, qk2, qk3, k1a, k2a, k1aa, k2aa = profile(kind, c * r2, al)
            if mixed:
                f = -4 * c * c * da * db * (0 if only_same else 1)
                h = -2 * c * (1 if same else 0)
                be, bea = f * k2 + h * k1, np.abs(f * k2) + np.abs(h * k1)
                bc = f * (2 * k2 + qk3) + h * (k1 + qk2)
                bca = np.abs(f) * (np.abs(2 * k2) + np.abs(qk3)) + np.abs(h) * (np.abs(k1) + np.abs(qk2))
                ba, baa = f * k2a + h * k1a, np.abs(f) * k2aa + np.abs(h) * k1aa
            else:
                if only_same:
                    continue
                f = 2 * c * sd
                be, bea = f * k1, np.abs(f * k1)
                bc, bca = f * (k1 + qk2), np.abs(f) * (np.abs(k1) + np.abs(qk2))
                ba, baa = f * k1a, np.abs(f) * k1aa
                cD += v * 2 * c * f * k2
                cDa += np.abs(v * 2 * c * f * k2)
                cS += (2 if b is None else -2) * v * c * k1
                cSa += np.abs(2 * v * c * k1)
            S[t, 0] += (G * be).sum()
            Sa[t, 0] += (Ga * bea).sum()
            S[t, 1] += (G * bc).sum()
            Sa[t, 1] += (Ga * bca).sum()
            if ns == 3:
                S[t, 2] += (G * ba).sum()
                Sa[t, 2] += (Ga * baa).sum()
        if want_gx:
            for e in range(d):
                xe, ye = xr[:, e, None], yc[None, :, e]
                gx[i0:i1, e] += (G * cD * (xe - ye)).sum(1)
                gxa[i0:i1, e] += (Ga * cDa * (np.abs(xe) + np.abs(ye))).sum(1)
            gx[i0:i1, sel] += (G * cS).sum(1)
            gxa[i0:i1, sel] += (Ga * cSa).sum(1)
    return {"S": (S, Sa), "gradx": None if not want_gx else (gx, gxa)}


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
TABLES = dict(D.TABLES)
#: the table of the large case: fp32 parameters (1 / 0.8 is 1.25 in double), so one reference serves both dtypes
TABLES["eq-exact"] = ([("eq", 1.25, 0.8)], None)
SHAPES = [(64, 64), (65, 63), (1, 130), (129, 65), (200, 1)]
DIMS = [1, 3, 8, 9, 17]
MODES = ["dx", "dy", "dxy-same", "dxy-diff"]


def _dims_of(mode, d, k):
    """The selected dimensions of a mode at the edges of ``d``: 0, ``d - 1`` (8 of 9 and 16 of 17: the first one behind a chunk of
    8) and, for d = 17, 8; ``k`` rotates through them."""
    edges = [0, d - 1] + ([8] if d > 9 else [])
    p = edges[k % len(edges)]
    if mode == "dx":
        return p, None
    if mode == "dy":
        return None, p
    if mode == "dxy-same" or d == 1:
        return p, p
    return p, edges[(k + 1) % len(edges)]


def _case(n, m, d, table, mode, k=0, **flags):
    a, b = _dims_of(mode, d, k)
    name = f"n{n}-m{m}-d{d}-{table}-a{a}-b{b}" + "".join(f"-{f}" for f in sorted(flags))
    return dict(id=name, n=n, m=m, d=d, table=table, a=a, b=b, **flags)


MULTI_TILE_CHUNK = _case(2049, 4100, 2, "eq-exact", "dxy-same", 1)


def _cases():
    cs, seen = [], set()

    def add(c):
        if c["id"] not in seen:
            seen.add(c["id"])
            cs.append(c)

    names = list(D.TABLES)
    # every table in every mode, shapes / dimension counts / selected dimensions rotating; positive and signed cotangents alternate
    i = 0
    for table in names:
        for mode in MODES:
            n, m = SHAPES[i % 5]
            flags = dict(positive=True) if i % 2 else {}
            add(_case(n, m, DIMS[(i + i // 5) % 5], table, mode, i, **flags))
            i += 1
    # every dimension count in every mode with all eight terms, both edges
    for d in DIMS:
        for j, mode in enumerate(MODES):
            for k in (0, 1, 2):
                add(_case(65, 63, d, "all8", mode, k, **(dict(positive=True) if (j + k) % 2 else {})))
    # every shape with all eight terms: the mixed block, and a one-sided block with its input gradient
    for j, (n, m) in enumerate(SHAPES):
        add(_case(n, m, 3, "all8", "dxy-same", j))
        add(_case(n, m, 8, "all8", "dx" if j % 2 else "dy", j, positive=True))
    # coincident points (y is x): matern32 adds exactly 0 there; a cotangent view over NaN padding
    for table in ("matern32", "all8"):
        for j, mode in enumerate(MODES):
            add(_case(64, 64, 3, table, mode, j, y_is_x=True))
    add(_case(65, 63, 9, "all8", "dxy-diff", 0, padded=True))
    add(_case(129, 65, 3, "rq0.7", "dx", 1, padded=True, positive=True))
    add(_case(1, 130, 17, "eq+linear+const", "dy", 1, padded=True))
    add(MULTI_TILE_CHUNK)
    return cs


CASES = _cases()


def make_inputs(case):
    """The inputs of a case: fp64 arrays holding fp32 numbers, points scaled so that q <= 12 for the term of the smallest scale."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    terms, shapes = TABLES[case["table"]]
    n, m, d = case["n"], case["m"], case["d"]
    side = min(t[2] for t in terms) * np.sqrt(12.0 / d)
    x = round32(rng.uniform(-0.5, 0.5, (n, d)) * side)
    y = x if case.get("y_is_x") else round32(rng.uniform(-0.5, 0.5, (m, d)) * side)
    g = round32(rng.uniform(0.5, 1.5, (n, m)) if case.get("positive") else rng.standard_normal((n, m)))
    return dict(terms=terms, shapes=shapes, x=x, y=y, a=case["a"], b=case["b"], g=g)


_CACHE = {}


def reference(case, dtype):
    """``(inputs, reference)`` of a case for a dtype, computed once per process and shared (read-only) by every test that needs it."""
    inp = _CACHE.get(case["id"])
    if inp is None:
        inp = _CACHE[case["id"]] = make_inputs(case)
        for v in inp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    key = (case["id"], None if params_are_fp32(inp["terms"], inp["shapes"]) else dtype)
    if key not in _CACHE:
        ref = diff_vjp(**inp, dtype=key[1])
        for pair in ref.values():
            for arr in pair or ():
                arr.setflags(write=False)
        _CACHE[key] = ref
    return inp, _CACHE[key]


ratios = D.ratios
