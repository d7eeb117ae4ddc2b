"""The VJP of a derivative block on the host: the closed forms of ``include/gpk.h`` (gpk_kmat_diff_vjp) as ``tests/diff_vjp_reference.py``
evaluates them against torch's double backward, ``_HostDelta.kmat_diff_vjp`` against that reference, the discrimination of every case
the GPU module runs, and the argument codes of the entry point (checked before anything is launched: no GPU needed, but the built
library)."""
import ctypes

import numpy as np
import pytest
import torch

from stheno_amd import _native, autograd, ops

from . import diff_reference as D
from . import diff_vjp_reference as R

LD = R.LD
CAP = 50          # the largest constant the GPU module may use (tests/test_diff_vjp_gpu.py)
FACTOR = 4
MODES = [("dx", 1, None), ("dy", None, 0), ("dxy-same", 1, 1), ("dxy-diff", 0, 1)]
TORCH_TABLES = dict(D.TABLES, matern52=([("matern52", 0.75, 1.5)], None), linear_eq=([("linear", 0.25, 4.0), ("eq", 1.0, 1.0)], None))


# ---- the closed forms against torch ------------------------------------------------------------------------------------------------
def _torch_grads(terms, shapes, x, y, a, b, g):
    """Gradients of ``sum(g * block)`` by autograd, the block itself by autograd of ``D.torch_kernel`` on one pair per row: with respect
    to the variances, scales, alphas (``None`` where unused) and ``x``."""
    n, m, d = x.shape[0], y.shape[0], x.shape[1]
    t64 = lambda v: torch.tensor(float(v), dtype=torch.float64, requires_grad=True)      # noqa: E731
    vs, ls = [t64(v) for _, v, _ in terms], [t64(s) for _, _, s in terms]
    als = [None if al is None else t64(al) for al in (shapes or [None] * len(terms))]
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    xe = xt[:, None, :].expand(n, m, d).reshape(n * m, d)
    ye = torch.tensor(y, dtype=torch.float64)[None, :, :].expand(n, m, d).reshape(n * m, d).clone().requires_grad_(True)
    k = torch.diagonal(D.torch_kernel([(kd, v, s) for (kd, _, _), v, s in zip(terms, vs, ls)], als, xe, ye))
    if a is not None:
        blk = torch.autograd.grad(k.sum(), xe, create_graph=True)[0][:, a]
        if b is not None:
            got = torch.autograd.grad(blk.sum(), ye, create_graph=True, allow_unused=True)[0]
            blk = got[:, b] if got is not None else None
    else:
        blk = torch.autograd.grad(k.sum(), ye, create_graph=True)[0][:, b]
    leaves = vs + ls + [al for al in als if al is not None] + [xt]
    if blk is None or not blk.requires_grad:
        grads = [None] * len(leaves)
    else:
        loss = (torch.tensor(g, dtype=torch.float64).reshape(-1) * blk).sum()
        grads = list(torch.autograd.grad(loss, leaves, allow_unused=True))
    num = lambda t: 0.0 if t is None else t.detach().numpy()      # noqa: E731
    nt = len(terms)
    ga, rest = [], grads[2 * nt:-1]
    for al in als:
        ga.append(None if al is None else num(rest.pop(0)))
    return [num(t) for t in grads[:nt]], [num(t) for t in grads[nt:2 * nt]], ga, num(grads[-1])


def _close(got, want, scale):
    assert np.all(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) <= 1e-9 * scale), (got, want)


@pytest.mark.parametrize("mode,a,b", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("table", list(TORCH_TABLES))
def test_closed_forms_agree_with_torch_double_backward(table, mode, a, b):
    terms, shapes = TORCH_TABLES[table]
    rng = np.random.default_rng(len(table) + 7 * len(mode))
    n, m, d = 6, 5, 3
    x, y = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (m, d))
    g = rng.standard_normal((n, m))
    ref = R.diff_vjp(terms, shapes, x, y, a, b, g)
    S, Sa = (np.asarray(v, dtype=np.float64) for v in ref["S"])
    kinds = tuple(k for k, _, _ in terms)
    values = ([v for _, v, _ in terms], [s for _, _, s in terms], None if shapes is None else [al or 0.0 for al in shapes])
    meta = [(torch.device("cpu"), torch.float64)] * (len(terms) * (2 if shapes is None else 3))
    mine = autograd._param_grads(kinds, values, torch.as_tensor(S), meta)
    nt = len(terms)
    gv, gl, ga, gxt = _torch_grads(terms, shapes, x, y, a, b, g)
    # relative to the gradient itself; a gradient that is an exact zero (const, linear off the diagonal) has to come out as one
    for t in range(nt):
        _close(float(mine[t]), gv[t], abs(gv[t]))
        _close(float(mine[nt + t]), gl[t], abs(gl[t]))
        if ga[t] is not None:
            _close(float(mine[2 * nt + t]), ga[t], abs(ga[t]))
        elif shapes is not None:
            assert mine[2 * nt + t] is None and S[t, 2] == 0
    if a is None or b is None:
        gx = np.asarray(ref["gradx"][0], dtype=np.float64)
        _close(gx, gxt, np.max(np.abs(gxt)))
    else:
        assert ref["gradx"] is None
    assert np.all(Sa >= np.abs(S))


# ---- the NumPy backend ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.CASES if c is not R.MULTI_TILE_CHUNK], ids=lambda c: c["id"])
def test_host_backend_agrees_with_the_reference(case):
    inp, ref = R.reference(case, "float64")
    t = lambda v: torch.as_tensor(np.array(v), dtype=torch.float64)      # noqa: E731
    want_gx = ref["gradx"] is not None
    S, gx = ops._HostDelta(None).kmat_diff_vjp(ops.KTerms(inp["terms"], inp["shapes"]), t(inp["x"]), t(inp["y"]), inp["a"], inp["b"],
                                               t(inp["g"]), want_gradx=want_gx)
    assert float(np.max(R.ratios(S.numpy(), *ref["S"], "float64"))) <= CAP
    if want_gx:
        assert float(np.max(R.ratios(gx.numpy(), *ref["gradx"], "float64"))) <= CAP
    else:
        assert gx is None
        with pytest.raises(RuntimeError, match="gpk_kmat_diff_vjp"):
            ops._HostDelta(None).kmat_diff_vjp(ops.KTerms(inp["terms"], inp["shapes"]), t(inp["x"]), t(inp["y"]), inp["a"], inp["b"],
                                               t(inp["g"]), want_gradx=True)


# ---- cases and discrimination ------------------------------------------------------------------------------------------------------
def test_cases_cover_what_they_are_meant_to():
    cs = R.CASES
    assert len({c["id"] for c in cs}) == len(cs)
    assert {(c["n"], c["m"]) for c in cs} >= set(R.SHAPES) and {c["d"] for c in cs} >= set(R.DIMS)
    assert {c["table"] for c in cs} >= set(D.TABLES)
    for d in R.DIMS:      # both edges of every dimension count in every mode
        sel = [(c["a"], c["b"]) for c in cs if c["d"] == d]
        assert {(0, None), (d - 1, None), (None, 0), (None, d - 1), (0, 0), (d - 1, d - 1)} <= set(sel)
        if d > 1:
            assert any(a is not None and b is not None and a != b for a, b in sel)
    assert (8, None) in [(c["a"], c["b"]) for c in cs if c["d"] == 9] and (16, 16) in [(c["a"], c["b"]) for c in cs if c["d"] == 17]
    assert any(c.get("y_is_x") for c in cs) and any(c.get("padded") for c in cs) and any(c.get("positive") for c in cs)
    for c in cs:
        inp = R.make_inputs(c)
        if c["n"] * c["m"] <= 1 << 16:
            r2 = ((inp["x"][:, None, :] - inp["y"][None, :, :]) ** 2).sum(-1).max()
            assert r2 / min(t[2] for t in inp["terms"]) ** 2 <= 12.0 * (1 + 1e-6)
        assert np.array_equal(R.round32(inp["x"]), inp["x"]) and np.array_equal(R.round32(inp["g"]), inp["g"])
    assert R.params_are_fp32(*R.TABLES["eq-exact"])


def test_matern32_adds_exactly_zero_at_coincident_points():
    terms, shapes = D.M32
    x = R.round32(np.random.default_rng(3).uniform(-1, 1, (9, 3)))
    g = np.ones((9, 9))
    for a, b in ((1, None), (None, 2), (1, 1), (0, 2)):
        ref = R.diff_vjp(terms, shapes, x, x, a, b, g)
        off = R.diff_vjp(terms, shapes, x, x, a, b, g * (1 - np.eye(9)))
        if a == b:      # (the diagonal of the mixed block is -2 c kappa'(0): not zero, but free of the singular factor)
            assert np.all(np.isfinite(np.asarray(ref["S"][0], dtype=np.float64)))
        else:
            assert np.array_equal(ref["S"][0], off["S"][0])
        if ref["gradx"] is not None:
            assert np.all(np.isfinite(np.asarray(ref["gradx"][0], dtype=np.float64)))


def _tile(t):
    return (t * R.TILE, (t + 1) * R.TILE)


def _removals(case, terms):
    n, m, d, a, b = case["n"], case["m"], case["d"], case["a"], case["b"]
    rt, ct = -(-n // R.TILE), -(-m // R.TILE)
    out = []
    if n >= R.TILE and m >= R.TILE:
        out.append(("last full tile", dict(rows=_tile(n // R.TILE - 1), cols=_tile(m // R.TILE - 1))))
    if n % R.TILE or m % R.TILE:
        out.append(("partial tile", dict(rows=_tile(rt - 1), cols=_tile(ct - 1))))
    last = (max(n - R.BLOCK, 0), n)
    out.append(("last chunk of dimensions", dict(ndims=d - (d % R.DCHUNK or R.DCHUNK), rows=last)))
    # the last term that adds anything: const never does, linear not off the diagonal of the mixed block
    dead = ("const", "linear") if (a is not None and b is not None and a != b) else ("const",)
    out.append(("term", dict(only_term=max(t for t, row in enumerate(terms) if row[0] not in dead), rows=last)))
    if a is not None and a == b:
        out.append(("[a == b] addend", dict(only_same=True, rows=last)))
    return out


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_a_lost_contribution_moves_an_output_past_the_bound(case):
    for dtype in ("float64", "float32"):
        inp, full = R.reference(case, dtype)
        dt = None if R.params_are_fp32(inp["terms"], inp["shapes"]) else dtype
        outs = ["gradx"] if full["gradx"] is not None else []
        if dtype == "float64" or case.get("positive"):
            outs.append("S")
        if not outs:
            continue
        for name, kw in _removals(case, inp["terms"]):
            part = R.diff_vjp(**inp, dtype=dt, **kw)
            if "ndims" in kw:
                whole = R.diff_vjp(**inp, dtype=dt, rows=kw["rows"])
                moved = {k: np.abs(whole[k][0] - part[k][0]) for k in outs}      # the chunk is lost to the pairs of one block of rows
            else:
                moved = {k: np.abs(part[k][0]) for k in outs}                     # by linearity: what the contribution added
            worst = max(float(np.max(moved[k] / np.where(full[k][1] > 0, full[k][1], np.inf))) for k in outs) / float(R.EPS[dtype])
            assert worst > FACTOR * CAP, (name, dtype, worst)


# ---- the entry point's argument checks (nothing is launched) -----------------------------------------------------------------------
def test_version_and_argument_codes():
    lib = _native.load()
    assert lib.gpk_version() >= 106
    EQ, M12, RQ, DELTA = (ops._KIND_IDS[k] for k in ("eq", "matern12", "rq", "delta"))
    one = (ctypes.c_double * 8)(*([1.0] * 8))
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(buf, ctypes.c_void_p)

    def call(kinds=(EQ,), shapes=None, nterms=None, dim_x=0, dim_y=-1, n=0, m=0, d=3, gradx=None, dtype=_native.GPK_F64):
        ks = (ctypes.c_int * 9)(*(list(kinds) + [EQ] * (9 - len(kinds))))
        sh = None if shapes is None else (ctypes.c_double * 8)(*(list(shapes) + [1.0] * (8 - len(shapes))))
        return lib.gpk_kmat_diff_vjp(dtype, ks, one, one, sh, len(kinds) if nterms is None else nterms, dim_x, dim_y, ptr, n, d, ptr, m, d, d,
                                     ptr, max(m, 1), ptr, gradx, None)

    # every argument is checked before the empty problem (n = m = 0) returns 0
    assert call() == 0 and call(dim_x=-1, dim_y=2) == 0 and call(dim_x=2, dim_y=0) == 0 and call(gradx=ptr, d=8) == 0
    assert call(kinds=(RQ, EQ), shapes=(0.7,)) == 0
    assert call(nterms=9) == -6 and call(nterms=-1) == -6
    assert call(kinds=(EQ, M12)) == -2 and call(kinds=(DELTA,), shapes=(1e-6,)) == -2 and call(kinds=(99,)) == -2
    assert call(kinds=(RQ,)) == -1 and call(kinds=(EQ, RQ), shapes=(1.0, 0.0)) == -5
    assert call(d=-1) == -15
    assert call(dim_x=3) == -7 and call(dim_x=-2) == -7 and call(dim_x=-1, dim_y=-1) == -7
    assert call(dim_y=3) == -8 and call(dim_y=-2) == -8
    assert call(n=1 << 31) == -10 and call(m=1 << 31) == -13
    assert call(gradx=ptr, dim_x=0, dim_y=0) == -19 and call(gradx=ptr, d=9) == -19
    assert call(dtype=7) == -1
