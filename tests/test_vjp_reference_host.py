"""The extended-precision reference of the kernel-gradient kernels (``tests/vjp_reference.py``), checked on the host: against the
test-only oracle backend, against central differences of ``kappa``, and -- for every case the GPU module runs -- for discrimination:
a lost tile, partial tile, partial chunk of input dimensions, column of A or term moves at least one output element by more than four
times what the GPU test accepts at the cap of its constant."""
import numpy as np
import pytest
import torch

from stheno_amd import ops

from . import vjp_reference as R
from .conftest import OracleBackend

LD = R.LD
CAP = 50          # the largest constant the GPU module may use (tests/test_vjp_kernels_gpu.py)
FACTOR = 4


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


# ---- cross-check with the oracle backend -------------------------------------------------------------------------------------------
def _close(a, ref, rel=1e-12):
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    assert a.shape == ref.shape
    assert np.all(np.abs(a - ref) <= rel * np.abs(ref)), (a, ref)


NO_SHAPE = [("eq", 1.25, 0.8), ("matern12", 0.75, 1.0), ("matern32", 1.5, 1.6), ("matern52", 0.5, 2.0), ("linear", 0.75, 2.0),
            ("const", 0.25, 1.0)]


@pytest.mark.parametrize("n,C,d", [(7, 1, 2), (70, 3, 9)])
def test_logdensity_reference_agrees_with_the_oracle_backend(n, C, d):
    rng = np.random.default_rng(n)
    x = rng.integers(-64, 65, (n, d)) / 64.0          # the oracle takes its distances from the norm expansion: exact for these
    kinv = R.round32(rng.standard_normal((n, n)) + 4 * np.eye(n))
    alpha = R.round32(rng.standard_normal((n, C)))
    g = rng.integers(1, 9, C) / 8.0
    ref = R.logdensity(NO_SHAPE, x, kinv, alpha, g)
    S, tr, dg = OracleBackend().kmat_vjp(ops.KTerms(NO_SHAPE), _t(x), _t(kinv), _t(alpha), list(g))
    assert np.all(np.abs(S.numpy() - ref["S"][0]) <= 1e-12 * ref["S"][1])
    _close(tr.numpy().reshape(()), ref["trace"][0])
    _close(dg.numpy(), ref["diag"][0])


@pytest.mark.parametrize("n,m,d", [(5, 9, 3), (70, 66, 8)])
def test_dense_reference_agrees_with_the_oracle_backend(n, m, d):
    rng = np.random.default_rng(n + m)
    x, y = R.round32(rng.uniform(-1, 1, (n, d))), R.round32(rng.uniform(-1, 1, (m, d)))
    g, cs = R.round32(rng.uniform(0.5, 1.5, (n, m))), R.round32(rng.uniform(0.5, 2, m))
    w, b = R.round32(rng.uniform(0.5, 1.5, n)), R.round32(rng.uniform(0.5, 1.5, m))
    ref = R.dense(NO_SHAPE, x, y, g, cs, w, b)
    S, colsum, gradx = OracleBackend().kmat_vjp_dense(ops.KTerms(NO_SHAPE), _t(x), _t(y), _t(g), _t(cs), _t(w), _t(b), True, True)
    for got, name in ((S, "S"), (colsum, "colsum"), (gradx, "gradx")):
        assert np.all(np.abs(got.numpy() - ref[name][0]) <= 1e-12 * ref[name][1]), name
    _close(S.numpy()[:, 0], ref["S"][0][:, 0])          # a positive cotangent: kappa sums are free of cancellation
    _close(colsum.numpy(), ref["colsum"][0])


# ---- derivatives ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,alpha", [("eq", None), ("matern12", None), ("matern32", None), ("matern52", None), ("linear", None),
                                        ("const", None), ("rq", 0.4), ("rq", 1.0), ("rq", 9.0)])
def test_kappa_derivatives_agree_with_central_differences(kind, alpha):
    q = np.linspace(LD(0.05), LD(12), 97)
    h = q * LD(1e-6)
    k, dkq, dk, da, _ = R.kappa_all(kind, q, alpha)
    fd = (R.kappa_all(kind, q + h, alpha)[0] - R.kappa_all(kind, q - h, alpha)[0]) / (2 * h)
    assert np.all(np.abs(dk - fd) <= 1e-7 * np.maximum(1, np.abs(fd)))
    assert np.all(np.abs(dkq - fd * q) <= 1e-7 * np.maximum(1, np.abs(fd * q)))
    if kind == "rq":
        ha = LD(alpha) * LD(1e-6)
        fa = (R.kappa_all(kind, q, LD(alpha) + ha)[0] - R.kappa_all(kind, q, LD(alpha) - ha)[0]) / (2 * ha)
        assert np.all(np.abs(da - fa) <= 1e-7 * np.maximum(1, np.abs(fa)))
    else:
        assert not np.any(da)
    assert k.dtype == LD


def test_matern12_slope_is_reported_as_zero_at_zero():
    k, dkq, dk, _, _ = R.kappa_all("matern12", np.zeros(3, dtype=LD))
    assert np.all(k == 1) and not np.any(dkq) and not np.any(dk)


def test_term_parameters_are_fp32_numbers():
    for terms in R.TERMSETS.values():
        for t in terms:
            assert np.float32(t[1]) == t[1] and LD(np.float32(R.ils2_of(t[2]))) == R.ils2_of(t[2])


def test_case_ids_are_unique_and_q_stays_below_twelve():
    cases = R.LOGDENSITY_CASES + R.DENSE_CASES
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        if c["n"] > 300:
            continue
        inp = R.make_inputs(c)
        y = inp.get("y", inp["x"])
        r2 = ((inp["x"][:, None, :] - y[None, :, :]) ** 2).sum(-1).max()
        assert r2 / min(t[2] for t in inp["terms"]) ** 2 <= 12.0 * (1 + 1e-6)


# ---- discrimination ---------------------------------------------------------------------------------------------------------------
def _tile(t):
    return (t * R.TILE, (t + 1) * R.TILE)


def _removals(case):
    """``(name, keyword arguments restricting the reference to the removed contribution)``; ``ndims`` names what is left instead.  A chunk
    of dimensions and a term are lost to the pairs of the last block of rows."""
    n, d = case["n"], case["d"]
    m = case.get("m", n)
    rt, ct = -(-n // R.TILE), -(-m // R.TILE)
    out = []
    if case["form"] == "logdensity":
        if n >= 2 * R.TILE:
            out.append(("tile", dict(rows=_tile(1), cols=_tile(0))))
        elif n >= R.TILE:
            out.append(("tile", dict(rows=_tile(0), cols=_tile(0))))
        if n % R.TILE:
            out.append(("partial tile", dict(rows=_tile(rt - 1), cols=_tile(rt - 1))))
        out.append(("column of A", dict(only_col=case["C"] - 1)))
    else:
        if n >= R.TILE and m >= R.TILE:
            # the second tile of a chunk where chunks hold two, a full tile otherwise
            out.append(("tile", dict(rows=_tile(min(1, n // R.TILE - 1)), cols=_tile(min(1, m // R.TILE - 1)))))
        if n % R.TILE or m % R.TILE:
            out.append(("partial tile", dict(rows=_tile(rt - 1), cols=_tile(ct - 1))))
    last = (max(n - R.BLOCK, 0), n)
    if d % R.DCHUNK:
        out.append(("partial chunk of dimensions", dict(ndims=d - d % R.DCHUNK, rows=last)))
    out.append(("last term", dict(only_term=len(R.TERMSETS[case["terms"]]) - 1, rows=last)))
    return out


def _outputs(case, dtype):
    """The outputs a removal has to show in: all in fp64; in fp32 those whose sums do not cancel."""
    if case["form"] == "logdensity":
        return ("S", "trace", "diag")
    outs = [k for k, on in (("colsum", case["colsum"]), ("gradx", case["gradx"])) if on]
    if dtype == "float64" or case.get("positive"):
        outs.append("S")
    return tuple(outs)


@pytest.mark.parametrize("case", R.LOGDENSITY_CASES + R.DENSE_CASES, ids=lambda c: c["form"] + "-" + c["id"])
def test_a_lost_contribution_moves_an_output_past_the_bound(case):
    inp, full = R.reference(case)
    fn = R.logdensity if case["form"] == "logdensity" else R.dense
    for name, kw in _removals(case):
        part = fn(**inp, **kw)
        if "ndims" in kw:
            whole = fn(**inp, rows=kw["rows"])
            moved = {k: np.abs(whole[k][0] - part[k][0]) for k in full}      # the chunk is lost to the pairs of one block of rows
        else:
            removed = R.difference(full, part)                                # the reference without the contribution
            moved = {k: np.abs(full[k][0] - removed[k]) for k in full}
        for dtype in ("float64", "float32"):
            outs = _outputs(case, dtype)
            if not outs:
                continue
            worst = max(float(np.max(moved[k] / np.where(full[k][1] > 0, full[k][1], np.inf))) for k in outs) / float(R.EPS[dtype])
            assert worst > FACTOR * CAP, (name, dtype, worst)
