"""``Observations.append`` / ``Chol.append`` on the CPU: the host logic of the growing Cholesky factor.

The backend is the tests' ``OracleBackend`` plus ``potrf_border`` in NumPy (``longdouble``), written from the contract of
``gpk_potrf_border`` in ``include/gpk.h``; it records its calls, so the tests can say which path ran: an admissible append borders the
factor and builds no N x N kernel matrix, everything else returns the plain, lazy, differentiable ``Observations`` on the concatenated
data."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import matrix, ops
from stheno_amd.torch import EQ, Matern52

from .conftest import OracleBackend


class BorderBackend(OracleBackend):
    """``OracleBackend`` with ``potrf_border`` and a record of what was called."""

    def __init__(self):
        self.border, self.kmat_shapes, self.potrf = [], [], 0

    def kmat(self, terms, x, y=None, **kw):
        out = OracleBackend.kmat(self, terms, x, y, **kw)
        self.kmat_shapes.append(tuple(out.shape))
        return out

    def potrf_(self, a, nbo=0, rhs=None):
        self.potrf += 1
        return OracleBackend.potrf_(self, a, nbo, rhs)

    def potrf_rows_(self, a, **kw):
        self.potrf += 1
        return OracleBackend.potrf_rows_(self, a, **kw)

    def potrf_border(self, a_buf, n, q, v, dinv, w1=None, r2=None):
        assert 1 <= q <= 128 and n >= 1 and tuple(v.shape) == (n, q) and min(a_buf.shape) >= n + q
        assert (w1 is None) == (r2 is None)
        self.border.append((n, q, a_buf.data_ptr()))
        ld = np.longdouble
        V = v.detach().numpy().astype(ld)
        k22 = a_buf[n : n + q, n : n + q].detach().numpy().astype(ld)
        S = np.tril(k22) + np.tril(k22, -1).T - V.T @ V
        L = np.zeros((q, q), dtype=ld)
        info = torch.zeros((1,), dtype=torch.int32)
        for j in range(q):
            d = S[j, j] - L[j, :j] @ L[j, :j]
            if not d > 0:
                info[0] = n + j + 1
                return info
            L[j, j] = np.sqrt(d)
            L[j + 1 :, j] = (S[j + 1 :, j] - L[j + 1 :, :j] @ L[j, :j]) / L[j, j]
        a_buf[n : n + q, :n] = torch.as_tensor(V.T.astype(np.float64), dtype=a_buf.dtype)
        low = torch.as_tensor(L.astype(np.float64), dtype=a_buf.dtype)
        blk = a_buf[n : n + q, n : n + q]
        blk.copy_(torch.tril(low) + torch.triu(blk, 1))
        if r2 is not None:
            t = r2.detach().numpy().astype(ld).reshape(-1) - V.T @ w1.detach().numpy().astype(ld).reshape(-1)
            for j in range(q):
                t[j] = (t[j] - L[j, :j] @ t[:j]) / L[j, j]
            r2.copy_(torch.as_tensor(t.astype(np.float64), dtype=r2.dtype).reshape(r2.shape))
        return info


@pytest.fixture()
def border_backend():
    be = BorderBackend()
    prev = ops.set_backend(be)
    yield be
    ops.set_backend(prev)


@pytest.fixture(autouse=True)
def no_size_limit():
    """The sizes here are far below the ones the refactorisation crossover was measured at: the size rule is off, except in its own test."""
    old = matrix.config.append_refactor_fraction
    matrix.config.append_refactor_fraction = None
    yield
    matrix.config.append_refactor_fraction = old


@pytest.fixture()
def tight_buffers():
    """No spare capacity: every buffer is the next multiple of 128, so small cases reach the growth branch."""
    old = matrix.config.append_growth, matrix.config.append_min_rows
    matrix.config.append_growth, matrix.config.append_min_rows = 0.0, 0
    yield
    matrix.config.append_growth, matrix.config.append_min_rows = old


def _data(n, d=2, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.as_tensor(0.8 * rng.standard_normal((n, d)))
    y = torch.as_tensor(np.sin(x.numpy().sum(-1, keepdims=True)) + 0.1 * rng.standard_normal((n, 1)))
    return x, y


def _model(mean=True):
    f = st.GP(lambda x: 0.3 * x[:, :1] + 0.5, Matern52() + 0.7 * EQ().stretch(1.5)) if mean else st.GP(Matern52() + 0.7 * EQ().stretch(1.5))
    return f


def _predict(f, obs, xs):
    post = f.measure | obs
    mean, var = post(f)(xs).marginals()
    return mean, var


def _close(a, b, rel=1e-9):
    a, b = a.detach(), b.detach()
    assert float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300), (float((a - b).abs().max()), float(b.abs().max()))


def _grown(obs, f):
    """The factor ``obs`` holds for ``f``'s measure, or None."""
    K = obs._K_x.get(f.measure)
    return None if K is None else K._chol


def test_append_borders_the_factor_and_builds_no_square_kernel_matrix(border_backend):
    n, q = 150, 7
    f = _model()
    x, y = _data(n + q)
    xs = _data(20, seed=1)[0]
    obs = st.Obs(f(x[:n], 0.1), y[:n])
    _predict(f, obs, xs)                              # (factorises K_x under the prior measure)
    border_backend.kmat_shapes.clear()
    before = border_backend.potrf
    obs2 = obs.append(f(x[n:], 0.1), y[n:])
    assert [(c[0], c[1]) for c in border_backend.border] == [(n, q)]
    assert border_backend.potrf == before
    assert sorted(set(border_backend.kmat_shapes)) == [(q, q), (n, q)]
    assert _grown(obs2, f) is not None and _grown(obs2, f).n == n + q
    border_backend.kmat_shapes.clear()
    got = _predict(f, obs2, xs)
    assert border_backend.potrf == before             # (the prediction solves against the grown factor)
    assert (n + q, n + q) not in border_backend.kmat_shapes
    want = _predict(f, st.Obs(f(x, 0.1), y), xs)
    _close(got[0], want[0])
    _close(got[1], want[1])
    assert isinstance(obs2, st.Obs) and obs2.y.shape == (n + q, 1) and obs2.fdd._xr.shape == (n + q, 2)


def test_vector_noise_missing_values_and_no_noise(border_backend):
    n, q = 90, 6
    f = _model()
    x, y = _data(n + q, seed=3)
    xs = _data(15, seed=4)[0]
    noise = torch.as_tensor(np.linspace(0.05, 0.2, n + q))
    y_new = y[n:].clone()
    y_new[2, 0] = float("nan")
    keep = torch.tensor([i for i in range(n + q) if i != n + 2])
    obs = st.Obs(f(x[:n], noise[:n]), y[:n])
    _predict(f, obs, xs)
    obs2 = obs.append(f(x[n:], noise[n:]), y_new)
    assert [(c[0], c[1]) for c in border_backend.border] == [(n, q - 1)]
    got = _predict(f, obs2, xs)
    want = _predict(f, st.Obs(f(x[keep], noise[keep]), y[keep]), xs)
    _close(got[0], want[0])
    _close(got[1], want[1])
    # scalar noise behind vector noise
    obs3 = obs.append(f(x[n:], 0.3), y[n:])
    got = _predict(f, obs3, xs)
    want = _predict(f, st.Obs(f(x, torch.cat([noise[:n], torch.full((q,), 0.3, dtype=torch.float64)])), y), xs)
    _close(got[0], want[0])
    _close(got[1], want[1])


def test_three_hundred_points_are_two_full_chunks_and_one_of_44(border_backend):
    n, q = 100, 300
    f = _model(mean=False)
    x, y = _data(n + q, seed=5)
    xs = _data(10, seed=6)[0]
    obs = st.Obs(f(x[:n], 0.1), y[:n])
    _predict(f, obs, xs)
    obs2 = obs.append(f(x[n:], 0.1), y[n:])
    assert [(c[0], c[1]) for c in border_backend.border] == [(100, 128), (228, 128), (356, 44)]
    got = _predict(f, obs2, xs)
    want = _predict(f, st.Obs(f(x, 0.1), y), xs)
    _close(got[0], want[0])
    _close(got[1], want[1])


def _fallback_case(name, n=40, q=5):
    """(prior measure's process, obs, (fdd_new, y_new), fresh observations on everything, logpdf of everything) per case."""
    x, y = _data(n + q, seed=7)
    if name == "learnable":
        var = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
        f = st.GP(var * EQ())
        return f, st.Obs(f(x[:n], 0.1), y[:n]), (f(x[n:], 0.1), y[n:]), lambda: f(x, 0.1).logpdf(y)
    f = _model(mean=False)
    if name == "batch":
        xb, yb = torch.stack([x, x + 0.1]), torch.stack([y, y * 0.5])
        return f, st.Obs(f(xb[:, :n], 0.1), yb[:, :n]), (f(xb[:, n:], 0.1), yb[:, n:]), None
    if name == "dense noise":
        nz = torch.eye(q, dtype=torch.float64) * 0.1 + 0.01
        return f, st.Obs(f(x[:n], 0.1), y[:n]), (f(x[n:], nz), y[n:]), None
    if name == "another process":
        g = st.GP(EQ(), measure=f.measure)
        return f, st.Obs(f(x[:n], 0.1), y[:n]), (g(x[n:], 0.1), y[n:]), None
    if name == "pseudo":
        return f, st.PseudoObs(f(x[:8]), f(x[:n], 0.1), y[:n]), (f(x[n:], 0.1), y[n:]), None
    raise KeyError(name)


@pytest.mark.parametrize("name", ["learnable", "batch", "dense noise", "another process", "pseudo"])
def test_inadmissible_appends_take_the_plain_observations(border_backend, name):
    f, obs, (fdd_new, y_new), logpdf = _fallback_case(name)
    xs = _data(6, seed=8)[0]
    if name == "batch":
        xs = torch.stack([xs, xs])
    if name == "learnable":
        with torch.no_grad():
            _predict(f, obs, xs)                      # (a factor is there to be grown -- and must not be)
    elif name != "pseudo":
        _predict(f, obs, xs)
    obs2 = obs.append(fdd_new, y_new)
    assert border_backend.border == []
    assert type(obs2) is type(obs)
    n_all = obs.y.shape[-2] + y_new.shape[-2]
    assert obs2.y.shape[-2] == n_all
    if name == "another process":
        mean, _ = (f.measure | obs2)(f)(xs).marginals()
        want, _ = (f.measure | st.Obs((obs.fdd, obs.y), (fdd_new, y_new)))(f)(xs).marginals()
        _close(mean, want)
    if logpdf is not None:
        # the learnable model is not cut off from its graph: the density of the appended observations' data has a gradient where the
        # fresh one has
        lp = obs2.fdd.logpdf(obs2.y)
        assert lp.requires_grad == logpdf().requires_grad and lp.requires_grad
        _close(lp, logpdf())


def test_backend_without_potrf_border_takes_the_plain_observations(oracle_backend):
    n, q = 60, 4
    f = _model()
    x, y = _data(n + q, seed=9)
    xs = _data(8, seed=10)[0]
    obs = st.Obs(f(x[:n], 0.1), y[:n])
    _predict(f, obs, xs)
    obs2 = obs.append(f(x[n:], 0.1), y[n:])
    assert _grown(obs2, f) is None
    got, want = _predict(f, obs2, xs), _predict(f, st.Obs(f(x, 0.1), y), xs)
    _close(got[0], want[0])
    _close(got[1], want[1])


def test_an_append_above_the_crossover_fraction_takes_the_plain_observations(border_backend):
    n = 64
    f = _model()
    x, y = _data(n + 10, seed=20)
    xs = _data(8, seed=21)[0]
    obs = st.Obs(f(x[:n], 0.1), y[:n])
    _predict(f, obs, xs)
    matrix.config.append_refactor_fraction = 1.0 / 16.0
    small = obs.append(f(x[n : n + 4], 0.1), y[n : n + 4])          # 4 <= 64 / 16: grown
    assert [(c[0], c[1]) for c in border_backend.border] == [(n, 4)] and _grown(small, f) is not None
    large = obs.append(f(x[n : n + 5], 0.1), y[n : n + 5])          # 5 > 64 / 16: the plain observations
    assert len(border_backend.border) == 1 and _grown(large, f) is None
    got, want = _predict(f, large, xs), _predict(f, st.Obs(f(x[: n + 5], 0.1), y[: n + 5]), xs)
    _close(got[0], want[0])
    _close(got[1], want[1])


def test_the_border_test_matrices_leave_room_under_the_derived_cap():
    """The matrices of tests/test_potrf_border_gpu.py, factorised by LAPACK in fp64 here: rho of the new rows (|A - L L^T| over
    eps |L| |L|^T, in longdouble) stays far under n + q + 1, the cap no bound of that test may exceed -- so the inputs leave room."""
    from .test_potrf_border_gpu import SHAPES, _bordered, _rho

    eps = float(np.finfo(np.float64).eps)
    for n, q in SHAPES:
        if n > 1000:
            continue                                  # (the n = 4133 case is left to the GPU run: its longdouble products take the host too long)
        a, _ = _bordered(n, q)
        l = np.linalg.cholesky(a)
        rho = _rho(a, l.astype(np.longdouble), np.arange(n, n + q), eps)
        assert rho < 0.25 * (n + q + 1) and rho < 32, (n, q, rho)


def test_a_measure_without_a_factor_triggers_nothing(border_backend):
    n, q = 50, 3
    f = _model()
    x, y = _data(n + q, seed=11)
    obs = st.Obs(f(x[:n], 0.1), y[:n])
    before = list(border_backend.kmat_shapes)
    obs2 = obs.append(f(x[n:], 0.1), y[n:])
    assert border_backend.border == [] and border_backend.potrf == 0 and border_backend.kmat_shapes == before
    assert len(obs2._K_x) == 0 and obs2.y.shape == (n + q, 1)


def test_buffer_ownership_in_place_branch_and_growth(border_backend, tight_buffers):
    n = 100
    f = _model(mean=False)
    x, y = _data(n + 40, seed=12)
    xs = _data(9, seed=13)[0]
    obs = st.Obs(f(x[:n], 0.1), y[:n])
    _predict(f, obs, xs)
    c0 = _grown(obs, f)
    a = obs.append(f(x[n : n + 5], 0.1), y[n : n + 5])                # first append: a copy into a capacity buffer (128 rows)
    ca = _grown(a, f)
    assert ca._grow is not None and ca._grow.buf.shape == (128, 128) and ca._grow.filled == n + 5
    assert c0._grow is None and ca.l.data_ptr() == ca._grow.buf.data_ptr()
    b = a.append(f(x[n + 5 : n + 12], 0.1), y[n + 5 : n + 12])        # fits: in place
    cb = _grown(b, f)
    assert cb._grow is ca._grow and cb._grow.filled == n + 12 and cb.l.data_ptr() == ca.l.data_ptr()
    old = _predict(f, a, xs)
    c = a.append(f(x[n + 20 : n + 26], 0.1), y[n + 20 : n + 26])      # a second continuation of `a`: a branch, its own buffer
    cc = _grown(c, f)
    assert cc._grow is not ca._grow and cc.l.data_ptr() != ca.l.data_ptr()
    d = b.append(f(x[n + 12 :], 0.1), y[n + 12 :])                    # 112 + 28 rows do not fit into 128: growth, a copy
    cd = _grown(d, f)
    assert cd._grow is not cb._grow and cd._grow.buf.shape == (256, 256) and cd.n == n + 40
    assert [q for _, q, _ in border_backend.border] == [5, 7, 6, 28]
    # nobody's values moved: `a` after two continuations, the branch, the chain
    again = _predict(f, a, xs)
    assert torch.equal(old[0], again[0]) and torch.equal(old[1], again[1])
    keep = torch.cat([torch.arange(n + 5), torch.arange(n + 20, n + 26)])
    for got_obs, idx in ((c, keep), (d, torch.arange(n + 40)), (b, torch.arange(n + 12))):
        got, want = _predict(f, got_obs, xs), _predict(f, st.Obs(f(x[idx], 0.1), y[idx]), xs)
        _close(got[0], want[0])
        _close(got[1], want[1])


def test_append_to_an_empty_first_set_is_the_new_observations(border_backend):
    f = _model()
    x, y = _data(12, seed=14)
    xs = _data(5, seed=15)[0]
    empty = st.Obs(f(x[:0], 0.1), y[:0])
    obs = empty.append(f(x, 0.1), y)
    assert border_backend.border == []
    got, want = _predict(f, obs, xs), _predict(f, st.Obs(f(x, 0.1), y), xs)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_a_non_positive_pivot_is_reported_with_its_order_in_the_grown_matrix(border_backend):
    n = 30
    f = _model(mean=False)
    x, y = _data(n + 4, seed=16)
    xs = _data(5, seed=17)[0]
    obs = st.Obs(f(x[:n], 0.1), y[:n])
    _predict(f, obs, xs)
    chol = _grown(obs, f)
    kern = f.measure.kernels[f]
    k12 = kern.pairwise(x[:n], x[n:])
    k22 = kern.pairwise(x[n:]) + 0.1 * torch.eye(4, dtype=torch.float64)
    k22[2, 2] = 1e-3                                   # (far below what the first 32 rows explain of it)
    with pytest.raises(torch.linalg.LinAlgError, match=f"order {n + 3} "):
        chol.append(k12, k22)
    with pytest.raises(torch.linalg.LinAlgError, match=f"order {n + 3} "):
        with matrix.deferred_checks():
            bad = chol.append(k12, k22)                # (nothing raised here)
            assert bad.n == n + 4
