"""``Observations.append`` on the device: a posterior whose Cholesky factor grows by ``gpk_potrf_border`` is the posterior of a fresh
``Observations`` on all the data, to the project's parity tolerance (README.md, "Correctness": 1e-6 relative in fp64, 1e-3 in fp32).

N = 300, then appends of q = 1, 7 and 140 points (the last: two chunks and one growth of the capacity buffer, the buffers being sized
without spare rows here); D = 2, ``Matern52 + EQ``, noise 0.1, a non-zero mean function."""
import numpy as np
import pytest
import torch

import stheno_amd as st
from stheno_amd import B, matrix

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_backend")]

TOL = {torch.float64: 1e-6, torch.float32: 1e-3}
EPS = {torch.float64: 1e-12, torch.float32: 1e-6}
N, QS, NS = 300, (1, 7, 140), 50


@pytest.fixture()
def tight(request):
    """Buffers without spare rows, and the size rule off: 140 points behind 308 are above the crossover fraction measured at n = 16384."""
    old = matrix.config.append_growth, matrix.config.append_min_rows, matrix.config.append_refactor_fraction, B.epsilon
    matrix.config.append_growth, matrix.config.append_min_rows, matrix.config.append_refactor_fraction = 0.0, 0, None
    yield
    matrix.config.append_growth, matrix.config.append_min_rows, matrix.config.append_refactor_fraction, B.epsilon = old


def rel(a, b):
    a, b = (t.detach().double().cpu().numpy() for t in (a, b))
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _setup(dtype, zero_mean=False, seed=0):
    B.epsilon = EPS[dtype]
    rng = np.random.default_rng(seed)
    total = N + sum(QS) + 12
    x = torch.as_tensor(rng.standard_normal((total, 2)), dtype=dtype, device="cuda")
    y = torch.sin(x.sum(-1, keepdim=True)) + 0.5 + torch.as_tensor(0.1 * rng.standard_normal((total, 1)), dtype=dtype, device="cuda")
    xs = torch.as_tensor(rng.standard_normal((NS, 2)), dtype=dtype, device="cuda")
    kernel = st.Matern52() + 0.6 * st.EQ().stretch(1.3)
    f = st.GP(kernel) if zero_mean else st.GP(lambda t: 0.4 * t[:, :1] - 0.2 * t[:, 1:2] + 0.5, kernel)
    return f, x, y, xs


def _values(f, obs, xs, noise, dense=True):
    post = f.measure | obs
    mean, var = post(f)(xs).marginals()
    cov = B.dense(post(f)(xs).var) if dense else None
    return mean, var, cov


def _agree(f, got_obs, x, y, noise, xs, tol):
    fresh = st.Obs(f(x, noise), y)
    got, want = _values(f, got_obs, xs, noise), _values(f, fresh, xs, noise)
    for g, w in zip(got, want):
        assert rel(g, w) < tol, rel(g, w)
    # the data the appended observations hold are the concatenated data: their density is the fresh one's
    lp, lp_fresh = float(got_obs.fdd.logpdf(got_obs.y)), float(f(x, noise).logpdf(y))
    assert abs(lp - lp_fresh) <= tol * abs(lp_fresh), (lp, lp_fresh)
    assert got_obs.y.shape == y.shape and torch.equal(got_obs.fdd._xr, x)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("zero_mean", [False, True], ids=["mean", "zero-mean"])
def test_three_appends_agree_with_fresh_observations(tight, dtype, zero_mean):
    f, x, y, xs = _setup(dtype, zero_mean)
    tol = TOL[dtype]
    obs = st.Obs(f(x[:N], 0.1), y[:N])
    _values(f, obs, xs, 0.1, dense=False)                # (the factor the appends grow)
    n = N
    for q in QS:
        old_values = _values(f, obs, xs, 0.1)
        new = obs.append(f(x[n : n + q], 0.1), y[n : n + q])
        chol = new._K_x[f.measure]._chol
        assert chol is not None and chol.n == n + q and chol._grow is not None and chol.lookahead_nb == 0 and chol.rows_under == 0
        _agree(f, new, x[: n + q], y[: n + q], 0.1, xs, tol)
        # the old posterior still gives its old values, bit for bit: the shared buffer is not clobbered
        for a, b in zip(_values(f, obs, xs, 0.1), old_values):
            assert torch.equal(a, b)
        obs, n = new, n + q
    assert chol._grow.buf.shape[0] == 512                # 300 -> 384 (first copy), 308 + 140 = 448 -> growth to 512


def test_the_whitened_residual_is_extended_for_a_zero_mean(tight):
    f, x, y, xs = _setup(torch.float64, zero_mean=True)
    obs = st.Obs(f(x[:N], 0.1), y[:N])
    _values(f, obs, xs, 0.1, dense=False)
    new = obs.append(f(x[N : N + 7], 0.1), y[N : N + 7])
    chol = new._K_x[f.measure]._chol
    w = chol._remembered(new.y)
    assert w is not None and tuple(w.shape) == (N + 7, 1)
    want = chol.solve(new.y)
    assert rel(w, want) < 1e-10


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_a_branch_two_appends_from_one_observations(tight, dtype):
    f, x, y, xs = _setup(dtype)
    tol = TOL[dtype]
    obs = st.Obs(f(x[:N], 0.1), y[:N])
    _values(f, obs, xs, 0.1, dense=False)
    first = obs.append(f(x[N : N + 7], 0.1), y[N : N + 7])
    a = first.append(f(x[N + 7 : N + 12], 0.1), y[N + 7 : N + 12])          # in place behind `first`
    b = first.append(f(x[N + 20 : N + 29], 0.1), y[N + 20 : N + 29])        # a second continuation of `first`
    assert a._K_x[f.measure]._chol._grow is first._K_x[f.measure]._chol._grow
    assert b._K_x[f.measure]._chol._grow is not first._K_x[f.measure]._chol._grow
    idx_b = torch.cat([torch.arange(N + 7), torch.arange(N + 20, N + 29)]).to("cuda")
    _agree(f, a, x[: N + 12], y[: N + 12], 0.1, xs, tol)
    _agree(f, b, x[idx_b], y[idx_b], 0.1, xs, tol)
    _agree(f, first, x[: N + 7], y[: N + 7], 0.1, xs, tol)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_vector_noise_and_a_missing_value(tight, dtype):
    f, x, y, xs = _setup(dtype)
    tol = TOL[dtype]
    n, q = N, 9
    noise = torch.linspace(0.05, 0.2, n + q, dtype=dtype, device="cuda")
    obs = st.Obs(f(x[:n], noise[:n]), y[:n])
    _values(f, obs, xs, None, dense=False)
    y_new = y[n : n + q].clone()
    y_new[4, 0] = float("nan")
    new = obs.append(f(x[n : n + q], noise[n:]), y_new)
    keep = torch.tensor([i for i in range(n + q) if i != n + 4], device="cuda")
    assert new._K_x[f.measure]._chol.n == n + q - 1
    _agree(f, new, x[keep], y[keep], noise[keep], xs, tol)


def test_deferred_checks_report_an_append_that_is_not_positive_definite(tight):
    f, x, y, xs = _setup(torch.float64, zero_mean=True)
    obs = st.Obs(f(x[:N], 0.1), y[:N])
    _values(f, obs, xs, 0.1, dense=False)
    chol = obs._K_x[f.measure]._chol
    kern = f.measure.kernels[f]
    k12 = kern.pairwise(x[:N], x[N : N + 6])
    k22 = kern.pairwise(x[N : N + 6]) + 0.1 * torch.eye(6, dtype=torch.float64, device="cuda")
    k22[3, 3] = 1e-3                                    # (far below what the rows before it explain of it)
    with pytest.raises(torch.linalg.LinAlgError, match=f"order {N + 4} "):
        with matrix.deferred_checks():
            chol.append(k12, k22)
    with pytest.raises(torch.linalg.LinAlgError, match=f"order {N + 4} "):
        chol.append(k12, k22)
    # the factor that was appended to is as good as before
    mean, _, _ = _values(f, obs, xs, 0.1, dense=False)
    assert rel(mean, _values(f, st.Obs(f(x[:N], 0.1), y[:N]), xs, 0.1, dense=False)[0]) < 1e-9
