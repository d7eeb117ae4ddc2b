"""``Normal.w2``, the 2-Wasserstein distance on the nuclear norm of ``L_o^T L_s`` -- the host logic on the test-only oracle backend,
whose ``nuclear_norm`` (``ops._HostDelta``) is ``numpy.linalg.svd``: an independent formula.  Checked against closed forms and against
the reference's dense formula, the double matrix root by ``numpy.linalg.eigh`` (``stheno/random.py:313-329``), written here."""
import numpy as np
import pytest
import torch

import stheno_amd as st
from stheno_amd import ops

from .conftest import OracleBackend


def sym_root(a):
    w, q = np.linalg.eigh(0.5 * (a + a.T))
    return (q * np.sqrt(np.clip(w, 0.0, None))) @ q.T


def w2_squared_dense(m1, v1, m2, v2):
    """``(W2^2, scale)`` by the reference's formula in fp64: ``|dm|^2 + tr V1 + tr V2 - 2 tr root(root(V1) V2 root(V1))``, and the scale
    ``|dm|^2 + tr V1 + tr V2`` the comparisons are relative to."""
    m1, v1, m2, v2 = (np.asarray(a, dtype=np.float64) for a in (m1, v1, m2, v2))
    r = sym_root(v1)
    scale = float(((m1 - m2) ** 2).sum() + np.trace(v1) + np.trace(v2))
    return scale - 2.0 * float(np.trace(sym_root(r @ v2 @ r))), scale


def kernel_pair(n, noise, seed, d=2):
    """Two kernel-matrix covariances on the same points with different means:
    ``1.3 EQ(0.9) + noise I`` and ``0.8 EQ(1.7) + 0.5 Linear + 2 noise I``; fp64 arrays ``(m1, V1, m2, V2)``."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, (n, d))
    sq = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    v1 = 1.3 * np.exp(-0.5 * sq / 0.9 ** 2) + noise * np.eye(n)
    v2 = 0.8 * np.exp(-0.5 * sq / 1.7 ** 2) + 0.5 * (x @ x.T) + 2.0 * noise * np.eye(n)
    return rng.standard_normal((n, 1)), v1, rng.standard_normal((n, 1)) + 0.3, v2


def normal(m, v, dtype=torch.float64, device="cpu"):
    return st.Normal(torch.as_tensor(m, dtype=dtype, device=device), torch.as_tensor(v, dtype=dtype, device=device))


def test_one_dimension(oracle_backend):
    p, q = normal([[0.7]], [[1.5 ** 2]]), normal([[-0.4]], [[0.6 ** 2]])
    assert abs(float(p.w2(q)) - np.sqrt(1.1 ** 2 + 0.9 ** 2)) < 1e-9
    pd, qd = st.Normal(torch.tensor([[0.7]], dtype=torch.float64), st.Diagonal(torch.tensor([2.25], dtype=torch.float64))), \
        st.Normal(torch.tensor([[-0.4]], dtype=torch.float64), st.Diagonal(torch.tensor([0.36], dtype=torch.float64)))
    assert abs(float(pd.w2(qd)) - np.sqrt(1.1 ** 2 + 0.9 ** 2)) < 1e-12


def test_diagonal_closed_form(oracle_backend):
    rng = np.random.default_rng(0)
    a, b = rng.uniform(0.2, 3.0, 17), rng.uniform(0.2, 3.0, 17)
    m1, m2 = rng.standard_normal((17, 1)), rng.standard_normal((17, 1))
    want = np.sqrt(((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    t = lambda v: torch.as_tensor(v, dtype=torch.float64)      # noqa: E731
    p, q = st.Normal(t(m1), st.Diagonal(t(a))), st.Normal(t(m2), st.Diagonal(t(b)))
    assert abs(float(p.w2(q)) - want) < 1e-12
    q_dense = st.Normal(t(m2), st.Dense(t(np.diag(b))))      # a Diagonal against a Dense diagonal matrix: the factor path
    assert abs(float(p.w2(q_dense)) - want) < 1e-12 * want + 1e-12
    assert abs(float(q_dense.w2(p)) - want) < 1e-12 * want + 1e-12


def test_commuting_covariances(oracle_backend):
    rng = np.random.default_rng(1)
    n = 23
    qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a, b = rng.uniform(0.1, 2.0, n), rng.uniform(0.1, 2.0, n)
    p, q = normal(np.zeros((n, 1)), (qm * a) @ qm.T), normal(np.zeros((n, 1)), (qm * b) @ qm.T)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(float(p.w2(q)) ** 2 - want) < 1e-9 * (a.sum() + b.sum())


@pytest.mark.parametrize("n", [1, 2, 33, 200])
def test_against_the_dense_formula(oracle_backend, n):
    m1, v1, m2, v2 = kernel_pair(n, 0.05, seed=n)
    want, scale = w2_squared_dense(m1, v1, m2, v2)
    got = float(normal(m1, v1).w2(normal(m2, v2))) ** 2
    print(f"w2^2 n={n}: {got:.12e} against {want:.12e}, error {abs(got - want) / scale:.2e} of the scale")
    assert abs(got - want) <= 1e-9 * scale


def test_the_reference_pins_and_symmetry(oracle_backend):
    """``tests/test_random.py:223-225`` of the reference, and ``p.w2(q) == q.w2(p)``."""
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((3, 3)), rng.standard_normal((3, 3))
    p, q = normal(rng.standard_normal((3, 1)), a @ a.T), normal(rng.standard_normal((3, 1)), b @ b.T)
    assert float(p.w2(p)) < 5e-5
    assert float(p.w2(q)) > 0.1
    assert abs(float(p.w2(q)) - float(q.w2(p))) < 1e-10
    m1, v1, m2, v2 = kernel_pair(40, 0.1, seed=5)
    assert abs(float(normal(m1, v1).w2(normal(m2, v2))) - float(normal(m2, v2).w2(normal(m1, v1)))) < 1e-10


def test_batch_equals_unbatched(oracle_backend):
    cases = [kernel_pair(40, 0.1, seed=10 + i) for i in range(3)]
    stack = lambda k: np.stack([c[k] for c in cases])      # noqa: E731
    got = normal(stack(0), stack(1)).w2(normal(stack(2), stack(3)))
    assert tuple(got.shape) == (3,)
    for i, c in enumerate(cases):
        assert abs(float(got[i]) - float(normal(c[0], c[1]).w2(normal(c[2], c[3])))) < 1e-12


def test_fdd_spellings(oracle_backend):
    rng = np.random.default_rng(3)
    x, y = torch.tensor(rng.uniform(-2, 2, (30, 2))), torch.tensor(rng.standard_normal((30, 1)))
    f, g = st.GP(1.3 * st.EQ().stretch(0.9)), st.GP(0.8 * st.EQ().stretch(1.7) + 0.5 * st.Linear())
    xn = x.numpy()
    sq = ((xn[:, None, :] - xn[None, :, :]) ** 2).sum(-1)
    v1 = 1.3 * np.exp(-0.5 * sq / 0.81) + 0.1 * np.eye(30)
    v2 = 0.8 * np.exp(-0.5 * sq / 1.7 ** 2) + 0.5 * (xn @ xn.T) + 0.2 * np.eye(30)
    want, scale = w2_squared_dense(np.zeros((30, 1)), v1, np.zeros((30, 1)), v2)
    assert abs(float(f(x, 0.1).w2(g(x, 0.2))) ** 2 - want) <= 1e-9 * scale
    # a posterior prediction against the prior's, both lazy until asked
    xs = torch.tensor(rng.uniform(-2, 2, (12, 2)))
    post = f | (f(x, 0.1), y)
    d = post(xs, 0.05)
    want, scale = w2_squared_dense(d.mean.numpy(), d.var.mat.numpy(), np.zeros((12, 1)), f(xs, 0.05).var.mat.numpy())
    got = float(post(xs, 0.05).w2(f(xs, 0.05))) ** 2
    assert want > 0.1 and abs(got - want) <= 1e-9 * scale


def sparse_posterior_distances(device="cpu", counts=(5, 10, 20, 40), width=30.0):
    """W2 between the exact posterior's prediction and a pseudo-point posterior's at the same 25 points, for a growing number of
    inducing points on 60 observations.  The points spread over 30 length scales: 40 inducing points are then 0.77 length scales
    apart and their kernel matrix has a condition number of 2e3 -- the pseudo-point posterior itself stays accurate (with 40 points on
    10 length scales that matrix is singular to working precision and the posterior's own moments move by 3e-2 with the rounding)."""
    rng = np.random.default_rng(11)
    x = torch.tensor(np.sort(rng.uniform(0.0, width, 60))[:, None], device=device)
    y = torch.sin(x) + 0.3 * torch.tensor(rng.standard_normal((60, 1)), device=device)
    xs = torch.linspace(0.5, width - 0.5, 25, dtype=torch.float64, device=device)[:, None]
    f = st.GP(st.EQ())
    exact = f | (f(x, 0.09), y)
    out = []
    for m in counts:
        z = torch.linspace(0.0, width, m, dtype=torch.float64, device=device)[:, None]
        sparse = f | st.PseudoObs(f(z), f(x, 0.09), y)
        out.append(float(sparse(xs).w2(exact(xs))))
    return out


def test_sparse_posterior_approaches_the_exact_one(oracle_backend):
    d = sparse_posterior_distances()
    print("w2(sparse, exact) for 5, 10, 20, 40 inducing points:", d)
    assert d[0] > d[1] > d[2] > d[3] >= 0.0
    assert d[0] > 0.1 and d[3] < 1e-2 * d[0]


class _Recording(OracleBackend):
    def __init__(self):
        self.calls = []

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if callable(attr) and not name.startswith("_"):
            object.__getattribute__(self, "calls").append(name)
        return attr


def _learnable_pair(rec):
    rng = np.random.default_rng(4)
    x = torch.tensor(rng.uniform(-2, 2, (15, 2)))
    ls = torch.tensor(0.9, dtype=torch.float64, requires_grad=True)
    prev = ops.set_backend(rec)
    try:
        return st.GP(st.EQ().stretch(ls))(x, 0.1).w2(st.GP(st.EQ())(x, 0.2))
    finally:
        ops.set_backend(prev)


def test_a_learnable_variance_is_refused_before_any_launch():
    rec = _Recording()
    with pytest.raises(NotImplementedError, match="gradients of w2 are not implemented.*cut off from the autograd graph"):
        _learnable_pair(rec)
    assert rec.calls == []
    with torch.no_grad():
        value = _learnable_pair(rec)
    assert value.grad_fn is None and float(value) > 0.1 and "gemm" in rec.calls


def test_tensors_that_require_grad_are_refused(oracle_backend):
    m1, v1, m2, v2 = kernel_pair(6, 0.1, seed=6)
    mean = torch.tensor(m1, requires_grad=True)
    with pytest.raises(NotImplementedError, match="gradients of w2"):
        st.Normal(mean, torch.tensor(v1)).w2(normal(m2, v2))
    var = torch.tensor(v2, requires_grad=True)
    with pytest.raises(NotImplementedError, match="gradients of w2"):
        normal(m1, v1).w2(st.Normal(torch.tensor(m2), var))
    with torch.no_grad():
        assert float(normal(m1, v1).w2(st.Normal(torch.tensor(m2), var))) > 0


def test_mismatched_dimensions(oracle_backend):
    a, b = kernel_pair(5, 0.1, seed=7), kernel_pair(6, 0.1, seed=8)
    with pytest.raises(ValueError):
        normal(a[0], a[1]).w2(normal(b[0], b[1]))
