"""Gradients through the JOINT posterior covariance of an exact posterior (``post(xs).var``, ``.sample()``, ``.entropy()``;
``autograd._PosteriorCovariance`` and the differentiable factorisation / log-determinant behind ``Normal``) -- the host logic on the
test-only oracle backend with the transposed solve of ``test_posterior_grad_host.py``, the Cholesky VJP in NumPy from
``ops._HostDelta``.  Checked against torch autograd through a dense fp64 formula of the same posterior."""
import numpy as np
import pytest
import torch

import stheno_amd as st
from stheno_amd import ops

from . import posterior_cov_cases as C
from .test_posterior_grad_host import KERNELS, TransposedSolveOracle, tsolve_backend      # noqa: F401


@pytest.mark.parametrize("kinds", KERNELS + [C.TWO_GROUP])
@pytest.mark.parametrize("loss", ["var", "sample", "entropy"])
def test_joint_covariance_gradients_host_logic(tsolve_backend, kinds, loss):      # noqa: F811
    C.run_case(kinds, loss)


@pytest.mark.parametrize("loss", ["var", "sample"])
def test_per_point_noise_and_one_test_point_host_logic(tsolve_backend, loss):      # noqa: F811
    C.run_case(("eq", "linear"), loss, per_point=True, seed=3)
    C.run_case(("eq",), loss, ns=1, seed=4)


def test_predictive_noise_on_the_dense_covariance_host_logic(tsolve_backend):      # noqa: F811
    C.run_case(("matern52",), "var", pred_noise=True, seed=5)


def test_sample_noise_argument_and_generator_host_logic(tsolve_backend):      # noqa: F811
    """``sample(noise=...)`` with a number is the predictive noise of ``post(xs, noise)``; a generator's draws are the ``xi`` it makes."""
    p, fixed = C.make(("eq",), seed=6)
    P = C.leaves(p, ("lv", "ls", "xs"), torch.float64, "cpu")
    f = C.process(("eq",), P)
    post = f | (f(P["x"], 0.2), P["y"])
    xi = torch.tensor(fixed["xi"])
    a = post(P["xs"]).sample(noise=C.PRED_NOISE, xi=xi)
    b = post(P["xs"], C.PRED_NOISE).sample(xi=xi)
    assert a.requires_grad and torch.allclose(a, b, rtol=0, atol=1e-12)
    ga = torch.autograd.grad(a.sum(), [P["lv"], P["ls"], P["xs"]], retain_graph=True)      # (the two share exp(lv), exp(ls))
    gb = torch.autograd.grad(b.sum(), [P["lv"], P["ls"], P["xs"]])
    for u, v in zip(ga, gb):
        assert torch.allclose(u, v, rtol=1e-9, atol=1e-12)
    g1 = post(P["xs"]).sample(3, generator=torch.Generator().manual_seed(1))
    xi1 = torch.randn((7, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert g1.requires_grad and torch.equal(g1.detach(), post(P["xs"]).sample(xi=xi1).detach())


class _Recording(TransposedSolveOracle):
    def __init__(self):
        self.calls = []

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if callable(attr) and not name.startswith("_"):
            object.__getattribute__(self, "calls").append(name)
        return attr


def _plain_calls(learnable):
    rng = np.random.default_rng(1)
    x, y, xs = (torch.tensor(a) for a in (rng.standard_normal((20, 2)), rng.standard_normal((20, 1)), rng.standard_normal((5, 2))))
    v = torch.tensor(1.3, requires_grad=learnable)
    rec = _Recording()
    prev = ops.set_backend(rec)
    try:
        f = st.GP(v * st.EQ())
        fdd = (f | (f(x, 0.1), y))(xs, 0.05)
        cov = fdd.var.mat
        s = fdd.sample(xi=torch.ones((5, 2), dtype=torch.float64))
        h = fdd.entropy()
    finally:
        ops.set_backend(prev)
    return rec.calls, cov, s, h


def test_nothing_learnable_keeps_the_plain_path():
    """Without a learnable quantity the covariance, the samples and the entropy come from the plain path: no autograd node, and the
    backend sees exactly the calls it sees under ``torch.no_grad()`` -- no new backend call."""
    calls, cov, s, h = _plain_calls(False)
    assert cov.grad_fn is None and s.grad_fn is None and h.grad_fn is None
    with torch.no_grad():
        calls_ng, cov_ng, s_ng, h_ng = _plain_calls(True)
    assert sorted(calls) == sorted(calls_ng)              # (the same launches; an argument may be formed before or after its callee is looked up)
    assert torch.equal(cov, cov_ng) and torch.equal(s, s_ng) and torch.equal(h, h_ng)
    assert "potrf_vjp" not in calls and "tri_solve_t_" not in calls and "kmat_vjp_dense" not in calls
    learn_calls, cov_l, s_l, h_l = _plain_calls(True)
    assert cov_l.requires_grad and s_l.requires_grad and h_l.requires_grad
    assert torch.equal(cov_l.detach(), cov)
    assert "tri_solve_t_" not in learn_calls and "kmat_vjp_dense" not in learn_calls      # (the forward is the plain path's: B is formed in the backward)


def _outside_cases(learnable):
    """Calls outside the admitted case: ``(values, requires_grad)`` of a batched covariance, a pseudo-point posterior's covariance and
    a ``kl`` between two posterior predictions."""
    rng = np.random.default_rng(2)
    v = torch.tensor(1.2, requires_grad=learnable)
    ls = torch.tensor(0.9, requires_grad=learnable)
    f = st.GP(v * st.EQ().stretch(ls))
    out = []
    xb, yb, xsb = (torch.tensor(a) for a in (rng.standard_normal((2, 12, 2)), rng.standard_normal((2, 12, 1)), rng.standard_normal((2, 4, 2))))
    out.append((f | (f(xb, 0.1), yb))(xsb).var.mat)
    x, y, xs, z = (torch.tensor(a) for a in (rng.standard_normal((15, 2)), rng.standard_normal((15, 1)), rng.standard_normal((4, 2)),
                                             rng.standard_normal((6, 2))))
    sparse = f | st.PseudoObs(f(z), f(x, 0.1), y)
    out.append(sparse(xs).var.mat)
    exact = f | (f(x, 0.1), y)
    with torch.no_grad():
        other = exact(xs, 0.3)
        other.mean_var
    out.append(sparse(xs, 0.2).kl(other))
    return [(t.detach().clone(), t.requires_grad) for t in out]


def test_calls_outside_the_admitted_case_are_unchanged(oracle_backend):
    """A batched call, a pseudo-point posterior and ``kl`` return what they return under ``torch.no_grad()`` -- the values of the plain
    path -- with the ``requires_grad`` they had before this path existed (recorded on the parent commit: the two covariances carry no
    graph; ``kl`` carries the one of the pseudo-point posterior MEAN, which has had its differentiable path for long)."""
    got = _outside_cases(True)
    with torch.no_grad():
        ref = _outside_cases(True)
    for (a, ga), (b, gb), before in zip(got, ref, (False, False, True)):
        assert torch.equal(a, b)
        assert ga is before and gb is False
