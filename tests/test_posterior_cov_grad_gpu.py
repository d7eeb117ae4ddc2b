"""Gradients through the JOINT posterior covariance (``post(xs).var``, ``.sample()``, ``.entropy()``) through ``libgpk.so``:
``autograd._PosteriorCovariance``, the differentiable factorisation on ``gpk_potrf_vjp`` and the differentiable log-determinant,
against torch autograd through a dense fp64 formula of the same posterior (``tests/posterior_cov_cases.py``).

Bounds: 1e-6 relative (``max |got - ref| / max |ref|`` per leaf) in fp64; the one fp32 case at 1e-3 with ``B.epsilon = 1e-6`` and the
denominator ``test_posterior_marginal_gradients_gpu_fp32`` uses (at least 1)."""
import numpy as np
import pytest
import torch

import stheno_amd as st

from . import posterior_cov_cases as C

pytestmark = pytest.mark.gpu

LOSSES = ["var", "sample", "entropy"]
KERNELS = [("eq",), ("eq", "linear"), ("matern52", "matern12"), C.TWO_GROUP]


@pytest.mark.parametrize("kinds", KERNELS)
@pytest.mark.parametrize("loss", LOSSES)
def test_joint_covariance_gradients_gpu(hip_backend, kinds, loss):
    C.run_case(kinds, loss, dev="cuda", n=300, ns=64, tol=1e-6)


@pytest.mark.parametrize("loss", LOSSES)
def test_joint_covariance_gradients_gpu_ragged_per_point_noise(hip_backend, loss):
    C.run_case(("eq",), loss, dev="cuda", n=1000, ns=129, d=4, per_point=True, tol=1e-6, seed=11)


@pytest.mark.parametrize("loss", LOSSES)
def test_joint_covariance_gradients_gpu_one_test_point(hip_backend, loss):
    C.run_case(("eq", "linear"), loss, dev="cuda", n=300, ns=1, tol=1e-6, seed=13)


def test_joint_covariance_gradients_gpu_fp32(hip_backend):
    st.B.epsilon = 1e-6
    try:
        C.run_case(("eq",), "sample", dev="cuda", dtype=torch.float32, n=1000, ns=64, tol=1e-3, clamp=True, seed=12)
    finally:
        st.B.epsilon = 1e-12


def _grads(order, n=2048, ns=64, repeat=1):          # (the smallest shape that takes the rows-under-the-matrix factorisation)
    rng = np.random.default_rng(21)
    x, y, xs = rng.standard_normal((n, 3)), rng.standard_normal((n, 1)), rng.standard_normal((ns, 3))
    xi = torch.tensor(rng.standard_normal((ns, C.NUM)), device="cuda")
    out = []
    for _ in range(repeat):
        lv = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
        ls = torch.tensor(0.2, dtype=torch.float64, requires_grad=True)
        txs = torch.tensor(xs, device="cuda", requires_grad=True)
        f = st.GP(torch.exp(lv) * st.EQ().stretch(torch.exp(ls)))
        fdd = f(torch.tensor(x, device="cuda"), 0.1)
        ty = torch.tensor(y, device="cuda")
        if order == "logpdf_first":
            with torch.no_grad():
                fdd.logpdf(ty)
        post = f | (fdd, ty)
        pred = post(txs, C.PRED_NOISE)
        s = pred.sample(xi=xi)
        if order == "rows":
            assert fdd.var.chol().rows_under == ns, "the factorisation with rows under the matrix did not run"
        ((s * s).sum() + pred.entropy()).backward()
        out.append([lv.grad.clone(), ls.grad.clone(), txs.grad.clone()])
    return out


def test_rows_path_and_cached_factor_give_the_same_gradients(hip_backend):
    a, b = _grads("rows")[0], _grads("logpdf_first")[0]
    for ga, gb in zip(a, b):
        assert float((ga - gb).abs().max() / gb.abs().max()) <= 1e-9


def test_repeated_backward_is_bit_identical(hip_backend):
    first, second = _grads("rows", repeat=2)
    for ga, gb in zip(first, second):
        assert torch.equal(ga, gb)


def test_q_batch_ascent_raises_the_acquisition(hip_backend):
    """Adam ascent of a q = 8 candidate batch on a Monte-Carlo acquisition from joint samples with fixed draws (the expected best
    value of the batch)."""
    rng = np.random.default_rng(8)
    x = torch.tensor(rng.uniform(-3, 3, (500, 2)), device="cuda")
    y = torch.sin(x[:, :1]) + torch.cos(x[:, 1:])
    f = st.GP(st.EQ().stretch(1.2))
    post = f | (f(x, 0.01), y)
    xs = torch.tensor(rng.uniform(-3, 3, (8, 2)), device="cuda", requires_grad=True)
    xi = torch.tensor(rng.standard_normal((8, 64)), device="cuda")
    opt = torch.optim.Adam([xs], lr=0.05)

    def acquisition():
        return post(xs).sample(xi=xi).max(dim=0).values.mean()

    start = float(acquisition().detach())
    for _ in range(20):
        opt.zero_grad()
        (-acquisition()).backward()
        opt.step()
    assert float(acquisition().detach()) > start
