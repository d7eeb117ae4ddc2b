"""Gradients through the mean and the marginal variances of a pseudo-point posterior (VFE / FITC / DTC) through ``libgpk.so``
(``autograd._SparsePosteriorMarginals``), against the dense fp64 torch reference on the CPU (``tests/sparse_posterior_reference.py``).
Shapes, inducing inputs and the reference's stability under the jitter: ``tests/test_sparse_posterior_grad_host.py`` (``GPU_CASES``).
Every case asserts the forward values first (1e-9 of the largest entry in fp64), then the gradients of the UCB loss with respect to
``z``, ``xs`` and every hyper-parameter: ``max |got - ref| <= tol max(max |ref|, 1)``, ``tol = 1e-6`` in fp64 and ``1e-3`` in fp32."""
import pytest
import torch

import stheno_amd as st

from .test_sparse_posterior_grad_host import GPU_CASES, run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", ["vfe", "fitc", "dtc"])
def test_partial_tiles_all_methods_all_leaves(hip_backend, method):
    """N = 200, M = 70, N* = 45, D = 3 with per-dimension length scales: ``x`` is a leaf here too."""
    run_case(("eq",), "ucb", method, dev="cuda", tol=1e-6, **GPU_CASES["partial_tiles"])


@pytest.mark.parametrize("loss", ["mean", "var"])
def test_partial_tiles_mean_only_and_variance_only(hip_backend, loss):
    run_case(("eq", "matern52"), loss, "fitc", dev="cuda", tol=1e-6, per_point=True, **GPU_CASES["partial_tiles"])


def test_inducing_points_a_multiple_of_128(hip_backend):
    """N = 300, M = 128, N* = 64, D = 2: whichever whitening route the plain path takes at whole 128-tiles."""
    run_case(("eq",), "ucb", "vfe", dev="cuda", tol=1e-6, fixed=("x",), **GPU_CASES["m_multiple_of_128"])


def test_fp32(hip_backend):
    """N = 1000, M = 128, N* = 64, D = 2 in fp32, at the fp32 jitter."""
    st.B.epsilon = 1e-6
    try:
        run_case(("eq",), "ucb", "vfe", dev="cuda", dtype=torch.float32, tol=1e-3, vtol=1e-3, fixed=("x",), **GPU_CASES["fp32"])
    finally:
        st.B.epsilon = 1e-12
