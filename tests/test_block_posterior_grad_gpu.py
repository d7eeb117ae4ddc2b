"""Gradients through posteriors across processes through ``libgpk.so`` (``autograd._BlockPosteriorMarginals``: the plain groups on
``gpk_kmat_vjp_dense``, the derivative groups on ``gpk_kmat_diff_vjp``), in fp64 and fp32, against the dense torch reference of
``tests/block_posterior_cases.py`` at sizes across the 64-tile and 128-block edges (N1 = 70, N2 = 61, N* = 65)."""
import pytest
import torch

import stheno_amd as st

from . import block_posterior_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", C.CASES)
def test_gradients_against_the_dense_reference_fp64(hip_backend, case):
    C.check_case(case, C.GPU_SIZES, torch.float64, "cuda")


@pytest.mark.parametrize("case", C.CASES)
def test_gradients_against_the_dense_reference_fp32(hip_backend, case):
    st.B.epsilon = 1e-6
    try:
        C.check_case(case, C.GPU_SIZES, torch.float32, "cuda")
    finally:
        st.B.epsilon = 1e-12


def test_refusals(hip_backend):
    g = torch.Generator().manual_seed(3)
    t = lambda *shape, **kw: torch.randn(*shape, generator=g, dtype=torch.float64).to("cuda").requires_grad_(kw.get("grad", False))      # noqa: E731
    x1, x2, y1, y2 = t(12, 2), t(9, 2), t(12, 1), t(9, 1)
    with st.Measure() as prior:
        f = st.GP(st.EQ().stretch(0.9))
        df = f.diff(1)
    post = prior | ((f(x1, 0.1), y1), (df(x2, 0.1), y2))
    with pytest.raises(NotImplementedError, match="inputs of a mixed derivative block"):
        post(df)(t(5, 2, grad=True)).marginals()
    scales = torch.tensor([0.8, 1.3], dtype=torch.float64, device="cuda", requires_grad=True)
    with st.Measure() as prior:
        f = st.GP(st.EQ().stretch(scales))
        df = f.diff(1)
    post = prior | ((f(x1, 0.1), y1), (df(x2, 0.1), y2))
    with pytest.raises(NotImplementedError, match="per-dimension length scales under a derivative"):
        post(f)(t(5, 2)).marginals()
