"""Gradients through BATCHED posterior means and marginal variances on the HIP path (``autograd._BatchedPosteriorMarginals``: the
batched factor, ``gpk_trsm_lower_t`` / ``gpk_trsv_lower_t``, ``gpk_gemm``, ``gpk_symmetrize`` and one ``gpk_kmat_vjp_dense_batch``
launch per reduction), against torch autograd through the pure-torch fp64 formula entry by entry (``tests/batch_posterior_cases.py``).
Tolerances are the project's parity tolerances: 1e-6 in fp64, 1e-3 in fp32 with ``B.epsilon = 1e-6``."""
import numpy as np
import pytest
import torch

import stheno_amd as st

from .batch_posterior_cases import run_case

pytestmark = pytest.mark.gpu

#: three row tiles of the reductions (the last one two rows wide) and two column tiles
MAIN = dict(nb=3, n=130, ns=70, d=3, per_point=True, dev="cuda", tol=1e-6)
KERNELS = [("eq",), ("eq", "linear"), ("matern52", "matern12"), "rq"]


@pytest.mark.parametrize("kinds", KERNELS, ids=str)
@pytest.mark.parametrize("loss", ["mean", "var", "ucb"])
def test_batched_posterior_marginal_gradients_gpu(hip_backend, kinds, loss):
    run_case(kinds, loss, **MAIN)


def test_per_dimension_scales(hip_backend):
    run_case(("eq", "matern52"), "ucb", **dict(MAIN, d=4, ard=True, seed=3))


@pytest.mark.parametrize("model", ["two_groups", "period"])
def test_sums_behind_different_maps(hip_backend, model):
    run_case(model, "ucb", **dict(MAIN, seed=4))


@pytest.mark.parametrize("opts", [dict(shared_x=True), dict(pred_noise=True, per_point=False), dict(call="bounds"), dict(call="mean", loss="mean"),
                                  dict(call="var", loss="var")], ids=str)
def test_options_gpu(hip_backend, opts):
    opts = dict(opts)
    run_case(("eq", "linear"), opts.pop("loss", "ucb"), **dict(MAIN, seed=5, **opts))


def test_block_multiple(hip_backend):
    run_case(("eq",), "ucb", **dict(MAIN, n=256, ns=64, seed=6))


def test_mixed_phase_factor_fp32(hip_backend):
    """64 x 512 in fp32: the factor comes from the mixed-phase batched factorisation."""
    st.B.epsilon = 1e-6
    try:
        run_case(("eq",), "ucb", nb=64, n=512, ns=64, d=3, dev="cuda", dtype=torch.float32, tol=1e-3, mean_fn=False, seed=12)
    finally:
        st.B.epsilon = 1e-12


def test_repeated_backward_is_bit_identical(hip_backend):
    run_case(("eq", "matern12"), "ucb", **dict(MAIN, seed=7, repeat=True))


def test_logpdf_first_and_posterior_first_give_the_same_gradients(hip_backend):
    a = run_case(("eq", "linear"), "ucb", **dict(MAIN, seed=8))
    b = run_case(("eq", "linear"), "ucb", **dict(MAIN, seed=8, logpdf_first=True))
    for k in ("x", "xs", "y", "lv", "ls", "lnoise", "c"):
        assert float((a[k].grad - b[k].grad).abs().max() / b[k].grad.abs().max()) <= 1e-9, k


def test_batched_ucb_ascent_raises_the_acquisition_in_every_entry(hip_backend):
    rng = np.random.default_rng(8)
    nb = 4
    x = torch.tensor(rng.uniform(-3, 3, (nb, 200, 2)), device="cuda")
    y = torch.sin(x[..., :1]) + torch.cos(x[..., 1:]) * torch.linspace(0.5, 1.5, nb, device="cuda", dtype=x.dtype).reshape(nb, 1, 1)
    f = st.GP(st.EQ().stretch(1.2))
    post = f | (f(x, 0.01), y)
    xs = torch.tensor(rng.uniform(-3, 3, (nb, 16, 2)), device="cuda", requires_grad=True)
    opt = torch.optim.Adam([xs], lr=0.05)

    def ucb():
        mean, var = post(xs).marginals()
        return (mean.reshape(nb, -1) + 2.0 * torch.sqrt(var.reshape(nb, -1))).sum(-1)

    start = ucb().detach()
    for _ in range(20):
        opt.zero_grad()
        (-ucb().sum()).backward()
        opt.step()
    assert bool((ucb().detach() > start).all())
