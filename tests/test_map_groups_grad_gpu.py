"""Learning sums of kernels behind DIFFERENT input maps on the device (MI355X): the log-density of one process, the joint log-density
of a sum process and one of its parts, and the posterior marginals, through ``libgpk.so`` -- one ``gpk_kmat`` launch and one
``gpk_kmat_vjp`` / ``gpk_kmat_vjp_dense`` reduction per group.  The same models, data, references and tolerances as
``tests/test_map_groups_grad_host.py`` (``tests/map_groups_cases.py``): central finite differences of the NumPy closed form,
``|autograd - fd| <= 1e-6 max(max|fd|, 1)`` in fp64, 1e-3 in fp32.

N = 130 puts the matrix across one 128-wide diagonal block, the blocks of 70 + 60 rows put a block border inside a 128-tile, N* = 33 is
past one 32-row tile."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st

from . import map_groups_cases as C

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float64, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda", requires_grad=grad)


@pytest.fixture()
def eps():
    old = st.B.epsilon
    st.B.epsilon = C.EPS
    yield
    st.B.epsilon = old


def test_logpdf_of_three_groups_all_gradients(hip_backend, eps):
    x, _, y, _ = C.data()
    ref = C.logpdf_reference()
    k, t = C.three_group_kernel()
    tx, ty = dev(x, grad=True), dev(y, grad=True)
    noise = torch.tensor(C.NOISE, dtype=torch.float64, requires_grad=True)
    lp = st.GP(k)(tx, noise).logpdf(ty)
    assert lp.requires_grad
    C.assert_value("logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    C.assert_close("hyper-parameters", C.hyper_grads(t), ref["hyper"])
    C.assert_close("noise", float(noise.grad), ref["noise"])
    C.assert_close("y", ty.grad.cpu().numpy(), ref["y"])
    C.assert_close("x", tx.grad.cpu().numpy(), ref["x"])


def test_logpdf_of_three_groups_without_learnable_maps(hip_backend, eps):
    """The implicit form: one ``gpk_kmat_vjp`` pass over the lower triangle of ``K^{-1}`` per group."""
    x, _, y, _ = C.data()
    ref = C.logpdf_reference()
    k, t = C.three_group_kernel(learn=C.PLAIN)
    lp = st.GP(k)(dev(x), C.NOISE).logpdf(dev(y))
    C.assert_value("logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    pick = [C.NAMES.index(n) for n in C.PLAIN]
    C.assert_close("variances and scalar scales", C.hyper_grads(t, C.PLAIN), ref["hyper"][pick])


def test_logpdf_of_three_groups_fp32_hyper_parameters(hip_backend):
    """fp32 on the device against the fp64 reference: the project's fp32 parity figure, 1e-3 of ``max(max|fd|, 1)``.  (fp32 takes the
    jitter fp32 can hold: 1e-6 against a noise of 0.3 moves the reference by less than 1e-5 of itself.)"""
    x, _, y, _ = C.data()
    ref = C.logpdf_reference()
    old = st.B.epsilon
    st.B.epsilon = 1e-6
    try:
        k, t = C.three_group_kernel(dtype=torch.float32)
        lp = st.GP(k)(dev(x, torch.float32), C.NOISE).logpdf(dev(y, torch.float32))
        assert lp.requires_grad and lp.dtype == torch.float32
        C.assert_value("logpdf (fp32)", float(lp.detach()), ref["value"], tol=1e-3)
        lp.backward()
    finally:
        st.B.epsilon = old
    C.assert_close("hyper-parameters (fp32)", C.hyper_grads(t), ref["hyper"], tol=1e-3)


def test_joint_logpdf_of_a_sum_process_and_its_periodic_part(hip_backend, eps):
    x, _, y, _ = C.data()
    ref = C.joint_reference()
    prior, f, f2, t = C.joint_model()
    lp = prior.logpdf((f(dev(x[:C.NA]), C.NOISE), dev(y[:C.NA])), (f2(dev(x[C.NA:]), C.NOISE_B), dev(y[C.NA:])))
    assert lp.requires_grad
    C.assert_value("joint logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    C.assert_close("hyper-parameters", np.array([float(t[n].grad) for n in C.JOINT_NAMES]), ref["hyper"])


def test_posterior_marginals_of_three_groups(hip_backend, eps):
    x, xs, y, _ = C.data()
    ref = C.marginals_reference()
    k, t = C.three_group_kernel()
    f = st.GP(k)
    tx, txs = dev(x, grad=True), dev(xs, grad=True)
    post = f | (f(tx, C.NOISE), dev(y))
    fdd = post(txs)
    loss = fdd.mean.sum() + fdd.var_diag.sum()
    assert loss.requires_grad
    C.assert_value("loss", float(loss.detach()), ref["value"])
    loss.backward()
    C.assert_close("hyper-parameters", C.hyper_grads(t), ref["hyper"])
    C.assert_close("x", tx.grad.cpu().numpy(), ref["x"])
    C.assert_close("xs", txs.grad.cpu().numpy(), ref["xs"])


def test_learning_a_period_end_to_end(hip_backend):
    """A short version of ``examples/learn_decomposition.py``: N = 300, 60 Adam steps from a period 15 % off."""
    old = st.B.epsilon
    st.B.epsilon = 1e-8
    try:
        losses, period = C.fit_decomposition("cuda")
    finally:
        st.B.epsilon = old
    print(f"loss {losses[0]:.3f} -> {losses[-1]:.3f}, learnt period {period:.4f} (generating: {C.FIT_PERIOD})")
    assert losses[-1] < losses[0]
    assert abs(period - C.FIT_PERIOD) <= 0.05 * C.FIT_PERIOD
