"""Input maps for kernels, means and processes on the device (MI355X): values, the in-place factorisation, the lag model's joint
matrix and posterior, and the gradients of the additive, lag and deep-kernel models through ``libgpk.so`` -- one ``gpk_kmat`` launch and
one ``gpk_kmat_vjp`` / ``gpk_kmat_vjp_dense`` reduction per group, the maps in torch in front of them.  The same models, data,
references and tolerances as ``tests/test_input_maps_host.py`` (``tests/input_maps_cases.py``): central finite differences of the NumPy
closed form, ``|autograd - fd| <= 1e-6 max(max|fd|, 1)`` in fp64, 1e-3 in fp32; values 1e-6 and 1e-3.

N = 130 puts the matrix across one 128-wide diagonal block and two 64-row tiles of the reductions, the blocks of 70 + 60 rows put a
block border inside a tile, N* = 33 is past one 32-row tile of the kernel-matrix kernel."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import kernels as K
from stheno_amd.matrix import KernelDense

from . import input_maps_cases as C

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-6, torch.float32: 1e-3}


def dev(a, dtype=torch.float64, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda", requires_grad=grad)


@pytest.fixture()
def eps():
    old = st.B.epsilon
    st.B.epsilon = C.EPS
    yield
    st.B.epsilon = old


@pytest.fixture()
def eps32():
    """fp32 takes the jitter fp32 can hold: 1e-6 against noises of 0.2 and more moves the references by less than 1e-5 of themselves."""
    old = st.B.epsilon
    st.B.epsilon = 1e-6
    yield
    st.B.epsilon = old


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", range(4))
def test_values_against_numpy(hip_backend, case, dtype):
    d = C.data()
    name, k, ref = C.value_cases()[case]
    x, xs, tol = d["x"], d["xs"], TOL[dtype]
    C.assert_matrix(f"{name}: k(x, xs)", k.pairwise(dev(x, dtype), dev(xs, dtype)), ref(x, xs), tol)
    C.assert_matrix(f"{name}: k(x)", k.pairwise(dev(x, dtype)), ref(x, x), tol)
    C.assert_matrix(f"{name}: elwise", k.elwise(dev(x, dtype))[:, 0], C.diag_np(ref, x), tol)
    if case == 0:
        xb = d["xbatch"]
        got = k.pairwise(dev(xb, dtype))
        C.assert_matrix("a batch", got, np.stack([ref(xb[b], xb[b]) for b in range(4)]), tol)


def test_additive_kernel_matrix_is_factorised_in_place(hip_backend, eps):
    d = C.data()
    k, _ = C.model_a()
    with torch.no_grad():
        fdd = st.GP(k)(dev(d["x"]), C.NOISE)
        var = fdd.var
        assert isinstance(var, KernelDense) and var._mat is None
        lp = fdd.logpdf(dev(d["y"]))
        assert var._mat is None and var._chol is not None             # never materialised beside its factor
    C.assert_value("logpdf from the in-place factor", float(lp), C.a_logpdf_reference()["value"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_lag_model_joint_matrix_and_posterior(hip_backend, dtype):
    d = C.data()
    old = st.B.epsilon
    st.B.epsilon = C.EPS if dtype == torch.float64 else 1e-6
    try:
        prior, f, g, _ = C.model_b(dtype, learn=False)
        xa, xb = dev(d["xa"], dtype), dev(d["xb"], dtype)
        fdd = prior(st.cross(f, g)((f(xa), g(xb))))
        C.assert_matrix("the joint matrix", fdd.var.mat, C.b_matrix(C.B_P0), TOL[dtype])
        post = f | (g(xb, C.NOISE_B), dev(d["yb"], dtype))
        out = post(dev(d["xt"], dtype))
        ref = C.b_posterior_reference()
        C.assert_close("posterior mean", out.mean[:, 0].cpu().numpy(), ref["mean"], TOL[dtype])
        C.assert_close("posterior variances", out.var_diag.cpu().numpy(), ref["var"], TOL[dtype])
    finally:
        st.B.epsilon = old


def test_additive_logpdf_gradients(hip_backend, eps):
    d = C.data()
    ref = C.a_logpdf_reference()
    k, t = C.model_a()
    tx = dev(d["x"], grad=True)
    lp = st.GP(k)(tx, C.NOISE).logpdf(dev(d["y"]))
    assert lp.requires_grad
    C.assert_value("logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    C.assert_close("hyper-parameters", [float(t[n].grad) for n in C.A_NAMES], ref["hyper"])
    C.assert_close("x", C.picked(tx.grad), ref["x"])


def test_additive_logpdf_gradients_fp32(hip_backend, eps32):
    d = C.data()
    ref = C.a_logpdf_reference()
    k, t = C.model_a(torch.float32)
    lp = st.GP(k)(dev(d["x"], torch.float32), C.NOISE).logpdf(dev(d["y"], torch.float32))
    assert lp.requires_grad and lp.dtype == torch.float32
    C.assert_value("logpdf (fp32)", float(lp.detach()), ref["value"], tol=1e-3)
    lp.backward()
    C.assert_close("hyper-parameters (fp32)", [float(t[n].grad) for n in C.A_NAMES], ref["hyper"], tol=1e-3)


def test_additive_posterior_marginal_gradients(hip_backend, eps):
    d = C.data()
    ref = C.a_marginals_reference()
    k, t = C.model_a()
    f = st.GP(k)
    tx = dev(d["x"], grad=True)
    fdd = (f | (f(tx, C.NOISE_MARGINALS), dev(d["y"])))(dev(d["xs"]))
    loss = fdd.mean.sum() + fdd.var_diag.sum()
    assert loss.requires_grad
    C.assert_value("loss", float(loss.detach()), ref["value"])
    loss.backward()
    C.assert_close("hyper-parameters", [float(t[n].grad) for n in C.A_NAMES], ref["hyper"])
    C.assert_close("x", C.picked(tx.grad), ref["x"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_lag_joint_logpdf_gradients(hip_backend, dtype):
    d = C.data()
    ref = C.b_joint_reference()
    old = st.B.epsilon
    st.B.epsilon = C.EPS if dtype == torch.float64 else 1e-6
    try:
        prior, f, g, t = C.model_b(dtype)
        lp = prior.logpdf((f(dev(d["xa"], dtype), C.NOISE), dev(d["ya"], dtype)), (g(dev(d["xb"], dtype), C.NOISE_B), dev(d["yb"], dtype)))
        assert lp.requires_grad
        C.assert_value("joint logpdf", float(lp.detach()), ref["value"], TOL[dtype])
        lp.backward()
    finally:
        st.B.epsilon = old
    C.assert_close("(v, s, tau)", [float(t[n].grad) for n in C.B_NAMES], ref["hyper"], TOL[dtype])


def test_deep_kernel_logpdf_gradients(hip_backend, eps):
    d = C.data()
    ref = C.c_logpdf_reference()
    k, v, fn = C.model_c(device="cuda")
    lp = st.GP(k)(dev(d["x"]), C.NOISE).logpdf(dev(d["y"]))
    assert lp.requires_grad
    C.assert_value("logpdf", float(lp.detach()), ref["value"])
    lp.backward()
    C.assert_close("variance and the 24 network entries", np.concatenate([[float(v.grad)], fn.grads()]), ref["params"])


def test_deep_kernel_bound_gradients(hip_backend, eps):
    d = C.data()
    ref = C.c_elbo_reference()
    k, v, fn = C.model_c(device="cuda", learn=("w2",), w2_scale=C.W2_BOUND)
    f = st.GP(k)
    z = dev(d["z"], grad=True)
    elbo = st.PseudoObs(f(z), f(dev(d["x"]), C.NOISE), dev(d["y"])).elbo(f.measure)
    assert elbo.requires_grad
    C.assert_value("bound", float(elbo.detach()), ref["value"])
    elbo.backward()
    got = np.concatenate([[float(v.grad)], fn.w2.grad.cpu().numpy().ravel(), z.grad.cpu().numpy().ravel()])
    C.assert_close("variance, W2 and the inducing inputs", got, ref["params"])


def test_a_mapped_block_is_written_in_place(hip_backend, monkeypatch):
    """``_eval_into`` hands the block's own view to the fused launches (no temporary, no copy): every launch writes at the view's
    address, the values are right and nothing outside the block is touched."""
    d = C.data()
    x, xs = d["x"], d["xs"]
    _, k, ref = C.value_cases()[0]
    cross = k.shift(0.25, 0)
    targets = []
    kmat = hip_backend.kmat

    def recording(terms, a, b=None, **kw):
        targets.append(None if kw.get("out") is None else kw["out"].data_ptr())
        return kmat(terms, a, b, **kw)

    monkeypatch.setattr(hip_backend, "kmat", recording)
    buf = torch.full((C.N + 7, C.NS + 5), float("nan"), dtype=torch.float64, device="cuda")
    view = buf[3:3 + C.N, 2:2 + C.NS]
    K._eval_into(cross, dev(x), dev(xs), view)
    assert targets == [view.data_ptr()] * 3
    assert view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    C.assert_matrix("the block", view, ref(x - 0.25, xs))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[3:3 + C.N, 2:2 + C.NS] = False
    assert bool(torch.isnan(buf[outside]).all())
    # a symmetric diagonal block, lower triangle only
    del targets[:]
    sq = torch.full((C.N, C.N), float("nan"), dtype=torch.float64, device="cuda")
    K._eval_into(k, dev(x), None, sq, lower=True)
    assert targets == [sq.data_ptr()] * 3
    C.assert_matrix("the lower triangle", torch.tril(sq), np.tril(ref(x, x)))


def test_scaled_sum_behind_different_maps_inside_a_multi_process_matrix(hip_backend, eps):
    """``h = 2 (f1 + f2)``, ``f1`` behind per-dimension scales and ``f2`` periodic: the blocks of ``h`` go group by group into the
    multi-process matrix, which is factorised in place."""
    d = C.data()
    x, y = d["x"][:, :2], d["y"]
    ls = np.array([1.0, 2.0])

    def k1(a, b):
        return C.eq_np(a / ls, b / ls)

    def k2(a, b):
        return C.eq_np(C.pmap(a, 3.0), C.pmap(b, 3.0))

    with st.Measure() as prior:
        f1, f2 = st.GP(st.EQ().stretch([1.0, 2.0])), st.GP(st.EQ().periodic(3.0))
        h = 2.0 * (f1 + f2)
    ref = np.block([[4.0 * (k1(x, x) + k2(x, x)), 2.0 * k1(x, x)], [2.0 * k1(x, x), k1(x, x)]])
    with torch.no_grad():
        fdd = prior(st.cross(h, f1)((h(dev(x)), f1(dev(x)))))
        C.assert_matrix("the joint matrix", fdd.var.mat, ref)
        lp = prior.logpdf((h(dev(x), 0.1), dev(y)), (f1(dev(x), 0.1), dev(y)))
    C.assert_value("joint logpdf", float(lp), C.logpdf_np(ref + (0.1 + C.EPS) * np.eye(2 * C.N), np.concatenate([y, y])))


def test_stretch_of_a_process_with_a_periodic_kernel(hip_backend):
    d = C.data()
    x = d["x"][:, :2]

    def ref(a, b):
        return C.eq_np(C.pmap(a, 3.1), C.pmap(b, 3.1))

    with st.Measure() as prior:
        f = st.GP(st.EQ().periodic(3.1))
        u = f.stretch(2.0)
    fdd = prior(st.cross(u, f)((u(dev(x)), f(dev(x)))))
    C.assert_matrix("the joint matrix", fdd.var.mat, np.block([[ref(x / 2, x / 2), ref(x / 2, x)], [ref(x, x / 2), ref(x, x)]]))
