"""Host logic of the rational-quadratic term kind and of ``k.periodic(p)``: the term algebra with shape parameters, the input-map
view, group-wise evaluation of sums behind different maps, the refusals, and the C ABI of the entries with shapes.  Periodic
kernels of the kinds the test suite's CPU backend knows are evaluated through it and held against the closed form
``exp(-2 sum_d sin^2(pi (x_d - y_d) / p_d))``; ``"rq"`` values are a GPU matter (``tests/test_rq_periodic_gpu.py``)."""
import os
import re

import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import _native, kernels as K, ops
from stheno_amd.torch import EQ, RQ, Linear, Matern32

from .conftest import ROOT, T


def per_eq(x, y, p, scale=1.0):
    x, y = np.atleast_2d(x.T).T if x.ndim == 1 else x, np.atleast_2d(y.T).T if y.ndim == 1 else y
    delta = x[..., :, None, :] - y[..., None, :, :]
    return np.exp(-2.0 * (np.sin(np.pi * delta / np.asarray(p)) ** 2).sum(-1) / scale**2)


def np_(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------
# periodic values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17,), (17, 1), (17, 3), (2, 17, 3)], ids=["N", "Nx1", "NxD", "BxNxD"])
def test_periodic_eq_values(any_backend, shape):
    rng = np.random.default_rng(len(shape) + shape[-1])
    x = rng.uniform(-4, 4, shape)
    y = rng.uniform(-4, 4, shape[:-2] + (11,) + shape[-1:]) if len(shape) > 1 else rng.uniform(-4, 4, (11,))
    d = 1 if len(shape) == 1 else shape[-1]
    periods = [2.5, torch.tensor(2.5, dtype=torch.float64)]
    if d > 1:
        periods += [[2.5, 1.5, 4.0], T([2.5, 1.5, 4.0])]
    for p in periods:
        k = EQ().periodic(p)
        pn = np_(p) if torch.is_tensor(p) else p
        ref = per_eq(x, y, pn)
        assert np.allclose(np_(k.pairwise(T(x), T(y))), ref, rtol=0, atol=1e-12)
        sym = per_eq(x, x, pn)
        assert np.allclose(np_(k.pairwise(T(x))), sym, rtol=0, atol=1e-12)
        assert np.allclose(np_(k.elwise(T(x)))[..., 0], np.diagonal(sym, axis1=-2, axis2=-1), rtol=0, atol=1e-12)
        assert k.stationary and reversed(k) is k and k.terms() is None


def test_periodic_matern_stretch_and_scale(any_backend):
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-3, 3, (20, 2)), rng.uniform(-3, 3, (9, 2))
    r = 2.0 * np.sqrt((np.sin(np.pi * (x[:, None, :] - y[None, :, :]) / 1.7) ** 2).sum(-1))
    k = Matern32().periodic(1.7)
    assert np.allclose(np_(k.pairwise(T(x), T(y))), (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r), rtol=0, atol=1e-12)
    # stretch goes to the kernel behind the map; a scale in front stays one fused launch on the mapped inputs
    ks = 1.5 * EQ().periodic(1.7).stretch(0.6)
    assert isinstance(EQ().periodic(1.7).stretch(0.6), K.Periodic)
    assert np.allclose(np_(ks.pairwise(T(x), T(y))), 1.5 * per_eq(x, y, 1.7, 0.6), rtol=0, atol=1e-12)
    assert reversed(ks) is ks


def test_sums_mixing_periodic_and_plain_terms(any_backend):
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-3, 3, (23, 2)), rng.uniform(-3, 3, (8, 2))
    plain = np.exp(-0.5 * ((x[:, None] - y[None]) ** 2).sum(-1) / 0.8**2)
    k = 0.5 * EQ().stretch(0.8) + EQ().periodic(2.0) + 2.0 * EQ().periodic([1.0, 3.0]) + 0.3 * Linear()
    ref = 0.5 * plain + per_eq(x, y, 2.0) + 2.0 * per_eq(x, y, [1.0, 3.0]) + 0.3 * x @ y.T
    groups = K._map_groups(k)
    assert k.terms() is None and k.input_scaled_view() is None and len(groups) == 3      # plain (EQ + Linear), period 2, periods (1, 3)
    assert np.allclose(np_(k.pairwise(T(x), T(y))), ref, rtol=0, atol=1e-12)
    # the same period twice is ONE group (one fused launch on the mapped inputs)
    k2 = EQ().periodic(2.0) + Matern32().periodic(2.0)
    assert k2.input_scaled_view() is not None and len(K._map_groups(k2)) == 1
    # symmetric: lower triangle only, diagonal additions once, into a caller's strided view, group by group
    n = x.shape[0]
    refs = 0.5 * np.exp(-0.5 * ((x[:, None] - x[None]) ** 2).sum(-1) / 0.8**2) + per_eq(x, x, 2.0) + 2.0 * per_eq(x, x, [1.0, 3.0]) + 0.3 * x @ x.T
    dv = np.linspace(0.1, 0.4, n)
    buf = torch.full((n, n + 4), -7.0, dtype=torch.float64, device=T(x).device)
    out = k.pairwise(T(x), lower=True, diag_add=0.25, diag_vec=T(dv), out=buf[:, :n])
    assert out.data_ptr() == buf.data_ptr()
    assert np.allclose(np.tril(np_(buf[:, :n])), np.tril(refs + np.diag(0.25 + dv)), rtol=0, atol=1e-12)
    assert bool((buf[:, n:] == -7.0).all())
    assert np.allclose(np_(k.elwise(T(x)))[:, 0], np.diag(refs), rtol=0, atol=1e-12)
    assert reversed(k) is k
    # a GP with such a kernel: logpdf against the dense computation
    yv = rng.standard_normal((n, 1))
    lp = float(st.GP(k)(T(x), 0.2).logpdf(T(yv)))
    cov = refs + (0.2 + st.B.epsilon) * np.eye(n)
    sign, logdet = np.linalg.slogdet(cov)
    want = -0.5 * (logdet + n * np.log(2 * np.pi) + (yv.T @ np.linalg.solve(cov, yv)).item())
    assert abs(lp - want) <= 1e-9 * abs(want)


def test_period_gradient_of_logpdf(oracle_backend):
    rng = np.random.default_rng(3)
    n = 40
    x, y = rng.uniform(-3, 3, (n, 2)), rng.standard_normal((n, 1))

    def logpdf(p, xx):
        cov = 1.3 * per_eq(xx, xx, p, 0.9) + (0.2 + st.B.epsilon) * np.eye(n)
        _, logdet = np.linalg.slogdet(cov)
        return -0.5 * (logdet + n * np.log(2 * np.pi) + (y.T @ np.linalg.solve(cov, y)).item())

    p = torch.tensor([2.2, 3.4], dtype=torch.float64, requires_grad=True)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lp = st.GP(1.3 * EQ().stretch(0.9).periodic(p))(tx, 0.2).logpdf(torch.tensor(y))
    assert lp.requires_grad and abs(float(lp) - logpdf(np.array([2.2, 3.4]), x)) <= 1e-9 * abs(float(lp))
    lp.backward()
    h = 1e-6
    for i in range(2):
        e = np.zeros(2)
        e[i] = h
        ref = (logpdf(np.array([2.2, 3.4]) + e, x) - logpdf(np.array([2.2, 3.4]) - e, x)) / (2 * h)
        assert abs(float(p.grad[i]) - ref) <= 2e-6 * max(abs(ref), 1.0)
    for (i, c) in [(0, 0), (17, 1), (39, 0)]:
        e = np.zeros_like(x)
        e[i, c] = h
        ref = (logpdf(np.array([2.2, 3.4]), x + e) - logpdf(np.array([2.2, 3.4]), x - e)) / (2 * h)
        assert abs(float(tx.grad[i, c]) - ref) <= 2e-6 * max(abs(ref), 1.0)


def test_period_and_input_gradients_need_at_most_four_dimensions(oracle_backend):
    rng = np.random.default_rng(4)
    x, y = torch.tensor(rng.standard_normal((12, 5))), torch.tensor(rng.standard_normal((12, 1)))
    p = torch.tensor(2.0, dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        st.GP(EQ().periodic(p))(x, 0.1).logpdf(y)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        st.GP(EQ().periodic(2.0))(xg, 0.1).logpdf(y)
    # (a learnable variance alone needs no input gradient: any dimension)
    v = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    assert st.GP(v * EQ().periodic(2.0))(x, 0.1).logpdf(y).requires_grad


# ---------------------------------------------------------------------------------------------
# term algebra and refusals
# ---------------------------------------------------------------------------------------------
def test_rq_term_algebra():
    assert RQ(0.3).terms() == [("rq", 1.0, 1.0)] and RQ(0.3).shapes() == [0.3] and RQ(0.3).stationary
    k = RQ(0.3) + RQ(0.3)
    assert k.terms() == [("rq", 2.0, 1.0)] and k.shapes() == [0.3]
    k = RQ(0.3) + RQ(0.4)
    assert len(k.terms()) == 2 and k.shapes() == [0.3, 0.4]
    k = RQ(0.3) + RQ(0.3).stretch(2.0) + EQ()
    assert [t[0] for t in k.terms()] == ["rq", "rq", "eq"] and k.shapes() == [0.3, 0.3, None]
    k = (2 * RQ(0.3)).stretch(3)
    assert k.terms() == [("rq", 2.0, 3.0)] and k.shapes() == [0.3] and reversed(k) is k
    a = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    k = 2 * RQ(a).stretch(1.5) + EQ()
    assert k.tensor_shapes()[0] is a and k.tensor_shapes()[1] is None and k.shapes() == [0.7, None]
    assert (RQ(a) + RQ(a)).tensor_shapes() == [a] and len((RQ(a) + RQ(torch.tensor(0.7))).tensor_terms()) == 2
    from stheno_amd import learnable as autograd
    assert autograd.kernel_requires_grad(k) and not autograd.kernel_requires_grad(RQ(0.7) + EQ())
    for bad in (0.0, -1.0, torch.tensor(-0.5)):
        with pytest.raises(ValueError, match="positive"):
            RQ(bad)
    for k in (EQ() + Linear(), EQ().stretch(2.0)):
        assert k.shapes() == [None] * len(k.terms())


def test_kterms_shapes():
    t = ops.KTerms([("rq", 1.0, 2.0), ("eq", 1.0, 1.0)], [0.5, None])
    assert t.shapes == [0.5, None] and list(t.c_shapes()) == [0.5, 0.0] and t.terms == [("rq", 1.0, 2.0), ("eq", 1.0, 1.0)]
    assert ops.KTerms([("eq", 1.0, 1.0)]).c_shapes() is None
    assert ops.KTerms([("eq", 1.0, 1.0)]).shapes is None and ops.KTerms([("eq", 1.0, 1.0)], [None]).shapes is None
    for bad in ([0.0], [-1.0], [None], None):
        with pytest.raises(ValueError, match="positive shape"):
            ops.KTerms([("rq", 1.0, 1.0)], bad)
    with pytest.raises(ValueError, match="unknown kernel kind"):
        ops.KTerms([("cubic", 1.0, 1.0)])
    with pytest.raises(ValueError, match="one shape entry per term"):
        ops.KTerms([("rq", 1.0, 1.0)], [0.5, 0.5])


def test_a_ninth_distinct_term_still_raises(oracle_backend):
    k = sum((RQ(0.1 * (i + 1)) for i in range(1, 9)), RQ(0.1))
    assert len(k.terms()) == 9
    with pytest.raises(ValueError, match="at most 8"):
        k.pairwise(torch.zeros(3, 1, dtype=torch.float64))


def test_refusals_stay():
    with pytest.raises(NotImplementedError, match="products of kernels"):
        RQ(1.0) * EQ()
    with pytest.raises(NotImplementedError, match="products of kernels"):
        EQ().periodic(1.0) * EQ()

    class Opaque(K.Kernel):
        pass

    with pytest.raises(NotImplementedError, match="periodic is implemented for sums of primitive kernels"):
        Opaque().periodic(1.0)
    with pytest.raises(NotImplementedError):
        EQ().stretch([1.0, 2.0]).periodic(1.0)
    with pytest.raises(NotImplementedError):
        EQ().periodic(1.0).stretch([1.0, 2.0])
    for bad in (0.0, -2.0, [1.0, -1.0], torch.tensor([1.0, 0.0])):
        with pytest.raises(ValueError, match="positive"):
            EQ().periodic(bad)


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def test_abi_of_the_entries_with_shapes():
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"#define\s+GPK_K_RQ\s+6\b", text) and _native.K_RQ == 6
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__ as g

        g.build()
    lib = _native.load()
    assert lib.gpk_version() >= 104
    with open(os.path.join(ROOT, "include", "gpk.h")) as f:
        whole = f.read()
    # one entry per operation: `shapes` directly behind `inv_ls` (kinds, [variances,] inv_ls, shapes, nterms), no twin with a suffix
    for base, at in (("gpk_kmat", 4), ("gpk_kdiag", 4), ("gpk_kmat_vjp", 3), ("gpk_kmat_vjp_dense", 4)):
        old = base + "_s"
        assert not re.search(r"\b" + old + r"\b", whole), f"{old} is still named in include/gpk.h"
        assert old not in _native.SIGNATURES and not hasattr(lib, old)
        decl = re.search(r"\b" + base + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert decl[at - 1].split()[-1] == "inv_ls" and decl[at].split() == ["const", "double*", "shapes"], decl[: at + 2]
        argtypes = _native.SIGNATURES[base][1]
        assert argtypes[at - 1] is _native._p_dbl and argtypes[at] is _native._p_dbl and argtypes[at + 1] is _native._c_int
        assert len(argtypes) == len(decl) and hasattr(lib, base)
