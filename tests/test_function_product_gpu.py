"""Processes times functions under ``any_backend``: the models of ``tests/test_function_product_host.py`` on the test-only oracle backend
(CPU) and on ``libgpk.so`` (MI355X) -- Bayesian linear regression against weight space, the algebra's values against the oracle, and the
GP-modulated network's log-density and gradients in fp64 at N = 200 on the GPU against the NumPy closed form.  Models, references and
bars: ``tests/function_product_cases.py``."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd.torch import EQ, Matern32

from oracle import gp_oracle as O

from . import function_product_cases as F
from . import map_groups_cases as C
from .conftest import T, _np


def test_blr_matches_weight_space(any_backend):
    x, y, xs = F.blr_data()
    w, cov, pm, pv, lml = F.blr_reference(x, y, xs)
    prior, slope, intercept, f = F.blr_model()
    C.assert_value("log marginal likelihood", float(f(T(x), F.NOISE).logpdf(T(y)[:, None])), lml)
    post = prior | (f(T(x), F.NOISE), T(y)[:, None])
    for name, p, i in (("slope", slope, 0), ("intercept", intercept, 1)):
        fdd = post(p)(T([0.0]))
        C.assert_value(f"{name} mean", float(fdd.mean), w[i])
        C.assert_value(f"{name} variance", float(_np(fdd.var.mat)[0, 0]), cov[i, i])
    mean, var = post(f)(T(xs)).marginals()
    C.assert_close("predictive mean", _np(mean).ravel(), pm)
    C.assert_close("predictive variances", _np(var).ravel(), pv)


def _fn(x):
    return torch.sin(x[..., 0]) + 0.5 * x[..., 1]


def _fn_np(x):
    return np.sin(x[..., 0]) + 0.5 * x[..., 1]


TERMS = [("eq", 1.3, 0.8), ("matern32", 0.4, 1.1)]


def test_values_of_the_product_and_a_sum_around_it(any_backend):
    rng = np.random.default_rng(3)
    x, xb = rng.standard_normal((150, 2)), rng.standard_normal((3, 40, 2))
    s, Kxx = _fn_np(x), O.kernel_matrix(TERMS, x, x)
    with st.Measure():
        f = st.GP(1.3 * EQ().stretch(0.8) + 0.4 * Matern32().stretch(1.1))
        g = f * st.ScaleFn(_fn)
        h = g + st.GP(0.7 * EQ())
    C.assert_close("var", _np(g(T(x)).var.mat), np.outer(s, s) * Kxx)
    C.assert_close("var_diag", _np(g(T(x)).var_diag), s * s * np.diag(Kxx))
    ref = np.outer(s, s) * Kxx + 0.7 * O.kernel_matrix([("eq", 1.0, 1.0)], x, x) + 0.1 * np.eye(len(x))
    C.assert_close("fn k_a fn + k_b + noise", np.tril(_np(h(T(x), 0.1).var.mat)), np.tril(ref))
    sb = _fn_np(xb)
    refb = np.stack([np.outer(sb[i], sb[i]) * O.kernel_matrix(TERMS, xb[i], xb[i]) for i in range(3)])
    C.assert_close("batch (3, N, 2)", _np(g(T(xb)).var.mat), refb)


@pytest.mark.gpu
def test_modulated_network_learns_on_the_gpu_as_the_closed_form_says(hip_backend):
    """fp64, N = 200: value and gradients with respect to both length scales, both variances, the noise and every net parameter against
    the host's closed form (finite differences, h = 1e-6) under the bar of ``tests/map_groups_cases.py``."""
    x, y = F.modulated_data(200)
    p = F.net_params()
    ref, fd = F.fd_reference(p, F.NET_NAMES, x, y)
    net = F.TanhNet(p, "cuda")
    f, a, b, prior, t = F.modulated_model(p, net, "cuda")
    dev = lambda v: torch.as_tensor(v, dtype=torch.float64, device="cuda")      # noqa: E731
    lp = f(dev(x), t["noise"]).logpdf(dev(y)[:, None])
    C.assert_value("logpdf", float(lp.detach()), ref)
    lp.backward()
    C.assert_close("d logpdf / d (l_a, l_b, v_a, v_b, noise, net)", F.net_grads(t, net), fd)
    with torch.no_grad():          # the posteriors of the pieces, values only
        post = prior | (f(dev(x), t["noise"]), dev(y)[:, None])
        for proc in (f, a, b):
            mean, var = post(proc)(dev(x[:20])).marginals()
            assert bool(torch.isfinite(mean).all()) and bool((var > -1e-9).all())
