"""Gradients through posteriors across processes (``autograd._BlockPosteriorMarginals``, ``learnable._block_marginals``) -- the
host logic on a NumPy backend, against the dense torch reference of ``tests/block_posterior_cases.py``: a component of a sum, two
observed processes, values and slopes observed together, a slope predicted from values, predictive noise; the values under
``torch.no_grad()``; the two refusals."""
import numpy as np
import pytest
import torch

import stheno_amd as st
from stheno_amd import kernels as K
from stheno_amd import learnable as L
from stheno_amd import ops

from . import block_posterior_cases as C


class CountingOracle(C.BlockOracle):
    """Counts everything that would be a launch."""

    def __init__(self):
        self.calls = 0

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if callable(attr) and not name.startswith("_") and name != "calls":
            object.__setattr__(self, "calls", object.__getattribute__(self, "calls") + 1)
        return attr


@pytest.fixture()
def block_backend():
    be = CountingOracle()
    prev = ops.set_backend(be)
    yield be
    ops.set_backend(prev)


def _graph(fn, seen):
    """The names of the autograd nodes behind ``fn``."""
    if fn is not None and type(fn).__name__ + str(id(fn)) not in seen:
        seen.add(type(fn).__name__ + str(id(fn)))
        for nxt, _ in fn.next_functions:
            _graph(nxt, seen)
    return seen


@pytest.mark.parametrize("case", C.CASES)
def test_gradients_against_the_dense_reference(block_backend, case):
    C.check_case(case, C.HOST_SIZES)


def test_the_block_path_is_what_runs(block_backend):
    """The marginals of a component of a sum come out of ONE node of the block function, for the mean and the variance together."""
    P = C.leaves("decomposition", C.HOST_SIZES)
    mean, var = C.ours("decomposition", P)

    for out in (mean, var):
        assert any("_BlockPosteriorMarginals" in name for name in _graph(out.grad_fn, set()))


def test_one_process_case_stays_on_its_own_function(block_backend):
    rng = np.random.default_rng(0)
    x, y, xs = (torch.tensor(a) for a in (rng.standard_normal((20, 2)), rng.standard_normal((20, 1)), rng.standard_normal((5, 2))))
    v = torch.tensor(1.2, dtype=torch.float64, requires_grad=True)
    f = st.GP(v * st.EQ())
    mean, _ = (f | (f(x, 0.1), y))(xs).marginals()
    nodes = _graph(mean.grad_fn, set())
    assert any(name.startswith("_PosteriorMarginals") for name in nodes) and not any("_BlockPosteriorMarginals" in name for name in nodes)


def test_nothing_learnable_keeps_the_plain_path(block_backend):
    P = {k: v.detach() for k, v in C.leaves("values_slopes", C.HOST_SIZES).items()}
    mean, var = C.ours("values_slopes", P)
    assert mean.grad_fn is None and var.grad_fn is None


def test_block_groups():
    k = 1.5 * st.EQ().stretch(0.7) + 0.5 * st.Matern52()
    (g,) = L._block_groups(k)
    assert g[:3] == (1.0, None, None) and g[4] is None
    (g,) = L._block_groups(k.diff(1, None))
    assert g[:3] == (1.0, 1, None) and g[3].terms() == k.terms()
    (g,) = L._block_groups(reversed(k.diff(1, None)))
    assert g[:3] == (1.0, None, 1)
    g2 = L._block_groups(2.0 * k.diff(0) + k)
    assert [(s, a, b) for s, a, b, *_ in g2] == [(2.0, 0, 0), (1.0, None, None)]
    assert L._block_groups(K.ZeroKernel()) == []
    ard = st.EQ().stretch(torch.tensor([0.5, 2.0], dtype=torch.float64))
    (g,) = L._block_groups(ard.diff(1))
    assert g[1:3] == (1, 1) and isinstance(g[4], K._ScaleMap)
    assert float(L._group_factor(*g[:3], g[4])) == 0.25                     # 1 / l_1^2 rides in the variances
    assert L._block_groups(st.EQ() * 1.0 + K.Reversed(K.PosteriorKernel(k, k, k, None, None))) is None


def _slopes_model(**grad):
    rng = np.random.default_rng(9)
    t = lambda a, name: torch.tensor(a, dtype=torch.float64, requires_grad=grad.get(name, False))      # noqa: E731
    x1, x2, xs = t(rng.uniform(-1, 1, (12, 2)), "x1"), t(rng.uniform(-1, 1, (9, 2)), "x2"), t(rng.uniform(-1, 1, (5, 2)), "xs")
    y1, y2 = t(rng.standard_normal((12, 1)), "y1"), t(rng.standard_normal((9, 1)), "y2")
    scales = t(np.array([0.8, 1.3]), "scales")
    with st.Measure() as prior:
        f = st.GP(st.EQ().stretch(scales) if grad.get("ard") or grad.get("scales") else st.EQ().stretch(0.9))
        df = f.diff(1)
    post = prior | ((f(x1, 0.1), y1), (df(x2, 0.1), y2))
    return post, f, df, xs


def test_refusals_come_before_any_launch(block_backend):
    # a gradient to the test inputs through a mixed block: a derivative predicted from observed derivatives
    post, f, df, xs = _slopes_model(xs=True, y1=True)
    before = block_backend.calls
    with pytest.raises(NotImplementedError, match="inputs of a mixed derivative block"):
        post(df)(xs).marginals()
    assert block_backend.calls == before
    # ... and the inputs of derivative observations
    post, f, df, xs = _slopes_model(x2=True)
    before = block_backend.calls
    with pytest.raises(NotImplementedError, match="inputs of a mixed derivative block"):
        post(f)(xs).marginals()
    assert block_backend.calls == before
    # learnable per-dimension length scales under a derivative
    post, f, df, xs = _slopes_model(scales=True)
    before = block_backend.calls
    with pytest.raises(NotImplementedError, match="per-dimension length scales under a derivative"):
        post(f)(xs).marginals()
    assert block_backend.calls == before
    # the same model with everything fixed but y: served
    post, f, df, xs = _slopes_model(y1=True, ard=True)
    mean, var = post(f)(xs).marginals()
    assert mean.requires_grad


def test_fixed_per_dimension_scales_under_a_derivative(block_backend):
    """Behind fixed per-dimension length scales the chain-rule factors ride in the variances: gradient with respect to ``y`` and ``xs``
    against finite differences of the plain path's values."""
    post, f, df, xs = _slopes_model(y1=True, xs=True, ard=True)
    w = torch.linspace(0.5, 1.5, 5, dtype=torch.float64)
    mean, var = post(f)(xs).marginals()
    ((mean.reshape(-1) + 2 * torch.sqrt(var.reshape(-1))) * w).sum().backward()
    base = xs.detach().clone()
    for idx in ((0, 0), (3, 1)):
        vals = []
        for h in (1e-6, -1e-6):
            z = base.clone()
            z[idx] += h
            with torch.no_grad():
                m, v = post(f)(z).marginals()
            vals.append(float(((m.reshape(-1) + 2 * torch.sqrt(v.reshape(-1))) * w).sum()))
        fd = (vals[0] - vals[1]) / 2e-6
        assert abs(float(xs.grad[idx]) - fd) <= 1e-6 * max(abs(fd), 1.0), (idx, float(xs.grad[idx]), fd)
