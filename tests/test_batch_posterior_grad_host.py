"""Gradients through BATCHED posterior means and marginal variances (``x`` (B, N, D), shared hyper-parameters;
``autograd._BatchedPosteriorMarginals``): the host logic on a test-local NumPy backend -- ``TransposedSolveOracle`` with batched
``kmat`` / ``tri_solve_t_``, the ``"rq"`` kind, ``kmat_vjp_dense_batch`` as the unbatched reduction looped over the entries, and a
record of the calls.  Checked against torch autograd through the pure-torch dense formula entry by entry (1e-8) and against central
finite differences (``tests/batch_posterior_cases.py``).  The last test is the host part of ``tests/test_vjp_batch_kernels_gpu.py``: its
cases tell two entries apart."""
import numpy as np
import pytest
import torch

import stheno_amd as st
from stheno_amd import ops

from . import vjp_batch_cases as VC
from . import vjp_reference as R
from .batch_posterior_cases import run_case
from .conftest import _np
from .test_map_groups_grad_host import GroupsOracle, _profile, _q
from .test_posterior_grad_host import TransposedSolveOracle

B, N, NS, D = 3, 12, 5, 2


class BatchOracle(TransposedSolveOracle):
    """``TransposedSolveOracle`` for a leading batch dimension: ``kmat`` and ``tri_solve_t_`` entry by entry (with the ``"rq"`` kind),
    ``kmat_vjp_dense_batch`` = the unbatched reduction looped over the entries; ``calls``: the backend calls in the order made."""

    _shapes, _dense = GroupsOracle._shapes, GroupsOracle._dense

    def __init__(self):
        self.calls = []

    def _kmat2(self, terms, x, y, diag_add, diag_vec):
        """One entry: the inherited kernel matrix, or -- a table with ``"rq"`` -- ``GroupsOracle``'s profiles."""
        if terms.shapes is None:
            return super().kmat(terms, x, y, diag_add=diag_add, diag_vec=diag_vec)
        a = _np(x)
        b = a if y is None else _np(y)
        k = np.zeros((a.shape[0], b.shape[0]))
        for (kind, v, s), shp in zip(terms.terms, self._shapes(terms)):
            k += v * _profile(kind, _q(kind, a, b, s), shp)[0]
        if y is None:
            k[np.diag_indices(a.shape[0])] += diag_add + (0.0 if diag_vec is None else _np(diag_vec))
        return self._t(k, x)

    def kmat(self, terms, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        self.calls.append("kmat")
        if x.dim() == 3 or (y is not None and y.dim() == 3):
            nb = x.shape[0] if x.dim() == 3 else y.shape[0]
            x = x if x.dim() == 3 else x.expand(nb, *x.shape)
            y = y if (y is None or y.dim() == 3) else y.expand(nb, *y.shape)
            dv = None if diag_vec is None else diag_vec.reshape(x.shape[0], -1)
            res = torch.stack([self._kmat2(terms, x[e], None if y is None else y[e], diag_add, None if dv is None else dv[e])
                               for e in range(x.shape[0])])
        else:
            res = self._kmat2(terms, x, y, diag_add, diag_vec)
        if out is not None:
            out.copy_(out + res if accumulate else res)
            return out
        return res

    def tri_solve_t_(self, l, dinv_sb, sb, b):
        self.calls.append("tri_solve_t_")
        L, Bm = np.tril(_np(l)), _np(b)
        b.copy_(self._t(np.linalg.solve(np.swapaxes(L, -1, -2), Bm), b))
        return b

    def _reduce(self, terms, x, y, g, colscale, w, b, want_colsum, want_gradx):
        Ge = _np(g).copy()
        if colscale is not None:
            Ge = Ge * _np(colscale)[None, :]
        if w is not None:
            Ge = Ge + _np(w)[:, None] * _np(b)[None, :]
        return self._dense(terms, x, y, Ge, want_colsum, want_gradx)

    def _reduce_any(self, terms, x, y, g, colscale, w, b, want_colsum, want_gradx):
        """The inherited unbatched reduction, or -- a table with ``"rq"`` -- ``GroupsOracle``'s."""
        if terms.shapes is None:
            return super().kmat_vjp_dense(terms, x, y, g, colscale, w, b, want_colsum=want_colsum, want_gradx=want_gradx)
        return self._reduce(terms, x, y, g, colscale, w, b, want_colsum, want_gradx)

    def kmat_vjp_dense(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        self.calls.append("kmat_vjp_dense")
        return self._reduce_any(terms, x, y, g, colscale, w, b, want_colsum, want_gradx)

    def kmat_vjp(self, terms, x, kinv, alpha, g):
        self.calls.append("kmat_vjp")
        return super().kmat_vjp(terms, x, kinv, alpha, g)

    def kmat_vjp_dense_batch(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        self.calls.append("kmat_vjp_dense_batch")
        terms.c_arrays()                                   # (one table for the whole batch: a per-batch one is refused here)
        assert x.dim() == y.dim() == g.dim() == 3 and tuple(g.shape) == (x.shape[0], x.shape[1], y.shape[1])
        at = lambda t, e: None if t is None else t[e]      # noqa: E731
        outs = [self._reduce_any(terms, x[e], y[e], g[e], at(colscale, e), at(w, e), at(b, e), want_colsum, want_gradx) for e in range(x.shape[0])]
        return tuple(None if outs[0][i] is None else torch.stack([o[i] for o in outs]) for i in range(3))


def _recorded(name):
    base = getattr(TransposedSolveOracle, name)

    def method(self, *args, **kw):
        self.calls.append(name)
        return base(self, *args, **kw)

    return method


for _name in ("gemm", "gemv", "scale_cols_", "symmetrize_", "copy", "colreduce", "tri_solve_", "potrf_"):
    setattr(BatchOracle, _name, _recorded(_name))


@pytest.fixture()
def be():
    backend = BatchOracle()
    prev = ops.set_backend(backend)
    yield backend
    ops.set_backend(prev)


KERNELS = [("eq",), ("eq", "linear"), ("matern52", "matern12"), "rq"]


@pytest.mark.parametrize("kinds", KERNELS, ids=str)
@pytest.mark.parametrize("loss", ["mean", "var", "ucb"])
def test_batched_posterior_marginal_gradients(be, kinds, loss):
    run_case(kinds, loss, nb=B, n=N, ns=NS, d=D, fd=True)
    assert "kmat_vjp" not in be.calls and "kmat_vjp_dense" not in be.calls and "kmat_vjp_dense_batch" in be.calls


@pytest.mark.parametrize("kinds", KERNELS, ids=str)
def test_per_point_noise(be, kinds):
    run_case(kinds, "ucb", nb=B, n=N, ns=NS, d=D, per_point=True, fd=True)


@pytest.mark.parametrize("opts", [dict(ard=True), dict(kinds="two_groups"), dict(shared_x=True), dict(pred_noise=True), dict(mean_fn=False),
                                  dict(logpdf_first=True), dict(shared_x=True, per_point=True, ard=True), dict(repeat=True)], ids=str)
def test_options(be, opts):
    opts = dict(opts)
    run_case(opts.pop("kinds", ("eq", "linear")), "ucb", nb=B, n=N, ns=NS, d=D, **opts)


@pytest.mark.parametrize("call,loss", [("mean", "mean"), ("var", "var"), ("bounds", "ucb"), ("auto", "ucb")])
def test_every_entry_point(be, call, loss):
    run_case(("eq", "matern12"), loss, nb=B, n=N, ns=NS, d=D, call=call, per_point=True)


def _backward_calls(be, nb, loss):
    g = torch.Generator().manual_seed(1)
    x, xs = (torch.randn((nb, k, D), generator=g, dtype=torch.float64).requires_grad_() for k in (N, NS))
    y = torch.randn((nb, N, 1), generator=g, dtype=torch.float64)
    v, l = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (1.3, 0.9))
    f = st.GP(v * st.EQ().stretch(l) + st.Matern52().stretch(torch.tensor([1.0, 2.0], dtype=torch.float64)))
    mean, var = (f | (f(x, 0.1), y))(xs).marginals()
    total = mean.sum() if loss == "mean" else (mean + 2 * var.sqrt()).sum()
    be.calls.clear()
    total.backward()
    assert all(t.grad is not None and bool(t.grad.abs().sum() > 0) for t in (x, xs, v, l))
    return list(be.calls)


@pytest.mark.parametrize("loss", ["mean", "ucb"])
def test_backend_calls_of_a_backward_do_not_depend_on_the_batch(be, loss):
    small, large = _backward_calls(be, 2, loss), _backward_calls(be, 5, loss)
    assert small == large
    assert "kmat_vjp" not in small and "kmat_vjp_dense" not in small
    assert small.count("kmat_vjp_dense_batch") == 6       # two groups x ((x, xs), (xs, x), (x, x))
    # alpha and (mean only) beta, or alpha and B; the rank-two update, and (with a variance cotangent) B diag(gs) B^T in front of it
    assert small.count("tri_solve_t_") == 2 and small.count("gemm") == (2 if loss == "ucb" else 1)


def _batch_data(d=D, grad_xs=False):
    g = torch.Generator().manual_seed(2)
    x = torch.randn((B, N, d), generator=g, dtype=torch.float64)
    xs = torch.randn((B, NS, d), generator=g, dtype=torch.float64).requires_grad_(grad_xs)
    return x, xs, torch.randn((B, N, 1), generator=g, dtype=torch.float64)


def test_nothing_learnable_leaves_no_node(be):
    x, xs, y = _batch_data()
    f = st.GP(1.5 * st.EQ().stretch(0.8))
    mean, var = (f | (f(x, 0.1), y))(xs).marginals()
    assert not mean.requires_grad and not var.requires_grad and "kmat_vjp_dense_batch" not in be.calls


def test_per_batch_parameter_stays_refused(be):
    x, xs, y = _batch_data()
    v = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64).reshape(B, 1, 1).requires_grad_()
    f = st.GP(v * st.EQ())
    fdd = (f | (f(x, 0.1), y))(xs)
    with pytest.raises(NotImplementedError, match="per-batch hyper-parameters"):
        fdd.marginals()
    # ... and without a gradient on it the call stays the plain path: values, no node
    f = st.GP(v.detach() * st.EQ())
    xs2 = xs.clone().requires_grad_()
    assert not (f | (f(x, 0.1), y))(xs2).mean.requires_grad


def test_nine_dimensions_are_refused_before_any_launch(be):
    x, xs, y = _batch_data(9, grad_xs=True)
    f = st.GP(st.EQ())
    fdd = (f | (f(x, 0.1), y))(xs)
    be.calls.clear()
    with pytest.raises(NotImplementedError, match="at most 8 input dimensions"):
        fdd.mean
    assert be.calls == []


# ---- the host part of tests/test_vjp_batch_kernels_gpu.py ------------------------------------------------------------------------
@pytest.mark.parametrize("case", VC.CASES + [VC.WALK], ids=lambda c: c["id"])
def test_exchanged_entries_move_every_checked_output_past_the_bound(case):
    """Were two entries' inputs exchanged (a wrong batch stride, a wrong entry's output block), every checked output of either entry
    would move by more than four times the bound at c = 50, in both dtypes."""
    for a, b in ((0, 1), (1, 2), (0, 2)):
        ra, rb = VC.entry(case, a)[1], VC.entry(case, b)[1]
        for k in VC.outputs(case):
            for mine, other in ((ra, rb), (rb, ra)):
                val, ab = mine[k]
                moved = np.abs(val - other[k][0]) / np.where(ab > 0, ab, np.inf)
                assert float(np.max(moved)) / float(R.EPS["float32"]) > 4 * 50, (k, a, b)
