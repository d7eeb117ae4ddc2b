"""The term table of a kernel (``Kernel._table``) and its four public views ``terms()`` / ``tensor_terms()`` / ``shapes()`` /
``tensor_shapes()``: the views against values written out by hand, the arithmetic of the float views under fp32 tensor parameters, one
visit per leaf and per view, and the predicate "does this table carry a gradient" (``autograd.table_requires_grad``).  No GPU."""
import pytest
import torch

from stheno_amd import kernels as K, learnable as autograd
from stheno_amd.torch import EQ, RQ, Delta, Linear, ZeroKernel


def leaf(value, dtype=torch.float64):
    return torch.tensor(value, dtype=dtype, requires_grad=True)


def check_views(k, terms, shapes, tensor_terms=None, tensor_shapes=None):
    """Float views by ``==``; tensor views entry by entry, tensors by identity."""
    assert k.terms() == terms and k.shapes() == shapes
    for got, want in ((k.tensor_terms(), terms if tensor_terms is None else tensor_terms),
                      (k.tensor_shapes(), shapes if tensor_shapes is None else tensor_shapes)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            if isinstance(w, tuple):
                assert len(g) == len(w) and all((a is b) if torch.is_tensor(b) else (not torch.is_tensor(a) and a == b) for a, b in zip(g, w))
            else:
                assert (g is w) if (torch.is_tensor(w) or w is None) else (not torch.is_tensor(g) and g == w)


# ---------------------------------------------------------------------------------------------
# 1: the views against literals
# ---------------------------------------------------------------------------------------------
def test_views_of_plain_kernels():
    check_views(EQ(), [("eq", 1.0, 1.0)], [None])
    check_views(2.0 * RQ(0.3), [("rq", 2.0, 1.0)], [0.3])
    check_views(Delta(1e-3).stretch(4.0) * 0.5, [("delta", 0.5, 4.0)], [1e-3])
    both = [("eq", 1.0, 1.0), ("linear", 1.0, 1.0)]
    check_views(reversed(EQ() + Linear()), both, [None, None])
    check_views(K.Reversed(EQ() + Linear()), both, [None, None])
    check_views(ZeroKernel(), [], [])


def test_views_keep_the_callers_tensors():
    a = torch.tensor(0.7, dtype=torch.float64)
    check_views(RQ(a) + EQ(), [("rq", 1.0, 1.0), ("eq", 1.0, 1.0)], [0.7, None], tensor_shapes=[a, None])
    # the same tensor twice: one term; another tensor of the same value: two (learnable parameters are the same only by identity)
    check_views(RQ(a) + RQ(a), [("rq", 2.0, 1.0)], [0.7], tensor_shapes=[a])
    b = torch.tensor(0.7)                                  # fp32: 0.7 rounds to the double below
    check_views(RQ(a) + RQ(b), [("rq", 1.0, 1.0), ("rq", 1.0, 1.0)], [0.7, 0.699999988079071044921875], tensor_shapes=[a, b])
    c = torch.tensor(0.7, dtype=torch.float64)             # ... and of the same double: the float view merges, the tensor view does not
    k = RQ(a) + RQ(c)
    assert k.terms() == [("rq", 2.0, 1.0)] and k.shapes() == [0.7]
    assert k.tensor_terms() == [("rq", 1.0, 1.0), ("rq", 1.0, 1.0)] and k.tensor_shapes()[0] is a and k.tensor_shapes()[1] is c


def test_a_kernel_that_is_no_sum_of_primitives_has_no_views():
    for k in (EQ().diff(0), EQ().periodic(2.0), EQ().stretch([1.0, 2.0]) + EQ()):
        assert k.terms() is None and k.tensor_terms() is None and k.shapes() is None and k.tensor_shapes() is None
        assert k.tensor_table() is None


# ---------------------------------------------------------------------------------------------
# 2: the float views multiply in Python doubles, the tensor views in the tensors' dtype
# ---------------------------------------------------------------------------------------------
def test_float_views_multiply_in_doubles_under_fp32_parameters():
    v = leaf(0.1, torch.float32)
    k = 3.0 * (v * EQ())
    assert k.terms()[0][1] == float(v.detach()) * 3.0 == 0.1000000014901161193847656 * 3.0
    got = k.tensor_terms()[0][1]
    assert got.dtype == torch.float32 and got.requires_grad and torch.equal(got.detach(), (v * 3.0).detach())
    assert float(got.detach()) != k.terms()[0][1]                   # (the fp32 product rounds: the two views are NOT one converted into the other)

    s = leaf(0.1, torch.float32)
    k = EQ().stretch(s).stretch(3.0)
    assert k.terms()[0][2] == float(s.detach()) * 3.0
    got = k.tensor_terms()[0][2]
    assert got.dtype == torch.float32 and got.requires_grad and torch.equal(got.detach(), (s * 3.0).detach())
    assert float(got.detach()) != k.terms()[0][2]

    alpha = leaf(0.1, torch.float32)
    k = 2.0 * RQ(alpha).stretch(0.5)
    assert k.shapes() == [float(alpha.detach())] == [0.1000000014901161193847656]
    assert k.tensor_shapes()[0] is alpha and k.tensor_shapes()[0].dtype == torch.float32 and k.tensor_shapes()[0].requires_grad


# ---------------------------------------------------------------------------------------------
# 3: one visit per leaf
# ---------------------------------------------------------------------------------------------
@pytest.fixture()
def visits(monkeypatch):
    """Calls of the leaves' ``_table``, counted."""
    seen = []
    inner = K._Primitive._table

    def counted(self, conv):
        seen.append(self)
        return inner(self, conv)

    monkeypatch.setattr(K._Primitive, "_table", counted)
    return seen


def nested_sum():
    """Left-nested sum of eight ``EQ`` terms of distinct scales: nothing merges."""
    k = EQ().stretch(0.5)
    for i in range(1, 8):
        k = k + EQ().stretch(0.5 + 0.1 * i)
    return k


def test_every_view_visits_every_leaf_once(visits):
    k = nested_sum()
    for view in (k.terms, k.tensor_terms, k.shapes, k.tensor_shapes):
        del visits[:]
        assert len(view()) == 8
        assert len(visits) == 8 and len({id(p) for p in visits}) == 8       # (382 visits when every view of a sum asked two of its children's)


def test_one_evaluation_asks_for_the_table_twice(visits, oracle_backend):
    k = nested_sum()
    x = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)[:, None]
    del visits[:]
    assert k.pairwise(x).shape == (5, 5)
    assert len(visits) == 16          # `Sum.pairwise` asks whether it is a sum of primitives, `Kernel.pairwise` packs the table (before: 1146)
    del visits[:]
    assert k.elwise(x).shape == (5, 1)
    assert len(visits) == 16          # (before: 1146)


# ---------------------------------------------------------------------------------------------
# 4: does a table carry a gradient?
# ---------------------------------------------------------------------------------------------
def test_table_requires_grad():
    learnable = [leaf(0.5) * EQ(), EQ().stretch(leaf(0.5)), RQ(leaf(0.5)),
                 2.0 * EQ().stretch(0.5) + 0.3 * (leaf(0.5) * Linear()) + Delta()]
    for k in learnable:
        assert autograd.table_requires_grad(k.tensor_table()) and autograd.kernel_requires_grad(k)
    for k in (EQ(), 2.0 * EQ().stretch(0.5) + RQ(0.3) + 0.1 * Delta(1e-3), torch.tensor(0.5) * RQ(torch.tensor(0.5)), ZeroKernel(),
              Delta(torch.tensor(1e-3))):
        assert not autograd.table_requires_grad(k.tensor_table()) and not autograd.kernel_requires_grad(k)
    with torch.no_grad():
        for k in learnable:
            assert not autograd.table_requires_grad(k.tensor_table())
