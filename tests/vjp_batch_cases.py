"""The cases of the batched explicit-cotangent kernel gradient (``gpk_kmat_vjp_dense_batch``) that ``tests/test_vjp_batch_kernels_gpu.py``
runs on the device and ``tests/test_batch_posterior_grad_host.py`` checks for discrimination on the host.  Not collected by pytest.

An entry of a batched case is an unbatched dense case of ``tests/vjp_reference.py`` (its inputs from ``make_inputs`` under the id
``<case>-e<entry>``, its reference from ``dense``), so the batched launch is held entry by entry and element by element against the
reference the unbatched entry is held against.  ``B = 3`` entries; the options of a case:

* ``cot``: ``"plain"``, ``"scaled+rank1"``, or ``"zero+rank1"`` -- the all-zero cotangent operand read through ``ldg = sg = 0``;
* ``layout``: ``"packed"``, ``"padded"`` (a leading dimension 5 past ``m``) or ``"carved"`` (every input a view into a NaN-filled
  buffer, with leading dimensions and batch strides larger than packed: a read outside a view shows as NaN);
* ``shared_x``: the entries share one data set, read through ``sx = 0``.
"""
import numpy as np

from . import vjp_reference as R

B = 3


def _case(n, m, d, terms, cot, layout="packed", gradx=True, shared_x=False):
    name = f"n{n}-m{m}-d{d}-{terms}-{cot}-{layout}" + ("-x" if gradx else "") + ("-sx0" if shared_x else "")
    return dict(id=name, n=n, m=m, d=d, terms=terms, cot=cot, layout=layout, colsum=True, gradx=gradx, shared_x=shared_x)


CASES = [
    _case(1, 1, 1, "eq", "plain"),
    _case(1, 1, 8, "mix8rq", "scaled+rank1", "carved"),
    _case(63, 65, 3, "mix8", "plain", "padded"),
    _case(63, 65, 9, "mix8rq", "scaled+rank1", "carved", gradx=False),
    _case(65, 129, 8, "eq", "scaled+rank1", "carved"),
    _case(65, 129, 1, "mix8", "plain", shared_x=True),
    _case(65, 129, 3, "mix8rq", "zero+rank1"),
    _case(130, 200, 3, "mix8rq", "plain", "carved"),
    _case(130, 200, 8, "mix8", "scaled+rank1", "padded", shared_x=True),
    _case(130, 200, 9, "eq", "plain", "padded", gradx=False),
    _case(130, 200, 1, "eq", "zero+rank1", shared_x=True),
]

#: a workgroup of this launch walks two of the four column tiles: 600 entries x 2 row tiles leave two chunks (three data sets, cyclically)
WALK = _case(65, 200, 3, "mix8", "scaled+rank1")
WALK_BATCH = 600

_CACHE = {}


def entry(case, e):
    """``(inputs, reference)`` of entry ``e``: ``vjp_reference.make_inputs`` / ``dense`` (computed once per process, read-only)."""
    key = (case["id"], e)
    if key not in _CACHE:
        sub = dict(form="dense", id=f"{case['id']}-e{e}", n=case["n"], m=case["m"], d=case["d"], terms=case["terms"],
                   cot=case["cot"].replace("zero+", ""))
        inp = R.make_inputs(sub)
        if case["cot"].startswith("zero"):
            inp["g"] = np.zeros_like(inp["g"])
        if case["shared_x"] and e:
            inp["x"] = entry(case, 0)[0]["x"]
        ref = R.dense(inp["terms"], inp["x"], inp["y"], inp["g"], inp["colscale"], inp["w"], inp["b"])
        for a in list(inp.values()) + [v for pair in ref.values() for v in pair]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = (inp, ref)
    return _CACHE[key]


def outputs(case):
    return ("S", "colsum") + (("gradx",) if case["gradx"] else ())
