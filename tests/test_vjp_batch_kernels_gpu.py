"""The batched explicit-cotangent kernel gradient (``gpk_kmat_vjp_dense_batch``, ``stheno_amd/csrc/gpk_vjp.hip``) called directly --
through ``HipBackend.kmat_vjp_dense_batch`` and through the C entry -- and compared entry by entry and element by element with the
extended-precision reference of ``tests/vjp_reference.py``, in fp64 and fp32: tile edges, padded leading dimensions, batch strides
larger than packed (entries carved out of NaN-filled buffers), shared inputs (``sx = 0``), the all-zero cotangent operand
(``ldg = sg = 0``), outputs prefilled with a sentinel, a launch whose workgroups walk several column tiles, the bits of the unbatched
entry at ``batch = 1`` and the argument errors.

Acceptance, for every output element: ``|got - ref| <= c * eps(dtype) * absum`` with ``c`` the constant the unbatched entry is held to
(``test_vjp_kernels_gpu.BOUND``: the batched launch runs the same element program) where the worst ratio measured with these cases on
an MI355X stays below it, else twice that worst ratio; never above 50 (``profiles/README.md``, "Batched kernel-gradient launch,
element by element").  ``tests/test_batch_posterior_grad_host.py`` shows that exchanging two entries' inputs moves every checked
output by more than four times the bound at c = 50."""
import ctypes

import numpy as np
import pytest
import torch

from stheno_amd import _native, ops

from . import vjp_batch_cases as C
from . import vjp_reference as R
from .test_vjp_kernels_gpu import BOUND as UNBATCHED

pytestmark = pytest.mark.gpu

CAP = 50
#: per output and dtype: the unbatched constant (measured worst ratios of these cases: S 1.17 / 1.72, colsum 1.21 / 1.85,
#: gradx 1.41 / 1.39 in fp64 / fp32 -- all below it)
BOUND = {(out, dtype): UNBATCHED[("dense", out, dtype)] for out in ("S", "colsum", "gradx") for dtype in ("float64", "float32")}
assert max(BOUND.values()) <= CAP
DTYPES = {"float64": torch.float64, "float32": torch.float32}
NAN = float("nan")


def _t(a, dtype):
    return torch.as_tensor(np.array(a), dtype=DTYPES[dtype], device="cuda")


def _carve(a, dtype, pad):
    """``a`` (B, ...) as a view into a NaN-filled buffer: one entry more, ``pad`` elements more along every other axis, offset by one."""
    t = _t(a, dtype)
    buf = torch.full((t.shape[0] + 1,) + tuple(s + pad for s in t.shape[1:]), NAN, dtype=t.dtype, device="cuda")
    view = buf[(slice(0, t.shape[0]),) + tuple(slice(1, 1 + s) for s in t.shape[1:])]
    view.copy_(t)
    assert view.stride(0) > int(np.prod(t.shape[1:])) and view.stride(-1) == 1
    return view


def operands(case, dtype, entries):
    """The device operands of a case over the given entries, in the case's layout."""
    inps = [C.entry(case, e)[0] for e in entries]
    nb, n, m = len(entries), case["n"], case["m"]
    stack = lambda k: None if inps[0][k] is None else np.stack([i[k] for i in inps])      # noqa: E731
    carved = case["layout"] == "carved"
    put = (lambda a: None if a is None else _carve(a, dtype, 3)) if carved else (lambda a: None if a is None else _t(a, dtype))
    x = _t(inps[0]["x"], dtype)[None].expand(nb, n, case["d"]) if case["shared_x"] else put(stack("x"))
    y, cs, w, b = put(stack("y")), put(stack("colscale")), put(stack("w")), put(stack("b"))
    if case["cot"].startswith("zero"):
        g = torch.zeros((1, 1, m), dtype=DTYPES[dtype], device="cuda").expand(nb, n, m)
    elif case["layout"] == "padded":
        buf = torch.full((nb, n, m + 5), NAN, dtype=DTYPES[dtype], device="cuda")
        g = buf[:, :, :m]
        g.copy_(_t(stack("g"), dtype))
    else:
        g = put(stack("g"))
    return x, y, g, cs, w, b


def _ratios(case, dtype, got, e):
    """Worst ratio per output of entry ``e`` (``got``: that entry's outputs)."""
    ref = C.entry(case, e)[1]
    out = {}
    for k in C.outputs(case):
        val, ab = ref[k]
        gk = got[k].cpu().numpy()
        assert gk.shape == np.shape(val), (k, gk.shape, np.shape(val))
        out[k] = float(np.max(R.ratios(gk, val, ab, dtype)))
    return out


def _accept(case, dtype, worst):
    print(f"batch {case['id']} {dtype}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BOUND[(k, dtype)], (k, v)


def _kterms(case):
    return ops.KTerms(*R.split_terms(R.TERMSETS[case["terms"]]))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_batched_launch_entry_by_entry_element_by_element(hip_backend, case, dtype):
    x, y, g, cs, w, b = operands(case, dtype, range(C.B))
    S, colsum, gradx = hip_backend.kmat_vjp_dense_batch(_kterms(case), x, y, g, cs, w, b, want_colsum=True, want_gradx=case["gradx"])
    assert (gradx is not None) == case["gradx"] and S.shape[0] == colsum.shape[0] == C.B
    worst = {}
    for e in range(C.B):
        got = {"S": S[e], "colsum": colsum[e], "gradx": None if gradx is None else gradx[e]}
        for k, v in _ratios(case, dtype, got, e).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _accept(case, dtype, worst)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_workgroups_walk_several_column_tiles(hip_backend, dtype):
    """600 entries of 2 row tiles x 4 column tiles: fewer chunks than column tiles, so a workgroup walks two tiles with its ``gradx``
    accumulators in registers.  Three data sets assigned cyclically: every entry equals its data set's first entry bit for bit, and
    those lie within the bound."""
    case, nb = C.WALK, C.WALK_BATCH
    rt, nc = ctypes.c_int64(), ctypes.c_int64()
    assert hip_backend.lib.gpk_kmat_vjp_dense_batch_grid(case["n"], case["m"], nb, ctypes.byref(rt), ctypes.byref(nc)) == 0
    ctiles = -(-case["m"] // R.TILE)
    assert rt.value == -(-case["n"] // R.TILE) and nc.value < ctiles, "chunks hold one tile: the case no longer covers the tile loop"
    idx = torch.arange(nb, device="cuda") % 3
    x, y, g, cs, w, b = (t[idx] for t in operands(case, dtype, range(3)))
    S, colsum, gradx = hip_backend.kmat_vjp_dense_batch(_kterms(case), x, y, g, cs, w, b, want_colsum=True, want_gradx=True)
    for out in (S, colsum, gradx):
        assert torch.equal(out, out[:3][idx]), "entries of one data set differ"
    worst = {}
    for e in range(3):
        for k, v in _ratios(case, dtype, {"S": S[e], "colsum": colsum[e], "gradx": gradx[e]}, e).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _accept(case, dtype, worst)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _direct(lib, case, dtype, ops_, nb, *, unbatched=False, sentinel=-12345.0, tail=64):
    """The C entry on the operands ``ops_``: ``(status, partial, colsum, gradx, tails)`` with the outputs prefilled with ``sentinel``
    and ``tail`` more elements behind each."""
    x, y, g, cs, w, b = ops_
    T = DTYPES[dtype]
    terms = _kterms(case)
    kinds, var, ils, nt = terms.c_arrays()
    n, m, d = case["n"], case["m"], case["d"]
    rt, nc = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gpk_kmat_vjp_dense_batch_grid(n, m, nb, ctypes.byref(rt), ctypes.byref(nc)) == 0
    rt, nc = rt.value, nc.value
    W = (3 if terms.shapes is not None else 2) * _native.MAX_TERMS + 1
    sizes = (nb * rt * nc * W, nb * rt * m, nb * nc * n * d)
    bufs = [torch.full((s + tail,), sentinel, dtype=T, device="cuda") for s in sizes]
    dt = _native.GPK_F64 if T == torch.float64 else _native.GPK_F32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bs = (lambda t: 0 if t is None or nb == 1 else t.stride(0))
    if unbatched:
        st = lib.gpk_kmat_vjp_dense(dt, kinds, var, ils, terms.c_shapes(), nt, _p(x), n, x.stride(1), _p(y), m, y.stride(1), d, _p(g), g.stride(1),
                                    _p(cs), _p(w), _p(b), *(_p(t) for t in bufs), stream)
    else:
        st = lib.gpk_kmat_vjp_dense_batch(dt, kinds, var, ils, terms.c_shapes(), nt, _p(x), n, x.stride(1), bs(x), _p(y), m, y.stride(1), bs(y), d,
                                          _p(g), g.stride(1), bs(g), _p(cs), bs(cs), _p(w), bs(w), _p(b), bs(b), *(_p(t) for t in bufs), nb, stream)
    return st, [t[:s] for t, s in zip(bufs, sizes)], [t[s:] for t, s in zip(bufs, sizes)]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", [C.CASES[4], C.CASES[7]], ids=lambda c: c["id"])
def test_outputs_are_packed_and_nothing_is_written_behind_them(hip_backend, case, dtype):
    """Carved inputs, outputs prefilled: every element of the packed outputs is written, nothing behind them, and no NaN of the
    buffers around the views reaches an output."""
    st, outs, tails = _direct(hip_backend.lib, case, dtype, operands(case, dtype, range(C.B)), C.B)
    assert st == 0
    for o, t in zip(outs, tails):
        assert bool((o != -12345.0).all()) and bool(torch.isfinite(o).all()) and bool((t == -12345.0).all())


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", [C.CASES[2], C.CASES[7]], ids=lambda c: c["id"])
def test_batch_of_one_writes_the_bits_of_the_unbatched_entry(hip_backend, case, dtype):
    ops_ = operands(case, dtype, [1])
    a = _direct(hip_backend.lib, case, dtype, ops_, 1)
    b = _direct(hip_backend.lib, case, dtype, ops_, 1, unbatched=True)
    assert a[0] == 0 and b[0] == 0
    bits = lambda t: t.cpu().view(torch.int64 if t.dtype == torch.float64 else torch.int32)   # noqa: E731
    for u, v in zip(a[1], b[1]):
        assert bool((u != -12345.0).all()) and torch.equal(bits(u), bits(v))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_argument_errors(hip_backend, dtype):
    lib, T = hip_backend.lib, DTYPES[dtype]
    dt = _native.GPK_F64 if T == torch.float64 else _native.GPK_F32
    kinds, var, ils, nt = ops.KTerms([("eq", 1.0, 1.0)]).c_arrays()
    z = torch.zeros((64,), dtype=T, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(d, gradx, batch):
        return lib.gpk_kmat_vjp_dense_batch(dt, kinds, var, ils, None, nt, _p(z), 2, d, 0, _p(z), 2, d, 0, d, _p(z), 2, 0, None, 0, None, 0, None, 0,
                                            _p(z), None, _p(z) if gradx else None, batch, stream)

    assert call(3, True, 65536) == -28                  # the grid's third dimension
    assert call(9, True, 1) == -12                      # d/dX past eight dimensions
    assert call(9, False, 1) == 0
    assert call(3, True, 0) == 0 and call(3, True, -1) == 0          # an empty problem, behind the checks
    assert call(9, True, 0) == -12
    rt, nc = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gpk_kmat_vjp_dense_batch_grid(130, 200, 1, ctypes.byref(rt), ctypes.byref(nc)) == 0 and (rt.value, nc.value) == (3, 4)
    assert lib.gpk_kmat_vjp_dense_batch_grid(130, 200, 600, ctypes.byref(rt), ctypes.byref(nc)) == 0 and (rt.value, nc.value) == (3, 2)
    assert lib.gpk_kmat_vjp_dense_batch_grid(130, 200, 4000, ctypes.byref(rt), ctypes.byref(nc)) == 0 and (rt.value, nc.value) == (3, 1)
    # the op refuses a per-batch term table and a gradient past eight dimensions
    x = torch.zeros((2, 5, 9), dtype=T, device="cuda")
    g = torch.ones((2, 5, 5), dtype=T, device="cuda")
    with pytest.raises(RuntimeError, match="gpk_kmat_vjp_dense_batch"):
        hip_backend.kmat_vjp_dense_batch(ops.KTerms([("eq", 1.0, 1.0)]), x, x, g, want_gradx=True)
    per_batch = ops.KTerms([("eq", torch.tensor([1.0, 2.0], dtype=torch.float64), 1.0)])
    with pytest.raises(NotImplementedError, match="per-batch hyper-parameters"):
        hip_backend.kmat_vjp_dense_batch(per_batch, x, x, g)
