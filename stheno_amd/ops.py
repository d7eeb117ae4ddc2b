"""Tensor-level ops of the GP hot path, backed by ``libgpk.so`` (HIP, gfx950).

Every function takes/returns ``torch.Tensor`` objects that live on a HIP device; the
tensors provide memory and the stream, ``libgpk.so`` does the arithmetic.  There is
no CPU implementation in this package: calling an op with a CPU tensor, or without
the built extension, raises.

``set_backend`` exists so that the host-side model logic can be unit-tested on a
machine without a GPU by injecting a checker backend from ``tests/`` (see
``tests/conftest.py``); nothing in the package ever installs another backend.
"""
import ctypes

import torch

from . import _native

__all__ = ["get_backend", "set_backend", "HipBackend", "KTerms"]

_KIND_IDS = {
    "eq": _native.K_EQ,
    "matern12": _native.K_MATERN12,
    "matern32": _native.K_MATERN32,
    "matern52": _native.K_MATERN52,
    "linear": _native.K_LINEAR,
    "const": _native.K_CONST,
    "rq": _native.K_RQ,
    "delta": _native.K_DELTA,
}

#: kinds with a shape parameter (``rq``: alpha of ``(1 + r^2 / (2 alpha))^(-alpha)``; ``delta``: epsilon of ``r^2 < epsilon``)
_SHAPED = ("rq", "delta")
#: ... of which these have a LEARNABLE one (``delta`` is piecewise constant in its epsilon: no gradient)
_LEARNABLE_SHAPE = ("rq",)
_SHAPE_NAME = {"rq": "alpha", "delta": "epsilon"}

#: Default Newton-Schulz step counts of :meth:`HipBackend.nuclear_norm`.  A singular value that has not reached 1 after k steps was
#: below about ``1.5^-(k - 8) |M|_F`` to begin with and costs at most its own size.  Emulated in the working dtype on Cholesky-factor
#: products (error of ``2 |M|_*`` relative to ``tr V1 + tr V2``): with noise >= 0.01, n <= 600, 30 steps reach
#: rounding level in both dtypes (7e-16 / 5e-8) where 20 leave up to 8e-3; the noise-free pair (jitter 1e-12 / 1e-6, smallest singular
#: value 8e-15 / 8e-9 of ``|M|_F``) goes 3e-4, 5e-6, 9e-8, 2e-9, 4e-11 at 20 ... 60 steps in fp64 and stalls at 2e-8 from 40 on in fp32.
NUCLEAR_ITERS_F64 = 60
NUCLEAR_ITERS_F32 = 40


def _per_batch_value(v):
    """A per-batch entry of a term table: a tensor with more than one element (``(B,)`` or ``(B, 1, 1)``)."""
    return torch.is_tensor(v) and v.numel() > 1


class KTerms:
    """A kernel as a sum of ``variance * kind(. / scale)`` terms (host-side descriptor).  ``shapes``: one entry per term, the shape
    parameter of the kinds that have one (``"rq"``: alpha > 0, ``"delta"``: epsilon > 0) and ``None`` for the others; ``self.shapes`` is ``None`` when no term
    has one -- the library then gets a NULL ``shapes`` array.

    Every entry is a float -- one table for the whole launch, handed to the library as host arrays -- unless some variance, scale or
    shape is a tensor of ``B`` values: then the descriptor is PER BATCH (``self.batch == B``): such columns stay on their device
    (``tables()``: fp64 ``(B, nterms)`` per column, floats broadcast), the values are not read on the host (so their signs are not checked:
    a non-positive scale or alpha gives NaN in its batch entry), and the launch is ``gpk_kmat_batch_terms`` / ``gpk_kdiag_batch_terms``."""

    batch = None

    def __init__(self, terms, shapes=None):
        terms = list(terms)
        shapes = [None] * len(terms) if shapes is None else list(shapes)
        if len(terms) > _native.MAX_TERMS:
            raise ValueError(f"at most {_native.MAX_TERMS} kernel terms are supported")
        if len(shapes) != len(terms):
            raise ValueError("one shape entry per term (None for the kinds without a shape parameter)")
        sizes = sorted({v.numel() for row, a in zip(terms, shapes) for v in (row[1], row[2], a) if _per_batch_value(v)})
        if sizes:
            if len(sizes) > 1:
                raise ValueError(f"per-batch hyper-parameters of different batch sizes in one kernel: {sizes[0]} and {sizes[1]}")
            self.batch = sizes[0]
        conv = (lambda v: v.detach().reshape(-1).to(torch.float64) if _per_batch_value(v) else float(v))      # noqa: E731
        self.terms = [(str(k), conv(v), conv(s)) for k, v, s in terms]
        for k, _, s in self.terms:
            if k not in _KIND_IDS:
                raise ValueError(f"unknown kernel kind {k!r}")
            if not torch.is_tensor(s) and not s > 0:
                raise ValueError("length scales must be positive")
        out = []
        for (k, _, _), a in zip(self.terms, shapes):
            if k in _SHAPED:
                if a is None or not (_per_batch_value(a) or float(a) > 0):
                    raise ValueError(f"a {k!r} term needs a positive shape parameter ({_SHAPE_NAME[k]}), got {a!r}")
                out.append(conv(a))
            else:
                out.append(None)
        self.shapes = out if any(a is not None for a in out) else None
        self._tables = self._entries = None

    def __len__(self):
        return len(self.terms)

    def check_batch(self, size):
        """A per-batch table serves inputs of exactly its own batch size."""
        if self.batch is not None and self.batch != size:
            raise ValueError(f"per-batch hyper-parameters for a batch of {self.batch} met inputs with a batch of {size}")

    def tables(self, device):
        """``(variances, inverse scales, shapes or None)`` of a per-batch descriptor: contiguous fp64 ``(B, nterms)`` tensors on
        ``device`` (what ``gpk_kmat_batch_terms`` reads; 0 where a term has no shape)."""
        if self._tables is None or self._tables[0].device != device:
            def column(vals):
                cols = [v.to(device) if torch.is_tensor(v) else torch.full((self.batch,), float(v), dtype=torch.float64, device=device) for v in vals]
                return torch.stack(cols, dim=1).contiguous()
            var = column([v for _, v, _ in self.terms])
            ils = 1.0 / column([s for _, _, s in self.terms])
            shp = None if self.shapes is None else column([0.0 if a is None else a for a in self.shapes])
            self._tables = (var, ils, shp)
        return self._tables

    def entry(self, b):
        """Batch entry ``b`` of a per-batch descriptor as a descriptor in floats (one device-to-host copy of the table, kept): what the
        walks over the batch hand to the unbatched launches."""
        if self.batch is None:
            return self
        if self._entries is None:
            host = lambda v: v.tolist() if torch.is_tensor(v) else [float(v)] * self.batch      # noqa: E731
            cols = [(k, host(v), host(s)) for k, v, s in self.terms]
            shp = None if self.shapes is None else [None if a is None else host(a) for a in self.shapes]
            self._entries = [KTerms([(k, v[i], s[i]) for k, v, s in cols], None if shp is None else [None if a is None else a[i] for a in shp])
                             for i in range(self.batch)]
        return self._entries[b]

    def c_arrays(self):
        if self.batch is not None:
            raise NotImplementedError("this launch takes one term table for the whole batch: it is not implemented with per-batch hyper-parameters")
        n = len(self.terms)
        kinds = (ctypes.c_int * max(n, 1))(*[_KIND_IDS[k] for k, _, _ in self.terms])
        var = (ctypes.c_double * max(n, 1))(*[v for _, v, _ in self.terms])
        ils = (ctypes.c_double * max(n, 1))(*[1.0 / s for _, _, s in self.terms])
        return kinds, var, ils, n

    def c_shapes(self):
        """The ``shapes`` host array of the library's entries (0 where a term has none); ``None`` (NULL) when no term has one."""
        if self.shapes is None:
            return None
        n = len(self.terms)
        return (ctypes.c_double * max(n, 1))(*[0.0 if a is None else a for a in self.shapes])


def _dtype_id(t):
    if t.dtype == torch.float64:
        return _native.GPK_F64
    if t.dtype == torch.float32:
        return _native.GPK_F32
    raise TypeError(f"stheno_amd supports float32/float64 tensors, got {t.dtype}")


def _as3(t):
    """View a (..., R, C) tensor as (B, R, C) with unit inner stride; returns (t3, batch_shape)."""
    if t.dim() < 2:
        raise ValueError("expected a matrix")
    bshape = tuple(t.shape[:-2])
    if t.stride(-1) != 1 and t.shape[-1] > 1:
        t = t.contiguous()
    if t.dim() == 2:
        return t.unsqueeze(0), bshape
    if t.dim() > 3:
        t = t.reshape(-1, t.shape[-2], t.shape[-1])
    if t.dim() == 3 and t.shape[0] > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    return t, bshape


def _as3_out(t):
    """``_as3`` for an OUTPUT: a tensor that would have to be copied to get a unit inner stride cannot
    receive results in place -- refuse it (a transposed view once swallowed a GEMM update silently)."""
    t3, bshape = _as3(t)
    if t3.data_ptr() != t.data_ptr() or (t.dim() >= 2 and t.shape[-1] > 1 and t.stride(-1) != 1):
        raise ValueError("output tensors need a unit inner stride (and a regular batch stride); pass a contiguous buffer")
    return t3, bshape


def alloc_matrix(bshape, rows, cols, dtype, device):
    """An uninitialised (..., rows, cols) matrix whose leading dimension is padded to a multiple
    of 16 elements when ``cols`` is not one: rows stay 16-byte aligned, so the kernels keep their
    vector loads for odd sizes.  Returned as a view (unit inner stride, stride(-2) = padded ld)."""
    if cols >= 64 and cols % 16:
        ldp = (cols + 15) // 16 * 16
        return torch.empty(tuple(bshape) + (rows, ldp), dtype=dtype, device=device)[..., :cols]
    return torch.empty(tuple(bshape) + (rows, cols), dtype=dtype, device=device)


_alloc = alloc_matrix      # (module-internal spelling)


def _ld(t3):
    # leading dimension of the (R, C) slices of a (B, R, C) tensor
    return t3.stride(1) if t3.shape[1] > 1 else max(t3.shape[2], 1)


def _bs(t3):
    return t3.stride(0) if t3.shape[0] > 1 else 0


def _tensors_of(args):
    for a in args:
        if torch.is_tensor(a):
            yield a
        elif isinstance(a, (list, tuple)):
            yield from _tensors_of(a)


def _on_operand_device(fn):
    """Run ``fn`` with the operands' device as the current device: ``libgpk`` launches on the CURRENT HIP
    device and ``torch.cuda.current_stream()`` is per device, so a call made while another device is current
    would run on that device's stream against this device's memory.  Operands on different devices are refused."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        dev = None
        for t in _tensors_of(list(args) + list(kwargs.values())):
            if not t.is_cuda:
                continue
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RuntimeError(f"operands live on different devices ({dev} and {t.device})")
        if dev is None or dev.index is None or dev.index == torch.cuda.current_device():
            return fn(self, *args, **kwargs)
        with torch.cuda.device(dev):
            return fn(self, *args, **kwargs)

    return wrapped


class HipBackend:
    """ctypes calls into ``libgpk.so`` on the current torch HIP stream of the operands' device."""

    name = "hip"

    def __init__(self):
        self.lib = _native.load()

    # -- helpers -------------------------------------------------------------
    @staticmethod
    def _check(*tensors):
        for t in tensors:
            if t is None:
                continue
            if not t.is_cuda:
                raise RuntimeError(
                    "stheno_amd ops run on a HIP device only (got a CPU tensor); "
                    "there is no CPU fallback in this package"
                )

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    @staticmethod
    def _st(code, what):
        if code != 0:
            raise RuntimeError(f"libgpk {what} failed with status {code}")

    # -- kernel matrices -----------------------------------------------------
    def _kmat(self, entry, dims, terms, x, y, lower, diag_add, diag_vec, out, accumulate, scales=None):
        """One launch of ``gpk_kmat``, ``gpk_kmat_diff`` or ``gpk_kmat_scaled`` (``entry``): they take the same arguments, apart from
        ``dims`` -- what ``gpk_kmat_diff`` has between the term table and the tensors -- and ``scales`` -- the ``(row_scale, col_scale)`` that
        ``gpk_kmat_scaled`` has between ``d`` and ``out``."""
        symmetric = y is None
        x3, bshape = _as3(x)
        y3 = x3 if symmetric else _as3(y)[0]
        self._check(x3, y3, diag_vec, out)
        B, n, d = x3.shape
        m = y3.shape[1]
        if y3.shape[0] != B or y3.shape[2] != d:
            raise ValueError("x and y must agree in batch size and input dimension")
        if out is None:
            out = _alloc(bshape, n, m, x.dtype, x.device)
        o3, _ = _as3_out(out)
        dv = None
        if diag_vec is not None:
            dv = diag_vec.reshape(B, n).contiguous()
        sc = ()
        if scales is not None:
            # each scale: (..., len) with the inputs' batch shape, or (len,) shared by the batch (stride 0)
            held = []      # (the contiguous copies live until the launch is enqueued)
            for v, length in zip(scales, (n, m)):
                if v is not None:
                    self._check(v)
                    if v.dtype != x.dtype or v.dim() < 1 or v.shape[-1] != length or v.numel() not in (length, B * length):
                        raise ValueError(f"a scale of shape {tuple(v.shape)} and dtype {v.dtype} does not fit {B} x {length} values of {x.dtype}")
                    v = v.detach().reshape(-1, length).contiguous()
                    held.append(v)
                sc += (self._ptr(v), length if v is not None and v.shape[0] > 1 else 0)
        tail = (self._ptr(x3), n, _ld(x3), _bs(x3), self._ptr(y3), m, _ld(y3),
                _bs(y3), d, *sc, self._ptr(o3), _ld(o3), _bs(o3), B, int(lower), int(symmetric), float(diag_add),
                self._ptr(dv), n if dv is not None else 0, int(accumulate), self._stream())
        if terms.batch is not None:
            # one term table per batch entry: the tables stay on the device (gpk_kmat_batch_terms); derivative blocks have no such entry
            if entry != "gpk_kmat":
                raise NotImplementedError("derivative kernels are not implemented with per-batch hyper-parameters")
            terms.check_batch(B)
            kinds, var, ils, shp, nt = self._batch_tables(terms, x3.device)
            code = self.lib.gpk_kmat_batch_terms(_dtype_id(x3), kinds, self._ptr(var), self._ptr(ils), self._ptr(shp), nt, nt, *tail)
            self._st(code, "gpk_kmat_batch_terms")
            return out
        kinds, var, ils, nt = terms.c_arrays()
        code = getattr(self.lib, entry)(_dtype_id(x3), kinds, var, ils, terms.c_shapes(), nt, *dims, *tail)
        self._st(code, entry)
        return out

    @staticmethod
    def _batch_tables(terms, device):
        nt = len(terms)
        kinds = (ctypes.c_int * max(nt, 1))(*[_KIND_IDS[k] for k, _, _ in terms.terms])
        var, ils, shp = terms.tables(device)
        return kinds, var, ils, shp, nt

    @_on_operand_device
    def kmat(self, terms, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        """``out[b, i, j] (+)= k(x[b, i], y[b, j])``; ``y is None`` means the symmetric case
        (then ``diag_add`` / ``diag_vec`` go on the diagonal)."""
        return self._kmat("gpk_kmat", (), terms, x, y, lower, diag_add, diag_vec, out, accumulate)

    @_on_operand_device
    def kmat_scaled(self, terms, x, y, row_scale, col_scale, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        """:meth:`kmat` times ``row_scale[b, i] * col_scale[b, j]`` in the same pass (``gpk_kmat_scaled``); ``diag_add`` / ``diag_vec`` go on
        the diagonal UNSCALED.  A scale is ``(..., N)`` with the inputs' batch shape or ``(N,)`` shared by the batch, in the inputs' dtype;
        ``None`` means all ones.  One term table for the whole launch: per-batch hyper-parameters are refused."""
        if terms.batch is not None:
            terms.c_arrays()       # (raises: no per-batch term tables under a scale)
        return self._kmat("gpk_kmat_scaled", (), terms, x, y, lower, diag_add, diag_vec, out, accumulate, scales=(row_scale, col_scale))

    @_on_operand_device
    def kmat_diff(self, terms, x, y, dim_x, dim_y, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        """Derivative blocks of the kernel matrix (``gpk_kmat_diff``): ``out[b, i, j] (+)=`` the derivative of ``k(x[b, i], y[b, j])`` with
        respect to ``x[b, i, dim_x]`` and / or ``y[b, j, dim_y]`` (``None``: not differentiated in that argument; at least one is given).
        ``y is None``: the symmetric case, which needs ``dim_x == dim_y`` (``lower``, ``diag_add`` / ``diag_vec`` as for :meth:`kmat`)."""
        dims = tuple(-1 if v is None else int(v) for v in (dim_x, dim_y))
        return self._kmat("gpk_kmat_diff", dims, terms, x, y, lower, diag_add, diag_vec, out, accumulate)

    @_on_operand_device
    def kdiag(self, terms, x):
        x3, bshape = _as3(x)
        self._check(x3)
        B, n, d = x3.shape
        out = torch.empty(bshape + (n,), dtype=x.dtype, device=x.device)
        if terms.batch is not None:
            terms.check_batch(B)
            kinds, var, ils, shp, nt = self._batch_tables(terms, x3.device)
            code = self.lib.gpk_kdiag_batch_terms(_dtype_id(x3), kinds, self._ptr(var), self._ptr(ils), self._ptr(shp), nt, nt, self._ptr(x3), n,
                                                  _ld(x3), _bs(x3), d, self._ptr(out), n, B, self._stream())
            self._st(code, "gpk_kdiag_batch_terms")
            return out
        kinds, var, ils, nt = terms.c_arrays()
        code = self.lib.gpk_kdiag(_dtype_id(x3), kinds, var, ils, terms.c_shapes(), nt, self._ptr(x3), n, _ld(x3), _bs(x3), d,
                                  self._ptr(out), n, B, self._stream())
        self._st(code, "gpk_kdiag")
        return out

    # -- factorisation -------------------------------------------------------
    supports_potrf_rhs = True

    @_on_operand_device
    def potrf_(self, a, nbo=0, lookahead_nb=0, lookahead_sb=0, rhs=None):
        """In-place lower Cholesky of ``a`` (..., n, n).  ``rhs`` (plain path only): a contiguous (B, n) tensor, one right-hand side per
        matrix, overwritten by ``L^{-1} rhs`` (``gpk_potrf_rhs``: batches that take the mixed-phase steps -- fp32, 64 or more aligned
        matrices -- solve it inside the steps' solve tiles; every other shape sweeps with ``gpk_trsv_lower`` behind the factorisation).
        Returns ``(dinv, info)``, or
        ``(dinv, info, dinv_sb)`` when ``lookahead_nb`` (256 ... 4096) selects the look-ahead
        factorisation of ONE large matrix: ``dinv_sb`` are the inverses of the ``sb x sb`` diagonal
        blocks of the factor (what ``trtri_merge(l, dinv, sb)`` would compute), ``sb = lookahead_sb`` or ``lookahead_nb``."""
        a3, _ = _as3(a)
        if a3.data_ptr() != a.data_ptr():
            raise ValueError("potrf_ needs a tensor with unit inner stride (it factorises in place)")
        self._check(a3)
        B, n, _ = a3.shape
        nblk = (max(n, 1) + 127) // 128
        dinv = torch.empty((B, nblk, 128, 128), dtype=a.dtype, device=a.device)
        info = torch.zeros((B,), dtype=torch.int32, device=a.device)
        if lookahead_nb:
            if B != 1 or rhs is not None:
                raise ValueError("the look-ahead factorisation takes one matrix (and no right-hand side: gpk_potrf_rows_rhs)")
            nb = int(lookahead_nb)
            sb = int(lookahead_sb) or nb
            dnb = torch.empty((1, (n + sb - 1) // sb, sb, sb), dtype=a.dtype, device=a.device)
            ws = torch.empty((int(self.lib.gpk_potrf_la_ws_elems(n, nb)),), dtype=a.dtype, device=a.device)
            if sb == nb:
                code = self.lib.gpk_potrf_la(_dtype_id(a3), self._ptr(a3), n, _ld(a3), self._ptr(dinv), self._ptr(dnb), nb,
                                             self._ptr(ws), self._ptr(info), self._stream())
            else:
                code = self.lib.gpk_potrf_la_split(_dtype_id(a3), self._ptr(a3), n, _ld(a3), self._ptr(dinv), self._ptr(dnb), nb, sb,
                                                   self._ptr(ws), self._ptr(info), self._stream())
            self._st(code, "gpk_potrf_la")
            # `ws` is freed here while the factorisation may still be running: torch's caching allocator only reuses the
            # block for work enqueued later on this same stream, and the helper stream has joined it by then
            return dinv, info, dnb
        if rhs is not None:
            if tuple(rhs.shape) != (B, n) or not rhs.is_contiguous() or rhs.dtype != a.dtype or rhs.device != a.device:
                raise ValueError("potrf_: rhs must be a contiguous (batch, n) tensor of the matrices' dtype and device")
            tmp = torch.empty((B * 128 + 16,), dtype=a.dtype, device=a.device)
            code = self.lib.gpk_potrf_rhs(_dtype_id(a3), self._ptr(a3), n, _ld(a3), _bs(a3), B, self._ptr(dinv), self._ptr(info), int(nbo),
                                          self._ptr(rhs), n, self._ptr(tmp), self._stream())
            self._st(code, "gpk_potrf_rhs")
            # (`tmp` is released here: the caching allocator hands it to later work of THIS stream only)
            return dinv, info
        code = self.lib.gpk_potrf(_dtype_id(a3), self._ptr(a3), n, _ld(a3), _bs(a3), B, self._ptr(dinv),
                                  self._ptr(info), int(nbo), self._stream())
        self._st(code, "gpk_potrf")
        return dinv, info

    @_on_operand_device
    def potrf_rows_(self, a, lookahead_nb=0, lookahead_sb=0, rhs_row=False, tail_inverses=True):
        """In-place lower Cholesky of the leading ``n x n`` of ``a`` (rows, n), rows > n, carrying the rows under it through the
        factorisation (``gpk_potrf_rows``): they come out as ``a[n:] L^{-T}``.  ``n`` a multiple of 128.  Returns ``(dinv, info, dinv_sb or None)``.
        ``rhs_row``: the last 64 rows are a strip whose first row is ONE right-hand side, the rest zero padding (``gpk_potrf_rows_rhs``,
        ``GPK_ROWS_RHS``: same result, ``L^{-1} b`` in that row; through the look-ahead steps it is computed by matrix-vector products on the
        helper stream's CUs beside the trailing updates, through the plain tail -- and without the look-ahead -- it is a row like the others).  ``tail_inverses=False``: the merged inverses of the
        look-ahead's plain tail are not computed -- ``dinv_sb`` comes back as ``None`` (incomplete), callers merge on demand."""
        if a.dim() != 2 or a.stride(-1) != 1 or a.shape[0] <= a.shape[1] or a.shape[1] % 128 != 0:
            raise ValueError("potrf_rows_ takes one (rows, n) matrix with rows > n, n a multiple of 128 and unit inner stride")
        self._check(a)
        rows, n = a.shape
        dinv = torch.empty((1, n // 128 + 1, 128, 128), dtype=a.dtype, device=a.device)      # (one slot more: control words of the last panel)
        info = torch.zeros((1,), dtype=torch.int32, device=a.device)
        nb = int(lookahead_nb)
        sb = (int(lookahead_sb) or nb) if nb else 0
        dnb = ws = None
        if nb:
            dnb = torch.empty((1, (n + sb - 1) // sb, sb, sb), dtype=a.dtype, device=a.device)
            ws = torch.empty((int(self.lib.gpk_potrf_la_ws_elems(rows, nb)),), dtype=a.dtype, device=a.device)
        flags = (1 if rhs_row else 0) | (0 if tail_inverses else 2)
        if flags:
            code = self.lib.gpk_potrf_rows_rhs(_dtype_id(a), self._ptr(a), n, rows, a.stride(0), self._ptr(dinv), self._ptr(dnb) if nb else None,
                                               nb, sb if sb != nb else 0, self._ptr(ws) if nb else None, self._ptr(info), flags, self._stream())
            self._st(code, "gpk_potrf_rows_rhs")
            return dinv[:, : n // 128], info, (dnb if tail_inverses else None)
        code = self.lib.gpk_potrf_rows(_dtype_id(a), self._ptr(a), n, rows, a.stride(0), self._ptr(dinv), self._ptr(dnb) if nb else None, nb,
                                       sb if sb != nb else 0, self._ptr(ws) if nb else None, self._ptr(info), self._stream())
        self._st(code, "gpk_potrf_rows")
        return dinv[:, : n // 128], info, dnb

    @_on_operand_device
    def potrf_border(self, a_buf, n, q, v, dinv, w1=None, r2=None):
        """Grow the factor in the leading ``n x n`` of ``a_buf`` by ``q <= 128`` rows IN PLACE (``gpk_potrf_border``): ``a_buf`` (rows,
        cols >= n + q each, unit inner stride) holds ``L11`` in its rows ``< n`` and the lower triangle of ``K22`` (diagonal additions in)
        at ``[n:n+q, n:n+q]``; ``v = L11^{-1} K12`` (n, q), unit inner stride.  On return rows ``n .. n + q`` hold ``[V^T, L22]``.
        ``dinv``: ``ceil((n + q) / 128)`` contiguous 128 x 128 blocks, those of ``L11`` in front; the blocks from ``n // 128`` on are
        written.  ``w1`` (n values, ``L11^{-1} r1``) and ``r2`` (q values, contiguous; overwritten by ``L22^{-1} (r2 - V^T w1)``): both or
        neither.  Returns ``info`` (one int32: 0, or the order of the leading minor that is not positive definite)."""
        n, q = int(n), int(q)
        if a_buf.dim() != 2 or (a_buf.shape[1] > 1 and a_buf.stride(1) != 1) or min(a_buf.shape) < n + q:
            raise ValueError("potrf_border: the buffer is one matrix of at least n + q rows and columns with unit inner stride")
        if v.dim() != 2 or tuple(v.shape) != (n, q) or (q > 1 and v.stride(1) != 1):
            raise ValueError("potrf_border: v is (n, q) with unit inner stride")
        if (w1 is None) != (r2 is None):
            raise ValueError("potrf_border: w1 and r2 are given together or not at all")
        if dinv is None or not dinv.is_contiguous() or dinv.numel() < (n + q + 127) // 128 * 128 * 128:
            raise ValueError("potrf_border: dinv holds ceil((n + q) / 128) contiguous blocks of 128 x 128")
        if r2 is not None and (w1.numel() != n or r2.numel() != q or not w1.is_contiguous() or not r2.is_contiguous()):
            raise ValueError("potrf_border: w1 has n and r2 has q contiguous values")
        for t in (v, dinv, w1, r2):
            if t is not None and (t.dtype != a_buf.dtype or t.device != a_buf.device):
                raise TypeError("potrf_border: one dtype and one device")
        self._check(a_buf, v, dinv, w1, r2)
        info = torch.zeros((1,), dtype=torch.int32, device=a_buf.device)
        ws = torch.empty((max(int(self.lib.gpk_potrf_border_ws_elems(n, q)), 1),), dtype=a_buf.dtype, device=a_buf.device)
        ld = a_buf.stride(0) if a_buf.shape[0] > 1 else a_buf.shape[1]
        ldv = v.stride(0) if n > 1 else q
        code = self.lib.gpk_potrf_border(_dtype_id(a_buf), self._ptr(a_buf), n, q, ld, self._ptr(v), ldv, self._ptr(dinv), self._ptr(w1),
                                         self._ptr(r2), self._ptr(info), self._ptr(ws), self._stream())
        self._st(code, "gpk_potrf_border")
        # (`ws` is released here: the caching allocator hands it to later work of THIS stream only)
        return info

    @_on_operand_device
    def rowreduce(self, z, w=None, *, want_dot=True, want_ss=False):
        """Row reductions of ``z`` (rows, n): ``dot[i] = sum_k z[i, k] w[k]`` and / or ``ss[i] = sum_k z[i, k]^2`` in one pass
        (``gpk_rowreduce``) -- the posterior mean and marginal variance from the TRANSPOSED whitened cross-covariance."""
        if z.dim() != 2 or z.stride(-1) != 1:
            raise ValueError("rowreduce takes one matrix with unit inner stride")
        self._check(z, w)
        rows, n = z.shape
        dot = torch.empty((rows,), dtype=z.dtype, device=z.device) if (want_dot and w is not None) else None
        ss = torch.empty((rows,), dtype=z.dtype, device=z.device) if want_ss else None
        if w is not None:
            w = w.reshape(-1).contiguous()
            if w.shape[0] != n:
                raise ValueError("rowreduce: the vector has %d entries, the rows %d" % (w.shape[0], n))
        code = self.lib.gpk_rowreduce(_dtype_id(z), self._ptr(z), rows, n, z.stride(0), self._ptr(w) if dot is not None else None,
                                      self._ptr(dot) if dot is not None else None, self._ptr(ss) if ss is not None else None, self._stream())
        self._st(code, "gpk_rowreduce")
        return dot, ss

    @_on_operand_device
    def trtri_merge(self, l, dinv, sb):
        l3, _ = _as3(l)
        self._check(l3, dinv)
        B, n, _ = l3.shape
        nsb = (n + sb - 1) // sb
        dsb = torch.empty((B, nsb, sb, sb), dtype=l.dtype, device=l.device)
        tmp = torch.empty((nsb * sb * sb // 4 + 16,), dtype=l.dtype, device=l.device)
        code = self.lib.gpk_trtri_merge(_dtype_id(l3), self._ptr(l3), n, _ld(l3), _bs(l3), B, self._ptr(dinv), sb,
                                        self._ptr(dsb), self._ptr(tmp), self._stream())
        self._st(code, "gpk_trtri_merge")
        return dsb

    def _tri_solve(self, name, trsv, trsm, l, dinv_sb, sb, b):
        """``tri_solve_`` / ``tri_solve_t_`` (``name``) through the library's sweep ``trsv`` for up to 8 columns and its blocked solve
        ``trsm`` above: the two pairs of entries take the same arguments."""
        l3, _ = _as3(l)
        b3, _ = _as3(b)
        if b3.data_ptr() != b.data_ptr():
            raise ValueError(f"{name} needs a right-hand side with unit inner stride")
        self._check(l3, b3, dinv_sb)
        B, n, _ = l3.shape
        nrhs = b3.shape[2]
        if b3.shape[0] != B or b3.shape[1] != n:
            raise ValueError("right-hand side does not match the factor")
        if n == 0 or nrhs == 0:
            return b
        if nrhs <= 8:
            tmp = torch.empty((B * sb * nrhs + 16,), dtype=b.dtype, device=b.device)     # (+ GPK_TRSV_CTRL_ELEMS: reserved)
            code = getattr(self.lib, trsv)(_dtype_id(l3), self._ptr(l3), n, _ld(l3), _bs(l3), self._ptr(dinv_sb), sb,
                                           self._ptr(b3), nrhs, _ld(b3), _bs(b3), self._ptr(tmp), B, self._stream())
            self._st(code, trsv)
            return b
        # many right-hand sides: the recursive blocked solve, out of place -- solved blocks go to a second buffer (no copy per
        # block), `b` is used up as workspace; the caller takes the return value (Chol.solve_)
        x = torch.empty(b.shape, dtype=b.dtype, device=b.device)
        x3, _ = _as3(x)
        code = getattr(self.lib, trsm)(_dtype_id(l3), self._ptr(l3), n, _ld(l3), _bs(l3), self._ptr(dinv_sb), sb,
                                       self._ptr(b3), nrhs, _ld(b3), _bs(b3), self._ptr(x3), _ld(x3), _bs(x3), B, self._stream())
        self._st(code, trsm)
        return x

    @_on_operand_device
    def tri_solve_(self, l, dinv_sb, sb, b):
        """``L^{-1} b``; ``b`` is (..., n, nrhs) with unit inner stride and is OVERWRITTEN (with the solution for up to 8 columns,
        with intermediate values otherwise): use the return value."""
        return self._tri_solve("tri_solve_", "gpk_trsv_lower", "gpk_trsm_lower_to", l, dinv_sb, sb, b)

    @_on_operand_device
    def tri_solve_t_(self, l, dinv_sb, sb, b):
        """``L^{-T} b`` with the TRANSPOSED factor (``gpk_trsv_lower_t`` for up to 8 columns, ``gpk_trsm_lower_t`` above), the mirror of
        :meth:`tri_solve_`: ``b`` (..., n, nrhs), unit inner stride, is OVERWRITTEN (with the solution for up to 8 columns, used up as
        workspace otherwise): use the return value."""
        return self._tri_solve("tri_solve_t_", "gpk_trsv_lower_t", "gpk_trsm_lower_t", l, dinv_sb, sb, b)

    # -- products ------------------------------------------------------------
    @_on_operand_device
    def trtri(self, l, dinv_sb, sb):
        """``L^{-1}`` of an unbatched factor as a full (n, n) lower-triangular matrix."""
        self._check(l, dinv_sb)
        n = l.shape[-1]
        w = _alloc((), n, n, l.dtype, l.device)
        tmp = torch.empty((sb * n,), dtype=l.dtype, device=l.device)
        code = self.lib.gpk_trtri_lower(_dtype_id(l), self._ptr(l), n, l.stride(0), self._ptr(dinv_sb), sb,
                                        self._ptr(w), w.stride(0), self._ptr(tmp), self._stream())
        self._st(code, "gpk_trtri_lower")
        return w

    @_on_operand_device
    def potrf_vjp(self, l, dinv_sb, sb, lbar):
        """The vector-Jacobian product of the Cholesky factorisation (``gpk_potrf_vjp``): ``l`` (n, n) the factor ``potrf_`` left (only its
        lower triangle is read), ``dinv_sb`` / ``sb`` its merged inverses as for :meth:`tri_solve_`, ``lbar`` (n, n) the cotangent of
        ``L`` (only its lower triangle is read).  Returns the cotangent of ``A = L L^T`` as a full, exactly symmetric (n, n) matrix."""
        if l.dim() != 2 or lbar.dim() != 2 or l.shape[0] != l.shape[1] or tuple(lbar.shape) != tuple(l.shape):
            raise ValueError("potrf_vjp takes one (n, n) factor and an (n, n) cotangent")
        if lbar.dtype != l.dtype:
            raise TypeError("potrf_vjp: the cotangent must have the factor's dtype")
        n = l.shape[0]
        if (n > 1 and l.stride(1) != 1) or (n > 1 and lbar.stride(1) != 1):
            raise ValueError("potrf_vjp: unit inner strides")
        self._check(l, dinv_sb, lbar)
        abar = _alloc((), n, n, l.dtype, l.device)
        if n == 0:
            return abar
        ws = torch.empty((int(self.lib.gpk_potrf_vjp_ws_elems(n, sb)),), dtype=l.dtype, device=l.device)
        ld = lambda t: _ld(t.unsqueeze(0))      # noqa: E731
        code = self.lib.gpk_potrf_vjp(_dtype_id(l), self._ptr(l), n, ld(l), self._ptr(dinv_sb), sb, self._ptr(lbar), ld(lbar),
                                      self._ptr(abar), ld(abar), self._ptr(ws), self._stream())
        self._st(code, "gpk_potrf_vjp")
        # (`ws` is released here: the caching allocator hands it to later work of THIS stream only)
        return abar

    @_on_operand_device
    def nuclear_norm(self, m, iters=None):
        """The nuclear norm (sum of the singular values) of ``m`` (..., n, n), unit inner stride: ``(...,)``, by ``iters`` steps of the
        Newton-Schulz polar iteration on the MFMA GEMM (``gpk_nuclear_norm``; one launch sequence for the whole batch).  ``iters``
        defaults to :data:`NUCLEAR_ITERS_F64` / :data:`NUCLEAR_ITERS_F32`."""
        if m.dim() < 2 or m.shape[-1] != m.shape[-2]:
            raise ValueError("nuclear_norm takes square matrices (..., n, n)")
        if m.shape[-1] > 1 and m.stride(-1) != 1:
            raise ValueError("nuclear_norm: unit inner stride")
        if iters is None:
            iters = NUCLEAR_ITERS_F64 if m.dtype == torch.float64 else NUCLEAR_ITERS_F32
        if int(iters) < 1:
            raise ValueError("nuclear_norm: at least one step")
        m3, bshape = _as3(m)
        self._check(m3)
        B, n, _ = m3.shape
        out = torch.zeros((B,), dtype=m.dtype, device=m.device)
        if n == 0 or B == 0:
            return out.reshape(bshape)
        ws = torch.empty((int(self.lib.gpk_nuclear_norm_ws_elems(n, B)),), dtype=m.dtype, device=m.device)
        code = self.lib.gpk_nuclear_norm(_dtype_id(m3), self._ptr(m3), n, _ld(m3), _bs(m3), B, int(iters), self._ptr(out),
                                         self._ptr(ws), self._stream())
        self._st(code, "gpk_nuclear_norm")
        return out.reshape(bshape)

    @_on_operand_device
    def gemm(self, a, b, *, a_kmajor=True, b_kmajor=True, alpha=1.0, beta=0.0, out=None, lower_only=False,
             tri_k=False, tri_k_lower=False, tri_k_lower_b=False, panel_solve=False):
        """``out[m, n] = alpha * sum_k a(m, k) b(n, k) + beta * out``.

        ``a_kmajor``: ``a`` is stored (M, K); otherwise (K, M).  ``b_kmajor``: ``b`` is stored
        (N, K); otherwise (K, N).  ``tri_k`` / ``tri_k_lower`` / ``tri_k_lower_b``: the ``GPK_GEMM_TRI_K*`` flags of ``include/gpk.h``
        (the operands vanish where the k loop is cut short); ``panel_solve``: flag bit 16, the in-place panel solve of the Cholesky."""
        a3, bshape = _as3(a)
        b3, _ = _as3(b)
        self._check(a3, b3, out)
        B = max(a3.shape[0], b3.shape[0])
        M, K = (a3.shape[1], a3.shape[2]) if a_kmajor else (a3.shape[2], a3.shape[1])
        N, K2 = (b3.shape[1], b3.shape[2]) if b_kmajor else (b3.shape[2], b3.shape[1])
        if K != K2:
            raise ValueError("inner dimensions do not match")
        if out is None:
            if beta != 0.0:
                raise ValueError("beta != 0 requires `out`")
            out = _alloc(bshape if a3.shape[0] >= b3.shape[0] else tuple(b.shape[:-2]), M, N, a.dtype, a.device)
        o3, _ = _as3_out(out)
        code = self.lib.gpk_gemm(_dtype_id(a3), int(a_kmajor), int(b_kmajor), M, N, K, float(alpha), self._ptr(a3),
                                 _ld(a3), _bs(a3), self._ptr(b3), _ld(b3), _bs(b3), float(beta), self._ptr(o3),
                                 _ld(o3), _bs(o3), B, int(lower_only) | (2 if tri_k else 0) | (4 if tri_k_lower else 0)
                                 | (8 if tri_k_lower_b else 0) | (16 if panel_solve else 0), self._stream())
        self._st(code, "gpk_gemm")
        return out

    @_on_operand_device
    def gemm_colscale(self, a, b, colscale=None, *, want_colss=False, a_kmajor=True, b_kmajor=True, tri_k_lower=False, alpha=1.0,
                      flags=0, out=None, colss_rows=None):
        """``out[m, n] = sum_k a(m, k) b(n, k) * colscale[n]`` (unbatched) and, with ``want_colss``, the column sums of squares of the
        UNSCALED product -- both in the epilogue of the one GEMM (``gpk_gemm_colscale``).  Returns ``(out, colss or None)``.

        ``alpha`` scales the product, ``flags`` are or-ed into the library's flag word, ``out`` receives the product (unit inner stride)
        and ``colss_rows``, a ``(gpk_gemm_colss_rows(M), N)`` view with unit inner stride, receives the per-slab partial sums, which are
        then returned as they are instead of their sum."""
        M, K = (a.shape[0], a.shape[1]) if a_kmajor else (a.shape[1], a.shape[0])
        N, K2 = (b.shape[0], b.shape[1]) if b_kmajor else (b.shape[1], b.shape[0])
        if a.dim() != 2 or b.dim() != 2 or K != K2:
            raise ValueError("gemm_colscale takes two matrices with matching inner dimensions")
        a3, _ = _as3(a)
        b3, _ = _as3(b)
        self._check(a3, b3, None)
        if out is None:
            out = torch.empty((M, N), dtype=a.dtype, device=a.device)
        self._check(out, colss_rows)
        part = colss_rows
        if want_colss and part is None:
            part = torch.empty((int(self.lib.gpk_gemm_colss_rows(M)), N), dtype=a.dtype, device=a.device)
        if colscale is not None:
            colscale = colscale.to(dtype=a.dtype).contiguous()
            if colscale.shape != (N,):
                raise ValueError("colscale must have one entry per column")
        code = self.lib.gpk_gemm_colscale(_dtype_id(a3), int(a_kmajor), int(b_kmajor), M, N, K, float(alpha), self._ptr(a3), _ld(a3), self._ptr(b3),
                                          _ld(b3), self._ptr(out), _ld(out.unsqueeze(0)), (4 if tri_k_lower else 0) | int(flags),
                                          self._ptr(colscale) if colscale is not None else None,
                                          self._ptr(part) if part is not None else None,
                                          N if colss_rows is None else colss_rows.stride(0), self._stream())
        self._st(code, "gpk_gemm_colscale")
        if colss_rows is not None:
            return out, colss_rows
        return out, (part.sum(0) if part is not None else None)       # (64 x N partial sums: a statistics buffer, added up by torch)

    @_on_operand_device
    def gemm_update2(self, updates, alpha, reserve_cus=False, ctrl=None):
        """Up to two rank-k updates ``c = cin + alpha * a b^T`` in one persistent launch (``gpk_gemm_update2``).  ``updates``: dicts with
        the matrices ``a`` (m, k), ``b`` (n, k), ``c`` (m, n), optionally ``cin`` (default: ``c``, in place) and ``lower_only``; unit inner
        strides.  ``ctrl``: 256 bytes of device scratch (allocated when not given; the call zeroes it)."""
        ts = [t for u in updates for t in (u["a"], u["b"], u["c"], u.get("cin"))]
        self._check(*ts)
        first = updates[0]["c"] if updates else None
        if ctrl is None and first is not None:
            ctrl = torch.empty((64,), dtype=torch.int32, device=first.device)
        arr = (_native.gpk_update_t * max(len(updates), 1))()
        for i, u in enumerate(updates):
            a, b, c = u["a"], u["b"], u["c"]
            cin = u.get("cin")
            cin = c if cin is None else cin
            for t in (a, b, c, cin):
                if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
                    raise ValueError("gemm_update2 takes matrices with a unit inner stride")
            m, k = a.shape
            n = b.shape[0]
            if b.shape[1] != k or tuple(c.shape) != (m, n) or tuple(cin.shape) != (m, n):
                raise ValueError("gemm_update2: shapes do not match")
            ld = lambda t: _ld(t.unsqueeze(0))      # noqa: E731
            arr[i] = _native.gpk_update_t(m, n, k, a.data_ptr(), ld(a), b.data_ptr(), ld(b), cin.data_ptr(), ld(cin), c.data_ptr(), ld(c),
                                          int(bool(u.get("lower_only", False))))
        dt = _dtype_id(first) if first is not None else _native.GPK_F64
        cp = ctypes.c_void_p(ctrl) if isinstance(ctrl, int) else self._ptr(ctrl)      # (an integer: a raw address, 0 = NULL)
        code = self.lib.gpk_gemm_update2(dt, arr, len(updates), float(alpha), cp, int(bool(reserve_cus)), self._stream())
        self._st(code, "gpk_gemm_update2")
        return [u["c"] for u in updates]

    @_on_operand_device
    def gemv(self, a, x, *, alpha=1.0, beta=0.0, out=None):
        """``out = alpha * a @ x + beta * out`` for (..., M, K) @ (..., K, nrhs <= 8)."""
        a3, bshape = _as3(a)
        x3, _ = _as3(x)
        self._check(a3, x3, out)
        B, M, K = a3.shape
        nrhs = x3.shape[2]
        if out is None:
            out = torch.empty(bshape + (M, nrhs), dtype=a.dtype, device=a.device)
        o3, _ = _as3_out(out)
        code = self.lib.gpk_gemv(_dtype_id(a3), 0, M, K, nrhs, float(alpha), self._ptr(a3), _ld(a3), _bs(a3),
                                 self._ptr(x3), _ld(x3), _bs(x3), float(beta), self._ptr(o3), _ld(o3), _bs(o3), B,
                                 self._stream())
        self._st(code, "gpk_gemv")
        return out

    # -- reductions ----------------------------------------------------------
    @_on_operand_device
    def logdet_chol(self, l):
        l3, bshape = _as3(l)
        self._check(l3)
        B, n, _ = l3.shape
        out = torch.empty((B,), dtype=l.dtype, device=l.device)
        code = self.lib.gpk_logdet_chol(_dtype_id(l3), self._ptr(l3), n, _ld(l3), _bs(l3), B, self._ptr(out),
                                        self._stream())
        self._st(code, "gpk_logdet_chol")
        return out.reshape(bshape)

    @_on_operand_device
    def colreduce(self, v, w=None, *, want_dot=False, want_ss=True):
        """Column reductions of ``v`` (..., R, C): ``(v^T w, colsumsq(v))`` (``None`` for the
        one not requested).  ``w``: (..., R) or (..., R, 1)."""
        v3, bshape = _as3(v)
        self._check(v3, w)
        B, R, C = v3.shape
        dot = ss = None
        w2 = None
        if want_dot:
            if w is None:
                raise ValueError("want_dot needs w")
            w2 = w.reshape(B, R).contiguous()
            dot = torch.empty((B, C), dtype=v.dtype, device=v.device)
        if want_ss:
            ss = torch.empty((B, C), dtype=v.dtype, device=v.device)
        nchunk = int(self.lib.gpk_colreduce_chunks(R))
        ws = torch.empty((2 * B * nchunk * max(C, 1),), dtype=v.dtype, device=v.device)
        code = self.lib.gpk_colreduce(_dtype_id(v3), self._ptr(v3), R, C, _ld(v3), _bs(v3), self._ptr(w2), R,
                                      self._ptr(dot), self._ptr(ss), self._ptr(ws), B, self._stream())
        self._st(code, "gpk_colreduce")
        if dot is not None:
            dot = dot.reshape(bshape + (C,))
        if ss is not None:
            ss = ss.reshape(bshape + (C,))
        return dot, ss

    @_on_operand_device
    def kmat_vjp(self, terms, x, kinv, alpha, g):
        """Sums for the hyper-parameter gradient of the log-density (see gpk_kmat_vjp):
        returns ``(S, trace_G, diag_G)`` with ``S[t] = (sum G kappa_t, sum G kappa_t' q)``.
        ``x`` (n, d), ``kinv`` (n, n; lower triangle read), ``alpha`` (n, C <= 8), ``g``: C floats.
        Terms with a shape parameter (``terms.shapes``): ``S`` has a third column, ``sum G d kappa_t / d shape_t``."""
        self._check(x, kinv, alpha)
        n, d = x.shape
        C = alpha.shape[1]
        kinds, _, ils, nt = terms.c_arrays()
        nb = int(self.lib.gpk_kmat_vjp_blocks(n))
        ns = 3 if terms.shapes is not None else 2       # sums per term: the library's partial rows (gpk.h)
        partial = torch.zeros((nb, ns * _native.MAX_TERMS + 1), dtype=x.dtype, device=x.device)
        diag_g = torch.empty((n,), dtype=x.dtype, device=x.device)
        gs = (ctypes.c_double * max(C, 1))(*[float(v) for v in g])
        alpha = alpha.contiguous()
        code = self.lib.gpk_kmat_vjp(_dtype_id(x), kinds, ils, terms.c_shapes(), nt, self._ptr(x), n, x.stride(0), d, self._ptr(kinv),
                                     kinv.stride(0), self._ptr(alpha), C, alpha.stride(0), gs, self._ptr(partial),
                                     self._ptr(diag_g), self._stream())
        self._st(code, "gpk_kmat_vjp")
        tot = partial.sum(0)
        return tot[: ns * nt].reshape(nt, ns), tot[ns * _native.MAX_TERMS], diag_g

    @_on_operand_device
    def kmat_vjp_dense(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        """Sums over an explicit cotangent ``Geff = g * colscale[None, :] + w[:, None] b[None, :]`` of
        ``K = k(x, y)`` (see gpk_kmat_vjp_dense): returns ``(S, colsum, gradx)`` with
        ``S[t] = (sum Geff kappa_t, sum Geff kappa_t' q)``, ``colsum[j] = sum_i Geff_ij K_ij`` and
        ``gradx[i] = sum_j Geff_ij dK_ij/dx_i`` (``None`` unless asked for).
        Terms with a shape parameter: ``S`` has a third column, ``sum Geff d kappa_t / d shape_t``."""
        self._check(x, y, g, colscale, w, b)
        n, d = x.shape
        m = y.shape[0]
        if g.shape != (n, m) or g.stride(1) != 1:
            raise ValueError("cotangent must be an (n, m) matrix with unit inner stride")
        rt, nc = ctypes.c_int64(), ctypes.c_int64()
        self._st(self.lib.gpk_kmat_vjp_dense_grid(n, m, ctypes.byref(rt), ctypes.byref(nc)), "gpk_kmat_vjp_dense_grid")
        rt, nc = rt.value, nc.value
        ns = 2 if terms.shapes is None else 3
        width = ns * _native.MAX_TERMS + 1
        partial = torch.zeros((rt * nc, width), dtype=x.dtype, device=x.device)
        colsum = torch.zeros((rt, m), dtype=x.dtype, device=x.device) if want_colsum else None
        gradx = torch.zeros((nc, n, d), dtype=x.dtype, device=x.device) if want_gradx else None
        kinds, var, ils, nt = terms.c_arrays()
        x, y = x.contiguous(), y.contiguous()
        cs = colscale.contiguous() if colscale is not None else None
        w = w.contiguous() if w is not None else None
        b = b.contiguous() if b is not None else None
        tail = (self._ptr(x), n, x.stride(0), self._ptr(y),
                m, y.stride(0), d, self._ptr(g), g.stride(0), self._ptr(cs), self._ptr(w),
                self._ptr(b), self._ptr(partial), self._ptr(colsum), self._ptr(gradx),
                self._stream())
        self._st(self.lib.gpk_kmat_vjp_dense(_dtype_id(x), kinds, var, ils, terms.c_shapes(), nt, *tail), "gpk_kmat_vjp_dense")
        tot = partial.sum(0)
        return (tot[: ns * nt].reshape(nt, ns), colsum.sum(0) if want_colsum else None,
                gradx.sum(0) if want_gradx else None)

    @_on_operand_device
    def kmat_vjp_dense_batch(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        """``kmat_vjp_dense`` for a batch of independent problems under ONE term table, in one launch (``gpk_kmat_vjp_dense_batch``):
        ``x`` (B, n, d), ``y`` (B, m, d), ``g`` (B, n, m) with unit inner stride, ``colscale`` (B, m), ``w`` (B, n), ``b`` (B, m).
        Expanded (zero-stride) views pass through without a copy: shared inputs, the all-zero cotangent operand.  Returns PER ENTRY
        ``(S (B, nt, 2 or 3), colsum (B, m) or None, gradx (B, n, d) or None)``: the sum over the batch, for a parameter the entries
        share, is the caller's.  A per-batch term table is refused (``KTerms.c_arrays``)."""
        self._check(x, y, g, colscale, w, b)
        kinds, var, ils, nt = terms.c_arrays()
        if x.dim() != 3 or y.dim() != 3 or g.dim() != 3:
            raise ValueError("batched operands are (B, n, d), (B, m, d) and (B, n, m)")
        B, n, d = x.shape
        m = y.shape[1]
        if y.shape[0] != B or y.shape[2] != d or tuple(g.shape) != (B, n, m) or (m > 1 and g.stride(2) != 1):
            raise ValueError("cotangent must be a (B, n, m) tensor with unit inner stride over (B, n, d) and (B, m, d) inputs")

        def rows(t):          # (B, r, c) with unit inner stride; a zero batch stride stays
            return t if (t.stride(2) == 1 or t.shape[2] == 1) and (t.stride(1) >= t.shape[2] or t.shape[1] == 1) else t.contiguous()

        def vec(t, size):     # (B, size) with unit inner stride
            if t is None:
                return None, 0
            if tuple(t.shape) != (B, size):
                raise ValueError(f"expected a ({B}, {size}) operand, got {tuple(t.shape)}")
            t = t if (t.stride(1) == 1 or size == 1) else t.contiguous()
            return t, (t.stride(0) if B > 1 else 0)

        x, y = rows(x), rows(y)
        cs, s_cs = vec(colscale, m)
        w, s_w = vec(w, n)
        b, s_b = vec(b, m)
        rt, nc = ctypes.c_int64(), ctypes.c_int64()
        self._st(self.lib.gpk_kmat_vjp_dense_batch_grid(n, m, B, ctypes.byref(rt), ctypes.byref(nc)), "gpk_kmat_vjp_dense_batch_grid")
        rt, nc = rt.value, nc.value
        ns = 2 if terms.shapes is None else 3
        width = ns * _native.MAX_TERMS + 1
        partial = torch.zeros((B, rt * nc, width), dtype=x.dtype, device=x.device)
        colsum = torch.zeros((B, rt, m), dtype=x.dtype, device=x.device) if want_colsum else None
        gradx = torch.zeros((B, nc, n, d), dtype=x.dtype, device=x.device) if want_gradx else None
        bs = lambda t: t.stride(0) if B > 1 else 0      # noqa: E731
        code = self.lib.gpk_kmat_vjp_dense_batch(
            _dtype_id(x), kinds, var, ils, terms.c_shapes(), nt, self._ptr(x), n, x.stride(1), bs(x), self._ptr(y), m, y.stride(1), bs(y), d,
            self._ptr(g), g.stride(1), bs(g), self._ptr(cs), s_cs, self._ptr(w), s_w, self._ptr(b), s_b,
            self._ptr(partial), self._ptr(colsum), self._ptr(gradx), B, self._stream())
        self._st(code, "gpk_kmat_vjp_dense_batch")
        tot = partial.sum(1)
        return (tot[:, : ns * nt].reshape(B, nt, ns), colsum.sum(1) if want_colsum else None,
                (gradx[:, 0] if nc == 1 else gradx.sum(1)) if want_gradx else None)

    @_on_operand_device
    def kmat_diff_vjp(self, terms, x, y, dim_x, dim_y, g, want_gradx=False):
        """Sums over the explicit cotangent ``g`` (n, m) of the derivative block ``kmat_diff(terms, x, y, dim_x, dim_y)``, which is never
        formed (``gpk_kmat_diff_vjp``): returns ``(S, gradx)`` with ``S[t] = (sum g beta_t, sum g c dbeta_t/dc[, sum g dbeta_t/dalpha_t])``
        in the conventions of ``kmat_vjp_dense`` -- a block element is ``sum_t v_t beta_t`` -- and ``gradx[i] = sum_j g_ij d block_ij /
        dx_i`` (``None`` unless asked for; the one-sided blocks and at most 8 input dimensions)."""
        self._check(x, y, g)
        n, d = x.shape
        m = y.shape[0]
        if g.shape != (n, m) or g.stride(1) != 1:
            raise ValueError("cotangent must be an (n, m) matrix with unit inner stride")
        dims = tuple(-1 if v is None else int(v) for v in (dim_x, dim_y))
        rt, nc = ctypes.c_int64(), ctypes.c_int64()
        self._st(self.lib.gpk_kmat_vjp_dense_grid(n, m, ctypes.byref(rt), ctypes.byref(nc)), "gpk_kmat_vjp_dense_grid")
        rt, nc = rt.value, nc.value
        ns = 2 if terms.shapes is None else 3
        partial = torch.zeros((rt * nc, ns * _native.MAX_TERMS + 1), dtype=x.dtype, device=x.device)
        gradx = torch.zeros((nc, n, d), dtype=x.dtype, device=x.device) if want_gradx else None
        kinds, var, ils, nt = terms.c_arrays()
        x, y = x.contiguous(), y.contiguous()
        code = self.lib.gpk_kmat_diff_vjp(_dtype_id(x), kinds, var, ils, terms.c_shapes(), nt, *dims, self._ptr(x), n, x.stride(0),
                                          self._ptr(y), m, y.stride(0), d, self._ptr(g), g.stride(0), self._ptr(partial),
                                          self._ptr(gradx), self._stream())
        self._st(code, "gpk_kmat_diff_vjp")
        return partial.sum(0)[: ns * nt].reshape(nt, ns), gradx.sum(0) if want_gradx else None

    # -- in-place odds and ends ------------------------------------------------
    @_on_operand_device
    def tril_(self, a):
        a3, _ = _as3_out(a)
        self._check(a3)
        B, n, _ = a3.shape
        self._st(self.lib.gpk_tril(_dtype_id(a3), self._ptr(a3), n, _ld(a3), _bs(a3), B, self._stream()), "gpk_tril")
        return a

    @_on_operand_device
    def sum_lower(self, parts, out):
        """``out[i, j] = sum_s parts[s, i, j]`` for ``j <= i`` (``gpk_sum_lower``): the partial products of a split-K symmetric update,
        of which only the lower tiles were written, added up in a fixed order.  Entries above the diagonal of ``out`` are not written: they
        keep what they held."""
        if parts.dim() != 3 or out.dim() != 2 or parts.shape[1] != parts.shape[2] or tuple(out.shape) != tuple(parts.shape[1:]):
            raise ValueError("sum_lower takes (S, n, n) partial products and an (n, n) output")
        if parts.stride(-1) != 1 or out.stride(-1) != 1:
            raise ValueError("sum_lower: unit inner strides")
        self._check(parts, out)
        self._st(self.lib.gpk_sum_lower(_dtype_id(out), self._ptr(parts), parts.shape[0], out.shape[0], parts.stride(1), parts.stride(0),
                                        self._ptr(out), out.stride(0), self._stream()), "gpk_sum_lower")
        return out

    @_on_operand_device
    def symmetrize_(self, a):
        a3, _ = _as3_out(a)
        self._check(a3)
        B, n, _ = a3.shape
        self._st(self.lib.gpk_symmetrize(_dtype_id(a3), self._ptr(a3), n, _ld(a3), _bs(a3), B, self._stream()),
                 "gpk_symmetrize")
        return a

    @_on_operand_device
    def add_diag_(self, a, s=0.0, v=None):
        a3, _ = _as3_out(a)
        self._check(a3, v)
        B, n, _ = a3.shape
        v2 = v.reshape(B, n).contiguous() if v is not None else None
        self._st(self.lib.gpk_add_diag(_dtype_id(a3), self._ptr(a3), n, _ld(a3), _bs(a3), float(s), self._ptr(v2),
                                       n if v2 is not None else 0, B, self._stream()), "gpk_add_diag")
        return a

    @_on_operand_device
    def scale_cols_(self, v, s):
        v3, _ = _as3_out(v)
        self._check(v3, s)
        B, R, C = v3.shape
        s2 = s.reshape(B, C).contiguous()
        self._st(self.lib.gpk_scale_cols(_dtype_id(v3), self._ptr(v3), R, C, _ld(v3), _bs(v3), self._ptr(s2), C, B,
                                         self._stream()), "gpk_scale_cols")
        return v

    @_on_operand_device
    def copy(self, src, out=None):
        """Fresh copy of a (..., R, C) tensor (strided 2-D copy kernel; rows 16-byte aligned); ``out``: into that tensor of the same
        shape and dtype (unit inner stride) instead -- a view of a larger buffer, say."""
        s3, bshape = _as3(src)
        self._check(s3, out)
        B, R, C = s3.shape
        if out is None:
            out = _alloc(bshape, R, C, src.dtype, src.device)
        elif tuple(out.shape) != tuple(src.shape) or out.dtype != src.dtype:
            raise ValueError("copy: the output has the source's shape and dtype")
        o3, _ = _as3_out(out)
        self._st(self.lib.gpk_copy2d(_dtype_id(s3), self._ptr(s3), _ld(s3), _bs(s3), self._ptr(o3), _ld(o3), _bs(o3),
                                     R, C, B, self._stream()), "gpk_copy2d")
        return out


class _HostDelta:
    """Around a backend that is not the HIP one (the checker backends of ``tests/``, built on an oracle that predates the ``"delta"``
    kind): ``"delta"`` terms are evaluated here, in NumPy, and every other term is handed on unchanged; so are the derivative blocks of
    ``kmat_diff``, the Cholesky VJP ``potrf_vjp`` and the nuclear norm ``nuclear_norm``, which that oracle does not know either.
    ``HipBackend`` is never wrapped: there all of these are launches of the HIP library."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    @staticmethod
    def _split(terms):
        sh = terms.shapes or [None] * len(terms)
        rest = [(t, a) for t, a in zip(terms.terms, sh) if t[0] != "delta"]
        delta = [(i, t, a) for i, (t, a) in enumerate(zip(terms.terms, sh)) if t[0] == "delta"]
        keep = [i for i, t in enumerate(terms.terms) if t[0] != "delta"]
        return KTerms([t for t, _ in rest], [a for _, a in rest]), delta, keep

    @staticmethod
    def _kappa(x, y, scale, eps):
        import numpy as np

        a, b = x.detach().cpu().numpy(), y.detach().cpu().numpy()
        q = ((a[..., :, None, :] - b[..., None, :, :]) ** 2).sum(-1) * (1.0 / scale) ** 2
        return np.where(np.isnan(q), q, (q < eps).astype(q.dtype))

    @staticmethod
    def _t(a, like):
        import numpy as np

        return torch.as_tensor(np.ascontiguousarray(a), dtype=like.dtype, device=like.device)

    @staticmethod
    def _deliver(res, out, accumulate):
        """``res`` as the result of a call with ``out`` / ``accumulate``."""
        if out is None:
            return res
        if accumulate:
            out += res
        else:
            out.copy_(res)
        return out

    @staticmethod
    def _batch3(terms, x):
        """The inputs of a per-batch call as ``(B, N, D)`` (the batch sizes checked: what ``HipBackend`` does before its launch)."""
        x3 = x if x.dim() == 3 else x.reshape((-1,) + tuple(x.shape[-2:])) if x.dim() > 3 else x.unsqueeze(0)
        terms.check_batch(x3.shape[0])
        return x3

    def kmat(self, terms, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        if terms.batch is not None:
            # one term table per batch entry: the scalar form, entry by entry
            x3 = self._batch3(terms, x)
            y3 = None if y is None else self._batch3(terms, y)
            dv = None if diag_vec is None else diag_vec.reshape(x3.shape[0], -1)
            res = torch.stack([self.kmat(terms.entry(b), x3[b], None if y3 is None else y3[b], lower=lower, diag_add=diag_add,
                                         diag_vec=None if dv is None else dv[b]) for b in range(x3.shape[0])])
            return self._deliver(res.reshape(tuple(x.shape[:-2]) + tuple(res.shape[-2:])), out, accumulate)
        rest, delta, _ = self._split(terms)
        if not delta:
            return self._inner.kmat(terms, x, y, lower=lower, diag_add=diag_add, diag_vec=diag_vec, out=out, accumulate=accumulate)
        res = self._inner.kmat(rest, x, y, lower=lower, diag_add=diag_add, diag_vec=diag_vec)
        for _, (_, var, scale), eps in delta:
            res = res + self._t(var * self._kappa(x, x if y is None else y, scale, eps), res)
        return self._deliver(res, out, accumulate)

    def kmat_scaled(self, terms, x, y, row_scale, col_scale, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        """``HipBackend.kmat_scaled`` on a backend without the fused launch: the inner ``kmat`` and the two multiplications in torch, the
        diagonal additions behind them (unscaled)."""
        if terms.batch is not None:
            terms.c_arrays()       # (raises, as the HIP backend does)
        res = _HostDelta.kmat(self, terms, x, y, lower=lower)      # (this class's own: a recording subclass sees ONE call)
        if row_scale is not None:
            res = res * row_scale.detach().unsqueeze(-1)
        if col_scale is not None:
            res = res * col_scale.detach().unsqueeze(-2)
        if y is None and (diag_vec is not None or diag_add != 0.0):
            res = res.clone()
            dg = torch.diagonal(res, dim1=-2, dim2=-1)
            dg += diag_add
            if diag_vec is not None:
                dg += diag_vec.reshape(dg.shape)
        return self._deliver(res, out, accumulate)

    def kmat_diff(self, terms, x, y, dim_x, dim_y, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
        """``HipBackend.kmat_diff`` in NumPy (fp64, rounded to the inputs' dtype), from the closed forms in ``include/gpk.h``: the
        checker backends know no derivative blocks, so the host logic of ``DiffKernel`` runs on this."""
        import numpy as np

        if dim_x is None and dim_y is None:
            raise ValueError("a derivative block differentiates at least one argument")
        if y is None and dim_x != dim_y:
            raise ValueError("the symmetric form needs the same dimension in both arguments")
        a = x.detach().cpu().numpy().astype(np.float64)
        b = a if y is None else y.detach().cpu().numpy().astype(np.float64)
        for dim in (dim_x, dim_y):
            if dim is not None and not 0 <= dim < a.shape[-1]:
                raise ValueError(f"dimension {dim} outside the {a.shape[-1]} input dimensions")
        df = a[..., :, None, :] - b[..., None, :, :]
        r2 = (df ** 2).sum(-1)
        da = df[..., dim_x] if dim_x is not None else None
        db = df[..., dim_y] if dim_y is not None else None
        res = np.zeros_like(r2)
        for (kind, v, scale), alpha in zip(terms.terms, terms.shapes or [None] * len(terms)):
            c = (1.0 / scale) ** 2
            if kind == "const":
                continue
            if kind == "linear":
                if dim_y is None:
                    res += c * v * b[..., None, :, dim_x]
                elif dim_x is None:
                    res += c * v * a[..., :, None, dim_y]
                elif dim_x == dim_y:
                    res += c * v
                continue
            q = c * r2
            if kind == "eq":
                k1 = -0.5 * np.exp(-0.5 * q)
                k2dd = 0.25 * np.exp(-0.5 * q) * (da * db) if db is not None and da is not None else None
            elif kind == "rq":
                u = q / (2.0 * alpha)
                k1 = -0.5 * np.exp(-(alpha + 1.0) * np.log1p(u))
                k2dd = (alpha + 1.0) / (4.0 * alpha) * np.exp(-(alpha + 2.0) * np.log1p(u)) * (da * db) if db is not None and da is not None else None
            elif kind == "matern52":
                sd = np.sqrt(5.0 * q)
                k1 = -(5.0 / 6.0) * (1.0 + sd) * np.exp(-sd)
                k2dd = (25.0 / 12.0) * np.exp(-sd) * (da * db) if db is not None and da is not None else None
            elif kind == "matern32":
                sd = np.sqrt(3.0 * q)
                k1 = -1.5 * np.exp(-sd)
                k2dd = None
                if da is not None and db is not None:      # kappa'' D_a D_b -> 0 with the distance: 0 at coincident points
                    pos = sd > 0
                    k2dd = 2.25 * np.exp(-sd) * np.where(pos, (da * db) / np.where(pos, sd, 1.0), np.where(np.isnan(sd), np.nan, 0.0))
            else:
                raise NotImplementedError(f"a {kind!r} term has no derivative")
            if dim_y is None:
                res += 2.0 * c * v * k1 * da
            elif dim_x is None:
                res += -2.0 * c * v * k1 * db
            else:
                res += v * (-4.0 * c * c * k2dd - (2.0 * c * k1 if dim_x == dim_y else 0.0))
        if y is None:
            idx = np.arange(res.shape[-1])
            res[..., idx, idx] += diag_add
            if diag_vec is not None:
                res[..., idx, idx] += diag_vec.detach().cpu().numpy().reshape(res.shape[:-2] + (res.shape[-1],))
        return self._deliver(self._t(res, x), out, accumulate)

    def kmat_diff_vjp(self, terms, x, y, dim_x, dim_y, g, want_gradx=False):
        """``HipBackend.kmat_diff_vjp`` in NumPy (fp64), from the closed forms in ``include/gpk.h`` (gpk_kmat_diff_vjp)."""
        import numpy as np

        if dim_x is None and dim_y is None:
            raise ValueError("a derivative block differentiates at least one argument")
        a = x.detach().cpu().numpy().astype(np.float64)
        b = y.detach().cpu().numpy().astype(np.float64)
        G = g.detach().cpu().numpy().astype(np.float64)
        n, d = a.shape
        for dim in (dim_x, dim_y):
            if dim is not None and not 0 <= dim < d:
                raise ValueError(f"dimension {dim} outside the {d} input dimensions")
        mixed = dim_x is not None and dim_y is not None
        if want_gradx and (mixed or d > 8):
            raise RuntimeError("libgpk gpk_kmat_diff_vjp failed with status -19")
        df = a[:, None, :] - b[None, :, :]
        r2 = (df ** 2).sum(-1)
        da = df[..., dim_x] if dim_x is not None else None
        db = df[..., dim_y] if dim_y is not None else None
        sd = None if mixed else (da if dim_y is None else -db)      # D_a, or -D_b
        same = mixed and dim_x == dim_y
        sel = dim_x if dim_y is None else dim_y
        shapes = terms.shapes or [None] * len(terms)
        S = np.zeros((len(terms), 2 if terms.shapes is None else 3))
        cD, cS = np.zeros_like(r2), np.zeros_like(r2)
        for t, ((kind, v, scale), al) in enumerate(zip(terms.terms, shapes)):
            c = (1.0 / scale) ** 2
            if kind == "const":
                continue
            if kind == "linear":
                if dim_y is None:
                    be = c * b[None, :, dim_x]
                elif dim_x is None:
                    be = c * a[:, None, dim_y]
                else:
                    be = c * float(same)
                S[t, 0] = S[t, 1] = (G * be).sum()
                if dim_x is None:
                    cS += v * c
                continue
            q = c * r2
            k1a = k2a = 0.0
            if kind == "eq":
                e = np.exp(-0.5 * q)
                k1, k2, qk2, m3 = -0.5 * e, 0.25 * e, 0.25 * q * e, e * (0.5 - 0.125 * q)
            elif kind == "matern32":
                s = np.sqrt(3.0 * q)
                e = np.exp(-s)
                with np.errstate(divide="ignore", invalid="ignore"):
                    inv = np.where(s > 0, 1.0 / np.where(s > 0, s, 1.0), 0.0)
                k1, k2, qk2, m3 = -1.5 * e, 2.25 * e * inv, 0.75 * s * e, 1.125 * (3.0 - s) * e * inv
            elif kind == "matern52":
                s = np.sqrt(5.0 * q)
                e = np.exp(-s)
                k1, k2, qk2, m3 = -(5.0 / 6.0) * (1.0 + s) * e, (25.0 / 12.0) * e, (5.0 / 12.0) * s * s * e, e * (25.0 / 6.0 - 25.0 / 24.0 * s)
            elif kind == "rq":
                u = q / (2.0 * al)
                lg, ri = np.log1p(u), 1.0 / (1.0 + u)
                p1 = np.exp(-(al + 1.0) * lg)
                p2 = p1 * ri
                w = u * ri / al
                r2c = (al + 1.0) / (4.0 * al)
                k1, k2 = -0.5 * p1, r2c * p2
                qk2 = q * k2
                m3 = k2 * (2.0 - q * ri * (al + 2.0) / (2.0 * al))
                k1a = -0.5 * p1 * ((al + 1.0) * w - lg)
                k2a = r2c * p2 * ((al + 2.0) * w - lg) - p2 / (4.0 * al * al)
            else:
                raise NotImplementedError(f"a {kind!r} term has no derivative")
            if mixed:
                f, h = -4.0 * c * c * da * db, (-2.0 * c if same else 0.0)
                be, bc, ba = f * k2 + h * k1, f * m3 + h * (k1 + qk2), f * k2a + h * k1a
            else:
                f = 2.0 * c * sd
                be, bc, ba = f * k1, f * (k1 + qk2), f * k1a
                cD += v * 2.0 * c * f * k2
                cS += (2.0 if dim_y is None else -2.0) * v * c * k1
            S[t, 0], S[t, 1] = (G * be).sum(), (G * bc).sum()
            if kind == "rq":
                S[t, 2] = (G * ba).sum()
        gradx = None
        if want_gradx:
            gradx = ((G * cD)[:, :, None] * df).sum(1)
            gradx[:, sel] += (G * cS).sum(1)
        return self._t(S, x), (self._t(gradx, x) if want_gradx else None)

    def potrf_vjp(self, l, dinv_sb, sb, lbar):
        """``HipBackend.potrf_vjp`` in NumPy (fp64, rounded to the factor's dtype), the formula of ``include/gpk.h`` (gpk_potrf_vjp):
        ``abar = W^T Psym W``, ``W = L^{-1}``, ``Psym = (P + P^T) / 2``, ``P = Phi(L^T tril(lbar))``; the strict upper triangles of ``l``
        and ``lbar`` are not read."""
        import numpy as np

        L = np.tril(l.detach().cpu().numpy().astype(np.float64))
        P = np.tril(L.T @ np.tril(lbar.detach().cpu().numpy().astype(np.float64)))
        P[np.diag_indices_from(P)] *= 0.5
        W = np.linalg.inv(L)
        abar = W.T @ (0.5 * (P + P.T)) @ W
        return self._t(0.5 * (abar + abar.T), l)

    def nuclear_norm(self, m, iters=None):
        """``HipBackend.nuclear_norm`` by its definition: the sum of the singular values (``numpy.linalg.svd`` in fp64, rounded to the
        input's dtype) -- no iteration, so ``iters`` has no effect here."""
        import numpy as np

        if m.dim() < 2 or m.shape[-1] != m.shape[-2]:
            raise ValueError("nuclear_norm takes square matrices (..., n, n)")
        a = m.detach().cpu().numpy().astype(np.float64)
        if a.shape[-1] == 0:
            return self._t(np.zeros(a.shape[:-2]), m)
        return self._t(np.linalg.svd(a, compute_uv=False).sum(-1), m)

    def kdiag(self, terms, x):
        if terms.batch is not None:
            x3 = self._batch3(terms, x)
            return torch.stack([self.kdiag(terms.entry(b), x3[b]) for b in range(x3.shape[0])]).reshape(tuple(x.shape[:-1]))
        rest, delta, _ = self._split(terms)
        if not delta:
            return self._inner.kdiag(terms, x)
        base = self._inner.kdiag(rest, x) if len(rest) else torch.zeros(x.shape[:-1], dtype=x.dtype, device=x.device)
        return base + sum(var for _, (_, var, _), _ in delta)

    def _merge_sums(self, terms, S_rest, keep, delta, sums):
        S = torch.zeros((len(terms), 3), dtype=S_rest.dtype, device=S_rest.device)
        if keep:
            S[keep, : S_rest.shape[1]] = S_rest
        for (i, _, _), v in zip(delta, sums):
            S[i, 0] = v
        return S

    def kmat_vjp(self, terms, x, kinv, alpha, g):
        import numpy as np

        rest, delta, keep = self._split(terms)
        if not delta:
            return self._inner.kmat_vjp(terms, x, kinv, alpha, g)
        S_rest, tr, dg = self._inner.kmat_vjp(rest, x, kinv, alpha, g)
        ki = kinv.detach().cpu().numpy()
        ki = np.tril(ki) + np.tril(ki, -1).T
        A, gv = alpha.detach().cpu().numpy(), np.asarray(g, dtype=np.float64)
        G = 0.5 * ((A * gv) @ A.T - gv.sum() * ki)
        sums = [float(np.sum(G * self._kappa(x, x, scale, eps))) for _, (_, _, scale), eps in delta]
        return self._merge_sums(terms, S_rest, keep, delta, sums), tr, dg

    def kmat_vjp_dense(self, terms, x, y, g, colscale=None, w=None, b=None, want_colsum=False, want_gradx=False):
        rest, delta, keep = self._split(terms)
        if not delta:
            return self._inner.kmat_vjp_dense(terms, x, y, g, colscale, w, b, want_colsum=want_colsum, want_gradx=want_gradx)
        S_rest, colsum, gradx = self._inner.kmat_vjp_dense(rest, x, y, g, colscale, w, b, want_colsum=want_colsum, want_gradx=want_gradx)
        Ge = g.detach().cpu().numpy().copy()
        if colscale is not None:
            Ge = Ge * colscale.detach().cpu().numpy()[None, :]
        if w is not None:
            Ge = Ge + w.detach().cpu().numpy()[:, None] * b.detach().cpu().numpy()[None, :]
        sums = []
        for _, (_, var, scale), eps in delta:          # piecewise constant: S1 and the column sums, nothing for the scale or the inputs
            k = self._kappa(x, y, scale, eps)
            sums.append(float((Ge * k).sum()))
            if want_colsum:
                colsum = colsum + self._t(var * (Ge * k).sum(0), colsum)
        return self._merge_sums(terms, S_rest, keep, delta, sums), colsum, gradx


_backend = None


def get_backend():
    """The op backend; instantiates :class:`HipBackend` on first use (raises if
    ``libgpk.so`` is not built)."""
    global _backend
    if _backend is None:
        _backend = HipBackend()
    return _backend


def set_backend(backend):
    """Install an op backend.  TEST HOOK ONLY (host-logic unit tests without a GPU);
    returns the previous backend.  A backend other than the HIP one is wrapped in :class:`_HostDelta`."""
    global _backend
    if backend is not None and not isinstance(backend, _HostDelta) and getattr(backend, "name", None) != "hip":
        backend = _HostDelta(backend)
    prev, _backend = _backend, backend
    return prev
