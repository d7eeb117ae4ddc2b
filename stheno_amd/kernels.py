"""Kernels and means on the GP hot path -- the slice of the reference's ``mlkernels``
dependency that ``stheno/model/*.py`` uses:

* primitives ``EQ``, ``RQ``, ``Exp``/``Matern12``, ``Matern32``, ``Matern52``, ``Linear``, ``Delta``,
  ``OneKernel``, ``ZeroKernel`` with the ``v * k``, ``k1 + k2``, ``k.stretch(l)``, ``k.periodic(p)`` algebra
  (usage: ``readme_example13_optimisation_torch.py:34``, ``tests/model/test_cases.py:138``,
  ``readme_example1_simple_regression.py``);
* ``pairwise`` (``k(x, y)``) and ``elwise`` (``k.elwise(x)``) evaluation -- one fused HIP
  kernel launch per call for any sum of primitives (``gpk_kmat`` / ``gpk_kdiag``);
* ``k.diff(dim)`` / ``m.diff(dim)`` (``DiffKernel``, ``DiffMean``; mlkernels' ``DerivativeKernel`` behind ``GP.diff``,
  ``stheno/model/measure.py:343-360``): first derivatives in either argument, one fused launch per block (``gpk_kmat_diff``);
* ``PosteriorKernel``, ``PosteriorMean``, ``SubspaceKernel`` (constructed at
  ``stheno/model/observations.py:148-168,256-277``) and ``mean_var`` / ``mean_var_diag``
  (``stheno/model/fdd.py:69,73``), which share one ``L^{-1} k(z, x)`` between the mean and
  the variance and never form the N* x N* covariance for marginals.

Inputs follow the reference's conventions: ``(N,)`` -> ``(N, 1)``; ``(N, D)``;
``(B, N, D)`` batched.
"""
import numpy as np
import torch

from . import ops
from .matrix import Dense, KernelDense

__all__ = [
    "Kernel", "EQ", "RQ", "Delta", "Periodic", "Exp", "Matern12", "Matern32", "Matern52", "Linear", "OneKernel", "ZeroKernel",
    "Mean", "ZeroMean", "OneMean", "PosteriorKernel", "PosteriorMean", "SubspaceKernel",
    "mean_var", "mean_var_diag", "uprank", "num_elements",
    "MultiInput", "MultiOutputKernel", "MultiOutputMean", "InputScaled", "DiffKernel", "DiffMean", "ScaleFn", "FnScaled",
]


class MultiInput:
    """Inputs of a Cartesian product of processes (``cross(f1, f2)((f1(x1), f2(x2)))``): the
    role of the reference's tuple-of-FDDs input (``stheno/mo/input.py:7-36``,
    ``stheno/model/observations.py:28-47``).  ``parts`` is a list of ``(process, x_i)`` with
    ``x_i`` upranked; the object quacks like an ``(N_1 + ... + N_k, .)`` input where the host
    code only asks for ``dtype`` / ``device`` / the number of rows."""

    def __init__(self, parts):
        self.parts = [(p, uprank(x)) for p, x in parts]
        if not self.parts:
            raise ValueError("a multi-input needs at least one part")
        if len({tuple(x.shape[:-2]) for _, x in self.parts}) != 1:
            raise ValueError("the parts of a multi-process input must share their batch dimensions")

    dtype = property(lambda self: self.parts[0][1].dtype)
    device = property(lambda self: self.parts[0][1].device)
    # rows each part contributes: a plain input under a product process stands for ALL its components
    sizes = property(lambda self: [p.kernel.num_outputs(x) for p, x in self.parts])
    shape = property(lambda self: tuple(self.parts[0][1].shape[:-2]) + (sum(self.sizes), 1))

    def dim(self):
        return self.parts[0][1].dim()

    def offsets(self):
        out, o = [], 0
        for n in self.sizes:
            out.append((o, o + n))
            o += n
        return out

    def __getitem__(self, idx):
        """Row selection by a sorted index vector (``B.take`` on the observations, ``fdd.py:125-132``)."""
        if not (torch.is_tensor(idx) and idx.dim() == 1 and idx.dtype == torch.long):
            raise TypeError("a multi-input is sub-selected by an index vector")
        parts = []
        for (p, x), (a, b) in zip(self.parts, self.offsets()):
            sel = idx[(idx >= a) & (idx < b)] - a
            parts.append((p, x[sel]))
        return MultiInput(parts)

    def __repr__(self):
        return "MultiInput(" + ", ".join(f"{tuple(x.shape)}" for _, x in self.parts) + ")"


def uprank(x):
    """``B.uprank``: scalars and vectors become column matrices."""
    if isinstance(x, MultiInput):
        return x
    if not torch.is_tensor(x):
        # host data (NumPy arrays, lists, Python numbers -- what the reference's default backend is fed): one copy to the
        # device the HIP backend computes on; tensors stay where the caller put them (a CPU tensor is refused by the backend)
        x = torch.as_tensor(x)
        if ops.get_backend().name == "hip":
            x = x.to(torch.device("cuda", torch.cuda.current_device()))
    if x.dim() == 0:
        return x.reshape(1, 1)
    if x.dim() == 1:
        return x[:, None]
    return x


def num_elements(x):
    """``mlkernels.num_elements``: number of inputs (rows)."""
    x = uprank(x)
    return x.shape[-2]


PER_BATCH = "per-batch hyper-parameters"


def _is_per_batch(v):
    """A hyper-parameter given once per batch entry: a tensor of shape ``(B, 1, 1)``, ``B > 1`` -- the shape that broadcasts against a
    ``(B, N, M)`` kernel matrix and ``(B, N, D)`` inputs.  (A 1-D tensor stays what it was: one length scale per input dimension in
    ``stretch``, an error as a variance.)"""
    return torch.is_tensor(v) and v.dim() == 3 and v.shape[0] > 1 and v.shape[1] == 1 and v.shape[2] == 1


def _per_batch_size(v):
    """``B`` of a per-batch value in either view -- ``(B, 1, 1)`` as the caller gave it, ``(B,)`` in the float view -- else None."""
    return v.shape[0] if torch.is_tensor(v) and v.dim() in (1, 3) and v.numel() > 1 else None


def _same_batch(a, b):
    """Refuse to combine per-batch values of different batch sizes (torch would raise a broadcasting error, or broadcast)."""
    na, nb = _per_batch_size(a), _per_batch_size(b)
    if na is not None and nb is not None and na != nb:
        raise ValueError(f"{PER_BATCH} of different batch sizes in one kernel: {na} and {nb}")


def _times(a, b):
    _same_batch(a, b)
    return a * b


def _as_float(v):
    """The float view of a parameter: a Python double; for a per-batch parameter its values as a detached fp64 vector ``(B,)``."""
    if torch.is_tensor(v):
        if _is_per_batch(v):
            return v.detach().reshape(-1).to(torch.float64)
        if v.numel() != 1:
            raise ValueError("kernel hyper-parameters must be scalars")
        return float(v.detach())
    return float(v)


def _as_factor(v):
    """A parameter as a factor of an evaluated kernel matrix ``(..., N, M)``: a float, or the detached ``(B, 1, 1)`` values."""
    return v.detach() if _is_per_batch(v) else _as_float(v)


_UNSET = object()


def _is_vector_scale(scale):
    """One length scale per input dimension (torch tensor, NumPy array, list or tuple with more than one entry)?"""
    if torch.is_tensor(scale):
        return scale.numel() > 1 and not _is_per_batch(scale)
    if isinstance(scale, (list, tuple)):
        return True
    return np.ndim(scale) > 0 and np.size(scale) > 1


def _as_is(v):
    """The conversion of the tensor views (``Kernel._table``): parameters are stored as ``_as_param`` left them."""
    return v


def _as_param(v):
    """Keep scalar tensors (they may carry an autograd graph: learnable hyper-parameters) and per-batch tensors ``(B, 1, 1)`` -- the
    caller's object --, turn everything else into a float."""
    if torch.is_tensor(v):
        if _is_per_batch(v):
            return v
        if v.numel() != 1:
            raise ValueError("kernel hyper-parameters must be scalars")
        return v.reshape(())
    return float(v)


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
class Kernel:
    """Base class.  A kernel that is a sum of stretched/scaled primitives describes itself in ONE method, ``_table(conv)`` -> rows
    ``(kind, variance, scale, shape)`` (``shape``: ``RQ``'s alpha, ``Delta``'s epsilon, ``None`` for the kinds without one); other
    kernels leave it at ``None`` and override ``pairwise`` / ``elwise``.  ``conv`` is applied to the node's OWN parameter before it is
    combined with its children's: ``_as_float`` for the float views (Python doubles: what the fused launches are handed),
    ``_as_is`` for the tensor views (the caller's tensors, so gradients can flow back to them).  The four public views below are
    columns of that table; one call visits every leaf of the expression once.

    A parameter given once per batch entry -- a tensor of shape ``(B, 1, 1)`` -- stays the caller's tensor in the tensor view and is
    a detached fp64 vector ``(B,)`` in the float view; products with scalar parameters broadcast, so a table mixes both freely and
    ``_kterms()`` hands the backends a per-batch descriptor (``ops.KTerms.batch``)."""

    stationary = False

    def _table(self, conv):
        return None

    def terms(self):
        """``[(kind, variance, scale)]`` in floats; None when the kernel is no sum of primitives, ``[]`` for the zero kernel."""
        rows = self._table(_as_float)
        return None if rows is None else [row[:3] for row in rows]

    def tensor_table(self):
        """The whole table in its tensor view (what the differentiable paths pack: ``autograd._pack``), or None."""
        return self._table(_as_is)

    def tensor_terms(self):
        """Like ``terms()`` but variances / scales stay scalar tensors where the user gave tensors."""
        rows = self.tensor_table()
        return None if rows is None else [row[:3] for row in rows]

    def shapes(self):
        """One shape parameter per entry of ``terms()`` (a float; ``None`` for kinds without one), or None like ``terms()``."""
        rows = self._table(_as_float)
        return None if rows is None else [row[3] for row in rows]

    def tensor_shapes(self):
        """Like ``shapes()``, beside ``tensor_terms()``: a tensor the user gave stays that tensor."""
        rows = self.tensor_table()
        return None if rows is None else [row[3] for row in rows]

    def _kterms(self, factor=1.0):
        """The float view as the backends' descriptor, every variance times ``factor``; None when the kernel is no sum of primitives."""
        rows = self._table(_as_float)
        if rows is None:
            return None
        return ops.KTerms([(kind, var * factor, s) for kind, var, s, _ in rows], [row[3] for row in rows])

    def num_outputs(self, x):
        return num_elements(x)

    def input_scaled_view(self):
        """``(k, imap_x, imap_y)`` such that ``self(x, y) == k(imap_x(x), imap_y(y))`` with ``k`` a sum of primitives
        (``k.terms()`` is not None) and each ``imap`` a differentiable map of the inputs (:class:`InputMap`: the division by
        per-dimension length scales of ``k.stretch(vector)``, the ``(sin, cos)`` embedding of ``k.periodic(p)``, a shift, a selection of
        dimensions, a feature map, a chain of those), or None for "inputs as they are"; None when the kernel has no such form.  A kernel
        that sees both arguments through the same map -- every kernel of a process with itself -- carries that map twice
        (``_same_map(imap_x, imap_y)``); the two differ for cross-kernels such as ``k.shift(c, 0)``, the covariance of ``f.shift(c)``
        with ``f``.  The differentiable paths run ``k`` on the mapped inputs and leave the maps to torch, which carries the gradient to
        their parameters (length scales, period, shift, the weights of a feature map) and to ``x``."""
        return (self, None, None) if self.terms() is not None else None

    # -- evaluation ------------------------------------------------------------
    def pairwise(self, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, cache=None, out=None, accumulate=False):
        """``k(x, y)`` as a tensor (..., N, M); ``y is None``: symmetric case, where
        ``diag_add`` / ``diag_vec`` are added to the diagonal in the same pass.  ``out``: a
        (strided) matrix view to write into (blocks of a multi-output kernel matrix); ``accumulate``: add to it
        (the groups of a sum whose terms see differently mapped inputs)."""
        kt = self._kterms()
        if kt is None:
            raise NotImplementedError(f"pairwise evaluation is not implemented for {type(self).__name__}")
        x = uprank(x)
        y = None if y is None else uprank(y)
        if isinstance(x, MultiInput) or isinstance(y, MultiInput):
            raise ValueError(f"{type(self).__name__} is a single-output kernel; it cannot take multi-process inputs")
        return ops.get_backend().kmat(kt, x, y, lower=lower, diag_add=diag_add, diag_vec=diag_vec, out=out, accumulate=accumulate)

    def elwise(self, x, y=None, *, cache=None):
        """``k(x_i, x_i)`` as a column (..., N, 1)."""
        if y is not None and y is not x:
            raise NotImplementedError("elwise is implemented for identical inputs")
        kt = self._kterms()
        if kt is None:
            raise NotImplementedError(f"elwise evaluation is not implemented for {type(self).__name__}")
        return ops.get_backend().kdiag(kt, uprank(x))[..., None]

    def __call__(self, x, y=None):
        """``k(x)`` / ``k(x, y)`` as a ``Dense`` matrix (lazily materialised for ``k(x)``)."""
        if y is None:
            return KernelDense(self, uprank(x), None)
        return Dense(self.pairwise(x, y))

    # -- algebra ---------------------------------------------------------------
    def __add__(self, other):
        if isinstance(other, (int, float)):
            if other == 0:
                return self
            other = other * OneKernel()
        if isinstance(other, ZeroKernel):
            return self
        if isinstance(self, ZeroKernel):
            return other
        if not isinstance(other, Kernel):
            return NotImplemented
        return Sum(self, other)

    __radd__ = __add__

    def __mul__(self, other):
        # (a Kernel is itself callable: asked first)
        if isinstance(other, Kernel):
            raise NotImplementedError("products of kernels are outside the accelerated path")
        if callable(other) and not torch.is_tensor(other):
            # k * fn: fn(x) k(x, y) fn(y), mlkernels' k * TensorProductKernel(fn)
            fn = other if isinstance(other, ScaleFn) else ScaleFn(other)
            return _fn_scaled(self, fn, fn)
        v = _as_param(other)
        if isinstance(self, ZeroKernel) or (not torch.is_tensor(v) and v == 0):
            return ZeroKernel()
        return Scaled(self, v)

    __rmul__ = __mul__

    def stretch(self, scale, scale_y=_UNSET):
        """``k.stretch(l)``: ``k(x / l, y / l)``.  ``l``: a scalar, or one length scale per input dimension.
        ``k.stretch(l_x, l_y)``: ``k(x / l_x, y / l_y)``, scalars only (the cross-kernel of ``f.stretch(l)`` with ``f`` is
        ``k.stretch(l, 1)``, its kernel ``k.stretch(l, l)``).  The two-argument form always divides the INPUTS; the one-argument form
        of a periodic kernel hands the stretch to the kernel behind the embedding, as it always did."""
        _refuse_fn_scaled(self, "input maps (stretch)")
        if scale_y is not _UNSET:
            if _is_per_batch(scale) or _is_per_batch(scale_y) or has_per_batch(self):
                raise NotImplementedError(f"the two-argument stretch is not implemented with {PER_BATCH}")
            if _is_vector_scale(scale) or _is_vector_scale(scale_y):
                raise NotImplementedError("the two-argument stretch takes scalars: per-dimension length scales that differ between the "
                                          "arguments are not implemented")
            return _stretch_arguments(self, scale, scale_y)
        if _is_vector_scale(scale):
            return InputScaled(self, scale)
        if self.terms() is None and _map_groups(self) is not None:
            return _stretch_groups(self, _as_param(scale))
        return Stretched(self, _as_param(scale))

    def shift(self, c, c_y=_UNSET):
        """``k.shift(c)``: ``k(x - c, y - c)`` (a stationary kernel is its own shift: ``k`` itself comes back);
        ``k.shift(c_x, c_y)``: ``k(x - c_x, y - c_y)``.  ``c``: a number, a 0-dim tensor or one entry per input dimension, kept as
        given (a learnable lag); the number ``0`` leaves that argument as it is."""
        _refuse_fn_scaled(self, "input maps (shift)")
        if c_y is _UNSET:
            if self.stationary:
                return self
            c_y = c
        mx = None if _is_number(c, 0) else _ShiftMap(c)
        return _behind(self, mx, mx if c_y is c else (None if _is_number(c_y, 0) else _ShiftMap(c_y)))

    def select(self, dims, dims_y=_UNSET):
        """``k.select(dims)``: ``k(x[:, dims], y[:, dims])``; ``k.select(dims_x, dims_y)``: one selection per argument, ``None`` leaves
        that argument as it is.  ``dims``: an input dimension or a sequence of them."""
        _refuse_fn_scaled(self, "input maps (select)")
        mx = None if dims is None else _SelectMap(dims)
        return _behind(self, mx, mx if dims_y is _UNSET else (None if dims_y is None else _SelectMap(dims_y)))

    def transform(self, fn, fn_y=_UNSET):
        """``k.transform(fn)``: ``k(fn(x), fn(y))`` for a callable from ``(..., N, D)`` to ``(..., N, D')`` -- a warping, a feature
        map, a small ``torch.nn`` network whose parameters are learnt through ``logpdf``; ``k.transform(fn_x, fn_y)``: one per argument,
        ``None`` is the identity."""
        _refuse_fn_scaled(self, "input maps (transform)")
        mx = None if fn is None else _TransformMap(fn)
        return _behind(self, mx, mx if fn_y is _UNSET else (None if fn_y is None else _TransformMap(fn_y)))

    def periodic(self, period):
        """``k.periodic(p)``: ``k`` on ``(sin(2 pi x / p), cos(2 pi x / p))`` (mlkernels' ``Periodic``).  ``p``: a positive scalar,
        or one period per input dimension."""
        _refuse_fn_scaled(self, "input maps (periodic)")
        return Periodic(self, period)

    def diff(self, *dims):
        """``k.diff(dim)``: the derivative with respect to input dimension ``dim`` of BOTH arguments, ``d^2 k / dx[dim] dy[dim]`` -- the
        kernel of ``f.diff(dim)``; ``k.diff(dim_x, dim_y)``: either may be ``None`` (that argument is not differentiated) --
        ``k.diff(dim, None)`` is the covariance of ``f.diff(dim)`` with ``f``."""
        if len(dims) == 1:
            dims = (dims[0], dims[0])
        if len(dims) != 2:
            raise TypeError("diff(dim) or diff(dim_x, dim_y)")
        _refuse_fn_scaled(self, "derivatives")
        return _diff_kernel(self, *(None if v is None else _as_dim(v) for v in dims))

    def __reversed__(self):
        # sums of (stretched / scaled) primitives are symmetric, the zero kernel included -- and so are they behind input maps
        # (... unless a group sees its two arguments through different maps: then the maps change places, group by group)
        if self.terms() is not None or _symmetric_groups(self) is not None:
            return self
        groups = _map_groups(self)
        if groups is not None:
            return _sum_of_groups([(kern, my, mx) for kern, mx, my in groups])
        return Reversed(self)

    def __eq__(self, other):
        if isinstance(self, ZeroKernel) and isinstance(other, ZeroKernel):
            return True
        return self is other

    def __hash__(self):
        return id(self)


class _Primitive(Kernel):
    kind = None
    shape = None          # the kind's shape parameter, for those that have one

    def _table(self, conv):
        return [(self.kind, 1.0, 1.0, None if self.shape is None else conv(self.shape))]

    def __repr__(self):
        return f"{type(self).__name__}()"


class EQ(_Primitive):
    """Exponentiated quadratic ``exp(-r^2 / 2)``."""
    kind = "eq"
    stationary = True


class RQ(_Primitive):
    """Rational quadratic ``(1 + r^2 / (2 alpha))^(-alpha)`` (mlkernels' ``RQ(alpha)``).  ``alpha``: a positive number, or a
    scalar tensor -- kept as the caller's object (a learnable shape parameter, like a length scale)."""
    kind = "rq"
    stationary = True

    def __init__(self, alpha):
        if _is_per_batch(alpha):
            self.alpha = alpha               # one alpha per batch entry: the caller's (B, 1, 1) tensor
        elif torch.is_tensor(alpha):
            if alpha.numel() != 1:
                raise ValueError("kernel hyper-parameters must be scalars")
            self.alpha = alpha if alpha.dim() == 0 else alpha.reshape(())
        else:
            self.alpha = float(alpha)
        if not bool((torch.as_tensor(_as_float(self.alpha)) > 0).all()):
            raise ValueError("the shape parameter alpha of RQ must be positive")

    shape = property(lambda self: self.alpha)

    def __repr__(self):
        return f"RQ({PER_BATCH})" if _is_per_batch(self.alpha) else f"RQ({_as_float(self.alpha):g})"


class Delta(_Primitive):
    """Kronecker delta ``1 if r^2 < epsilon else 0`` (mlkernels' ``Delta(epsilon=1e-6)``): the kernel of a noise process,
    ``e = GP(v * Delta())`` in ``y = f + e``.  ``r^2`` is the squared distance of the inputs as the term sees them (after a stretch or an
    input map).  ``epsilon``: a positive number -- a threshold, not a hyper-parameter: a tensor that requires a gradient is refused."""
    kind = "delta"
    stationary = True

    def __init__(self, epsilon=1e-6):
        if torch.is_tensor(epsilon) and epsilon.requires_grad:
            raise ValueError("the epsilon of Delta is not learnable (the kernel is piecewise constant in it); pass a number")
        if _is_per_batch(epsilon):
            raise ValueError("the epsilon of Delta is a number (a threshold shared by the batch), not one value per batch entry")
        self.epsilon = _as_float(epsilon)
        if not self.epsilon > 0:
            raise ValueError("the epsilon of Delta must be positive")

    shape = property(lambda self: self.epsilon)

    def __repr__(self):
        return f"Delta({self.epsilon:g})"


class Matern12(_Primitive):
    """Exponential kernel ``exp(-r)``."""
    kind = "matern12"
    stationary = True


Exp = Matern12


class Matern32(_Primitive):
    kind = "matern32"
    stationary = True


class Matern52(_Primitive):
    kind = "matern52"
    stationary = True


class Linear(_Primitive):
    """``<x, y>``."""
    kind = "linear"


class OneKernel(_Primitive):
    kind = "const"
    stationary = True


class ZeroKernel(Kernel):
    stationary = True

    def _table(self, conv):
        return []

    def pairwise(self, x, y=None, *, out=None, diag_add=0.0, diag_vec=None, **kw):
        x = uprank(x)
        sym = y is None
        y = x if sym else uprank(y)
        shape = tuple(x.shape[:-1]) + (y.shape[-2],)
        if out is not None:               # a caller's (strided) view: the zeros go THERE (blocks of one buffer, rows under a matrix)
            if tuple(out.shape) != shape:
                raise ValueError(f"out has shape {tuple(out.shape)}, the kernel matrix {shape}")
            out.zero_()
        else:
            out = torch.zeros(shape, dtype=x.dtype, device=x.device)
        return _add_diag(out, diag_add, diag_vec) if sym else out      # (noise / jitter of `k(x) + noise`: the diagonal is all there is)

    def elwise(self, x, y=None, **kw):
        x = uprank(x)
        return torch.zeros(x.shape[:-1] + (1,), dtype=x.dtype, device=x.device)

    def __repr__(self):
        return "0"


class Scaled(Kernel):
    def __init__(self, k, v):
        self.k, self.v = k, v
        self.stationary = k.stationary

    def num_outputs(self, x):
        return self.k.num_outputs(x)

    def _table(self, conv):
        rows = self.k._table(conv)
        return None if rows is None else [(kind, _times(var, conv(self.v)), s, a) for kind, var, s, a in rows]

    def input_scaled_view(self):
        v = self.k.input_scaled_view()
        return None if v is None else (Scaled(v[0], self.v), v[1], v[2])

    def pairwise(self, x, y=None, **kw):
        if self.terms() is not None:
            return super().pairwise(x, y, **kw)
        view = self.input_scaled_view()
        if view is not None:                       # v * k0(x / l): still ONE fused launch, on the divided inputs
            return _Mapped(*view).pairwise(x, y, **kw)
        if kw.get("out") is not None or kw.get("accumulate"):
            # a caller's view (a block of a multi-process matrix, rows under a matrix): the product below would leave it in a new
            # tensor -- a scaled sum behind different maps goes group by group into the view, the factor in each group's variances
            groups = _map_groups(self)
            if groups is not None:
                return _sum_of_groups(groups).pairwise(x, y, **kw)
        groups = _scaled_groups(self)
        if groups is not None:                     # ... and so does a sum with function-scaled groups, with or without a view
            return _pairwise_groups(groups, x, y, kw)
        da, dv = kw.pop("diag_add", 0.0), kw.pop("diag_vec", None)
        out = _as_factor(self.v) * self.k.pairwise(x, y, **kw)
        return _add_diag(out, da, dv) if y is None else out

    def elwise(self, x, y=None, **kw):
        if self.terms() is not None:
            return super().elwise(x, y, **kw)
        view = self.input_scaled_view()
        if view is not None:
            return _Mapped(*view).elwise(x, y, **kw)
        return _as_factor(self.v) * self.k.elwise(x, y, **kw)

    def __repr__(self):
        return f"{self.v} * {self.k!r}"


class Stretched(Kernel):
    def __init__(self, k, scale):
        if k.terms() is None:
            raise NotImplementedError("stretch is implemented for sums of primitive kernels")
        self.k, self.scale = k, scale
        self.stationary = k.stationary

    def _table(self, conv):
        return [(kind, var, _times(s, conv(self.scale)), a) for kind, var, s, a in self.k._table(conv)]

    def __repr__(self):
        return f"({self.k!r} > {self.scale})"


class InputMap:
    """A differentiable map of the inputs in front of a sum of primitives: ``k(x, y) = k0(imap(x), imap(y))``.  ``imap(x)`` is a
    torch expression (gradients reach the map's parameter and ``x``), ``imap.values(x)`` the same numbers cut off from the graph
    (what the fused launch of a plain evaluation sees).  The map costs O(N D); the kernel matrix behind it is the unchanged
    fused launch, lower-triangle-only / in-place-factorisable like any other."""

    param = None          # the tensor (or host value) the map depends on
    keeps_stationary = True      # k0(m(x), m(y)) of a stationary k0 is still a function of x - y (a feature map: not in general)

    def __call__(self, x):
        raise NotImplementedError

    def values(self, x):
        with torch.no_grad():
            return self(x.detach())

    @property
    def requires_grad(self):
        return bool(torch.is_tensor(self.param) and self.param.requires_grad)

    def stamp(self):
        """Identity + version of the parameter (what a cached comparison of two maps was made for); None: nothing vouches for it."""
        if not torch.is_tensor(self.param):
            return (id(self), 0)
        return _scale_stamp(self.param)

    def same(self, other):
        """The same map as ``other``?  (Learnable parameters are the same only if they are the same tensor.)"""
        if type(other) is not type(self):
            return False
        a, b = self.param, other.param
        if a is b:
            return True
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            if torch.is_tensor(a) or torch.is_tensor(b):
                return False
            return bool(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)))
        return bool(a.shape == b.shape and not a.requires_grad and not b.requires_grad
                    and (a.data_ptr() == b.data_ptr() and a.device == b.device and a.dtype == b.dtype
                         or bool(torch.equal(a, b.to(a)))))


class _ScaleMap(InputMap):
    """``x / scales``: one length scale per input dimension."""

    def __init__(self, scales):
        self.param = scales

    def __call__(self, x):
        if x.shape[-1] != self.param.numel():
            raise ValueError(f"inputs have {x.shape[-1]} dimensions, the kernel has {self.param.numel()} length scales")
        return x / self.param.to(dtype=x.dtype, device=x.device)


class _PeriodMap(InputMap):
    """``x -> cat(sin(2 pi x / p), cos(2 pi x / p))``: squared distances become ``4 sum_d sin^2(pi (x_d - y_d) / p_d)``."""

    def __init__(self, period):
        self.param = period

    def __call__(self, x):
        p = self.param
        p = p.to(dtype=x.dtype, device=x.device) if torch.is_tensor(p) else torch.as_tensor(p, dtype=x.dtype, device=x.device)
        if p.numel() > 1:
            p = p.reshape(-1)
            if p.numel() != x.shape[-1]:
                raise ValueError(f"inputs have {x.shape[-1]} dimensions, the kernel has {p.numel()} periods")
        a = (2.0 * np.pi) * x / p
        return torch.cat([torch.sin(a), torch.cos(a)], dim=-1)


class _ShiftMap(InputMap):
    """``x - c``: ``c`` a number, a 0-dim tensor, or one entry per input dimension (kept as given: a learnable lag)."""

    def __init__(self, c):
        if not torch.is_tensor(c) and np.ndim(c) > 0:
            c = tuple(float(v) for v in np.asarray(c, dtype=np.float64).reshape(-1))
        elif not torch.is_tensor(c):
            c = float(c)
        elif c.dim() > 1:
            raise ValueError("a shift is a scalar or a vector (one entry per input dimension)")
        self.param = c

    def __call__(self, x):
        c = self.param
        c = c.to(dtype=x.dtype, device=x.device) if torch.is_tensor(c) else torch.as_tensor(c, dtype=x.dtype, device=x.device)
        if c.numel() > 1 and c.numel() != x.shape[-1]:
            raise ValueError(f"inputs have {x.shape[-1]} dimensions, the shift has {c.numel()} entries")
        return x - c


class _StretchMap(InputMap):
    """``x / s`` with a scalar ``s``: a stretch that cannot be folded into the term table, because a shift or a feature map sits behind
    it or because the two arguments are stretched differently."""

    def __init__(self, s):
        self.param = _as_param(s)

    def __call__(self, x):
        s = self.param
        return x / (s.to(dtype=x.dtype, device=x.device) if torch.is_tensor(s) else s)


class _SelectMap(InputMap):
    """``x[..., dims]``: the kernel sees these input dimensions only."""

    def __init__(self, dims):
        dims = [dims] if isinstance(dims, (int, np.integer)) and not isinstance(dims, bool) else list(dims)
        if not dims:
            raise ValueError("select needs at least one input dimension")
        self.param = tuple(_as_dim(d) for d in dims)

    def __call__(self, x):
        if max(self.param) >= x.shape[-1]:
            raise ValueError(f"inputs have {x.shape[-1]} dimensions, the kernel selects dimension {max(self.param)}")
        return x[..., list(self.param)]


class _TransformMap(InputMap):
    """``fn(x)`` for any callable from ``(..., N, D)`` to ``(..., N, D')`` -- a feature map, a warping, a small network.  Two transform
    maps are the same only if they hold the same callable OBJECT, and nothing vouches for a cached comparison (``stamp()`` is None).

    ``requires_grad``: ONE rule for every callable, ``nn.Module`` or not -- the probe.  ``fn`` runs on a detached copy of the first row
    of an input it was given, and the map is learnable if that output requires a gradient: parameters of a module, tensors a
    function or a module's ``forward`` closes over, are all seen this way.  Before the first evaluation nothing is known, and unknown
    counts as learnable: the guards err towards refusing, never towards a value cut off from the graph."""

    keeps_stationary = False

    def __init__(self, fn):
        if not callable(fn):
            raise TypeError("transform takes a callable from (..., N, D) to (..., N, D')")
        self.param = self.fn = fn
        self._probe = None

    def __call__(self, x):
        p = self._probe
        if p is None or p.shape[-1] != x.shape[-1] or p.dtype != x.dtype or p.device != x.device:
            # (one row of its own, taken once per kind of input: the input itself is not kept alive)
            self._probe = x.detach()[(0,) * (x.dim() - 2)][:1].clone()
        out = self.fn(x)
        if not (torch.is_tensor(out) and out.dim() == x.dim() and out.shape[:-1] == x.shape[:-1]):
            raise ValueError(f"a transform maps inputs (..., N, D) to (..., N, D'); got {tuple(getattr(out, 'shape', ()))} for "
                             f"{tuple(x.shape)}")
        return out

    @property
    def requires_grad(self):
        if self._probe is None or self._probe.shape[-2] == 0:
            return True
        with torch.enable_grad():
            out = self.fn(self._probe)
        return bool(torch.is_tensor(out) and out.requires_grad)

    def stamp(self):
        return None

    def same(self, other):
        return type(other) is type(self) and other.fn is self.fn


class _ChainMap(InputMap):
    """Maps applied one after the other, ``maps[0]`` first.  An operation applied LATER in the kernel algebra acts FIRST on the inputs
    (mlkernels): ``k.shift(c).select(0)`` is ``k(x[:, [0]] - c, ...)``, the chain ``(select, shift)``.  Built by :func:`_chain`, which
    flattens nested chains and hands a chain of one element back as that element."""

    def __init__(self, maps):
        self.maps = tuple(maps)
        self.keeps_stationary = all(m.keeps_stationary for m in self.maps)

    param = property(lambda self: tuple(m.param for m in self.maps))

    def __call__(self, x):
        for m in self.maps:
            x = m(x)
        return x

    @property
    def requires_grad(self):
        return any(m.requires_grad for m in self.maps)

    def stamp(self):
        stamps = tuple(m.stamp() for m in self.maps)
        return None if None in stamps else stamps

    def same(self, other):
        return (type(other) is type(self) and len(other.maps) == len(self.maps)
                and all(a.same(b) for a, b in zip(self.maps, other.maps)))


def _chain(first, then):
    """The map ``x -> then(first(x))`` (either may be None: the inputs as they are)."""
    maps = [e for m in (first, then) if m is not None for e in (m.maps if isinstance(m, _ChainMap) else (m,))]
    if not maps:
        return None
    return maps[0] if len(maps) == 1 else _ChainMap(maps)


#: maps a scalar stretch applied in front of them may be folded THROUGH, into the term table behind them (today's behaviour of
#: ``InputScaled.stretch`` / ``Periodic.stretch``, where mlkernels hands the stretch to the kernel behind the map)
_STRETCH_FOLDS_THROUGH = (_ScaleMap, _PeriodMap, _SelectMap, _StretchMap)


def _folds_stretch(imap):
    return imap is None or all(isinstance(m, _STRETCH_FOLDS_THROUGH) for m in (imap.maps if isinstance(imap, _ChainMap) else (imap,)))


class _Mapped(Kernel):
    """``k0(imap_x(x), imap_y(y))`` for a sum of primitives ``k0`` (or anything whose ``pairwise`` takes mapped inputs).  One map: both
    arguments see it.  With two DIFFERENT maps the kernel is a cross-kernel: ``k(x)`` is the full block ``k0(imap_x(x), imap_y(x))``,
    not symmetric -- ``lower`` and the diagonal additions are refused, as the one-sided blocks of ``gpk_kmat_diff`` refuse them."""

    def __init__(self, k, imap, imap_y=_UNSET):
        self.k, self.imap_x, self.imap_y = k, imap, (imap if imap_y is _UNSET else imap_y)
        self.stationary = bool(k.stationary and self.symmetric and (imap is None or imap.keeps_stationary))

    @property
    def symmetric(self):
        return _same_map(self.imap_x, self.imap_y)

    def _mapped(self, x, imap):
        x = uprank(x)
        if isinstance(x, MultiInput):
            raise ValueError(f"{type(self).__name__} is a single-output kernel; it cannot take multi-process inputs")
        # (values only: the differentiable log-density / bound take the kernel apart through `input_scaled_view`
        # and map the inputs themselves; everything that is not covered there refuses loudly at its own entry)
        return x.detach() if imap is None else imap.values(x)

    def input_scaled_view(self):
        return (self.k, self.imap_x, self.imap_y)

    def num_outputs(self, x):
        return self.k.num_outputs(x)

    def pairwise(self, x, y=None, **kw):
        if self.symmetric:
            return self.k.pairwise(self._mapped(x, self.imap_x), None if y is None else self._mapped(y, self.imap_x), **kw)
        if y is None:
            if kw.get("lower") or kw.get("diag_add") or kw.get("diag_vec") is not None:
                raise ValueError("a kernel behind two different input maps is not symmetric: k(x) is the full block, without `lower` "
                                 "and without additions to the diagonal")
            kw = {key: val for key, val in kw.items() if key not in ("lower", "diag_add", "diag_vec")}
            y = x
        return self.k.pairwise(self._mapped(x, self.imap_x), self._mapped(y, self.imap_y), **kw)

    def elwise(self, x, y=None, **kw):
        if y is not None and y is not x:
            raise NotImplementedError("elwise is implemented for identical inputs")
        if not self.symmetric:
            raise NotImplementedError("elwise is implemented for identical inputs behind the same map in both arguments")
        return self.k.elwise(self._mapped(x, self.imap_x), **kw)

    def __reversed__(self):
        # k(m(x), m(y)) of a symmetric k is symmetric; behind two maps the maps change places
        return self if self.symmetric else _Mapped(self.k, self.imap_y, self.imap_x)

    def __repr__(self):
        return f"({self.k!r} behind {type(self.imap_x).__name__}, {type(self.imap_y).__name__})"


class InputScaled(_Mapped):
    """``k.stretch(l)`` with one length scale per input dimension (mlkernels' ``Stretched`` with a vector:
    ``k(x / l, y / l)``).  The inputs are divided once -- O(N D) -- and the inner kernel (a sum of primitives) runs
    its fused kernel-matrix launch on them, lower-triangle-only / in-place-factorisable like any other; sums of
    kernels with DIFFERENT per-dimension scales are evaluated term group by term group (``Sum.pairwise``)."""

    def __init__(self, k, scales):
        if k.terms() is None:
            raise NotImplementedError("stretch is implemented for sums of primitive kernels")
        # (a tensor is kept AS IT IS -- the caller's object: in-place updates and autograd leaves must stay visible; under a
        # `torch.set_default_device(...)` mode `torch.as_tensor(tensor)` would silently copy it to that device)
        if not torch.is_tensor(scales):
            scales = torch.as_tensor(scales)
        if scales.dim() != 1:
            raise ValueError("per-dimension length scales are a vector (one entry per input dimension)")
        if not bool((scales > 0).all()):
            raise ValueError("length scales must be positive")
        self.k, self.scales = k, scales
        self.imap_x = self.imap_y = _ScaleMap(scales)
        self.stationary = k.stationary

    def stretch(self, scale, scale_y=_UNSET):
        if scale_y is not _UNSET:
            return Kernel.stretch(self, scale, scale_y)
        if _is_vector_scale(scale):
            return InputScaled(self.k, self.scales * (scale if torch.is_tensor(scale) else torch.as_tensor(scale)).to(self.scales))
        if _is_per_batch(scale):
            raise NotImplementedError(f"a stretch by {PER_BATCH} of a kernel behind per-dimension length scales is not implemented: "
                                      "stretch the kernel first, then by the vector (`k.stretch(l).stretch(vector)`)")
        return InputScaled(self.k, self.scales * _as_float(scale))

    def __repr__(self):
        return f"({self.k!r} > {self.scales.tolist()})"


class Periodic(_Mapped):
    """``k.periodic(p)`` (mlkernels' ``Periodic``): ``k`` evaluated on ``(sin(2 pi x / p), cos(2 pi x / p))`` -- for ``EQ`` that is
    ``exp(-2 sum_d sin^2(pi (x_d - y_d) / p_d))``.  ``p``: a positive scalar or one period per input dimension, a number or a tensor
    (kept as given: a learnable period).  The inputs are mapped once -- O(N D), twice the dimension behind the map -- and the inner
    kernel, a sum of primitives, runs its fused kernel-matrix launch on them, exactly as ``InputScaled`` does behind its division."""

    def __init__(self, k, period):
        if k.terms() is None:
            raise NotImplementedError("periodic is implemented for sums of primitive kernels")
        if torch.is_tensor(period):
            if period.dim() > 1:
                raise ValueError("a period is a scalar or a vector (one entry per input dimension)")
            ok = bool((period.detach() > 0).all())
        else:
            period = tuple(float(v) for v in period) if isinstance(period, (list, tuple)) or np.ndim(period) > 0 else float(period)
            ok = bool(np.all(np.asarray(period) > 0))
        if not ok:
            raise ValueError("periods must be positive")
        self.k, self.period = k, period
        self.imap_x = self.imap_y = _PeriodMap(period)
        self.stationary = k.stationary

    def stretch(self, scale, scale_y=_UNSET):
        if scale_y is not _UNSET:
            return Kernel.stretch(self, scale, scale_y)
        return Periodic(self.k.stretch(scale), self.period)      # (mlkernels: the stretch goes to the kernel behind the map)

    def __repr__(self):
        return f"({self.k!r} per {self.period})"


def _same_param(a, b):
    return (a is b) if (torch.is_tensor(a) or torch.is_tensor(b)) else (a == b)


def has_per_batch(kernel, _depth=0):
    """Does any hyper-parameter reachable from ``kernel`` come once per batch entry (a ``(B, 1, 1)`` tensor)?  What the paths that
    do not admit such parameters ask before they refuse."""
    if _depth > 16 or not isinstance(kernel, Kernel):
        return False
    rows = kernel.tensor_table()
    if rows is not None:
        return any(_is_per_batch(p) for row in rows for p in row[1:])
    if isinstance(kernel, MultiOutputKernel):
        return any(has_per_batch(kernel.kernels[p], _depth + 1) for p in kernel.pids)
    for val in vars(kernel).values():
        if _is_per_batch(val) or (isinstance(val, InputMap) and _is_per_batch(val.param)):
            return True
        if isinstance(val, Kernel) and has_per_batch(val, _depth + 1):
            return True
    return False


def _merge(rows):
    """Add up the variances of rows with the same primitive, the same length scale and the same shape parameter (``p + p``
    has the kernel ``4 k``, not four terms; the fused kernels take at most 8 distinct terms)."""
    out = []
    for kind, var, scale, shp in rows:
        for i, (k2, v2, s2, a2) in enumerate(out):
            if k2 == kind and _same_param(scale, s2) and _same_param(shp, a2):
                _same_batch(v2, var)
                out[i] = (k2, v2 + var, s2, a2)
                break
        else:
            out.append((kind, var, scale, shp))
    return out


def _scale_stamp(t):
    """Identity + version of the parameter of an input map -- a length-scale vector, a period (``None``: no map, a constant stamp;
    a tensor nothing vouches for: ``None``)."""
    if t is None:
        return (0, 0)
    if isinstance(t, InputMap):
        return t.stamp()
    if not torch.is_tensor(t) or t.is_inference() or not t.is_cuda:
        return None
    return (id(t), t._version)


def _same_map(a, b):
    return (a is b) or (a is not None and b is not None and a.same(b))


def _map_groups(k):
    """A kernel as groups of terms that see the same inputs: ``[(k_g, imap_x, imap_y)]`` with ``k(x, y) = sum_g k_g(imap_x(x),
    imap_y(y))``, every ``k_g`` a sum of primitives; None when the kernel has no such form.  One group: ``input_scaled_view()``.  Two
    summands share a group only when they agree on BOTH maps."""
    v = k.input_scaled_view()
    if v is not None:
        return [v]
    if isinstance(k, Sum):
        ga, gb = _map_groups(k.a), _map_groups(k.b)
        if ga is None or gb is None:
            return None
        out = list(ga)
        for kern, mx, my in gb:
            for i, (k2, mx2, my2) in enumerate(out):
                if _same_map(mx, mx2) and _same_map(my, my2):
                    out[i] = (Sum(k2, kern), mx2, my2)
                    break
            else:
                out.append((kern, mx, my))
        return out
    if isinstance(k, Scaled):
        g = _map_groups(k.k)
        return None if g is None else [(Scaled(kern, k.v), mx, my) for kern, mx, my in g]
    return None


def _symmetric_groups(k):
    """``_map_groups(k)`` if every group sees both arguments through the same map (a kernel matrix ``k(x)`` is then symmetric: built
    lower-only, factorised in place), else None."""
    groups = _map_groups(k)
    if groups is None or not all(_same_map(mx, my) for _, mx, my in groups):
        return None
    return groups


class Sum(Kernel):
    def __init__(self, a, b):
        self.a, self.b = a, b
        self.stationary = a.stationary and b.stationary
        self._view = _UNSET
        self._view_stamp = None

    def num_outputs(self, x):
        return self.a.num_outputs(x)

    def _table(self, conv):
        ra, rb = self.a._table(conv), self.b._table(conv)
        return None if ra is None or rb is None else _merge(ra + rb)

    def input_scaled_view(self):
        # asked several times per FDD / log-density: the comparison of the two length-scale vectors (a device-to-host
        # synchronisation when they live on the GPU) is made once per kernel object
        # -- and again whenever one of them has been written in place since (the answer of `torch.equal` must not outlive
        # the values it compared; tensors without a version counter are compared every time)
        va, vb = self.a.input_scaled_view(), self.b.input_scaled_view()
        stamp = tuple(_scale_stamp(m) for v in (va, vb) if v is not None for m in v[1:])
        if self._view is _UNSET or None in stamp or stamp != self._view_stamp:
            self._view = self._input_scaled_view()
            self._view_stamp = stamp
        return self._view

    def _input_scaled_view(self):
        va, vb = self.a.input_scaled_view(), self.b.input_scaled_view()
        if va is None or vb is None:
            return None
        # different maps (length-scale vectors, periods, shifts, ...) in either argument: no common one
        return (Sum(va[0], vb[0]), va[1], va[2]) if (_same_map(va[1], vb[1]) and _same_map(va[2], vb[2])) else None

    def pairwise(self, x, y=None, **kw):
        if self.terms() is not None:
            return super().pairwise(x, y, **kw)
        view = self.input_scaled_view()
        if view is not None:                       # both summands see the inputs through the same map
            return _Mapped(*view).pairwise(x, y, **kw)
        groups = _map_groups(self)
        if groups is not None:
            # terms behind DIFFERENT input maps (per-dimension length scales, periods, none): group by group into ONE buffer -- the
            # first fused launch writes it (with the diagonal), the others add to it; `lower` / `out` keep their meaning
            kw.pop("cache", None)
            out, da, dv = kw.pop("out", None), kw.pop("diag_add", 0.0), kw.pop("diag_vec", None)
            first = not kw.pop("accumulate", False)
            xr = uprank(x)
            yr = None if y is None else uprank(y)
            for group in groups:
                g = _Mapped(*group)
                out = g.pairwise(xr, yr, out=out, accumulate=not first, diag_add=da if first else 0.0, diag_vec=dv if first else None, **kw)
                first = False
            return out
        groups = _scaled_groups(self)
        if groups is not None:
            # some groups between two functions, fn_x(x) k_g(x, y) fn_y(y): the same walk, such a group as ONE scaled launch
            # (`kmat_scaled`) -- no N x M temporary for the scaled summand
            return _pairwise_groups(groups, x, y, kw)
        da, dv = kw.pop("diag_add", 0.0), kw.pop("diag_vec", None)
        kw.pop("lower", None)
        out = self.a.pairwise(x, y, **kw) + self.b.pairwise(x, y, **kw)
        return _add_diag(out, da, dv) if y is None else out

    def elwise(self, x, y=None, **kw):
        if self.terms() is not None:
            return super().elwise(x, y, **kw)
        view = self.input_scaled_view()
        if view is not None:
            return _Mapped(*view).elwise(x, y, **kw)
        if y is None:
            from . import learnable                                       # (a pseudo-point posterior under learnable quantities)
            got = learnable.marginals(None, self, uprank(x), kw.get("cache"))
            if got is not None:
                return got[1]
        return self.a.elwise(x, y, **kw) + self.b.elwise(x, y, **kw)

    def __repr__(self):
        return f"{self.a!r} + {self.b!r}"


class Reversed(Kernel):
    """``reversed(k)(x, y) = k(y, x)^T`` (used for cross-kernels, measure.py:111)."""

    def __init__(self, k):
        self.k = k
        self.stationary = k.stationary

    def num_outputs(self, x):
        return self.k.num_outputs(x)

    def _table(self, conv):
        return self.k._table(conv)   # sums of primitives are symmetric

    def pairwise(self, x, y=None, **kw):
        if self.terms() is not None or y is None:
            return self.k.pairwise(x, y, **kw)
        return self.k.pairwise(y, x, **kw).transpose(-1, -2)

    def elwise(self, x, y=None, **kw):
        return self.k.elwise(x, y, **kw)


# ---------------------------------------------------------------------------
# input maps in the kernel algebra: shift, select, transform, the two-argument stretch (mlkernels' semantics)
# ---------------------------------------------------------------------------
class PosteriorOperationError(NotImplementedError):
    """A posterior mean / kernel was asked for an operation it has no form for.  ``GP`` catches exactly this when it registers a derived
    process in a posterior conditioned earlier, and ``post(p)`` there refuses with the reason."""


class PosteriorInputMapError(PosteriorOperationError):
    """A posterior mean / kernel was asked to shift, stretch, select or transform its inputs: map the prior process, condition then,
    and look the mapped process up under the posterior."""


def _is_number(v, value):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v == value


def _sum_of_groups(groups):
    """The kernel ``sum_g k_g(imap_x(x), imap_y(y))`` of groups as ``_map_groups`` lists them."""
    out = None
    for kern, mx, my in groups:
        g = kern if (mx is None and my is None) else _Mapped(kern, mx, my)
        out = g if out is None else out + g
    return out


def _behind(k, mx, my):
    """``k(mx(x), my(y))`` as a kernel (a map that is None: that argument as it is).  The new maps act FIRST on the inputs, whatever
    maps ``k`` sits behind already come after them.  Refuses, loudly, what has no form as groups of primitives behind maps."""
    if mx is None and my is None or isinstance(k, ZeroKernel):
        return k
    groups = _map_groups(k)
    if groups is not None:
        both = mx is my
        out = []
        for kern, gx, gy in groups:
            cx = _chain(mx, gx)
            out.append((kern, cx, cx if (both and gx is gy) else _chain(my, gy)))
        return _sum_of_groups(out)
    if isinstance(k, Sum):
        return _behind(k.a, mx, my) + _behind(k.b, mx, my)
    if isinstance(k, Scaled):
        return Scaled(_behind(k.k, mx, my), k.v)
    if isinstance(k, Reversed):
        return reversed(_behind(k.k, my, mx))
    if isinstance(k, (PosteriorKernel, SubspaceKernel)):
        raise PosteriorInputMapError("input maps (shift / stretch / select / transform) of posterior kernels are not implemented: map the "
                                     "prior process, condition then, and look the mapped process up under the posterior")
    raise NotImplementedError(f"input maps (shift / select / transform / the two-argument stretch) are not implemented for "
                              f"{type(k).__name__}: it is no sum of primitive kernels behind input maps")


def _stretch_arguments(k, sx, sy):
    """``k(x / sx, y / sy)`` for scalars: the inputs themselves are divided, whatever maps ``k`` sits behind.  The same stretch in both
    arguments is folded into a group's term table where that is the same function (no map, a selection, per-dimension scales, another
    stretch -- NOT the periodic embedding); everything else becomes a stretch map at the head of each argument's chain."""
    same = sx is sy or (not torch.is_tensor(sx) and not torch.is_tensor(sy) and float(sx) == float(sy))
    groups = _map_groups(k) if same and not _is_number(sx, 1) else None
    if groups is None:
        return _behind(k, *(None if _is_number(s, 1) else _StretchMap(s) for s in (sx, sy)))

    def divides_inputs(imap):
        return _folds_stretch(imap) and not any(isinstance(m, _PeriodMap) for m in (getattr(imap, "maps", None) or (imap,)))

    out, m = [], _StretchMap(sx)
    for kern, gx, gy in groups:
        if divides_inputs(gx) and divides_inputs(gy):
            out.append((kern.stretch(_as_param(sx)), gx, gy))
        else:
            cx = _chain(m, gx)
            out.append((kern, cx, cx if gx is gy else _chain(m, gy)))
    return _sum_of_groups(out)


def _stretch_groups(k, s):
    """``k.stretch(s)`` with a scalar ``s`` for a kernel that is groups of primitives behind maps: the stretch is folded into the
    group's term table where it commutes with the maps (a selection, per-dimension scales, the periodic embedding), and becomes a map
    of its own, applied first, in front of a shift or a feature map (``k.shift(c).stretch(s)`` is ``k(x / s - c, ...)``)."""
    out = []
    for kern, gx, gy in _map_groups(k):
        if _folds_stretch(gx) and _folds_stretch(gy):
            out.append((kern.stretch(s), gx, gy))
        else:
            m = _StretchMap(s)
            cx = _chain(m, gx)
            out.append((kern, cx, cx if gx is gy else _chain(m, gy)))
    return _sum_of_groups(out)


# ---------------------------------------------------------------------------
# a kernel between two functions: fn_x(x) k(x, y) fn_y(y), the kernel of a process times a function (stheno/model/measure.py:242-251)
# ---------------------------------------------------------------------------
FN_SCALED = "function-scaled"


class ScaleFn:
    """A function of the inputs that multiplies a process: ``fn`` takes the upranked inputs ``(..., N, D)`` and returns one value per
    point, ``(..., N)`` or ``(..., N, 1)``.  Any callable (an ``nn.Module`` included).  ``self(x)`` is a torch expression ``(..., N)`` in the
    inputs' dtype, ``values(x)`` the same numbers cut off from the graph (what the fused launch sees).  Two are the same only if they
    hold the same callable OBJECT; ``requires_grad`` follows :class:`_TransformMap`'s probe rule."""

    def __init__(self, fn):
        if not callable(fn):
            raise TypeError("a process is multiplied by a callable from (..., N, D) to (..., N)")
        self.fn = fn
        self._probe = None

    def __call__(self, x):
        p = self._probe
        if p is None or p.shape[-1] != x.shape[-1] or p.dtype != x.dtype or p.device != x.device:
            self._probe = x.detach()[(0,) * (x.dim() - 2)][:1].clone()
        out = self.fn(x)
        if torch.is_tensor(out) and out.dim() == x.dim() and out.shape[-1] == 1:
            out = out[..., 0]
        if not (torch.is_tensor(out) and tuple(out.shape) == tuple(x.shape[:-1])):
            raise ValueError(f"a function that multiplies a process maps inputs (..., N, D) to (..., N) or (..., N, 1); got "
                             f"{tuple(getattr(out, 'shape', ()))} for inputs {tuple(x.shape)}")
        return out.to(x.dtype)

    def values(self, x):
        with torch.no_grad():
            return self(x.detach())

    @property
    def requires_grad(self):
        if self._probe is None or self._probe.shape[-2] == 0:
            return True
        try:
            with torch.enable_grad():
                out = self.fn(self._probe)
        except Exception:        # (a probe row the function cannot take: unknown, and unknown counts as learnable)
            return True
        return bool(torch.is_tensor(out) and out.requires_grad)

    def same(self, other):
        return type(other) is type(self) and other.fn is self.fn

    def __repr__(self):
        return getattr(self.fn, "__name__", type(self.fn).__name__)


class _ProductFn(ScaleFn):
    """``a(x) b(x)``: what ``(k * fn1) * fn2`` puts on a side."""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.fn = self

    def __call__(self, x):
        return self.a(x) * self.b(x)

    @property
    def requires_grad(self):
        return self.a.requires_grad or self.b.requires_grad

    def same(self, other):
        return type(other) is type(self) and self.a.same(other.a) and self.b.same(other.b)

    def __repr__(self):
        return f"{self.a!r} * {self.b!r}"


def _same_fn(a, b):
    return (a is b) or (a is not None and b is not None and a.same(b))


def _fn_product(a, b):
    return b if a is None else a if b is None else _ProductFn(a, b)


def _fn_scaled(k, fx, fy):
    """``fx(x) k(x, y) fy(y)`` as a kernel (``None``: that side as it is).  Zero stays zero, the functions of a kernel that sits
    between two already are multiplied, a numeric factor stays outside, and a sum that is no sum of groups is scaled summand by summand."""
    if (fx is None and fy is None) or isinstance(k, ZeroKernel):
        return k
    if isinstance(k, FnScaled):
        px = _fn_product(k.fx, fx)
        return FnScaled(k.k, px, px if (k.fx is k.fy and fx is fy) else _fn_product(k.fy, fy))
    if isinstance(k, Sum) and _map_groups(k) is None:
        return _fn_scaled(k.a, fx, fy) + _fn_scaled(k.b, fx, fy)
    return FnScaled(k, fx, fy)


def _contains_fn_scaled(k, _depth=0):
    """Does a function-scaled kernel sit anywhere in ``k``?"""
    if isinstance(k, FnScaled):
        return True
    return any(True for _ in _fn_scaled_nodes(k, _depth))


def _fn_scaled_nodes(k, _depth=0):
    """Every function-scaled kernel reachable from ``k`` (through sums, factors, posterior kernels, the blocks of several processes)."""
    if isinstance(k, FnScaled):
        yield k
    if _depth > 16 or not isinstance(k, Kernel):
        return
    if isinstance(k, MultiOutputKernel):
        for p in k.pids:
            yield from _fn_scaled_nodes(k.kernels[p], _depth + 1)
        return
    for v in vars(k).values():
        if isinstance(v, Kernel):
            yield from _fn_scaled_nodes(v, _depth + 1)


def prime_scale_fns(k, x):
    """Give every function behind ``k`` that has not seen an input yet its probe row from ``x`` (a tensor, or a multi-process input whose
    first part serves): a guard that asks ``requires_grad`` before the first evaluation then gets the probe's answer, not "unknown"."""
    while isinstance(x, MultiInput):
        x = x.parts[0][1] if x.parts else None
    if not torch.is_tensor(x) or x.dim() < 2 or x.shape[-2] == 0:
        return
    def leaves(fn):
        if isinstance(fn, _ProductFn):
            yield from leaves(fn.a)
            yield from leaves(fn.b)
        elif fn is not None:
            yield fn

    row = None
    for node in _fn_scaled_nodes(k):
        for fn in (*leaves(node.fx), *leaves(node.fy)):
            if fn._probe is None:
                row = x.detach()[(0,) * (x.dim() - 2)][:1].clone() if row is None else row
                fn._probe = row


def _refuse_fn_scaled(k, what):
    if _contains_fn_scaled(k):
        raise NotImplementedError(f"{what} of a {FN_SCALED} kernel (the kernel of a process times a function) are not implemented: map "
                                  "or differentiate the process first, multiply then")


class FnScaled(Kernel):
    """``fn_x(x) k(x, y) fn_y(y)``: the kernel of a process times a function (both sides hold the same :class:`ScaleFn`) and its
    cross-kernels with other processes (one side is ``None``).  Built by ``k * fn``.

    Where ``k`` is a sum of groups of primitives behind input maps, every group is ONE launch of ``kmat_scaled`` -- the two factors are
    applied where the tile is stored, the diagonal additions stay unscaled -- written or accumulated into the caller's buffer like any
    other group: lower-triangle-only and factorisable in place where both sides hold the same function.  Over any other kernel (a
    posterior kernel) the inner kernel is evaluated and scaled in torch.  Values only, like every plain evaluation: the differentiable
    log-density takes the kernel apart through ``_scaled_groups`` and forms ``fn(x)`` in torch."""

    def __init__(self, k, fx, fy=_UNSET):
        self.k, self.fx, self.fy = k, fx, (fx if fy is _UNSET else fy)

    @property
    def symmetric(self):
        return _same_fn(self.fx, self.fy)

    def num_outputs(self, x):
        return self.k.num_outputs(x)

    def __mul__(self, other):
        if isinstance(other, Kernel) or (callable(other) and not torch.is_tensor(other)):
            return super().__mul__(other)
        inner = self.k * other                     # c * (k * fn): the factor goes into the group's variances
        return inner if isinstance(inner, ZeroKernel) else FnScaled(inner, self.fx, self.fy)

    __rmul__ = __mul__

    def pairwise(self, x, y=None, **kw):
        groups = _scaled_groups(self)
        if groups is not None:
            return _pairwise_groups(groups, x, y, kw)
        x = uprank(x)
        yr = x if y is None else uprank(y)
        if isinstance(x, MultiInput) or isinstance(yr, MultiInput):
            raise ValueError("FnScaled is a single-output kernel; it cannot take multi-process inputs")
        out, accumulate = kw.pop("out", None), kw.pop("accumulate", False)
        da, dv, lower = kw.pop("diag_add", 0.0), kw.pop("diag_vec", None), kw.pop("lower", False)
        if y is None and not self.symmetric:
            if lower or da or dv is not None:
                raise ValueError("a kernel between two different functions is not symmetric: k(x) is the full block, without `lower` and "
                                 "without additions to the diagonal")
            y = x
        res = self.k.pairwise(x, y, **kw)          # (any other inner kernel: evaluated, then scaled in torch)
        if self.fx is not None:
            res = res * self.fx.values(x)[..., :, None]
        if self.fy is not None:
            res = res * self.fy.values(yr)[..., None, :]
        if y is None:
            res = _add_diag(res if (self.fx is not None or self.fy is not None) else res.clone(), da, dv)
        if out is None:
            return res
        if accumulate:
            out += res
        else:
            out.copy_(res)
        return out

    def elwise(self, x, y=None, *, cache=None):
        if y is not None and y is not x:
            raise NotImplementedError("elwise is implemented for identical inputs")
        if not self.symmetric:
            raise NotImplementedError("elwise is implemented for the same function on both sides")
        x = uprank(x)
        s = self.fx.values(x)
        return (s * s)[..., None] * self.k.elwise(x, cache=cache)

    def __reversed__(self):
        inner = reversed(self.k)
        return self if (inner is self.k and self.fx is self.fy) else FnScaled(inner, self.fy, self.fx)

    def __repr__(self):
        return f"({self.fx!r} {self.k!r} {self.fy!r})"


def _scaled_groups(k):
    """``_map_groups`` with a function on either side of a group: ``[(k_g, imap_x, imap_y, fn_x, fn_y)]`` with ``k(x, y) = sum_g
    fn_x(x) k_g(imap_x(x), imap_y(y)) fn_y(y)``, every ``k_g`` a sum of primitives, a missing function ``None``; None when the kernel has
    no such form.  What ``_map_groups`` knows comes back as it lists it, between two ``None``."""
    groups = _map_groups(k)
    if groups is not None:
        return [(kern, mx, my, None, None) for kern, mx, my in groups]
    if isinstance(k, FnScaled):
        inner = _scaled_groups(k.k)
        if inner is None:
            return None
        out = []
        for kern, mx, my, gx, gy in inner:
            px = _fn_product(gx, k.fx)
            out.append((kern, mx, my, px, px if (gx is gy and k.fx is k.fy) else _fn_product(gy, k.fy)))
        return out
    if isinstance(k, Sum):
        ga, gb = _scaled_groups(k.a), _scaled_groups(k.b)
        return None if ga is None or gb is None else ga + gb
    if isinstance(k, Scaled):
        g = _scaled_groups(k.k)
        return None if g is None else [(Scaled(kern, k.v), mx, my, fx, fy) for kern, mx, my, fx, fy in g]
    return None


def _symmetric_scaled_groups(k):
    """``_scaled_groups(k)`` if every group sees both arguments through the same map and between the same function, else None."""
    groups = _scaled_groups(k)
    if groups is None or not all(_same_map(mx, my) and _same_fn(fx, fy) for _, mx, my, fx, fy in groups):
        return None
    return groups


def _pairwise_groups(groups, x, y, kw):
    """The groups of ``_scaled_groups`` into ONE buffer: the first launch writes it (with the diagonal), the others add to it; a plain
    group is a ``kmat`` launch, a group between functions a ``kmat_scaled`` launch.  ``lower`` / ``out`` / ``accumulate`` keep their meaning."""
    kw = dict(kw)
    kw.pop("cache", None)
    out, da, dv = kw.pop("out", None), kw.pop("diag_add", 0.0), kw.pop("diag_vec", None)
    first = not kw.pop("accumulate", False)
    xr = uprank(x)
    yr = None if y is None else uprank(y)
    if isinstance(xr, MultiInput) or isinstance(yr, MultiInput):
        raise ValueError("a sum of (function-scaled) groups is a single-output kernel; it cannot take multi-process inputs")
    for kern, mx, my, fx, fy in groups:
        args = dict(out=out, accumulate=not first, diag_add=da if first else 0.0, diag_vec=dv if first else None, **kw)
        if fx is None and fy is None:
            out = _Mapped(kern, mx, my).pairwise(xr, yr, **args)
        else:
            out = _scaled_launch(kern, mx, my, fx, fy, xr, yr, **args)
        first = False
    return out


def _scaled_launch(kern, mx, my, fx, fy, x, y, *, lower=False, diag_add=0.0, diag_vec=None, out=None, accumulate=False):
    """One group between functions as one ``kmat_scaled`` launch on the mapped inputs (values only)."""
    kt = kern._kterms()
    xm = x.detach() if mx is None else mx.values(x)
    sx = None if fx is None else fx.values(x)
    be = ops.get_backend()
    if y is None and _same_map(mx, my) and _same_fn(fx, fy):
        return be.kmat_scaled(kt, xm, None, sx, sx, lower=lower, diag_add=diag_add, diag_vec=diag_vec, out=out, accumulate=accumulate)
    if y is None:
        if lower or diag_add or diag_vec is not None:
            raise ValueError("a kernel between two different functions (or behind two different input maps) is not symmetric: k(x) is the "
                             "full block, without `lower` and without additions to the diagonal")
        y = x
    ym = y.detach() if my is None else my.values(y)
    sy = None if fy is None else fy.values(y)
    return be.kmat_scaled(kt, xm, ym, sx, sy, out=out, accumulate=accumulate)


# ---------------------------------------------------------------------------
# derivatives (mlkernels' DerivativeKernel behind GP.diff: stheno/model/measure.py:343-360)
# ---------------------------------------------------------------------------
#: kinds the fused derivative launch knows, with the value of ``-2 kappa'(0)``: what ``d^2 k / dx_a dy_a`` is at coincident points per unit
#: ``variance / scale^2`` (``include/gpk.h``, gpk_kmat_diff)
_DIFF_AT_ZERO = {"eq": 1.0, "rq": 1.0, "matern32": 3.0, "matern52": 5.0 / 3.0, "linear": 1.0, "const": 0.0}


class PosteriorDerivativeError(PosteriorOperationError):
    """A posterior mean / kernel was asked for its derivative: differentiate the prior process, then look the derivative up under the
    posterior (``post(f.diff())``)."""


def _as_dim(v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError(f"a derivative is taken with respect to an input dimension (a non-negative integer), got {v!r}")
    return int(v)


def _diff_kernel(k, a, b):
    """``d k / dx[a] dy[b]`` (``None``: that argument as it is) as a kernel; refuses, loudly, what the derivative launch does not cover."""
    if a is None and b is None:
        return k
    if isinstance(k, ZeroKernel):
        return ZeroKernel()
    if has_per_batch(k):
        raise NotImplementedError(f"derivative kernels are not implemented with {PER_BATCH}")
    if isinstance(k, DiffKernel):
        if (a is not None and k.dim_x is not None) or (b is not None and k.dim_y is not None):
            raise NotImplementedError("second derivatives in one argument (f.diff().diff()) are not implemented: they need the third and "
                                      "fourth derivatives of the kernels' profiles")
        return DiffKernel(k.k, k.dim_x if a is None else a, k.dim_y if b is None else b)
    view = k.input_scaled_view()
    if view is not None:
        kern, imap, imap_y = view
        if isinstance(imap, _PeriodMap):
            raise NotImplementedError("derivatives of kernels behind a periodic map are not implemented")
        for m in (imap, imap_y):
            if m is not None and not isinstance(m, _ScaleMap):
                raise NotImplementedError(f"derivatives behind the input map {type(m).__name__} are not implemented")
        if not _same_map(imap, imap_y):
            raise NotImplementedError("derivatives behind two different input maps are not implemented")
        bad = sorted({kind for kind, _, _ in kern.terms() if kind not in _DIFF_AT_ZERO})
        if bad:
            raise NotImplementedError(f"kernels of the kind {', '.join(bad)} are not differentiable (Matern12 has a kink at distance 0, "
                                      "Delta is piecewise constant)")
        return DiffKernel(k, a, b)
    if isinstance(k, Sum):
        if _map_groups(k) is not None:
            raise NotImplementedError("derivatives of sums whose parts sit behind different input maps are not implemented")
        return _diff_kernel(k.a, a, b) + _diff_kernel(k.b, a, b)
    if isinstance(k, Scaled):
        return k.v * _diff_kernel(k.k, a, b)
    if isinstance(k, Reversed):
        return reversed(_diff_kernel(k.k, b, a))
    if isinstance(k, (PosteriorKernel, SubspaceKernel)):
        raise PosteriorDerivativeError("derivatives of posterior kernels are not implemented: differentiate the prior process and look its "
                                       "derivative up under the posterior (`post(f.diff())`)")
    raise NotImplementedError(f"derivatives are not implemented for {type(k).__name__}")


class DiffKernel(Kernel):
    """``d k(x, y) / dx[dim_x] dy[dim_y]`` for a (symmetric) kernel ``k`` that is a sum of primitives, possibly behind per-dimension
    length scales; ``None`` in a slot: not differentiated in that argument.  ``DiffKernel(k, a, b)`` is the covariance of
    ``f.diff(a)`` with ``f.diff(b)``, ``DiffKernel(k, a, None)`` that of ``f.diff(a)`` with ``f``.  Built by ``Kernel.diff``.

    Every block is ONE fused launch (``gpk_kmat_diff``) written straight into the caller's view, lower-triangle-only and with the
    diagonal additions where the block is symmetric (``dim_x == dim_y``) -- it is assembled and factorised in place like a plain kernel
    matrix.  Behind per-dimension length scales the launch runs on the divided inputs and the chain-rule factors ``1 / l_a``, ``1 / l_b``
    ride in the variances.  ``terms()`` is None: this is no sum of primitives, nobody may add its "terms" to a plain launch."""

    def __init__(self, k, dim_x, dim_y):
        if dim_x is None and dim_y is None:
            raise ValueError("a derivative kernel differentiates at least one argument")
        self.k, self.dim_x, self.dim_y = k, dim_x, dim_y
        self.stationary = k.stationary

    def _parts(self, x):
        """``(kern, imap, fa, fb)``: the sum of primitives behind the map and the chain-rule factors of the two slots."""
        kern, imap, _ = self.k.input_scaled_view()          # (one map for both arguments: _diff_kernel admits nothing else)
        fa = fb = 1.0
        if imap is not None:
            scales = imap.param.detach().to(dtype=torch.float64, device="cpu")
            for dim in (self.dim_x, self.dim_y):
                if dim is not None and dim >= scales.numel():
                    raise ValueError(f"dimension {dim} outside the kernel's {scales.numel()} length scales")
            fa = 1.0 if self.dim_x is None else 1.0 / float(scales[self.dim_x])
            fb = 1.0 if self.dim_y is None else 1.0 / float(scales[self.dim_y])
        return kern, imap, fa, fb

    def _check_dims(self, x):
        d = x.shape[-1]
        for dim in (self.dim_x, self.dim_y):
            if dim is not None and dim >= d:
                raise ValueError(f"derivative with respect to dimension {dim} of inputs with {d} dimensions")

    def pairwise(self, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, cache=None, out=None, accumulate=False):
        x = uprank(x)
        sym = y is None
        y = None if sym else uprank(y)
        if isinstance(x, MultiInput) or isinstance(y, MultiInput):
            raise ValueError(f"{type(self).__name__} is a single-output kernel; it cannot take multi-process inputs")
        self._check_dims(x)
        kern, imap, fa, fb = self._parts(x)
        xm = x.detach() if imap is None else imap.values(x)
        ym = None if sym else (y.detach() if imap is None else imap.values(y))
        be, kt = ops.get_backend(), kern._kterms(fa * fb)
        if sym and self.dim_x == self.dim_y:       # symmetric: lower-triangle-only and the diagonal additions in the same pass
            return be.kmat_diff(kt, xm, None, self.dim_x, self.dim_y, lower=lower, diag_add=diag_add, diag_vec=diag_vec, out=out,
                                accumulate=accumulate)
        res = be.kmat_diff(kt, xm, xm if sym else ym, self.dim_x, self.dim_y, out=out, accumulate=accumulate)
        return _add_diag(res, diag_add, diag_vec) if sym else res

    def elwise(self, x, y=None, *, cache=None):
        """No launch: at coincident points a stationary term contributes ``v / scale^2`` times ``-2 kappa'(0)`` to ``d^2 / dx_a dy_a`` and
        nothing to any other derivative; a linear term ``v / scale^2`` times ``[a == b]``, ``x[a]`` or ``x[b]``."""
        if y is not None and y is not x:
            raise NotImplementedError("elwise is implemented for identical inputs")
        x = uprank(x)
        if isinstance(x, MultiInput):
            raise ValueError(f"{type(self).__name__} is a single-output kernel; it cannot take multi-process inputs")
        self._check_dims(x)
        kern, imap, fa, fb = self._parts(x)
        terms = kern.terms()
        shape = tuple(x.shape[:-1]) + (1,)
        if self.dim_x is not None and self.dim_y is not None:
            if self.dim_x != self.dim_y:
                return torch.zeros(shape, dtype=x.dtype, device=x.device)
            value = sum(var / scale ** 2 * _DIFF_AT_ZERO[kind] for kind, var, scale in terms) * fa * fb
            return torch.full(shape, value, dtype=x.dtype, device=x.device)
        lin = sum(var / scale ** 2 for kind, var, scale in terms if kind == "linear") * fa * fb
        if lin == 0.0:
            return torch.zeros(shape, dtype=x.dtype, device=x.device)
        dim = self.dim_x if self.dim_y is None else self.dim_y
        xm = x.detach() if imap is None else imap.values(x)
        return lin * xm[..., dim:dim + 1]

    def __reversed__(self):
        return DiffKernel(self.k, self.dim_y, self.dim_x)       # (k itself is symmetric: _diff_kernel admits nothing else)

    def __repr__(self):
        dims = f"{self.dim_x}" if self.dim_x == self.dim_y else f"{self.dim_x}, {self.dim_y}"
        return f"d({dims}) {self.k!r}"


# ---------------------------------------------------------------------------
# Cartesian products of processes (stheno/mo/kernel.py, stheno/mo/mean.py, measure.py:404-423)
# ---------------------------------------------------------------------------
def _eval_into(k, x, y, view, lower=False):
    """Write ``k(x, y)`` (``y is None``: symmetric) into the matrix view ``view``: a sum of primitives, a derivative of one
    (``DiffKernel``), or groups of primitives behind input maps go straight into the block (one fused launch per group, no temporary)."""
    if isinstance(k, ZeroKernel):
        view.zero_()
    elif (k.terms() is not None or isinstance(k, DiffKernel)) and not isinstance(y, MultiInput):
        k.pairwise(x, y, lower=lower, out=view)
    elif isinstance(k, Kernel) and _map_groups(k) is not None and not isinstance(x, MultiInput) and not isinstance(y, MultiInput):
        # (`lower` only where the block is symmetric: a cross-kernel behind two maps writes its full block)
        got = k.pairwise(x, y, out=view, **({"lower": True} if lower else {}))
        if got.data_ptr() != view.data_ptr():          # (a kernel that handed back a tensor of its own: the copy it always paid)
            view.copy_(got)
    else:
        view.copy_(k.pairwise(x, y))


class MultiOutputKernel(Kernel):
    """Kernel of the Cartesian product of the processes ``ps`` of a measure: block ``(i, j)``
    of ``k(X, Y)`` is ``measure.kernels[p_i, p_j](x_i, y_j)`` (``stheno/mo/kernel.py:39-76``,
    ``stheno/mo/input.py:7-9``).  A plain input stands for "every process at these inputs".
    The block matrix is assembled in ONE buffer (each block is written in place through its
    leading dimension); in the symmetric ``lower`` mode the blocks above the diagonal are skipped,
    so the buffer can be Cholesky-factorised in place like a single-process kernel matrix.

    The measure is referenced weakly and the processes by id (the kernel lives in the measure's
    own store); a ``MultiInput`` keeps its processes alive."""

    def __init__(self, measure, ps):
        import weakref

        self._measure = weakref.ref(measure)
        self.pids = tuple(id(p) for p in ps)

    @property
    def kernels(self):
        return self._measure().kernels

    def _split(self, x):
        if hasattr(x, "p") and hasattr(x, "_xr"):          # an FDD: that process at those inputs
            xr = x._xr
            return [(id(q), xi) for q, xi in xr.parts] if isinstance(xr, MultiInput) else [(id(x.p), xr)]
        if isinstance(x, (tuple, list)):                   # several FDDs (mo/input.py:7-9)
            return [part for e in x for part in self._split(e)]
        x = uprank(x)
        if isinstance(x, MultiInput):
            return [(id(p), xi) for p, xi in x.parts]
        return [(pid, x) for pid in self.pids]

    def num_outputs(self, x):
        kernels = self.kernels
        return sum(kernels[pi].num_outputs(xi) for pi, xi in self._split(x))

    def pairwise(self, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, cache=None, out=None):
        kernels = self.kernels
        if has_per_batch(self):
            raise NotImplementedError(f"several processes observed or predicted jointly (a `MultiInput`) are not implemented with {PER_BATCH}")
        sym = y is None
        X = self._split(x)
        Y = X if sym else self._split(y)
        # a part's process may itself be a product process (then its plain input expands): sizes come
        # from the processes' own kernels (the reference marks such kernels "ADK": stheno/mo/adk.py)
        sx = [kernels[pi].num_outputs(xi) for pi, xi in X]
        sy = sx if sym else [kernels[pj].num_outputs(yj) for pj, yj in Y]
        nx, ny = sum(sx), sum(sy)
        if out is None:
            out = ops.alloc_matrix(tuple(X[0][1].shape[:-2]), nx, ny, X[0][1].dtype, X[0][1].device)
        r0 = 0
        for i, (pi, xi) in enumerate(X):
            r1, c0 = r0 + sx[i], 0
            for j, (pj, yj) in enumerate(Y):
                c1 = c0 + sy[j]
                if not (sym and lower and j > i) and r1 > r0 and c1 > c0:
                    if sym and i == j:
                        _eval_into(kernels[pi], xi, None, out[..., r0:r1, c0:c1], lower=lower)
                    else:
                        _eval_into(kernels[pi, pj], xi, yj, out[..., r0:r1, c0:c1])
                c0 = c1
            r0 = r1
        return _add_diag(out, diag_add, diag_vec) if sym else out

    def elwise(self, x, y=None, *, cache=None):
        if y is not None and y is not x:
            raise NotImplementedError("elwise is implemented for identical inputs")
        kernels = self.kernels
        if has_per_batch(self):
            raise NotImplementedError(f"several processes observed or predicted jointly (a `MultiInput`) are not implemented with {PER_BATCH}")
        return torch.cat([kernels[pi].elwise(xi) for pi, xi in self._split(x)], dim=-2)

    def __repr__(self):
        return "MultiOutputKernel(" + ", ".join(repr(self.kernels[pid]) for pid in self.pids) + ")"


class _CrossKernel(Kernel):
    """``k(p_cross, p_j)``: rows follow the multi-input of the product process, columns the
    inputs of process ``j`` (the left rule of ``Measure.cross``, ``measure.py:419-422``)."""

    def __init__(self, mok, j):
        self.mok, self.j = mok, j

    def num_outputs(self, x):
        return self.mok.num_outputs(x)

    def pairwise(self, x, y=None, *, cache=None, **kw):
        if y is None:
            raise ValueError("a cross-kernel between a product process and another process needs both inputs")
        kernels = self.mok.kernels
        X = self.mok._split(x)
        y = uprank(y)
        sx = [kernels[pi].num_outputs(xi) for pi, xi in X]
        nx, ny = sum(sx), kernels[self.j].num_outputs(y)
        out = ops.alloc_matrix(tuple(X[0][1].shape[:-2]), nx, ny, X[0][1].dtype, X[0][1].device)
        r0 = 0
        for (pi, xi), n_i in zip(X, sx):
            r1 = r0 + n_i
            if r1 > r0 and ny > 0:
                _eval_into(kernels[pi, self.j], xi, y, out[..., r0:r1, :])
            r0 = r1
        return out

    def elwise(self, x, y=None, **kw):
        raise ValueError('Unclear combination of arguments given to "elwise".')    # mo/kernel.py:63-70


def _add_diag(out, diag_add, diag_vec):
    if diag_add or diag_vec is not None:
        ops.get_backend().add_diag_(out, diag_add, diag_vec)
    return out


# ---------------------------------------------------------------------------
# means
# ---------------------------------------------------------------------------
class Mean:
    def __call__(self, x, cache=None):
        raise NotImplementedError

    def __add__(self, other):
        if isinstance(other, (int, float)) and other == 0:
            return self
        return SumMean(self, other if isinstance(other, Mean) else _wrap_mean(other))

    __radd__ = __add__

    def __mul__(self, other):
        if callable(other) and not torch.is_tensor(other) and not isinstance(other, Mean):
            # m * fn: the mean of f * fn, evaluated in torch inside the graph; zero stays zero
            return self if isinstance(self, ZeroMean) else ProductMean(self, other if isinstance(other, ScaleFn) else ScaleFn(other))
        if _is_per_batch(other):
            raise NotImplementedError(f"means scaled by {PER_BATCH} are not implemented")
        return ScaledMean(self, _as_float(other))

    __rmul__ = __mul__

    def diff(self, dim=0):
        """``dm / dx[dim]`` as a mean (the mean of ``f.diff(dim)``, ``measure.py:357``)."""
        raise NotImplementedError(f"derivatives are not implemented for {type(self).__name__}")

    # -- input maps: m(imap(x)), the mean of f.shift(c) / f.stretch(s) / f.select(dims) / f.transform(fn) -------------------------
    def shift(self, c):
        return self if _is_number(c, 0) else self._behind(_ShiftMap(c))

    def stretch(self, s):
        if _is_vector_scale(s):
            return self._behind(_ScaleMap(s if torch.is_tensor(s) else torch.as_tensor(s)))
        return self if _is_number(s, 1) else self._behind(_StretchMap(s))

    def select(self, dims):
        return self._behind(_SelectMap(dims))

    def transform(self, fn):
        return self._behind(_TransformMap(fn))

    def _behind(self, imap):
        """``x -> self(imap(x))`` as a mean; constants are their own, sums and scalings distribute."""
        return MappedMean(self, imap)


class ZeroMean(Mean):
    def __call__(self, x, cache=None):
        x = uprank(x)
        return torch.zeros(x.shape[:-1] + (1,), dtype=x.dtype, device=x.device)

    def diff(self, dim=0):
        return ZeroMean()

    def _behind(self, imap):
        return self

    def __repr__(self):
        return "0"


class OneMean(Mean):
    def __call__(self, x, cache=None):
        x = uprank(x)
        return torch.ones(x.shape[:-1] + (1,), dtype=x.dtype, device=x.device)

    def _behind(self, imap):
        return self

    def diff(self, dim=0):
        return ZeroMean()

    def __repr__(self):
        return "1"


class FunctionMean(Mean):
    """Mean given by a Python function of the (upranked) inputs, e.g. ``lambda x: x ** 2``."""

    def __init__(self, f):
        self.f = f

    def __call__(self, x, cache=None):
        return uprank(self.f(uprank(x)))

    def diff(self, dim=0):
        return DiffMean(self, _as_dim(dim))

    def __repr__(self):
        return getattr(self.f, "__name__", "f")


class DiffMean(Mean):
    """``dm / dx[dim]`` of a function mean, by ``torch.autograd.grad`` on a detached copy of the inputs (the reference differentiates
    the mean function by autodiff as well).  The function acts point by point: row ``i`` of ``m(x)`` depends on row ``i`` of ``x`` only.
    While the caller records a graph the derivative stays part of it (``create_graph``): a mean function with learnable parameters
    hands on a derivative that still depends on them, never a detached value."""

    def __init__(self, m, dim):
        self.m, self.dim = m, dim

    def __call__(self, x, cache=None):
        x = uprank(x)
        if self.dim >= x.shape[-1]:
            raise ValueError(f"derivative with respect to dimension {self.dim} of inputs with {x.shape[-1]} dimensions")
        recording = torch.is_grad_enabled()
        with torch.enable_grad():
            xg = x.detach().clone().requires_grad_(True)
            out = _call_mean(self.m, xg, None)
            if not (torch.is_tensor(out) and out.requires_grad):       # a mean that does not depend on its inputs
                return torch.zeros(x.shape[:-1] + (1,), dtype=x.dtype, device=x.device)
            (g,) = torch.autograd.grad(out.sum(), xg, create_graph=recording, allow_unused=True)
            if g is None:                                              # ... or on its parameters only
                return torch.zeros(x.shape[:-1] + (1,), dtype=x.dtype, device=x.device)
        return g[..., self.dim:self.dim + 1].contiguous()

    def diff(self, dim=0):
        raise NotImplementedError("second derivatives (f.diff().diff()) are not implemented")

    def _behind(self, imap):
        raise NotImplementedError("input maps (shift / stretch / select / transform) of a derivative mean are not implemented: map the "
                                  "process first, differentiate then")

    def __repr__(self):
        return f"d({self.dim}) {self.m!r}"


class ScaledMean(Mean):
    def __init__(self, m, v):
        self.m, self.v = m, v

    def __call__(self, x, cache=None):
        return self.v * self.m(x, cache)

    def diff(self, dim=0):
        return ScaledMean(self.m.diff(dim), self.v)

    def _behind(self, imap):
        return ScaledMean(self.m._behind(imap), self.v)

    def __repr__(self):
        return f"{self.v} * {self.m!r}"


class SumMean(Mean):
    def __init__(self, a, b):
        self.a, self.b = a, b

    def __call__(self, x, cache=None):
        return self.a(x, cache) + self.b(x, cache)

    def diff(self, dim=0):
        return self.a.diff(dim) + self.b.diff(dim)

    def _behind(self, imap):
        return self.a._behind(imap) + self.b._behind(imap)

    def __repr__(self):
        return f"{self.a!r} + {self.b!r}"


class ProductMean(Mean):
    """``fn(x) m(x)``: the mean of the process ``f * fn`` (``measure.py:242-251``).  A torch expression: the parameters behind ``fn`` and
    behind ``m`` get their gradient through it."""

    def __init__(self, m, fn):
        self.m, self.fn = m, fn

    def __call__(self, x, cache=None):
        x = uprank(x)
        if isinstance(x, MultiInput):
            raise ValueError("the mean of a process times a function is the mean of one process; it cannot take multi-process inputs")
        return _call_mean(self.m, x, cache) * self.fn(x)[..., None]

    def diff(self, dim=0):
        raise NotImplementedError("derivatives of a function-scaled mean (the mean of f * fn) are not implemented")

    def _behind(self, imap):
        raise NotImplementedError("input maps (shift / stretch / select / transform) of a function-scaled mean (the mean of f * fn) are not "
                                  "implemented: map the process first, multiply then")

    def __repr__(self):
        return f"({self.m!r} * {self.fn!r})"


class MappedMean(Mean):
    """``m(imap(x))``: a mean behind a map of its inputs (:class:`InputMap`).  The map is a torch expression: a learnable shift or the
    parameters of a feature map get their gradient through the mean as through the kernel.  A map applied later acts first."""

    def __init__(self, m, imap):
        self.m, self.imap = m, imap

    def __call__(self, x, cache=None):
        x = uprank(x)
        if isinstance(x, MultiInput):
            raise ValueError("a mean behind an input map is the mean of one process; it cannot take multi-process inputs")
        return _call_mean(self.m, self.imap(x), None)

    def _behind(self, imap):
        return MappedMean(self.m, _chain(imap, self.imap))

    def diff(self, dim=0):
        raise NotImplementedError(f"derivatives behind the input map {type(self.imap).__name__} are not implemented")

    def __repr__(self):
        return f"({self.m!r} behind {type(self.imap).__name__})"


def _wrap_mean(m):
    if isinstance(m, Mean):
        return m
    if callable(m):
        return FunctionMean(m)
    v = _as_float(m)
    if v == 0:
        return ZeroMean()
    return OneMean() if v == 1 else ScaledMean(OneMean(), v)


class MultiOutputMean(Mean):
    """Mean of the Cartesian product: the per-process means stacked (``stheno/mo/mean.py``)."""

    def __init__(self, measure, ps):
        import weakref

        self._measure = weakref.ref(measure)
        self.pids = tuple(id(p) for p in ps)

    def _behind(self, imap):
        raise NotImplementedError("input maps of the mean of a product process are not implemented: map the component processes")

    def __call__(self, x, cache=None):
        means = self._measure().means
        x = uprank(x)
        parts = [(id(p), xi) for p, xi in x.parts] if isinstance(x, MultiInput) else [(pid, x) for pid in self.pids]
        return torch.cat([_call_mean(means[pi], xi, cache) for pi, xi in parts], dim=-2)


# ---------------------------------------------------------------------------
# posterior objects
# ---------------------------------------------------------------------------
def _cross(cache, k, z, x):
    """Memoised ``k(z, x)`` tensor within one ``mean_var(_diag)`` evaluation: the
    reference evaluates the data/inducing cross-kernel once per prediction
    (pinned by ``tests/model/test_model.py:335-365``).  Entries are keyed by object identity and
    keep their key objects alive, so an id cannot be recycled while the cache lives."""
    if cache is None:
        return k.pairwise(z, x)
    key = ("kzx", id(k), id(z), id(x))
    if key not in cache:
        cache[key] = (k.pairwise(z, x), k, z, x)
    return cache[key][0]


def note_built_from(mat, kernel, x, noise):
    """``mat`` -- the materialised ``kernel(x) + noise`` of a BATCH under a sum of terms behind different input maps, which has no fused
    build with the noise on the diagonal -- with ``(kernel, x, noise)`` noted on it (``built_from``): the values are the ones it has
    always had; the differentiable path of the batched posterior marginals (``learnable._exact_marginals``) reads the note to know
    whose matrix it is.  Anything else is handed back untouched."""
    if torch.is_tensor(x) and x.dim() == 3 and isinstance(kernel, Kernel) and hasattr(mat, "chol") and _map_groups(kernel) is not None:
        mat.built_from = (kernel, x, noise)
    return mat


class WhitenedT:
    """``k(x, z) L^{-T}`` (ns, n): the TRANSPOSE of the whitened cross-covariance ``L^{-1} k(z, x)`` -- what the factorisation with
    rows under the matrix leaves behind (``KernelDense.chol_with_rows``).  The consumers below take either form."""

    def __init__(self, zt):
        self.zt = zt

    def plain(self):
        return self.zt.transpose(-1, -2).contiguous()


def _whiten(cache, K_z, k, z, x, own_cross=False, rhs=None):
    """``L^{-1} k(z, x)`` (memoised), ``L = chol(K_z)``.  ``own_cross``: nobody else will ask for ``k(z, x)`` itself (dense
    conditioning: ``K_z`` is the only matrix it is ever solved against) -- the cross matrix is then not kept and the blocked solve
    takes it as its workspace instead of a copy (N x N* elements: 268 MB and 0.1 ms at cfg2).
    ``rhs = (r, took)``: if THIS call is what factorises ``K_z`` (rows under the matrix), the residual ``r`` (n, 1) rides along as a
    right-hand side (``matrix.config.posterior_rows_rhs``) and ``took(w)`` is called with ``w = L^{-1} r``."""
    key = ("v", id(K_z), id(k), id(z), id(x))
    if cache is not None and key in cache:
        return cache[key][0]
    # Nothing factorised yet (conditioning, then prediction, no log-density in between): the cross-covariance rides in the
    # factorisation as rows under the kernel matrix and comes out whitened, transposed -- no separate many-column solve.
    # (a non-empty term list: the zero kernel -- the cross-kernel of a process independent of the observed one -- has `terms() == []`,
    #  nothing to whiten and no business in the factorisation)
    if (own_cross and hasattr(K_z, "can_factor_with_rows") and k.terms() and not isinstance(k, ZeroKernel) and x.dim() == 2 and z.dim() == 2 and not x.requires_grad
            and ("kzx", id(k), id(z), id(x)) not in (cache or {}) and z is getattr(K_z, "x", None) and K_z.can_factor_with_rows(x.shape[-2])):
        from .matrix import config as _mconfig
        if rhs is not None and _mconfig.posterior_rows_rhs:
            got = K_z.chol_with_rows(k, x, rhs=rhs[0])
            if len(got) == 3:
                rhs[1](got[2])
            zt = got[1]
        else:
            _, zt = K_z.chol_with_rows(k, x)
        v = WhitenedT(zt)
        if cache is not None:
            cache[key] = (v, K_z, k, z, x)
        return v
    if isinstance(k, ZeroKernel):         # an independent process: L^{-1} 0 = 0, nothing to solve
        v = k.pairwise(z, x)
        if cache is not None:
            cache[key] = (v, K_z, k, z, x)
        return v
    chol = K_z.chol()
    if own_cross and hasattr(chol, "solve_") and ("kzx", id(k), id(z), id(x)) not in (cache or {}):
        kzx = k.pairwise(z, x)
        same_batch = kzx.dim() == chol.l.dim() and tuple(kzx.shape[:-2]) == tuple(chol.l.shape[:-2])
        v = chol.solve_(kzx) if (same_batch and kzx.is_contiguous() and not kzx.requires_grad and kzx.shape[-2] == chol.n) else chol.solve(kzx)
    else:
        v = chol.solve(_cross(cache, k, z, x))
    if cache is not None:
        cache[key] = (v, K_z, k, z, x)
    return v


class PosteriorKernel(Kernel):
    """``k_ij(x, y) - k_zi(z, x)^T K_z^{-1} k_zj(z, y)`` (mlkernels.PosteriorKernel;
    constructed at ``observations.py:148-154,256-261``)."""

    def __init__(self, k_ij, k_zi, k_zj, z, K_z, own_cross=False, exact=False):
        self.k_ij, self.k_zi, self.k_zj, self.z, self.K_z = k_ij, k_zi, k_zj, z, K_z
        self.own_cross = own_cross       # see _whiten
        self.exact = exact               # exact conditioning on observations of the process itself (see learnable.marginals)
        self.sparse = None               # weak (obs, measure) of a pseudo-point conditioning (likewise)

    def num_outputs(self, x):
        return self.k_ij.num_outputs(x)

    def pairwise(self, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, cache=None):
        x = uprank(x)
        sym = y is None
        if sym and torch.is_grad_enabled():
            from . import learnable
            got = learnable.covariance(self, x, cache, lower=lower, diag_add=diag_add, diag_vec=diag_vec)      # (the joint covariance under learnable quantities)
            if got is not None:
                return got
        y = x if sym else uprank(y)
        out = self.k_ij.pairwise(x, None if sym else y, cache=cache) if _accepts_cache(self.k_ij) else \
            self.k_ij.pairwise(x, None if sym else y)
        vx = _whiten(cache, self.K_z, self.k_zi, self.z, x, self.own_cross)
        vy = vx if (sym and self.k_zi is self.k_zj) else _whiten(cache, self.K_z, self.k_zj, self.z, y, self.own_cross)
        # out -= vx^T vy   (operands stored (K, M) / (K, N): row index contiguous)
        if out.stride(-1) != 1 and out.shape[-1] > 1:
            out = out.contiguous()          # e.g. the transposed view a reversed cross-kernel hands back
        if isinstance(vx, WhitenedT) and isinstance(vy, WhitenedT):      # both transposed: the k-contiguous form of the same product
            ops.get_backend().gemm(vx.zt, vy.zt, a_kmajor=True, b_kmajor=True, alpha=-1.0, beta=1.0, out=out)
        else:
            vx, vy = (v.plain() if isinstance(v, WhitenedT) else v for v in (vx, vy))
            ops.get_backend().gemm(vx, vy, a_kmajor=False, b_kmajor=False, alpha=-1.0, beta=1.0, out=out)
        return _add_diag(out, diag_add, diag_vec) if sym else out

    def elwise(self, x, y=None, *, cache=None):
        from . import learnable
        x = uprank(x)
        got = learnable.marginals(None, self, x, cache)
        if got is not None:
            return got[1]
        out = self.k_ij.elwise(x)
        vx = _whiten(cache, self.K_z, self.k_zi, self.z, x, self.own_cross)
        if self.k_zi is self.k_zj:
            if isinstance(vx, WhitenedT):
                # (the posterior mean of the same evaluation has read these rows already and left their sums of squares: one pass)
                hit = cache.pop(("rowss", id(vx)), None) if cache is not None else None
                if hit is not None and hit[1] is vx:
                    ss = hit[0]
                else:
                    _, ss = ops.get_backend().rowreduce(vx.zt, want_dot=False, want_ss=True)
            else:
                _, ss = ops.get_backend().colreduce(vx, want_ss=True)
            return out - ss[..., None]
        vy = _whiten(cache, self.K_z, self.k_zj, self.z, x, self.own_cross)
        vx, vy = (v.plain() if isinstance(v, WhitenedT) else v for v in (vx, vy))
        return out - (vx * vy).sum(-2)[..., None]


class SubspaceKernel(Kernel):
    """``k_zi(z, x)^T A^{-1} k_zj(z, y)`` (mlkernels.SubspaceKernel; ``observations.py:262-267``)."""

    def __init__(self, k_zi, k_zj, z, A):
        self.k_zi, self.k_zj, self.z, self.A = k_zi, k_zj, z, A
        self.sparse = None               # see PosteriorKernel

    def pairwise(self, x, y=None, *, lower=False, diag_add=0.0, diag_vec=None, cache=None):
        x = uprank(x)
        sym = y is None
        y = x if sym else uprank(y)
        vx = _whiten(cache, self.A, self.k_zi, self.z, x)
        vy = vx if (sym and self.k_zi is self.k_zj) else _whiten(cache, self.A, self.k_zj, self.z, y)
        out = ops.get_backend().gemm(vx, vy, a_kmajor=False, b_kmajor=False)
        return _add_diag(out, diag_add, diag_vec) if sym else out

    def elwise(self, x, y=None, *, cache=None):
        x = uprank(x)
        vx = _whiten(cache, self.A, self.k_zi, self.z, x)
        if self.k_zi is self.k_zj:
            _, ss = ops.get_backend().colreduce(vx, want_ss=True)
            return ss[..., None]
        vy = _whiten(cache, self.A, self.k_zj, self.z, x)
        return (vx * vy).sum(-2)[..., None]


def _accepts_cache(k):
    return isinstance(k, (PosteriorKernel, SubspaceKernel, Sum, Scaled, Reversed))


class PosteriorMean(Mean):
    """``m_i(x) + k_zi(z, x)^T K_z^{-1} (y - m_z(z))`` (mlkernels.PosteriorMean;
    ``observations.py:161-168,270-277``), evaluated as ``(L^{-1} k_zx)^T (L^{-1} (y - m_z(z)))``."""

    def __init__(self, m_i, m_z, k_zi, z, K_z, y, own_cross=False, exact=False):
        self.m_i, self.m_z, self.k_zi, self.z, self.K_z, self.y = m_i, m_z, k_zi, z, K_z, y
        self.own_cross = own_cross       # see _whiten
        self.exact = exact               # see PosteriorKernel
        self.sparse = None               # see PosteriorKernel
        self._w = None
        self._r = None
        self._r_detached = False         # the residual was formed under torch.no_grad() (cut off from a learnable mean / y)

    def diff(self, dim=0):
        raise PosteriorDerivativeError("derivatives of posterior means are not implemented: differentiate the prior process and look its "
                                       "derivative up under the posterior (`post(f.diff())`)")

    def _behind(self, imap):
        raise PosteriorInputMapError("input maps (shift / stretch / select / transform) of posterior means are not implemented: map the "
                                     "prior process, condition then, and look the mapped process up under the posterior")

    def _residual(self):
        if self._r is None:
            y = uprank(self.y)
            # (a zero mean: the residual IS the data -- nobody below writes into it)
            self._r = (y, y if (isinstance(self.m_z, ZeroMean) and torch.is_tensor(y) and not y.requires_grad) else y - self.m_z(self.z))
            self._r_detached = not torch.is_grad_enabled()
        return self._r

    def _whitened_residual(self):
        if self._w is None:
            y, r = self._residual()
            chol = self.K_z.chol()
            if isinstance(self.m_z, ZeroMean) and hasattr(chol, "solve_residual"):
                self._w = chol.solve_residual(r, y)     # shared with the log-density of the same observations
            else:
                self._w = chol.solve(r)                 # (..., N, 1)
        return self._w

    def _took(self, w):
        """``w = L^{-1} (y - m_z(z))`` came out of the factorisation (a right-hand side under the matrix): kept here and, for a zero
        mean, filed with the factor under ``y`` -- the log-density of the same observations finds it (``Chol.solve_residual``)."""
        self._w = w
        if isinstance(self.m_z, ZeroMean):
            chol = self.K_z.chol()
            if hasattr(chol, "remember_residual"):
                chol.remember_residual(self._residual()[0], w)

    def __call__(self, x, cache=None):
        from . import learnable
        x = uprank(x)
        got = learnable.marginals(self, None, x, cache)
        if got is not None:
            return got[0]
        rhs = None
        if self._w is None and self.own_cross and hasattr(self.K_z, "can_factor_with_rows") and x.dim() == 2:
            y, r = self._residual()
            if r.dim() == 2 and r.shape[-1] == 1 and not r.requires_grad:
                rhs = (r, self._took)
        v = _whiten(cache, self.K_z, self.k_zi, self.z, x, self.own_cross, rhs)       # (first: it may be what factorises K_z)
        w = self._whitened_residual()
        if isinstance(v, WhitenedT):
            if w.shape[-1] == 1:
                # mean AND the rows' sums of squares (what the marginal variance of the same evaluation subtracts, PosteriorKernel.elwise)
                # from ONE pass over the whitened rows: they are N* x N elements, read from HBM either way
                dot, ss = ops.get_backend().rowreduce(v.zt, w, want_dot=True, want_ss=cache is not None)
                if cache is not None and ss is not None:
                    cache[("rowss", id(v))] = (ss, v)
                return self.m_i(x) + dot[..., None]
            v = v.plain()
        dot, _ = ops.get_backend().colreduce(v, w, want_dot=True, want_ss=False)
        return self.m_i(x) + dot[..., None]


# ---------------------------------------------------------------------------
# mean_var / mean_var_diag  (fdd.py:68-74)
# ---------------------------------------------------------------------------
def _call_mean(mean, x, cache):
    return mean(x, cache) if isinstance(mean, Mean) else mean(x)


def mean_var(mean, kernel, x):
    """Mean and variance sharing the cross-kernel evaluations."""
    from .matrix import deferred_checks

    cache = {}
    x = uprank(x)
    # (a posterior evaluated before anything factorised its observations factorises here: the `info` word is read when the
    # reductions / products that depend on the factor are queued behind it, not in front of them -- as `Normal.logpdf` does)
    with deferred_checks():
        m = _call_mean(mean, x, cache)
        if _accepts_cache(kernel):
            var = Dense(kernel.pairwise(x, None, cache=cache))
        else:
            var = KernelDense(kernel, x, None)
    return m, var


def mean_var_diag(mean, kernel, x):
    """Mean and marginal variances without forming the covariance
    (``tests/model/test_gp.py:201-211``)."""
    from .matrix import deferred_checks

    cache = {}
    x = uprank(x)
    with deferred_checks():          # (see mean_var)
        if isinstance(mean, PosteriorMean):
            from . import learnable
            got = learnable.marginals(mean, kernel, x, cache)        # (under learnable quantities: ONE autograd node for both)
            if got is not None:
                return got
        m = _call_mean(mean, x, cache)
        vd = kernel.elwise(x, cache=cache) if _accepts_cache(kernel) else kernel.elwise(x)
    return m, vd
