"""The admission layer of the differentiable paths: the host code that decides whether a call is in the case an autograd function of
``stheno_amd/autograd.py`` covers.  It unpacks the kernel into groups of primitives behind input maps (``kernels._map_groups``; across
processes ``_block_groups``), forms the mapped inputs in torch -- so the graph reaches the maps' parameters and ``x`` --, checks
dimensions, and then dispatches, leaves the call to the plain path, or refuses loudly.  Three entry points -- ``marginals`` (posterior
mean / marginal variances: exact, across processes, pseudo-point), ``logpdf`` (one process, a batch, several processes jointly, the
refusal) and ``elbo`` (the pseudo-point bound; ``requested``: its predicate) -- each return the differentiable result, or None for "run
the plain path", or raise where a value would come out cut off from the graph.  The hooks in ``kernels.py``, ``random.py`` and
``model/`` import this module where they call it: it imports ``kernels`` and ``autograd``, neither of which imports the other.
``covariance`` (the joint posterior covariance of the exact one-process case; ``graph_matrix``: what ``Normal.sample`` / ``.entropy``
ask) follows the same rule."""
import functools

import numpy as np
import torch

from . import autograd as _ag
from . import kernels as _k
from . import ops
from .matrix import Dense, Diagonal, KernelDense, Zero, config


# ---- does anything carry a gradient? ------------------------------------------------------------
def table_requires_grad(rows):
    """Does a term table in its tensor view (``Kernel.tensor_table()``) carry a gradient -- on a variance, a scale or a shape parameter?"""
    return torch.is_grad_enabled() and any(torch.is_tensor(p) and p.requires_grad for row in rows for p in row[1:])


def kernel_requires_grad(kernel, _depth=0):
    """Does any hyper-parameter reachable from ``kernel`` carry a gradient?  (Used to refuse -- loudly --
    the cases the differentiable paths do not cover, instead of returning a value cut off from the graph.)"""
    if _depth > 16:
        return False
    rows = kernel.tensor_table() if isinstance(kernel, _k.Kernel) else None
    if rows is not None:
        return table_requires_grad(rows)
    if isinstance(kernel, _k.MultiOutputKernel):
        return any(kernel_requires_grad(kernel.kernels[p], _depth + 1) for p in kernel.pids)
    for val in vars(kernel).values():
        if torch.is_tensor(val) and val.requires_grad:
            return True
        if isinstance(val, (_k.InputMap, _k.ScaleFn)) and val.requires_grad:       # a learnable shift, the parameters behind a feature
            return True                                                            # map or behind the function of `f * fn`
        if isinstance(val, _k.Kernel) and kernel_requires_grad(val, _depth + 1):
            return True
    return False


def groups_need_grad(groups, *others):
    """Does anything behind a kernel given as groups ``[(k_g, u_g)]`` require a gradient: a group's term table or mapped inputs, or one
    of the ``others`` (noise, residual, inducing inputs; ``None`` entries are skipped)?"""
    return torch.is_grad_enabled() and (
        any(table_requires_grad(kern.tensor_table()) or (torch.is_tensor(u) and u.requires_grad) for kern, u in groups)
        or any(t is not None and t.requires_grad for t in others))


def x_requires_grad(x):
    """Whether (any component of) an input specification carries gradients."""
    return x.requires_grad if torch.is_tensor(x) else any(x_requires_grad(q) for _, q in getattr(x, "parts", ()))


def density_requires_grad(kernel, x, noise, y):
    """Does anything behind a log-density require a gradient: the kernel, the inputs, the noise (diagonal or dense), the data ``y``?"""
    noisy = ((isinstance(noise, Diagonal) and noise.diag().requires_grad)
             or (isinstance(noise, Dense) and noise.mat is not None and noise.mat.requires_grad))
    return bool(noisy or (torch.is_tensor(y) and y.requires_grad) or x_requires_grad(x) or kernel_requires_grad(kernel))


def _matrix_requires_grad(v):
    """Does a structured matrix carry a gradient -- in what it holds already, or, for a kernel matrix that is not built yet, behind it?"""
    if isinstance(v, Diagonal):
        return bool(v.diag().requires_grad)
    if isinstance(v, KernelDense):
        if v._mat is not None and v._mat.requires_grad:
            return True
        return density_requires_grad(v.kernel, v.x, v.noise, None)
    if isinstance(v, Dense):
        return bool(v._mat is not None and v._mat.requires_grad)
    return bool(torch.is_tensor(v) and v.requires_grad)


def mean_requires_grad(mean, _depth=0):
    """Does anything reachable from a mean carry a gradient: a tensor among its attributes (a scale, the observations and inputs of a
    posterior mean), a learnable map or function (a module's parameters included), a kernel, a kernel matrix, another mean?"""
    if _depth > 16 or mean is None:
        return False
    if isinstance(mean, _k.MultiOutputMean):
        measure = mean._measure()
        return measure is not None and any(mean_requires_grad(measure.means[p], _depth + 1) for p in mean.pids)
    for val in vars(mean).values():
        if torch.is_tensor(val):
            if val.requires_grad:
                return True
        elif isinstance(val, (_k.InputMap, _k.ScaleFn)):
            if val.requires_grad:
                return True
        elif isinstance(val, _k.Kernel):
            if kernel_requires_grad(val):
                return True
        elif isinstance(val, _k.Mean):
            if mean_requires_grad(val, _depth + 1):
                return True
        elif isinstance(val, (Dense, Diagonal)):
            if _matrix_requires_grad(val):
                return True
        elif isinstance(val, torch.nn.Module):
            if any(p.requires_grad for p in val.parameters()):
                return True
    return False


def normal_requires_grad(dist):
    """Does the mean or the variance of a ``Normal`` carry a graph?  Asked of what exists already (tensors, structured matrices) and, for
    a finite-dimensional distribution of a process whose quantities are still lazy, of the process's mean and kernel, the inputs and
    the noise -- nothing is computed by asking.  What ``Normal.w2`` asks before it refuses."""
    if not torch.is_grad_enabled():
        return False
    if any(_matrix_requires_grad(q.value) for q in (dist._m, dist._v, dist._d) if q.known):
        return True
    p = getattr(dist, "p", None)
    if p is None or isinstance(p, int):
        return False
    return bool(density_requires_grad(p.kernel, dist._xr, dist.noise, None) or mean_requires_grad(p.mean))


def refuse_fn_scaled(what, kernels, x, *others):
    """Refuse -- before any launch -- ``what`` under a learnable quantity behind a function-scaled kernel (``f * fn``): the one
    differentiable case there is the log-density of one process (``_scaled_process_logpdf``).  ``kernels``: what the call evaluates;
    ``x``: an input that primes the functions' probes; ``others``: further tensors whose gradient the call would drop (None: skipped)."""
    if not torch.is_grad_enabled():
        return
    kernels = [k for k in kernels if isinstance(k, _k.Kernel) and _k._contains_fn_scaled(k)]
    if not kernels:
        return
    for k in kernels:
        _k.prime_scale_fns(k, x)
    if (any(kernel_requires_grad(k) for k in kernels) or x_requires_grad(x)
            or any(torch.is_tensor(t) and t.requires_grad for t in others)):
        raise NotImplementedError(
            f"{what} under learnable quantities behind a {_k.FN_SCALED} kernel (a process times a function) is not implemented -- "
            "gradients there cover `f(x, noise).logpdf(y)` of ONE process, unbatched, with respect to variances, scalar length scales, "
            "RQ's alpha, the noise, y, the mean and the function's parameters --: its value would be cut off from the autograd graph.  "
            "Wrap the call in torch.no_grad() if that is intended")


# ---- pieces the entry points share ------------------------------------------------------------
def kdiag_terms(tensor_terms, x):
    """``k(x_i, x_i)`` (N,) of a sum of primitives as a differentiable torch expression (O(N D)): stationary terms are their variance,
    a linear term ``v |x_i|^2 / s^2``."""
    out = None
    for kind, v, s in tensor_terms:
        t = v * (x * x).sum(-1) / (s * s) if kind == "linear" else v * torch.ones(x.shape[:-1], dtype=x.dtype, device=x.device)
        out = t if out is None else out + t
    return out


def _diagonal_noise(K):
    """The noise of the kernel matrix ``K`` as a vector (N,) or None (no noise); ``NotImplemented`` when it is neither (dense, batched)."""
    noise_vec = K.differentiable_noise()
    if noise_vec is NotImplemented or (noise_vec is not None and noise_vec.dim() != 1):
        return NotImplemented
    return noise_vec


def _residual_in_graph(pm, z, batched=False):
    """``(True, r)``: the residual ``r = y - m_z(z)`` (N, 1) -- ``batched``: (B, N, 1) -- of the posterior mean ``pm``, inside the graph
    (None without a mean); ``(False, None)`` when it is not one column."""
    if pm is None:
        return True, None
    y, r = pm._residual()
    if r.dim() != (3 if batched else 2) or r.shape[-1] != 1 or (batched and tuple(r.shape[:2]) != tuple(z.shape[:2])):
        return False, None
    if pm._r_detached and not r.requires_grad:        # (formed under no_grad: form it again inside the graph)
        r = y - pm.m_z(z)
    return True, r


def _columns(pm, x, mu, s, prior_diag, kt, always=True):
    """``(mean column or None, marginal-variance column or None)`` from the outputs ``(mu, s)`` of an autograd function: the prior mean
    is added in torch; the value of ``k(x, x)`` comes from the plain path (``prior_diag()``, its bits; None without a posterior kernel),
    its gradient from the same sum written in torch (``kt``; ``always=False``: added only where it carries a gradient)."""
    mean = pm.m_i(x) + mu[..., None] if pm is not None else None
    vd = None
    if prior_diag is not None:
        vd = prior_diag()
        if always or (torch.is_tensor(kt) and kt.requires_grad):
            vd = vd + (kt - kt.detach())[..., None]
        vd = vd - s[..., None]
    return mean, vd


class _Layout:
    """The block layout of ``autograd._JointLogpdf`` / ``_BlockPosteriorMarginals`` under construction: ``blocks`` (one
    ``autograd.Block`` per group), the flat ``params`` behind them, and ``us``, the mapped inputs -- ``imap(ins[i])``, formed once per
    input and map, in torch: the graph reaches the map's parameter."""

    def __init__(self, ins):
        self.ins, self.us, self.blocks, self.params = ins, [], [], []
        self._where = {}

    def mapped(self, i, imap):
        """Position of ``imap(ins[i])`` among the mapped inputs."""
        key = (i, id(imap))
        if key not in self._where:
            self._where[key] = (len(self.us), imap)    # (the map is kept: its id cannot be recycled while the table lives)
            self.us.append(self.ins[i] if imap is None else imap(self.ins[i]))
        return self._where[key][0]

    def add(self, which, i, j, rows, factor, row, col, mx, my, a=None, b=None):
        """One group ``factor * D^(a, b) k_g(mx(ins[row]), my(ins[col]))`` of block ``(i, j)``, ``rows`` its term table in the tensor
        view; the factor rides in the variances."""
        kinds, pr = _ag._pack(rows)
        if torch.is_tensor(factor) or factor != 1.0:
            pr[: len(kinds)] = [v * factor for v in pr[: len(kinds)]]
        self.blocks.append(_ag.Block(which, i, j, kinds, len(pr), self.mapped(row, mx), self.mapped(col, my), a, b))
        self.params.extend(pr)


# ---- posterior mean and marginal variances ------------------------------------------------------------
def sparse_pair(kernel):
    """The link (weak references to ``(obs, measure)``) behind ``PosteriorKernel + SubspaceKernel`` of one pseudo-point conditioning
    (``AbstractPseudoObservations.posterior_kernel``), else None."""
    if isinstance(kernel, _k.Sum) and isinstance(kernel.a, _k.PosteriorKernel) and isinstance(kernel.b, _k.SubspaceKernel):
        link = getattr(kernel.a, "sparse", None)
        if link is not None and getattr(kernel.b, "sparse", None) is link:
            return link
    return None


def marginals(pm, kernel, x, cache):
    """Posterior mean / marginal variances under learnable quantities: ``(mean column or None, marginal-variance column or None)`` for
    the posterior mean ``pm`` and / or the posterior kernel ``kernel`` (a ``PosteriorKernel``, or the ``PosteriorKernel +
    SubspaceKernel`` of a pseudo-point conditioning) at the test inputs ``x``; either may be None.  None when grad is off, when nothing
    learnable is behind them or when the call is outside the three covered cases: the plain path then runs exactly as before."""
    if not torch.is_grad_enabled():
        return None
    src = pm if pm is not None else kernel
    K_z = getattr(src, "K_z", None)
    refuse_fn_scaled("a posterior mean / marginal variance", (kernel, getattr(pm, "k_zi", None), getattr(K_z, "kernel", None)), x,
                     getattr(src, "z", None) if torch.is_tensor(getattr(src, "z", None)) else None, *_posterior_tensors(pm, K_z))
    for k in (kernel, getattr(pm, "k_zi", None)):
        if isinstance(k, _k.Kernel) and _k.has_per_batch(k) and kernel_requires_grad(k):
            raise NotImplementedError(f"gradients of posterior means and marginal variances are not implemented with {_k.PER_BATCH}: "
                                      "this call would return values cut off from the autograd graph -- wrap it in torch.no_grad() if "
                                      "that is intended")
    if isinstance(kernel, _k.PosteriorKernel) or (kernel is None and pm.sparse is None):
        return _exact_marginals(pm, kernel, x, cache)
    link = pm.sparse if pm is not None else sparse_pair(kernel)
    if link is None or (pm is not None and kernel is not None and sparse_pair(kernel) is not link):
        return None
    return _sparse_marginals(pm, kernel, link, x, cache)


def _posterior_tensors(pm, K_z):
    """The tensors beside kernel and inputs that a posterior mean / variance depends on: the observations' noise and residual."""
    out = []
    noise = getattr(K_z, "noise", None)
    if isinstance(noise, Diagonal):
        out.append(noise.diag())
    elif isinstance(noise, Dense) and noise.mat is not None:
        out.append(noise.mat)
    for name in ("y", "r", "rhs"):
        t = getattr(pm, name, None)
        if torch.is_tensor(t):
            out.append(t)
    return out


def _posterior_parts(pm, K_z, k, z, x, cache, own_cross):
    """The plain HIP path of the posterior marginals, unchanged (``PosteriorMean.__call__`` / ``PosteriorKernel.elwise``): returns
    ``(chol, w, v, mu, s)`` -- the factor, ``w = L^{-1} r`` (None without a mean), ``v = L^{-1} k(z, x)`` (or ``WhitenedT``),
    ``mu = v^T w`` and ``s = |v_j|^2`` (N*,), the latter two from one pass over ``v``."""
    rhs = None
    if pm is not None and pm._w is None and own_cross and hasattr(K_z, "can_factor_with_rows"):
        _, r = pm._residual()
        if r.dim() == 2 and r.shape[-1] == 1 and not r.requires_grad:
            rhs = (r, pm._took)
    v = _k._whiten(cache, K_z, k, z, x, own_cross, rhs)
    w = pm._whitened_residual() if pm is not None else None
    be = ops.get_backend()
    if isinstance(v, _k.WhitenedT):
        mu, s = be.rowreduce(v.zt, w, want_dot=w is not None, want_ss=True)
    else:
        mu = be.colreduce(v, w, want_dot=True, want_ss=False)[0] if w is not None else None
        _, s = be.colreduce(v, want_ss=True)
    return K_z.chol(), w, v, mu, s


def _exact_marginals(pm, pk, x, cache):
    """An EXACT posterior of one process predicted from its own observations, through ``autograd._PosteriorMarginals``.  Anything else
    behind an exact conditioning -- a component of a sum, several observed processes, derivatives -- is the block path's
    (``_block_marginals``), which answers None itself where it does not apply: pseudo-point posteriors, chained conditioning, batched
    inputs, a block that is no sum of groups of primitives behind input maps, dense noise.  BATCHED inputs -- ``x`` and the observed
    inputs (B, ., D) with one batch size, scalar or (B, N) noise, hyper-parameters shared by the batch -- are the same case through
    ``autograd._BatchedPosteriorMarginals`` (the forward and the first stages of the backward are the unbatched function's own code);
    per-batch hyper-parameters were refused by the caller, without a gradient they stay the plain path's."""
    src = pm if pm is not None else pk
    if not getattr(src, "exact", False):
        return None
    K_z, k, z = src.K_z, src.k_zi, src.z
    if pk is not None and not (pk.exact and pk.K_z is K_z and pk.z is z and pk.k_zi is k and pk.k_zj is k and pk.k_ij is k):
        return _block_marginals(pm, pk, x, cache)
    noted = getattr(K_z, "built_from", None)       # (a batch under a sum behind different maps: materialised, `kernels.note_built_from`)
    if noted is not None and not isinstance(K_z, KernelDense) and noted[0] is k and noted[1] is z and torch.is_tensor(z) and z.dim() == 3:
        observed = KernelDense(*noted)             # (never built: asked for its noise only)
    else:
        observed = K_z
    if not isinstance(observed, KernelDense) or observed.kernel is not k:
        return _block_marginals(pm, pk, x, cache)
    if not (torch.is_tensor(x) and torch.is_tensor(z) and x.dim() == z.dim() and x.dim() in (2, 3) and x.shape[-1] == z.shape[-1]
            and x.dtype == z.dtype and x.device == z.device):
        return None
    batched = x.dim() == 3     # B independent posteriors under shared hyper-parameters: autograd._BatchedPosteriorMarginals
    if batched and (x.shape[0] != z.shape[0] or _k.has_per_batch(k)):
        return None
    noise_vec = observed.differentiable_noise() if batched else _diagonal_noise(K_z)
    if noise_vec is NotImplemented or (batched and noise_vec is not None and tuple(noise_vec.shape) != tuple(z.shape[:2])):
        return None
    groups = _k._symmetric_groups(k)        # terms behind the same input map: one group is the plain case
    if groups is None or not all(kern.tensor_terms() for kern, _, _ in groups):
        return None if batched else _block_marginals(pm, pk, x, cache)
    ok, r = _residual_in_graph(pm, z, batched)
    if not ok:
        return None
    if not (kernel_requires_grad(k) or x.requires_grad or z.requires_grad
            or (noise_vec is not None and noise_vec.requires_grad) or (r is not None and r.requires_grad)):
        return None
    mapped = [(kern, z if imap is None else imap(z), x if imap is None else imap(x)) for kern, imap, _ in groups]
    for _, zin, xin in mapped:
        if zin.requires_grad or xin.requires_grad:
            _ag.check_input_dims(xin)
    xd = x.detach()                  # (the plain path sees values only: the rows path stays open, one whitening serves mean and variance)
    run = functools.partial(_posterior_parts, pm, K_z, k, z, xd, cache, src.own_cross)
    mu, s = _ag.posterior_marginals(mapped, r, noise_vec, run)
    kt = sum(kdiag_terms(kern.tensor_terms(), xin) for kern, _, xin in mapped) if pk is not None else None
    return _columns(pm, x, mu, s, (lambda: k.elwise(xd)) if pk is not None else None, kt)


def _block_groups(k):
    """A kernel as groups ``s * D^(a, b) k_g(imap_x(x), imap_y(y))``: ``[(s, a, b, k_g, imap_x, imap_y)]`` with ``k_g`` a sum of
    primitives, ``(a, b)`` the derivative slots of a ``DiffKernel`` (both ``None``: the plain case of ``_map_groups``) and ``s`` a
    factor (a float, or the tensor a ``Scaled`` carries).  ``_map_groups`` extended to look inside ``DiffKernel``, ``Sum``, ``Scaled``
    and ``Reversed``: what the blocks of several processes' covariance are made of.  ``[]`` for the zero kernel (independent
    processes); None when the kernel has no such form."""
    if isinstance(k, _k.ZeroKernel):
        return []
    if isinstance(k, _k.DiffKernel):
        kern, imap, imap_y = k.k.input_scaled_view()
        return [(1.0, k.dim_x, k.dim_y, kern, imap, imap_y)]
    if not isinstance(k, _k.Kernel) or isinstance(k, (_k.MultiOutputKernel, _k._CrossKernel, _k.PosteriorKernel, _k.SubspaceKernel)):
        return None
    plain = _k._map_groups(k)
    if plain is not None:
        return [(1.0, None, None, kern, mx, my) for kern, mx, my in plain]
    if isinstance(k, _k.Sum):
        ga, gb = _block_groups(k.a), _block_groups(k.b)
        return None if ga is None or gb is None else ga + gb
    if isinstance(k, _k.Scaled):
        g = _block_groups(k.k)
        return None if g is None else [(s * k.v, a, b, kern, mx, my) for s, a, b, kern, mx, my in g]
    if isinstance(k, _k.Reversed):
        g = _block_groups(k.k)      # (a sum of primitives is symmetric: the slots and the maps change places)
        return None if g is None else [(s, b, a, kern, my, mx) for s, a, b, kern, mx, my in g]
    return None


def _group_factor(s, a, b, imap):
    """The factor in front of a group's term table: ``s``, times the chain-rule factors ``1 / l_a``, ``1 / l_b`` of a derivative behind
    per-dimension length scales (a torch expression where ``s`` or the scales are tensors)."""
    f = s
    if isinstance(imap, _k._ScaleMap):
        for dim in (a, b):
            if dim is not None:
                f = f / (imap.param[dim] if torch.is_tensor(imap.param) else float(np.asarray(imap.param, dtype=np.float64).reshape(-1)[dim]))
    return f


def _group_diag(group, x):
    """``s D^(a, b) k_g(imap(x_j), imap(x_j))`` (N,) of a group as a torch expression -- ``kdiag_terms`` for a plain group, the closed
    form of ``DiffKernel.elwise`` for a derivative -- or None when the group sees its two arguments through different maps."""
    s, a, b, kern, mx, my = group
    if not _k._same_map(mx, my):
        return None
    xm = x if mx is None else mx(x)
    if a is None and b is None:
        return s * kdiag_terms(kern.tensor_terms(), xm)
    f = _group_factor(s, a, b, mx)
    if a is not None and b is not None:
        if a != b:
            return torch.zeros(x.shape[:-1], dtype=x.dtype, device=x.device)
        value = sum(var / (scale * scale) * _k._DIFF_AT_ZERO[kind] for kind, var, scale in kern.tensor_terms()) * f
        return value * torch.ones(x.shape[:-1], dtype=x.dtype, device=x.device)
    lin = sum(var / (scale * scale) for kind, var, scale in kern.tensor_terms() if kind == "linear") * f
    return lin * xm[..., a if b is None else b]


def _block_marginals(pm, pk, x, cache):
    """What ``_exact_marginals`` returns, for ONE exact conditioning step on a prior measure that the one-process case does not cover:
    one or several observation sets (``z`` a tensor or a ``MultiInput``), a prediction of any one process of the measure -- a
    component of a sum, another observed process, a derivative --, through ``autograd._BlockPosteriorMarginals``.  Every block of the
    lower block triangle of the observed processes' covariance, every cross-kernel with the predicted process and that process's own
    kernel has to be a sum of groups (``_block_groups``); None otherwise (the plain path then runs as before).  Refuses, before any
    launch, the two gradients the derivative kernels do not provide."""
    src = pm if pm is not None else pk
    K_z, k_cross, z = src.K_z, src.k_zi, src.z
    if pk is not None and not (pk.exact and pk.K_z is K_z and pk.z is z and pk.k_zi is k_cross and pk.k_zj is k_cross):
        return None
    if not isinstance(K_z, KernelDense) or K_z.x is not z:
        return None
    kz = K_z.kernel
    if isinstance(z, _k.MultiInput):
        if not (isinstance(kz, _k.MultiOutputKernel) and isinstance(k_cross, _k._CrossKernel) and k_cross.mok is kz):
            return None
        kernels = kz.kernels
        parts = kz._split(z)
        if any(not torch.is_tensor(zi) or kernels[pid].num_outputs(zi) != zi.shape[-2] for pid, zi in parts):
            return None                               # (nested product processes)
        block = lambda i, j: kernels[parts[i][0]] if i == j else kernels[parts[i][0], parts[j][0]]      # noqa: E731
        cross = lambda i: kernels[parts[i][0], k_cross.j]                                               # noqa: E731
    else:
        if isinstance(kz, _k.MultiOutputKernel) or not torch.is_tensor(z):
            return None
        parts = [(None, z)]
        block, cross = (lambda i, j: kz), (lambda i: k_cross)
    ins = [zi for _, zi in parts] + [x]
    if not (torch.is_tensor(x) and all(t.dim() == 2 and t.shape[-1] == x.shape[-1] and t.dtype == x.dtype and t.device == x.device for t in ins)):
        return None
    noise_vec = _diagonal_noise(K_z)
    if noise_vec is NotImplemented:
        return None
    P = len(parts)
    spec = []                                          # (which, i, j, group, row input, column input)
    for which, i, j, col in [("K", i, j, j) for i in range(P) for j in range(i + 1)] + [("C", i, 0, P) for i in range(P)]:
        groups = _block_groups(block(i, j) if which == "K" else cross(i))
        if groups is None:
            return None
        spec += [(which, i, j, g, i, col) for g in groups]
    own = _block_groups(pk.k_ij) if pk is not None else []
    if own is None:
        return None
    ok, r = _residual_in_graph(pm, z)
    if not ok:
        return None
    lay = _Layout(ins)
    for which, i, j, (s, a, b, kern, mx, my), row, col in spec:
        rows = kern.tensor_table()
        if rows is None:
            return None
        if not rows:
            continue
        if (a is not None or b is not None) and ((mx is not None and mx.requires_grad) or (my is not None and my.requires_grad)):
            raise NotImplementedError("gradients of a posterior with respect to per-dimension length scales under a derivative "
                                      "(`k.stretch(vector)` behind `f.diff()`) are not implemented")
        lay.add(which, i, j, rows, _group_factor(s, a, b, mx), row, col, mx, my, a, b)
    own_diag = [_group_diag(g, x) for g in own if g[3].tensor_table()]
    if any(t is None for t in own_diag):
        return None
    kt = sum(own_diag) if own_diag else None
    if not (any(t.requires_grad for t in lay.params + lay.us) or (torch.is_tensor(kt) and kt.requires_grad)
            or (noise_vec is not None and noise_vec.requires_grad) or (r is not None and r.requires_grad)):
        return None
    for blk in lay.blocks:
        if lay.us[blk.ua].requires_grad or lay.us[blk.ub].requires_grad:
            if blk.a is not None and blk.b is not None:
                raise NotImplementedError("gradients with respect to the inputs of a mixed derivative block (both the row and the column "
                                          "process are derivatives: `xs.requires_grad` when a derivative is predicted from observed "
                                          "derivatives, or inputs of derivative observations that require a gradient) are not implemented")
            _ag.check_input_dims(lay.us[blk.ua] if lay.us[blk.ua].requires_grad else lay.us[blk.ub])
    xd = x.detach()
    run = functools.partial(_posterior_parts, pm, K_z, k_cross, z, xd, cache, src.own_cross)
    mu, s = _ag.block_posterior_marginals(r, noise_vec, run, tuple(zi.shape[-2] for _, zi in parts), tuple(lay.blocks), lay.us, lay.params)
    return _columns(pm, x, mu, s, (lambda: pk.k_ij.elwise(xd)) if pk is not None else None, kt, always=False)


def _sparse_posterior_parts(pm, pk, sk, k, z, x, cache, chol_a):
    """The plain HIP path of the pseudo-point posterior marginals, unchanged (``PosteriorMean.__call__``, ``PosteriorKernel.elwise`` +
    ``SubspaceKernel.elwise``): returns ``(chol_z, chol_a, chol_post, w, vz, va, mu, s)`` as ``autograd._SparsePosteriorMarginals``
    takes them -- ``mu = vz^T w``, ``s = |vz_j|^2 - |va_j|^2``; what a mean-only (``pk`` None) or variance-only (``pm`` None) call does
    not need is None."""
    be = ops.get_backend()
    K_z = (pm if pm is not None else pk).K_z
    vz = _k._whiten(cache, K_z, k, z, x)
    w = mu = va = s = chol_post = None
    if pm is not None:
        w = pm._whitened_residual()
        mu = be.colreduce(vz, w, want_dot=True, want_ss=False)[0]
    if pk is not None:
        va = _k._whiten(cache, sk.A, k, z, x)
        s = be.colreduce(vz, want_ss=True)[1] - be.colreduce(va, want_ss=True)[1]
        chol_post = sk.A.chol().chols[1]
    return K_z.chol(), chol_a, chol_post, w, vz, va, mu, s


def _sparse_marginals(pm, kernel, link, x, cache):
    """A PSEUDO-POINT posterior (VFE / FITC / DTC; ``link``: its ``(obs, measure)``, weakly), through
    ``autograd._SparsePosteriorMarginals``.  None when nothing learnable is behind it or when the call is outside the case the bound
    admits (``elbo``: noise-free inducing points of the observed process itself, one kernel that is a sum of primitives behind one
    input map, diagonal noise, unbatched) at the inducing process."""
    obs, measure = link[0](), link[1]()
    if obs is None or measure is None:
        return None
    p_x, xo, noise_x = obs.fdd.p, obs.fdd._xr, obs.fdd.noise
    p_z, z, noise_z = obs.u.p, obs.u._xr, obs.u.noise
    if isinstance(xo, _k.MultiInput) or isinstance(z, _k.MultiInput) or not isinstance(noise_x, Diagonal) or not isinstance(noise_z, Zero):
        return None
    k = measure.kernels[p_z]
    view = k.input_scaled_view() if isinstance(k, _k.Kernel) else None
    if view is None or not _k._same_map(view[1], view[2]):
        return None
    if not (measure.kernels[p_x] is k and measure.kernels[p_z, p_x] is k):
        return None
    if not all(torch.is_tensor(t) and t.dim() == 2 and t.shape[-1] == z.shape[-1] and t.dtype == z.dtype and t.device == z.device
               for t in (x, xo, z)):
        return None
    pk = sk = None
    if kernel is not None:
        pk, sk = kernel.a, kernel.b
        if not (pk.k_ij is k and pk.k_zi is k and pk.k_zj is k and sk.k_zi is k and sk.k_zj is k and pk.z is z and sk.z is z):
            return None
    if pm is not None and not (pm.k_zi is k and pm.z is z and pm.m_i is measure.means[p_z] and (pk is None or pk.K_z is pm.K_z)):
        return None
    parts = obs._parts.get(measure)
    if parts is None or parts["K_z"] is not (pm if pm is not None else pk).K_z or noise_x.diag().dim() != 1:
        return None
    kern, imap, _ = view                          # k(a, b) = kern(imap(a), imap(b))
    if not kern.tensor_terms():
        return None
    noise_vec = noise_x.diag()
    learnable = kernel_requires_grad(k) or any(t.requires_grad for t in (x, xo, z, noise_vec, obs.y))
    if not learnable and isinstance(measure.means[p_x], _k.ZeroMean):
        return None                               # (nothing learnable, and no mean that could hide a parameter: not even the residual)
    r = obs.y - measure.means[p_x](xo)
    if r.dim() != 2 or r.shape[-1] != 1 or not (learnable or r.requires_grad):
        return None
    xm, zm, xsm = (t if imap is None else imap(t) for t in (xo, z, x))
    if xm.requires_grad or zm.requires_grad or xsm.requires_grad:
        _ag.check_input_dims(xsm)
    xd = x.detach()                  # (the plain path sees values only)
    cache = {} if cache is None else cache        # (K_s is evaluated once for the two whitenings)
    run = functools.partial(_sparse_posterior_parts, pm, pk, sk, k, z, xd, cache, parts["chol_A"])
    mu, s = _ag.sparse_posterior_marginals(kern, xm, zm, xsm, r, noise_vec, obs.method, run)
    kt = kdiag_terms(kern.tensor_terms(), xsm) if pk is not None else None
    return _columns(pm, x, mu, s, (lambda: k.elwise(xd)) if pk is not None else None, kt)


# ---- the joint posterior covariance ------------------------------------------------------------
def _admit_covariance(pk, x):
    """The admitted case of the differentiable joint covariance, or None: an EXACT posterior of one process predicted from its own
    observations, unbatched, scalar or per-point noise, a kernel that is a sum of groups of primitives behind input maps -- the case
    ``_exact_marginals`` handles directly -- with something learnable behind it.  Returns ``(groups, noise_vec)``.  Nothing is launched
    here: every other call is the plain path's, exactly as before."""
    if not (isinstance(pk, _k.PosteriorKernel) and pk.exact):
        return None
    K_z, k, z = pk.K_z, pk.k_zi, pk.z
    if not (pk.k_zj is k and pk.k_ij is k and isinstance(K_z, KernelDense) and K_z.kernel is k and K_z.x is z):
        return None
    if not (torch.is_tensor(x) and torch.is_tensor(z) and x.dim() == 2 and z.dim() == 2 and x.shape[-1] == z.shape[-1]
            and x.dtype == z.dtype and x.device == z.device):
        return None
    noise_vec = _diagonal_noise(K_z)
    if noise_vec is NotImplemented:
        return None
    groups = _k._symmetric_groups(k)
    if groups is None or not all(kern.tensor_terms() for kern, _, _ in groups):
        return None
    if not (kernel_requires_grad(k) or x.requires_grad or z.requires_grad or (noise_vec is not None and noise_vec.requires_grad)):
        return None
    return groups, noise_vec


def covariance(pk, x, cache, **kw):
    """The joint posterior covariance ``pk.pairwise(x)`` (N*, N*) under learnable quantities, through ``autograd._PosteriorCovariance``:
    the plain path's bits with a gradient to variances, scales, shapes, map parameters, the observation noise, ``x`` and the observed
    inputs.  ``kw``: what ``pairwise`` was called with (``lower``, ``diag_add``, ``diag_vec``: constants, added by the plain path
    itself).  None when grad is off or the call is outside the admitted case (``_admit_covariance``).  A function-scaled kernel and
    per-batch hyper-parameters under a gradient are refused as the marginals refuse them."""
    if not torch.is_grad_enabled():
        return None
    K_z = getattr(pk, "K_z", None)
    z = getattr(pk, "z", None)
    refuse_fn_scaled("a posterior covariance", (pk, getattr(pk, "k_zi", None), getattr(K_z, "kernel", None)), x,
                     z if torch.is_tensor(z) else None, *_posterior_tensors(None, K_z))
    if _k.has_per_batch(pk) and kernel_requires_grad(pk):
        raise NotImplementedError(f"gradients of posterior covariances are not implemented with {_k.PER_BATCH}: this call would return "
                                  "values cut off from the autograd graph -- wrap it in torch.no_grad() if that is intended")
    got = _admit_covariance(pk, x)
    if got is None:
        return None
    groups, noise_vec = got
    k = pk.k_zi
    mapped = [(kern, z if imap is None else imap(z), x if imap is None else imap(x)) for kern, imap, _ in groups]
    for _, zin, xin in mapped:
        if zin.requires_grad or xin.requires_grad:
            _ag.check_input_dims(xin)
    xd = x.detach()
    cache = {} if cache is None else cache

    def run():
        cov = pk.pairwise(xd, None, cache=cache, **kw)          # (grad is off in here: the plain path, as it is)
        return K_z.chol(), _k._whiten(cache, K_z, k, z, xd, pk.own_cross), cov

    return _ag.posterior_covariance(mapped, noise_vec, run)


def graph_matrix(var):
    """The matrix of a variance (``matrix.Dense``) as a tensor inside the autograd graph, or None when it carries none: what
    ``Normal.sample`` / ``Normal.entropy`` ask before they take their differentiable form.  A lazily materialised posterior
    covariance is materialised here only in the admitted case of :func:`covariance`; nothing else is touched."""
    if not torch.is_grad_enabled() or not isinstance(var, Dense):
        return None
    mat = var._mat
    if mat is None and isinstance(var, KernelDense) and var._chol is None and isinstance(var.noise, (type(None), Zero)) \
            and _admit_covariance(var.kernel, _k.uprank(var.x)) is not None:
        mat = var.mat
    return mat if (torch.is_tensor(mat) and mat.dim() == 2 and mat.requires_grad) else None


# ---- the log-density ------------------------------------------------------------
def logpdf(var, r):
    """The log-density of the residual ``r`` -- (N, C), or (B, N, 1) for a batch of data sets -- under the kernel-matrix variance
    ``var`` (a ``KernelDense``) as a node of the graph; None when nothing behind it is learnable, or with grad off.  Raises for a call
    outside the covered cases whose value would come out cut off from the graph."""
    batched_ok = (r.dim() == 3 and r.shape[-1] == 1 and torch.is_tensor(getattr(var, "x", None)) and var.x.dim() == 3
                  and tuple(var.x.shape[:-2]) == tuple(r.shape[:-2]))
    if r.dim() == 2 or batched_ok:
        lp = _process_logpdf(var, r)
        if lp is not None:
            return lp if (r.dim() == 3 or lp.shape[0] != 1) else lp[0]
    if not torch.is_grad_enabled():
        return None
    if isinstance(var.kernel, _k.Kernel) and _k._contains_fn_scaled(var.kernel):
        lp = _scaled_process_logpdf(var, r)
        if lp is not None:
            return lp[0] if lp.shape[0] == 1 else lp
        return None               # (nothing learnable behind it: the plain path)
    if r.dim() == 2 and isinstance(var.kernel, _k.MultiOutputKernel):      # several processes observed jointly
        lp = _joint_logpdf(var, r)
        if lp is not None:
            return lp[0] if lp.shape[0] == 1 else lp
    if density_requires_grad(var.kernel, var.x, var.noise, r):
        if isinstance(var.kernel, _k.Kernel) and _k.has_per_batch(var.kernel):
            raise NotImplementedError(f"gradients of logpdf with {_k.PER_BATCH} are implemented for one batch of independent data sets whose "
                                      "kernel is a sum of primitives behind ONE input map, with scalar or per-point noise; this call (sums "
                                      "behind different maps, several processes, a posterior) would return a value cut off from the "
                                      "autograd graph -- wrap it in torch.no_grad() if that is intended")
        raise NotImplementedError("gradients of logpdf are implemented for one process (or one batch of independent data sets) whose kernel "
                                  "is a sum of primitives with scalar or per-point noise; this call (multi-process, posterior or "
                                  "dense-noise) would return a value cut off from the autograd graph -- wrap it in torch.no_grad() "
                                  "if that is intended")
    return None


def _process_logpdf(var, r):
    """One process, or one batch of independent data sets under shared hyper-parameters: ``k(x) = sum_g k_g(m_g(x))`` with every
    ``k_g`` a sum of primitives (``m_g``: the division by per-dimension length scales, the periodic embedding, or none) -- the fused
    path runs ``k_g`` on the mapped inputs; torch differentiates the maps (d/dl, d/dperiod, d/dx).  One group is the plain case;
    several go group by group through the unbatched log-density only."""
    noise_vec, noise_mat = var.differentiable_noise(), None
    if noise_vec is NotImplemented and r.dim() == 2 and isinstance(var.noise, Dense) and var.noise.mat is not None and var.noise.mat.dim() == 2:
        noise_vec, noise_mat = None, var.noise.mat       # a dense noise covariance: its cotangent is that of K
    if noise_vec is not None and noise_vec is not NotImplemented and noise_vec.dim() != r.dim() - 1:
        noise_vec = NotImplemented
    # (a kernel matrix k(x) is symmetric: every group sees both arguments through the same map)
    groups = _k._symmetric_groups(var.kernel) if torch.is_tensor(var.x) else None
    if groups is not None and len(groups) > 1 and r.dim() != 2:
        groups = None
    if noise_vec is NotImplemented or groups is None or not all(kern.tensor_terms() is not None for kern, _, _ in groups):
        return None
    mapped = [(kern, var.x if imap is None else imap(var.x)) for kern, imap, _ in groups]
    if not groups_need_grad(mapped, noise_vec, r, noise_mat):
        return None
    for _, xin in mapped:
        if xin.requires_grad:
            _ag.check_input_dims(xin)
    return _ag.gp_logpdf(mapped, noise_vec, r, noise_mat)


def _scaled_process_logpdf(var, r):
    """One process, unbatched, whose kernel is a sum of groups, each optionally between one function on both sides: ``k(x) = sum_g
    diag(s_g) k_g(m_g(x)) diag(s_g)``, ``s_g = fn_g(x)`` formed HERE in torch -- the graph carries its gradient into the function's
    parameters -- and handed to ``autograd._GPLogpdf`` (``gp_logpdf_scaled``) as a tensor.  None when nothing behind the density is learnable; every other
    call under a learnable quantity is refused, before any launch."""
    what = "this log-density (inputs with a gradient, a batch, several processes, a posterior, dense noise, learnable input maps)"
    noise = var.noise
    noise_t = noise.diag() if isinstance(noise, Diagonal) else getattr(noise, "mat", None) if isinstance(noise, Dense) else None
    groups = _k._symmetric_scaled_groups(var.kernel) if torch.is_tensor(var.x) else None
    noise_vec = var.differentiable_noise()
    covered = (groups is not None and r.dim() == 2 and var.x.dim() == 2 and noise_vec is not NotImplemented and not var.x.requires_grad
               and (noise_vec is None or noise_vec.dim() == 1) and not _k.has_per_batch(var.kernel)
               and all(kern.tensor_terms() is not None for kern, *_ in groups))
    if not covered:
        refuse_fn_scaled(what, (var.kernel,), var.x, r, noise_t)
        return None
    x = var.x
    mapped = [(kern, x if imap is None else imap(x), None if fx is None else fx(x)) for kern, imap, _, fx, _ in groups]
    if any(u.requires_grad for _, u, _ in mapped):
        refuse_fn_scaled(what, (var.kernel,), x, *[u for _, u, _ in mapped])
    if not (groups_need_grad([(kern, u) for kern, u, _ in mapped], noise_vec, r) or any(s is not None and s.requires_grad for _, _, s in mapped)):
        return None
    return _ag.gp_logpdf_scaled(mapped, noise_vec, r)


def _joint_logpdf(var, r):
    """Differentiable joint log-density under the ``MultiOutputKernel`` of ``var`` at its multi-input; None when the noise is not
    diagonal or a block of the lower block triangle is not a sum of primitives behind input maps with scalar hyper-parameters (the
    caller then refuses)."""
    mok, x, noise_vec = var.kernel, var.x, _diagonal_noise(var)
    if _k.has_per_batch(mok):
        raise NotImplementedError(f"several processes observed jointly are not implemented with {_k.PER_BATCH}")
    if noise_vec is NotImplemented:
        return None
    kernels = mok.kernels
    parts = [(pid, xi) for pid, xi in mok._split(x)]
    if any((not torch.is_tensor(xi)) or xi.dim() != 2 or kernels[pid].num_outputs(xi) != xi.shape[0] for pid, xi in parts):
        return None                                   # batched inputs / nested product processes: not covered
    if any(xi.requires_grad for _, xi in parts):
        return None                                   # d/dx through the block matrix: not covered (the caller refuses)
    lay = _Layout([xi for _, xi in parts])
    for i, (pi, _) in enumerate(parts):
        for j in range(i + 1):
            kern = kernels[pi] if i == j else kernels[pi, parts[j][0]]
            groups = _k._map_groups(kern) if isinstance(kern, _k.Kernel) else None
            if groups is None:
                return None
            for kg, imap_x, imap_y in groups:            # block (i, j) = sum_g k_g(imap_x(x_i), imap_y(x_j))
                rows = kg.tensor_table()
                if rows is None or (i == j and not _k._same_map(imap_x, imap_y)):
                    return None
                # (a diagonal block sees both arguments through the same map: ONE mapped input, which moves both at once)
                lay.add("K", i, j, rows, 1.0, i, j, imap_x, imap_x if i == j else imap_y)
    if not (any(t.requires_grad for t in lay.params + lay.us) or r.requires_grad or (noise_vec is not None and noise_vec.requires_grad)):
        return None
    for u in lay.us:
        if u.requires_grad:
            _ag.check_input_dims(u)
    build = functools.partial(mok.pairwise, x, None, lower=True, diag_add=config.epsilon, diag_vec=noise_vec)
    return _ag.joint_logpdf(r, noise_vec, build, tuple(xi.shape[0] for _, xi in parts), tuple(lay.blocks), lay.us, lay.params)


# ---- the pseudo-point bound ------------------------------------------------------------
def requested(obs, measure):
    """Whether anything the bound depends on carries a gradient (kernel hyper-parameters, noise, inducing inputs, y)."""
    p_x, x, noise_x = obs.fdd.p, obs.fdd._xr, obs.fdd.noise
    z = obs.u._xr
    k = measure.kernels[obs.u.p]
    view = k.input_scaled_view() if hasattr(k, "input_scaled_view") else None
    if view is None or isinstance(x, _k.MultiInput) or isinstance(z, _k.MultiInput) or not isinstance(noise_x, Diagonal):
        return kernel_requires_grad(k) or obs.y.requires_grad
    return (groups_need_grad([(view[0], x)], noise_x.diag(), z, obs.y - measure.means[p_x](x))
            or any(m is not None and m.requires_grad for m in view[1:]))


def elbo(obs, measure):
    """The VFE / FITC / DTC bound of the pseudo-point observations ``obs`` as a node of the graph (``autograd.sparse_elbo``); None when
    nothing it depends on carries a gradient, or with grad off."""
    if not torch.is_grad_enabled():
        return None
    p_x, x, noise_x = obs.fdd.p, obs.fdd._xr, obs.fdd.noise
    p_z, z, noise_z = obs.u.p, obs.u._xr, obs.u.noise
    refuse_fn_scaled("the pseudo-point bound", (measure.kernels[p_z], measure.kernels[p_x], measure.kernels[p_z, p_x]), x,
                     z if torch.is_tensor(z) else None, obs.y, noise_x.diag() if isinstance(noise_x, Diagonal) else None)
    if isinstance(x, _k.MultiInput) or isinstance(z, _k.MultiInput) or not isinstance(noise_x, Diagonal):
        return None
    k = measure.kernels[p_z]
    if _k.has_per_batch(k):
        raise NotImplementedError(f"inducing points and the pseudo-point bound are not implemented with {_k.PER_BATCH}")
    view = k.input_scaled_view()
    if view is None or not _k._same_map(view[1], view[2]):
        return None
    kern, imap, _ = view                      # k(a, b) = kern(imap(a), imap(b))
    y_bar = obs.y - measure.means[p_x](x)
    need = groups_need_grad([(kern, x)], noise_x.diag(), z, y_bar) or (imap is not None and imap.requires_grad)
    if not need and p_x is not p_z:
        # data on a process mapped from the inducing points' one (`g = f.shift(tau)`, `f.transform(net)`): a learnable map sits in
        # the data's kernel and in the cross-kernel only -- outside this path, and refused below rather than detached
        need = any(m is not None and m.requires_grad for other in (measure.kernels[p_x], measure.kernels[p_z, p_x])
                   for g in (_k._map_groups(other) or []) for m in g[1:])
    if not need:
        return None
    if not (measure.kernels[p_x] is k and measure.kernels[p_z, p_x] is k and isinstance(noise_z, Zero) and x.dim() == 2 and z.dim() == 2):
        raise NotImplementedError("gradients of the bound are implemented for noise-free inducing points of the observed "
                                  "process itself (one kernel that is a sum of primitives), unbatched")
    if imap is not None:                      # torch differentiates the map (d/d scales or period, d/dx, d/dz)
        x, z = imap(x), imap(z)
    if x.requires_grad:
        _ag.check_input_dims(x)
    return _ag.sparse_elbo(kern, x, z, noise_x.diag(), y_bar, obs.method)
