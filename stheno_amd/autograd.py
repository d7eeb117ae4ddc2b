"""Differentiable ``f(x, noise).logpdf(y)`` -- row 8(f)-1 of SURVEY.md: the dominant use of
``stheno.torch`` is hyper-parameter learning (``readme_example13_optimisation_torch.py:47-53``).

Forward: the same HIP path as the plain logpdf (fused kernel matrix, in-place Cholesky, GEMV
sweep).  Backward, from the stored factor:

    G = d logpdf / dK = 1/2 (A diag(g) A^T - sum(g) K^{-1}),     A = K^{-1} (y - m)

``K^{-1} = W^T W`` with ``W = L^{-1}`` (blocked TRSM on the identity + lower SYRK, both on the
MFMA GEMM), then ONE pass over the lower triangle of ``K^{-1}`` (``gpk_kmat_vjp``) yields the
gradients w.r.t. every variance, length scale and the noise; ``d/d(y - m) = -A g``.
Gradients w.r.t. the inputs ``x`` (learnt input warps, latent inputs, per-dimension length scales --
``k.stretch(vector)`` divides the inputs) take one more pass: the explicit symmetric cotangent
``G`` is formed in the buffer of ``K^{-1}`` (a rank-C GEMM update) and ``gpk_kmat_vjp_dense`` reduces it
against ``dK_ij/dx_i``; both arguments of ``k(x, x)`` move with ``x``, hence the factor two.

A kernel enters every function here as GROUPS of terms that see the same inputs (``Kernel`` objects taken apart by ``kernels._map_groups``): ``k(x, y) = sum_g
k_g(u_g(x), u_g(y))`` with ``k_g`` a sum of primitives and ``u_g`` a differentiable map of the inputs (none, the division by
per-dimension length scales, the periodic embedding), formed in torch by the caller.  The cotangent of ``K`` is the same for every group;
the reductions against it run once per group, on that group's term table and mapped inputs, and each group's input gradient goes back to
torch, which carries it through the map to its parameter and to ``x``.  One group is the plain case: the same launches as ever.

A stage that several functions share is written once, as a plain function in front of its first user: the tail of every log-density
forward (``_density``); the pieces of its backward (``_inverse_parts``, ``_cotangent``, ``_grad_inputs``); the cotangents the
posterior-marginal backwards start from (``_output_cotangents``, ``_posterior_cotangents``) and their reduction through ``k(x, xs)``
(``_through_cross``), for one posterior or a batch alike; the rank-two update of an explicit cotangent (``_rank_two_``); the walk over
the blocks of several processes (``_walk_blocks``); and the way from the per-term sums to the parameters' gradients (``_param_grads``,
``_sum_param_grads``).  A group between one function on both sides (``f * fn``) is a case of ``_GPLogpdf``, not a function of its own.

The posterior marginals (``post(xs).mean`` / ``.var_diag`` / ``.marginals()`` / ``.marginal_credible_bounds()``) have three functions
further down: ``_PosteriorMarginals`` (an exact posterior of one process predicted from its own observations; a batch of them under
shared hyper-parameters: ``_BatchedPosteriorMarginals``, every reduction one ``gpk_kmat_vjp_dense_batch`` launch), ``_BlockPosteriorMarginals``
(one exact conditioning step ACROSS processes: a component of a sum, several observed processes, derivatives -- the blocks are sums of
groups ``s D^(a, b) k_g(u_g(x), u_g(y))``, ``learnable._block_groups``, and a derivative group's cotangent is reduced by
``gpk_kmat_diff_vjp``) and ``_SparsePosteriorMarginals`` (pseudo-point posteriors).  Each runs the plain path as its forward, so the
values are that path's bits, and derives everything else from the stored factors.  The JOINT covariance of the first case
(``post(xs).var``) is ``_PosteriorCovariance`` at the end of the module, with the differentiable factorisation (``_FactorTimes``, on
``gpk_potrf_vjp``) and log-determinant (``_LogdetSPD``) that ``Normal.sample`` / ``Normal.entropy`` take for a covariance inside the graph.

This module holds the maths on ``libgpk`` launches and the packing of a kernel into a function's arguments; it imports nothing from
``kernels``.  Whether a call is in a covered case (groups, mapped inputs, dimension checks, dispatch, plain path or refusal) is decided in
``stheno_amd/learnable.py``, which calls the thin ``apply`` wrappers here.
"""
import collections
import itertools
import math

import torch

from . import ops
from .matrix import LOG_2_PI, Chol, config

__all__ = ["gp_logpdf", "joint_logpdf", "sparse_elbo", "posterior_marginals", "block_posterior_marginals", "sparse_posterior_marginals",
           "posterior_covariance", "add_diagonal", "factor_times", "logdet_spd"]


# Hyper-parameters travel through the autograd functions as one flat list of scalar tensors: the variances, then the scales and --
# only when a term has a shape parameter (RQ's alpha, Delta's epsilon) -- one more entry per term behind them (a constant 0 for the
# kinds without).  Only RQ's is learnable: Delta is piecewise constant in its epsilon, whose gradient entry is None.
def _as_t(v):
    return v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)


def _pack(rows):
    """``(kinds, params)`` of a term table in its tensor view (``Kernel.tensor_table()``: rows ``(kind, variance, scale, shape)``)."""
    kinds = tuple(row[0] for row in rows)
    params = [_as_t(v) for _, v, _, _ in rows] + [_as_t(s) for _, _, s, _ in rows]
    if any(a is not None for _, _, _, a in rows):
        for k, _, _, a in rows:
            if k not in ops._LEARNABLE_SHAPE and torch.is_tensor(a) and a.requires_grad:
                raise ValueError(f"the shape parameter of a {k!r} term is not learnable")
        params += [_as_t(0.0 if a is None else a) for _, _, _, a in rows]
    return kinds, params


def _pack_groups(kernels):
    """``(layout, params)`` of the groups' kernels: ``layout`` = one ``(kinds, number of parameters)`` per group, ``params`` = the flat
    parameter lists (``_pack``) group after group."""
    layout, params = [], []
    for kern in kernels:
        kinds, pr = _pack(kern.tensor_table())
        layout.append((kinds, len(pr)))
        params.extend(pr)
    return tuple(layout), params


#: one group inside an autograd function: its kinds, the host descriptor for the fused kernels and the parameters' values (``_unpack``),
#: the parameters' ``(device, dtype)`` and the group's input tensors
_Group = collections.namedtuple("_Group", "kinds terms values meta inputs")


def _split_groups(layout, tensors, per_group=1):
    """The tensors behind ``layout`` in an autograd function's arguments: ``per_group`` input tensors per group first, then the flat
    parameters group after group.  Returns one ``_Group`` per group."""
    pos = per_group * len(layout)
    out = []
    for i, (kinds, npar) in enumerate(layout):
        params = tensors[pos: pos + npar]
        out.append(_Group(kinds, *_unpack(kinds, params), [(p.device, p.dtype) for p in params], tensors[per_group * i: per_group * (i + 1)]))
        pos += npar
    return out


def check_input_dims(u):
    """The input-gradient kernels cover at most 8 input dimensions (as the fused kernels see them: behind a periodic map, twice)."""
    if u.shape[-1] > 8:
        raise NotImplementedError("gradients with respect to the inputs (or per-dimension length scales) "
                                  "are implemented for at most 8 input dimensions")


def _unpack(kinds, params):
    """``(terms, values)``: the host descriptor for the fused kernels and the parameters' values
    ``(variances, scales, alphas or None)`` as floats.  A parameter that comes once per batch entry (a ``(B, 1, 1)`` tensor) stays on the
    device, as a detached fp64 vector ``(B,)``, in the descriptor (``ops.KTerms``, per batch) and in the values."""
    nt = len(kinds)
    vals = [p.detach().reshape(-1).to(torch.float64) if torch.is_tensor(p) and p.numel() > 1 else float(p) for p in params]
    variances, scales = vals[:nt], vals[nt:2 * nt]
    alphas = vals[2 * nt:3 * nt] if len(params) > 2 * nt else None
    shapes = None if alphas is None else [a if k in ops._SHAPED else None for k, a in zip(kinds, alphas)]
    return ops.KTerms(list(zip(kinds, variances, scales)), shapes), (variances, scales, alphas)


def _param_grads_per_batch(kinds, values, S, meta, shapes):
    """``_param_grads`` from one row of sums PER BATCH ENTRY, ``S`` (B, nt, 2 or 3), entry b's taken with entry b's parameters: a
    per-batch parameter (``shapes``: the parameters' shapes) gets entry b's gradient at index b, a scalar one the sum over the batch."""
    variances, scales, alphas = values
    nt = len(kinds)
    on = lambda v: v.to(device=S.device, dtype=S.dtype) if torch.is_tensor(v) else v      # noqa: E731
    gr = [S[:, t, 0] for t in range(nt)] + [-2.0 * on(variances[t]) / on(scales[t]) * S[:, t, 1] for t in range(nt)]
    if alphas is not None:
        gr += [(on(variances[t]) * S[:, t, 2]) if kinds[t] in ops._LEARNABLE_SHAPE else None for t in range(nt)]
    out = []
    for g_, (dev, dt), shape in zip(gr, meta, shapes):
        if g_ is not None:
            g_ = (g_.reshape(shape) if len(shape) else g_.sum()).to(device=dev, dtype=dt)
        out.append(g_)
    return out


def _param_grads(kinds, values, S, meta, wgt=1.0):
    """Gradients for the flat parameter list from the per-term sums ``S`` (nt, 2 or 3): d/dv_t = S1_t, d/dl_t = -2 v_t S2_t / l_t,
    d/dalpha_t = v_t S3_t (None for the kinds without a shape)."""
    variances, scales, alphas = values
    nt = len(kinds)
    gr = [wgt * S[t, 0] for t in range(nt)] + [wgt * -2.0 * variances[t] / scales[t] * S[t, 1] for t in range(nt)]
    if alphas is not None:
        gr += [(wgt * variances[t] * S[t, 2]) if kinds[t] in ops._LEARNABLE_SHAPE else None for t in range(nt)]
    return [None if g_ is None else g_.to(device=dev, dtype=dt) for g_, (dev, dt) in zip(gr, meta)]


def _sum_param_grads(groups, S):
    """The gradients of the flat parameter list of ``groups`` (``_param_grads``, group after group) from one table of sums per group."""
    grads = []
    for grp, S_g in zip(groups, S):
        grads += _param_grads(grp.kinds, grp.values, S_g, grp.meta)
    return grads


def _density(be, k, r):
    """The tail of every log-density forward: ``k`` (the lower triangle of the covariance, jitter and noise on its diagonal) is factorised
    in place; ``r`` (n, C), or (B, n, 1) against a batch of matrices.  Returns ``(log-densities (C,) or (B,), factor, w = L^{-1} r)``."""
    chol = Chol.factor_(k)
    w = chol.solve(r)                                            # L^{-1} r
    _, ss = be.colreduce(w, want_ss=True)                        # (C,), or (B, 1)
    if r.dim() == 3:
        ss = ss[..., 0]
    return -(chol.logdet() + r.shape[-2] * LOG_2_PI + ss) / 2, chol, w


def _cotangent(be, kinv_lower, alpha, g):
    """``G = d logpdf / dK = 1/2 (alpha diag(g) alpha^T - sum(g) K^{-1})`` as an explicit symmetric (n, n) matrix, formed in the
    buffer of the lower triangle of ``K^{-1}`` (consumed): ``alpha = K^{-1} r`` (n, C), ``g`` the C output cotangents."""
    gt = torch.as_tensor(g, dtype=alpha.dtype, device=alpha.device)
    G = be.symmetrize_(kinv_lower)
    return be.gemm(alpha * gt[None, :], alpha, a_kmajor=True, b_kmajor=True, alpha=0.5, beta=-0.5 * float(sum(g)), out=G)


def _grad_inputs(be, terms, x, G):
    """``d logpdf / dx`` (n, D) from the explicit cotangent: ``dx_i = 2 sum_j G_ij dk(x_i, x_j)/dx_i`` (both arguments of
    ``k(x, x)`` move with ``x``)."""
    check_input_dims(x)
    _, _, gx = be.kmat_vjp_dense(terms, x, x, G, want_gradx=True)
    return 2.0 * gx


def _inverse_parts(be, chol, w):
    """``(W, lower triangle of K^{-1}, alpha)`` from the stored factor and ``w = L^{-1} r`` (n, C): ``W = L^{-1}`` (lower triangular),
    ``K^{-1} = W^T W``, ``alpha = K^{-1} r = W^T w``."""
    W = chol.inverse_lower()                                                             # N^3/3 flops
    kinv = be.gemm(W, W, a_kmajor=False, b_kmajor=False, lower_only=True, tri_k=True)    # N^3/3 flops
    cols = [be.colreduce(W, w[:, c], want_dot=True, want_ss=False)[0] for c in range(w.shape[1])]
    return W, kinv, (cols[0][:, None] if len(cols) == 1 else torch.stack(cols, dim=1))


def _zeros(rows, cols, like):
    """An all-zero (rows, cols) operand read through a zero row stride (no rows x cols buffer): dtype, device and leading batch
    dimension (another zero stride) of ``like``."""
    lead = like.shape[:-2]
    return torch.zeros((1,) * len(lead) + (1, cols), dtype=like.dtype, device=like.device).expand(*lead, rows, cols)


def _rank_two_(be, G, alpha, beta):
    """``G -= 1/2 (beta alpha^T + alpha beta^T)`` in place, as a GEMM of contraction length 2; vectors (n,), or (B, n) against a batch."""
    return be.gemm(torch.stack([beta, alpha], dim=-1), torch.stack([alpha, beta], dim=-1), a_kmajor=True, b_kmajor=True, alpha=-0.5,
                   beta=1.0, out=G)


def _offsets(sizes):
    """The first row of each observation set in the block matrix, and the total behind them."""
    return [0, *itertools.accumulate(sizes)]


#: one group of one block in the layout of ``_JointLogpdf`` / ``_BlockPosteriorMarginals``: ``which`` = ``"K"`` for block ``(i, j)`` of the
#: lower block triangle of the observed covariance, ``"C"`` for the rows of set ``i`` of the cross-covariance; its ``kinds`` and number of
#: parameters (``_pack``); ``ua`` / ``ub``: its row / column inputs among the mapped inputs; ``(a, b)``: its derivative slots, or None
Block = collections.namedtuple("Block", "which i j kinds npar ua ub a b")


def _walk_blocks(be, layout, sizes, values, meta, us, need_u, kbar, cbar=None):
    """One reduction per group and block over the block's view of its cotangent -- ``kbar`` (N, N, explicit and symmetric) for the
    ``"K"`` entries of ``layout``, ``cbar`` (N, N*) for the ``"C"`` ones: ``gpk_kmat_vjp_dense`` for a plain group, ``gpk_kmat_diff_vjp``
    for a derivative group; off-diagonal blocks of ``kbar`` count twice.  A mapped input that requires a gradient gets it from the pass
    where it is the row input and from one more pass over the transposed view, with the derivative slots exchanged, where it is the
    column input; a group that is symmetric in a diagonal block moves both arguments at once, hence twice its one reduction.  Returns
    ``(gradients of the mapped inputs, gradients of the flat parameters)``."""
    offs = _offsets(sizes)
    cbar_t = None
    grads, grad_us, pos = [None] * len(values), [None] * len(us), 0

    def add(a, gx):
        grad_us[a] = gx if grad_us[a] is None else grad_us[a] + gx

    def reduce(terms, x, y, a, b, g, want_gx):
        if a is None and b is None:
            S, _, gx = be.kmat_vjp_dense(terms, x, y, g, want_gradx=want_gx)
            return S, gx
        return be.kmat_diff_vjp(terms, x, y, a, b, g, want_gradx=want_gx)

    for (which, i, j, kinds, npar, ua, ub, a, b) in layout:
        terms, vals = _unpack(kinds, values[pos: pos + npar])
        if which == "K":
            g = kbar[offs[i]: offs[i + 1], offs[j]: offs[j + 1]]
            wgt = 1.0 if i == j else 2.0
        else:
            g = cbar[offs[i]: offs[i + 1], :]
            wgt = 1.0
        S, gx = reduce(terms, us[ua], us[ub], a, b, g, need_u[ua])
        grads[pos: pos + npar] = _param_grads(kinds, vals, S, meta[pos: pos + npar], wgt)
        pos += npar
        symmetric = which == "K" and i == j and ua == ub and a == b
        if need_u[ua]:
            add(ua, (2.0 if symmetric else wgt) * gx)
        if need_u[ub] and not symmetric:
            # the input is the column one: the transposed view (the cotangent of K is symmetric, explicitly), the derivative slots exchanged
            if which == "K":
                gt = kbar[offs[j]: offs[j + 1], offs[i]: offs[i + 1]]
            else:
                if cbar_t is None:
                    cbar_t = cbar.t().contiguous()
                gt = cbar_t[:, offs[i]: offs[i + 1]]
            _, gx = reduce(terms, us[ub], us[ua], b, a, gt, True)
            add(ub, wgt * gx)
    return grad_us, grads


class _GPLogpdf(torch.autograd.Function):
    """The log-density of one process.  A group may stand between one function on both sides, ``K = sum_g diag(s_g) k_g(u_g) diag(s_g)``
    (a group without a function: ``s_g`` absent) -- the kernel of ``(1 + a) * net + b``.  ``s_g = fn(x)`` is formed in torch by the
    caller and is an input here, so the graph carries the gradient on into the function's parameters."""

    @staticmethod
    def forward(ctx, r, noise_vec, noise_mat, layout, scaled, *tensors):
        """``layout`` = one ``(kinds, number of parameters)`` per group of terms; ``scaled``: one bool per group; ``tensors`` = the
        groups' inputs ``u_g`` (n, D_g), then one scale ``s_g`` (n,) per scaled group, then the parameters group after group --
        variances, scales (and shape parameters: ``_pack``; scalar tensors, any device); ``noise_vec`` (n,) or None; ``noise_mat`` (n, n)
        dense noise covariance or None; ``r = y - mean`` (n, C).  Returns (C,)."""
        be = ops.get_backend()
        ng, ns = len(layout), sum(scaled)
        groups = _split_groups(layout, tensors[:ng] + tensors[ng + ns:])
        it = iter(tensors[ng: ng + ns])
        scales = [next(it).detach() if sc else None for sc in scaled]
        k = None
        for grp, s in zip(groups, scales):
            # the first group writes the lower triangle with the (unscaled) diagonal additions, the others add to it (as `Sum.pairwise` does)
            kw = dict(lower=True, diag_add=config.epsilon, diag_vec=noise_vec) if k is None else dict(lower=True, out=k, accumulate=True)
            if s is None:
                k = be.kmat(grp.terms, grp.inputs[0], None, **kw)
            else:
                k = be.kmat_scaled(grp.terms, grp.inputs[0], None, s, s, **kw)
        if noise_mat is not None:
            k += noise_mat                                       # (only the lower triangle is read from here on)
        out, ctx.chol, ctx.w = _density(be, k, r)
        ctx.groups, ctx.scales = groups, scales
        ctx.has_noise, ctx.has_noise_mat = noise_vec is not None, noise_mat is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        be = ops.get_backend()
        chol, w, groups, scales = ctx.chol, ctx.w, ctx.groups, ctx.scales
        n, C = w.shape
        ng = len(groups)
        any_scaled = any(s is not None for s in scales)
        if C > 8:
            raise NotImplementedError("backward through logpdf supports at most 8 columns of y")
        need_u = [ctx.needs_input_grad[5 + i] for i in range(ng)]
        need_nm = ctx.has_noise_mat and ctx.needs_input_grad[2]
        if any_scaled and any(need_u):
            raise NotImplementedError("gradients with respect to the inputs of a function-scaled kernel are not implemented")
        for grp, need in zip(groups, need_u):
            if need:
                check_input_dims(grp.inputs[0])
        g = [float(v) for v in grad_out.reshape(-1).tolist()]    # host sync: C scalars
        _, kinv, alpha = _inverse_parts(be, chol, w)
        # several groups of which one passes a gradient to its inputs: every group reads the explicit cotangent once, its sums and its
        # input gradient out of the same pass -- and so under a scale, where a group has no implicit form; otherwise the implicit form,
        # one pass over the lower triangle of K^{-1} per group
        dense = (ng > 1 and any(need_u)) or any_scaled
        S, grad_us, grad_s, diag_g = [None] * ng, [None] * ng, [], None
        if not dense:
            for i, grp in enumerate(groups):
                S[i], _, dg = be.kmat_vjp(grp.terms, grp.inputs[0], kinv, alpha, g)
                if i == 0:
                    diag_g = dg                                  # (the cotangent's diagonal: the same from every group)
        grad_nm = None
        if dense or any(need_u) or need_nm:
            G = _cotangent(be, kinv, alpha, g)                   # explicit, in the buffer of K^{-1}
            pos = 5 + ng
            for i, (grp, s) in enumerate(zip(groups, scales)):
                u = grp.inputs[0]
                if s is not None:
                    # d/d theta of sum_ij G_ij s_i s_j k_ij: the row factor in the cotangent G_r = diag(s) G, the column factor as `colscale`
                    Gr = G * s[:, None]
                    S[i], _, _ = be.kmat_vjp_dense(grp.terms, u, u, Gr, colscale=s)
                    gs = None
                    if ctx.needs_input_grad[pos]:
                        # d/ds_j = 2 sum_i s_i G_ij k_ij (G and K are symmetric): the column sums of G_r . K -- never a scaled sum
                        # divided by s_j, which may vanish
                        _, colsum, _ = be.kmat_vjp_dense(grp.terms, u, u, Gr, want_colsum=True)
                        gs = 2.0 * colsum
                    grad_s.append(gs)
                    pos += 1
                elif dense:
                    S[i], _, gx = be.kmat_vjp_dense(grp.terms, u, u, G, want_gradx=need_u[i])
                    if need_u[i]:
                        grad_us[i] = 2.0 * gx
                elif need_u[i]:
                    grad_us[i] = _grad_inputs(be, grp.terms, u, G)
            if dense:
                diag_g = torch.diagonal(G).clone()
            if need_nm:
                grad_nm = G                                      # d/d noise matrix: the cotangent of K itself
        grad_r = -(alpha * grad_out.reshape(1, -1).to(alpha.dtype))
        grad_noise = diag_g if ctx.has_noise else None
        return (grad_r, grad_noise, grad_nm, None, None, *grad_us, *grad_s, *_sum_param_grads(groups, S))


def gp_logpdf_scaled(groups, noise_vec, r):
    """Differentiable log-density of ``r`` under ``N(0, sum_g diag(s_g) k_g(u_g) diag(s_g) + diag(noise_vec) + eps I)``; ``groups`` =
    ``[(k_g, u_g, s_g)]`` with ``s_g`` (n,) a torch expression in the graph, or None for a group without a function.  Unbatched."""
    layout, params = _pack_groups([kern for kern, _, _ in groups])
    scaled = tuple(s is not None for _, _, s in groups)
    return _GPLogpdf.apply(r, noise_vec, None, layout, scaled, *[u for _, u, _ in groups], *[s for _, _, s in groups if s is not None], *params)


class _GPLogpdfBatched(torch.autograd.Function):
    """The same for stheno's batched computation (``README.md:744-766``): ``x`` (B, N, D), ``r`` (B, N, 1), optional
    per-point noise (B, N), hyper-parameters SHARED by the B independent GPs -- learning over a batch of data sets
    (the configuration that shards over GPUs).  Forward = the batched HIP path (one launch sequence for all B);
    backward walks the batch: ``K_b^{-1}`` from the stored factor of entry b, one ``gpk_kmat_vjp`` pass, sums over b.

    A hyper-parameter may also come ONCE PER BATCH ENTRY, as a ``(B, 1, 1)`` tensor (restarts, one GP per task, a grid): the forward is
    the same launch sequence on ``gpk_kmat_batch_terms``; the backward evaluates entry b with entry b's parameters and leaves its row of
    sums at index b of such a parameter -- the scalar parameters still get the sum over b."""

    @staticmethod
    def forward(ctx, r, noise_vec, layout, *tensors):
        """``layout`` / ``tensors`` as in ``_GPLogpdf``, ONE group: its inputs ``x`` (B, N, D), then its parameters."""
        be = ops.get_backend()
        (grp,) = _split_groups(layout, tensors)
        k = be.kmat(grp.terms, grp.inputs[0], None, lower=True, diag_add=config.epsilon, diag_vec=noise_vec)
        out, ctx.chol, ctx.w = _density(be, k, r)                # (B,), the batched factor, (B, N, 1)
        ctx.group, ctx.has_noise = grp, noise_vec is not None
        ctx.param_shapes = [tuple(p.shape) for p in tensors[1:]]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        be = ops.get_backend()
        chol, w, grp = ctx.chol, ctx.w, ctx.group
        x, terms = grp.inputs[0], grp.terms
        B = x.shape[0]
        g_host = [float(v) for v in grad_out.reshape(-1).tolist()]            # host sync: B scalars
        S_tot, S_each = None, []
        per_batch = terms.batch is not None
        grad_r = torch.empty_like(w)
        grad_noise = torch.empty(w.shape[:-1], dtype=w.dtype, device=w.device) if ctx.has_noise else None
        grad_x = torch.empty_like(x) if ctx.needs_input_grad[3] else None
        if grad_x is not None and per_batch:
            grad_x = torch.empty(x.shape, dtype=x.dtype, device=x.device)       # (shared inputs arrive as an expanded view: a buffer of its own)
        for b in range(B):
            sl = lambda t: None if t is None else t[b:b + 1]      # noqa: E731
            cb = Chol(chol.l[b], sl(chol.dinv), sl(chol.info))                 # entry b as an unbatched factor (views)
            tb = terms.entry(b)                                                # (the launch's own table, or entry b's)
            _, kinv, alpha = _inverse_parts(be, cb, w[b])
            S, _, diag_g = be.kmat_vjp(tb, x[b], kinv, alpha, [g_host[b]])
            if per_batch:
                S_each.append(S)
            else:
                S_tot = S if S_tot is None else S_tot + S
            grad_r[b] = -alpha * g_host[b]
            if grad_noise is not None:
                grad_noise[b] = diag_g
            if grad_x is not None:
                grad_x[b] = _grad_inputs(be, tb, x[b], _cotangent(be, kinv, alpha, [g_host[b]]))
        if per_batch:
            grads = _param_grads_per_batch(grp.kinds, grp.values, torch.stack(S_each), grp.meta, ctx.param_shapes)
            return (grad_r, grad_noise, None, grad_x, *grads)
        return (grad_r, grad_noise, None, grad_x, *_param_grads(grp.kinds, grp.values, S_tot, grp.meta))


class _JointLogpdf(torch.autograd.Function):
    """Log-density of SEVERAL processes of one measure observed jointly (``measure.logpdf((f1(x1), y1), (f2(x2), y2))``,
    ``f(x).logpdf(y)`` of a product process): the variance is the block matrix of ``MultiOutputKernel``, block (i, j) =
    ``kernels[p_i, p_j](x_i, x_j)``, every block a sum of groups of primitives behind input maps.  Forward = the plain HIP path (blocks
    written into one buffer, factorised in place).  Backward: the explicit cotangent ``G = 1/2 (alpha diag(g) alpha^T - sum(g) K^{-1})``
    once, then one ``gpk_kmat_vjp_dense`` pass per group of every block of the lower block triangle over the block's view of ``G``
    (off-diagonal blocks count twice: ``G`` and the block matrix are symmetric: ``_walk_blocks``).  ``layout`` = one ``Block`` per group,
    all of them ``"K"`` and without derivative slots; the ``nu`` mapped inputs lead ``tensors``; behind
    them the variances, scales (and shape parameters, for a group that has any: ``_pack``) of group after group: autograd carries them
    back to the user's leaves through whatever kernel algebra produced them.  A mapped input that requires a gradient (a learnable
    period, learnable per-dimension scales) gets twice its reduction, as the row input or, mirrored, as the column input."""

    @staticmethod
    def forward(ctx, r, noise_vec, build, sizes, layout, nu, *tensors):
        out, ctx.chol, ctx.w = _density(ops.get_backend(), build(), r)      # (build: lower block triangle + eps + noise on the diagonal)
        params = tensors[nu:]
        ctx.sizes, ctx.layout, ctx.us = sizes, layout, tensors[:nu]
        ctx.has_noise = noise_vec is not None
        ctx.param_meta = [(p.device, p.dtype) for p in params]
        ctx.values = [float(p) for p in params]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        be = ops.get_backend()
        chol, w, us = ctx.chol, ctx.w, ctx.us
        nu = len(us)
        need_u = [ctx.needs_input_grad[6 + a] for a in range(nu)]
        for u, need in zip(us, need_u):
            if need:
                check_input_dims(u)
        g = [float(v) for v in grad_out.reshape(-1).tolist()]    # host sync: C scalars
        _, kinv, alpha = _inverse_parts(be, chol, w)
        G = _cotangent(be, kinv, alpha, g)
        grad_us, grads = _walk_blocks(be, ctx.layout, ctx.sizes, ctx.values, ctx.param_meta, us, need_u, G)
        grad_r = -(alpha * grad_out.reshape(1, -1).to(alpha.dtype)) if ctx.needs_input_grad[0] else None
        grad_noise = torch.diagonal(G).clone() if ctx.has_noise else None
        return (grad_r, grad_noise, None, None, None, None, *grad_us, *grads)


def joint_logpdf(r, noise_vec, build, sizes, layout, us, params):
    """Differentiable log-density of ``_JointLogpdf`` (``learnable.logpdf`` builds the arguments)."""
    return _JointLogpdf.apply(r, noise_vec, build, sizes, layout, len(us), *us, *params)


def gp_logpdf(groups, noise_vec, r, noise_mat=None):
    """Differentiable log-density of ``r = y - m(x)`` under ``N(0, sum_g k_g(u_g) + diag(noise_vec) + noise_mat + eps I)``; ``groups``
    = ``[(k_g, u_g)]``, every ``k_g`` a sum of primitives on its (mapped) inputs ``u_g``.  Batched inputs: one group."""
    layout, params = _pack_groups([kern for kern, _ in groups])
    if groups[0][1].dim() == 3:
        (x,) = [u for _, u in groups]
        return _GPLogpdfBatched.apply(r, noise_vec, layout, x, *params)
    return _GPLogpdf.apply(r, noise_vec, noise_mat, layout, (False,) * len(groups), *[u for _, u in groups], *params)


def _diag_share(grp, x, g_kd, gr, gx, need_x):
    """The share of ``k(x_j, x_j)`` (cotangent ``g_kd`` (N,): the trace term of VFE, FITC's effective noise) in the parameter gradients
    ``gr`` (``_param_grads``' list, updated in place) and in the gradient ``gx`` of the inputs ``x`` (returned; only with ``need_x``):
    a stationary term is its variance there, whatever its scale and shape; a linear term is ``v |x_j|^2 / l^2`` and moves with ``x_j``."""
    kinds, nt = grp.kinds, len(grp.kinds)
    variances, scales, _ = grp.values
    for t in range(nt):
        if kinds[t] == "linear":
            xx = ((x * x).sum(-1) * g_kd).sum() / scales[t] ** 2
            gr[t], gr[nt + t] = gr[t] + xx, gr[nt + t] - 2.0 * variances[t] / scales[t] * xx
            if need_x:
                gx = gx + (2.0 * variances[t] / scales[t] ** 2) * g_kd[:, None] * x
        else:
            gr[t] = gr[t] + g_kd.sum()
    return gx


# ---------------------------------------------------------------------------------------------
# Pseudo-point ELBO (VFE / FITC / DTC), stheno/model/observations.py:279-336, differentiable w.r.t. the
# kernel variances / length scales, the (diagonal) observation noise, the inducing inputs z and
# the residual r = y - m(x).
#
# With K_z = L L^T, V = L^{-1} K_zx, D = diag(noise), A = I + V D^{-1} V^T, c = A^{-1} V D^{-1} r,
# beta = r - V^T c (so Sigma^{-1} r = D^{-1} beta), tau = 1 (VFE) or 0 (DTC):
#     dELBO/dK_zx = L^{-T} [ (tau I - A^{-1}) V + c beta^T ] D^{-1}                  (M x N)
#     dELBO/dK_z  = -1/2 L^{-T} [ tau A - (tau + 1) I + A^{-1} + c c^T ] L^{-1}      (M x M)
#     dELBO/dD_j  = -1/2 [ 1/d_j - ((V^T A^{-1} V)_jj + beta_j^2 + tau (k_jj - q_jj)) / d_j^2 ]
#     dELBO/dk_jj = -tau / (2 d_j),      dELBO/dr = -D^{-1} beta
# The M x N cotangent costs ONE extra MFMA GEMM (2 M^2 N flops) on the stored, whitened and scaled
# V; gpk_kmat_vjp_dense then reads it once and returns the per-term sums, the column sums that
# give (V^T A^{-1} V)_jj without another TRSM, and d/dz.  Everything else is M x M.
# FITC = the DTC bound at the noise d + (k_jj - q_jj); its dependence on V through q_jj adds one M x N GEMM,
# one weighted M x M SYRK and a second pass of gpk_kmat_vjp_dense.
# ---------------------------------------------------------------------------------------------
class _SparseELBO(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, noise_vec, tau, layout, *tensors):
        """``layout`` / ``tensors`` as in ``_PosteriorMarginals``, ONE group: its inputs ``x`` (N, D) and ``z`` (M, D), then its
        parameters; ``tau``: 1 (VFE), 0 (DTC), -1 (FITC)."""
        from .model.observations import _syrk_lower

        be = ops.get_backend()
        (grp,) = _split_groups(layout, tensors, 2)
        (x, z), terms = grp.inputs, grp.terms
        n, m = x.shape[0], z.shape[0]
        d = noise_vec.detach()
        v = be.kmat(terms, z, x)                                               # K_zx
        chol_z = Chol.factor_(be.kmat(terms, z, None, lower=True, diag_add=config.epsilon))
        v = chol_z.solve_(v)                                                   # V
        _, q = be.colreduce(v, want_ss=True)
        corr = be.kdiag(terms, x) - q
        fitc = tau < 0
        if fitc:                     # FITC: the DTC bound with the noise d + (k_jj - q_jj)   (observations.py:312)
            d, tau = d + corr, 0.0
        s = torch.rsqrt(d)
        be.scale_cols_(v, s)                                                   # V D^{-1/2}
        a = torch.zeros((m, m), dtype=x.dtype, device=x.device)
        _syrk_lower(be, v, a)
        be.add_diag_(a, 1.0)
        p = be.gemv(v, r * s[:, None])
        a_fac = be.copy(a)
        if config.epsilon:
            be.add_diag_(a_fac, config.epsilon)
        chol_a = Chol.factor_(a_fac)
        u = chol_a.solve(p)
        _, uu = be.colreduce(u, want_ss=True)
        elbo = -0.5 * (torch.log(2 * math.pi * d).sum() + chol_a.logdet() + (r[:, 0] ** 2 / d).sum() - uu[0]
                       + tau * (corr / d).sum())
        ctx.saved = dict(r=r, d=d, s=s, v=v, q=q, corr=corr, a=a, u=u, chol_z=chol_z, chol_a=chol_a, tau=tau, fitc=fitc)
        ctx.group = grp
        return elbo

    @staticmethod
    def backward(ctx, grad_out):
        be = ops.get_backend()
        sv, grp = ctx.saved, ctx.group
        r, d, s, v, q, corr, tau = sv["r"], sv["d"], sv["s"], sv["v"], sv["q"], sv["corr"], sv["tau"]
        (x, z), terms, kinds = grp.inputs, grp.terms, grp.kinds
        m = z.shape[0]
        eye = torch.eye(m, dtype=x.dtype, device=x.device)
        w_a = sv["chol_a"].inverse_lower()                                     # L_A^{-1}
        a_inv = be.symmetrize_(be.gemm(w_a, w_a, a_kmajor=False, b_kmajor=False, lower_only=True, tri_k=True))
        c = be.colreduce(w_a, sv["u"][:, 0], want_dot=True, want_ss=False)[0]  # A^{-1} p
        vtc = be.colreduce(v, c, want_dot=True, want_ss=False)[0] / s          # V^T c
        beta = r[:, 0] - vtc
        b = beta / d
        w_z = sv["chol_z"].inverse_lower()                                     # L^{-1}
        h = be.gemm(w_z, tau * eye - a_inv, a_kmajor=False, b_kmajor=True)     # L^{-T} (tau I - A^{-1})
        w = be.colreduce(w_z, c, want_dot=True, want_ss=False)[0]              # L^{-T} c
        g_k = be.gemm(h, v, a_kmajor=True, b_kmajor=False)                     # M x N, the one big GEMM
        need_x, need_z = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        fitc = sv["fitc"]
        s_k, colsum, gz_k = be.kmat_vjp_dense(terms, z, x, g_k, colscale=s, w=w, b=b, want_colsum=True,
                                              want_gradx=need_z and not fitc)
        vav = tau * q - d * colsum + vtc * beta                                # (V^T A^{-1} V)_jj
        g_d = -0.5 * (1.0 / d - (vav + beta * beta + tau * corr) / (d * d))
        a_full = be.symmetrize_(be.copy(sv["a"]))
        mid = tau * a_full - (tau + 1.0) * eye + a_inv + c[:, None] * c[None, :]
        if fitc:
            # the effective noise depends on V through q_jj = |V_j|^2:  dELBO/dV -= 2 V diag(g_d), i.e. the
            # cotangent of K_zx gets  -2 (L^{-T} V) diag(g_d)  and the K_z part  -2 V diag(g_d) V^T
            rr = be.gemm(w_z, v, a_kmajor=False, b_kmajor=False)               # L^{-T} V D^{-1/2}   (M x N)
            g_k.addcmul_(rr, (-2.0 * g_d / (s * s))[None, :])
            s_k, _, gz_k = be.kmat_vjp_dense(terms, z, x, g_k, colscale=s, w=w, b=b, want_gradx=need_z)
            rr.copy_(v)
            be.scale_cols_(rr, g_d * d)
            vgv = be.symmetrize_(be.gemm(rr, v, a_kmajor=True, b_kmajor=True, lower_only=True))
            mid = mid - 2.0 * vgv
            del rr
        gx_k = None
        if need_x:
            # d/dx through K_zx: the same reduction with the roles of the arguments swapped, on the explicit N x M
            # transpose of the effective cotangent  g_k diag(s) + w b^T  (one extra N x M buffer, backward only)
            be.scale_cols_(g_k, s)
            g_t = g_k.t().contiguous()
            del g_k
            g_t.addcmul_(b[:, None], w[None, :])
            _, _, gx_k = be.kmat_vjp_dense(terms, x, z, g_t, want_gradx=True)
            del g_t
        else:
            del g_k
        t1 = be.gemm(mid, w_z, a_kmajor=True, b_kmajor=False)
        g_kz = be.gemm(w_z, t1, a_kmajor=False, b_kmajor=False, alpha=-0.5)
        s_kz, _, gz_kz = be.kmat_vjp_dense(terms, z, z, g_kz, want_gradx=need_z)
        S = s_k + s_kz
        # through k(x_j, x_j) (VFE: trace term; FITC: the effective noise): stationary terms are constant there
        g_kd = g_d if fitc else -0.5 * tau / d
        go = grad_out.to(x.dtype)
        # through the kernel matrices: the sums' own formulas, left where they were computed -- the diagonal's share is added term by
        # term BEFORE the output cotangent multiplies (the order the sums have always been taken in)
        gr = _param_grads(kinds, grp.values, S, [(S.device, S.dtype)] * len(grp.meta))
        if tau or fitc:
            gx_k = _diag_share(grp, x, g_kd, gr, gx_k, need_x)
        grads = [None if g_ is None else (g_ * go).to(device=dev, dtype=dt) for g_, (dev, dt) in zip(gr, grp.meta)]
        grad_z = (gz_k + 2.0 * gz_kz) * go if need_z else None
        grad_x = gx_k * go if need_x else None
        grad_r = (-b * go)[:, None] if ctx.needs_input_grad[0] else None
        grad_noise = g_d * go if ctx.needs_input_grad[1] else None
        return (grad_r, grad_noise, None, None, grad_x, grad_z, *grads)


def _check_method(method):
    if method not in ("vfe", "fitc", "dtc"):
        raise ValueError(f'Invalid approximation method "{method}".')


def sparse_elbo(kernel, x, z, noise_vec, r, method):
    """Differentiable VFE / FITC / DTC bound for ``r = y - m(x)`` with inducing inputs ``z``."""
    _check_method(method)
    layout, params = _pack_groups([kernel])
    return _SparseELBO.apply(r, noise_vec, {"vfe": 1.0, "dtc": 0.0, "fitc": -1.0}[method], layout, x, z, *params)


# ---------------------------------------------------------------------------------------------
# Posterior marginals of an exact posterior of ONE process, f | (f(x, noise), y) evaluated at test inputs xs: the latent mean
# part and the variance reduction, differentiable w.r.t. the kernel variances / length scales, the noise, r = y - m(x), the
# inputs x and the test inputs xs (observations.py:148-168 through lab/torch in the reference).
#
# K = k(x, x) + noise + eps I = L L^T,  V = L^{-1} k(x, xs) (N x N*),  w = L^{-1} r,  alpha = L^{-T} w = K^{-1} r,
# B = L^{-T} V = K^{-1} k(x, xs).  Outputs: mu = V^T w (the mean minus m(xs)) and s_j = |V_j|^2 (k(xs_j, xs_j) minus the marginal
# variance); the caller adds m(xs) and k(xs, xs) in torch.  With the cotangents gm of mu and gs of s (gs = -g_var):
#     beta         = B gm                    (gs == 0: L^{-T} (V gm), one single-column back-substitution, no N x N* solve)
#     dL/dk(x, xs) = alpha gm^T + 2 B diag(gs)                                    (N x N*)
#     dL/dK        = -B diag(gs) B^T - 1/2 (beta alpha^T + alpha beta^T)        (N x N, symmetric; its diagonal: d/dnoise)
#     dL/dr        = beta
# The cross cotangent is reduced by gpk_kmat_vjp_dense on (x, xs): the rank-1 part rides in its w / b operands, 2 diag(gs) in its
# colscale; d/dxs takes the same reduction on (xs, x) over the explicit transpose (_through_cross).  dL/dK is reduced by gpk_kmat_vjp in its own form
# 1/2 (A diag(g) A^T - sum(g) S) with S = B diag(gs) B^T (ONE lower SYRK on the MFMA GEMM), A = [alpha + beta, alpha - beta, 0],
# g = [-1/2, 1/2, 2] (the rank-2 part as a difference of squares); d/dx through K takes the explicit symmetric cotangent
# (gpk_kmat_vjp_dense, x 2, as in the log-density).  The one new operation is the back-substitution with the transposed factor,
# gpk_trsm_lower_t / gpk_trsv_lower_t: N^2 N* flops for B against N^3/3 for an explicit inverse.
# ---------------------------------------------------------------------------------------------
def _output_cotangents(g_mu, g_s, has_mu, has_s, dt):
    """``(gm, gs)``: the cotangents of the two outputs of a posterior-marginals function in the path's dtype, None for an output that has
    none or that the forward returned as zeros (``has_mu`` / ``has_s``) -- ``gs`` also when it is all zero (one host read): a loss of the
    mean only."""
    gm = g_mu.to(dt).contiguous() if (g_mu is not None and has_mu) else None
    gs = g_s.to(dt).contiguous() if (g_s is not None and has_s) else None
    if gs is not None and not bool(torch.any(gs != 0)):
        gs = None
    return gm, gs


def _posterior_cotangents(be, ctx, g_mu, g_s, dt, dims=()):
    """What the backward of the exact posterior marginals starts from, one process, a batch of them or several processes:
    ``(gm, gs, alpha, bm, beta)`` -- the cotangents of ``mu`` and ``s`` (``_output_cotangents``), ``alpha = K^{-1} r``, ``bm = B = L^{-T} V``
    (only with ``gs``: the N x N* back-substitution) and ``beta = B gm`` (without ``gs``: one single-column back-substitution) -- or None
    when neither output has a cotangent.  With the batched factor every one of them has the leading batch dimension and each solve is ONE
    batched launch.  ``dims``: the inputs whose gradient is wanted (``check_input_dims`` behind that answer, in front of the first launch)."""
    chol, v = ctx.chol, ctx.v
    gm, gs = _output_cotangents(g_mu, g_s, ctx.has_r, True, dt)
    if gm is None and gs is None:
        return None
    for u in dims:
        check_input_dims(u)
    transposed = hasattr(v, "zt")                                 # (the rows that rode through the factorisation: V^T; never a batch)
    alpha = chol.solve_t(ctx.w)[..., 0] if gm is not None else None  # K^{-1} r
    bm = beta = None
    if gs is not None:
        # B = L^{-T} V: the N x N* back-substitution (its right-hand side is a private copy: the solve uses it up)
        bm = chol.solve_t_(v.plain() if transposed else be.copy(v))
        if gm is not None:
            beta = be.gemv(bm, gm[..., None])[..., 0]
    else:
        vg = be.colreduce(v.zt, gm, want_dot=True, want_ss=False)[0] if transposed else be.gemv(v, gm[..., None])[..., 0]
        beta = chol.solve_t(vg[..., None])[..., 0]
    return gm, gs, alpha, bm, beta


def _marginals_forward(ctx, r, noise_vec, run, layout, tensors):
    """The forward of ``_PosteriorMarginals`` and ``_BatchedPosteriorMarginals``: the plain path ``run()`` and what the backward keeps."""
    chol, w, v, mu, s = run()
    ctx.groups = _split_groups(layout, tensors, 2)
    ctx.chol, ctx.w, ctx.v = chol, w, v
    ctx.has_noise, ctx.has_r = noise_vec is not None, r is not None
    ctx.set_materialize_grads(False)
    if mu is None:
        mu = torch.zeros_like(s)
    return mu, s


def _through_cross(be, groups, bm, cs, alpha, gm, need_x, need_xs):
    """The cotangent ``alpha gm^T + B diag(cs)`` of ``k(x, xs)``, the same for every group, reduced per group on (x, xs) -- the rank-one
    part in ``w`` / ``b``, ``cs = 2 gs`` in ``colscale``, ``B`` absent (``bm`` None): a zero operand of zero stride -- and, for ``d/dxs``,
    on (xs, x) over the explicit transpose.  ``gpk_kmat_vjp_dense``, or ONE ``gpk_kmat_vjp_dense_batch`` launch over all entries for
    batched inputs.  Returns ``(S, grad_x, grad_xs)``, one entry per group."""
    ng = len(groups)
    x0, xs0 = groups[0].inputs
    n, ns = x0.shape[-2], xs0.shape[-2]
    reduce = be.kmat_vjp_dense_batch if x0.dim() == 3 else be.kmat_vjp_dense
    S, grad_x, grad_xs = [None] * ng, [None] * ng, [None] * ng
    g_t = None
    for i, grp in enumerate(groups):
        terms, (x, xs) = grp.terms, grp.inputs
        S[i], _, grad_x[i] = reduce(terms, x, xs, bm if bm is not None else _zeros(n, ns, x0), colscale=cs, w=alpha, b=gm, want_gradx=need_x[i])
        if need_xs[i]:
            if g_t is None:
                if bm is not None:
                    g_t = be.scale_cols_(be.copy(bm), cs).transpose(-1, -2).contiguous()      # (N*, N): diag(cs) B^T, explicit
                else:
                    g_t = _zeros(ns, n, x0)
            _, _, grad_xs[i] = reduce(terms, xs, x, g_t, w=gm, b=alpha, want_gradx=True)
    return S, grad_x, grad_xs


class _PosteriorMarginals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, noise_vec, run, layout, *tensors):
        """``run()`` -> ``(chol, w, v, mu, s)``: the plain HIP path of the posterior (``learnable._posterior_parts``: the factor a
        preceding log-density left, or the one whose factorisation carried the cross-covariance as rows under the matrix); ``v`` is
        ``L^{-1} k(x, xs)`` (N, N*) or its transpose as a ``WhitenedT``.  ``layout`` = one ``(kinds, number of parameters)`` per group of
        terms; ``tensors`` = per group ``x`` / ``xs`` as its fused kernels see them (behind the group's input map), then the groups'
        parameters; ``r`` (N, 1) or None (marginal variances only: ``mu`` comes back as zeros)."""
        return _marginals_forward(ctx, r, noise_vec, run, layout, tensors)

    @staticmethod
    def backward(ctx, g_mu, g_s):
        be = ops.get_backend()
        groups = ctx.groups
        ng = len(groups)
        x0 = groups[0].inputs[0]
        n = x0.shape[0]
        dt, dev = x0.dtype, x0.device
        need_x = [ctx.needs_input_grad[4 + 2 * i] for i in range(ng)]
        need_xs = [ctx.needs_input_grad[5 + 2 * i] for i in range(ng)]
        pre = _posterior_cotangents(be, ctx, g_mu, g_s, dt, [grp.inputs[0] for grp, nx, nxs in zip(groups, need_x, need_xs) if nx or nxs])
        if pre is None:
            return (None,) * (4 + 2 * ng + sum(len(grp.meta) for grp in groups))
        gm, gs, alpha, bm, beta = pre
        S, grad_x, grad_xs = _through_cross(be, groups, bm, 2.0 * gs if gs is not None else None, alpha, gm, need_x, need_xs)
        # through K: -B diag(gs) B^T - 1/2 (beta alpha^T + alpha beta^T) = 1/2 (A diag(g) A^T - sum(g) S)
        cols, g = [], []
        if gm is not None:
            cols += [alpha + beta, alpha - beta]
            g += [-0.5, 0.5]
        if bm is not None:
            bs = be.copy(bm)
            be.scale_cols_(bs, gs)
            kinv = be.gemm(bs, bm, a_kmajor=True, b_kmajor=True, lower_only=True)      # S = B diag(gs) B^T (lower triangle)
            del bs, bm
            cols.append(torch.zeros_like(x0[:, 0]))
            g.append(2.0)
        else:
            kinv = _zeros(n, n, x0)
        A = torch.stack(cols, dim=1)
        diag_g = None
        for i, grp in enumerate(groups):
            S_k, _, dg = be.kmat_vjp(grp.terms, grp.inputs[0], kinv, A, g)
            S[i] = S[i] + S_k
            if i == 0:
                diag_g = dg                                           # (the cotangent's diagonal: the same from every group)
        if any(need_x):
            if kinv.stride(0) == 0:
                kinv = torch.zeros((n, n), dtype=dt, device=dev)
            G = _cotangent(be, kinv, A, g)                            # once, in the buffer of S
            for i, grp in enumerate(groups):
                if need_x[i]:
                    grad_x[i] = grad_x[i] + _grad_inputs(be, grp.terms, grp.inputs[0], G)
        grad_r = beta[:, None] if (beta is not None and ctx.needs_input_grad[0]) else None
        grad_noise = diag_g if (ctx.has_noise and ctx.needs_input_grad[1]) else None
        inputs = [t for pair in zip(grad_x, grad_xs) for t in pair]
        return (grad_r, grad_noise, None, None, *inputs, *_sum_param_grads(groups, S))


# ---------------------------------------------------------------------------------------------
# The same for a BATCH of independent exact posteriors under SHARED hyper-parameters: x (B, N, D), xs (B, N*, D), r (B, N, 1), noise
# (B, N) -- a held-out predictive loss over B tasks, B acquisition ascents at once.  The forward is the plain batched path as it is; the
# backward is the algebra above for all entries at once, in the same two functions (_posterior_cotangents, _through_cross) on the batched
# factor: one batched back-substitution for B = L^{-T} V (or, for a loss of the mean only, one single-column one for beta), and every
# reduction against a kernel matrix one launch of gpk_kmat_vjp_dense_batch over all entries -- on (x, xs) with the rank-one part in
# w / b and 2 gs in colscale, on (xs, x) over the explicit transpose for d/dxs, and, the one stage of its own, on (x, x) over the
# explicit symmetric cotangent of K,
#     G = -B diag(gs) B^T - 1/2 (beta alpha^T + alpha beta^T)
# (one batched lower GEMM, gpk_symmetrize, and the rank-two part as a GEMM of contraction length 2: _rank_two_), whose diagonal is d/dnoise and
# whose input gradient counts twice.  The launch gives the sums per entry; the parameters are shared, so their gradients come from the
# sum over the batch.  The number of backend calls does not depend on B.
# ---------------------------------------------------------------------------------------------
class _BatchedPosteriorMarginals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, noise_vec, run, layout, *tensors):
        """As ``_PosteriorMarginals.forward``, every tensor with a leading batch dimension: ``run()`` -> ``(chol, w, v, mu, s)`` with the
        batched factor, ``w`` (B, N, 1), ``v`` (B, N, N*), ``mu`` / ``s`` (B, N*); per group ``x`` (B, N, D_g) / ``xs`` (B, N*, D_g)."""
        return _marginals_forward(ctx, r, noise_vec, run, layout, tensors)

    @staticmethod
    def backward(ctx, g_mu, g_s):
        be = ops.get_backend()
        groups = ctx.groups
        ng = len(groups)
        x0 = groups[0].inputs[0]
        nb, n = x0.shape[:2]
        need_x = [ctx.needs_input_grad[4 + 2 * i] for i in range(ng)]
        need_xs = [ctx.needs_input_grad[5 + 2 * i] for i in range(ng)]
        pre = _posterior_cotangents(be, ctx, g_mu, g_s, x0.dtype, [grp.inputs[0] for grp, nx, nxs in zip(groups, need_x, need_xs) if nx or nxs])
        if pre is None:
            return (None,) * (4 + 2 * ng + sum(len(grp.meta) for grp in groups))
        gm, gs, alpha, bm, beta = pre                            # (B, N*), (B, N*), (B, N), (B, N, N*), (B, N)
        S, grad_x, grad_xs = _through_cross(be, groups, bm, 2.0 * gs if gs is not None else None, alpha, gm, need_x, need_xs)
        # through K: the explicit symmetric cotangent, once
        if bm is not None:
            bs = be.scale_cols_(be.copy(bm), gs)
            G = be.symmetrize_(be.gemm(bs, bm, a_kmajor=True, b_kmajor=True, alpha=-1.0, lower_only=True))
            del bs, bm
        else:
            G = torch.zeros((nb, n, n), dtype=x0.dtype, device=x0.device)
        if gm is not None:
            _rank_two_(be, G, alpha, beta)
        for i, grp in enumerate(groups):
            u = grp.inputs[0]
            S_k, _, gx = be.kmat_vjp_dense_batch(grp.terms, u, u, G, want_gradx=need_x[i])
            S[i] = S[i] + S_k
            if need_x[i]:
                grad_x[i] = grad_x[i] + 2.0 * gx                       # (both arguments of k(x, x) move with x)
        grad_r = beta[..., None] if (beta is not None and ctx.needs_input_grad[0]) else None
        grad_noise = torch.diagonal(G, dim1=-2, dim2=-1).clone() if (ctx.has_noise and ctx.needs_input_grad[1]) else None
        inputs = [t for pair in zip(grad_x, grad_xs) for t in pair]
        return (grad_r, grad_noise, None, None, *inputs, *_sum_param_grads(groups, [S_g.sum(0) for S_g in S]))      # (shared by the batch)


# ---------------------------------------------------------------------------------------------
# Posterior marginals ACROSS processes: one exact conditioning step on one or several observation sets, any one process p of the
# measure predicted at xs -- a component of a sum, another observed process, a derivative (`post(f.diff())`), or values predicted from
# observed slopes.  K is the block matrix of the observed processes (MultiOutputKernel), C = K(x_obs, xs) the stacked cross-covariances
# with p; every block is a sum of groups s D^(a, b) k_g(u_g(x), u_g(y)) (learnable._block_groups), (a, b) the derivative slots of a
# DiffKernel, both None for a plain group.  Forward: the plain path, as it is.  Backward, from the stored factor and V = L^{-1} C, with
# B = L^{-T} V, alpha = K^{-1} r, beta = B gm (the same algebra as above):
#     dL/dC = alpha gm^T + 2 B diag(gs)                                   (N x N*, explicit)
#     dL/dK = -B diag(gs) B^T - 1/2 (beta alpha^T + alpha beta^T)         (N x N, explicit and symmetric; its diagonal: d/dnoise)
#     dL/dr = beta
# -- one gpk_trsm_lower_t and one N x N x N* GEMM (the rank-one and rank-two parts are GEMMs of contraction length 1 and 2) -- and then
# one reduction per group and block over the block's view of either cotangent (_walk_blocks), which also gives a mapped input that
# requires a gradient (the test inputs, a learnable period, ...) its own.  The one-sided derivative blocks have an input gradient
# (d <= 8), the mixed block has none: the caller refuses that before anything is launched.
# ---------------------------------------------------------------------------------------------
class _BlockPosteriorMarginals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, noise_vec, run, sizes, layout, nu, *tensors):
        """``run()`` -> ``(chol, w, v, mu, s)`` as for ``_PosteriorMarginals``; ``sizes``: the rows of each observation set; ``layout``:
        one ``Block`` per group; the ``nu`` mapped inputs lead ``tensors``, behind them the groups' parameters (``_pack``; the group's
        factor is in the variances)."""
        chol, w, v, mu, s = run()
        params = tensors[nu:]
        ctx.chol, ctx.w, ctx.v, ctx.sizes, ctx.layout, ctx.us = chol, w, v, sizes, layout, tensors[:nu]
        ctx.has_noise, ctx.has_r = noise_vec is not None, r is not None
        ctx.param_meta = [(p.device, p.dtype) for p in params]
        ctx.values = [float(p) for p in params]
        ctx.set_materialize_grads(False)
        if mu is None:
            mu = torch.zeros_like(s)
        return mu, s

    @staticmethod
    def backward(ctx, g_mu, g_s):
        be = ops.get_backend()
        us = ctx.us
        nu = len(us)
        dt, dev = us[0].dtype, us[0].device
        pre = _posterior_cotangents(be, ctx, g_mu, g_s, dt)
        if pre is None:
            return (None,) * (6 + nu + len(ctx.values))
        gm, gs, alpha, bm, beta = pre
        need_u = [ctx.needs_input_grad[6 + a] for a in range(nu)]
        n = sum(ctx.sizes)
        ns = gm.shape[0] if gm is not None else gs.shape[0]
        # the two cotangents, explicit
        if bm is not None:
            cbar = be.copy(bm)
            be.scale_cols_(cbar, 2.0 * gs)
            bs = be.copy(bm)
            be.scale_cols_(bs, gs)
            kbar = be.gemm(bs, bm, a_kmajor=True, b_kmajor=True, alpha=-1.0)
            del bs, bm
        else:
            cbar = torch.zeros((n, ns), dtype=dt, device=dev)
            kbar = torch.zeros((n, n), dtype=dt, device=dev)
        if gm is not None:
            be.gemm(alpha[:, None].contiguous(), gm[:, None].contiguous(), a_kmajor=True, b_kmajor=True, alpha=1.0, beta=1.0, out=cbar)
            _rank_two_(be, kbar, alpha, beta)
        grad_us, grads = _walk_blocks(be, ctx.layout, ctx.sizes, ctx.values, ctx.param_meta, us, need_u, kbar, cbar)
        grad_r = beta[:, None] if (beta is not None and ctx.has_r and ctx.needs_input_grad[0]) else None
        grad_noise = torch.diagonal(kbar).clone() if (ctx.has_noise and ctx.needs_input_grad[1]) else None
        return (grad_r, grad_noise, None, None, None, None, *grad_us, *grads)


def block_posterior_marginals(r, noise_vec, run, sizes, layout, us, params):
    """Differentiable ``(mu, s)`` of ``_BlockPosteriorMarginals`` (``learnable._block_marginals`` builds the arguments)."""
    return _BlockPosteriorMarginals.apply(r, noise_vec, run, sizes, layout, len(us), *us, *params)


# ---------------------------------------------------------------------------------------------
# Posterior marginals of a PSEUDO-POINT posterior (VFE / FITC / DTC; observations.py:255-336), f | PseudoObs(f(z), f(x, noise), y)
# evaluated at test inputs xs, differentiable w.r.t. the kernel parameters, the noise, r = y - m(x), z, x and xs.
#
# D = diag(d) the effective noise (VFE / DTC: the noise; FITC: noise_i + k(x_i, x_i) - k_i^T K_z^{-1} k_i, k_i = k(z, x_i)),
# Sigma = K_z + K_zx D^{-1} K_xz, a = Sigma^{-1} K_zx D^{-1} r, K_s = k(z, xs).  Outputs: mu_j = K_s[:, j]^T a (the mean minus m(xs))
# and s_j = K_s[:, j]^T (K_z^{-1} - Sigma^{-1}) K_s[:, j] (k(xs_j, xs_j) minus the marginal variance).  With the cotangents gm of mu
# and gs of s, P = K_z^{-1} K_s, Q = Sigma^{-1} K_s, e = Q gm, G_v = Q diag(gs) Q^T, G_m = -1/2 (e a^T + a e^T), G = G_v + G_m:
#     dL/dK_s  = a gm^T + 2 (P - Q) diag(gs)                              (M x N*)
#     dL/dK_z  = -P diag(gs) P^T + G                                       (M x M)
#     dL/dK_zx = 2 G K_zx D^{-1} + e (D^{-1} r)^T                          (M x N: ONE MFMA GEMM, 2 M^2 N flops)
#     dL/dd_i  = -[ k_i^T G k_i + (e^T k_i) r_i ] / d_i^2,       dL/dr_i = (e^T k_i) / d_i
#     FITC, g_d = dL/dd:  dL/dk(x_i, x_i) += g_d_i,  dL/dK_zx -= 2 K_z^{-1} K_zx diag(g_d),  dL/dK_z += K_z^{-1} K_zx diag(g_d) K_xz K_z^{-1}
# Each kernel-matrix cotangent is reduced by gpk_kmat_vjp_dense on its own pair of inputs -- (z, xs), (z, x), (z, z) -- the rank-one
# parts in its w / b operands, the diagonal scalings in its colscale; k_i^T G k_i comes out of its column sums.  The jitter is a
# constant: the plain path holds the mean's Sigma as L_z (A + eps I) L_z^T = Sigma + eps K_z and the variance's as Sigma + eps I
# (`AbstractPseudoObservations.A`); Q is taken with the latter, e and a with the former, whose K_z share counts (1 + eps) times.
# A loss of the mean only (gs = 0) has G = G_m of rank two: no M x N* solve, and (VFE / DTC) no GEMM either -- the cotangent of K_zx is
# e ((r - K_xz a) / d)^T - a (K_xz e / d)^T, two rank-one passes.  Nothing of size M x N lives between forward and backward: K_zx (and
# FITC's V, for d) is evaluated again in the backward.
# ---------------------------------------------------------------------------------------------
class _SparsePosteriorMarginals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, noise_vec, run, fitc, layout, *tensors):
        """``run()`` -> ``(chol_z, chol_a, chol_post, w, vz, va, mu, s)``: the plain HIP path of the pseudo-point posterior
        (``learnable._sparse_posterior_parts``) -- the factors of ``K_z``, of ``A + eps I`` (the mean's) and of ``A + eps L_z^{-1} L_z^{-T}``
        (the variance's), ``w = L_z^{-1} (mu_z - m(z))`` (M, 1), ``vz = L_z^{-1} K_s``, ``va = L_post^{-1} vz`` (M, N*) and the outputs;
        what a mean-only / variance-only call does not need is None.  ``layout`` / ``tensors``: ONE group, its inputs ``x`` (N, D), ``z``
        (M, D) and ``xs`` (N*, D) as the fused kernels see them, then its parameters; ``r`` (N, 1), ``noise_vec`` (N,)."""
        chol_z, chol_a, chol_post, w, vz, va, mu, s = run()
        (ctx.group,) = _split_groups(layout, tensors, 3)
        ctx.parts = (chol_z, chol_a, chol_post, w, vz, va)
        ctx.r, ctx.noise, ctx.fitc = r.detach(), noise_vec.detach(), fitc
        ctx.set_materialize_grads(False)
        ref = mu if mu is not None else s
        return (torch.zeros_like(ref) if mu is None else mu), (torch.zeros_like(ref) if s is None else s)

    @staticmethod
    def backward(ctx, g_mu, g_s):
        be = ops.get_backend()
        chol_z, chol_a, chol_post, w, vz, va = ctx.parts
        grp, fitc = ctx.group, ctx.fitc
        (x, z, xs), terms, kinds = grp.inputs, grp.terms, grp.kinds
        x, z, xs = x.detach(), z.detach(), xs.detach()
        n, m, ns = x.shape[0], z.shape[0], xs.shape[0]
        dt, dev = x.dtype, x.device
        gm, gs = _output_cotangents(g_mu, g_s, w is not None, va is not None, dt)
        need_r, need_noise, need_x, need_z, need_xs = (ctx.needs_input_grad[i] for i in (0, 1, 5, 6, 7))
        if gm is None and gs is None:
            return (None,) * (8 + len(grp.meta))
        if need_x or need_z or need_xs:
            check_input_dims(x)
        eps = float(config.epsilon)
        # (an ascent over xs alone -- an acquisition function on a fitted surrogate -- ends behind the k(z, xs) block: nothing of size N)
        model = need_r or need_noise or need_x or need_z or any(ctx.needs_input_grad[8:])

        def outer(u, v):
            return u[:, None] * v[None, :]

        r = ctx.r[:, 0]
        a = e = None
        if gm is not None:
            a = chol_z.solve_t(w)[:, 0]                                            # Sigma^{-1} K_zx D^{-1} r
            t = chol_a.solve_t(chol_a.solve(be.gemv(vz, gm[:, None])))             # (A + eps I)^{-1} L_z^{-1} K_s gm
            e = chol_z.solve_t(t)[:, 0]                                            # Sigma^{-1} K_s gm
        pq = g_v = g_kz = None
        if gs is not None:
            # P = K_z^{-1} K_s and Q = Sigma^{-1} K_s: the M x N* back-substitutions (on private copies: the solves use them up)
            pm = chol_z.solve_t_(be.copy(vz))
            qm = chol_z.solve_t_(chol_post.solve_t_(be.copy(va)))
            if model:
                sc = be.scale_cols_(be.copy(qm), gs)
                g_v = be.symmetrize_(be.gemm(sc, qm, a_kmajor=True, b_kmajor=True, lower_only=True))       # Q diag(gs) Q^T
                sc.copy_(pm)
                be.scale_cols_(sc, gs)
                g_kz = be.symmetrize_(be.gemm(sc, pm, a_kmajor=True, b_kmajor=True, alpha=-1.0, lower_only=True))
                del sc
            pq = pm.sub_(qm)
            del pm, qm
        # through k(z, xs): cotangent a gm^T + 2 (P - Q) diag(gs)
        cs = 2.0 * gs if gs is not None else None
        if model:
            S, _, gz = be.kmat_vjp_dense(terms, z, xs, pq if pq is not None else _zeros(m, ns, x), colscale=cs, w=a, b=gm, want_gradx=need_z)
        gxs = None
        if need_xs:
            if pq is not None:
                be.scale_cols_(pq, cs)
                g_t = pq.t().contiguous()                                          # (N*, M): 2 diag(gs) (P - Q)^T, explicit
            else:
                g_t = _zeros(ns, m, x)
            _, _, gxs = be.kmat_vjp_dense(terms, xs, z, g_t, w=gm, b=a, want_gradx=True)
            del g_t
        del pq
        if not model:
            return (None,) * 7 + (gxs,) + (None,) * len(grp.meta)
        # the effective noise: FITC's takes V = L_z^{-1} K_zx once more
        kzx = be.kmat(terms, z, x)
        d, rr = ctx.noise, None
        if fitc:
            rr = chol_z.solve(kzx)
            _, q = be.colreduce(rr, want_ss=True)
            d = d + be.kdiag(terms, x) - q
        ek = be.colreduce(kzx, e, want_dot=True, want_ss=False)[0] if gm is not None else None      # K_xz e
        # through k(z, x): cotangent 2 G K_zx D^{-1} + e (D^{-1} r)^T
        if gs is None and not fitc:
            # G = G_m, of rank two: e ((r - K_xz a) / d)^T - a (K_xz e / d)^T, two rank-one passes and no M x N cotangent
            ak = be.colreduce(kzx, a, want_dot=True, want_ss=False)[0]
            del kzx
            g_k, cs_k = None, None
            ranks = [(e, (r - ak) / d), (a, -ek / d)]
            g_d = -ek * (r - ak) / (d * d)
            gz_k = None
            for wv, bv in ranks:
                s_k, _, gz_p = be.kmat_vjp_dense(terms, z, x, _zeros(m, n, x), w=wv, b=bv, want_gradx=need_z)
                S = S + s_k
                if need_z:
                    gz_k = gz_p if gz_k is None else gz_k + gz_p
        else:
            g_sig = g_v if g_v is not None else torch.zeros((m, m), dtype=dt, device=dev)
            if gm is not None:
                g_sig = g_sig - 0.5 * (outer(e, a) + outer(a, e))
            g_k = be.gemm(g_sig, kzx, a_kmajor=True, b_kmajor=False, alpha=2.0)    # M x N, the one big GEMM
            del kzx
            cs_k = 1.0 / d
            ranks = [(e, r / d)] if gm is not None else [(None, None)]
            s_k, colsum, gz_k = be.kmat_vjp_dense(terms, z, x, g_k, colscale=cs_k, w=ranks[0][0], b=ranks[0][1], want_colsum=True,
                                                  want_gradx=need_z and not fitc)
            g_d = -(colsum * d + (ek * r if gm is not None else 0.0)) / (2.0 * d * d)
            if fitc:
                # the effective noise depends on K_zx and K_z through q_i = k_i^T K_z^{-1} k_i: the cotangent of K_zx gets
                # -2 K_z^{-1} K_zx diag(g_d) and that of K_z  K_z^{-1} K_zx diag(g_d) K_xz K_z^{-1}
                rr = chol_z.solve_t_(rr)                                           # K_z^{-1} K_zx   (M x N)
                g_k.addcmul_(rr, (-2.0 * g_d * d)[None, :])
                s_k, _, gz_k = be.kmat_vjp_dense(terms, z, x, g_k, colscale=cs_k, w=ranks[0][0], b=ranks[0][1], want_gradx=need_z)
                sc = be.scale_cols_(be.copy(rr), g_d)
                rgr = be.symmetrize_(be.gemm(sc, rr, a_kmajor=True, b_kmajor=True, lower_only=True))
                g_kz = rgr if g_kz is None else g_kz + rgr
                del sc, rr
            S = S + s_k
        gx = None
        if need_x:
            # d/dx through K_zx: the same reduction with the roles of the arguments swapped, on the explicit N x M transpose of the
            # cotangent's full-rank part (one extra N x M buffer, backward only)
            if g_k is not None:
                be.scale_cols_(g_k, cs_k)
                g_t = g_k.t().contiguous()
            else:
                g_t = _zeros(n, m, x)
            del g_k
            for i, (wv, bv) in enumerate(ranks):
                _, _, gx_p = be.kmat_vjp_dense(terms, x, z, g_t if i == 0 else _zeros(n, m, x), w=bv, b=wv, want_gradx=True)
                gx = gx_p if gx is None else gx + gx_p
            del g_t
        else:
            del g_k
        # through K_z: -P diag(gs) P^T + G  (the mean's share of G sits behind Sigma + eps K_z)
        if g_kz is None:
            g_kz = torch.zeros((m, m), dtype=dt, device=dev)
        if g_v is not None:
            g_kz = g_kz + g_v
        if gm is not None:
            g_kz = g_kz - (0.5 * (1.0 + eps)) * (outer(e, a) + outer(a, e))
        s_kz, _, gz_kz = be.kmat_vjp_dense(terms, z, z, g_kz, want_gradx=need_z)
        S = S + s_kz
        gr = _param_grads(kinds, grp.values, S, [(S.device, S.dtype)] * len(grp.meta))
        if fitc:
            gx = _diag_share(grp, x, g_d, gr, gx, need_x)                         # (through k(x_i, x_i) in the effective noise)
        grads = [None if g_ is None else g_.to(device=dv, dtype=dty) for g_, (dv, dty) in zip(gr, grp.meta)]
        grad_z = None
        if need_z:
            grad_z = gz + 2.0 * gz_kz + (gz_k if gz_k is not None else 0.0)
        grad_r = (ek / d)[:, None] if (need_r and ek is not None) else None
        grad_noise = g_d if need_noise else None
        return (grad_r, grad_noise, None, None, None, gx, grad_z, gxs, *grads)


def sparse_posterior_marginals(kernel, x, z, xs, r, noise_vec, method, run):
    """Differentiable ``(mu, s)`` of ``_SparsePosteriorMarginals``: ``kernel`` a sum of primitives evaluated on ``x`` / ``z`` / ``xs``
    (already behind its input map, so torch carries the map's parameter)."""
    _check_method(method)
    layout, params = _pack_groups([kernel])
    return _SparsePosteriorMarginals.apply(r, noise_vec, run, method == "fitc", layout, x, z, xs, *params)


def posterior_marginals(groups, r, noise_vec, run):
    """Differentiable ``(mu, s)`` of ``_PosteriorMarginals``; ``groups`` = ``[(k_g, x_g, xs_g)]``, every ``k_g`` a sum of primitives
    evaluated on ``x_g`` / ``xs_g`` (already behind the group's input map, so torch carries the map's parameter).  Batched inputs
    (B, N, D) / (B, N*, D), shared hyper-parameters: ``_BatchedPosteriorMarginals``."""
    layout, params = _pack_groups([kern for kern, _, _ in groups])
    fn = _BatchedPosteriorMarginals if groups[0][1].dim() == 3 else _PosteriorMarginals
    return fn.apply(r, noise_vec, run, layout, *[t for _, x, xs in groups for t in (x, xs)], *params)


# ---------------------------------------------------------------------------------------------
# The JOINT posterior covariance of the same exact posterior, Sigma = k(xs, xs) - V^T V (N* x N*; `post(xs).var`, and through it
# `.sample()` and `.entropy()`), differentiable w.r.t. everything the marginal variances cover.  The marginal-variance backward with
# diag(g_s) replaced by a symmetric matrix: with G the cotangent of Sigma, Gs = (G + G^T) / 2, B = L^{-T} V = K^{-1} k(x, xs),
#     dL/dk(xs, xs) = Gs                          (N* x N*; its input gradient counts for both arguments)
#     dL/dk(x, xs)  = -2 B Gs = -2 C              (N x N*, ONE N x N* x N* GEMM; d/dxs over its explicit transpose)
#     dL/dK         = B Gs B^T = C B^T            (N x N, ONE lower-only N x N x N* GEMM; its diagonal: d/dnoise)
# and the predictive noise sees the diagonal of G (`add_diagonal`).  Every reduction is a launch the marginal path uses:
# gpk_kmat_vjp_dense on (xs, xs), (x, xs) and (xs, x), gpk_kmat_vjp on the lower triangle of dL/dK (A = 0, g = [-2]: its form
# 1/2 (A diag(g) A^T - sum(g) S) is then S itself), and gpk_kmat_vjp_dense on (x, x) over the mirrored dL/dK where x needs a gradient.
# Their number depends on the number of groups, not on N*.  The mean of the same evaluation has a node of its own
# (`_PosteriorMarginals`): B is formed there only for a loss of the marginal variances, so the two share the factor and V, not B.
# ---------------------------------------------------------------------------------------------
class _PosteriorCovariance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, noise_vec, run, layout, *tensors):
        """``run()`` -> ``(chol, v, cov)``: the plain HIP path (``PosteriorKernel.pairwise`` on detached values, as it is) with the
        factor and ``v = L^{-1} k(x, xs)`` (N, N*) or its transpose as a ``WhitenedT`` it left behind.  ``layout`` / ``tensors`` as in
        ``_PosteriorMarginals``: per group ``x`` / ``xs`` behind the group's input map, then the groups' parameters."""
        chol, v, cov = run()
        ctx.groups = _split_groups(layout, tensors, 2)
        ctx.chol, ctx.v = chol, v
        ctx.has_noise = noise_vec is not None
        return cov

    @staticmethod
    def backward(ctx, g_cov):
        be = ops.get_backend()
        groups, chol, v = ctx.groups, ctx.chol, ctx.v
        ng = len(groups)
        x0, xs0 = groups[0].inputs
        n, ns = x0.shape[0], xs0.shape[0]
        dt = x0.dtype
        need_x = [ctx.needs_input_grad[3 + 2 * i] for i in range(ng)]
        need_xs = [ctx.needs_input_grad[4 + 2 * i] for i in range(ng)]
        for grp, nx, nxs in zip(groups, need_x, need_xs):
            if nx or nxs:
                check_input_dims(grp.inputs[0])
        g_cov = g_cov.to(dt)
        gsym = (0.5 * (g_cov + g_cov.transpose(-1, -2))).contiguous()
        bm = chol.solve_t_(v.plain() if hasattr(v, "zt") else be.copy(v))                 # B = L^{-T} V  (N, N*)
        c = be.gemm(bm, gsym, a_kmajor=True, b_kmajor=True)                               # C = B Gs     (N, N*)
        c_t = c.t().contiguous() if any(need_xs) else None                                # (N*, N), explicit
        gk = be.gemm(c, bm, a_kmajor=True, b_kmajor=True, lower_only=True)                # C B^T = B Gs B^T, lower triangle (N, N)
        del bm
        zero = torch.zeros((n, 1), dtype=dt, device=x0.device)
        if any(need_x):
            be.symmetrize_(gk)
        S, grad_x, grad_xs, diag_g = [None] * ng, [None] * ng, [None] * ng, None
        for i, grp in enumerate(groups):
            terms, (x, xs) = grp.terms, grp.inputs
            S_ss, _, gx_ss = be.kmat_vjp_dense(terms, xs, xs, gsym, want_gradx=need_xs[i])        # through k(xs, xs)
            S_c, _, gx_c = be.kmat_vjp_dense(terms, x, xs, c, want_gradx=need_x[i])               # through k(x, xs): -2 C
            S_k, _, dg = be.kmat_vjp(terms, x, gk, zero, [-2.0])                                  # through K: the lower triangle of C B^T
            S[i] = S_ss - 2.0 * S_c + S_k
            if i == 0:
                diag_g = dg                                                                       # (the same from every group)
            if need_xs[i]:
                _, _, gx_t = be.kmat_vjp_dense(terms, xs, x, c_t, want_gradx=True)
                grad_xs[i] = 2.0 * gx_ss - 2.0 * gx_t
            if need_x[i]:
                grad_x[i] = _grad_inputs(be, terms, x, gk) - 2.0 * gx_c
        grad_noise = diag_g if (ctx.has_noise and ctx.needs_input_grad[0]) else None
        inputs = [t for pair in zip(grad_x, grad_xs) for t in pair]
        return (grad_noise, None, None, *inputs, *_sum_param_grads(groups, S))


def posterior_covariance(groups, noise_vec, run):
    """The differentiable joint covariance ``k(xs, xs) - V^T V`` (N*, N*) of ``_PosteriorCovariance``; ``groups`` = ``[(k_g, u_g(x),
    u_g(xs))]``; ``run``: the plain path."""
    layout, params = _pack_groups([kern for kern, _, _ in groups])
    return _PosteriorCovariance.apply(noise_vec, run, layout, *[t for _, xin, xsin in groups for t in (xin, xsin)], *params)


class _AddDiagonal(torch.autograd.Function):
    """``mat + diag(d)`` by the launches ``Dense.__add__`` has always made (a copy, ``gpk_add_diag``), recorded: the cotangent goes to the
    matrix as it is and its diagonal to ``d`` -- a learnable predictive noise under a joint posterior."""

    @staticmethod
    def forward(ctx, mat, d):
        be = ops.get_backend()
        return be.add_diag_(be.copy(mat), 0.0, d)

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.needs_input_grad[0] else None,
                torch.diagonal(g, dim1=-2, dim2=-1).clone() if ctx.needs_input_grad[1] else None)


def add_diagonal(mat, d):
    return _AddDiagonal.apply(mat, d)


class _FactorTimes(torch.autograd.Function):
    """``chol(A) xi`` for a covariance ``A`` (n, n) inside the graph -- the factorisation of ``Normal.sample``, differentiable.
    Forward: the factor the matrix object caches (``gpk_potrf``, as ever) and the one GEMM.  Backward: the cotangent of ``L`` is
    ``tril(ybar xi^T)`` (one GEMM; ``gpk_potrf_vjp`` reads its lower triangle only), the cotangent of ``A`` is ``gpk_potrf_vjp`` of it."""

    @staticmethod
    def forward(ctx, a, factor, xi):
        chol = factor()
        ctx.chol, ctx.xi = chol, xi
        return ops.get_backend().gemm(chol.lower(), xi, a_kmajor=True, b_kmajor=False)

    @staticmethod
    def backward(ctx, ybar):
        be = ops.get_backend()
        lbar = be.gemm(ybar.contiguous(), ctx.xi, a_kmajor=True, b_kmajor=True)           # ybar xi^T  (n, n)
        return ctx.chol.potrf_vjp(lbar), None, None


def factor_times(a, factor, xi):
    """``chol(a) @ xi`` with the gradient to ``a``; ``factor()`` -> the ``Chol`` of ``a`` (plus jitter), ``xi`` (n, num) detached."""
    return _FactorTimes.apply(a, factor, xi)


class _LogdetSPD(torch.autograd.Function):
    """``log det A`` for a covariance ``A`` (n, n) inside the graph -- ``Normal.entropy``.  Forward: the cached factor's
    ``gpk_logdet_chol``.  Backward: ``A^{-1} = W^T W`` from ``gpk_trtri_lower`` and the triangular GEMM the log-density's backward
    uses, mirrored."""

    @staticmethod
    def forward(ctx, a, factor):
        chol = factor()
        ctx.chol = chol
        return chol.logdet()

    @staticmethod
    def backward(ctx, g):
        be = ops.get_backend()
        w = ctx.chol.inverse_lower()
        ainv = be.symmetrize_(be.gemm(w, w, a_kmajor=False, b_kmajor=False, lower_only=True, tri_k=True))
        return ainv * g.to(ainv.dtype), None


def logdet_spd(a, factor):
    return _LogdetSPD.apply(a, factor)
