"""Dense fp64 torch reference, on the CPU, for the mean and the marginal variances of a pseudo-point posterior
``f | PseudoObs(f(z), f(x, noise), y)`` at test inputs ``xs`` -- straight from the reference's ``observations.py:255-336`` for VFE, FITC
and DTC, differentiated by torch autograd.  Not collected (no ``test_`` prefix): shared by ``test_sparse_posterior_grad_host.py`` and
``test_sparse_posterior_grad_gpu.py``.

The jitter sits where the plain path puts it, so that the forward values agree to rounding:

* ``K_z + eps I`` is what is factorised, ``L_z``;
* the mean of the optimal distribution comes from ``chol(A + eps I)``, ``A = I + V D^{-1} V^T``, ``V = L_z^{-1} K_zx``
  (``AbstractPseudoObservations._compute`` / ``mu``), i.e. from ``Sigma + eps (K_z + eps I)``;
* the subspace kernel comes from ``chol(L_z A L_z^T + eps I)`` (``AbstractPseudoObservations.A``), i.e. from ``Sigma + eps I``.
"""
import math

import torch


def kmat_t(kinds, vs, ss, alphas, a, b):
    """``sum_t v_t kappa_t(a / s_t, b / s_t)`` for the kinds eq / matern12 / matern52 / rq / linear."""
    out = 0
    for t, (kind, v, s) in enumerate(zip(kinds, vs, ss)):
        if kind == "linear":
            k = (a @ b.T) / (s * s)
        else:
            q = (((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / (s * s)).clamp_min(1e-300)
            if kind == "eq":
                k = torch.exp(-0.5 * q)
            elif kind == "matern12":
                k = torch.exp(-torch.sqrt(q))
            elif kind == "matern52":
                r = torch.sqrt(5.0 * q)
                k = (1 + r + r * r / 3) * torch.exp(-r)
            elif kind == "rq":
                k = (1 + q / (2 * alphas[t])) ** (-alphas[t])
            else:
                raise NotImplementedError(kind)
        out = out + v * k
    return out


def kdiag_t(kinds, vs, ss, a):
    return sum(v * ((a * a).sum(-1) / (s * s) if kind == "linear" else torch.ones(a.shape[0], dtype=a.dtype)) for kind, v, s in zip(kinds, vs, ss))


def input_map(kind, param):
    """The maps of the inputs: None, ``"ard"`` (division by per-dimension length scales), ``"periodic"``."""
    if kind is None:
        return lambda t: t
    if kind == "ard":
        return lambda t: t / param
    if kind == "periodic":
        return lambda t: torch.cat([torch.sin(2 * math.pi * t / param), torch.cos(2 * math.pi * t / param)], dim=-1)
    raise NotImplementedError(kind)


def sparse_posterior_t(method, kinds, vs, ss, alphas, x, z, xs, y, noise, mean_c, eps, imap=lambda t: t):
    """``(mean (N*,), marginal variance (N*,))`` of the latent process under the pseudo-point posterior; ``noise`` (N,) or a scalar,
    ``mean_c`` the constant prior mean, ``eps`` the jitter."""
    x, z, xs = imap(x), imap(z), imap(xs)
    n, m = x.shape[0], z.shape[0]
    eye = torch.eye(m, dtype=x.dtype)
    L_z = torch.linalg.cholesky(kmat_t(kinds, vs, ss, alphas, z, z) + eps * eye)
    K_zx = kmat_t(kinds, vs, ss, alphas, z, x)
    K_s = kmat_t(kinds, vs, ss, alphas, z, xs)
    V = torch.linalg.solve_triangular(L_z, K_zx, upper=False)                     # :300-301
    d = noise.expand(n)
    if method == "fitc":
        d = d + kdiag_t(kinds, vs, ss, x) - (V * V).sum(0)                         # :312
    elif method not in ("vfe", "dtc"):
        raise ValueError(method)
    A = eye + (V / d) @ V.T                                                       # :322
    r = y - mean_c
    # the mean of the optimal distribution (:224-237) and the posterior mean (:270-277)
    L_a = torch.linalg.cholesky(A + eps * eye)
    u = torch.cholesky_solve((V / d) @ r, L_a)                                    # (A + eps I)^{-1} V D^{-1} r
    Vs = torch.linalg.solve_triangular(L_z, K_s, upper=False)
    mean = mean_c + (Vs.T @ u)[:, 0]
    # the posterior kernel (:256-267): k - K_s^T K_z^{-1} K_s + K_s^T (L_z A L_z^T + eps I)^{-1} K_s
    L_post = torch.linalg.cholesky(L_z @ A @ L_z.T + eps * eye)
    Va = torch.linalg.solve_triangular(L_post, K_s, upper=False)
    var = kdiag_t(kinds, vs, ss, xs) - (Vs * Vs).sum(0) + (Va * Va).sum(0)
    return mean, var


def loss_of(kind, mean, var, wts):
    if kind == "mean":
        return (mean * wts).sum()
    if kind == "var":
        return (var * wts).sum()
    return ((mean + 2.0 * torch.sqrt(var)) * wts).sum()          # UCB
