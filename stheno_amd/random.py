"""``Normal``: the multivariate normal of the reference (``stheno/random.py``), restated
over torch tensors on a HIP device, with the lazy mean / variance / variance-diagonal
resolution semantics of ``random.py:96-117,149-227`` and ``logpdf`` of
``random.py:248-280``.

What is computed once: the variance is resolved once; its Cholesky factor is cached on
the matrix object and shared by ``logdet`` and ``iqf_diag`` (one POTRF per logpdf, one
per conditioning).
"""
import types

import torch

from . import ops
from .matrix import LOG_2_PI, AbstractMatrix, Dense, Diagonal, KernelDense, Zero, any_missing, config, deferred_checks, to_matrix

__all__ = ["Random", "RandomProcess", "RandomVector", "Normal"]


class Random:
    """A random object."""

    def __radd__(self, other):
        return self + other

    def __rmul__(self, other):
        return self * other

    def __neg__(self):
        return -1 * self

    def __sub__(self, other):
        return self + (-other)

    def __rsub__(self, other):
        return (-self) + other

    def __truediv__(self, other):
        return self * (1 / other)


class RandomProcess(Random):
    """A random process."""


class RandomVector(Random):
    """A random vector."""


def _is_zero(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool) and x == 0


class _Deferred:
    """One quantity of a distribution that may not exist yet: given up front, or made on first use by a zero-argument callable
    (the reference's ``Normal`` takes such constructors so that a prior's ``f(x)`` costs nothing until something is asked of it,
    ``random.py:56-117``)."""

    __slots__ = ("value", "make")

    def __init__(self, value=None, make=None):
        self.value, self.make = value, make

    @property
    def known(self):
        return self.value is not None

    def get(self):
        if self.value is None and self.make is not None:
            self.value = self.make()
        return self.value


class Normal(RandomVector):
    """Normal random variable.

    ``Normal(var)``, ``Normal(mean, var)`` with tensors / structured matrices, or
    ``Normal(mean_fn, var_fn, var_diag=..., mean_var=..., mean_var_diag=...)`` with
    zero-argument constructors that are called lazily (``random.py:56-94``).

    State: three deferred quantities (mean, variance, marginal variances) and two optional JOINT constructors that produce the mean
    together with the variance / the marginal variances in one go (a posterior shares the whitened cross-kernel between them).  A
    joint constructor is only worth calling while neither of its two quantities exists; after that the single ones are used.
    """

    def __init__(self, *args, var_diag=None, mean_var=None, mean_var_diag=None):
        if len(args) == 1:
            mean, var = (lambda: 0) if isinstance(args[0], types.FunctionType) else 0, args[0]
        elif len(args) == 2:
            mean, var = args
        else:
            raise TypeError("Normal(var) or Normal(mean, var)")
        lazy = isinstance(var, types.FunctionType)
        if lazy and not isinstance(mean, types.FunctionType):
            raise TypeError("mean and var must both be constructors or both be values")
        self._m = _Deferred(make=mean) if lazy else _Deferred(mean)
        self._v = _Deferred(make=var) if lazy else _Deferred(var)
        self._d = _Deferred(make=var_diag if lazy else None)
        self._joint_var = mean_var if lazy else None
        self._joint_diag = mean_var_diag if lazy else None
        self._mean_vanishes = None       # whether the mean is identically zero, decided when the mean first exists

    def computed(self, what):
        """Whether ``"mean"``, ``"var"`` or ``"var_diag"`` has been given or computed already (nothing is computed by asking)."""
        return {"mean": self._m, "var": self._v, "var_diag": self._d}[what].known

    # -- the deferred quantities (random.py:96-202) ----------------------------
    def _settle_mean(self, as_tensor):
        """The mean exists after this; a scalar zero stays a scalar unless ``as_tensor`` (then it becomes a zero column of the
        variance's shape and type, which makes the variance exist too)."""
        m = self._m.get()
        if self._mean_vanishes is None:
            self._mean_vanishes = _is_zero(m) or isinstance(m, Zero)
        if as_tensor and _is_zero(m):
            var = self.var
            shape = tuple(var.shape)
            self._m.value = torch.zeros(shape[:-2] + (shape[-1], 1), dtype=var.dtype, device=var.device)

    def _settle_jointly(self, other, joint):
        """``other`` is the variance or the marginal-variance slot: while neither it nor the mean exists, one call of ``joint``
        (if there is one) makes both."""
        if joint is not None and not self._m.known and not other.known:
            self._m.value, other.value = joint()

    def __repr__(self):
        m = repr(self._m.value) if self._m.known else "unresolved"
        v = repr(self._v.value) if self._v.known else "unresolved"
        return f"<Normal:\n mean={m},\n var={v}>"

    __str__ = __repr__

    @property
    def _mean_t(self):
        """The mean as a plain column-vector tensor (what every computation below uses)."""
        self._settle_mean(as_tensor=True)
        m = self._m.value
        return m.dense() if isinstance(m, AbstractMatrix) else m

    @property
    def mean(self):
        """Column vector: mean.  A plain tensor -- or, with ``config.mean_as_matrix``, the reference's return type (``matrix.Dense``,
        README.md:58-68; ``B.dense`` strips it)."""
        m = self._mean_t
        return Dense(m) if config.mean_as_matrix else m

    @property
    def mean_is_zero(self):
        self._settle_mean(as_tensor=False)
        return self._mean_vanishes

    @property
    def var(self):
        """Variance as a structured matrix (``B.dense(d.var)`` for the plain tensor)."""
        self._v.value = to_matrix(self._v.get())
        return self._v.value

    @property
    def var_diag(self):
        if not self._d.known and self._d.make is None:
            self._d.value = self.var.diag()
        return self._d.get()

    @property
    def mean_var(self):
        self._settle_jointly(self._v, self._joint_var)
        return self.mean, self.var

    @property
    def dtype(self):
        return self.var.dtype

    @property
    def dim(self):
        return self.var.shape[-1]

    # -- marginals (random.py:204-238) -----------------------------------------
    def marginals(self):
        """Marginal means and variances (the covariance is not formed when a
        ``mean_var_diag`` constructor is available)."""
        self._settle_jointly(self._d, self._joint_diag)
        mean, var_diag = self._mean_t, self.var_diag
        if isinstance(var_diag, AbstractMatrix):
            var_diag = var_diag.dense()
        # Variances can come out slightly negative through round-off (random.py:221-227).
        if torch.is_tensor(mean) and mean.dim() >= 1:
            mean = mean[..., 0]
        if torch.is_tensor(var_diag):
            var_diag = torch.clamp(var_diag, min=0)
        return mean, var_diag

    def marginal_credible_bounds(self):
        """Marginal means with lower and upper 95% central credible bounds."""
        mean, var = self.marginals()
        error = 1.96 * torch.sqrt(var)
        return mean, mean - error, mean + error

    # -- logpdf (random.py:248-280) --------------------------------------------
    def logpdf(self, x):
        """Log-density at ``x``: ``(N,)``/``(N, 1)`` -> scalar tensor, ``(N, C)`` -> ``(C,)``,
        batched ``(B, N, 1)`` -> ``(B,)``."""
        return self._logpdf(x)[0]

    def _logpdf(self, x):
        """``(value, differentiable)``: whether the value came from one of the autograd paths (``stheno_amd/autograd.py``) --
        everything else is computed by ``libgpk.so`` on detached buffers, whatever ``value.requires_grad`` says."""
        if not torch.is_tensor(x):
            x = torch.as_tensor(x, dtype=self.dtype, device=self.var.device)
        if x.dim() <= 1:
            x = x.reshape(-1, 1)

        # Missing data (not for batched computation): random.py:261-270.
        if config.check_nan and x.dim() == 2 and x.shape[1] == 1:
            if any_missing(x):
                available = ~torch.isnan(x[:, 0])
                idx = torch.nonzero(available)[:, 0]
                mean = self._mean_t[idx]
                var = self.var
                if isinstance(var, KernelDense) and torch.is_tensor(var.x) and var.x.dim() == 2 and var._mat is None and not isinstance(var.noise, Dense) \
                        and var.kernel.num_outputs(var.x) == var.x.shape[0]:
                    # a kernel matrix restricted to the observed points is the kernel matrix OF those points:
                    # stay lazy (lower-only build, in-place factor) and differentiable
                    noise = var.noise
                    if isinstance(noise, Diagonal):
                        noise = Diagonal(noise.diag()[idx])
                    elif isinstance(noise, Zero):
                        noise = Zero(noise.dtype, idx.numel(), idx.numel(), device=noise.device)
                    sub = KernelDense(var.kernel, var.x[idx], noise)
                else:
                    sub = var.dense()[idx][:, idx]
                return Normal(mean, sub)._logpdf(x[idx])

        var = self.var
        n = self.dim
        # (a zero prior mean: the residual IS the data -- no zeros materialised, nothing subtracted; aliasing is safe: every consumer
        #  below reads `r` or copies it before solving in place)
        if (getattr(self, "_zero_mean", False) and x.dtype == self.dtype and x.dim() == 2 and x.shape[0] == n and not x.requires_grad
                and x.device == self.var.device):
            r = x
        else:
            r = x - self._mean_t
        if isinstance(var, KernelDense):     # hyper-parameter learning: the differentiable paths, or their refusal
            from . import learnable
            lp = learnable.logpdf(var, r)
            if lp is not None:
                return lp, True
        if isinstance(var, Zero):
            raise torch.linalg.LinAlgError("the variance is identically zero")
        with deferred_checks():      # the factor's `info` is read after the log-determinant and the solve are queued behind it
            # (a zero prior mean: `r` IS `x`; naming it lets the factor hand the same L^{-1} y to the posterior mean later)
            src = x if (getattr(self, "_zero_mean", False) and isinstance(var, Dense)) else None
            if hasattr(var, "chol_with_rhs"):
                var.chol_with_rhs(r, src)      # (a batch that has not been factorised yet: L^{-1} r comes out of the factorisation)
            logdet = var.logdet()
            iqf = var.iqf_diag(r, src) if src is not None else var.iqf_diag(r)
            logpdfs = torch.add(logdet[..., None], iqf).add_(n * LOG_2_PI).mul_(-0.5)       # -(logdet + n log 2 pi + iqf) / 2 in three launches
        return (logpdfs[..., 0] if logpdfs.shape[-1] == 1 else logpdfs), False

    def entropy(self):
        var = self.var
        mat = self._graph_matrix(var)
        if mat is not None:          # the covariance carries a graph (a joint posterior under learnable quantities): its gradient too
            from .autograd import logdet_spd
            return (logdet_spd(mat, var.chol) + self.dim * (LOG_2_PI + 1)) / 2
        return (var.logdet() + self.dim * (LOG_2_PI + 1)) / 2

    @staticmethod
    def _graph_matrix(var):
        """The variance's matrix if it is inside the autograd graph (``learnable.graph_matrix``), else None: the plain path."""
        if not torch.is_grad_enabled():
            return None
        from . import learnable
        return learnable.graph_matrix(var)

    @property
    def m2(self):
        """Second moment ``V + m m^T`` (``random.py:200-202``)."""
        m = self._mean_t.contiguous()
        be = ops.get_backend()
        return Dense(be.gemm(m, m, a_kmajor=True, b_kmajor=True, alpha=1.0, beta=1.0, out=be.copy(self.var.dense())))

    def diagonalise(self):
        """The distribution with its correlations set to zero (``random.py:240-246``)."""
        return Normal(self._mean_t, Diagonal(self.var_diag))

    def kl(self, other):
        """``KL(self || other)`` (``random.py:294-311``): ``tr(V_o^{-1} V_s) = |L_o^{-1} L_s|_F^2`` from the two
        Cholesky factors (one TRSM), the quadratic term by a TRSV."""
        vs, vo = to_matrix(self.var), to_matrix(other.var)
        if isinstance(vs, Diagonal) or isinstance(vo, Diagonal):
            vs, vo = Dense(vs.dense()), Dense(vo.dense())
        w = vo.chol().solve(vs.chol().lower())
        _, ss = ops.get_backend().colreduce(w, want_ss=True)
        ratio = ss.sum(-1)
        iqf = vo.iqf_diag(other._mean_t - self._mean_t)[..., 0]
        return (iqf + ratio + vo.logdet() - vs.logdet() - self.dim) / 2

    def w2(self, other, iters=None):
        """2-Wasserstein distance to ``other`` (``random.py:313-329``); ``(B, n)`` distributions give ``(B,)``.

        With ``V_s = L_s L_s^T`` and ``V_o = L_o L_o^T``,
        ``W2^2 = |m_s - m_o|^2 + tr V_s + tr V_o - 2 |L_o^T L_s|_*``: the trace of ``(V_s^(1/2) V_o V_s^(1/2))^(1/2)`` is the sum of the
        singular values of ``M = L_o^T L_s`` (the two share their non-zero eigenvalues with ``M^T M``).  One GEMM forms ``M`` from the two
        cached Cholesky factors, ``HipBackend.nuclear_norm`` sums its singular values by ``iters`` Newton-Schulz steps on the GEMM
        (default: 60 in fp64, 40 in fp32) -- no eigendecomposition.  Two ``Diagonal`` variances take the closed form
        ``|m_s - m_o|^2 + sum (sqrt(a) - sqrt(b))^2`` without a factorisation.

        The factors are those of ``V + epsilon I`` (the library's jitter, ``B.epsilon``); the traces are taken without it.  For a
        singular covariance the result is therefore that of ``V + epsilon I``: off by up to about ``sqrt(epsilon lambda)`` per null
        direction, ``lambda`` the other covariance's size along it.

        Values only: with grad enabled, a mean or variance that carries a graph (a tensor that requires grad, a learnable kernel
        behind a lazy variance) is refused before any launch; under ``torch.no_grad()`` the value is returned."""
        if not isinstance(other, Normal):
            raise TypeError(f"w2 takes another Normal, got a {type(other).__name__}")
        from . import learnable
        refusal = ("gradients of w2 are not implemented: this call would return a value cut off from the autograd graph -- wrap it in "
                   "torch.no_grad() if that is intended")
        if learnable.normal_requires_grad(self) or learnable.normal_requires_grad(other):
            raise NotImplementedError(refusal)
        vs, vo = self.var, other.var
        if tuple(vs.shape) != tuple(vo.shape):
            raise ValueError(f"w2 between distributions of different shapes: variances {tuple(vs.shape)} and {tuple(vo.shape)}")
        ms, mo = self._mean_t, other._mean_t
        if torch.is_grad_enabled() and (ms.requires_grad or mo.requires_grad):       # (a graph that only shows once the mean exists)
            raise NotImplementedError(refusal)
        mean_part = ((ms - mo) ** 2).sum((-2, -1))
        if isinstance(vs, Zero):
            vs = Diagonal(vs.diag())
        if isinstance(vo, Zero):
            vo = Diagonal(vo.diag())
        if isinstance(vs, Diagonal) and isinstance(vo, Diagonal):
            var_part = ((torch.sqrt(vs.diag()) - torch.sqrt(vo.diag())) ** 2).sum(-1)
        else:
            if isinstance(vs, Diagonal):
                vs = Dense(vs.dense())
            if isinstance(vo, Diagonal):
                vo = Dense(vo.dense())
            be = ops.get_backend()
            # M = L_o^T L_s: both factors are stored K x M and vanish for k < their row index (clean lower triangles)
            m = be.gemm(vo.chol().lower(), vs.chol().lower(), a_kmajor=False, b_kmajor=False, tri_k=True)
            var_part = vs.diag().sum(-1) + vo.diag().sum(-1) - 2 * be.nuclear_norm(m, iters)
        # the sum is positive, but round-off may say otherwise (random.py:327-329)
        return torch.sqrt(torch.clamp(mean_part + var_part, min=0))

    # -- sampling (random.py:331-363; adjacent to the hot path) ----------------
    def sample(self, num=1, noise=None, generator=None, xi=None):
        """Samples as column vectors (..., N, num): ``chol(var) @ xi`` on the MFMA GEMM.

        ``xi``: the standard-normal draws to transform, (..., N, num) -- what ``B.randn`` produces inside the
        reference's ``B.sample`` (``random.py:351``); given, the result is a deterministic function of the
        distribution (used to compare samples with the oracle)."""
        var = self.var
        if xi is not None:
            if xi.dim() == 1:
                xi = xi[:, None]
            if xi.shape[-2] != self.dim:
                raise ValueError(f"xi has {xi.shape[-2]} rows, the distribution has dimension {self.dim}")
            num = xi.shape[-1]
        if isinstance(var, Diagonal):
            d = var.diag() + (noise if noise is not None else 0)
            if xi is None:
                xi = torch.randn(d.shape + (num,), dtype=d.dtype, device=d.device, generator=generator)
            out = torch.sqrt(d)[..., None] * xi
        else:
            graph = self._graph_matrix(var) is not None
            if noise is not None:
                if graph and torch.is_tensor(noise) and noise.requires_grad:
                    d = noise.to(dtype=var.dtype, device=var.device) * torch.ones(tuple(var.shape[:-1]), dtype=var.dtype, device=var.device)
                else:
                    d = torch.full(tuple(var.shape[:-1]), float(noise), dtype=var.dtype, device=var.device)
                var = var + Diagonal(d)
            if xi is None:
                xi = torch.randn(tuple(var.shape[:-1]) + (num,), dtype=var.dtype, device=var.device, generator=generator)
            mat = self._graph_matrix(var) if graph else None
            if mat is not None:
                # the covariance carries a graph: the same factorisation and product, recorded (the reparameterised sample)
                from .autograd import factor_times
                out = factor_times(mat, var.chol, xi.detach().to(var.dtype).contiguous())
            else:
                chol = var.chol() if isinstance(var, Dense) else to_matrix(var.dense()).chol()
                out = ops.get_backend().gemm(chol.lower(), xi.to(var.dtype), a_kmajor=True, b_kmajor=False)
        if not self.mean_is_zero:
            out = out + self._mean_t
        return out

    # -- arithmetic (random.py:365-393) ----------------------------------------
    def __add__(self, other):
        if isinstance(other, Normal):
            return Normal(self._mean_t + other._mean_t, self.var + other.var)
        if isinstance(other, Random):
            raise TypeError(f"cannot add a {type(other).__name__} to a Normal")
        return Normal(self._mean_t + other, self.var)

    def __mul__(self, other):
        if isinstance(other, Random):
            raise TypeError(f"cannot multiply a Normal by a {type(other).__name__}")
        return Normal(self._mean_t * other, Dense(self.var.dense() * (other * other)))

    def lmatmul(self, a):
        """Distribution of ``a @ x`` (``random.py:365-371``): mean ``a m``, variance ``a V a^T`` (two GEMMs)."""
        a = a.dense() if isinstance(a, AbstractMatrix) else a
        be = ops.get_backend()
        av = be.gemm(a, self.var.dense(), a_kmajor=True, b_kmajor=False)          # a V
        return Normal(be.gemm(a, self._mean_t, a_kmajor=True, b_kmajor=False), Dense(be.gemm(av, a, a_kmajor=True, b_kmajor=True)))

    def rmatmul(self, a):
        """Distribution of ``a^T @ x`` (``random.py:373-379``)."""
        a = a.dense() if isinstance(a, AbstractMatrix) else a
        return self.lmatmul(a.transpose(-1, -2).contiguous())
