"""One set of hyper-parameters per batch entry on the fused HIP path (MI355X): ``gpk_kmat_batch_terms`` / ``gpk_kdiag_batch_terms`` and
the model paths on top of them.

Kernel tests.  Entry ``b`` of a per-batch launch is compared BIT FOR BIT with ``gpk_kmat`` called unbatched on ``x[b]``, ``y[b]`` with
entry ``b``'s parameters: both run the same element program on the same numbers (the per-batch kernels derive ``1 / scale^2`` and
``1 / (2 alpha)`` in fp64 and round them to the dtype, as the host does for ``gpk_kmat``).  ``B = 3``; the three entries differ in every
column of the table; every parameter is a value fp32 holds exactly (scales and alphas are powers of two, so the inverse scales and
``1 / (2 alpha)`` are exact too).  Shapes: ``n, m`` in ``{1, 33, 130}`` (partial row tiles, a partial last lane vector, more than one
band), ``d`` in ``{1, 3, 8}`` (row-band launch) and ``9`` (one-tile launch).

Model tests.  ``B = 3, N = 70, N* = 9, D = 2``; fp64 to 1e-6, fp32 to 1e-3 of the reference value's scale (the project's parity bars):
the batched model with per-batch parameters against three unbatched models with scalar parameters, those against the CPU oracle
evaluated per entry (``oracle/gp_oracle.py``, its kernel matrix extended here by the rational-quadratic term), and the gradients of
``lp.sum()`` and of a weighted sum with distinct weights -- which a gradient routed to the wrong entry cannot pass -- against the
gradients of the three unbatched runs, stacked for per-batch parameters and summed for a shared one."""
import ctypes

import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from oracle import gp_oracle as O
from stheno_amd import _native, ops
from stheno_amd.torch import EQ, GP, RQ, Linear

pytestmark = pytest.mark.gpu

DTYPES = {"float64": torch.float64, "float32": torch.float32}
B = 3
SIZES = (1, 33, 130)

#: kind lists (name -> kinds) and, per kind, the three entries' (variance, scale, shape): all exact in fp32
KINDS = {
    "eq": ["eq"],
    "matern52": ["matern52"],
    "rq": ["rq"],
    "eq+linear": ["eq", "linear"],
    "generic3": ["matern32", "eq", "const"],
    "all8": ["eq", "matern12", "matern32", "matern52", "linear", "const", "rq", "delta"],
}
_VAR = {"eq": (1.25, 0.75, 2.5), "matern12": (0.5, 1.5, 0.25), "matern32": (0.75, 1.25, 0.375), "matern52": (1.5, 0.625, 1.125),
        "linear": (0.125, 0.25, 0.0625), "const": (0.25, 0.5, 0.75), "rq": (1.75, 0.875, 1.375), "delta": (0.5, 1.0, 2.0)}
_SCALE = {"eq": (2.0, 1.0, 0.5), "matern12": (1.0, 4.0, 2.0), "matern32": (0.5, 2.0, 1.0), "matern52": (4.0, 1.0, 2.0),
          "linear": (2.0, 4.0, 1.0), "const": (1.0, 2.0, 4.0), "rq": (1.0, 0.5, 2.0), "delta": (1.0, 2.0, 0.5)}
_SHAPE = {"rq": (2.0, 0.5, 4.0), "delta": (2.0 ** -20, 2.0 ** -18, 2.0 ** -22)}


def table(name):
    """``(per-batch KTerms, [the three entries' scalar KTerms])`` of a kind list."""
    kinds = KINDS[name]
    col = lambda vals: torch.tensor(vals, dtype=torch.float64, device="cuda")      # noqa: E731
    shaped = any(k in _SHAPE for k in kinds)
    batch = ops.KTerms([(k, col(_VAR[k]), col(_SCALE[k])) for k in kinds],
                       [col(_SHAPE[k]) if k in _SHAPE else None for k in kinds] if shaped else None)
    each = [ops.KTerms([(k, _VAR[k][b], _SCALE[k][b]) for k in kinds],
                       [_SHAPE[k][b] if k in _SHAPE else None for k in kinds] if shaped else None) for b in range(B)]
    assert batch.batch == B
    return batch, each


def points(n, m, d, dtype, seed=0):
    """``x`` (B, n, d) and ``y`` (B, m, d): fp32 values in both dtypes; some ``y`` rows repeat ``x`` rows (distance exactly 0: the Delta
    term is 1 there)."""
    g = torch.Generator().manual_seed(1000 * n + 10 * m + d + seed)
    x = torch.randn((B, n, d), generator=g, dtype=torch.float32)
    y = torch.randn((B, m, d), generator=g, dtype=torch.float32)
    r = min(n, m) // 2
    y[:, :r] = x[:, :r]
    return x.to(DTYPES[dtype]).cuda(), y.to(DTYPES[dtype]).cuda()


def same_bits(what, got, want):
    bad = int((got.view(torch.int64 if got.dtype == torch.float64 else torch.int32)
               != want.view(torch.int64 if want.dtype == torch.float64 else torch.int32)).sum())
    print(f"{what}: {bad} of {got.numel()} elements differ")
    assert got.shape == want.shape and bad == 0, what


# ---------------------------------------------------------------------------------------------
# gpk_kmat_batch_terms: every program, both launch shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [1, 3, 8, 9])
@pytest.mark.parametrize("name", list(KINDS))
def test_rectangular_entries_are_the_unbatched_launch(hip_backend, name, d, dtype):
    batch, each = table(name)
    for n in SIZES:
        for m in SIZES:
            if n == m:
                continue
            x, y = points(n, m, d, dtype)
            got = hip_backend.kmat(batch, x, y)
            assert got.shape == (B, n, m)
            want = torch.stack([hip_backend.kmat(each[b], x[b], y[b]) for b in range(B)])
            same_bits(f"{name} {n}x{m} d{d} {dtype}", got, want)
            assert bool(torch.isfinite(got).all())
    # the entries do differ: a launch that read entry 0's row everywhere would not pass the above
    assert not torch.equal(got[0], hip_backend.kmat(each[1], x[0], y[0]))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9], ids=["d3-row-band", "d9-tile"])
@pytest.mark.parametrize("name", list(KINDS))
def test_symmetric_variants(hip_backend, name, d, dtype):
    n = 130
    dt = DTYPES[dtype]
    batch, each = table(name)
    x, _ = points(n, 1, d, dtype)
    dv = ((torch.arange(B * n, dtype=torch.float64).reshape(B, n) % 16) / 8.0).to(dt).cuda()
    # lower triangle only, with diag_add and a diag_vec
    got = hip_backend.kmat(batch, x, None, lower=True, diag_add=0.25, diag_vec=dv)
    want = torch.stack([hip_backend.kmat(each[b], x[b], None, lower=True, diag_add=0.25, diag_vec=dv[b]) for b in range(B)])
    same_bits(f"{name} lower+diag d{d} {dtype}", torch.tril(got), torch.tril(want))
    # accumulate onto a filled buffer
    base = ((torch.arange(B * n * n, dtype=torch.float64).reshape(B, n, n) % 7) - 3.0).to(dt).cuda()
    acc = base.clone()
    hip_backend.kmat(batch, x, None, out=acc, accumulate=True)
    want = torch.stack([hip_backend.kmat(each[b], x[b], None, out=base[b].clone(), accumulate=True) for b in range(B)])
    same_bits(f"{name} accumulate d{d} {dtype}", acc, want)
    # out= a strided view inside a wider buffer: the guard cells around it stay
    buf = torch.full((B, n + 2, n + 5), -7.0, dtype=dt, device="cuda")
    view = buf[:, 1:n + 1, 2:n + 2]
    out = hip_backend.kmat(batch, x, None, out=view)
    assert out.data_ptr() == view.data_ptr()
    full = torch.stack([hip_backend.kmat(each[b], x[b], None) for b in range(B)])
    same_bits(f"{name} strided out d{d} {dtype}", view, full)
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[:, 1:n + 1, 2:n + 2] = False
    assert bool((buf[guard] == -7.0).all())
    # shared inputs: an expanded view, batch stride 0
    xe = x[0].expand(B, n, d)
    assert xe.stride(0) == 0
    got = hip_backend.kmat(batch, xe, None)
    want = torch.stack([hip_backend.kmat(each[b], x[0], None) for b in range(B)])
    same_bits(f"{name} expanded x d{d} {dtype}", got, want)


def _raw_tables(name, pad):
    """The three device tables of a kind list with ``pad`` unused columns behind every row (filled with NaN), and their stride."""
    kinds = KINDS[name]
    nt = len(kinds)

    def tab(values):
        t = torch.full((B, nt + pad), float("nan"), dtype=torch.float64)
        t[:, :nt] = torch.tensor(values, dtype=torch.float64).T
        return t.cuda()

    var = tab([_VAR[k] for k in kinds])
    ils = tab([[1.0 / s for s in _SCALE[k]] for k in kinds])
    shp = tab([_SHAPE.get(k, (0.0, 0.0, 0.0)) for k in kinds])
    ck = (ctypes.c_int * nt)(*[ops._KIND_IDS[k] for k in kinds])
    return ck, var, ils, shp, nt


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", ["eq", "all8"])
def test_padded_parameter_rows(hip_backend, name, dtype):
    """A parameter batch stride larger than ``nterms``: the padding (NaN here) is never read."""
    n, d, pad = 130, 3, 5
    x, _ = points(n, 1, d, dtype)
    _, each = table(name)
    ck, var, ils, shp, nt = _raw_tables(name, pad)
    out = torch.empty((B, n, n), dtype=DTYPES[dtype], device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    code = hip_backend.lib.gpk_kmat_batch_terms(
        ops._dtype_id(x), ck, ptr(var), ptr(ils), ptr(shp), nt, nt + pad, ptr(x), n, d, n * d, ptr(x), n, d, n * d, d,
        ptr(out), n, n * n, B, 0, 1, 0.0, ctypes.c_void_p(0), 0, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0
    want = torch.stack([hip_backend.kmat(each[b], x[b], None) for b in range(B)])
    same_bits(f"{name} padded rows {dtype}", out, want)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_kdiag_closed_form(hip_backend, dtype):
    """``gpk_kdiag_batch_terms`` against the closed form ``sum_t v_t[b] (linear: |x_i|^2 / s_t[b]^2, else 1)``: coordinates in
    quarters and the exact parameters above keep every operation exact in both dtypes."""
    n, d = 257, 3
    g = torch.Generator().manual_seed(5)
    x = (torch.randint(-8, 9, (B, n, d), generator=g).double() / 4.0)
    batch, _ = table("all8")
    got = hip_backend.kdiag(batch, x.to(DTYPES[dtype]).cuda())
    assert got.shape == (B, n)
    want = torch.zeros((B, n), dtype=torch.float64)
    for k in KINDS["all8"]:
        for b in range(B):
            want[b] += _VAR[k][b] * ((x[b] * x[b]).sum(-1) / _SCALE[k][b] ** 2 if k == "linear" else 1.0)
    assert torch.equal(got.double().cpu(), want)


def test_error_returns_without_a_launch(hip_backend):
    """Every documented error return of the two entries, once each; none of them reaches a launch (the pointers are never read)."""
    lib = hip_backend.lib
    p = ctypes.c_void_p(64)
    null = ctypes.c_void_p(0)

    def kmat(kinds, var=p, ils=p, shp=p, nterms=None, s_terms=None, n=4, m=4, batch=2, d=2):
        nt = len(kinds) if nterms is None else nterms
        ck = (ctypes.c_int * max(len(kinds), 1))(*kinds)
        return lib.gpk_kmat_batch_terms(_native.GPK_F64, ck, var, ils, shp, nt, nt if s_terms is None else s_terms, p, n, d, n * d,
                                        p, m, d, m * d, d, p, m, n * m, batch, 0, 0, 0.0, null, 0, 0, null)

    def kdiag(kinds, var=p, ils=p, shp=p, nterms=None, s_terms=None, batch=2):
        nt = len(kinds) if nterms is None else nterms
        ck = (ctypes.c_int * max(len(kinds), 1))(*kinds)
        return lib.gpk_kdiag_batch_terms(_native.GPK_F64, ck, var, ils, shp, nt, nt if s_terms is None else s_terms, p, 4, 2, 8, 2, p, 4,
                                         batch, null)

    eq, rq = _native.K_EQ, _native.K_RQ
    assert kmat([eq], n=0) == 0 and kdiag([eq], batch=0) == 0               # the empty problem
    assert kmat([eq], nterms=_native.MAX_TERMS + 1) == -4
    assert kmat([eq], nterms=-1) == -4
    assert kmat([eq], batch=65536) == -6
    assert kmat([eq], n=2 ** 31) == -6
    assert kmat([eq], d=-1) == -13
    assert kmat([8]) == -1                                                  # an unknown kind
    assert kmat([eq, rq], shp=null) == -1                                   # a shaped kind without a table of shapes
    assert kmat([eq], var=null) == -3
    assert kmat([eq], ils=null) == -3
    assert kmat([eq, eq], s_terms=1) == -7
    assert kdiag([eq], nterms=_native.MAX_TERMS + 1) == -4
    assert kdiag([rq], shp=null) == -1
    assert kdiag([eq], var=null) == -3
    assert kdiag([eq, eq], s_terms=1) == -7
    assert kdiag([eq], batch=65536) == -6
    assert lib.gpk_version() >= 107


def test_batch_size_mismatch_names_both_sizes(hip_backend):
    batch, _ = table("eq")
    x = torch.randn((4, 5, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=r"batch of 3 .* batch of 4"):
        hip_backend.kmat(batch, x, None)
    with pytest.raises(ValueError, match=r"batch of 3 .* batch of 4"):
        hip_backend.kdiag(batch, x)


# ---------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------
N, NS, D = 70, 9, 2
TOL = {"float64": 1e-6, "float32": 1e-3}
EPS = {"float64": 1e-12, "float32": 1e-6}
V0, L0, A0, W0 = (1.3, 0.7, 2.1), (0.6, 1.1, 1.9), (0.8, 1.7, 3.5), 0.3
WEIGHTS = (1.0, -2.0, 0.5)


@pytest.fixture(params=list(DTYPES))
def setting(request, hip_backend):
    old = st.B.epsilon
    st.B.epsilon = EPS[request.param]
    yield request.param
    st.B.epsilon = old


def data(dtype, shared=False):
    g = torch.Generator().manual_seed(11)
    x = torch.randn((1 if shared else B, N, D), generator=g, dtype=torch.float64)
    y = torch.randn((B, N, 1), generator=g, dtype=torch.float64)
    xs = torch.randn((B, NS, D), generator=g, dtype=torch.float64)
    noise = 0.1 + torch.rand((B, N), generator=g, dtype=torch.float64)
    return tuple(t.to(DTYPES[dtype]).cuda() for t in (x, y, xs, noise))


def leaves(dtype, grad=True):
    dt = DTYPES[dtype]
    pb = lambda vals: torch.tensor(vals, dtype=dt, device="cuda").reshape(B, 1, 1).requires_grad_(grad)      # noqa: E731
    return pb(V0), pb(L0), pb(A0), torch.tensor(W0, dtype=dt, device="cuda", requires_grad=grad)


def model(v, l, a, w, period=None):
    k = v * EQ().stretch(l) + RQ(a) + w * Linear()
    return GP(k.periodic(period) if period is not None else k)


def entry(t, b, grad=False):
    """Entry ``b`` of a per-batch leaf as a scalar leaf of its own."""
    return t.detach()[b].reshape(()).clone().requires_grad_(grad)


def close(what, got, ref, dtype):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print(f"{what} {dtype}: max error {err:.3e}, scale {scale:.3e}")
    assert got.shape == ref.shape and err <= TOL[dtype] * scale, what


def oracle_kernel(b, x, y=None):
    """The CPU oracle's kernel matrix of entry ``b``'s model, its rational-quadratic term added in NumPy."""
    terms = [("eq", V0[b], L0[b]), ("linear", W0, 1.0)]
    y = x if y is None else y
    return O.kernel_matrix(terms, x, y) + np.exp(-A0[b] * np.log1p(O.pw_dists2(x, y) / (2.0 * A0[b])))


def oracle_entry(b, x, noise, y, xs, eps):
    """``(logpdf, posterior mean, marginal variances)`` of entry ``b`` from the CPU oracle's pieces."""
    kx = oracle_kernel(b, x) + np.diag(noise)
    lp = O.normal_logpdf(None, kx, y, eps)
    chol = O.cholesky(kx, eps)
    v = O.solve_lower(chol, oracle_kernel(b, x, xs))
    mean = (v.T @ O.solve_lower(chol, y))[:, 0]
    var = np.diag(oracle_kernel(b, xs)) - np.sum(v * v, axis=0)
    return float(lp), mean, np.maximum(var, 0)


def test_spelling_per_batch_variance_gives_one_density_per_entry(setting):
    dt = DTYPES[setting]
    x, y, _, _ = data(setting)
    v = torch.full((B, 1, 1), 1.0, dtype=dt, device="cuda", requires_grad=True)
    lp = GP(v * EQ())(x, 0.1).logpdf(y)
    assert lp.shape == (B,) and lp.requires_grad
    lp.sum().backward()
    assert v.grad.shape == (B, 1, 1) and bool(torch.isfinite(v.grad).all())


def test_values_against_unbatched_models_and_the_oracle(setting):
    x, y, xs, noise = data(setting)
    v, l, a, w = leaves(setting, grad=False)
    f = model(v, l, a, w)
    with torch.no_grad():
        lp = f(x, noise).logpdf(y)
        mean, var = (f | (f(x, noise), y))(xs).marginals()
        pair, kd = f.kernel.pairwise(x, xs), f.kernel.elwise(xs)
    assert lp.shape == (B,) and mean.shape[0] == B and var.shape[0] == B
    for b in range(B):
        fb = model(*(entry(t, b) for t in (v, l, a)), w)
        with torch.no_grad():
            lpb = fb(x[b], noise[b]).logpdf(y[b])
            mb, vb = (fb | (fb(x[b], noise[b]), y[b]))(xs[b]).marginals()
            assert torch.equal(pair[b], fb.kernel.pairwise(x[b], xs[b])) and torch.equal(kd[b], fb.kernel.elwise(xs[b]))
        close(f"logpdf[{b}] batched vs unbatched", lp[b].cpu(), lpb.cpu(), setting)
        close(f"mean[{b}] batched vs unbatched", mean[b].cpu().reshape(-1), mb.cpu().reshape(-1), setting)
        close(f"var[{b}] batched vs unbatched", var[b].cpu().reshape(-1), vb.cpu().reshape(-1), setting)
        npy = lambda t: t.double().cpu().numpy()      # noqa: E731
        olp, om, ov = oracle_entry(b, npy(x[b]), npy(noise[b]), npy(y[b]), npy(xs[b]), EPS[setting])
        close(f"logpdf[{b}] unbatched vs oracle", lpb.cpu(), olp, setting)
        close(f"mean[{b}] unbatched vs oracle", mb.cpu().reshape(-1), om, setting)
        close(f"var[{b}] unbatched vs oracle", vb.cpu().reshape(-1), ov, setting)


def _gradients(setting, weights, shared=False, period=None):
    """Gradients of ``(weights * lp).sum()`` of the batched model, and of the three unbatched runs: stacked, and summed for ``w``."""
    x, y, _, noise = data(setting, shared=shared)
    x.requires_grad_()
    noise.requires_grad_()
    xb = x.expand(B, N, D) if shared else x
    v, l, a, w = leaves(setting)
    lp = model(v, l, a, w, period)(xb, noise).logpdf(y)
    (torch.tensor(weights, dtype=lp.dtype, device="cuda") * lp).sum().backward()
    got = dict(v=v.grad, l=l.grad, a=a.grad, w=w.grad, x=x.grad, noise=noise.grad)
    assert v.grad.shape == l.grad.shape == a.grad.shape == (B, 1, 1)
    ref = dict(v=[], l=[], a=[], w=[], x=[], noise=[], lp=[])
    for b in range(B):
        vb, lb, ab = (entry(t, b, True) for t in (v, l, a))
        wb = w.detach().clone().requires_grad_()
        xb_ = x.detach()[0 if shared else b].clone().requires_grad_()
        nb = noise.detach()[b].clone().requires_grad_()
        lpb = model(vb, lb, ab, wb, period)(xb_, nb).logpdf(y[b])
        (weights[b] * lpb).backward()
        for key, t in dict(v=vb, l=lb, a=ab, w=wb, x=xb_, noise=nb).items():
            ref[key].append(t.grad)
        ref["lp"].append(lpb.detach())
    close("logpdf", lp.detach().cpu(), torch.stack(ref["lp"]).cpu(), setting)
    for key in ("v", "l", "a"):
        close(f"d/d{key}", got[key].reshape(-1).cpu(), torch.stack(ref[key]).cpu(), setting)
    close("d/dw (shared: summed)", got["w"].cpu(), torch.stack(ref["w"]).sum(0).cpu(), setting)
    close("d/dnoise", got["noise"].cpu(), torch.stack(ref["noise"]).cpu(), setting)
    xref = torch.stack(ref["x"]).sum(0, keepdim=True) if shared else torch.stack(ref["x"])
    close("d/dx", got["x"].cpu(), xref.cpu(), setting)


@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0), WEIGHTS], ids=["sum", "weighted"])
def test_gradients_against_unbatched_runs(setting, weights):
    _gradients(setting, weights)


def test_gradients_with_shared_expanded_inputs(setting):
    _gradients(setting, WEIGHTS, shared=True)


def test_gradients_behind_a_periodic_map(setting):
    _gradients(setting, WEIGHTS, period=3.0)
