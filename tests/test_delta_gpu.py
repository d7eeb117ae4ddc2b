"""The ``Delta`` kernel on the fused HIP path (MI355X): ``"delta"`` terms through ``HipBackend.kmat`` / ``kdiag`` and the two
kernel-gradient kernels against the longdouble reference of ``tests/delta_reference.py``, and noise as a process of its own,
``y = f + GP(v * Delta())``, end to end.

Inputs satisfy the condition stated in ``tests/delta_reference.py`` (no pair of points within a factor 4 of Delta's threshold; asserted
on the host before every launch), so a Delta value is exact in both dtypes:

* Delta-only matrices (and Delta beside a constant, with diagonal additions in eighths, accumulated into integers) are compared
  BIT FOR BIT;
* mixed sums, element by element: ``|got - ref| <= c eps sum_t |v_t kappa_t| (1 + |arg_t|)`` (+ ``|diag|`` / ``|what was there|`` where
  the launch adds those), ``c`` = ``VALUE_BOUND``: twice the worst ratio measured with these cases on an MI355X
  (``profiles/README.md``, "Delta kernel");
* kernel-gradient kernels: ``|got - ref| <= c eps absum`` as in ``tests/test_vjp_kernels_gpu.py``, ``c`` = ``VJP_BOUND`` measured the same
  way; the Delta term's ``S2`` and ``S3`` have nothing added up and must be exactly 0.

Kernels: ``d <= 8`` takes the row-band kernel, ``d = 9`` (past one staged chunk) the one-tile-per-workgroup kernel -- the switch the
release library offers; the native self-test (``gpk_selftest --delta``) forces each through the development knob as well."""
import numpy as np
import pytest
import torch

import stheno_amd.torch as st
from stheno_amd import ops
from stheno_amd.torch import EQ, Delta

from . import delta_reference as D
from . import vjp_reference as R

pytestmark = pytest.mark.gpu

DTYPES = {"float64": torch.float64, "float32": torch.float32}
#: twice the worst |got - ref| / (eps absum) measured over the mixed-sum cases below (profiles/README.md, "Delta kernel")
VALUE_BOUND = {"float64": 1.06, "float32": 1.05}                                            # measured 0.526, 0.523
#: ... and over the kernel-gradient cases, per output
VJP_BOUND = {
    ("logdensity", "S", "float64"): 0.28, ("logdensity", "S", "float32"): 0.33,             # measured 0.139, 0.164
    ("logdensity", "trace", "float64"): 0.62, ("logdensity", "trace", "float32"): 0.70,     # 0.305, 0.349
    ("logdensity", "diag", "float64"): 0.91, ("logdensity", "diag", "float32"): 1.29,       # 0.454, 0.644
    ("dense", "S", "float64"): 0.07, ("dense", "S", "float32"): 0.09,                       # 0.033, 0.040
    ("dense", "colsum", "float64"): 1.40, ("dense", "colsum", "float32"): 1.14,             # 0.695, 0.567
    ("dense", "gradx", "float64"): 0.66, ("dense", "gradx", "float32"): 0.72,               # 0.328, 0.356
}
TERMSETS = {"delta": D.DELTA1, "mix4": D.MIX4}
SHAPES = [(1, 1), (33, 65), (97, 259)]
DIMS = [1, 3, 8, 9]


def dev(a, dtype):
    return None if a is None else torch.as_tensor(np.array(a), dtype=DTYPES[dtype], device="cuda")


def worst_ratio(got, ref, absum, dtype):
    return float(np.max(R.ratios(got.double().cpu().numpy(), ref, absum, dtype)))


def accept(what, got, ref, absum, dtype, exact):
    """Bit for bit where the reference is exact, otherwise against ``VALUE_BOUND``; the figure is printed first."""
    g = got.double().cpu().numpy()
    assert g.shape == np.shape(ref), (what, g.shape, np.shape(ref))
    if exact:
        bad = int(np.sum(g != np.asarray(ref, dtype=np.float64)))
        print(f"{what} {dtype}: {bad} elements differ")
        assert bad == 0, what
    else:
        w = worst_ratio(got, ref, absum, dtype)
        print(f"{what} {dtype}: worst |got - ref| / (eps absum) = {w:.3f}")
        assert w <= VALUE_BOUND[dtype], (what, w)
    return g


def reference(name, x, y):
    terms, shapes = TERMSETS[name]
    D.check_inputs(terms, shapes, x, y)
    k, ab = D.kernel_matrix(terms, shapes, x, y, with_absum=True)
    return ops.KTerms(terms, shapes), k, ab


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", list(TERMSETS))
def test_rectangular_values_and_diagonal(hip_backend, name, d, dtype):
    for n, m in SHAPES:
        x, y = D.value_case(n, m, d)
        kt, ref, ab = reference(name, x, y)
        accept(f"kmat {name} {n}x{m} d{d}", hip_backend.kmat(kt, dev(x, dtype), dev(y, dtype)), ref, ab, dtype, name == "delta")
        diag = hip_backend.kdiag(kt, dev(x, dtype)).double().cpu().numpy()
        assert diag.shape == (n,) and np.all(diag == sum(v for _, v, _ in kt.terms))        # every term is 1 on the diagonal


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", list(TERMSETS))
def test_symmetric_lower_only_with_diag_vec(hip_backend, name, d, dtype):
    n = 130
    x, _ = D.value_case(n, None, d)
    kt, ref, ab = reference(name, x, None)
    dv = (np.arange(n) % 16) / 8.0
    full_ref, full_ab = ref + np.diag(0.25 + dv), ab + np.diag(0.25 + dv)
    tx = dev(x, dtype)
    full = hip_backend.kmat(kt, tx, None, diag_add=0.25, diag_vec=dev(dv, dtype))
    accept(f"kmat {name} symmetric {n} d{d}", full, full_ref, full_ab, dtype, name == "delta")
    assert float(full[3, 3]) == float(sum(v for _, v, _ in kt.terms) + 0.25 + dv[3])       # coincident points: exactly the variances
    low = hip_backend.kmat(kt, tx, None, lower=True, diag_add=0.25, diag_vec=dev(dv, dtype))
    assert torch.equal(torch.tril(low), torch.tril(full))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9], ids=["d3-row-band", "d9-tile"])
@pytest.mark.parametrize("name", list(TERMSETS))
def test_padded_view_batch_accumulate_and_nan(hip_backend, name, d, dtype):
    n, m = 33, 65
    x, y = D.value_case(n, m, d)
    kt, ref, ab = reference(name, x, y)
    tx, ty = dev(x, dtype), dev(y, dtype)
    exact = name == "delta"
    # ld > m: a view of a wider buffer (an odd leading dimension: rows off the 16-byte grid, the scalar store path), padding untouched
    buf = torch.full((n, m + 4), -7.0, dtype=DTYPES[dtype], device="cuda")
    out = hip_backend.kmat(kt, tx, ty, out=buf[:, :m])
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == m + 4
    accept(f"kmat {name} ld=m+4 d{d}", buf[:, :m], ref, ab, dtype, exact)
    assert bool((buf[:, m:] == -7.0).all())
    # accumulate into what is there (integers: the sum of a Delta-only launch stays exact)
    base = (np.arange(n * m).reshape(n, m) % 7 - 3).astype(np.float64)
    acc = dev(base, dtype)
    hip_backend.kmat(kt, tx, ty, out=acc, accumulate=True)
    accept(f"kmat {name} accumulate d{d}", acc, ref + base, ab + np.abs(base), dtype, exact)
    # a batch of two
    xb, yb = D.value_case(n, m, d, seed=1, batch=2)
    refs = [reference(name, xb[i], yb[i]) for i in range(2)]
    got = hip_backend.kmat(kt, dev(xb, dtype), dev(yb, dtype))
    accept(f"kmat {name} batch=2 d{d}", got, np.stack([r[1] for r in refs]), np.stack([r[2] for r in refs]), dtype, exact)
    # NaN in one input row: that row of the matrix is NaN, no other element is
    xn = np.array(x)
    xn[7, d - 1] = np.nan
    kn = hip_backend.kmat(kt, dev(xn, dtype), ty)
    assert bool(torch.isnan(kn[7]).all()) and not bool(torch.isnan(kn[:7]).any()) and not bool(torch.isnan(kn[8:]).any())
    keep = np.arange(n) != 7
    accept(f"kmat {name} rows beside the NaN row d{d}", kn[torch.as_tensor(keep, device="cuda")], ref[keep], ab[keep], dtype, exact)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_stretched_delta_through_the_kernel_algebra(hip_backend, dtype):
    """``v * Delta().stretch(s)`` beside a constant, scalar and per-dimension power-of-two scales: still exact."""
    terms, shapes = D.DELTA_STRETCHED
    x, y = D.value_case(97, 259, 3)
    D.check_inputs(terms, shapes, x, y)
    ref = D.kernel_matrix(terms, shapes, x, y)
    k = 1.5 * Delta().stretch(0.5) + 0.25 * st.OneKernel()
    assert k.terms() == terms and k.shapes() == shapes
    accept("Delta.stretch(0.5) + const", k.pairwise(dev(x, dtype), dev(y, dtype)), ref, None, dtype, True)
    scales = np.array([0.5, 2.0, 4.0])
    D.check_inputs(*D.DELTA1, x / scales, y / scales)
    ref = D.kernel_matrix(*D.DELTA1, x / scales, y / scales)
    accept("Delta.stretch(vector)", (1.5 * Delta()).stretch(scales).pairwise(dev(x, dtype), dev(y, dtype)), ref, None, dtype, True)


# ---------------------------------------------------------------------------------------------
# kernel-gradient kernels: Delta beside EQ and RQ
# ---------------------------------------------------------------------------------------------
def _accept_vjp(form, case_id, got, ref, dtype):
    worst = {}
    for k, (val, ab) in ref.items():
        if got[k] is None:
            continue
        g = got[k].cpu().numpy()
        assert g.shape == np.shape(val), (k, g.shape, np.shape(val))
        worst[k] = float(np.max(R.ratios(g, val, ab, dtype)))
    print(f"{form} {case_id} {dtype}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= VJP_BOUND[(form, k, dtype)], (k, v)
    delta_row = got["S"].cpu().numpy()[2]
    assert delta_row[1] == 0 and delta_row[2] == 0 and delta_row[0] != 0


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9])
@pytest.mark.parametrize("n", [33, 130])
def test_vjp_logdensity_form_with_a_delta_term(hip_backend, n, d, dtype):
    inp, ref = D.vjp_case("logdensity", n, None, d)
    kt = ops.KTerms(*D.VJP3)
    S, tr, dg = hip_backend.kmat_vjp(kt, dev(inp["x"], dtype), dev(inp["kinv"], dtype), dev(inp["alpha"], dtype), [float(v) for v in inp["g"]])
    _accept_vjp("logdensity", f"n{n}-d{d}", {"S": S, "trace": tr, "diag": dg}, ref, dtype)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [3, 9])
@pytest.mark.parametrize("n,m", [(33, 65), (130, 259), (33, 259), (130, 65)])
def test_vjp_dense_form_with_a_delta_term(hip_backend, n, m, d, dtype):
    inp, ref = D.vjp_case("dense", n, m, d)
    kt = ops.KTerms(*D.VJP3)
    gradx = d <= 8
    S, colsum, gx = hip_backend.kmat_vjp_dense(kt, dev(inp["x"], dtype), dev(inp["y"], dtype), dev(inp["g"], dtype), dev(inp["colscale"], dtype),
                                               dev(inp["w"], dtype), dev(inp["b"], dtype), want_colsum=True, want_gradx=gradx)
    assert (gx is not None) == gradx
    _accept_vjp("dense", f"n{n}-m{m}-d{d}", {"S": S, "colsum": colsum, "gradx": gx}, ref, dtype)


# ---------------------------------------------------------------------------------------------
# noise as a process of its own, end to end (fp64, n = 96, d = 2)
# ---------------------------------------------------------------------------------------------
N, NS, S2, EPS = 96, 12, 0.1, 1e-10


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    grid = rng.permutation(40 * 40)[: N + NS]
    pts = np.stack([grid // 40, grid % 40], axis=1) / 8.0            # distinct points on a grid of eighths
    x, xs = pts[:N], pts[N:].copy()
    xs[:3] = x[[5, 40, 77]]                                          # three test inputs repeat training inputs
    y = np.sin(x[:, :1]) * np.cos(x[:, 1:]) + 0.3 * rng.standard_normal((N, 1))
    return x, xs, y


@pytest.fixture()
def eps():
    old = st.B.epsilon
    st.B.epsilon = EPS
    yield
    st.B.epsilon = old


def _eq(a, b):
    return np.exp(-0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def _logpdf_np(k, y):
    l = np.linalg.cholesky(k)
    w = np.linalg.solve(l, y)
    return float(-0.5 * (2 * np.sum(np.log(np.diag(l))) + len(y) * np.log(2 * np.pi) + np.sum(w * w)))


def _t(a):
    return torch.tensor(np.array(a), dtype=torch.float64, device="cuda")


def test_noise_process_matches_the_noise_argument(hip_backend, eps, data):
    x, xs, y = data
    D.check_inputs(*D.DELTA1, x, xs, need_ones=False)
    with st.Measure() as prior:
        f = st.GP(EQ())
        e = st.GP(S2 * Delta())
        yp = f + e
    lp = float(yp(_t(x)).logpdf(_t(y)))
    lp_n = float(f(_t(x), S2).logpdf(_t(y)))
    want = _logpdf_np(_eq(x, x) + (S2 + EPS) * np.eye(N), y)
    print("logpdf: process", lp, "noise argument", lp_n, "numpy", want)
    assert abs(lp - lp_n) <= 1e-6 * abs(lp_n) and abs(lp - want) <= 1e-6 * abs(want)
    # posterior of the latent f at inputs that are not training inputs: the same as f | (f(x, s2), y)
    new = xs[3:]
    mean, var = (prior | (yp(_t(x)), _t(y)))(f)(_t(new)).marginals()
    mean_n, var_n = (f | (f(_t(x), S2), _t(y)))(_t(new)).marginals()
    for a, b in ((mean, mean_n), (var, var_n)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.max(np.abs(a - b)) <= 1e-6 * np.max(np.abs(b))


def test_predicting_y_at_repeated_inputs_shows_the_delta_cross_covariance(hip_backend, eps, data):
    x, xs, y = data
    with st.Measure() as prior:
        f = st.GP(EQ())
        yp = f + st.GP(S2 * Delta())
    post = prior | (yp(_t(x)), _t(y))
    mean_f, var_f = (a.cpu().numpy().ravel() for a in post(f)(_t(xs)).marginals())
    mean_y, var_y = (a.cpu().numpy().ravel() for a in post(yp)(_t(xs)).marginals())
    # dense NumPy: K = k_f(x, x) + s2 I; the cross-covariance of y(xs) with y(x) is k_f(xs, x) + s2 [xs_j == x_i]
    K = _eq(x, x) + (S2 + EPS) * np.eye(N)
    kf = _eq(xs, x)
    ky = kf + S2 * (((xs[:, None, :] - x[None, :, :]) ** 2).sum(-1) < 1e-6)
    assert ky[:3].sum() - kf[:3].sum() == pytest.approx(3 * S2) and np.array_equal(ky[3:], kf[3:])
    ref_var_f = 1.0 - np.einsum("ij,ij->i", kf, np.linalg.solve(K, kf.T).T)
    ref_var_y = 1.0 + S2 - np.einsum("ij,ij->i", ky, np.linalg.solve(K, ky.T).T)
    ref_mean_y = ky @ np.linalg.solve(K, y)[:, 0]
    print("var_y - var_f: got", (var_y - var_f)[:5], "expected", (ref_var_y - ref_var_f)[:5])
    scale = np.max(np.abs(ref_var_y))
    assert np.max(np.abs(var_f - ref_var_f)) <= 1e-6 * scale and np.max(np.abs(var_y - ref_var_y)) <= 1e-6 * scale
    assert np.max(np.abs((var_y - var_f) - (ref_var_y - ref_var_f))) <= 1e-6 * scale
    # at a new input the noisy prediction carries s2 on top; at a repeated one the observation pins y: variance ~ 0, mean = the datum
    assert np.max(np.abs((var_y - var_f)[3:] - S2)) <= 1e-6 * scale
    kinv_ii = np.diag(np.linalg.inv(K))[[5, 40, 77]]
    assert np.max(np.abs((var_y - var_f)[:3] + (S2 - S2**2 * kinv_ii))) <= 1e-6 * scale
    assert np.max(np.abs(mean_y - ref_mean_y)) <= 1e-6 * np.max(np.abs(ref_mean_y))
    assert np.max(np.abs(mean_y[:3] - y[[5, 40, 77], 0])) <= 1e-6 * np.max(np.abs(y))
    assert np.max(np.abs(mean_y[3:] - mean_f[3:])) <= 1e-6 * np.max(np.abs(ref_mean_y))


def test_delta_variance_gradient_of_the_log_density(hip_backend, eps, data):
    x, _, y = data
    v, sc = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (S2, 0.9))
    with st.Measure():
        lp = (st.GP(EQ().stretch(sc)) + st.GP(v * Delta()))(_t(x)).logpdf(_t(y))
    assert lp.requires_grad
    lp.backward()
    nz, sc_n = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (S2, 0.9))
    lp_n = st.GP(EQ().stretch(sc_n))(_t(x), nz).logpdf(_t(y))
    lp_n.backward()

    def obj(s2, l):
        return _logpdf_np(_eq(x / l, x / l) + (s2 + EPS) * np.eye(N), y)

    h = 1e-6
    fd_v = (obj(S2 + h, 0.9) - obj(S2 - h, 0.9)) / (2 * h)
    fd_l = (obj(S2, 0.9 + h) - obj(S2, 0.9 - h)) / (2 * h)
    print("d/dv: Delta", float(v.grad), "noise", float(nz.grad), "finite difference", fd_v, "| d/dscale:", float(sc.grad), float(sc_n.grad), fd_l)
    assert abs(float(lp.detach()) - float(lp_n.detach())) <= 1e-6 * abs(float(lp_n.detach()))
    assert abs(float(v.grad) - float(nz.grad)) <= 1e-6 * abs(float(nz.grad))
    assert abs(float(sc.grad) - float(sc_n.grad)) <= 1e-6 * abs(float(sc_n.grad))
    assert abs(float(v.grad) - fd_v) <= 1e-6 * max(abs(fd_v), 1.0) and abs(float(sc.grad) - fd_l) <= 1e-6 * max(abs(fd_l), 1.0)
