"""``Normal.w2`` on the HIP backend -- two factorisations, one GEMM for ``L_o^T L_s``, ``gpk_nuclear_norm`` -- against the reference's
dense double-root formula in fp64 on the CPU (``tests/test_w2_host.py``).  ``w2^2`` is compared relative to the scale
``|dm|^2 + tr V1 + tr V2`` at the project's parity bars: 1e-6 in fp64, 1e-3 in fp32 (with ``B.epsilon = 1e-6``, as the README
prescribes for fp32)."""
import numpy as np
import pytest
import torch

import stheno_amd as st

from .test_w2_host import kernel_pair, normal, sparse_posterior_distances, w2_squared_dense

pytestmark = pytest.mark.gpu

BAR = {torch.float64: 1e-6, torch.float32: 1e-3}
NP = {torch.float64: np.float64, torch.float32: np.float32}


@pytest.fixture()
def epsilon_for():
    def use(dtype):
        st.B.epsilon = 1e-6 if dtype == torch.float32 else 1e-12
    yield use
    st.B.epsilon = 1e-12


def _rounded_pair(n, dtype, seed):
    """A kernel-matrix pair as the device sees it: rounded to ``dtype``, handed back in fp64."""
    return tuple(a.astype(NP[dtype]).astype(np.float64) for a in kernel_pair(n, 0.1, seed=seed))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1, 33, 129, 300])
def test_against_the_dense_formula(hip_backend, epsilon_for, dtype, n):
    epsilon_for(dtype)
    m1, v1, m2, v2 = _rounded_pair(n, dtype, seed=n)
    want, scale = w2_squared_dense(m1, v1, m2, v2)
    d = normal(m1, v1, dtype, "cuda").w2(normal(m2, v2, dtype, "cuda"))
    got = float(d) ** 2
    print(f"w2^2 n={n} {dtype}: {got:.9e} against {want:.9e}, error {abs(got - want) / scale:.2e} of the scale")
    assert d.dtype == dtype and d.dim() == 0 and d.is_cuda
    assert abs(got - want) <= BAR[dtype] * scale


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_a_batch_of_three(hip_backend, epsilon_for, dtype):
    epsilon_for(dtype)
    cases = [_rounded_pair(40, dtype, seed=20 + i) for i in range(3)]
    stack = lambda k: np.stack([c[k] for c in cases])      # noqa: E731
    got = normal(stack(0), stack(1), dtype, "cuda").w2(normal(stack(2), stack(3), dtype, "cuda"))
    assert tuple(got.shape) == (3,)
    for i, c in enumerate(cases):
        want, scale = w2_squared_dense(*c)
        assert abs(float(got[i]) ** 2 - want) <= BAR[dtype] * scale
        one = normal(c[0], c[1], dtype, "cuda").w2(normal(c[2], c[3], dtype, "cuda"))
        assert abs(float(got[i]) ** 2 - float(one) ** 2) <= BAR[dtype] * scale


def test_fdd_spellings_and_self_distance(hip_backend):
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.uniform(-2, 2, (70, 2)), device="cuda")
    f, g = st.GP(1.3 * st.EQ().stretch(0.9)), st.GP(0.8 * st.EQ().stretch(1.7) + 0.5 * st.Linear())
    xn = x.cpu().numpy()
    sq = ((xn[:, None, :] - xn[None, :, :]) ** 2).sum(-1)
    v1 = 1.3 * np.exp(-0.5 * sq / 0.81) + 0.1 * np.eye(70)
    v2 = 0.8 * np.exp(-0.5 * sq / 1.7 ** 2) + 0.5 * (xn @ xn.T) + 0.2 * np.eye(70)
    zero = np.zeros((70, 1))
    want, scale = w2_squared_dense(zero, v1, zero, v2)
    p, q = f(x, 0.1), g(x, 0.2)
    assert abs(float(p.w2(q)) ** 2 - want) <= 1e-6 * scale
    assert abs(float(q.w2(p)) ** 2 - want) <= 1e-6 * scale
    assert float(p.w2(p)) < 5e-5                       # the reference's pin (tests/test_random.py:224)
    assert float(p.w2(f(x, 0.1))) < 5e-5               # ... and for an equal distribution with a factor of its own


def test_sparse_posterior_approaches_the_exact_one(hip_backend):
    d = sparse_posterior_distances("cuda")
    print("w2(sparse, exact) for 5, 10, 20, 40 inducing points:", d)
    assert d[0] > d[1] > d[2] > d[3] >= 0.0
    assert d[0] > 0.1 and d[3] < 1e-2 * d[0]


def test_a_learnable_length_scale_is_refused(hip_backend):
    x = torch.tensor(np.random.default_rng(4).uniform(-2, 2, (15, 2)), device="cuda")
    ls = torch.tensor(0.9, dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="gradients of w2 are not implemented"):
        st.GP(st.EQ().stretch(ls))(x, 0.1).w2(st.GP(st.EQ())(x, 0.2))
    with torch.no_grad():
        value = st.GP(st.EQ().stretch(ls))(x, 0.1).w2(st.GP(st.EQ())(x, 0.2))
    assert value.grad_fn is None and float(value) > 0.1
