"""Every output and every gradient of the differentiable paths on the test-only host backends, as raw fp64 in one ``.npz``: what a
host-side change of ``kernels.py`` / ``learnable.py`` / ``autograd.py`` must leave equal BIT FOR BIT.

    python scripts/dump_autograd_values.py OUT.npz            # dump
    python scripts/dump_autograd_values.py A.npz B.npz        # compare two dumps (exit status 1 when an entry differs)

Run it at the two commits and compare.  The models are those of ``tests/map_groups_cases.py`` on the ``GroupsOracle`` backend of
``tests/test_map_groups_grad_host.py`` (log-density of three groups with every gradient and without learnable maps, one group plain /
behind a learnable period / behind learnable per-dimension scales / under moving inputs, one group with a learnable RQ alpha, the joint
log-density of a sum process and its periodic part, posterior marginals, the predictive density) and, on ``OracleBackend``, one VFE, one
FITC and one DTC bound with an ``EQ + Linear`` kernel at N = 60, M = 12, D = 2, and a batched log-density.  No GPU is needed."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd.torch as st  # noqa: E402
from stheno_amd import ops  # noqa: E402
from stheno_amd.torch import EQ, RQ, Linear  # noqa: E402
from tests import map_groups_cases as C  # noqa: E402
from tests.conftest import OracleBackend  # noqa: E402
from tests.test_map_groups_grad_host import GroupsOracle  # noqa: E402


def T(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


def raw(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float64, copy=False))


def put(out, name, value, leaves):
    """``value`` and the gradient of every leaf in ``leaves`` (a dict name -> tensor) after ``value.sum().backward()``."""
    out[name + "/value"] = raw(value)
    value.sum().backward()
    for key, leaf in leaves.items():
        assert leaf.grad is not None, (name, key)
        out[f"{name}/d_{key}"] = raw(leaf.grad)


def map_group_models(out):
    x, xs, y, ys = C.data()

    k, t = C.three_group_kernel()
    tx, ty, noise = T(x, True), T(y, True), T(C.NOISE, True)
    put(out, "logpdf3", st.GP(k)(tx, noise).logpdf(ty), dict(t, x=tx, y=ty, noise=noise))

    k, t = C.three_group_kernel(learn=C.PLAIN)
    ty, noise = T(y, True), T(C.NOISE, True)
    put(out, "logpdf3_plain", st.GP(k)(T(x), noise).logpdf(ty), dict({n: t[n] for n in C.PLAIN}, y=ty, noise=noise))

    v, s = T(1.2, True), T(0.9, True)
    put(out, "logpdf1", st.GP(v * EQ().stretch(s))(T(x), C.NOISE).logpdf(T(y)), dict(v=v, s=s))
    p = T(3.1, True)
    put(out, "logpdf1_period", st.GP(1.2 * EQ().periodic(p))(T(x), C.NOISE).logpdf(T(y)), dict(p=p))
    ls = T([0.8, 1.7], True)
    put(out, "logpdf1_scales", st.GP(1.2 * EQ().stretch(ls))(T(x), C.NOISE).logpdf(T(y)), dict(l=ls))
    tx = T(x, True)
    put(out, "logpdf1_inputs", st.GP(1.2 * EQ().stretch(0.9))(tx, C.NOISE).logpdf(T(y)), dict(x=tx))
    a, v, s = T(0.8, True), T(0.5, True), T(1.3, True)
    put(out, "logpdf1_alpha", st.GP(v * RQ(a).stretch(s) + 0.4 * EQ())(T(x), C.NOISE).logpdf(T(y)), dict(alpha=a, v=v, s=s))
    ty = T(np.concatenate([y, y[::-1]], axis=1), True)
    v = T(1.2, True)
    put(out, "logpdf1_two_columns", st.GP(v * EQ().stretch(0.9))(T(x), C.NOISE).logpdf(ty), dict(v=v, y=ty))

    prior, f, f2, t = C.joint_model()
    lp = prior.logpdf((f(T(x[:C.NA]), C.NOISE), T(y[:C.NA])), (f2(T(x[C.NA:]), C.NOISE_B), T(y[C.NA:])))
    put(out, "joint", lp, t)

    k, t = C.three_group_kernel()
    f = st.GP(k)
    tx, txs = T(x, True), T(xs, True)
    fdd = (f | (f(tx, C.NOISE), T(y)))(txs)
    put(out, "marginals3", torch.stack([fdd.mean.sum(), fdd.var_diag.sum()]), dict(t, x=tx, xs=txs))

    k, t = C.three_group_kernel()
    f = st.GP(k)
    put(out, "predictive3", (f | (f(T(x), C.NOISE), T(y)))(T(xs), C.NOISE).logpdf(T(ys)), t)

    # a learnable shape parameter through the pseudo-point bound (this backend knows the rational quadratic), inputs fixed
    a, v = T(0.7, True), T(1.3, True)
    f = st.GP(v * RQ(a).stretch(1.2) + 0.2 * EQ())
    put(out, "elbo_vfe_alpha", st.PseudoObs(f(T(x[:12])), f(T(x[:60]), T(np.full(60, C.NOISE))), T(y[:60])).elbo(f.measure), dict(alpha=a, v=v))


def pseudo_point_bounds(out):
    rng = np.random.default_rng(72)
    n, m, d = 60, 12, 2
    x, z, y = rng.standard_normal((n, d)), rng.standard_normal((m, d)), rng.standard_normal((n, 1))
    nz0 = rng.uniform(0.1, 0.4, n)
    for method, cls in (("vfe", st.PseudoObs), ("fitc", st.PseudoObsFITC), ("dtc", st.PseudoObsDTC)):
        v1, s1, v2, s2 = T(1.1, True), T(0.9, True), T(0.4, True), T(1.6, True)
        tx, tz, ty, nz = T(x, True), T(z, True), T(y, True), T(nz0, True)
        f = st.GP(v1 * EQ().stretch(s1) + v2 * Linear().stretch(s2))
        put(out, f"elbo_{method}", cls(f(tz), f(tx, nz), ty).elbo(f.measure), dict(v1=v1, s1=s1, v2=v2, s2=s2, x=tx, z=tz, y=ty, noise=nz))
    # a batch of data sets under shared hyper-parameters
    xb, yb = rng.standard_normal((3, 40, d)), rng.standard_normal((3, 40, 1))
    v, s = T(1.2, True), T(0.9, True)
    txb, tyb, nzb = T(xb, True), T(yb, True), T(rng.uniform(0.1, 0.4, (3, 40)), True)
    put(out, "logpdf_batched", st.GP(v * EQ().stretch(s) + 0.3 * Linear())(txb, nzb).logpdf(tyb), dict(v=v, s=s, x=txb, y=tyb, noise=nzb))


def dump(path):
    out = {}
    old = st.B.epsilon
    st.B.epsilon = C.EPS
    try:
        for backend, models in ((GroupsOracle(), map_group_models), (OracleBackend(), pseudo_point_bounds)):
            prev = ops.set_backend(backend)
            try:
                models(out)
            finally:
                ops.set_backend(prev)
    finally:
        st.B.epsilon = old
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        if a[name].shape != b[name].shape or a[name].tobytes() != b[name].tobytes():
            bad.append(name)
    print(f"{len(a.files)} / {len(b.files)} arrays, {len(bad)} differ" + "".join(f"\n  {n}" for n in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2:
        dump(sys.argv[1])
    elif len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
