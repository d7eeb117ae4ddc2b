"""Every differentiable path behind the admission layer (``stheno_amd/learnable.py``), scenario by scenario, under a recording wrapper
around the active backend: what a host-side change in front of the autograd functions must leave as it is -- the ORDER and the SHAPES
of the backend calls, the refusals, and every value and gradient BIT FOR BIT.

    python scripts/dump_learnable.py OUT.npz [--backend host|hip] [--trace TRACE.json]     # dump
    python scripts/dump_learnable.py A.npz B.npz                                           # compare two dumps (exit status 1 on a difference)

The script uses the public API only (``GP``, ``Measure``, ``PseudoObs``, ``.logpdf``, ``.elbo``, ``post(xs).mean`` ...) and the package
of the tree it lies in: run it at two commits and compare.  ``--backend host`` (the default) runs on the test-only NumPy backends of
``tests/`` (``GroupsOracle``; ``BlockOracle`` for the models of ``tests/block_posterior_cases.py``, which need the Matern kinds;
``BatchOracle`` for the batched posteriors of ``tests/batch_posterior_cases.py``, which need ``kmat_vjp_dense_batch``);
``--backend hip`` on ``libgpk.so``.  The dump holds, per scenario, the values and every gradient as raw bytes, the exception type of a
refusal, and the trace: the backend methods in the order they were called, each with the shapes of its tensor arguments and the
optional arguments it was given.  ``--trace`` writes the traces and exception types alone, as JSON: the machine-independent part of a
host run (``tests/golden/learnable_backend_trace.json``, recorded before the admission layer moved into one module -- the entries of
``LATER_SCENARIOS`` before the autograd functions came to share their stages --, is what ``tests/test_learnable_trace_host.py`` replays
against).

Shapes: N = 70 observations (one 64-wide tile and a partial one), N* = 9 test points, M = 13 inducing points, d = 2 or 3 (1 under the
net of the function-scaled scenarios), a batch of 3; every
scenario draws its data from a generator with a fixed seed.  The ``rows_*`` scenarios (a posterior predicted before anything
factorised: the cross-covariance rides through the factorisation as rows under the matrix, ``WhitenedT``) run at N = 130 with
``matrix.config.posterior_rows_from`` / ``posterior_rows_min_points`` lowered to 128 / 8 for their duration."""
import inspect
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stheno_amd.torch as st  # noqa: E402
from stheno_amd import ops  # noqa: E402
from stheno_amd.matrix import config  # noqa: E402
from stheno_amd.torch import EQ, RQ, Linear  # noqa: E402
from tests import batch_posterior_cases as BP  # noqa: E402
from tests import block_posterior_cases as BC  # noqa: E402
from tests import function_product_cases as FP  # noqa: E402
from tests import input_maps_cases as IC  # noqa: E402
from tests import map_groups_cases as MC  # noqa: E402
from tests import posterior_cov_cases as PC  # noqa: E402

N, NS, M = 70, 9, 13
NB = 3                       # (the batch of the batched scenarios)
NR = 130                     # (the rows-path scenarios: an order the factorisation with rows takes once its thresholds are lowered)
NOISE = 0.3
DEV = ["cpu"]


def T(a, grad=False):
    """A tensor on the device of the run."""
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=DEV[0], requires_grad=grad)


def P(v):
    """A learnable scalar hyper-parameter (on the host, like every scalar hyper-parameter)."""
    return torch.tensor(float(v), dtype=torch.float64, requires_grad=True)


def data(seed, d=2, n=N):
    rng = np.random.default_rng(seed)
    x, xs, z = rng.uniform(-2.0, 2.0, (n, d)), rng.uniform(-2.0, 2.0, (NS, d)), rng.uniform(-2.0, 2.0, (M, d))
    y = np.sin(x[:, :1]) + 0.3 * rng.standard_normal((n, 1))
    return x, xs, z, y


# ---------------------------------------------------------------------------------------------
# the recording wrapper
# ---------------------------------------------------------------------------------------------
def describe(v):
    if torch.is_tensor(v):
        return "T" + "x".join(str(s) for s in v.shape) + ("~0" if v.dim() == 2 and v.shape[0] > 1 and v.stride(0) == 0 else "")
    if isinstance(v, ops.KTerms):
        return "terms(" + ",".join(t[0] for t in v.terms) + ("|shapes" if v.shapes is not None else "") + ")"
    if v is None or isinstance(v, (bool, int, str)):
        return repr(v)
    if isinstance(v, float):
        return "float"
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(describe(e) for e in v) + "]"
    return type(v).__name__


def _defaults(fn):
    """The default values in the signature of ``fn``, by parameter name."""
    try:
        params = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return {}
    return {p.name: p.default for p in params if p.default is not inspect.Parameter.empty}


class Recorder:
    """Delegates everything to ``inner`` and keeps ``calls``: one line per method called from outside the backend.  An optional argument
    given as None is not listed; with ``drop_defaults`` neither is one given at the default value of the wrapped method's signature:
    leaving it out is the same call."""

    def __init__(self, inner, drop_defaults=False):
        self._inner, self.calls, self._drop = inner, [], drop_defaults

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if name.startswith("_") or not callable(attr):
            return attr
        defaults = _defaults(attr)

        def is_default(k, v):
            return self._drop and k in defaults and type(v) is type(defaults[k]) and isinstance(v, (bool, int, float, str)) and v == defaults[k]

        def call(*args, **kw):
            given = [describe(a) for a in args] + [f"{k}={describe(v)}" for k, v in sorted(kw.items()) if v is not None and not is_default(k, v)]
            self.calls.append(f"{name}({', '.join(given)})")
            return attr(*args, **kw)

        return call


def install(which, drop_defaults=False):
    """Install the recording wrapper (``Recorder(backend, drop_defaults)``) around the backend ``which`` (``"hip"``, or the name of a host
    backend); returns ``(recorder, previous backend)``."""
    if which == "hip":
        prev = ops.set_backend(None)
        rec = Recorder(ops.get_backend(), drop_defaults)
        ops.set_backend(rec)                      # (it answers to the name "hip": installed as it is)
        return rec, prev
    from tests.test_batch_posterior_grad_host import BatchOracle
    from tests.test_map_groups_grad_host import GroupsOracle

    prev = ops.set_backend({"groups": GroupsOracle, "block": BC.BlockOracle, "batch": BatchOracle}[which]())
    rec = Recorder(ops.get_backend(), drop_defaults)      # around the host wrapper that serves the Delta kind and the derivative blocks, so
    ops._backend = rec                            # that those are recorded too (`set_backend` would put a second one around it)
    return rec, prev


# ---------------------------------------------------------------------------------------------
# scenarios: each returns (outputs, leaves[, loss])
# ---------------------------------------------------------------------------------------------
def _gp1():
    v, s = P(1.2), P(0.9)
    return v * EQ().stretch(s), dict(v=v, s=s)


def logpdf_one_group():
    x, _, _, y = data(1)
    k, t = _gp1()
    return st.GP(k)(T(x), NOISE).logpdf(T(y)), t


def logpdf_one_group_dx():
    x, _, _, y = data(2)
    k, t = _gp1()
    tx = T(x, True)
    return st.GP(k)(tx, NOISE).logpdf(T(y)), dict(t, x=tx)


def _three(learn, dx):
    x, _, y, _ = MC.data()
    k, t = MC.three_group_kernel(learn=learn)
    tx, ty, noise = T(x[:N], dx), T(y[:N], True), P(NOISE)
    leaves = dict({n: leaf for n, leaf in t.items() if leaf.requires_grad}, y=ty, noise=noise)
    if dx:
        leaves["x"] = tx
    return st.GP(k)(tx, noise).logpdf(ty), leaves


def logpdf_three_groups_implicit():
    return _three(MC.PLAIN, False)


def logpdf_three_groups_dense():
    return _three(MC.NAMES, True)


def logpdf_per_point_noise():
    x, _, _, y = data(3)
    k, t = _gp1()
    nz = T(np.random.default_rng(33).uniform(0.1, 0.4, N), True)
    return st.GP(k)(T(x), nz).logpdf(T(y)), dict(t, noise=nz)


def logpdf_dense_noise():
    x, _, _, y = data(4)
    k, t = _gp1()
    a = np.random.default_rng(44).standard_normal((N, 3))
    nm = T(0.2 * np.eye(N) + 0.02 * a @ a.T, True)
    return st.GP(k)(T(x), nm).logpdf(T(y)), dict(t, noise=nm)


def logpdf_two_columns():
    x, _, _, y = data(5)
    k, t = _gp1()
    ty = T(np.concatenate([y, y[::-1]], axis=1), True)
    return st.GP(k)(T(x), NOISE).logpdf(ty), dict(t, y=ty)


def logpdf_rq_table():
    x, _, _, y = data(6, d=3)
    a, v, s = P(0.8), P(0.5), P(1.3)
    return st.GP(v * RQ(a).stretch(s) + 0.4 * EQ())(T(x), NOISE).logpdf(T(y)), dict(alpha=a, v=v, s=s)


def _batch(dx, per_batch=False):
    rng = np.random.default_rng(7)
    xb, yb = rng.uniform(-2.0, 2.0, (NB, N, 2)), rng.standard_normal((NB, N, 1))
    v, s = (T(np.reshape([1.2, 0.7, 1.9], (NB, 1, 1)), True) if per_batch else P(1.2)), P(0.9)
    txb, tyb, nzb = T(xb, dx), T(yb, True), T(rng.uniform(0.1, 0.4, (NB, N)), True)
    leaves = dict(v=v, s=s, y=tyb, noise=nzb)
    if dx:
        leaves["x"] = txb
    return st.GP(v * EQ().stretch(s) + 0.3 * Linear())(txb, nzb).logpdf(tyb), leaves


def logpdf_batch():
    return _batch(False)


def logpdf_batch_dx():
    return _batch(True)


def logpdf_batch_variance_per_entry():
    return _batch(False, per_batch=True)


def logpdf_batch_variance_per_entry_dx():
    return _batch(True, per_batch=True)


def _scaled(learn_fn):
    """``(1 + a) * net + b`` of ``tests/function_product_cases.py`` (one input dimension: the net's): a function-scaled group beside a
    plain one."""
    x, y = FP.modulated_data(N)
    p = FP.net_params()
    net = FP.TanhNet(p, DEV[0]).requires_grad_(learn_fn)
    f, _, _, _, t = FP.modulated_model(p, net, DEV[0])
    if learn_fn:
        t = dict(t, w1=net.l1.weight, b1=net.l1.bias, w2=net.l2.weight, b2=net.l2.bias)
    return f(T(x), t["noise"]).logpdf(T(y)[:, None]), t


def logpdf_scaled_learnable_function():
    return _scaled(True)


def logpdf_scaled_constant_function():
    return _scaled(False)


def _joint(learn_period):
    x, _, y, _ = MC.data()
    prior, f, f2, t = MC.joint_model()
    if not learn_period:
        t["period"].requires_grad_(False)
        del t["period"]
    na = N - NS
    lp = prior.logpdf((f(T(x[:na]), MC.NOISE), T(y[:na])), (f2(T(x[na:N]), MC.NOISE_B), T(y[na:N])))
    return lp, t


def joint_two_processes():
    return _joint(False)


def joint_learnable_period():
    return _joint(True)


def joint_lag():
    d = IC.data()
    prior, f, g, t = IC.model_b()
    return prior.logpdf((f(T(d["xa"]), IC.NOISE), T(d["ya"])), (g(T(d["xb"][:M]), IC.NOISE_B), T(d["yb"][:M]))), t


def joint_equal_maps_given_twice():
    """A diagonal block whose two maps are equal but distinct objects (``k.transform(fn, fn)``), the map learnable."""
    d = IC.data()
    fn, v = IC.FeatureMap(device=DEV[0]), P(1.1)
    with st.Measure() as prior:
        f1 = st.GP(v * EQ().transform(fn, fn))
        f = f1 + st.GP(0.7 * EQ())
    x, y = d["x"], d["y"]
    lp = prior.logpdf((f(T(x[:N - NS]), IC.NOISE), T(y[:N - NS])), (f1(T(x[N - NS:N]), IC.NOISE_B), T(y[N - NS:N])))
    return lp, dict(v=v, w1=fn.w1, b1=fn.b1, w2=fn.w2)


def _bound(cls, seed):
    x, _, z, y = data(seed)
    v1, s1, v2, s2 = P(1.1), P(0.9), P(0.4), P(1.6)
    tx, tz, ty, nz = T(x, True), T(z, True), T(y, True), T(np.random.default_rng(seed).uniform(0.1, 0.4, N), True)
    f = st.GP(v1 * EQ().stretch(s1) + v2 * Linear().stretch(s2))
    return cls(f(tz), f(tx, nz), ty).elbo(f.measure), dict(v1=v1, s1=s1, v2=v2, s2=s2, x=tx, z=tz, y=ty, noise=nz)


def elbo_vfe():
    return _bound(st.PseudoObs, 8)


def elbo_dtc():
    return _bound(st.PseudoObsDTC, 9)


def elbo_fitc():
    return _bound(st.PseudoObsFITC, 10)


def elbo_stationary_only():
    x, _, z, y = data(11, d=3)
    v, ls = P(1.1), T([0.8, 1.3, 1.7], True)
    tz = T(z, True)
    f = st.GP(v * EQ().stretch(ls))
    return st.PseudoObs(f(tz), f(T(x), NOISE), T(y)).elbo(f.measure), dict(v=v, l=ls, z=tz)


def rows_path(fn):
    """``fn`` with the thresholds of the factorisation with rows under the matrix lowered to the shapes used here (as
    ``tests/test_round6_rhs.py`` lowers them): a posterior predicted before anything factorised takes the ``WhitenedT`` path."""
    def scenario():
        old = (config.posterior_rows_from, config.posterior_rows_min_points)
        config.posterior_rows_from, config.posterior_rows_min_points = 128, 8
        try:
            return fn()
        finally:
            config.posterior_rows_from, config.posterior_rows_min_points = old

    scenario.__name__ = fn.__name__
    return scenario


def _exact(seed, what, dx=False, dxs=False, logpdf_first=False, two_groups=False, n=N, dy=True):
    x, xs, _, y = data(seed, n=n)
    v, s = P(1.2), P(0.9)
    k, t = v * EQ().stretch(s) + 0.3 * Linear(), dict(v=v, s=s)
    if two_groups:
        p = P(3.1)
        k, t = k + 0.7 * EQ().periodic(p), dict(t, period=p)
    tx, txs, ty = T(x, dx), T(xs, dxs), T(y, dy)
    if dy:
        t["y"] = ty
    if dx:
        t["x"] = tx
    if dxs:
        t["xs"] = txs
    f = st.GP(k)
    fdd = f(tx, NOISE)
    outs = []
    if logpdf_first:
        outs.append(fdd.logpdf(ty))
    post = f | (fdd, ty)
    if what == "mean":
        outs.append(post(txs).mean)
    elif what == "var":
        t.pop("y", None)
        outs.append(post(txs).var_diag)
    else:
        outs += list(post(txs).marginals())
    return tuple(outs), t


def exact_mean_only():
    return _exact(12, "mean")


def exact_var_only():
    return _exact(13, "var")


def exact_both_dx_dxs():
    return _exact(14, "both", dx=True, dxs=True)


def exact_mean_dxs():
    return _exact(15, "mean", dxs=True)


def exact_two_groups():
    return _exact(16, "both", dxs=True, two_groups=True)


def exact_after_logpdf():
    return _exact(17, "both", logpdf_first=True)


@rows_path
def rows_both_residual_rides():
    return _exact(24, "both", dxs=True, n=NR, dy=False)


@rows_path
def rows_mean_only():
    return _exact(25, "mean", n=NR)


@rows_path
def rows_var_only():
    return _exact(26, "var", dxs=True, n=NR)


@rows_path
def rows_block_component_of_a_sum():
    return _block("decomposition", NR)


def _block(case, n1=N):
    Pm = BC.leaves(case, dict(n1=n1, n2=M, ns=NS), torch.float64, DEV[0])
    mean, var = BC.ours(case, Pm)
    leaves = {k: Pm[k] for k in list(BC.HYPER[case]) + [d for d in BC.DATA_LEAVES if d in BC.USES[case]]}
    return (mean, var), leaves, BC.loss(mean, var, Pm["w"])


def block_component_of_a_sum():
    return _block("decomposition")


def block_two_observation_sets():
    return _block("two_observed")


def block_values_and_slopes():
    return _block("values_slopes")


def block_slope_predicted():
    return _block("slope")


def _batch_exact(seed, what, model="rq", dx=False, dxs=False):
    """A batch of exact posteriors under shared hyper-parameters, per-point noise: the models of ``tests/batch_posterior_cases.py``."""
    p, _ = BP.values(model, NB, N, NS, 2, True, seed)
    names = ["lv", "ls", "lnoise"] + list(BP.MODELS[model][2]) + ["y"] * (what != "var") + ["x"] * dx + ["xs"] * dxs
    Pm = {k: T(p[k], k in names) for k in p}
    f = st.GP(BP.MODELS[model][0](Pm))
    fdd = (f | (f(Pm["x"], torch.exp(Pm["lnoise"])), Pm["y"]))(Pm["xs"])
    outs = (fdd.mean,) if what == "mean" else (fdd.var_diag,) if what == "var" else tuple(fdd.marginals())
    return outs, {k: Pm[k] for k in names}


def batch_exact_mean_only():
    return _batch_exact(27, "mean")


def batch_exact_var_only():
    return _batch_exact(28, "var")


def batch_exact_both_dx_dxs():
    return _batch_exact(29, "both", dx=True, dxs=True)


def batch_exact_two_groups():
    return _batch_exact(30, "both", model="two_groups", dxs=True)


def _covariance(seed, kinds=("eq", "linear"), dx=False, dxs=False, n=N):
    """The joint posterior covariance under a fixed cotangent: the models of ``tests/posterior_cov_cases.py``."""
    p, fixed = PC.make(kinds, n=n, ns=NS, d=2, seed=seed)
    names = ["lv", "lnoise"] + (["l12", "lp"] if kinds == PC.TWO_GROUP else ["ls"]) + ["x"] * dx + ["xs"] * dxs
    Pm = PC.leaves(p, names, torch.float64, DEV[0])
    loss, cov = PC.ours(kinds, Pm, "var", {k: T(v) for k, v in fixed.items()}, False)
    return (cov,), {k: Pm[k] for k in names}, loss


def covariance_parameters_only():
    return _covariance(31)


def covariance_dx_dxs():
    return _covariance(32, dx=True, dxs=True)


def covariance_two_groups():
    return _covariance(33, kinds=PC.TWO_GROUP, dxs=True)


@rows_path
def rows_covariance():
    return _covariance(34, dxs=True, n=NR)


def _sparse(cls, seed, what, only_xs=False):
    x, xs, z, y = data(seed)
    g = not only_xs
    v, s = torch.tensor(1.1, dtype=torch.float64, requires_grad=g), torch.tensor(0.9, dtype=torch.float64, requires_grad=g)
    tx, tz, txs, ty = T(x, g), T(z, g), T(xs, True), T(y, g)
    nz = T(np.random.default_rng(seed).uniform(0.1, 0.4, N), g)
    f = st.GP(v * EQ().stretch(s) + 0.3 * Linear())
    post = f | cls(f(tz), f(tx, nz), ty)
    outs = (post(txs).mean,) if what == "mean" else tuple(post(txs).marginals())
    leaves = dict(xs=txs) if only_xs else dict(v=v, s=s, x=tx, z=tz, xs=txs, y=ty, noise=nz)
    return outs, leaves


def sparse_vfe_mean_only():
    return _sparse(st.PseudoObs, 18, "mean")


def sparse_fitc_both():
    return _sparse(st.PseudoObsFITC, 19, "both")


def sparse_dtc_both():
    return _sparse(st.PseudoObsDTC, 20, "both")


def sparse_xs_the_only_leaf():
    return _sparse(st.PseudoObs, 21, "both", only_xs=True)


def _slopes(**grad):
    rng = np.random.default_rng(9)
    t = lambda a, name: T(a, grad.get(name, False))      # noqa: E731
    x1, x2, xs = t(rng.uniform(-1, 1, (N, 2)), "x1"), t(rng.uniform(-1, 1, (M, 2)), "x2"), t(rng.uniform(-1, 1, (NS, 2)), "xs")
    y1, y2 = t(rng.standard_normal((N, 1)), "y1"), t(rng.standard_normal((M, 1)), "y2")
    scales = torch.tensor([0.8, 1.3], dtype=torch.float64, device=DEV[0], requires_grad=grad.get("scales", False))
    with st.Measure() as prior:
        f = st.GP(EQ().stretch(scales) if grad.get("scales") else EQ().stretch(0.9))
        df = f.diff(1)
    return prior | ((f(x1, 0.1), y1), (df(x2, 0.1), y2)), f, df, xs


def refuse_input_gradient_of_a_mixed_block():
    post, f, df, xs = _slopes(xs=True, y1=True)
    return tuple(post(df)(xs).marginals()), {}


def refuse_per_dimension_scales_behind_a_derivative():
    post, f, df, xs = _slopes(scales=True)
    return tuple(post(f)(xs).marginals()), {}


def refuse_logpdf_of_a_learnable_posterior():
    x, xs, z, y = data(22)
    v = P(1.0)
    f = st.GP(v * EQ())
    post = f | st.PseudoObs(f(T(z)), f(T(x), 0.1), T(y))
    return post(T(xs), 0.1).logpdf(T(y[:NS])), {}


def refuse_learnable_map_under_a_pseudo_point_posterior():
    d = IC.data()
    prior, f, g, t = IC.model_b()
    post = prior | st.PseudoObs(f(T(d["xt"][:M])), f(T(d["xa"]), IC.NOISE), T(d["ya"]))
    return post(g)(T(d["xb"][:NS]), IC.NOISE_B).logpdf(T(d["yb"][:NS])), {}


def refuse_derivative_under_a_joint_logpdf():
    x, _, _, y = data(23)
    v = P(1.1)
    with st.Measure() as prior:
        f = st.GP(v * EQ())
        df = f.diff(0)
    return prior.logpdf((f(T(x), 0.1), T(y)), (df(T(x[:M]), 0.1), T(y[:M]))), {}


SCENARIOS = [(fn.__name__, host, fn) for host, fn in [
    ("groups", logpdf_one_group), ("groups", logpdf_one_group_dx), ("groups", logpdf_three_groups_implicit),
    ("groups", logpdf_three_groups_dense), ("groups", logpdf_per_point_noise), ("groups", logpdf_dense_noise),
    ("groups", logpdf_two_columns), ("groups", logpdf_rq_table), ("groups", logpdf_batch), ("groups", logpdf_batch_dx),
    ("groups", joint_two_processes), ("groups", joint_learnable_period), ("groups", joint_lag), ("groups", joint_equal_maps_given_twice),
    ("groups", elbo_vfe), ("groups", elbo_dtc), ("groups", elbo_fitc), ("groups", elbo_stationary_only),
    ("groups", exact_mean_only), ("groups", exact_var_only), ("groups", exact_both_dx_dxs), ("groups", exact_mean_dxs),
    ("groups", exact_two_groups), ("groups", exact_after_logpdf),
    ("block", block_component_of_a_sum), ("block", block_two_observation_sets), ("block", block_values_and_slopes),
    ("block", block_slope_predicted),
    ("groups", rows_both_residual_rides), ("groups", rows_mean_only), ("groups", rows_var_only),
    ("block", rows_block_component_of_a_sum),
    ("groups", sparse_vfe_mean_only), ("groups", sparse_fitc_both), ("groups", sparse_dtc_both), ("groups", sparse_xs_the_only_leaf),
    ("groups", refuse_input_gradient_of_a_mixed_block), ("groups", refuse_per_dimension_scales_behind_a_derivative),
    ("groups", refuse_logpdf_of_a_learnable_posterior), ("groups", refuse_learnable_map_under_a_pseudo_point_posterior),
    ("groups", refuse_derivative_under_a_joint_logpdf),
]]

#: the scenarios added when the autograd functions came to share their stages.  Their traces do not list an optional argument given at
#: its default (``Recorder(..., drop_defaults=True)``): one function leaves ``want_gradx`` out where another passes False for the same
#: launch.  The scenarios above keep the listing their fixture entries were recorded with.
LATER_SCENARIOS = [(fn.__name__, host, fn) for host, fn in [
    ("groups", logpdf_scaled_learnable_function), ("groups", logpdf_scaled_constant_function),
    ("batch", batch_exact_mean_only), ("batch", batch_exact_var_only), ("batch", batch_exact_both_dx_dxs), ("batch", batch_exact_two_groups),
    ("groups", covariance_parameters_only), ("groups", covariance_dx_dxs), ("groups", covariance_two_groups), ("groups", rows_covariance),
    ("groups", logpdf_batch_variance_per_entry), ("groups", logpdf_batch_variance_per_entry_dx),
]]


# ---------------------------------------------------------------------------------------------
def raw(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def run_scenario(name, host, fn, backend="host"):
    """``(trace, arrays)`` of one scenario: ``trace`` = ``{"calls": [...], "raises": exception type or None}``."""
    rec, prev = install("hip" if backend == "hip" else host, drop_defaults=any(name == later for later, _, _ in LATER_SCENARIOS))
    old = st.B.epsilon
    st.B.epsilon = MC.EPS
    arrays, raised = {}, None
    try:
        try:
            got = fn()
        except (NotImplementedError, ValueError) as exc:
            raised = type(exc).__name__
        else:
            outs, leaves = got[0], got[1]
            outs = outs if isinstance(outs, tuple) else (outs,)
            loss = got[2] if len(got) > 2 else sum(o.sum() for o in outs)
            for i, o in enumerate(outs):
                arrays[f"{name}/value{i}"] = raw(o)
            loss.backward()
            for key, leaf in leaves.items():
                assert leaf.grad is not None, (name, key)
                arrays[f"{name}/d_{key}"] = raw(leaf.grad)
    finally:
        st.B.epsilon = old
        ops.set_backend(prev)
    return dict(calls=rec.calls, raises=raised), arrays


def dump(path, backend, trace_path):
    DEV[0] = "cuda" if backend == "hip" else "cpu"
    traces, out = {}, {}
    for name, host, fn in SCENARIOS + LATER_SCENARIOS:
        traces[name], arrays = run_scenario(name, host, fn, backend)
        out.update(arrays)
    if backend == "hip":
        torch.cuda.synchronize()
    out["__traces__"] = np.frombuffer(json.dumps(traces, sort_keys=True).encode(), dtype=np.uint8)
    np.savez(path, **out)
    if trace_path:
        with open(trace_path, "w") as fh:
            json.dump(traces, fh, indent=0, sort_keys=True)
            fh.write("\n")
    print(f"{len(SCENARIOS + LATER_SCENARIOS)} scenarios, {len(out) - 1} arrays, {sum(len(t['calls']) for t in traces.values())} backend calls -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        if name == "__traces__":
            ta, tb = (json.loads(bytes(d[name]).decode()) for d in (a, b))
            bad += [f"trace of {s}" for s in sorted(set(ta) | set(tb)) if ta.get(s) != tb.get(s)]
        elif a[name].shape != b[name].shape or a[name].dtype != b[name].dtype or a[name].tobytes() != b[name].tobytes():
            bad.append(name)
    print(f"{len(SCENARIOS + LATER_SCENARIOS)} scenarios, {len(a.files) - 1} / {len(b.files) - 1} arrays compared, {len(bad)} differ" + "".join(f"\n  {n}" for n in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {}
    for flag in ("--backend", "--trace"):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i: i + 2]
    if len(args) == 1 and opts.get("--backend", "host") in ("host", "hip"):
        dump(args[0], opts.get("--backend", "host"), opts.get("--trace"))
    elif len(args) == 2 and not opts:
        sys.exit(compare(args[0], args[1]))
    else:
        sys.exit(__doc__)
