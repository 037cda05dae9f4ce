"""GPU tests of agp_sparse_nll_gradient / SparseGaussianProcessRegression.log_likelihood_gradient.

Reference: the numpy restatement of tests/sparse_gradient_cases.py with Kt and dKt assembled from the CPU oracle's Gram
matrices (central differences of the Gram matrices in each parameter); g_ref is the plain dense gradient
1/2 <Kt^-1 - alpha alpha^T, dKt>.  Bound (the dense gradient tests' form, tests/test_nll_gradient_gpu.py):
|g - g_ref| <= 1e-7 s_p with s_p the sum of the absolute values of the terms of all three contractions, and
|nll - nll_ref| <= 1e-8 n.  The bound presumes errors of order eps cond, and the sparse formulas contain K_uu^-1
explicitly, so every accuracy case first asserts cond(K_uu) <= 1e6 and cond(Kt) <= 1e6: a condition on the inputs.
Each case prints its largest |g - g_ref| / s_p (recorded in DESIGN.md)."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from conftest import golden
from oracle import oracle_py as orc
from sparse_gradient_cases import (assemble_dkt, assemble_kt, dense_gradient, dense_nll, golden_model, structured_gradient,
                                   structured_weights)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def keyed_grouper(x, keys):
    lookup = {np.asarray(f, dtype=np.float64).tobytes(): int(k) for f, k in zip(x, keys)}
    return lambda f: lookup[np.asarray(f, dtype=np.float64).tobytes()]


def group_keys(layout, x, rng):
    n = len(x)
    first = x[:, 0] if x.ndim > 1 else x
    if layout == "uniform":      # equal groups: the lock-step path
        return np.arange(n) // 51
    if layout == "ragged":       # comparable sizes: the padded lock-step path
        return np.floor((first - first.min()) / (first.max() - first.min()) * 19.999).astype(np.int64)
    if layout == "uneven":       # 3 very uneven groups: one block at a time
        return np.where(np.arange(n) < 1000, 0, np.where(np.arange(n) < n - 30, 1, 2))
    if layout == "singletons":   # FITC
        return np.arange(n)
    raise KeyError(layout)


def sparse_model(ctx, cov, x, keys, u, mean=None, inducing_nugget=1e-6, measurement_nugget=1e-8):
    model = ab.sparse_gp_from_covariance_and_mean(cov, mean, keyed_grouper(x, keys), ab.FixedInducingPoints(u), "sparse", context=ctx)
    model.set_param("inducing_nugget", inducing_nugget)
    model.set_param("measurement_nugget", measurement_nugget)
    return model


def reference(model, ds, max_cond=1e6):
    """({name: d log p / d name}, {name: s_p}, log p, cond(K_uu), cond(Kt)) in numpy from the oracle's Gram matrices"""
    cov = model.covariance_function_
    xr, offsets, y, yv, u = model._components(ds)
    n, m = len(xr), len(u)

    def mats(c):
        return (orc.gram(c, xr, x_meas=True, threads=16), orc.gram(c, xr, u, x_meas=True, y_meas=False, threads=16),
                orc.gram(c, u, threads=16))

    Kff, Kfu, Kuu0 = mats(cov)
    Kuu = Kuu0 + model.inducing_nugget_ * np.eye(m)
    d = (yv if yv is not None else np.zeros(n)) + model.measurement_nugget_
    Kt = assemble_kt(Kff, Kfu, Kuu, d, offsets)
    cond_uu, cond_t = np.linalg.cond(Kuu), np.linalg.cond(Kt)
    if max_cond is not None:
        assert cond_uu <= max_cond and cond_t <= max_cond, (cond_uu, cond_t)
    weights = structured_weights(Kff, Kfu, Kuu, d, offsets, y)
    grads, scales = {}, {}
    zero_ff, zero_fu, zero_uu = np.zeros((n, n)), np.zeros((n, m)), np.zeros((m, m))
    for name, value in model.get_params().items():
        if name in cov.get_params():
            h = 1e-5 * max(1., abs(value))
            up, down = copy.deepcopy(cov), copy.deepcopy(cov)
            up.set_param(name, value + h)
            down.set_param(name, value - h)
            dKff, dKfu, dKuu = [(a - b) / (2 * h) for a, b in zip(mats(up), mats(down))]
            dd = np.zeros(n)
        elif name == "measurement_nugget":
            dKff, dKfu, dKuu, dd = zero_ff, zero_fu, zero_uu, np.ones(n)
        elif name == "inducing_nugget":
            dKff, dKfu, dKuu, dd = zero_ff, zero_fu, np.eye(m), np.zeros(n)
        else:  # a mean parameter: the sparse likelihood is evaluated on the targets as given (sparse_gp.hpp:664-668)
            grads[name], scales[name] = 0., 0.
            continue
        g = dense_gradient(Kt, y, assemble_dkt(Kfu, Kuu, offsets, dKff, dKfu, dKuu, dd))
        grads[name], scales[name] = -g, structured_gradient(weights, dKff, dKfu, dKuu, dd)[1]
    return grads, scales, -dense_nll(Kt, y), cond_uu, cond_t


def check(model, ds, label):
    ll, grad = model.log_likelihood_gradient(ds)
    assert set(grad) == set(model.get_params())
    assert ll == model.log_likelihood(ds)  # bit for bit what agp_sparse_nll returns
    want, scale, ll_ref, cond_uu, cond_t = reference(model, ds)
    worst = max((abs(grad[k] - want[k]) / scale[k] for k in want if scale[k] > 0.), default=0.)
    print(f"\n[sparse gradient] {label}: max |g - g_ref| / s_p = {worst:.3e}  cond(K_uu) = {cond_uu:.2e}  cond(Kt) = {cond_t:.2e}")
    for name in want:
        assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (name, grad[name], want[name], scale[name])
    n = len(ds.targets.mean)
    assert abs(ll - ll_ref) <= 1e-8 * n
    return ll, grad


def data_3d(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0., 10., (n, 3))
    y = np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0]) + 0.05 * rng.standard_normal(n)
    return rng, x, y


@pytest.mark.parametrize("layout", ["uniform", "ragged", "uneven", "singletons"])
@pytest.mark.parametrize("with_yvar", [False, True])
def test_se_noise_3d_all_layouts(ctx, layout, with_yvar):
    n, m = 1530, 96  # n not a multiple of 64, m not a multiple of 128
    rng, x, y = data_3d(n, 5)
    u = x[rng.choice(n, m, replace=False)]
    cov = ab.SquaredExponential(2.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.3))
    model = sparse_model(ctx, cov, x, group_keys(layout, x, rng), u)
    targets = ab.MarginalDistribution(y, rng.uniform(0.01, 0.05, n)) if with_yvar else y
    check(model, ab.RegressionDataset(x, targets), f"SE + noise 3-D, {layout}, y_var={with_yvar}")


@pytest.mark.parametrize("dim", [4, 5, 8])
def test_se_noise_padded_dimensions(ctx, dim):
    """The <4> and <8> instantiations of the contraction (5 dimensions are zero-padded to 8, the largest the feature check
    accepts).  n = 130 in ragged groups, m = 65: full and partial tiles of k(u, x) and k(u, u), group blocks smaller than
    a tile.  The points fill [0, 3]^dim, close enough for the covariance to couple them.  check() asserts cond(K_uu),
    cond(Kt) <= 1e6; for these inputs cond(K_uu) = 4.5e4, 3.7e3, 7.2e1 and cond(Kt) = 4.6e2, 3.5e2, 9.2e1 (numpy)."""
    n, m = 130, 65
    rng = np.random.default_rng(40 + dim)
    x = rng.uniform(0., 3., (n, dim))
    y = np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0]) + 0.05 * rng.standard_normal(n)
    u = x[rng.choice(n, m, replace=False)]
    cov = ab.SquaredExponential(2.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.3))
    model = sparse_model(ctx, cov, x, group_keys("ragged", x, rng), u)
    check(model, ab.RegressionDataset(x, y), f"SE + noise {dim}-D, ragged")


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_matern52_times_se_plus_noise(ctx, layout):
    n, m = 1530, 90
    rng, x, y = data_3d(n, 8)
    u = x[rng.choice(n, m, replace=False)]
    cov = ab.Matern52(3.0, 1.2) * ab.SquaredExponential(4.0, 0.9) + ab.IndependentNoise(0.2)
    check(sparse_model(ctx, cov, x, group_keys(layout, x, rng), u), ab.RegressionDataset(x, y), f"Matern52 * SE + noise, {layout}")


@pytest.mark.parametrize("layout", ["uniform", "uneven"])
def test_polynomial_plus_se_1d(ctx, layout):
    """the tree of the sinc example: Polynomial<1> + SquaredExponential + noise, 16 uniformly spaced inducing points"""
    rng = np.random.default_rng(9)
    n = 1530
    x = np.sort(rng.uniform(-10., 10., n))
    y = np.sinc(x / np.pi) + 0.1 * x + 0.1 * rng.standard_normal(n)
    cov = ab.Polynomial(1, 1.0) + ab.SquaredExponential(1.5, 1.0) + ab.measurement_only(ab.IndependentNoise(0.3))
    model = ab.sparse_gp_from_covariance(cov, keyed_grouper(x, group_keys(layout, x, rng)), ab.UniformlySpacedInducingPoints(16), "sparse",
                                         context=ctx)
    model.set_param("inducing_nugget", 1e-6)
    check(model, ab.RegressionDataset(x, y), f"Polynomial + SE 1-D, {layout}")


class Elevation(ab.ScalingFunction):
    _params = {"elevation_scaling_center": 4.0, "elevation_scaling_factor": 0.3}

    def get_name(self):
        return "elevation_scaling"

    def _call_impl(self, c):
        p = self.get_params()
        return 1. + p["elevation_scaling_factor"] * np.maximum(p["elevation_scaling_center"] - np.asarray(c)[:, 2], 0.)


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_scaling_term_and_linear_mean(ctx, layout):
    """a ScalingTerm (both tangent tables) with a LinearMean, whose parameters the sparse likelihood does not see"""
    n, m = 1530, 96
    rng, x, y = data_3d(n, 12)
    y = y + 0.3 * x[:, 0]
    u = x[rng.choice(n, m, replace=False)]
    cov = ab.ScalingTerm(Elevation()) * ab.Constant(0.5) + ab.Matern52(2.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.2))
    model = sparse_model(ctx, cov, x, group_keys(layout, x, rng), u, mean=ab.LinearMean())
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    ll, grad = check(model, ab.RegressionDataset(x, y), f"ScalingTerm + LinearMean, {layout}")
    assert grad["slope"] == 0. and grad["offset"] == 0.


def test_ill_conditioned_inducing_covariance(ctx):
    """Default nuggets (1e-8) and inducing points denser than the length scale; the LL^T path still succeeds.  No bound
    is fixed in advance: the error follows eps cond(K_uu) (include/albatross_amd.h).  Recorded on an MI355X (DESIGN.md,
    the sparse gradient's accuracy table) with cond(K_uu) = 5.75e8: max |g - g_ref| / s_p = 1.72e-7 against the numpy
    reference and 1.26e-5 max(1, |fd|) against central differences of agp_sparse_nll; the test allows ten times either."""
    rng = np.random.default_rng(4)
    n = 1530
    x = np.sort(rng.uniform(0., 10., n))
    y = np.sin(x) + 0.1 * rng.standard_normal(n)
    cov = ab.SquaredExponential(1.5, 1.0) + ab.measurement_only(ab.IndependentNoise(0.3))
    model = ab.sparse_gp_from_covariance(cov, keyed_grouper(x, group_keys("uniform", x, rng)), ab.UniformlySpacedInducingPoints(24), "sparse",
                                         context=ctx)
    ds = ab.RegressionDataset(x, y)
    ll, grad = model.log_likelihood_gradient(ds)
    assert np.isfinite(ll) and all(np.isfinite(v) for v in grad.values())
    want, scale, ll_ref, cond_uu, cond_t = reference(model, ds, max_cond=None)
    worst_ref = max(abs(grad[k] - want[k]) / scale[k] for k in want)
    worst_fd = 0.
    for name, value in cov.get_params().items():
        h = 1e-4 * max(1., abs(value))
        vals = []
        for v in (value + h, value - h):
            model.set_param(name, v)
            vals.append(model.log_likelihood(ds))
        model.set_param(name, value)
        fd = (vals[0] - vals[1]) / (2 * h)
        worst_fd = max(worst_fd, abs(grad[name] - fd) / max(1., abs(fd)))
    print(f"\n[sparse gradient] ill-conditioned: cond(K_uu) = {cond_uu:.2e}  max |g - g_ref| / s_p = {worst_ref:.3e}  "
          f"max |g - fd| / max(1, |fd|) = {worst_fd:.3e}")
    assert worst_ref <= 10 * 1.72e-7 and worst_fd <= 10 * 1.26e-5


def test_fit_outputs_equal_the_values_recorded_before_the_gradient_existed(ctx):
    rec = golden("sparse_fit_parent.json")
    for which in ("uniform_1d", "ragged_3d"):
        model, ds = golden_model(which, ctx)
        fit = model.fit(ds).get_fit()
        assert fit.nll == rec[which]["fit_nll"] and -model.log_likelihood(ds) == rec[which]["nll"]
        assert np.array_equal(fit.information, np.array(rec[which]["information"]))
        ll, _ = model.log_likelihood_gradient(ds)
        assert -ll == rec[which]["nll"]


def bench_like_model(ctx, n, m, gs, seed):
    """the benchmark's sparse workload (bench.py, config 5) at another size: 1-D, 16 points per unit length, SE(1, 1) +
    measurement-only noise(0.1), uniformly spaced inducing points, groups of gs neighbours"""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0., n / 16., n))
    y = np.sin(x) + 0.1 * np.cos(10. * x) + 0.1 * rng.standard_normal(n)
    cov = ab.SquaredExponential(1.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.1))
    u = np.linspace(x.min(), x.max(), m)

    def grouper(f):
        return np.searchsorted(x, np.asarray(f, dtype=np.float64).reshape(-1)) // gs
    grouper.vectorized = True
    model = ab.sparse_gp_from_covariance(cov, grouper, ab.FixedInducingPoints(u), "pitc", context=ctx)
    model.set_param_values({"inducing_nugget": 1e-3, "measurement_nugget": 1e-2})
    return model, ab.RegressionDataset(x, y)


def test_gradient_matches_central_differences_of_log_likelihood(ctx):
    """a size no dense reference reaches: n = 65536, m = 1024, groups of 512, the benchmark's covariance"""
    model, ds = bench_like_model(ctx, 65536, 1024, 512, 1)
    ll, grad = model.log_likelihood_gradient(ds)
    assert ll == model.log_likelihood(ds)
    for name, value in model.get_params().items():
        h = 1e-3 * value if "nugget" in name else 1e-4 * max(1., abs(value))
        vals = []
        for v in (value + h, value - h):
            model.set_param(name, v)
            vals.append(model.log_likelihood(ds))
        model.set_param(name, value)
        fd = (vals[0] - vals[1]) / (2 * h)
        print(f"\n[sparse gradient] n=65536 {name}: g = {grad[name]:.10e}  fd = {fd:.10e}")
        assert abs(grad[name] - fd) <= 1e-5 * max(1., abs(fd)), (name, grad[name], fd)


def raw_call(ctx, model, ds, n_slots=None, slots=None, with_tangents=True):
    """agp_sparse_nll_gradient through ctypes: (status, nll, grad, nuggets, alpha)"""
    cov = model.covariance_function_
    xr, offsets, y, yv, u = model._components(ds)
    fx, fu = cov.features(xr), cov.features(u)
    sx, su = fx.as_struct(), fu.as_struct()
    table_slots, columns = cov.param_slots()
    if slots is None:
        slots = [(node, p) for node, p, _ in table_slots]
    n_slots = len(slots) if n_slots is None else n_slots
    table = (capi.GradientSlot * max(1, len(slots)))(*[capi.GradientSlot(node, p) for node, p in slots])
    tx = tu = None
    if columns and with_tangents:
        tx, tu = np.empty((fx.n, len(columns)), order="F"), np.empty((fu.n, len(columns)), order="F")
        for c, (fn, name) in enumerate(columns):
            tx[:, c], tu[:, c] = fn.derivative(fx.coords, name), fn.derivative(fu.coords, name)
    nll = C.c_double(7.)
    grad, nug, alpha = np.full(max(1, len(slots)), 7.), np.full(2, 7.), np.full(fx.n, 7.)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    st = ctx._lib.agp_sparse_nll_gradient(ctx._h, ctx.kernel(cov), C.byref(sx), len(offsets) - 1, ptr(offsets), ptr(y), ptr(yv),
                                          C.byref(su), model.measurement_nugget_, model.inducing_nugget_, n_slots, table,
                                          ptr(tx), fx.n, ptr(tu), fu.n, C.byref(nll), ptr(grad), ptr(nug), ptr(alpha))
    return st, nll.value, grad, nug, alpha


def small_problem(ctx, layout="ragged", scaling=False):
    n, m = 700, 50
    rng, x, y = data_3d(n, 21)
    u = x[rng.choice(n, m, replace=False)]
    cov = ab.SquaredExponential(2.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.3))
    if scaling:
        cov = ab.ScalingTerm(Elevation()) * ab.Constant(0.5) + cov
    keys = np.floor(x[:, 0] / 0.7).astype(np.int64) if layout == "ragged" else np.arange(n) // 70
    return sparse_model(ctx, cov, x, keys, u), ab.RegressionDataset(x, y), x, u


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_gradient_is_deterministic_and_alpha_is_the_information_of_kt(ctx, layout):
    model, ds, x, u = small_problem(ctx, layout)
    a, b = raw_call(ctx, model, ds), raw_call(ctx, model, ds)
    assert a[0] == capi.AGP_OK and b[0] == capi.AGP_OK
    assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    cov = model.covariance_function_
    xr, offsets, y, yv, _ = model._components(ds)
    Kt = assemble_kt(orc.gram(cov, xr, x_meas=True), orc.gram(cov, xr, u, x_meas=True, y_meas=False),
                     orc.gram(cov, u) + model.inducing_nugget_ * np.eye(len(u)), np.full(len(xr), model.measurement_nugget_), offsets)
    want = np.linalg.solve(Kt, y)
    assert np.abs(a[4] - want).max() <= 1e-8 * np.abs(want).max()


def test_bad_slots_and_missing_tangents_are_rejected(ctx):
    model, ds, _, _ = small_problem(ctx, scaling=True)
    invalid = capi.AGP_ERR_INVALID_ARGUMENT
    assert raw_call(ctx, model, ds)[0] == capi.AGP_OK
    assert raw_call(ctx, model, ds, with_tangents=False)[0] == invalid       # a ScalingTerm slot without its tables
    assert raw_call(ctx, model, ds, slots=[(99, 0)])[0] == invalid           # no such node
    nodes, _ = model.covariance_function_.program()
    inner = next(i for i, nd in enumerate(nodes) if nd.op > capi.OP_SCALING)
    assert raw_call(ctx, model, ds, slots=[(inner, 0)])[0] == invalid        # not a leaf
    leaf = next(i for i, nd in enumerate(nodes) if nd.op == capi.OP_SQUARED_EXPONENTIAL)
    assert raw_call(ctx, model, ds, slots=[(leaf, 2)])[0] == invalid         # a parameter the leaf does not have
    assert raw_call(ctx, model, ds, n_slots=capi.MAX_GRADIENT_SLOTS + 1)[0] == invalid


def test_nan_input_and_singular_inducing_covariance(ctx):
    model, ds, x, u = small_problem(ctx)
    xbad = x.copy()
    xbad[5, 1] = np.nan
    model_bad = sparse_model(ctx, model.covariance_function_, xbad, np.arange(len(x)) // 70, u)
    st, nll, grad, nug, _ = raw_call(ctx, model_bad, ab.RegressionDataset(xbad, ds.targets.mean))
    assert st == capi.AGP_ERR_NAN_INPUT and np.isnan(nll) and np.isnan(grad).all() and np.isnan(nug).all()
    # a repeated inducing point with zero nugget: agp_sparse_fit_create would take the pivoted path, the gradient does not
    u2 = np.vstack([u, u[:1]])
    singular = sparse_model(ctx, model.covariance_function_, x, np.arange(len(x)) // 70, u2, inducing_nugget=0.)
    st, nll, grad, nug, _ = raw_call(ctx, singular, ds)
    assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and np.isnan(nll) and np.isnan(grad).all() and np.isnan(nug).all()


def test_cpp_sparse_gradient_matches_python(ctx):
    ex = os.path.join(ROOT, "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "sparse_gradient_check")], text=True)
    rows = {}
    for line in out.strip().splitlines():
        key, *vals = line.split(",")
        rows.setdefault(key, []).append(vals)
    data = np.array(rows["x"], dtype=float)
    x, y = data[:, 1:4], data[:, 4]
    cov = ab.ScalingTerm(Elevation()) * ab.Constant(0.5) + ab.Matern52(2.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.2))
    model = sparse_model(ctx, cov, x, np.floor(x[:, 0] / 0.7).astype(np.int64), x[::12])
    ll, grad = model.log_likelihood_gradient(ab.RegressionDataset(x, y))
    cpp = {k[len("grad_"):]: float(v[0][0]) for k, v in rows.items() if k.startswith("grad_")}
    assert set(cpp) == set(grad)
    assert abs(float(rows["loglik"][0][0]) - ll) <= 1e-10 * abs(ll)
    assert float(rows["loglik"][0][0]) == float(rows["loglik_plain"][0][0])
    for name in grad:
        assert abs(cpp[name] - grad[name]) <= 1e-10 * max(abs(grad[name]), 1e-3 * max(abs(g) for g in grad.values())), name
