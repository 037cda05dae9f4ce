"""GPU tests of the leave-one-out likelihood metric and its exact gradient: agp_loo_nll_gradient,
GaussianProcessRegression.leave_one_out_likelihood_gradient and LeaveOneOutLikelihood, and of the G^T G kernel.

Reference: numpy, independent of the library.  K = orc.gram(measurement features) + diag(s), C = K^-1,
alpha = C (y - mu); the value and W = C diag(b) C - 1/2 (u alpha^T + alpha u^T) by the closed form that
tests/test_loo_gradient_host.py checks against brute-force refits.  dK / dtheta is a central difference of orc.gram
at theta +- h, h = 1e-5 max(1, |theta|); mean terms -u^T dmu / dtheta with central differences of orc.mean_vector.

Tolerance: |g - g_ref| <= 1e-7 s_p with s_p = sum |S o dK| + sum |sym(u alpha^T) o dK| (S = C diag(b) C), the sum of
the magnitudes of the terms the gradient adds up, which does not cancel.  The library's gradient is exact to fp64
rounding: C carries a relative error ~ eps cond(K) (cond ~ 1e4 ... 1e6 here: <= 1e-10), and S, u and b carry it on
into every term.  The reference's own error is that of the central difference: truncation h^2 |d^3 K| / 6 ~ 1e-10
relative and cancellation eps |K| / h ~ 1e-11 relative per entry.  1e-7 leaves two to three orders of magnitude over
both, while a gradient that drops a term, a factor 2 off the diagonal, b's s-term or a leaf's chain rule is off by
O(1) s_p."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from conftest import synthetic_3d
from oracle import oracle_py as orc
from test_nll_gradient_gpu import LEAVES, _data, _elevation_model, _FirstCoordinateMean, _padded_data, perturbed

pytestmark = pytest.mark.gpu

LOG_2PI = np.log(2 * np.pi)


def closed_form(K, r, s):
    """(value, S = C diag(b) C, u, alpha) of the leave-one-out metric for K (target variance included)"""
    C_ = np.linalg.inv(K)
    C_ = 0.5 * (C_ + C_.T)
    alpha = C_ @ r
    c = np.diag(C_)
    v = 1. / c + s
    d = alpha / c
    value = 0.5 * np.sum(np.log(v) + d * d / v + LOG_2PI)
    b = (1. - d * d / v + 2. * alpha * d) / (2. * v * c * c)
    u = C_ @ (d / (v * c))
    S = (C_ * b[:, None]).T @ C_
    return value, S, u, alpha


def brute_force(K, r, s):
    """sum_i NLL_i of n refits that each leave point i out, scored with its variance s_i added"""
    n = len(r)
    total = 0.
    for i in range(n):
        rest = np.arange(n) != i
        w = np.linalg.solve(K[np.ix_(rest, rest)], K[rest, i])
        v = K[i, i] - w @ K[rest, i] + s[i]
        dev = r[i] - w @ r[rest]
        total += 0.5 * (np.log(v) + dev * dev / v + LOG_2PI)
    return total


def reference(model, x, y, s, threads=16, brute=False):
    """({name: d LOO / d name}, {name: s_p}, LOO value[, brute-force value]) in numpy from the oracle's Gram matrices"""
    cov, mean = model.covariance_function_, model.mean_function_
    sv = np.zeros(len(y)) if s is None else s
    K = orc.gram(cov, x, x_meas=True, threads=threads) + np.diag(sv)
    r = np.asarray(y, dtype=np.float64) - orc.mean_vector(mean, cov, x)
    value, S, u, alpha = closed_form(K, r, sv)
    sym = 0.5 * (np.outer(u, alpha) + np.outer(alpha, u))
    grads, scales = {}, {}
    cov_names = cov.get_params()
    for name, val in model.get_params().items():
        h = 1e-5 * max(1., abs(val))
        (cov_up, mean_up), (cov_down, mean_down) = perturbed(model, name, val + h), perturbed(model, name, val - h)
        if name in cov_names:
            dK = (orc.gram(cov_up, x, x_meas=True, threads=threads) - orc.gram(cov_down, x, x_meas=True, threads=threads)) / (2 * h)
            grads[name] = np.sum(S * dK) - np.sum(sym * dK)
            scales[name] = np.sum(np.abs(S * dK)) + np.sum(np.abs(sym * dK))
        else:
            dmu = (orc.mean_vector(mean_up, cov, x) - orc.mean_vector(mean_down, cov, x)) / (2 * h)
            grads[name] = -u @ dmu
            scales[name] = np.abs(u) @ np.abs(dmu)
    bf = brute_force(K, r, sv) if brute else None
    return grads, scales, value, bf


def _dataset(x, y, s):
    return ab.RegressionDataset(x, ab.MarginalDistribution(y, s))


def check(model, x, y, s=None, brute=False):
    ds = _dataset(x, y, s)
    loo, grad = model.leave_one_out_likelihood_gradient(ds)
    assert set(grad) == set(model.get_params())
    want, scale, value, bf = reference(model, x, y, s, brute=brute)
    assert abs(loo - value) <= 1e-10 * abs(value), (loo, value)
    if brute:
        assert abs(loo - bf) <= 1e-10 * abs(bf), (loo, bf)
    for name in want:
        assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (name, grad[name], want[name], scale[name])
    return loo, grad


def _variance(n, seed):
    return np.random.default_rng(seed).uniform(0.005, 0.05, n)


@pytest.mark.parametrize("with_variance", [False, True])
@pytest.mark.parametrize("n", [60, 1000])
def test_value_matches_closed_form(ctx, n, with_variance):
    x, y = _data(n, 3, 31 + n)
    s = _variance(n, n) if with_variance else None
    model = ab.gp_from_covariance(ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    ds = _dataset(x, y, s)
    loo = ab.LeaveOneOutLikelihood()(ds, model)
    _, _, value, bf = reference(model, x, y, s, brute=n <= 60)
    assert abs(loo - value) <= 1e-10 * abs(value), (loo, value)
    if bf is not None:
        assert abs(loo - bf) <= 1e-10 * abs(bf), (loo, bf)


@pytest.mark.parametrize("with_variance", [False, True])
def test_value_matches_leave_one_out_marginals(ctx, with_variance):
    n = 500
    x, y = _data(n, 3, 8)
    s = _variance(n, 9) if with_variance else None
    model = ab.gp_from_covariance(ab.SquaredExponential(1.5, 1.2) + ab.IndependentNoise(0.1), context=ctx)
    ds = _dataset(x, y, s)
    loo = ab.LeaveOneOutLikelihood()(ds, model)
    marg = model.fit(ds).get_fit().leave_one_out(y)
    v = marg.covariance + (0. if s is None else s)
    want = 0.5 * np.sum(np.log(v) + (y - marg.mean) ** 2 / v + LOG_2PI)
    assert abs(loo - want) <= 1e-12 * abs(want), (loo, want)
    full, _ = model.leave_one_out_likelihood_gradient(ds)
    assert abs(full - want) <= 1e-12 * abs(want), (full, want)
    if s is None:  # CrossValidation.scores scores without the truth's variance, which agrees only for s = 0

        def gaussian_nll(pred, truth):
            var = pred.covariance
            return float(np.sum(0.5 * (np.log(var) + (pred.mean - truth.mean) ** 2 / var + LOG_2PI)))

        scores = model.cross_validate().scores(gaussian_nll, ds, ab.LeaveOneOutGrouper())
        assert abs(loo - scores.sum()) <= 1e-12 * abs(loo)


@pytest.mark.parametrize("label,make,dim", LEAVES)
@pytest.mark.parametrize("n,with_variance", [(60, False), (60, True), (1000, True)])
def test_gradient_matches_reference(ctx, label, make, dim, n, with_variance):
    x, y = _data(n, dim, 11 + n)
    s = _variance(n, 5 + n) if with_variance else None
    check(ab.gp_from_covariance(make(), context=ctx), x, y, s, brute=n <= 60)


@pytest.mark.parametrize("n", [60, 1000, 4097])
def test_gradient_scaling_term_and_linear_mean(ctx, n):
    x, y = _data(n, 3, 3 + n)
    y = y + 0.3 * x[:, 0]
    cov, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    _, grad = check(model, x, y, _variance(n, n))
    assert {"elevation_scaling_center", "elevation_scaling_factor", "slope", "offset"} <= set(grad)


@pytest.mark.parametrize("dim", [4, 5, 8])
def test_gradient_padded_dimensions(ctx, dim):
    """The <4> and <8> instantiations of the contraction (5 dimensions are zero-padded to 8, the largest the feature check
    accepts) at n = 130: a full diagonal tile, a full off-diagonal tile and partial tiles of both kinds.
    The inputs of test_nll_gradient_gpu.py's case; cond(K + diag(s)) = 1.6e3, 4.6e2, 2.1e1 (numpy)."""
    x, y = _padded_data(dim)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.5, 1.2) + ab.IndependentNoise(0.1), context=ctx)
    check(model, x, y, _variance(130, dim))


def test_gradient_polynomial_1d(ctx):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1., 1., 300)
    y = 1. + 0.5 * x - x * x + 0.05 * rng.standard_normal(300)
    cov = ab.Polynomial(2, 0.8) + ab.SquaredExponential(0.5, 0.3) + ab.IndependentNoise(0.1)
    check(ab.gp_from_covariance(cov, context=ctx), x, y, _variance(300, 1))


def test_gradient_variant_tree(ctx):
    rng = np.random.default_rng(9)
    n = 400
    alt = rng.integers(0, 2, n)
    values = [rng.uniform(0., 5.) for _ in alt]
    feats = ab.VariantFeatures(alt, values)
    y = rng.standard_normal(n)
    cov = (ab.only_for_alternatives(ab.SquaredExponential(1.5, 1.0), 0) + ab.only_for_alternatives(ab.Matern52(2.0, 0.8), 1)
           + ab.only_for_alternatives(ab.Constant(0.4), 0, 1) + ab.IndependentNoise(0.3))
    check(ab.gp_from_covariance(cov, context=ctx), feats, y)


def test_gradient_4097_partial_tiles(ctx):
    x, y = _data(4097, 3, 1)
    cov = ab.Exponential(0.7, 1.1, ab.AngularDistance()) * ab.SquaredExponential(4.0, 1.3, ab.RadialDistance()) \
        + ab.Matern32(2.5, 0.5) + ab.IndependentNoise(0.2)
    check(ab.gp_from_covariance(cov, context=ctx), x, y, _variance(4097, 2))


def test_gradient_config3_8192(ctx):
    x, y = synthetic_3d(8192, 44)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    check(model, x, y)


def test_deterministic_and_value_only_agrees(ctx):
    n = 1000
    x, y = _data(n, 3, 2)
    cov, model = _elevation_model(ctx)
    ds = _dataset(x, y, _variance(n, 3))
    v1, g1 = model.leave_one_out_likelihood_gradient(ds)
    v2, g2 = model.leave_one_out_likelihood_gradient(ds)
    assert v1 == v2
    assert all(g1[k] == g2[k] for k in g1)
    # the value-only call reads c_i from R's column norms, the full call from R^T R's diagonal
    v0 = ab.LeaveOneOutLikelihood()(ds, model)
    assert abs(v0 - v1) <= 1e-13 * abs(v1), (v0, v1)


def test_errors(ctx):
    x, _ = _data(20, 2, 4)
    xd = np.concatenate([x[:10], x[:10]])
    bad = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0), context=ctx)
    with pytest.raises(ab.NotPositiveDefiniteError):
        bad.leave_one_out_likelihood_gradient(ab.RegressionDataset(xd, np.zeros(20)))
    with pytest.raises(ab.NotPositiveDefiniteError):
        ab.LeaveOneOutLikelihood()(ab.RegressionDataset(xd, np.zeros(20)), bad)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    xn = x.copy()
    xn[3, 1] = np.nan
    with pytest.raises(ab.NanInputError):
        model.leave_one_out_likelihood_gradient(ab.RegressionDataset(xn, np.zeros(20)))
    with pytest.raises(ab.NanInputError):
        ab.LeaveOneOutLikelihood()(ab.RegressionDataset(xn, np.zeros(20)), model)
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    with pytest.raises(NotImplementedError):
        model.leave_one_out_likelihood_gradient(ab.RegressionDataset(lc, np.zeros(2)))
    with pytest.raises(NotImplementedError):
        ab.LeaveOneOutLikelihood()(ab.RegressionDataset(lc, np.zeros(2)), model)
    mixed = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    mixed.precision = "mixed"
    with pytest.raises(ValueError):
        mixed.leave_one_out_likelihood_gradient(ab.RegressionDataset(x, np.zeros(20)))
    with pytest.raises(ValueError):
        ab.LeaveOneOutLikelihood()(ab.RegressionDataset(x, np.zeros(20)), mixed)


def test_bad_slots_are_rejected(ctx):
    x, y = _data(50, 2, 6)
    cov = ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1)  # nodes: 0 SE, 1 noise, 2 sum
    fs = cov.features(x)
    s = fs.as_struct()
    lib = ctx._lib
    value = C.c_double()
    g = np.zeros(2)

    def call(slots):
        table = (capi.GradientSlot * len(slots))(*[capi.GradientSlot(a, b) for a, b in slots])
        return lib.agp_loo_nll_gradient(ctx._h, ctx.kernel(cov), C.byref(s), C.c_void_p(y.ctypes.data), None, len(slots),
                                        table, None, 0, C.byref(value), C.c_void_p(g.ctypes.data), None)

    assert call([(0, 0), (1, 0)]) == capi.AGP_OK
    assert call([(2, 0)]) == capi.AGP_ERR_INVALID_ARGUMENT   # the sum node
    assert call([(0, 2)]) == capi.AGP_ERR_INVALID_ARGUMENT   # a radial leaf has two parameters
    assert call([(1, 1)]) == capi.AGP_ERR_INVALID_ARGUMENT   # noise has one
    assert call([(3, 0)]) == capi.AGP_ERR_INVALID_ARGUMENT   # no such node
    assert call([(0, 0)] * (capi.MAX_GRADIENT_SLOTS + 1)) == capi.AGP_ERR_INVALID_ARGUMENT
    xn = x.copy()
    xn[0, 0] = np.nan
    sn = cov.features(xn).as_struct()
    assert lib.agp_loo_nll_gradient(ctx._h, ctx.kernel(cov), C.byref(sn), C.c_void_p(y.ctypes.data), None, 0, None, None, 0,
                                    C.byref(value), None, None) == capi.AGP_ERR_NAN_INPUT


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("n", [128, 1000, 4096])
def test_gtg_kernel_matches_numpy(ctx, n):
    dbg = capi.load_debug()
    dbg.agp_debug_gtg_lower.restype = C.c_int
    dbg.agp_debug_gtg_lower.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_double)]
    rng = np.random.default_rng(n)
    ld = n + 8
    G = rng.uniform(-1., 1., (n, n)) / np.sqrt(n)
    Gd = np.full((ld, n), np.nan, order="F")  # the padding rows must not be read
    Gd[:n] = G
    Sd = np.zeros((ld, n), order="F")
    ms = C.c_double()
    assert dbg.agp_debug_gtg_lower(ctx._h, _p(Gd), n, ld, _p(Sd), C.byref(ms)) == 0
    want = G.T @ G
    low = np.tril_indices(n)
    assert np.abs(Sd[:n][low] - want[low]).max() <= 1e-13 * np.abs(want).max()
    assert np.all(Sd[n:] == 0.)  # nothing written below row n


def test_cpp_loo_gradient_matches_python(ctx):
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "loo_gradient_check")], text=True)
    rows = {}
    for line in out.strip().splitlines():
        key, *vals = line.split(",")
        rows.setdefault(key, []).append(vals)
    data = np.array(rows["x"], dtype=float)
    x, y, s = data[:, 1:4], data[:, 4], data[:, 5]
    cov, _ = _elevation_model(ctx)
    model = ab.gp_from_covariance_and_mean(cov, _FirstCoordinateMean(0.2, -0.4), context=ctx)
    ds = _dataset(x, y, s)
    loo, grad = model.leave_one_out_likelihood_gradient(ds)
    cpp = {k[len("grad_"):]: float(v[0][0]) for k, v in rows.items() if k.startswith("grad_")}
    assert set(cpp) == set(grad)
    assert abs(float(rows["loo_nll"][0][0]) - loo) <= 1e-10 * abs(loo)
    assert abs(float(rows["loo_nll_metric"][0][0]) - ab.LeaveOneOutLikelihood()(ds, model)) <= 1e-10 * abs(loo)
    for name in grad:
        assert abs(cpp[name] - grad[name]) <= 1e-10 * max(abs(grad[name]), 1e-3 * max(abs(g) for g in grad.values())), name
