"""GPU tests of GaussianProcessRegression.log_likelihood_gradient / agp_nll_gradient (exact gradient of the
log-likelihood with respect to the parameters) and of its R^T R kernel.

Reference: numpy, independent of the library.  K = orc.gram(measurement features), K^-1 and alpha = K^-1 (y - mu) in
numpy; dK / dtheta is a central difference of orc.gram at theta +- h, h = 1e-5 max(1, |theta|) (ScalingTerm
parameters through the features the perturbed function makes); mean terms are central differences of
orc.mean_vector.

Tolerance: |g - g_ref| <= 1e-7 s_p with s_p = 1/2 sum |K^-1_ij dK_ij| + 1/2 |alpha^T dK alpha|, a scale of the terms
the gradient sums that does not cancel.  The library's gradient is exact to fp64 rounding: the inverse carries a
relative error ~ eps cond(K) (cond ~ 1e4 ... 1e6 here: <= 1e-10) into every term.  The reference's own error is the
central difference's: truncation h^2 |d^3 K| / 6 ~ 1e-10 relative and cancellation eps |K| / h ~ 1e-11 relative per
entry.  1e-7 leaves two to three orders of magnitude over both; a gradient that drops a term, a factor 2 off the
diagonal or a leaf's chain rule is off by O(1) s_p."""
import copy
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from conftest import synthetic_3d
from oracle import oracle_py as orc

pytestmark = pytest.mark.gpu


def _elevation_model(ctx):
    """(copied from test_gp_gpu.py) ScalingTerm * Constant + Matern52 + noise with a LinearMean"""
    class Elevation(ab.ScalingFunction):
        _params = {"elevation_scaling_center": 4.0, "elevation_scaling_factor": 0.3}

        def get_name(self):
            return "elevation_scaling"

        def _call_impl(self, c):
            p = self.get_params()
            return 1. + p["elevation_scaling_factor"] * np.maximum(p["elevation_scaling_center"] - np.asarray(c)[:, 2], 0.)

    cov = ab.ScalingTerm(Elevation()) * ab.Constant(0.5) + ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1)
    return cov, ab.gp_from_covariance_and_mean(cov, ab.LinearMean(), context=ctx)


def perturbed(model, name, value):
    """copies of the model's covariance and mean functions with `name` set to `value`"""
    cov, mean = copy.deepcopy(model.covariance_function_), copy.deepcopy(model.mean_function_)
    if name in cov.get_params():
        cov.set_param(name, value)
    else:
        mean.set_param(name, value)
    return cov, mean


def reference_gradient(model, x, y, threads=16):
    """({name: d log p / d name}, {name: s_p}, log p) in numpy from the oracle's Gram matrices"""
    cov, mean = model.covariance_function_, model.mean_function_
    K = orc.gram(cov, x, x_meas=True, threads=threads)
    r = np.asarray(y, dtype=np.float64) - orc.mean_vector(mean, cov, x)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = Kinv @ r
    sign, logdet = np.linalg.slogdet(K)
    loglik = -0.5 * (logdet + r @ alpha + len(r) * np.log(2 * np.pi))
    grads, scales = {}, {}
    cov_names = cov.get_params()
    for name, value in model.get_params().items():
        h = 1e-5 * max(1., abs(value))
        (cov_up, mean_up), (cov_down, mean_down) = perturbed(model, name, value + h), perturbed(model, name, value - h)
        if name in cov_names:
            dK = (orc.gram(cov_up, x, x_meas=True, threads=threads) - orc.gram(cov_down, x, x_meas=True, threads=threads)) / (2 * h)
            q = alpha @ dK @ alpha
            grads[name] = -0.5 * np.sum(Kinv * dK) + 0.5 * q
            scales[name] = 0.5 * np.sum(np.abs(Kinv * dK)) + 0.5 * abs(q)
        else:
            dmu = (orc.mean_vector(mean_up, cov, x) - orc.mean_vector(mean_down, cov, x)) / (2 * h)
            grads[name] = dmu @ alpha
            scales[name] = np.abs(dmu) @ np.abs(alpha)
    return grads, scales, loglik


def check_against_reference(model, x, y, ds=None):
    ds = ds if ds is not None else ab.RegressionDataset(x, y)
    ll, grad = model.log_likelihood_gradient(ds)
    assert set(grad) == set(model.get_params())
    want, scale, ll_ref = reference_gradient(model, x, y)
    for name in want:
        assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (name, grad[name], want[name], scale[name])
    assert abs(ll - ll_ref) <= 1e-8 * len(y)
    assert abs(ll - model.log_likelihood(ds)) <= 1e-12 * abs(ll)
    return ll, grad


def _data(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0., 10., (n, dim))
    y = np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0])
    return x, y


def _padded_data(dim, n=130, seed=70):
    """n points in [0, 3]^dim: close enough for the covariance to couple them in 4 to 8 dimensions"""
    rng = np.random.default_rng(seed + dim)
    x = rng.uniform(0., 3., (n, dim))
    return x, np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0])


LEAVES = [
    ("se euclid", lambda: ab.SquaredExponential(1.5, 1.2) + ab.IndependentNoise(0.1), 3),
    ("exp euclid", lambda: ab.Exponential(3.0, 0.9) + ab.IndependentNoise(0.2), 2),
    ("m32 euclid", lambda: ab.Matern32(2.5, 1.1) + ab.IndependentNoise(0.1), 3),
    ("m52 euclid", lambda: ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1), 3),
    ("exp angular * se radial + const + nugget",
     lambda: ab.Exponential(0.7, 1.1, ab.AngularDistance()) * ab.SquaredExponential(4.0, 1.3, ab.RadialDistance())
     + ab.Constant(0.6) + ab.IndependentNoise(0.15) + ab.Nugget(1e-3), 3),
    ("m32 radial + m52 angular", lambda: ab.Matern32(3.0, 0.8, ab.RadialDistance())
     + ab.Matern52(0.9, 0.7, ab.AngularDistance()) + ab.IndependentNoise(0.1), 3),
    ("measurement_only noise", lambda: ab.SquaredExponential(2.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.2)), 2),
    ("shared name", lambda: ab.SquaredExponential(2.0, 1.0) * ab.SquaredExponential(2.0, 1.0) + ab.IndependentNoise(0.1), 2),
]


@pytest.mark.parametrize("label,make,dim", LEAVES)
@pytest.mark.parametrize("n", [60, 1000])
def test_gradient_matches_reference(ctx, label, make, dim, n):
    x, y = _data(n, dim, 11 + n)
    check_against_reference(ab.gp_from_covariance(make(), context=ctx), x, y)


def test_gradient_polynomial_1d(ctx):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1., 1., 300)
    y = 1. + 0.5 * x - x * x + 0.05 * rng.standard_normal(300)
    cov = ab.Polynomial(2, 0.8) + ab.SquaredExponential(0.5, 0.3) + ab.IndependentNoise(0.1)
    check_against_reference(ab.gp_from_covariance(cov, context=ctx), x, y)


@pytest.mark.parametrize("n", [60, 1000, 4097])
def test_gradient_scaling_term_and_linear_mean(ctx, n):
    x, y = _data(n, 3, 3 + n)
    y = y + 0.3 * x[:, 0]
    cov, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    ll, grad = check_against_reference(model, x, y)
    assert {"elevation_scaling_center", "elevation_scaling_factor", "slope", "offset"} <= set(grad)


def test_gradient_variant_tree(ctx):
    rng = np.random.default_rng(9)
    n = 400
    alt = rng.integers(0, 2, n)
    values = [rng.uniform(0., 5.) if a == 0 else rng.uniform(0., 5.) for a in alt]
    feats = ab.VariantFeatures(alt, values)
    y = rng.standard_normal(n)
    cov = (ab.only_for_alternatives(ab.SquaredExponential(1.5, 1.0), 0) + ab.only_for_alternatives(ab.Matern52(2.0, 0.8), 1)
           + ab.only_for_alternatives(ab.Constant(0.4), 0, 1) + ab.IndependentNoise(0.3))
    check_against_reference(ab.gp_from_covariance(cov, context=ctx), feats, y)


def test_gradient_config3_8192(ctx):
    x, y = synthetic_3d(8192, 44)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    check_against_reference(model, x, y)


def test_gradient_4097_partial_tiles(ctx):
    x, y = _data(4097, 3, 1)
    cov = ab.Exponential(0.7, 1.1, ab.AngularDistance()) * ab.SquaredExponential(4.0, 1.3, ab.RadialDistance()) \
        + ab.Matern32(2.5, 0.5) + ab.IndependentNoise(0.2)
    check_against_reference(ab.gp_from_covariance(cov, context=ctx), x, y)


@pytest.mark.parametrize("dim", [4, 5, 8])
def test_gradient_padded_dimensions(ctx, dim):
    """The <4> and <8> instantiations of the contraction (5 dimensions are zero-padded to 8, the largest the feature check
    accepts).  n = 130: three tile rows of 64 with a ragged last one - a full diagonal tile, a full off-diagonal tile and
    partial tiles of both kinds.  The points fill [0, 3]^dim: in [0, 10]^dim every pair would be many length scales apart
    and K all but diagonal.  Here the median off-diagonal |K_ij| is 0.15 ... 0.009 and cond(K) = 3.7e3, 8.5e2, 2.3e1 (numpy)."""
    x, y = _padded_data(dim)
    check_against_reference(ab.gp_from_covariance(ab.SquaredExponential(1.5, 1.2) + ab.IndependentNoise(0.1), context=ctx), x, y)


def test_gradient_matches_central_differences_of_log_likelihood(ctx):
    x, y = _data(256, 3, 21)
    y = y + 0.3 * x[:, 0]
    cov, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    ds = ab.RegressionDataset(x, y)
    ll, grad = model.log_likelihood_gradient(ds)
    for name, value in model.get_params().items():
        h = 1e-4 * max(1., abs(value))
        up = ab.gp_from_covariance_and_mean(*perturbed(model, name, value + h), context=ctx)
        down = ab.gp_from_covariance_and_mean(*perturbed(model, name, value - h), context=ctx)
        fd = (up.log_likelihood(ds) - down.log_likelihood(ds)) / (2 * h)
        assert abs(grad[name] - fd) <= 1e-5 * max(1., abs(fd)), (name, grad[name], fd)


def test_gradient_is_deterministic(ctx):
    x, y = _data(1000, 3, 2)
    cov, model = _elevation_model(ctx)
    ds = ab.RegressionDataset(x, y)
    ll1, g1 = model.log_likelihood_gradient(ds)
    ll2, g2 = model.log_likelihood_gradient(ds)
    assert ll1 == ll2
    assert all(g1[k] == g2[k] for k in g1)


def test_gradient_errors(ctx):
    x, _ = _data(20, 2, 4)
    xd = np.concatenate([x[:10], x[:10]])
    bad = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0), context=ctx)
    with pytest.raises(ab.NotPositiveDefiniteError):
        bad.log_likelihood_gradient(ab.RegressionDataset(xd, np.zeros(20)))
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    with pytest.raises(NotImplementedError):
        model.log_likelihood_gradient(ab.RegressionDataset(lc, np.zeros(2)))


def test_bad_slots_are_rejected(ctx):
    x, y = _data(50, 2, 6)
    cov = ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1)  # nodes: 0 SE, 1 noise, 2 sum
    fs = cov.features(x)
    s = fs.as_struct()
    lib = ctx._lib
    nll = C.c_double()
    g = np.zeros(2)

    def call(slots):
        table = (capi.GradientSlot * len(slots))(*[capi.GradientSlot(a, b) for a, b in slots])
        return lib.agp_nll_gradient(ctx._h, ctx.kernel(cov), C.byref(s), C.c_void_p(y.ctypes.data), None, len(slots),
                                    table, None, 0, C.byref(nll), C.c_void_p(g.ctypes.data), None)

    assert call([(0, 0), (1, 0)]) == capi.AGP_OK
    assert call([(2, 0)]) == capi.AGP_ERR_INVALID_ARGUMENT   # the sum node
    assert call([(0, 2)]) == capi.AGP_ERR_INVALID_ARGUMENT   # a radial leaf has two parameters
    assert call([(1, 1)]) == capi.AGP_ERR_INVALID_ARGUMENT   # noise has one
    assert call([(3, 0)]) == capi.AGP_ERR_INVALID_ARGUMENT   # no such node
    assert call([(0, 0)] * (capi.MAX_GRADIENT_SLOTS + 1)) == capi.AGP_ERR_INVALID_ARGUMENT


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("n", [128, 1000, 4096])
def test_rtr_kernel_matches_numpy(ctx, n):
    dbg = capi.load_debug()
    dbg.agp_debug_rtr_lower.restype = C.c_int
    dbg.agp_debug_rtr_lower.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_double)]
    rng = np.random.default_rng(n)
    ld = n + 8
    R = np.tril(rng.uniform(-1., 1., (n, n))) / np.sqrt(n)
    R[np.diag_indices(n)] = 1. + rng.uniform(0., 1., n)
    Rd = np.zeros((ld, n), order="F")
    Rd[:n] = R
    Cd = np.zeros((ld, n), order="F")
    ms = C.c_double()
    assert dbg.agp_debug_rtr_lower(ctx._h, _p(Rd), n, ld, _p(Cd), C.byref(ms)) == 0
    want = R.T @ R
    got = Cd[:n]
    low = np.tril_indices(n)
    assert np.abs(got[low] - want[low]).max() <= 1e-13 * np.abs(want).max()


class _FirstCoordinateMean(ab.MeanFunction):
    """slope * x[0] + offset on 3-D features: the mean function of examples/gradient_check.cpp"""

    def __init__(self, slope, offset):
        self._params = {"slope": float(slope), "offset": float(offset)}

    def get_params(self):
        return dict(self._params)

    def set_param(self, name, value):
        if name not in self._params:
            raise KeyError(name)
        self._params[name] = float(value)

    def __call__(self, coords):
        return self._params["slope"] * np.asarray(coords)[:, 0] + self._params["offset"]


def test_cpp_gradient_matches_python(ctx):
    import os
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "gradient_check")], text=True)
    rows = {}
    for line in out.strip().splitlines():
        key, *vals = line.split(",")
        rows.setdefault(key, []).append(vals)
    data = np.array(rows["x"], dtype=float)
    x, y = data[:, 1:4], data[:, 4]
    cov, _ = _elevation_model(ctx)
    model = ab.gp_from_covariance_and_mean(cov, _FirstCoordinateMean(0.2, -0.4), context=ctx)
    ll, grad = model.log_likelihood_gradient(ab.RegressionDataset(x, y))
    cpp = {k[len("grad_"):]: float(v[0][0]) for k, v in rows.items() if k.startswith("grad_")}
    assert set(cpp) == set(grad)
    assert abs(float(rows["loglik"][0][0]) - ll) <= 1e-10 * abs(ll)
    assert float(rows["loglik"][0][0]) == float(rows["loglik_plain"][0][0]) or \
        abs(float(rows["loglik"][0][0]) - float(rows["loglik_plain"][0][0])) <= 1e-12 * abs(ll)
    for name in grad:
        assert abs(cpp[name] - grad[name]) <= 1e-10 * max(abs(grad[name]), 1e-3 * max(abs(g) for g in grad.values())), name
