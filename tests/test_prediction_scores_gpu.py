"""GPU tests of the prediction scores (albatross_amd/csrc/scores.hip; include/albatross_amd.h, "scoring a joint
prediction"): the counter-based normal generator, draws through the resident LL^T factor, the energy score, the variogram
score and the CRPS against the numpy restatement of tests/prediction_score_cases.py, their status codes, their
run-to-run determinism, and the Python surface on device-resident predictions."""
import ctypes as C
import math

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi

import prediction_score_cases as pc

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def padded(a, extra=3):
    """(buffer, ld): `a` in the top rows of a column-major buffer with `extra` further rows of NaN"""
    a = np.asarray(a, dtype=np.float64)
    buf = np.full((a.shape[0] + extra, a.shape[1]), np.nan, order="F")
    buf[:a.shape[0]] = a
    return buf, buf.shape[0]


def normals(ctx, seed, m, first, n, extra=0):
    out = np.full((m + extra, n), np.nan, order="F")
    ctx._check(ctx._lib.agp_standard_normal(ctx._h, seed, m, first, n, p(out), m + extra, capi.HOST), "agp_standard_normal")
    return out[:m]


def covariance_case(m, seed):
    rng = np.random.default_rng(seed)
    c = pc.random_covariance(rng, m)
    assert pc.max_offdiagonal_correlation(c) <= 0.9
    return rng, c


def factor(ctx, c):
    """agp_factor_create of the LOWER triangle of c; the strict upper triangle of what is handed over is NaN"""
    m = c.shape[0]
    k = np.array(c, order="F")
    k[np.triu_indices(m, 1)] = np.nan
    h = C.c_void_p()
    ctx._check(ctx._lib.agp_factor_create(ctx._h, p(k), m, m, 0, capi.HOST, C.byref(h)), "agp_factor_create")
    L = np.empty((m, m), order="F")
    ctx._check(ctx._lib.agp_fit_download_factor(ctx._h, h, p(L), m), "agp_fit_download_factor")
    return h, L


def draw(ctx, h, mean, n_draws, seed, z, extra=3):
    m = mean.shape[0]
    out = np.full((m + extra, n_draws), np.nan, order="F")
    zb, ldz = (None, 0) if z is None else padded(z, extra)
    ctx._check(ctx._lib.agp_draw_mvn(ctx._h, h, p(mean), n_draws, seed, p(zb), ldz, p(out), m + extra, capi.HOST), "agp_draw_mvn")
    assert np.isnan(out[m:]).all()  # the padding rows are not written
    return out[:m]


def energy(ctx, mean, c, truth, truth_var, weights, seed, num_samples, z, extra=3):
    m = mean.shape[0]
    cb, ldc = padded(c, extra)
    cb[:m][np.triu_indices(m, 1)] = np.nan  # only the lower triangle is read
    zb, ldz = (None, 0) if z is None else padded(z, extra)
    out = C.c_double(-7.)
    st = ctx._lib.agp_energy_score(ctx._h, p(mean), p(cb), ldc, m, p(truth), p(truth_var), p(weights), seed, num_samples,
                                   p(zb), ldz, capi.HOST, C.byref(out))
    return st, out.value


def variogram(ctx, mean, c, truth, truth_var, weights, order, extra=3):
    m = mean.shape[0]
    cb, ldc = padded(c, extra)
    cb[:m][np.tril_indices(m, -1)] = np.nan  # the diagonal and the strict upper triangle are what is read
    wb, ldw = (None, 0)
    if weights is not None:
        wb, ldw = padded(weights, extra + 2)
        wb[:m][np.tril_indices(m)] = np.nan
    out = C.c_double(-7.)
    st = ctx._lib.agp_variogram_score(ctx._h, p(mean), p(cb), ldc, m, p(truth), p(truth_var), p(wb), ldw, order, capi.HOST,
                                      C.byref(out))
    return st, out.value


# ---- generator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,first", [(1, 1, 0), (129, 17, 0), (64, 130, 7)])
def test_generator_values(ctx, m, n, first):
    """the integers are exact; log / cos differ by a few ulp under a factor <= 8.6 (|z| <= sqrt(-2 ln 2^-54))"""
    got = normals(ctx, 22, m, first, n, extra=2)
    err = np.abs(got - pc.standard_normal(22, m, first, n)).max()
    print("generator max abs error", err)
    assert err <= 1e-12


def test_generator_columns_do_not_depend_on_the_call(ctx):
    a, b = normals(ctx, 22, 200, 0, 64), normals(ctx, 22, 200, 32, 64)
    assert np.array_equal(a[:, 32:], b[:, :32])
    assert not np.array_equal(a, normals(ctx, 23, 200, 0, 64))


def test_generator_moments(ctx):
    z = normals(ctx, 22, 256, 0, 1024)
    n = z.size
    print("mean", z.mean(), "var - 1", z.var() - 1.)
    assert abs(z.mean()) <= 5. / math.sqrt(n)
    assert abs(z.var() - 1.) <= 5. * math.sqrt(2. / n)


# ---- draws -------------------------------------------------------------------------------------------------------------------
DRAW_COLUMNS = [1, 15, 16, 17, 130]


@pytest.mark.parametrize("m", [1, 2, 127, 128, 129, 257, 640])
def test_draws_with_supplied_normals(ctx, m):
    rng, c = covariance_case(m, 100 + m)
    mean = rng.standard_normal(m) * 3.
    h, L = factor(ctx, c)
    try:
        assert np.array_equal(L, np.tril(L))
        for n_draws in DRAW_COLUMNS:
            z = rng.standard_normal((m, n_draws))
            got = draw(ctx, h, mean, n_draws, 0, z)
            want = mean[:, None] + L @ z
            # gamma bound of a length-(i + 1) dot product plus the addition of the mean, any accumulation order
            bound = 2. * (np.arange(m)[:, None] + 2.) * EPS * (np.abs(L) @ np.abs(z) + np.abs(mean)[:, None])
            ratio = (np.abs(got - want) / bound).max()
            print(f"m={m} n_draws={n_draws}: max error / bound {ratio:.3f}")
            assert np.isfinite(got).all() and ratio <= 1.
    finally:
        ctx._lib.agp_fit_destroy(h)


@pytest.mark.parametrize("m,n_draws", [(1, 3), (129, 17), (640, 130)])
def test_draws_from_the_generator_equal_draws_from_its_output(ctx, m, n_draws):
    rng, c = covariance_case(m, 200 + m)
    mean = rng.standard_normal(m)
    h, _ = factor(ctx, c)
    try:
        generated = draw(ctx, h, mean, n_draws, 31, None)
        supplied = draw(ctx, h, mean, n_draws, 0, normals(ctx, 31, m, 0, n_draws))
        assert np.array_equal(generated, supplied)
    finally:
        ctx._lib.agp_fit_destroy(h)


# ---- energy score ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 129, 300])
@pytest.mark.parametrize("num_samples", [2, 3, 1000])
def test_energy_score_with_supplied_normals(ctx, m, num_samples):
    rng, c = covariance_case(m, 300 + m)
    mean, truth = rng.standard_normal(m), rng.standard_normal(m)
    k = num_samples // 2 + 1
    z = rng.standard_normal((m, 2 * k))
    for weights in (None, rng.uniform(0.2, 2., m)):
        for truth_var in (None, rng.uniform(0.1, 1., m)):
            st, got = energy(ctx, mean, c, truth, truth_var, weights, 0, num_samples, z)
            assert st == capi.AGP_OK
            term1, paired = pc.energy_score_terms(mean, c, truth, weights, z, truth_var)
            want = max(0., term1 - 0.5 * paired)
            print(f"m={m} samples={num_samples}: |got - want| = {abs(got - want):.3e}, scale {term1 + paired:.3e}")
            assert abs(got - want) <= 1e-10 * (term1 + paired)
            if weights is None:
                st, ones = energy(ctx, mean, c, truth, truth_var, np.ones(m), 0, num_samples, z)
                assert st == capi.AGP_OK and abs(ones - got) <= 1e-10 * (term1 + paired)


def test_energy_score_zero_weight_hides_the_wrong_component(ctx):
    """tests/test_stats_scores.cc:689-704"""
    m = 40
    rng, c = covariance_case(m, 17)
    mean, truth = rng.standard_normal(m), rng.standard_normal(m)
    mean[0] += 1000.
    w = np.ones(m)
    w[0] = 0.
    st1, full = energy(ctx, mean, c, truth, None, None, 456, 500, None)
    st2, masked = energy(ctx, mean, c, truth, None, w, 456, 500, None)
    assert st1 == capi.AGP_OK and st2 == capi.AGP_OK
    assert masked < 0.5 * full


def test_energy_score_matches_crps_in_one_dimension(ctx):
    """tests/test_stats_scores.cc:215-250 with the library's generator: 500 samples, |ES - CRPS| <= 2 sqrt(2 sigma^2 / 500)"""
    rng = np.random.default_rng(9999)
    for _ in range(40):
        mu, sigma, truth = rng.uniform(-10., 10.), rng.uniform(0.1, 5.), rng.uniform(-10., 10.)
        st, es = energy(ctx, np.array([mu]), np.array([[sigma * sigma]]), np.array([truth]), None, None, 444, 500, None)
        assert st == capi.AGP_OK
        assert abs(es - pc.crps_normal(mu, sigma, truth)) <= 2. * math.sqrt(2. * sigma * sigma / 500.)


# ---- variogram score ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 513])
@pytest.mark.parametrize("order", [1, 2])
def test_variogram_score(ctx, m, order):
    rng, c = covariance_case(m, 400 + m)
    mean, truth = rng.standard_normal(m) * 2., rng.standard_normal(m) * 2.
    w = rng.uniform(0.1, 2., (m, m))
    for weights in (None, w):
        for truth_var in (None, rng.uniform(0.1, 1., m)):
            st, got = variogram(ctx, mean, c, truth, truth_var, weights, order)
            assert st == capi.AGP_OK
            want = pc.variogram_score(mean, c, truth, weights, order, truth_var)
            print(f"m={m} order={order}: got {got:.12e} want {want:.12e}")
            assert abs(got - want) <= 1e-10 * abs(want)
            if m == 1:
                assert got == 0.
            # an offset on mean and truth alike changes nothing (tests/test_stats_scores.cc:381-391)
            st, shifted = variogram(ctx, mean + 5., c, truth + 5., truth_var, weights, order)
            assert st == capi.AGP_OK and abs(shifted - got) <= 1e-10 * abs(got)
    st, zero = variogram(ctx, mean, c, truth, None, np.zeros((m, m)), order)
    assert st == capi.AGP_OK and zero == 0.


# ---- CRPS ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257])
def test_crps_normal(ctx, n):
    rng = np.random.default_rng(n)
    mu, sigma, y = rng.uniform(-10., 10., n), rng.uniform(0.1, 5., n), rng.uniform(-10., 10., n)
    special = {}
    if n > 8:
        sigma[1], sigma[2] = 0., -1.                       # degenerate: absolute error
        mu[3], sigma[4], y[5], sigma[6] = np.nan, np.inf, -np.inf, np.nan
        special = {1: abs(y[1] - mu[1]), 2: abs(y[2] - mu[2])}
    out = np.full(n, -7.)
    ctx._check(ctx._lib.agp_crps_normal(ctx._h, p(mu), p(sigma), p(y), n, p(out), capi.HOST), "agp_crps_normal")
    for i in range(n):
        want = pc.crps_normal(mu[i], sigma[i], y[i])
        if math.isnan(want):
            assert 3 <= i <= 6 and math.isnan(out[i])
        elif i in special:
            assert out[i] == special[i] == want
        else:
            assert abs(out[i] - want) <= 1e-14 * abs(want)
    assert ab.crps_normal(5., 0., 3.) == 2. and ab.crps_normal(5., 0., 5.) == 0. and ab.crps_normal(5., -1., 3.) == 2.


# ---- status codes --------------------------------------------------------------------------------------------------------------
def test_status_codes_and_nothing_written_on_failure(ctx):
    m = 20
    rng, c = covariance_case(m, 5)
    mean, truth = rng.standard_normal(m), rng.standard_normal(m)
    lib = ctx._lib
    assert energy(ctx, mean, c, truth, None, None, 1, 1, None) == (capi.AGP_ERR_INVALID_ARGUMENT, -7.)   # num_samples = 1
    out = C.c_double(-7.)
    cf = np.asfortranarray(c)
    assert lib.agp_energy_score(ctx._h, p(mean), p(cf), m - 1, m, p(truth), None, None, 1, 10, None, 0, capi.HOST,
                                C.byref(out)) == capi.AGP_ERR_INVALID_ARGUMENT and out.value == -7.       # ldc < m
    z = np.zeros((m - 1, 12), order="F")
    assert lib.agp_energy_score(ctx._h, p(mean), p(cf), m, m, p(truth), None, None, 1, 10, p(z), m - 1, capi.HOST,
                                C.byref(out)) == capi.AGP_ERR_INVALID_ARGUMENT and out.value == -7.       # ldz < m
    assert variogram(ctx, mean, c, truth, None, None, 3) == (capi.AGP_ERR_INVALID_ARGUMENT, -7.)          # order 3
    assert lib.agp_variogram_score(ctx._h, p(mean), p(cf), m - 1, m, p(truth), None, None, 0, 1, capi.HOST,
                                   C.byref(out)) == capi.AGP_ERR_INVALID_ARGUMENT and out.value == -7.
    indefinite = c.copy()
    indefinite[7, 7] = -1.
    assert energy(ctx, mean, indefinite, truth, None, None, 1, 10, None) == (capi.AGP_ERR_NOT_POSITIVE_DEFINITE, -7.)
    with_nan = c.copy()
    with_nan[9, 4] = np.nan
    assert energy(ctx, mean, with_nan, truth, None, None, 1, 10, None) == (capi.AGP_ERR_NAN_INPUT, -7.)
    # a fit grown by agp_fit_update from a size that is no multiple of 128 carries phantom rows
    x = rng.uniform(0., 10., (150, 2))
    model = ab.gp_from_covariance(ab.SquaredExponential(2., 1.) + ab.IndependentNoise(0.3), context=ctx)
    grown = model.fit(ab.RegressionDataset(x[:140], np.sin(x[:140]).sum(axis=1))).update(
        ab.RegressionDataset(x[140:], np.sin(x[140:]).sum(axis=1)))
    fit = grown.get_fit()
    assert isinstance(fit, ab.GPFit) and fit.rows() == 150
    res = np.full((150, 2), -7., order="F")
    assert lib.agp_draw_mvn(ctx._h, fit._h, p(np.zeros(150)), 2, 1, None, 0, p(res), 150, capi.HOST) == capi.AGP_ERR_UNSUPPORTED
    assert (res == -7.).all()


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_every_entry_is_bit_identical_between_two_calls(ctx):
    m = 257
    rng, c = covariance_case(m, 77)
    mean, truth, tv = rng.standard_normal(m), rng.standard_normal(m), rng.uniform(0.1, 1., m)
    w = rng.uniform(0.1, 2., (m, m))
    assert np.array_equal(normals(ctx, 5, m, 3, 70), normals(ctx, 5, m, 3, 70))
    h, _ = factor(ctx, c)
    try:
        assert np.array_equal(draw(ctx, h, mean, 70, 9, None), draw(ctx, h, mean, 70, 9, None))
    finally:
        ctx._lib.agp_fit_destroy(h)
    first = energy(ctx, mean, c, truth, tv, w[0], 22, 1000, None)
    assert first[0] == capi.AGP_OK and first == energy(ctx, mean, c, truth, tv, w[0], 22, 1000, None)
    for order in (1, 2):
        first = variogram(ctx, mean, c, truth, tv, w, order)
        assert first[0] == capi.AGP_OK and first == variogram(ctx, mean, c, truth, tv, w, order)
    out = [np.empty(m), np.empty(m)]
    for o in out:
        ctx._check(ctx._lib.agp_crps_normal(ctx._h, p(mean), p(tv), p(truth), m, p(o), capi.HOST), "agp_crps_normal")
    assert np.array_equal(*out)


# ---- Python surface ------------------------------------------------------------------------------------------------------------
def test_python_surface_on_device_resident_predictions(ctx):
    rng = np.random.default_rng(3)
    x, xs = rng.uniform(0., 10., (300, 3)), rng.uniform(0., 10., (129, 3))
    f = lambda a: np.sin(a).sum(axis=1)
    model = ab.gp_from_covariance(ab.Matern52(2., 1.) + ab.IndependentNoise(0.2), context=ctx)
    prediction = model.fit(ab.RegressionDataset(x, f(x))).predict_with_measurement_noise(xs)
    on_device = prediction.joint(on_device=True)
    assert isinstance(on_device.covariance, ab.DeviceArray) and on_device.covariance.shape == (129, 129)
    on_host = on_device.numpy()
    reference = prediction.joint()
    assert np.array_equal(on_host.mean, reference.mean) and np.array_equal(on_host.covariance, reference.covariance)
    truth = ab.MarginalDistribution(f(xs) + 0.1 * rng.standard_normal(129), np.full(129, 0.01))
    w = rng.uniform(0.5, 1.5, (129, 129))
    for order in ("madogram", "variogram"):
        assert ab.variogram_score(on_device, truth, w, order) == ab.variogram_score(on_host, truth, w, order)
    assert ab.variogram_score(on_device, truth.mean) == ab.variogram_score(on_host, truth.mean)
    es = ab.energy_score(on_device, truth, w[0])
    assert es == ab.energy_score(on_host, truth, w[0]) and es > 0.
    draws = ab.draw_mvn(on_device, 33, seed=4)
    assert isinstance(draws, ab.DeviceArray)
    assert np.array_equal(draws.numpy().ravel().reshape((129, 33), order="F"), ab.draw_mvn(on_host, 33, seed=4))
    cdf = ab.chi_squared_cdf(on_device, truth.mean)
    assert cdf == ab.chi_squared_cdf(on_host, truth.mean) and 0. <= cdf <= 1.
    # against numpy: the quadratic form and the regularised incomplete gamma of half of it
    d = on_host.mean - truth.mean
    cov = on_host.covariance + np.diag(truth.covariance)
    q = d @ np.linalg.solve(cov, d)
    from albatross_amd.scores import chi_squared_cdf_scalar
    assert abs(ab.chi_squared_cdf(on_host, truth) - chi_squared_cdf_scalar(q, 129)) <= 1e-9
