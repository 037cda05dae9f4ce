"""The matrix-free fit (csrc/iterative.hip: agp_iterative_fit_create, agp_iterative_solve, agp_iterative_predict_*) on the
GPU against the dense fp64 fit (agp_fit_create) and against the matrix K = ctx.gram(cov, x): the inputs, the bounds and
the restated definition are in tests/iterative_fit_cases.py, and tests/test_iterative_fit_host.py shows the float64
restatement meets every condition asserted here on the same inputs.  Iteration counts of the library are printed beside
the restatement's where that is cheap; they are not asserted equal (the summation orders differ)."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import iterative_fit_cases as ic

pytestmark = pytest.mark.gpu


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def dataset(name, with_var):
    cov, x, y, y_var = ic.inputs(name)
    targets = ab.MarginalDistribution(y, y_var) if with_var else y
    return cov, x, y, (y_var if with_var else None), ab.RegressionDataset(x, targets)


def create(ctx, cov, x, y, y_var, rank, tol=ic.TOL, max_iterations=1000, rel_tol=1e-12):
    """the C-ABI call: (status, handle or None, information, iterations, residual)"""
    fs = cov.features(x)
    s = fs.as_struct()
    opt = capi.IterativeOptions(rank, rel_tol, tol, max_iterations)
    h = C.c_void_p()
    info = np.full(fs.n, np.nan)
    it, res = C.c_int(-1), C.c_double(np.nan)
    yy = np.ascontiguousarray(y, dtype=np.float64)
    vv = None if y_var is None else np.ascontiguousarray(y_var, dtype=np.float64)
    st = ctx._lib.agp_iterative_fit_create(ctx._h, ctx.kernel(cov), C.byref(s), _p(yy), _p(vv), C.byref(opt), C.byref(h), _p(info),
                                           C.byref(it), C.byref(res))
    return st, (h if h.value else None), info, it.value, res.value


def destroy(ctx, h):
    if h is not None:
        ctx._lib.agp_iterative_fit_destroy(h)


@pytest.mark.parametrize("with_var", [False, True], ids=["no_var", "var"])
@pytest.mark.parametrize("name", sorted(ic.CASES))
def test_information_against_the_dense_fit(ctx, name, with_var):
    cov, x, y, y_var, ds = dataset(name, with_var)
    n = len(y)
    model = ab.gp_from_covariance(cov, context=ctx)
    dense = model.fit(ds).get_fit().information
    A = ic.system(ctx.gram(cov, x), y_var)
    for r in ic.RANKS:
        want = ic.rank_of(r, n)
        fit = model.fit_iterative(ds, preconditioner_rank=want, tolerance=ic.TOL).get_fit()
        assert fit.preconditioner_rank == want and fit.residual <= ic.TOL
        worst = ic.check_information(A, fit.information, dense, y)
        if r == "n":
            assert fit.iterations <= 6, fit.iterations
        host = ic.pcg(A, y, want)[2] if (r in (0, 1, 64) and n <= 777) or r == 0 else "-"
        print(name, "rank", want, "iterations", fit.iterations, "restatement", host, "fractions of the bounds", worst)
        if r == 64:  # determinism: a second fit, the same bits
            again = model.fit_iterative(ds, preconditioner_rank=want, tolerance=ic.TOL).get_fit()
            assert np.array_equal(_bits(again.information), _bits(fit.information))
            assert again.iterations == fit.iterations and again.residual == fit.residual


def test_preconditioner_halves_the_iterations(ctx):
    cov, x, y, _ = ic.inputs(ic.ONE_D)
    st0, h0, _, it0, _ = create(ctx, cov, x, y, None, 0)
    st64, h64, _, it64, _ = create(ctx, cov, x, y, None, 64)
    destroy(ctx, h0)
    destroy(ctx, h64)
    print("iterations: rank 0", it0, "rank 64", it64)
    assert st0 == capi.AGP_OK and st64 == capi.AGP_OK and 2 * it64 < it0


def test_duplicates_stop_the_preconditioner_early(ctx):
    cov, x, y, y_var, ds = dataset("duplicates", True)
    model = ab.gp_from_covariance(cov, context=ctx)
    fit = model.fit_iterative(ds, preconditioner_rank=ic.DUPLICATE_RANK_ASKED, preconditioner_tolerance=ic.DUPLICATE_REL_TOL).get_fit()
    assert 0 < fit.preconditioner_rank <= ic.DUPLICATE_DISTINCT < ic.DUPLICATE_RANK_ASKED
    A = ic.system(ctx.gram(cov, x), y_var)
    ic.check_information(A, fit.information, model.fit(ds).get_fit().information, y)
    print("duplicates: rank", fit.preconditioner_rank, "iterations", fit.iterations)


def test_iteration_count_is_the_first_that_meets_the_criterion(ctx):
    cov, x, y, y_var = ic.inputs("n777_2d")
    st, h, info, its, res = create(ctx, cov, x, y, y_var, 64)
    destroy(ctx, h)
    assert st == capi.AGP_OK and res <= ic.TOL and its > 1
    st2, h2, info2, its2, res2 = create(ctx, cov, x, y, y_var, 64, max_iterations=its - 1)
    assert st2 == capi.AGP_ERR_NOT_CONVERGED and h2 is None and its2 == its - 1 and res2 > ic.TOL
    st3, h3, info3, its3, res3 = create(ctx, cov, x, y, y_var, 64, max_iterations=its)
    destroy(ctx, h3)
    assert st3 == capi.AGP_OK and its3 == its and np.array_equal(_bits(info3), _bits(info)) and res3 == res


@pytest.mark.parametrize("nrhs", [1, 16, 17, 40])
def test_solve_against_the_dense_solve(ctx, nrhs):
    cov, x, y, y_var, ds = dataset("n777_2d", True)
    n = len(y)
    model = ab.gp_from_covariance(cov, context=ctx)
    dense_fit = model.fit(ds).get_fit()
    B = np.asfortranarray(np.random.default_rng(nrhs).standard_normal((n, nrhs)))
    zero = nrhs // 2
    if nrhs > 1:
        B[:, zero] = 0.
    want = np.empty((n, nrhs), order="F")
    ctx._check(ctx._lib.agp_solve(ctx._h, dense_fit._h, _p(B), nrhs, _p(want), capi.HOST), "agp_solve")
    fit = model.fit_iterative(ds, preconditioner_rank=64).get_fit()
    got, its, res = fit.solve(B, return_info=True)
    for c in range(nrhs):
        if nrhs > 1 and c == zero:
            assert its[c] == 0 and res[c] == 0. and not got[:, c].any()
            continue
        assert its[c] > 0 and 0. < res[c] <= ic.TOL
        assert np.abs(got[:, c] - want[:, c]).max() <= ic.PARITY * np.abs(want[:, c]).max(), c
    print("nrhs", nrhs, "iterations", its.min(), "..", its.max())
    # a padded host block: the rows past n and the columns past nrhs keep their bits
    ldo = n + 3
    ob = np.full((ldo, nrhs + 1), np.nan, order="F")
    st = ctx._lib.agp_iterative_solve(ctx._h, fit._h, _p(B), n, nrhs, _p(ob), ldo, capi.HOST, None, None)
    assert st == capi.AGP_OK and np.array_equal(_bits(ob[:n, :nrhs]), _bits(got))
    assert np.all(np.isnan(ob[n:])) and np.all(np.isnan(ob[:, nrhs:]))


@pytest.mark.parametrize("m", [1, 16, 17, 40])
def test_predictions_against_the_dense_model(ctx, m):
    """a non-zero mean function through the Python surface; mean 1e-8 relative, variance 1e-8 k(x*, x*) absolute"""
    cov, x, y, y_var = ic.inputs("n777_2d")
    yy = y + 0.3 * x[:, 0] - 1.
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(yy, y_var))
    model = ab.gp_from_covariance_and_mean(cov, ab.LinearMean(0.3, -1.), context=ctx)
    xs = ic.query_points(m, 2, 10.)
    dense = model.fit(ds).predict(xs).marginal()
    fm = model.fit_iterative(ds, preconditioner_rank=64)
    pred = fm.predict(xs)
    marg = pred.marginal()
    mean = pred.mean()
    assert np.array_equal(mean, marg.mean)
    assert np.abs(mean - dense.mean).max() <= ic.PARITY * np.abs(dense.mean).max()
    prior = ctx.gram_diagonal(cov, xs)
    assert np.all(np.abs(marg.covariance - dense.covariance) <= ic.PARITY * prior)
    with pytest.raises(NotImplementedError):
        pred.joint()
    assert np.abs(fm.get_fit().information - model.fit(ds).get_fit().information).max() <= ic.PARITY * np.abs(
        fm.get_fit().information).max()


def test_status_codes(ctx):
    cov, x, y, _ = ic.inputs(ic.ONE_D)
    st, h, info, its, res = create(ctx, cov, x, y, None, 0, max_iterations=3)
    assert st == capi.AGP_ERR_NOT_CONVERGED and h is None and its == 3 and np.isfinite(res) and res > ic.TOL
    model = ab.gp_from_covariance(cov, context=ctx)
    with pytest.raises(ab.NotConvergedError) as e:
        model.fit_iterative(ab.RegressionDataset(x, y), preconditioner_rank=0, max_iterations=3)
    assert e.value.iterations == 3 and e.value.residual > ic.TOL and e.value.status == capi.AGP_ERR_NOT_CONVERGED
    assert b"converge" in ctx._lib.agp_status_string(capi.AGP_ERR_NOT_CONVERGED)
    n = 777
    for rank in (0, 16):  # an indefinite matrix with a positive diagonal
        st, h, _, its, _ = create(ctx, cov, x[:n], y[:n], np.full(n, -0.5), rank)
        assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and h is None
        print("indefinite: rank", rank, "iterations", its)
    st, h, _, its, _ = create(ctx, cov, x[:n], y[:n], np.full(n, -5.), 16)  # a non-positive diagonal: before any iteration
    assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and h is None and its == 0
    bad_y = y[:n].copy()
    bad_y[5] = np.nan
    assert create(ctx, cov, x[:n], bad_y, None, 16)[0] == capi.AGP_ERR_NAN_INPUT
    bad_x = x[:n].copy()
    bad_x[9, 0] = np.nan
    for rank in (0, 16):
        assert create(ctx, cov, bad_x, y[:n], None, rank)[0] == capi.AGP_ERR_NAN_INPUT
    with pytest.raises(ab.NanInputError):
        model.fit_iterative(ab.RegressionDataset(bad_x, y[:n]))
    # malformed options: nothing is written
    for opt in ((-1, 1e-12, 1e-10, 10), (4, -1., 1e-10, 10), (4, 1e-12, 0., 10), (4, 1e-12, 1e-10, 0)):
        st, h, info, its, res = create(ctx, cov, x[:n], y[:n], None, opt[0], tol=opt[2], max_iterations=opt[3], rel_tol=opt[1])
        assert st == capi.AGP_ERR_INVALID_ARGUMENT and h is None and its == -1 and np.all(np.isnan(info))


def test_measurement_only_noise_as_the_dense_fit(ctx):
    """the fit sees its features as measurements (gp.hpp:288), the predictions see what they are given - as agp_fit_create"""
    _, x, y, y_var = ic.inputs("n777_2d")
    cov = ab.SquaredExponential(1.5, 1.) + ab.measurement_only(ab.IndependentNoise(0.05))
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(y, y_var))
    model = ab.gp_from_covariance(cov, context=ctx)
    dense, fm = model.fit(ds), model.fit_iterative(ds, preconditioner_rank=64)
    a, b = fm.get_fit().information, dense.get_fit().information
    assert np.abs(a - b).max() <= ic.PARITY * np.abs(b).max()
    xs = np.vstack([ic.query_points(19, 2, 10.), x[:3]])
    for which in ("predict", "predict_with_measurement_noise"):
        got, want = getattr(fm, which)(xs).marginal(), getattr(dense, which)(xs).marginal()
        assert np.abs(got.mean - want.mean).max() <= ic.PARITY * np.abs(want.mean).max()
        assert np.all(np.abs(got.covariance - want.covariance) <= ic.PARITY * 1.0025)
