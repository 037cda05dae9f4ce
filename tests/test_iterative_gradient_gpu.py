"""The probe gradient of the matrix-free fit on the device: agp_iterative_nll_gradient (csrc/iterative.hip) and
IterativeFitModel.log_likelihood_gradient.

    dNLL / dtheta_p = 1/2 tr(A^-1 dA_p) - 1/2 alpha^T dA_p alpha,  the trace from probes:  s_cp = (A^-1 z_c)^T dA_p z_c

The inputs, the float64 numpy restatement and the exact dense gradient are tests/gram_tangent_cases.py's
(tests/test_gram_tangent_host.py runs the same checks from numpy alone).  Bars: identity probes Z = sqrt(n) I make the
estimator exact - 1e-8 s_p against the dense gradient of the same model and 1e-7 s_p against the oracle's, s_p the scale of
tests/test_nll_gradient_gpu.py, at a fit tolerance of 1e-12 and cond(A) <= 2e3; a seeded sample is within 1e-8 of its own
scale sum |w_ic| |dA_ij| |z_jc| of numpy's value with an exact solve; the seeded estimate is within 4 of its own standard
errors of the dense gradient."""
import ctypes as C
import math

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import gram_path_cases as gp
import gram_tangent_cases as tc
import test_nll_gradient_gpu as ng

pytestmark = pytest.mark.gpu

FIT_TOL = 1e-12


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def fitted(ctx, name, rank, **kw):
    cov, x, y = tc.gradient_inputs(name)
    model = ab.gp_from_covariance(cov, context=ctx)
    ds = ab.RegressionDataset(x, y)
    kw.setdefault("tolerance", FIT_TOL)
    return model, ds, model.fit_iterative(ds, preconditioner_rank=rank, **kw)


def c_gradient(ctx, fm, t, seed=0, probes=None, slots=None, location=capi.HOST, extra=2):
    """the C entry on canary outputs: (status, grad, stderr, samples (t x P), iterations, residual, the raw buffers)"""
    cov = fm.get_model().covariance_function_
    table3 = cov.param_slots()[0]
    pairs = [(node, param) for node, param, _ in table3] if slots is None else slots
    P = len(pairs)
    arr = (capi.GradientSlot * max(1, P))(*[capi.GradientSlot(a, b) for a, b in pairs])
    n = fm.get_fit().n
    grad, se = gp.canaries(P + extra), gp.canaries(P + extra)
    lds = max(t, 1) + extra
    samples = gp.canaries(lds * (P + 1))
    its, res = np.full(max(t, 1) + extra, -7, dtype=np.int32), gp.canaries(max(t, 1) + extra)
    zp, ldp, keep = None, 0, None
    if probes is not None and location == capi.DEVICE:
        keep = ctx.to_device(np.ascontiguousarray(np.asarray(probes).T))  # (the bytes of the column-major n x t matrix)
        zp, ldp = C.c_void_p(keep.ptr), n
    elif probes is not None:
        keep = np.asfortranarray(probes)
        zp, ldp = _p(keep), n
    st = ctx._lib.agp_iterative_nll_gradient(ctx._h, fm.get_fit()._h, P, arr, None, n, t, seed, zp, ldp, location, _p(grad), _p(se),
                                             _p(samples), lds, _p(its), _p(res))
    S = samples.reshape((lds, P + 1), order="F")
    return st, grad[:P].copy(), se[:P].copy(), S[:max(t, 0), :P].copy(), its, res, (grad, se, samples)


# ---- 1. exact with identity probes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [0, 64])
@pytest.mark.parametrize("name", ["n65_3d", "n130_3d"])
def test_identity_probes_are_exact(ctx, name, rank):
    tc.identity_case(name)
    model, ds, fm = fitted(ctx, name, rank)
    _, x, y = tc.gradient_inputs(name)
    n = len(y)
    grad, stderr = fm.log_likelihood_gradient(probes=math.sqrt(n) * np.eye(n))
    assert set(grad) == set(stderr) == set(model.get_params())
    _, dense = model.log_likelihood_gradient(ds)
    want, scale, _ = ng.reference_gradient(model, x, y)
    host, _ = tc.dense_gradient_nll(name)
    for nm in want:
        a, b = abs(grad[nm] - dense[nm]) / scale[nm], abs(grad[nm] - want[nm]) / scale[nm]
        print(f"{name} rank {rank} {nm}: {a:.3g} s_p from the dense gradient, {b:.3g} s_p from the oracle's")
        assert a <= 1e-8 and b <= 1e-7, (nm, grad[nm], dense[nm], want[nm], scale[nm])
        assert abs(-grad[nm] - host[nm]) <= 1e-8 * scale[nm], nm
    assert fm.gradient_iterations.shape == (n,) and np.all(fm.gradient_iterations > 0)
    assert np.all(fm.gradient_residual <= FIT_TOL)


# ---- 2. seeded probes against their definition ------------------------------------------------------------------------------------
def _check_samples(ctx, name, rank, t, seed):
    model, ds, fm = fitted(ctx, name, rank)
    n = fm.get_fit().n
    st, grad, se, S, its, res, _ = c_gradient(ctx, fm, t, seed)
    assert st == capi.AGP_OK, st
    Z = tc.rademacher(seed, n, t)
    _, _, want, scales = tc.gradient_restated(name, Z)
    names = [nm for _, _, nm in model.covariance_function_.param_slots()[0]]
    assert len(set(names)) == len(names)
    # the alpha term of every slot from the public forms entry, U = V = the fit's information vector on the features as
    # measurements: grad_nll is then the stated function of the returned samples to 1e-12 relative
    _, x, _ = tc.gradient_inputs(name)
    info = fm.get_fit().information
    a_forms = ab.gram_tangent_forms(model.covariance_function_, ab.Measurement(x), info, info, context=ctx)
    worst = 0.
    for p, nm in enumerate(names):
        r = np.abs(S[:, p] - want[nm]) / scales[nm]
        worst = max(worst, float(r.max()))
        assert np.all(r <= 1e-8), (name, t, nm, float(r.max()))
        tau = S[:, p].sum() / t
        a_term = float(tc.dense_system(name)[2] @ tc.dense_system(name)[1][nm] @ tc.dense_system(name)[2])
        assert abs(grad[p] - (0.5 * tau - 0.5 * a_term)) <= 1e-8 * (0.5 * abs(tau) + 0.5 * abs(a_term)), nm
        a_dev = float(a_forms[nm][0])
        assert abs(grad[p] - (0.5 * tau - 0.5 * a_dev)) <= 1e-12 * (0.5 * abs(tau) + 0.5 * abs(a_dev)), (nm, grad[p], tau, a_dev)
        if t > 1:
            want_se = 0.5 * math.sqrt(((S[:, p] - tau) ** 2).sum() / (t * (t - 1)))
            assert abs(se[p] - want_se) <= 1e-12 * want_se, (nm, se[p], want_se)
        else:
            assert math.isnan(se[p])
    # grad_nll is the stated function of the samples: the alpha term it implies is the same for every t (checked by the caller)
    print(f"{name} rank {rank} t {t}: worst sample error {worst:.3g} of its scale; iterations {its[:t].min()}..{its[:t].max()}")
    assert np.all(its[:t] > 0) and np.all(res[:t] <= FIT_TOL) and np.all(its[t:] == -7) and gp.all_canary(res[t:])
    return grad, se, S


def test_seeded_samples_match_their_definition_n65(ctx):
    out = {t: _check_samples(ctx, "n65_3d", 64, t, seed=7) for t in (1, 16, 17)}
    g1, g16, g17 = (out[t] for t in (1, 16, 17))
    # column c depends on (seed, c) alone: the samples of t = 16 are the first 16 of t = 17, of t = 1 the first
    assert same_bits(g16[2], g17[2][:16]) and same_bits(g1[2], g17[2][:1])
    # grad = tau / 2 - a / 2 with ONE alpha term a, whatever t: to 1e-12 relative
    for p in range(g16[0].shape[0]):
        a = [0.5 * S[:, p].sum() / S.shape[0] - g[p] for g, _, S in (g1, g16, g17)]
        size = max(abs(v) for v in a) + abs(0.5 * g17[2][:, p].mean())
        assert max(a) - min(a) <= 1e-12 * size, (p, a)


def test_seeded_samples_match_their_definition_n777(ctx):
    _check_samples(ctx, "n777_2d", 64, 64, seed=1)


# ---- 3. the estimate is usable -----------------------------------------------------------------------------------------------------
def test_estimate_within_four_standard_errors(ctx):
    model, ds, fm = fitted(ctx, "n777_2d", 64)
    grad, stderr = fm.log_likelihood_gradient(num_probes=64, seed=1)
    _, dense = model.log_likelihood_gradient(ds)
    for nm in dense:
        z = abs(grad[nm] - dense[nm]) / stderr[nm]
        print(f"n777_2d {nm}: {grad[nm]:.6g} +- {stderr[nm]:.3g}, dense {dense[nm]:.6g}: {z:.2f} standard errors")
        assert z <= 4., (nm, z)


# ---- 4. parameter kinds ---------------------------------------------------------------------------------------------------------------
def test_mean_scaling_and_shared_names(ctx):
    rng = np.random.default_rng(11)
    n = 65
    x = rng.uniform(0., 6., (n, 3))
    y = np.sin(x).sum(axis=1) + 0.3 * x[:, 0] + 0.1 * rng.standard_normal(n)
    Z = math.sqrt(n) * np.eye(n)
    # a ScalingTerm slot and a LinearMean
    cov, model = ng._elevation_model(ctx)
    ds = ab.RegressionDataset(x, y)
    fm = model.fit_iterative(ds, preconditioner_rank=32, tolerance=FIT_TOL)
    grad, stderr, samples = fm.log_likelihood_gradient(probes=Z, return_samples=True)
    _, dense = model.log_likelihood_gradient(ds)
    want, scale, _ = ng.reference_gradient(model, x, y)
    assert set(grad) == set(model.get_params())
    for nm in dense:
        assert abs(grad[nm] - dense[nm]) <= 1e-8 * scale[nm] and abs(grad[nm] - want[nm]) <= 1e-7 * scale[nm], (nm, grad[nm], dense[nm])
    for nm in model.mean_function_.get_params():
        assert stderr[nm] == 0. and nm not in samples
    assert any("elevation" in nm for nm in samples)
    # two leaves share their parameter names: the samples of the two slots are summed before the standard error is taken
    cov2 = ab.SquaredExponential(1.0, 1.0) + ab.SquaredExponential(1.0, 1.0) * ab.Constant(0.5) + ab.IndependentNoise(0.1)
    model2 = ab.gp_from_covariance(cov2, context=ctx)
    fm2 = model2.fit_iterative(ds, preconditioner_rank=32, tolerance=FIT_TOL)
    g2, s2, smp = fm2.log_likelihood_gradient(num_probes=17, seed=3, return_samples=True)
    st, _, _, S, _, _, _ = c_gradient(ctx, fm2, 17, 3)
    names = [nm for _, _, nm in cov2.param_slots()[0]]
    assert st == capi.AGP_OK and len(names) == 6 and len(set(names)) == 4
    for nm in set(names):
        summed = sum(S[:, p] for p, q in enumerate(names) if q == nm)
        assert same_bits(smp[nm], summed)
        tau = summed.sum() / 17
        assert abs(s2[nm] - 0.5 * math.sqrt(((summed - tau) ** 2).sum() / (17 * 16))) <= 1e-12 * s2[nm]
    exact, _ = fm2.log_likelihood_gradient(probes=Z)
    _, dense2 = model2.log_likelihood_gradient(ds)
    _, scale2, _ = ng.reference_gradient(model2, x, y)
    for nm in dense2:
        assert abs(exact[nm] - dense2[nm]) <= 1e-8 * scale2[nm], (nm, exact[nm], dense2[nm])


# ---- 5. statuses ------------------------------------------------------------------------------------------------------------------------
def test_statuses(ctx):
    model, ds, fm = fitted(ctx, "n65_3d", 0)
    for bad in ([(99, 0)], [(2, 0)], [(0, 5)]):  # no such node, the sum (not a leaf), no such parameter
        st, _, _, _, its, res, raw = c_gradient(ctx, fm, 4, slots=bad)
        assert st == capi.AGP_ERR_INVALID_ARGUMENT and all(gp.all_canary(b) for b in raw) and np.all(its == -7), bad
    for t in (0, -1):
        st, _, _, _, its, _, raw = c_gradient(ctx, fm, t)
        assert st == capi.AGP_ERR_INVALID_ARGUMENT and all(gp.all_canary(b) for b in raw)
    with pytest.raises(ValueError):
        fm.log_likelihood_gradient(num_probes=0)
    # y = 0 converges in 0 iterations whatever max_iterations; one iteration is not enough for a probe
    cov, x, _ = tc.gradient_inputs("n65_3d")
    zero = model.fit_iterative(ab.RegressionDataset(x, np.zeros(len(x))), preconditioner_rank=0, max_iterations=1)
    assert zero.get_fit().iterations == 0 and not zero.get_fit().information.any()
    st, _, _, _, its, res, raw = c_gradient(ctx, zero, 3, seed=2)
    assert st == capi.AGP_ERR_NOT_CONVERGED and all(gp.all_canary(b) for b in raw)
    assert np.all(its[:3] == 1) and np.all(res[:3] > 1e-10) and np.all(its[3:] == -7)
    with pytest.raises(ab.NotConvergedError) as e:
        zero.log_likelihood_gradient(num_probes=3, seed=2)
    assert np.all(e.value.iterations == 1) and np.all(e.value.residual > 1e-10) and e.value.status == capi.AGP_ERR_NOT_CONVERGED
    with pytest.raises(ValueError):
        model.fit_iterative(ab.RegressionDataset([ab.LinearCombination([0.7, 2.9], [1., -1.])], np.zeros(1)))


# ---- 6. bits ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits_and_the_handle_is_not_modified(ctx):
    model, ds, fm = fitted(ctx, "n65_3d", 64)
    fit = fm.get_fit()
    n = fit.n
    info = np.empty(n)
    ctx._check(ctx._lib.agp_iterative_fit_download_information(ctx._h, fit._h, _p(info)), "download")
    rhs = np.random.default_rng(5).standard_normal((n, 3))
    before = fit.solve(rhs)
    a = c_gradient(ctx, fm, 17, seed=9)
    b = c_gradient(ctx, fm, 17, seed=9)
    assert a[0] == b[0] == capi.AGP_OK
    assert all(same_bits(u, v) for u, v in zip(a[6], b[6])) and np.array_equal(a[4], b[4]) and same_bits(a[5], b[5])
    # the caller's own probes at either location: the bits of the seeded call whose probes they restate
    for location in (capi.HOST, capi.DEVICE):
        h = c_gradient(ctx, fm, 17, probes=tc.rademacher(9, n, 17), location=location)
        assert h[0] == capi.AGP_OK and same_bits(h[3], a[3]) and same_bits(h[1], a[1]) and same_bits(h[2], a[2]), location
    again = np.empty(n)
    ctx._check(ctx._lib.agp_iterative_fit_download_information(ctx._h, fit._h, _p(again)), "download")
    assert same_bits(info, again) and same_bits(info, fit.information)
    assert same_bits(before, fit.solve(rhs))
