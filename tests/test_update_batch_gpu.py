"""agp_fit_update_batch (include/albatross_amd.h; csrc/update_batch.hip) and ab.update_batch: FitModel::update for B fits of
one size in lock step - against the oracle's literal _update_impl restatement and the per-handle update() loop, at the
edges of the 128-row diagonal block, the 128 x 32 covariance tile and the phantom padding, on either side of the
tile-shape threshold of the batched MFMA product, with uniform and mixed trees, old fits of mixed origin, nesting,
device-resident inputs, failed problems and malformed arguments.

Bounds: the project's own for this operation (tests/test_update_dense_gpu.py) against the oracle - information, mean and
solve 1e-8 relative, marginal and joint covariance 1e-8 relative + 1e-10, L L^T - M 1e-10 max|M|, log-determinant
1e-8 n; the batch against the update() loop within twice the relative bound, since both sit inside it."""
import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import update_batch_cases as ubc

pytestmark = pytest.mark.gpu


def _close(got, ref, relative, absolute, what):
    err, bound = np.abs(np.asarray(got) - np.asarray(ref)).max(), relative * np.abs(ref).max() + absolute
    print(f"{what}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def _check_against(fm, ref_info, ref_predict, xs, relative, label):
    """information and the three predictions of one grown FitModel against a reference"""
    _close(fm.get_fit().information, ref_info, relative, 0., f"{label} information")
    om, ov, oj = ref_predict
    pred = fm.predict(xs)
    _close(pred.mean(), om, relative, 0., f"{label} mean")
    _close(pred.marginal().covariance, ov, relative, 1e-10, f"{label} marginal")
    _close(pred.joint().covariance, oj, relative, 1e-10, f"{label} joint")


def _oracle_predict(of, xs):
    om, ov = of.predict_marginal(xs)
    return om, ov, of.predict_joint(xs)[1]


def _single_predict(fm, xs):
    pred = fm.predict(xs)
    return pred.mean(), pred.marginal().covariance, pred.joint().covariance


def _gemm_small_limit():
    """the number of 128 x 128 tiles below which launch_gemm_nt_sub_batched switches to smaller tiles, read from its code;
    the rule itself (csrc/update_plan.h: plan_nt_sub) is asked of the library: a triangular product of 3 large tiles per
    problem gets them from tiles * count >= limit on and smaller ones below"""
    import os
    import re
    import update_plan_cases as uc
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "albatross_amd", "csrc", "gemm.hip")).read()
    m = re.search(r"AGP_GEMM_SMALL_LIMIT.*?atoi\(e\)\s*:\s*(\d+)", text)
    assert m and "tiles * count < small_limit" in text
    limit = int(m.group(1))
    below = (limit - 1) // 3
    assert uc.planned_nt_sub(256, 256, 128, True, False, False, below, limit)["edge"] < 128
    assert uc.planned_nt_sub(256, 256, 128, True, False, False, below + 1, limit)["edge"] == 128
    return limit


def _threshold_counts():
    # the Schur complement of m = 256 new points is a triangular product of 2 x 2 tiles of 128: 3 tiles per problem; the
    # launch uses 128-tiles from tiles * count >= limit on
    limit = _gemm_small_limit()
    below = (limit - 1) // 3
    return below, below + 1


CASES = [
    # n0, m, count, kind, with_variance, origin
    (128, 1, 2, "fast1", False, "batch"),
    (128, 127, 3, "fast2", True, "batch"),
    (128, 128, 2, "fast3", False, "batch"),
    (128, 129, 2, "mixed", True, "batch"),
    (256, 33, 5, "update_tree", True, "mixed"),
    (250, 80, 3, "dim4", True, "batch"),        # phantom rows
    (130, 129, 2, "scaling", False, "batch"),   # phantom rows
    (384, 64, 1, "fast3", True, "batch"),       # count = 1 goes through the same code
    (128, 256, "below", "fast3", False, "batch"),
    (128, 256, "above", "fast3", True, "batch"),
]


@pytest.mark.parametrize("n0,m,count,kind,with_variance,origin", CASES)
def test_update_batch_matches_oracle_and_update_loop(ctx, n0, m, count, kind, with_variance, origin):
    if count in ("below", "above"):
        count = _threshold_counts()[0 if count == "below" else 1]
        assert (3 * count < _gemm_small_limit()) == (count == _threshold_counts()[0])
    n = n0 + m
    # a new observation AT an old point: IndependentNoise correlates them (plain features, by value); only with target
    # variances, which keep the block matrix definite then
    probs = ubc.problems(kind, n, count, n0 + m + count, with_variance, duplicate_at=(n0 + 1, 3) if with_variance else None)
    models, fms = ubc.fit_old(ctx, probs, n0, origin)
    new = slice(n0, n)
    grown = ab.update_batch(fms, [p.dataset(new) for p in probs])
    assert len(grown) == count
    xs = np.random.default_rng(5).uniform(0., 10., (33, probs[0].x.shape[1]))
    full = range(count) if count <= 5 else (0, count // 2, count - 1)  # predictions, solve and factor of these problems
    worst = 0.
    for b in range(count):
        p, fm = probs[b], grown[b]
        assert isinstance(fm.get_fit(), ab.GPFit) and fm.get_fit().rows() == n
        assert np.array_equal(fm.get_fit().train_features, p.x)
        of = p.oracle_update(p.oracle(slice(0, n0)), new)
        info = of.information
        _close(fm.get_fit().information, info, 1e-8, 0., f"problem {b} information vs oracle")
        single = fms[b].update(p.dataset(new))
        _close(fm.get_fit().information, single.get_fit().information, 2e-8, 0., f"problem {b} information vs update()")
        worst = max(worst, np.abs(fm.get_fit().information - single.get_fit().information).max() / np.abs(info).max())
        assert abs(fm.get_fit().log_determinant - single.get_fit().log_determinant) <= 2e-8 * n
        if b not in full:
            continue
        _check_against(fm, info, _oracle_predict(of, xs), xs, 1e-8, f"problem {b} vs oracle")
        _check_against(fm, single.get_fit().information, _single_predict(single, xs), xs, 2e-8, f"problem {b} vs update()")
        rhs = np.random.default_rng(b).standard_normal((n, 3))
        _close(fm.get_fit().solve(rhs), of.solve(rhs), 1e-8, 0., f"problem {b} solve")
        _close(fm.get_fit().solve(rhs[:, 0]), of.solve(rhs[:, 0]), 1e-8, 0., f"problem {b} solve, one vector")
        M = ubc.block_matrix(p, n0, n)
        L = fm.get_fit().factor()
        _close(L @ L.T, M, 1e-10, 0., f"problem {b} L L^T")
        assert abs(fm.get_fit().log_determinant - np.linalg.slogdet(M)[1]) <= 1e-8 * n
    print(f"n0={n0} m={m} count={count} {kind}: largest relative difference of the information from the update() loop {worst:.3e}")


def test_mixed_origin_old_fits_stay_intact_and_grown_fits_stand_alone(ctx):
    """two handles of one fit_batch call plus one from fit(): no constant stride between the old fits.  The old fits
    predict the same bits before and after, the grown fits predict correctly after the old fits are gone, and the grown
    handles can be destroyed in any order."""
    n0, m, count = 256, 40, 3
    probs = ubc.problems("fast3", n0 + m, count, 41, True)
    models, fms = ubc.fit_old(ctx, probs, n0, "mixed")
    xs = np.random.default_rng(6).uniform(0., 10., (20, 3))
    before = [_single_predict(fm, xs) for fm in fms]
    grown = ab.update_batch(fms, [p.dataset(slice(n0, n0 + m)) for p in probs])
    for fm, ref in zip(fms, before):
        for got, want in zip(_single_predict(fm, xs), ref):
            assert np.array_equal(got, want)
    refs = [_single_predict(fm.update(p.dataset(slice(n0, n0 + m))), xs) for fm, p in zip(fms, probs)]
    infos = [fm.update(p.dataset(slice(n0, n0 + m))).get_fit().information for fm, p in zip(fms, probs)]
    del fms, fm  # destroys the old handles (and the slab of the fit_batch call)
    ctx.synchronize()
    for b in (1, 0, 2):
        _check_against(grown[b], infos[b], refs[b], xs, 2e-8, f"problem {b} after the old fits were destroyed")
    # the fits of the batch without phantom rows run agp_predict_batch's lock-step path
    batch = ab.predict_batch(grown, xs, what="joint")
    for b in range(count):
        _close(batch[b].mean, refs[b][0], 1e-8, 0., f"predict_batch mean {b}")
        _close(batch[b].covariance, refs[b][2], 1e-8, 1e-10, f"predict_batch covariance {b}")
    marg = ab.predict_batch(grown, xs, what="marginal")
    for b in range(count):
        _close(marg[b].covariance, refs[b][1], 1e-8, 1e-10, f"predict_batch variance {b}")
    middle = grown[1]
    grown[1] = None
    del middle  # out of order: the allocation goes with the last handle
    _close(grown[2].predict(xs).mean(), refs[2][0], 2e-8, 0., "after destroying a neighbour")
    _close(grown[0].predict(xs).mean(), refs[0][0], 2e-8, 0., "after destroying a neighbour")
    del grown


def test_nested_batched_updates(ctx):
    """update_batch of the results of update_batch, 256 -> 384 -> 424, then once more from 424 (phantom rows from then on)"""
    sizes, count = [256, 384, 424, 470], 3
    probs = ubc.problems("update_tree", sizes[-1], count, 43, True)
    models, fms = ubc.fit_old(ctx, probs, sizes[0])
    ofs = [p.oracle(slice(0, sizes[0])) for p in probs]
    xs = np.random.default_rng(7).uniform(0., 10., (33, 3))
    for lo, hi in zip(sizes[:-1], sizes[1:]):
        sl = slice(lo, hi)
        fms = ab.update_batch(fms, [p.dataset(sl) for p in probs])
        ofs = [p.oracle_update(of, sl) for p, of in zip(probs, ofs)]
        for b in range(count):
            assert fms[b].get_fit().rows() == hi
            _check_against(fms[b], ofs[b].information, _oracle_predict(ofs[b], xs), xs, 1e-8, f"{lo} -> {hi} problem {b}")
    # ... and the single entry accepts a fit of the batch
    again = fms[0].update(ab.RegressionDataset(xs[:5], np.zeros(5)))
    assert again.get_fit().rows() == sizes[-1] + 5


def test_capi_outputs_determinism_and_device_inputs(ctx):
    """information / log_det host outputs agree with the downloads; two identical calls give the same bits; device-resident
    x_new / y_new / y_var_new give the same bits as host inputs"""
    n0, m, count = 250, 37, 3  # phantom rows: the information output is compacted to the real rows
    probs = ubc.problems("scaling", n0 + m, count, 47, True)
    models, fms = ubc.fit_old(ctx, probs, n0)
    sl = slice(n0, n0 + m)
    results = []
    for where in ("host", "host", "device"):
        call = ubc.CapiCall(ctx, models, fms, probs, sl, where)
        try:
            assert call.run() == capi.AGP_OK
            assert list(call.status) == [capi.AGP_OK] * count
            fits = call.fits()
            for b, fit in enumerate(fits):
                assert np.array_equal(fit.information, call.information[:, b])
                assert fit.log_determinant == call.log_det[b]
                assert ctx._lib.agp_fit_failed_pivot(fit._h) == -1
            results.append((call.information.copy(), call.log_det.copy()))
        finally:
            call.close()
    for info, log_det in results[1:]:
        assert np.array_equal(info, results[0][0]) and np.array_equal(log_det, results[0][1])
    single = [fm.update(p.dataset(sl)).get_fit().information for fm, p in zip(fms, probs)]
    for b in range(count):
        _close(results[0][0][:, b], single[b], 2e-8, 0., f"problem {b} information output")


def test_nan_problem_fails_alone(ctx):
    n0, m, count = 128, 40, 3
    probs = ubc.problems("fast2", n0 + m, count, 53, False)
    probs[1].x[n0 + 4, 0] = np.nan
    models, fms = ubc.fit_old(ctx, probs, n0)
    sl = slice(n0, n0 + m)
    call = ubc.CapiCall(ctx, models, fms, probs, sl)
    try:
        assert call.run() == capi.AGP_OK
        assert list(call.status) == [capi.AGP_OK, capi.AGP_ERR_NAN_INPUT, capi.AGP_OK]
        fits = call.fits()
        assert np.all(call.information[:, 1] == -7.0)  # a failed problem's column is left untouched
        for b in (0, 2):
            of = probs[b].oracle_update(probs[b].oracle(slice(0, n0)), sl)
            _close(call.information[:, b], of.information, 1e-8, 0., f"neighbour {b} of the NaN problem")
        del fits
    finally:
        call.close()
    with pytest.raises(ab.NanInputError, match="problem 1"):
        ab.update_batch(fms, [p.dataset(sl) for p in probs])


def test_not_positive_definite_problem_reports_its_pivot(ctx):
    """the construction of test_device_update_reports_not_positive_definite in problem 1 of 3"""
    n0, m, count = 200, 20, 3
    rng = np.random.default_rng(1)
    probs = []
    for b in range(count):
        x = rng.uniform(0., 10., (n0 + m, 2))
        y = np.concatenate([np.sin(x[:n0]).sum(axis=1), np.zeros(m)])
        var = np.concatenate([np.full(n0, 0.1), np.zeros(m) if b == 1 else np.full(m, 0.1)])
        if b == 1:
            x[n0 + 7] = x[n0 + 2]  # a duplicate among the NEW points whose negative variance makes the Schur complement
            var[n0 + 7] = -1e-3    # indefinite at exactly that pivot
        probs.append(ubc.Problem(ab.SquaredExponential(1.5, 1.0), None, x, y, var))
    models, fms = ubc.fit_old(ctx, probs, n0, "mixed")
    sl = slice(n0, n0 + m)
    call = ubc.CapiCall(ctx, models, fms, probs, sl)
    try:
        assert call.run() == capi.AGP_OK
        assert list(call.status) == [capi.AGP_OK, capi.AGP_ERR_NOT_POSITIVE_DEFINITE, capi.AGP_OK]
        fits = call.fits()
        assert ctx._lib.agp_fit_failed_pivot(fits[1]._h) == 207
        assert np.all(call.information[:, 1] == -7.0)
        for b in (0, 2):
            of = probs[b].oracle_update(probs[b].oracle(slice(0, n0)), sl)
            _close(call.information[:, b], of.information, 1e-8, 0., f"neighbour {b} of the indefinite problem")
        del fits
    finally:
        call.close()
    with pytest.raises(ab.NotPositiveDefiniteError, match=r"problem 1 \(pivot 207\)"):
        ab.update_batch(fms, [p.dataset(sl) for p in probs])


def test_argument_errors_write_nothing(ctx):
    n0, m, count = 256, 10, 2
    probs = ubc.problems("fast3", n0 + m, count, 59, False)
    models, fms = ubc.fit_old(ctx, probs, n0)
    other = ubc.fit_old(ctx, ubc.problems("fast3", 128 + m, 1, 61, False), 128)[1][0]
    mixed_model = probs[0].model(ctx)
    mixed_model.precision = "mixed"
    mixed = mixed_model.fit(probs[0].dataset(slice(0, n0)))
    assert mixed.get_fit().mixed_precision
    call = ubc.CapiCall(ctx, models, fms, probs, slice(n0, n0 + m))
    try:
        for kwargs in ({"count": 0}, {"olds": [call.olds[0], other.get_fit()._h.value]}, {"ldi": n0 + m - 1},
                       {"olds": [mixed.get_fit()._h.value, call.olds[1]]}):
            assert call.run(**kwargs) == capi.AGP_ERR_INVALID_ARGUMENT, kwargs
            assert list(call.status) == [-99] * count and [call.out[b] for b in range(count)] == [0xdead] * count
            assert np.all(call.information == -7.0) and np.all(call.log_det == -7.0)
        assert call.run() == capi.AGP_OK  # the same arguments, well formed
        del_fits = call.fits()
        del del_fits
    finally:
        call.close()
