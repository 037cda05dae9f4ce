"""GPU tests of GP RANSAC: agp_ransac_score_trials against the numpy restatement of tests/ransac_cases.py, its limits
and status path, and the model wrapper end to end.

Bound on a metric: |m - m_ref| <= 1e-8 max(1, |m_ref|), the bar predictions are held to against the oracle; the case
builder asserts that the restatement's two routes (Cholesky, solve) agree within a tenth of it on the same inputs."""
import ctypes as C
import math

import numpy as np
import pytest

import albatross_amd as ab
import ransac_cases as rc
from albatross_amd import _capi as capi

pytestmark = pytest.mark.gpu

_CASES = {}
CASE_NAMES = ["ten_points", "ten_points_mean", "singletons", "sixteen", "ragged", "ragged_var", "sixteen_mean"]


def case(name, ctx):
    """(problem, trials, the restatement's score_all): built once, shared and left unchanged"""
    if name not in _CASES:
        rng = np.random.default_rng(len(name))
        if name.startswith("ten_points"):
            problem = rc.ten_point_problem(context=ctx, with_mean=name.endswith("mean"))
            trials = rc.trials_for(problem, rng, 20)
        else:
            grouping = name.split("_")[0]
            problem = rc.synthetic_problem(grouping, with_var=name.endswith("var"), with_mean=name.endswith("mean"), context=ctx)
            trials = rc.trials_for(problem, rng, 65 if grouping == "ragged" else 20)
            if grouping == "ragged":
                trials[-1] = [4]  # the 17-point group as the only candidate
        _CASES[name] = (problem, trials, rc.assert_routes_agree(problem, trials))
    return _CASES[name]


def strategy_for(problem, kind, is_valid=None, consensus=None):
    inlier = {rc.NLL_JOINT: ab.NegativeLogLikelihood("joint"), rc.NLL_MARGINAL: ab.NegativeLogLikelihood("marginal"),
              rc.CHI_SQUARED_CDF: ab.ChiSquaredCdf()}[kind]
    return ab.GaussianProcessRansacStrategy(inlier, consensus or ab.FeatureCountConsensusMetric(),
                                            is_valid or ab.AlwaysAcceptCandidateMetric(), problem.indexer())


def scorer_for(problem, kind, threshold, **kw):
    return ab.GPRansacScorer(problem.model, problem.dataset(), strategy_for(problem, kind, **kw), threshold)


def test_case_shapes(ctx):
    """the shapes the cases are chosen for are really there: s = 1, 17, 64, 65 and 256 candidate points, trials of 1, 3
    and 16 groups, the first and the last groups, a tile boundary inside the grouping"""
    problem, trials, _ = case("ragged", ctx)
    sizes = {len(problem.points(t)) for t in trials}
    assert {1, 64, 65} <= sizes and max(sizes) <= 256 and len(trials) == 65
    assert {len(t) for t in trials} >= {1, 3, 16}
    assert {1, 17, 64, 65} <= sizes and [len(g) for g in problem.groups[:7]] == rc.RAGGED[:7]
    assert any(0 in t for t in trials) and any(len(problem.groups) - 1 in t for t in trials)
    problem16, trials16, _ = case("sixteen", ctx)
    assert 256 in {len(problem16.points(t)) for t in trials16}
    assert len(problem16.groups[-1]) == 301 - 18 * 16


@pytest.mark.parametrize("metric", list(rc.METRICS))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_metric_matrix(ctx, name, metric):
    problem, trials, ref = case(name, ctx)
    kind = rc.METRICS[metric]
    want = ref[0][kind]
    out = scorer_for(problem, kind, 1.).score_raw(trials)
    got = out["metric"]
    assert np.all(out["status"] == capi.AGP_OK)
    for t, positions in enumerate(trials):  # NaN exactly at the trial's candidates
        assert set(np.flatnonzero(np.isnan(got[:, t]))) == set(positions), (t, positions)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(1., np.abs(want[ok]))
    print(f"{name} {metric}: max error {err.max():.3e}")
    assert err.max() <= rc.METRIC_BOUND, err.max()
    assert np.abs(out["candidate_quadratic"] - ref[1]).max() <= rc.METRIC_BOUND * max(1., np.abs(ref[1]).max())
    assert np.abs(out["candidate_log_det"] - ref[2]).max() <= rc.METRIC_BOUND * max(1., np.abs(ref[2]).max())


@pytest.mark.parametrize("n_trials", [1, 2])
def test_few_trials(ctx, n_trials):
    problem, trials, ref = case("ragged", ctx)
    for first in (0, 4):
        out = scorer_for(problem, rc.NLL_JOINT, 1.).score_raw(trials[first:first + n_trials])
        want = ref[0][rc.NLL_JOINT][:, first:first + n_trials]
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(out["metric"]), ~ok)
        assert (np.abs(out["metric"][ok] - want[ok]) / np.maximum(1., np.abs(want[ok]))).max() <= rc.METRIC_BOUND


@pytest.mark.parametrize("name,metric,threshold", [("ragged", "chi_squared_cdf", 0.999), ("ragged_var", "nll_joint", 30.),
                                                   ("singletons", "nll_marginal", 1.5), ("ten_points", "nll_joint", 1.)])
def test_accept_bits_and_counts(ctx, name, metric, threshold):
    problem, trials, ref = case(name, ctx)
    kind = rc.METRICS[metric]
    want = ref[0][kind]
    values = want[~np.isnan(want)]
    gap = np.abs(values - threshold).min()
    print(f"{name} {metric}: nearest reference metric to the threshold {threshold} is {gap:.3e} away")
    assert gap > 1e-6 * max(1., abs(threshold))  # the condition, on the reference values alone
    out = scorer_for(problem, kind, threshold).score_raw(trials)
    accept = want <= threshold
    assert np.array_equal(out["metric"] <= threshold, accept)
    sizes = np.array([len(g) for g in problem.groups])
    assert np.array_equal(out["inlier_groups"], accept.sum(axis=0))
    assert np.array_equal(out["inlier_points"], (accept * sizes[:, None]).sum(axis=0))
    assert 0 < accept.sum() < accept.size
    assert np.abs(out["candidate_quadratic"] - ref[1]).max() <= rc.METRIC_BOUND * max(1., np.abs(ref[1]).max())
    assert np.abs(out["candidate_log_det"] - ref[2]).max() <= rc.METRIC_BOUND * max(1., np.abs(ref[2]).max())


@pytest.mark.parametrize("metric", list(rc.METRICS))
def test_a_trial_alone_and_inside_a_batch_is_bitwise_identical(ctx, metric):
    problem, trials, _ = case("ragged", ctx)
    kind = rc.METRICS[metric]
    scorer = scorer_for(problem, kind, 0.999 if metric == "chi_squared_cdf" else 30.)
    batch = scorer.score_raw(trials)
    for t in (36, 4, 6):  # number 37 of 65; a trial of 16 groups; the 64-point group
        alone = scorer.score_raw([trials[t]])
        assert np.array_equal(alone["metric"][:, 0], batch["metric"][:, t], equal_nan=True)
        for key in ("inlier_groups", "inlier_points", "candidate_quadratic", "candidate_log_det", "status"):
            assert alone[key][0] == batch[key][t], key
    again = scorer.score_raw(trials)
    assert np.array_equal(again["metric"], batch["metric"], equal_nan=True)


def _raw(ctx, problem, offsets, indices, cand_offsets, cand_groups, n_trials, sentinel=-7.):
    n_groups = len(offsets) - 1
    fs = problem.model.get_covariance().features(problem.x)
    s = fs.as_struct()
    width = max(n_trials, 1)
    metric = np.full((max(n_groups, 1), width), sentinel, order="F")
    ig, ip = np.full(width, -7, dtype=np.int64), np.full(width, -7, dtype=np.int64)
    cq, cl, status = np.full(width, sentinel), np.full(width, sentinel), np.full(width, -7, dtype=np.int32)
    arrays = [np.ascontiguousarray(a, dtype=np.int64) for a in (offsets, indices, cand_offsets, cand_groups)]
    p = [a.ctypes.data_as(C.c_void_p) for a in arrays]
    st = ctx._lib.agp_ransac_score_trials(
        ctx._h, ctx.kernel(problem.model.get_covariance()), C.byref(s), problem.d.ctypes.data_as(C.c_void_p), None, n_groups, p[0], p[1],
        n_trials, p[2], p[3], capi.RANSAC_NLL_JOINT, 1., metric.ctypes.data_as(C.c_void_p), max(n_groups, 1), capi.HOST,
        ig.ctypes.data_as(C.c_void_p), ip.ctypes.data_as(C.c_void_p), cq.ctypes.data_as(C.c_void_p), cl.ctypes.data_as(C.c_void_p),
        status.ctypes.data_as(C.c_void_p))
    untouched = (np.all(metric == sentinel) and np.all(ig == -7) and np.all(ip == -7) and np.all(cq == sentinel) and np.all(cl == sentinel)
                 and np.all(status == -7))
    return st, untouched


def test_limits(ctx):
    """beyond a stated limit the call returns AGP_ERR_INVALID_ARGUMENT and writes nothing"""
    problem, _, _ = case("singletons", ctx)
    n = 301
    single_off, single_idx = np.arange(n + 1), np.arange(n)
    assert _raw(ctx, problem, single_off, single_idx, [0, 256], np.arange(256), 1) == (capi.AGP_OK, False)
    bad = [
        (single_off, single_idx, [0, 257], np.arange(257), 1),             # 257 candidate points
        (single_off, single_idx, [0, 2], [3, n], 1),                       # a candidate id out of range
        (single_off, single_idx, [0, 2], [3, -1], 1),
        (single_off, single_idx, [0, 3], [3, 8, 3], 1),                    # a duplicate candidate
        (single_off, single_idx, [0], [], 0),                              # n_trials = 0
        (single_off, single_idx, [0, 1, 1], [3], 2),                       # a trial without candidates
        ([0, 65, 100], np.arange(100), [0, 1], [1], 1),                    # a group of 65
        ([0, 64, 64, 100], np.arange(100), [0, 1], [2], 1),                # an empty group
        ([0, 3, 6], [0, 1, 2, 2, 3, 4], [0, 1], [0], 1),                   # a point in two groups
        ([0, 3, 6], [0, 1, 2, 3, 4, n], [0, 1], [0], 1),                   # an index out of range
    ]
    for args in bad:
        assert _raw(ctx, problem, *args) == (capi.AGP_ERR_INVALID_ARGUMENT, True), args[2:]
    # 16 groups of 17 points: 272 candidate points from fewer than 257 groups
    off17 = np.arange(0, 17 * 17 + 1, 17)
    assert _raw(ctx, problem, off17, np.arange(289), [0, 16], np.arange(16), 1) == (capi.AGP_ERR_INVALID_ARGUMENT, True)
    assert _raw(ctx, problem, off17, np.arange(289), [0, 15], np.arange(15), 1) == (capi.AGP_OK, False)  # 255 points


def test_a_trial_that_is_not_positive_definite(ctx):
    """two identical noiseless points under a noise-free covariance among the candidates: that trial alone reports the
    status, its metrics are NaN, the host loop counts it as an invalid candidate, the others are untouched"""
    x = np.array([0., 1.5, 3., 3., 4.5, 6., 7.5, 9., 10.5, 12., 13.5, 15.])
    y = np.sin(0.4 * x)
    model = ab.gp_from_covariance(ab.SquaredExponential(2., 1.), context=ctx)
    problem = rc.Problem(model, x, y, None, [[i] for i in range(len(x))])
    good = [[0, 5, 9], [1, 6, 11], [4, 7, 10], [0, 1, 8]]
    trials = good[:2] + [[2, 3, 8]] + good[2:]
    scorer = scorer_for(problem, rc.NLL_JOINT, 1.)
    out = scorer.score_raw(trials)
    assert list(out["status"]) == [capi.AGP_OK, capi.AGP_OK, capi.AGP_ERR_NOT_POSITIVE_DEFINITE, capi.AGP_OK, capi.AGP_OK]
    assert np.all(np.isnan(out["metric"][:, 2])) and math.isnan(out["candidate_quadratic"][2]) and math.isnan(out["candidate_log_det"][2])
    assert out["inlier_groups"][2] == 0 and out["inlier_points"][2] == 0
    without = scorer.score_raw(good)
    keep = [0, 1, 3, 4]
    assert np.array_equal(out["metric"][:, keep], without["metric"], equal_nan=True)
    for key in ("inlier_groups", "inlier_points", "candidate_quadratic", "candidate_log_det"):
        assert np.array_equal(out[key][keep], without[key])
    assert np.isfinite(without["candidate_quadratic"]).all()
    _, valid, _ = scorer.score(trials)
    assert valid == [True, True, False, True, True]


def _close(u, v):
    return (math.isnan(u) and math.isnan(v)) or abs(u - v) <= 1e-8 * max(1., abs(v))


def _same_run(a, b):
    """the same iterations (candidates, inlier and outlier sets, consensus metric to 1e-8) and the same best.  Two
    iterations with one consensus set (the same points drawn as candidates in one and found as inliers in the other) have
    the same consensus metric up to rounding, and which of them is `best` is decided by that rounding: where the
    reference run has such ties within 1e-8 of its best metric, best must be one of the tied iterations with the same
    consensus set; where it has none, best must be the same iteration."""
    assert a.return_code == b.return_code and len(a.iterations) == len(b.iterations)
    for ia, ib in zip(a.iterations, b.iterations):
        assert ia.candidates == ib.candidates
        assert list(ia.inliers) == list(ib.inliers) and list(ia.outliers) == list(ib.outliers)
        assert _close(ia.consensus_metric_value, ib.consensus_metric_value)
    assert _close(a.best.consensus_metric_value, b.best.consensus_metric_value)
    assert sorted(a.best.consensus()) == sorted(b.best.consensus())
    tied = [it.candidates for it in b.iterations if not math.isnan(it.consensus_metric_value)
            and _close(it.consensus_metric_value, b.best.consensus_metric_value)]
    assert a.best.candidates in tied or (not tied and a.best.candidates == b.best.candidates == [])
    if len(tied) == 1:
        assert a.best.candidates == b.best.candidates


def test_toy_model_end_to_end(ctx):
    """test_ransac_direct / test_ransac_model through model.ransac(...).fit(dataset)"""
    problem = rc.toy_problem(context=ctx)
    ds = problem.dataset()
    ransac_model = problem.model.ransac(ab.DefaultGPRansacStrategy(), 1., 3, 3, 20)
    assert ransac_model.get_name() == "ransac[" + problem.model.get_name() + "]"
    fm = ransac_model.fit(ds)
    fit = fm.get_fit()
    out = fit.ransac_output
    assert ab.ransac_success(out.return_code) and fit.has_fit_model()
    assert len(out.best.consensus()) == 8 and 3 in out.best.outliers and 5 in out.best.outliers
    assert math.isfinite(out.best.consensus_metric_value)
    host = ab.ransac(rc.NumpyScorer(problem), list(range(10)), ab.RansacConfig(1., 3, 3, 20, 0))
    _same_run(out, host)
    good = sorted(out.best.consensus())
    direct = problem.model.fit(ab.RegressionDataset(problem.x[good], problem.y[good]))
    xs = np.linspace(-1., 10., 23)
    consensus_order = problem.model.fit(ab.RegressionDataset(problem.x[out.best.consensus()], problem.y[out.best.consensus()]))
    assert np.array_equal(fm.predict(xs).mean(), consensus_order.predict(xs).mean())
    assert np.abs(fm.predict(xs).mean() - direct.predict(xs).mean()).max() <= 1e-7 * np.abs(direct.predict(xs).mean()).max()
    # a run that finds no consensus has no fit model
    none = problem.model.ransac(ab.DefaultGPRansacStrategy(), -math.inf, 1, 2, 5).fit(ds).get_fit()
    assert none.ransac_output.return_code == ab.RANSAC_RETURN_CODE_NO_CONSENSUS and not none.has_fit_model()


def test_chi_squared_strategy_agrees_with_the_numpy_scorer(ctx):
    """MakeRansacChiSquaredGaussianProcess: ChiSquaredCdf inliers, ChiSquaredConsensusMetric, ChiSquaredIsValidCandidateMetric,
    max_failed_candidates = 20, on the toy data as they are (that test case's dataset), with the two outliers, and under
    the better-conditioned prior"""
    for problem in (rc.toy_problem(context=ctx, outliers=False), rc.toy_problem(context=ctx), rc.ten_point_problem(context=ctx)):
        strategy = ab.gp_ransac_strategy(ab.ChiSquaredCdf(), ab.ChiSquaredConsensusMetric(), ab.ChiSquaredIsValidCandidateMetric(),
                                         ab.LeaveOneOutGrouper())
        config = ab.RansacConfig(0.999, 3, 3, 20, 20)
        device = problem.model.ransac(strategy, config, seed=5).fit(problem.dataset()).get_fit().ransac_output
        host = ab.ransac(rc.NumpyScorer(problem, rc.CHI_SQUARED_CDF, "chi_squared", ab.ChiSquaredIsValidCandidateMetric()),
                         list(range(10)), config, seed=5)
        _same_run(device, host)
        assert device.return_code in (ab.RANSAC_RETURN_CODE_SUCCESS, ab.RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES)


def test_unbatched_consensus_metrics(ctx):
    problem, trials, _ = case("ragged_var", ctx)
    positions = sorted(set(trials[2]) | {5, 9, 11})
    for kind, metric in (("chi_squared", ab.ChiSquaredConsensusMetric()), ("entropy", ab.DifferentialEntropyConsensusMetric()),
                         ("feature_count", ab.FeatureCountConsensusMetric())):
        scorer = scorer_for(problem, rc.NLL_JOINT, 1., consensus=metric)
        got, want = scorer.consensus_metric(positions), problem.consensus_value(kind, positions)
        assert abs(got - want) <= 1e-8 * max(1., abs(want)), (kind, got, want)
