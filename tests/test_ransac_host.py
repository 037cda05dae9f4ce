"""The RANSAC host loop (albatross_amd/ransac.py: ransac.hpp:172-257) on the numpy restatement of the GP scorer
(tests/ransac_cases.py) and on fixed tables: no device."""
import itertools
import math

import numpy as np

import albatross_amd as ab
import ransac_cases as rc


def toy_config(**over):
    cfg = dict(inlier_threshold=1., random_sample_size=3, min_consensus_size=3, max_iterations=20, max_failed_candidates=0)
    cfg.update(over)
    return ab.RansacConfig(**cfg)


def test_toy_ransac_direct():
    """test_ransac_direct: observations 3 and 5 are outliers; LOO groups, threshold 1, sample 3, 20 iterations"""
    p = rc.toy_problem()
    out = ab.ransac(rc.NumpyScorer(p), list(range(10)), toy_config())
    assert ab.ransac_success(out.return_code) and out.return_code == ab.RANSAC_RETURN_CODE_SUCCESS
    assert len(out.best.consensus()) == 8
    assert 3 in out.best.outliers and 5 in out.best.outliers
    assert math.isfinite(out.best.consensus_metric_value) and out.best.consensus_metric_value == -8.
    assert len(out.iterations) == 20


def test_toy_every_clean_triple_finds_the_outliers():
    """all 120 candidate triples: a triple free of 3 and 5 yields consensus 8 with outliers {3, 5}, and no metric of any
    triple lies closer to the threshold 1 than 0.016 relative to the metric itself, so the toy case does not hinge on
    rounding.  (The nearest one is 0.98400797: 0.01625 of itself, 0.01599 of the threshold.)  The two numpy routes are
    compared on the clean triples only: a triple that holds a +-400 observation under this prior (condition number
    above 1e6) is scored with a relative error near 5e-8 by either route."""
    p = rc.toy_problem()
    triples = [list(t) for t in itertools.combinations(range(10), 3)]
    assert len(triples) == 120
    metric = p.score(triples, rc.NLL_JOINT)[0]
    clean = [t for t in triples if 3 not in t and 5 not in t]
    assert len(clean) == 56
    rc.assert_routes_agree(p, clean, (rc.NLL_JOINT,))
    for t, triple in enumerate(triples):
        if 3 in triple or 5 in triple:
            continue
        col = metric[:, t]
        outliers = {g for g in range(10) if g not in triple and not col[g] <= 1.}
        assert outliers == {3, 5}, (triple, col)
        assert 3 + sum(1 for g in range(10) if g not in triple and col[g] <= 1.) == 8
    values = metric[~np.isnan(metric)]
    gap = np.min(np.abs(values - 1.) / np.abs(values))
    print("nearest metric to the threshold, relative:", gap)
    assert gap >= 0.016, gap


def test_edge_cases():
    """test_ransac_edge_cases, on its get_reasonable_ransac_config: threshold 1, sample 1, min consensus 2, 20 iterations"""
    p = rc.toy_problem()
    groups = list(range(10))

    def reasonable(**over):
        return toy_config(**dict(dict(random_sample_size=1, min_consensus_size=2), **over))

    out = ab.ransac(rc.NumpyScorer(p), groups, reasonable(inlier_threshold=-math.inf))
    assert out.return_code == ab.RANSAC_RETURN_CODE_NO_CONSENSUS and not ab.ransac_success(out.return_code)
    assert out.best.consensus() == [] and len(out.iterations) == 20
    assert all(math.isnan(it.consensus_metric_value) and len(it.outliers) == 9 for it in out.iterations)
    for over in (dict(min_consensus_size=10), dict(random_sample_size=10), dict(max_iterations=0),
                 dict(random_sample_size=0), dict(random_sample_size=3)):
        scorer = rc.NumpyScorer(p)
        out = ab.ransac(scorer, groups, reasonable(**over))
        assert out.return_code == ab.RANSAC_RETURN_CODE_INVALID_ARGUMENTS, over
        assert scorer.calls == 0 and out.iterations == []
    never = rc.NumpyScorer(p, is_valid=lambda quadratic, dof: False)
    out = ab.ransac(never, groups, reasonable(max_failed_candidates=3))
    assert out.return_code == ab.RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES
    assert len(out.iterations) == 3 and all(not it.inliers and not it.outliers for it in out.iterations)
    assert ab.ransac_return_code_to_string(out.return_code) == "exceeded_max_failed_candidates"


def test_max_failed_candidates_zero_ends_at_the_first_invalid_candidate():
    """failed_candidates >= max_failed_candidates is tested AFTER the increment: with 0 the first invalid candidate ends
    the run; an invalid candidate uses up no iteration"""
    calls = []

    def valid(candidates):
        calls.append(candidates)
        return len(calls) != 3  # the third trial is invalid

    scorer = rc.TableScorer(10, lambda g, c: 0., valid)
    out = ab.ransac(scorer, list(range(10)), toy_config(max_failed_candidates=0))
    assert out.return_code == ab.RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES
    assert len(out.iterations) == 3 and out.iterations[2].inliers == {}
    # with room for failures the run goes on and still makes max_iterations valid iterations
    calls.clear()
    scorer = rc.TableScorer(10, lambda g, c: 0., valid)
    out = ab.ransac(scorer, list(range(10)), toy_config(max_failed_candidates=5, max_iterations=6))
    assert out.return_code == ab.RANSAC_RETURN_CODE_SUCCESS
    assert len(out.iterations) == 7 and sum(1 for it in out.iterations if it.inliers) == 6
    assert len(scorer.trials) == 6 + 1  # a second round of ONE trial for the iteration the invalid candidate left over


def test_best_is_kept_on_ties_and_replaced_on_nan():
    scorer = rc.TableScorer(10, lambda g, c: 0.)  # every trial: all inliers, consensus metric -10
    out = ab.ransac(scorer, list(range(10)), toy_config())
    assert out.best is out.iterations[0]
    assert all(it.consensus_metric_value == -10. for it in out.iterations)
    # a trial below min_consensus_size keeps a NaN consensus metric and never becomes best
    first = []

    def metric(g, candidates):
        if not first:
            first.append(list(candidates))
        return 2. if candidates == first[0] else 0.

    out = ab.ransac(rc.TableScorer(10, metric), list(range(10)), toy_config(min_consensus_size=4))
    assert math.isnan(out.iterations[0].consensus_metric_value) and len(out.iterations[0].outliers) == 7
    later = [it for it in out.iterations if it.candidates != first[0]]
    assert out.best is later[0] and out.best.consensus_metric_value == -10.
    # strictly smaller replaces
    sizes = iter([5, 5, 7, 7, 6])

    def consensus(positions):
        return -float(next(sizes))

    out = ab.ransac(rc.TableScorer(10, lambda g, c: 0., consensus=consensus), list(range(10)), toy_config(max_iterations=5))
    assert out.best is out.iterations[2]


def test_group_keys_and_outputs_compare():
    p = rc.toy_problem()
    keys = [f"k{i}" for i in range(10)]
    a = ab.ransac(rc.NumpyScorer(p), keys, toy_config(), seed=3)
    b = ab.ransac(rc.NumpyScorer(p), keys, toy_config(), seed=3)
    assert a == b and a.best == b.best
    assert set(a.best.outliers) == {"k3", "k5"} and len(a.best.consensus()) == 8
    c = ab.ransac(rc.NumpyScorer(p), keys, toy_config(), seed=4)
    assert [it.candidates for it in a.iterations] != [it.candidates for it in c.iterations]


def test_draw_candidates():
    a = ab.draw_candidates(11, 50, 8, 200)
    assert a.shape == (200, 8) and a.dtype == np.int64
    assert a.min() >= 0 and a.max() < 50
    assert np.all(np.diff(a, axis=1) > 0)  # sorted and distinct
    assert np.array_equal(a, ab.draw_candidates(11, 50, 8, 200))
    assert not np.array_equal(a, ab.draw_candidates(12, 50, 8, 200))
    assert np.array_equal(a[:7], ab.draw_candidates(11, 50, 8, 7))  # a trial's draw does not depend on n_trials
    assert len({tuple(r) for r in a}) > 150
    counts = np.bincount(ab.draw_candidates(5, 10, 3, 3000).ravel(), minlength=10)
    assert counts.min() > 750 and counts.max() < 1050  # 900 expected per group
    full = ab.draw_candidates(0, 6, 6, 2)
    assert np.array_equal(full, np.tile(np.arange(6), (2, 1)))
    assert ab.draw_candidates(0, 6, 0, 3).shape == (3, 0)
    try:
        ab.draw_candidates(0, 6, 7, 1)
    except ValueError:
        pass
    else:
        raise AssertionError("sample_size > n_groups must be refused")


def test_strategy_parts_and_model_wrapper_surface():
    s = ab.DefaultGPRansacStrategy()
    assert isinstance(s.inlier_metric_, ab.NegativeLogLikelihood) and s.inlier_metric_.predict_type == "joint"
    assert isinstance(s.consensus_metric_, ab.FeatureCountConsensusMetric)
    assert isinstance(s.is_valid_candidate_, ab.AlwaysAcceptCandidateMetric)
    assert isinstance(s.grouper_, ab.LeaveOneOutGrouper)
    t = ab.gp_ransac_strategy(ab.ChiSquaredCdf(), ab.ChiSquaredConsensusMetric(), ab.ChiSquaredIsValidCandidateMetric(),
                              ab.LeaveOneOutGrouper())
    assert t.is_valid_candidate_.chi_squared_threshold == 0.999
    assert t.is_valid_candidate_(3., 3) and not t.is_valid_candidate_(60., 3)
    u = ab.gp_ransac_strategy(ab.NegativeLogLikelihood("marginal"), ab.DifferentialEntropyConsensusMetric(), ab.LeaveOneOutGrouper())
    assert isinstance(u.is_valid_candidate_, ab.AlwaysAcceptCandidateMetric)
    model = ab.gp_from_covariance(ab.SquaredExponential(1., 1.), model_name="inner")
    r = model.ransac(s, 1., 3, 3, 20)
    assert r.get_name() == "ransac[inner]" and r.config_.max_failed_candidates == 0
    assert r.get_params() == model.get_params()
    name = next(iter(model.get_params()))
    r.set_param(name, 2.5)
    assert float(np.ravel(model.get_params()[name])[0]) == 2.5 or model.get_params()[name] == 2.5
    r2 = model.ransac(s, ab.RansacConfig(1., 3, 3, 20, 7))
    assert r2.config_.max_failed_candidates == 7 and isinstance(r2, ab.Ransac)
    fit = ab.RansacFit(ab.RansacOutput())
    assert not fit.has_fit_model() and fit.ransac_output.return_code == ab.RANSAC_RETURN_CODE_INVALID
