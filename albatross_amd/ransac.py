"""GP RANSAC outlier rejection (models/ransac.hpp, models/ransac_gp.hpp, models/conditional_gaussian.hpp).

The reference fits and predicts once per trial.  Here the trials of a round are ONE call: the prior covariance of the
measurements is built once on the device and every trial costs one small factorisation plus a conditional prediction of
the other groups (agp_ransac_score_trials, include/albatross_amd.h).  The loop around the trials is the reference's
(ransac.hpp:172-257), rule for rule; it runs on the host over the scored matrix and needs no device, so any object with

    score(trials) -> (metric, valid, consensus_metric)

can drive it: `trials` is an int64 array (T, sample) of positions into `groups`; `metric` is (G, T) with NaN at a trial's
own candidates; `valid[t]` says whether trial t's candidates pass the candidate check; `consensus_metric(positions)`
scores one consensus set (lower is better).

The candidate sets come from agp_ransac_draw_candidates, the project's own seeded draw (sorted group positions, without
replacement).  It does not reproduce libstdc++'s default_random_engine, so for one seed the trials are not the
reference's trials; the rules applied to them are.

Not provided: GenericRansacStrategy (refits of arbitrary models), serialisation, RANSAC on the sparse GP or across
ranks.
"""
import ctypes as C
import math

import numpy as np

from . import _capi as capi
from .covariance import as_measurements, has_linear_combinations
from .gp import (JointDistribution, LeaveOneOutGrouper, MarginalDistribution, RegressionDataset, _group_arrays, _ptr, _values_of,
                 group_indexer)
from .scores import chi_squared_cdf, chi_squared_cdf_scalar

RANSAC_RETURN_CODE_INVALID = -1
RANSAC_RETURN_CODE_SUCCESS = 0
RANSAC_RETURN_CODE_NO_CONSENSUS = 1
RANSAC_RETURN_CODE_INVALID_ARGUMENTS = 2
RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES = 3
RANSAC_RETURN_CODE_FAILURE = 4

_CODE_NAMES = {
    RANSAC_RETURN_CODE_INVALID: "invalid",
    RANSAC_RETURN_CODE_SUCCESS: "success",
    RANSAC_RETURN_CODE_NO_CONSENSUS: "no_consensus",
    RANSAC_RETURN_CODE_INVALID_ARGUMENTS: "invalid_arguments",
    RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES: "exceeded_max_failed_candidates",
    RANSAC_RETURN_CODE_FAILURE: "failure",
}


def ransac_return_code_to_string(return_code):
    return _CODE_NAMES[return_code]


def ransac_success(return_code):
    return return_code == RANSAC_RETURN_CODE_SUCCESS


class RansacConfig:
    """ransac.hpp:133-152"""

    def __init__(self, inlier_threshold=math.nan, random_sample_size=0, min_consensus_size=0, max_iterations=0,
                 max_failed_candidates=0):
        self.inlier_threshold = float(inlier_threshold)
        self.random_sample_size = int(random_sample_size)
        self.min_consensus_size = int(min_consensus_size)
        self.max_iterations = int(max_iterations)
        self.max_failed_candidates = int(max_failed_candidates)


def _same_metric(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


class RansacIteration:
    """ransac.hpp:92-116: candidates (group keys), inliers / outliers ({key: metric}), consensus_metric_value (NaN until
    the consensus is large enough to be scored)"""

    def __init__(self):
        self.candidates = []
        self.inliers = {}
        self.outliers = {}
        self.consensus_metric_value = math.nan

    def consensus(self):
        return list(self.candidates) + list(self.inliers.keys())

    def __eq__(self, other):
        return (self.candidates == other.candidates and self.inliers == other.inliers and self.outliers == other.outliers
                and _same_metric(self.consensus_metric_value, other.consensus_metric_value))


class RansacOutput:
    """ransac.hpp:118-131"""

    def __init__(self):
        self.return_code = RANSAC_RETURN_CODE_INVALID
        self.best = RansacIteration()
        self.iterations = []

    def __eq__(self, other):
        return self.return_code == other.return_code and self.best == other.best and self.iterations == other.iterations


_GOLDEN = 0x9E3779B97F4A7C15
_MASK64 = (1 << 64) - 1


def draw_candidates(seed, n_groups, sample_size, n_trials):
    """(n_trials, sample_size) int64: per trial `sample_size` distinct group positions in ascending order
    (agp_ransac_draw_candidates: splitmix64 + Floyd's sampling; the same sets in every binding)"""
    out = np.zeros((int(n_trials), int(sample_size)), dtype=np.int64)
    st = capi.load().agp_ransac_draw_candidates(int(seed) & _MASK64, int(n_groups), int(sample_size), int(n_trials), _ptr(out))
    if st != capi.AGP_OK:
        raise ValueError("draw_candidates: sample_size must lie in 0 .. n_groups")
    return out


def ransac(scorer, groups, config, seed=0):
    """ransac(ransac_functions, groups, config), ransac.hpp:172-257.  A round draws as many trials as iterations remain,
    scores them in one call and walks them in order; trials whose candidates are invalid use up no iteration, so a further
    round is drawn for what they left over (round r draws with seed + r * 0x9E3779B97F4A7C15)."""
    groups = list(groups)
    n_groups = len(groups)
    output = RansacOutput()
    output.return_code = RANSAC_RETURN_CODE_FAILURE
    if (config.min_consensus_size >= n_groups or config.min_consensus_size < config.random_sample_size
            or config.random_sample_size >= n_groups or config.random_sample_size <= 0 or config.max_iterations <= 0):
        output.return_code = RANSAC_RETURN_CODE_INVALID_ARGUMENTS
        return output
    i = 0
    failed_candidates = 0
    round_ = 0
    while i < config.max_iterations:
        trials = draw_candidates((int(seed) + round_ * _GOLDEN) & _MASK64, n_groups, config.random_sample_size,
                                 config.max_iterations - i)
        round_ += 1
        metric, valid, consensus_metric = scorer.score(trials)
        for t in range(trials.shape[0]):
            iteration = RansacIteration()
            output.iterations.append(iteration)
            positions = [int(p) for p in trials[t]]
            iteration.candidates = [groups[p] for p in positions]
            if not valid[t]:
                failed_candidates += 1
                if failed_candidates >= config.max_failed_candidates:
                    output.return_code = RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES
                    return output
                continue
            chosen = set(positions)
            inlier_positions = []
            for g in range(n_groups):
                if g in chosen:
                    continue
                value = float(metric[g, t])
                if value <= config.inlier_threshold:  # NaN: an outlier
                    iteration.inliers[groups[g]] = value
                    inlier_positions.append(g)
                else:
                    iteration.outliers[groups[g]] = value
            if len(positions) + len(inlier_positions) >= config.min_consensus_size:
                iteration.consensus_metric_value = float(consensus_metric(positions + inlier_positions))
                best = output.best.consensus_metric_value
                if math.isnan(best) or iteration.consensus_metric_value < best:
                    output.best = iteration
            i += 1
    output.return_code = RANSAC_RETURN_CODE_SUCCESS if output.best.consensus() else RANSAC_RETURN_CODE_NO_CONSENSUS
    return output


# ---- the parts of a GP strategy (ransac_gp.hpp:69-113, evaluation/prediction_metrics.hpp:112-145) -------------------
class NegativeLogLikelihood:
    """NegativeLogLikelihood<PredictType>: predict_type "joint" or "marginal" """

    def __init__(self, predict_type="joint"):
        if predict_type not in ("joint", "marginal"):
            raise ValueError(f"predict_type: 'joint' or 'marginal', not {predict_type!r}")
        self.predict_type = predict_type

    def _code(self):
        return capi.RANSAC_NLL_JOINT if self.predict_type == "joint" else capi.RANSAC_NLL_MARGINAL


class ChiSquaredCdf:
    def _code(self):
        return capi.RANSAC_CHI_SQUARED_CDF


class FeatureCountConsensusMetric:
    """minus the number of observations in the consensus"""


class ChiSquaredConsensusMetric:
    """chi_squared_cdf(d_S^T (Sigma_SS + R_S)^-1 d_S, |S|) over the consensus points S"""


class DifferentialEntropyConsensusMetric:
    """the differential entropy of the prior of the consensus, exactly as differential_entropy.hpp:37-42 writes it:
    1/2 k (1 + log 2 pi + log|Sigma_SS|)"""


class AlwaysAcceptCandidateMetric:
    def __call__(self, quadratic, dof):
        return True


class ChiSquaredIsValidCandidateMetric:
    """chi_squared_cdf(q_c, s) <= threshold on the candidates' own prior"""

    def __init__(self, chi_squared_threshold=0.999):
        self.chi_squared_threshold = chi_squared_threshold

    def __call__(self, quadratic, dof):
        return chi_squared_cdf_scalar(quadratic, dof) <= self.chi_squared_threshold


def differential_entropy_from_log_det(k, log_det):
    return 0.5 * k * (1. + math.log(2. * math.pi) + log_det)


class GaussianProcessRansacStrategy:
    """GaussianProcessRansacStrategy<InlierMetric, ConsensusMetric, IsValidCandidateMetric, GrouperFunction>
    (ransac_gp.hpp:147-180)"""

    def __init__(self, inlier_metric, consensus_metric, is_valid_candidate, grouper):
        if not isinstance(inlier_metric, (NegativeLogLikelihood, ChiSquaredCdf)):
            raise TypeError("inlier_metric: NegativeLogLikelihood or ChiSquaredCdf")
        if not isinstance(consensus_metric, (FeatureCountConsensusMetric, ChiSquaredConsensusMetric,
                                             DifferentialEntropyConsensusMetric)):
            raise TypeError("consensus_metric: FeatureCount-, ChiSquared- or DifferentialEntropyConsensusMetric")
        self.inlier_metric_ = inlier_metric
        self.consensus_metric_ = consensus_metric
        self.is_valid_candidate_ = is_valid_candidate
        self.grouper_ = grouper

    def get_indexer(self, dataset):
        return self.grouper_ if isinstance(self.grouper_, dict) else group_indexer(dataset.features, self.grouper_)

    def __call__(self, model, dataset, inlier_threshold):
        return GPRansacScorer(model, dataset, self, inlier_threshold)


class DefaultGPRansacStrategy(GaussianProcessRansacStrategy):
    def __init__(self):
        super().__init__(NegativeLogLikelihood("joint"), FeatureCountConsensusMetric(), AlwaysAcceptCandidateMetric(),
                         LeaveOneOutGrouper())


def gp_ransac_strategy(inlier_metric, consensus_metric, is_valid_candidate_or_grouper, grouper=None):
    """gp_ransac_strategy(inlier, consensus, grouper) / (inlier, consensus, is_valid_candidate, grouper)"""
    if grouper is None:
        return GaussianProcessRansacStrategy(inlier_metric, consensus_metric, AlwaysAcceptCandidateMetric(),
                                             is_valid_candidate_or_grouper)
    return GaussianProcessRansacStrategy(inlier_metric, consensus_metric, is_valid_candidate_or_grouper, grouper)


class GPRansacScorer:
    """The device scorer of a GP strategy: score(trials) is one agp_ransac_score_trials call.  The FeatureCount consensus
    metric needs the group sizes only; the ChiSquared and DifferentialEntropy ones are computed per qualifying trial from
    the gathered consensus block through the dense factor (agp_factor_create / agp_solve) - they are not batched."""

    def __init__(self, model, dataset, strategy, inlier_threshold):
        if model.precision != "fp64":
            raise ValueError(f"ransac: fp64 models only, not {model.precision!r}")
        if has_linear_combinations(dataset.features):
            raise NotImplementedError("ransac: LinearCombination features are not supported")
        self.model_, self.dataset_, self.strategy_ = model, dataset, strategy
        self.threshold_ = float(inlier_threshold)
        self.ctx_ = model._ctx()
        cov = model.covariance_function_
        self.fs_ = cov.features(_values_of(dataset.features))
        self.deviation_, self.y_var_ = model._targets(self.fs_, dataset.targets)
        self.indexer_ = strategy.get_indexer(dataset)
        self.offsets_, self.indices_ = _group_arrays(dataset, self.indexer_, self.fs_.n)
        self.n_groups_ = len(self.offsets_) - 1
        self.last_ = None  # the raw outputs of the last score call, for inspection

    def score_raw(self, trials, want_metric=True):
        """agp_ransac_score_trials for trials given as a list of position lists (they may differ in length)"""
        ctx = self.ctx_
        lists = [np.asarray(t, dtype=np.int64).reshape(-1) for t in trials]
        n_trials = len(lists)
        cand_offsets = np.zeros(n_trials + 1, dtype=np.int64)
        if n_trials:
            cand_offsets[1:] = np.cumsum([len(t) for t in lists])
        cand_groups = np.ascontiguousarray(np.concatenate(lists) if n_trials else np.zeros(0, dtype=np.int64))
        metric = np.full((self.n_groups_, n_trials), np.nan, order="F") if want_metric else None
        out = {"metric": metric,
               "inlier_groups": np.zeros(n_trials, dtype=np.int64), "inlier_points": np.zeros(n_trials, dtype=np.int64),
               "candidate_quadratic": np.zeros(n_trials), "candidate_log_det": np.zeros(n_trials),
               "status": np.zeros(n_trials, dtype=np.int32)}
        s = self.fs_.as_struct()
        st = ctx._lib.agp_ransac_score_trials(
            ctx._h, ctx.kernel(self.model_.covariance_function_), C.byref(s), _ptr(self.deviation_), _ptr(self.y_var_),
            self.n_groups_, _ptr(self.offsets_), _ptr(self.indices_), n_trials, _ptr(cand_offsets), _ptr(cand_groups),
            self.strategy_.inlier_metric_._code(), self.threshold_, _ptr(metric), max(self.n_groups_, 1), capi.HOST,
            _ptr(out["inlier_groups"]), _ptr(out["inlier_points"]), _ptr(out["candidate_quadratic"]),
            _ptr(out["candidate_log_det"]), _ptr(out["status"]))
        ctx._check(st, "agp_ransac_score_trials")
        out["candidate_points"] = np.array([int(sum(self.offsets_[g + 1] - self.offsets_[g] for g in t)) for t in lists],
                                           dtype=np.int64)
        self.last_ = out
        return out

    def score(self, trials):
        out = self.score_raw(list(trials))
        check = self.strategy_.is_valid_candidate_
        valid = [bool(out["status"][t] == capi.AGP_OK and check(float(out["candidate_quadratic"][t]), int(out["candidate_points"][t])))
                 for t in range(len(out["status"]))]
        return out["metric"], valid, self.consensus_metric

    def _points(self, positions):
        return np.concatenate([self.indices_[self.offsets_[g]:self.offsets_[g + 1]] for g in positions])

    def consensus_metric(self, positions):
        metric = self.strategy_.consensus_metric_
        pts = self._points(positions)
        if isinstance(metric, FeatureCountConsensusMetric):
            return -float(len(pts))
        feats = _values_of(self.dataset_.features)
        sub = [feats[int(i)] for i in pts] if isinstance(feats, list) else np.asarray(feats)[pts]
        sigma = np.array(self.ctx_.gram(self.model_.covariance_function_, as_measurements(sub)), dtype=np.float64, order="F")
        if isinstance(metric, ChiSquaredConsensusMetric):
            truth = MarginalDistribution(np.zeros(len(pts)), None if self.y_var_ is None else self.y_var_[pts])
            return chi_squared_cdf(JointDistribution(self.deviation_[pts], sigma), truth)
        from .gp import DenseFactor
        return differential_entropy_from_log_det(len(pts), DenseFactor(sigma, context=self.ctx_).log_determinant)


# ---- the model wrapper (ransac.hpp:380-505) --------------------------------------------------------------------------
class RansacFit:
    """Fit<RansacFit<...>>: ransac_output and, when RANSAC succeeded, the sub-model's fit on the consensus set"""

    def __init__(self, ransac_output, fit_model=None):
        self.ransac_output = ransac_output
        self.maybe_empty_fit_model = fit_model

    def has_fit_model(self):
        return self.maybe_empty_fit_model is not None

    def get_fit_model_or_assert(self):
        assert self.has_fit_model(), "RANSAC did not succeed: there is no fit model"
        return self.maybe_empty_fit_model


class RansacFitModel:
    def __init__(self, model, fit):
        self._model, self._fit = model, fit

    def get_fit(self):
        return self._fit

    def get_model(self):
        return self._model

    def predict(self, features):
        return self._fit.get_fit_model_or_assert().predict(features)


def indices_from_groups(indexer, keys):
    out = []
    for k in keys:
        out.extend(int(i) for i in indexer[k])
    return out


def subset_dataset(dataset, indices):
    feats = dataset.features
    idx = np.asarray(indices, dtype=np.int64)
    sub = [feats[int(i)] for i in idx] if isinstance(feats, list) else np.asarray(feats)[idx]
    cov = dataset.targets.covariance
    return RegressionDataset(sub, MarginalDistribution(dataset.targets.mean[idx], None if cov is None else cov[idx]))


class Ransac:
    """Ransac<ModelType, StrategyType> (ransac.hpp:427-505): wraps a model and performs RANSAC each time fit is called"""

    def __init__(self, sub_model, strategy, config, seed=0):
        self.sub_model_, self.strategy_, self.config_, self.seed_ = sub_model, strategy, config, seed

    def get_name(self):
        return "ransac[" + self.sub_model_.get_name() + "]"

    def get_params(self):
        return self.sub_model_.get_params()

    def set_param(self, name, value):
        self.sub_model_.set_param(name, value)

    def set_param_values(self, values):
        self.sub_model_.set_param_values(values)

    def fit(self, dataset, targets=None):
        if targets is not None:
            dataset = RegressionDataset(dataset, targets)
        indexer = self.strategy_.get_indexer(dataset)
        scorer = self.strategy_(self.sub_model_, dataset, self.config_.inlier_threshold)
        output = ransac(scorer, list(indexer.keys()), self.config_, seed=self.seed_)
        if not ransac_success(output.return_code):
            return RansacFitModel(self, RansacFit(output))
        good = indices_from_groups(indexer, output.best.consensus())
        return RansacFitModel(self, RansacFit(output, self.sub_model_.fit(subset_dataset(dataset, good))))


def _model_ransac(self, strategy, inlier_threshold_or_config, random_sample_size=None, min_consensus_size=None,
                  max_iterations=None, max_failed_candidates=0, seed=0):
    """model.ransac(strategy, inlier_threshold, random_sample_size, min_consensus_size, max_iterations
    [, max_failed_candidates]) or model.ransac(strategy, config) (core/model.hpp; ransac.hpp:507-524)"""
    if isinstance(inlier_threshold_or_config, RansacConfig):
        return Ransac(self, strategy, inlier_threshold_or_config, seed=seed)
    return Ransac(self, strategy, RansacConfig(inlier_threshold_or_config, random_sample_size, min_consensus_size,
                                               max_iterations, max_failed_candidates), seed=seed)
