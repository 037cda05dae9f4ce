"""The arithmetic of GP RANSAC restated in numpy, and the cases the RANSAC tests share.

Written from the formulas of conditional_gaussian.hpp:30-91, prediction_metrics.hpp:112-141, stats/chi_squared.hpp:29-81
and ransac_gp.hpp:69-113 as include/albatross_amd.h states them for agp_ransac_score_trials:

    Sigma = k(as_measurements(x), as_measurements(x)),  d = y - mean(x),  R = diag(y_var)
    trial with candidate points c:   A = Sigma_cc + R_c,  v = A^-1 d_c,  q_c = d_c^T v,  log|A|
    group g outside the candidates:  r = Sigma_gc v - d_g,  P = Sigma_gg - Sigma_gc A^-1 Sigma_cg + R_g
    NLL joint 1/2 (log|P| + r^T P^-1 r + |g| log 2 pi);  marginal: P -> diag(P);  chi-squared cdf of r^T P^-1 r, |g| dof

Two routes: "cholesky" (numpy.linalg.cholesky and triangular substitutions, the order of the device code) and "solve"
(numpy.linalg.solve / slogdet on the unfactored blocks).  The case builders assert that the two agree within a tenth of
the bound the device is held to, so the inputs are conditioned well enough for that bound to mean something.  The prior
covariance comes from the oracle's C restatement of the covariance functions (oracle/oracle_py.py), the chi-squared cdf
from scipy's regularised incomplete gamma function."""
import json
import math
import os

import numpy as np
import scipy.special

import albatross_amd as ab
from oracle import oracle_py as orc

NLL_JOINT, NLL_MARGINAL, CHI_SQUARED_CDF = 0, 1, 2
METRICS = {"nll_joint": NLL_JOINT, "nll_marginal": NLL_MARGINAL, "chi_squared_cdf": CHI_SQUARED_CDF}
METRIC_BOUND = 1e-8  # |m - m_ref| <= METRIC_BOUND * max(1, |m_ref|): the bar predictions are held to against the oracle
LOG_2PI = math.log(2. * math.pi)


def chi_squared_cdf(x, dof):
    if math.isnan(x) or x < 0.:
        return math.nan
    if dof == 0:
        return 1.
    if np.finfo(np.float64).eps > x:
        return 0.
    if math.isinf(x):
        return 1.
    return float(scipy.special.gammainc(0.5 * dof, 0.5 * x))


def inlier_metric_values(r, P):
    """the three inlier metrics of one group, in the order NLL_JOINT, NLL_MARGINAL, CHI_SQUARED_CDF"""
    m = len(r)
    v = np.diag(P)
    marginal = 0.5 * float(np.sum(np.log(v) + r * r / v) + m * LOG_2PI)
    quad = float(r @ np.linalg.solve(P, r))
    sign, log_det = np.linalg.slogdet(P)
    joint = 0.5 * (float(log_det) + quad + m * LOG_2PI) if sign > 0 else math.nan
    return joint, marginal, chi_squared_cdf(quad, m)


class Problem:
    """Sigma, d, y_var and the grouping (a list of index arrays) of one dataset"""

    def __init__(self, model, x, y, y_var, groups):
        self.model, self.x, self.y, self.y_var = model, x, y, y_var
        self.groups = [np.asarray(g, dtype=np.int64) for g in groups]
        cov = model.get_covariance()
        self.sigma = np.array(orc.gram(cov, x, x_meas=True))
        coords = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
        self.d = np.asarray(y, dtype=np.float64) - model.get_mean()(coords)
        self.r = np.zeros(len(y)) if y_var is None else np.asarray(y_var, dtype=np.float64)

    def dataset(self):
        return ab.RegressionDataset(self.x, ab.MarginalDistribution(self.y, self.y_var))

    def indexer(self):
        return {k: [int(i) for i in g] for k, g in enumerate(self.groups)}

    def points(self, positions):
        return np.concatenate([self.groups[int(p)] for p in positions])

    def score_trial(self, positions, route="cholesky"):
        """(the three metrics per group, 3 x G with NaN at the candidates, q_c, log|A|); a LinAlgError when A is not
        positive definite"""
        c = self.points(positions)
        A = self.sigma[np.ix_(c, c)] + np.diag(self.r[c])
        dc = self.d[c]
        if route == "cholesky":
            L = np.linalg.cholesky(A)
            z = np.linalg.solve(L, dc)
            v = np.linalg.solve(L.T, z)
            log_det = 2. * float(np.sum(np.log(np.diag(L))))
        else:
            L = None
            v = np.linalg.solve(A, dc)
            log_det = float(np.linalg.slogdet(A)[1])
        quad = float(dc @ v)
        out = np.full((3, len(self.groups)), np.nan)
        chosen = {int(p) for p in positions}
        for gi, g in enumerate(self.groups):
            if gi in chosen:
                continue
            cross = self.sigma[np.ix_(c, g)]
            r = cross.T @ v - self.d[g]
            if route == "cholesky":
                W = np.linalg.solve(L, cross)
                P = self.sigma[np.ix_(g, g)] - W.T @ W + np.diag(self.r[g])
            else:
                P = self.sigma[np.ix_(g, g)] - cross.T @ np.linalg.solve(A, cross) + np.diag(self.r[g])
            out[:, gi] = inlier_metric_values(r, P)
        return out, quad, log_det

    def score_all(self, trials, route="cholesky"):
        """(metrics 3 x G x T, q_c, log|A|, failed) over a list of position lists"""
        G, T = len(self.groups), len(trials)
        metric = np.full((3, G, T), np.nan)
        quad, log_det, failed = np.full(T, np.nan), np.full(T, np.nan), np.zeros(T, dtype=bool)
        for t, positions in enumerate(trials):
            try:
                metric[:, :, t], quad[t], log_det[t] = self.score_trial(positions, route)
            except np.linalg.LinAlgError:
                failed[t] = True
        return metric, quad, log_det, failed

    def score(self, trials, kind, route="cholesky"):
        metric, quad, log_det, failed = self.score_all(trials, route)
        return metric[kind], quad, log_det, failed

    def consensus_value(self, kind, positions):
        pts = self.points(positions)
        if kind == "feature_count":
            return -float(len(pts))
        S = self.sigma[np.ix_(pts, pts)]
        if kind == "chi_squared":
            dS = self.d[pts]
            return chi_squared_cdf(float(dS @ np.linalg.solve(S + np.diag(self.r[pts]), dS)), len(pts))
        return 0.5 * len(pts) * (1. + LOG_2PI + float(np.linalg.slogdet(S)[1]))  # differential_entropy.hpp:37-42


def assert_routes_agree(problem, trials, kinds=(NLL_JOINT, NLL_MARGINAL, CHI_SQUARED_CDF)):
    """the Cholesky route and the solve route within a tenth of the device's bound; returns the Cholesky route's
    score_all"""
    ref = problem.score_all(trials, "cholesky")
    a, b = ref[0], problem.score_all(trials, "solve")[0]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    for kind in kinds:
        ok = ~np.isnan(a[kind])
        err = np.abs(a[kind][ok] - b[kind][ok]) / np.maximum(1., np.abs(b[kind][ok]))
        assert err.max() <= 0.1 * METRIC_BOUND, (kind, err.max())
    return ref


class NumpyScorer:
    """the `scorer` of ab.ransac on the numpy restatement"""

    def __init__(self, problem, kind=NLL_JOINT, consensus="feature_count", is_valid=None):
        self.problem, self.kind, self.consensus, self.is_valid = problem, kind, consensus, is_valid
        self.calls = 0

    def score(self, trials):
        self.calls += 1
        trials = [list(int(p) for p in t) for t in trials]
        metric, quad, _, failed = self.problem.score(trials, self.kind)
        valid = []
        for t, positions in enumerate(trials):
            ok = not failed[t]
            if ok and self.is_valid is not None:
                ok = bool(self.is_valid(float(quad[t]), len(self.problem.points(positions))))
            valid.append(ok)
        return metric, valid, lambda positions: self.problem.consensus_value(self.consensus, positions)


class TableScorer:
    """a scorer over fixed tables, for the rules of the loop: metric(g, candidates) and valid(candidates) are callables"""

    def __init__(self, n_groups, metric, valid=lambda candidates: True, consensus=lambda positions: -float(len(positions))):
        self.n_groups, self.metric, self.valid, self.consensus = n_groups, metric, valid, consensus
        self.trials = []

    def score(self, trials):
        out = np.full((self.n_groups, len(trials)), np.nan)
        valid = []
        for t, positions in enumerate(trials):
            positions = [int(p) for p in positions]
            self.trials.append(positions)
            valid.append(bool(self.valid(positions)))
            for g in range(self.n_groups):
                if g not in positions:
                    out[g, t] = self.metric(g, positions)
        return out, valid, self.consensus


# ---- cases ------------------------------------------------------------------------------------------------------------
def toy_problem(context=None, with_mean=False, outliers=True):
    """test_ransac_direct (test_ransac.cc): make_toy_linear_data with observations 3 and 5 set to (-1)^i 400
    (outliers=False: the data as they are, the dataset of MakeRansacChiSquaredGaussianProcess)"""
    with open(os.path.join(os.path.dirname(__file__), "golden", "toy_linear.json")) as fh:
        g = json.load(fh)
    c = g["cov"]
    cov = (ab.SquaredExponential(c["squared_exponential_length_scale"], c["sigma_squared_exponential"])
           + ab.measurement_only(ab.IndependentNoise(c["sigma_independent_noise"])))
    x, y = np.array(g["x"]), np.array(g["y"])
    for i in (3, 5) if outliers else ():
        y[i] = (-1) ** i * 400.
    mean = ab.LinearMean(1., 5.) if with_mean else None
    model = ab.gp_from_covariance_and_mean(cov, mean, context=context) if with_mean else ab.gp_from_covariance(cov, context=context)
    return Problem(model, x, y, None, [[i] for i in range(len(y))])


def ten_point_problem(context=None, with_mean=False):
    """the toy observations (3 and 5 set to +-400) under a prior of condition number 1e5 instead of the toy's 1e7:
    SquaredExponential(10, 10) + measurement noise 0.1, where both numpy routes agree to 1e-11 on every trial"""
    toy = toy_problem()
    cov = ab.SquaredExponential(10., 10.) + ab.measurement_only(ab.IndependentNoise(0.1))
    mean = ab.LinearMean(1., 5.) if with_mean else None
    model = ab.gp_from_covariance_and_mean(cov, mean, context=context) if with_mean else ab.gp_from_covariance(cov, context=context)
    return Problem(model, toy.x, toy.y, None, toy.groups)


RAGGED = [1, 2, 3, 16, 17, 5, 64, 1, 31, 33]


def groups_of(kind, n, rng):
    if kind == "singletons":
        return [[i] for i in range(n)]
    if kind == "sixteen":
        return [list(range(a, min(a + 16, n))) for a in range(0, n, 16)]
    perm = rng.permutation(n)
    out, at, k = [], 0, 0
    while at < n:
        m = min(RAGGED[k % len(RAGGED)], n - at)
        out.append([int(i) for i in perm[at:at + m]])
        at += m
        k += 1
    return out


def synthetic_problem(grouping, n=301, with_var=False, with_mean=False, seed=7, context=None):
    """n points in 3-D, Matern52(2, 1) + IndependentNoise(0.1), targets drawn from the prior, every fifth group shifted"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0., 10., (n, 3))
    cov = ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1)
    mean = ab.LinearMean(0.3, -1.) if with_mean else None
    model = ab.gp_from_covariance_and_mean(cov, mean, context=context) if with_mean else ab.gp_from_covariance(cov, context=context)
    sigma = np.array(orc.gram(cov, x, x_meas=True))
    y = np.linalg.cholesky(sigma) @ rng.standard_normal(n)
    groups = groups_of(grouping, n, rng)
    for gi in range(0, len(groups), 5):
        y[groups[gi]] += 3.
    if with_mean:
        y = y + mean(x)
    y_var = rng.uniform(0.01, 0.05, n) if with_var else None
    return Problem(model, x, y, y_var, groups)


def trials_for(problem, rng, n_trials=65):
    """candidate lists of 1, 3 and 16 groups (at most 256 points), the first and the last groups among them"""
    G = len(problem.groups)
    sizes = np.array([len(g) for g in problem.groups])

    def fits(positions):
        return sizes[list(positions)].sum() <= 256

    trials = [[0], [G - 1], [0, 1, 2], [G - 3, G - 2, G - 1]]
    if G >= 32:
        first = list(range(16))
        while not fits(first):
            first = first[:-1]
        last = list(range(G - 16, G))
        while not fits(last):
            last = last[1:]
        trials += [first, last]
    trials.append([int(np.argmax(sizes))])                     # the largest group alone
    trials.append(sorted({int(np.argmax(sizes)), int(np.argmin(sizes))}))  # ... and with the smallest
    while len(trials) < n_trials:
        k = (1, 3, 16)[len(trials) % 3]
        k = min(k, G - 1)
        pick = sorted(int(p) for p in rng.choice(G, size=k, replace=False))
        if fits(pick):
            trials.append(pick)
    return trials[:n_trials]
