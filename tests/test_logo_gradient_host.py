"""CPU tests (no GPU) of the leave-one-group-out likelihood metric and its gradient (agp_logo_nll_gradient).

The closed form that agp_logo_nll_gradient evaluates, restated in numpy (logo_closed_form), is checked against brute
force: one refit per group that really leaves the group out, predicts it jointly and scores it with the truth's
variances added (LeaveOneGroupOutLikelihood, evaluation/model_metrics.hpp:74-93; held_out_prediction,
cross_validation_utils.hpp:188-197; prediction_metrics.hpp:112-119), and central differences of those refits.  The
GPU tests use the same restatement as their reference, so this checks the test reference itself.  Also: the blocks
B_g of the weight are indefinite for large residuals with a target variance (nothing may take their square root),
singleton groups reproduce the leave-one-out weight, the header declares the entry and _capi binds it."""
import os
import re

import numpy as np
import pytest

from albatross_amd import _capi as capi
from test_loo_gradient_host import loo_closed_form, se_gram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_2PI = np.log(2 * np.pi)
PARAMS = (1.3, 0.9, 0.2)


def logo_closed_form(K, y, s, groups):
    """(metric, W, u, alpha, [B_g]) from K = k(x, x) + diag(s) and the index arrays `groups`: the formulas of
    include/albatross_amd.h"""
    n = len(y)
    C = np.linalg.inv(K)
    C = 0.5 * (C + C.T)
    alpha = C @ y
    value = 0.
    a = np.zeros(n)
    B = np.zeros((n, n))
    blocks = []
    for I in groups:
        I = np.asarray(I, dtype=np.int64)
        if len(I) == 0:
            continue
        Sigma = np.linalg.inv(C[np.ix_(I, I)])
        Sigma = 0.5 * (Sigma + Sigma.T)
        d = Sigma @ alpha[I]
        V = Sigma + np.diag(s[I])
        q = np.linalg.solve(V, d)
        value += 0.5 * (np.linalg.slogdet(V)[1] + d @ q + len(I) * LOG_2PI)
        aI = Sigma @ q
        Bg = 0.5 * Sigma @ np.linalg.solve(V, Sigma) - 0.5 * np.outer(aI, aI) + 0.5 * (np.outer(aI, d) + np.outer(d, aI))
        Bg = 0.5 * (Bg + Bg.T)
        a[I] = aI
        B[np.ix_(I, I)] = Bg
        blocks.append(Bg)
    u = C @ a
    S = C @ B @ C
    W = S - 0.5 * (np.outer(u, alpha) + np.outer(alpha, u))
    return value, W, u, alpha, blocks


def logo_brute_force(K, y, s, groups):
    """sum_g NLL_g of the joint prediction of group g from a fit on all other points, scored against the group's
    targets with diag(s_I) added to the predictive covariance"""
    n = len(y)
    total = 0.
    for I in groups:
        I = np.asarray(I, dtype=np.int64)
        if len(I) == 0:
            continue
        rest = np.setdiff1d(np.arange(n), I)
        if len(rest):
            w = np.linalg.solve(K[np.ix_(rest, rest)], K[np.ix_(rest, I)])
            mean = w.T @ y[rest]
            cov = K[np.ix_(I, I)] - K[np.ix_(I, rest)] @ w  # the held-out measurements' covariance (s_I included)
        else:
            mean, cov = np.zeros(len(I)), K[np.ix_(I, I)]
        V = 0.5 * (cov + cov.T) + np.diag(s[I])
        dev = y[I] - mean
        total += 0.5 * (np.linalg.slogdet(V)[1] + dev @ np.linalg.solve(V, dev) + len(I) * LOG_2PI)
    return total


def groupings(n, seed=17):
    """ragged sizes from a random permutation, equal groups, one group, singletons"""
    perm = np.random.default_rng(seed).permutation(n)
    sizes = [1, 2, 3, 5, 8, 13, 8]
    assert sum(sizes) == n
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return {
        "ragged": [perm[edges[g]:edges[g + 1]] for g in range(len(sizes))],
        "fours": [np.arange(4 * g, 4 * g + 4) for g in range(n // 4)],
        "one": [perm.copy()],
        "singletons": [np.array([i]) for i in range(n)],
    }


def _problem(n, with_variance, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0., 5., (n, 2))
    y = np.sin(x).sum(axis=1) + 0.1 * rng.standard_normal(n)
    s = rng.uniform(0.01, 0.2, n) if with_variance else np.zeros(n)
    return x, y, s


def indefinite_problem(n, seed=23, residual=5.):
    """large target variances and residuals: some B_g has a negative eigenvalue"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0., 5., (n, 2))
    s = rng.uniform(0.01, 2., n)
    y = residual * np.sin(x).sum(axis=1) + residual * np.sqrt(s) * rng.standard_normal(n)
    return x, y, s


def _check_gradient(x, y, s, groups):
    params = np.array(PARAMS)
    K, dK = se_gram(x, params)
    _, W, _, _, _ = logo_closed_form(K + np.diag(s), y, s, groups)
    for p in range(len(params)):
        h = 1e-5 * max(1., abs(params[p]))
        up, down = params.copy(), params.copy()
        up[p] += h
        down[p] -= h
        fd = (logo_brute_force(se_gram(x, up)[0] + np.diag(s), y, s, groups)
              - logo_brute_force(se_gram(x, down)[0] + np.diag(s), y, s, groups)) / (2 * h)
        g = np.sum(W * dK[p])
        assert abs(g - fd) <= 1e-7 * max(1., abs(fd)), (p, g, fd)


GROUPINGS = ["ragged", "fours", "one", "singletons"]


@pytest.mark.parametrize("with_variance", [False, True])
@pytest.mark.parametrize("grouping", GROUPINGS)
def test_closed_form_value_matches_refits(grouping, with_variance):
    x, y, s = _problem(40, with_variance)
    K, _ = se_gram(x, PARAMS)
    groups = groupings(40)[grouping]
    value = logo_closed_form(K + np.diag(s), y, s, groups)[0]
    want = logo_brute_force(K + np.diag(s), y, s, groups)
    assert abs(value - want) <= 1e-12 * abs(want), (value, want)


@pytest.mark.parametrize("with_variance", [False, True])
@pytest.mark.parametrize("grouping", GROUPINGS)
def test_closed_form_gradient_matches_central_differences_of_refits(grouping, with_variance):
    x, y, s = _problem(40, with_variance, seed=4)
    _check_gradient(x, y, s, groupings(40)[grouping])


@pytest.mark.parametrize("grouping", GROUPINGS)
def test_closed_form_mean_gradient(grouping):
    """d LOGO / d theta = -u^T dm / dtheta for a mean m = theta * x_0: y = targets - m"""
    x, t, s = _problem(40, True, seed=5)
    groups = groupings(40)[grouping]
    K, _ = se_gram(x, PARAMS)
    K = K + np.diag(s)
    theta = 0.3
    u = logo_closed_form(K, t - theta * x[:, 0], s, groups)[2]
    h = 1e-5
    fd = (logo_brute_force(K, t - (theta + h) * x[:, 0], s, groups)
          - logo_brute_force(K, t - (theta - h) * x[:, 0], s, groups)) / (2 * h)
    assert abs(-u @ x[:, 0] - fd) <= 1e-7 * max(1., abs(fd))


def test_indefinite_blocks_keep_the_gradient_exact():
    """B_g = 1/2 Sigma V^-1 Sigma + 1/2 d d^T - 1/2 e e^T, e = diag(s_I) V^-1 d, is not positive semi-definite in
    general: no Cholesky factor or square root of it exists, and the formula still holds."""
    x, y, s = indefinite_problem(40)
    groups = groupings(40)["ragged"]
    K, _ = se_gram(x, PARAMS)
    value, _, _, _, blocks = logo_closed_form(K + np.diag(s), y, s, groups)
    assert min(np.linalg.eigvalsh(b).min() for b in blocks) < -0.1
    want = logo_brute_force(K + np.diag(s), y, s, groups)
    assert abs(value - want) <= 1e-12 * abs(want), (value, want)
    _check_gradient(x, y, s, groups)


@pytest.mark.parametrize("with_variance", [False, True])
def test_singleton_groups_reproduce_the_leave_one_out_weight(with_variance):
    x, y, s = _problem(40, with_variance, seed=6)
    K, _ = se_gram(x, PARAMS)
    K = K + np.diag(s)
    value, W, u, _, _ = logo_closed_form(K, y, s, groupings(40)["singletons"])
    loo_value, loo_W, loo_u, _, _ = loo_closed_form(K, y, s)
    assert abs(value - loo_value) <= 1e-13 * abs(loo_value)
    assert np.abs(W - loo_W).max() <= 1e-12 * np.abs(loo_W).max()
    assert np.abs(u - loo_u).max() <= 1e-12 * np.abs(loo_u).max()


def test_header_declares_logo_gradient_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    assert re.search(r"AGP_API int agp_logo_nll_gradient\(agp_context \*ctx, const agp_kernel \*k, const agp_features \*x,"
                     r"\s*const double \*y, const double \*y_var,\s*int64_t n_groups, const int64_t \*offsets,"
                     r"\s*const int64_t \*indices,\s*int n_slots, const agp_gradient_slot \*slots,"
                     r"\s*const double \*tangents, int64_t ldt,\s*double \*logo_nll, double \*grad_logo_nll,"
                     r"\s*double \*mean_weights\);", text)
    exports = {name: (res, args) for name, res, args in capi.EXPORTS}
    assert "agp_logo_nll_gradient" in exports
    loo = exports["agp_loo_nll_gradient"][1]
    assert exports["agp_logo_nll_gradient"][1] == loo[:5] + [capi.C.c_int64, loo[0], loo[0]] + loo[5:]
    assert hasattr(capi.load(), "agp_logo_nll_gradient")
