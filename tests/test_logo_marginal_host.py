"""CPU tests (no GPU) of the leave-one-group-out likelihood metric with the MARGINAL predict type and its gradient
(agp_logo_nll_gradient_typed, AGP_PREDICT_MARGINAL).

The closed form the entry evaluates, restated in numpy (logo_marginal_closed_form: the formulas of
include/albatross_amd.h), is checked against brute force: one refit per group that really leaves the group out,
predicts it and scores every point of it against its own predictive variance with the truth's variance added
(LeaveOneGroupOutLikelihood<FeatureType, MarginalDistribution>, evaluation/model_metrics.hpp:74-93;
prediction_metrics.hpp:112-128), and central differences of those refits.  The GPU tests use the same restatement as
their reference, so this checks the test reference itself.  Bounds: those of tests/test_logo_gradient_host.py.  Also:
the weights w_i = 1/2 (1 / v_i - q_i^2) are negative for large residuals, so the blocks B_g are indefinite (nothing may
take a root of w) and the gradient still holds; singleton groups reproduce the leave-one-out value and weight; the
header declares the entry with both predict-type constants and _capi binds it."""
import os
import re

import numpy as np
import pytest

from albatross_amd import _capi as capi
from test_logo_gradient_host import LOG_2PI, PARAMS, _problem, groupings, indefinite_problem
from test_loo_gradient_host import loo_closed_form, se_gram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def logo_marginal_closed_form(K, y, s, groups):
    """(metric, W, u, alpha, [B_g], [NLL_g]) from K = k(x, x) + diag(s) and the index arrays `groups` (an empty group
    has NLL_g = 0 and no block): the Marginal formulas of include/albatross_amd.h"""
    n = len(y)
    C = np.linalg.inv(K)
    C = 0.5 * (C + C.T)
    alpha = C @ y
    a = np.zeros(n)
    B = np.zeros((n, n))
    blocks, terms = [], []
    for I in groups:
        I = np.asarray(I, dtype=np.int64)
        if len(I) == 0:
            terms.append(0.)
            continue
        Sigma = np.linalg.inv(C[np.ix_(I, I)])
        Sigma = 0.5 * (Sigma + Sigma.T)
        d = Sigma @ alpha[I]
        v = np.diag(Sigma) + s[I]
        q = d / v
        w = 0.5 * (1. / v - q * q)
        terms.append(0.5 * np.sum(np.log(v) + d * q + LOG_2PI))
        aI = Sigma @ q
        Bg = Sigma @ (w[:, None] * Sigma) + 0.5 * (np.outer(aI, d) + np.outer(d, aI))
        Bg = 0.5 * (Bg + Bg.T)
        a[I] = aI
        B[np.ix_(I, I)] = Bg
        blocks.append(Bg)
    u = C @ a
    S = C @ B @ C
    W = S - 0.5 * (np.outer(u, alpha) + np.outer(alpha, u))
    return float(np.sum(terms)), W, u, alpha, blocks, terms


def logo_marginal_brute_force(K, y, s, groups):
    """sum over the groups, and over the points of a group, of the NLL of the point's prediction from a fit on all
    points outside the group, with s_i added to the predictive variance"""
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
            var = np.diag(K[np.ix_(I, I)]) - np.einsum("ij,ij->j", K[np.ix_(rest, I)], w)  # (s_I included: measurements)
        else:
            mean, var = np.zeros(len(I)), np.diag(K[np.ix_(I, I)])
        v = var + s[I]
        dev = y[I] - mean
        total += 0.5 * np.sum(np.log(v) + dev * dev / v + LOG_2PI)
    return total


def _check_gradient(x, y, s, groups):
    params = np.array(PARAMS)
    K, dK = se_gram(x, params)
    W = logo_marginal_closed_form(K + np.diag(s), y, s, groups)[1]
    for p in range(len(params)):
        h = 1e-5 * max(1., abs(params[p]))
        up, down = params.copy(), params.copy()
        up[p] += h
        down[p] -= h
        fd = (logo_marginal_brute_force(se_gram(x, up)[0] + np.diag(s), y, s, groups)
              - logo_marginal_brute_force(se_gram(x, down)[0] + np.diag(s), y, s, groups)) / (2 * h)
        g = np.sum(W * dK[p])
        assert abs(g - fd) <= 1e-7 * max(1., abs(fd)), (p, g, fd)


GROUPINGS = ["ragged", "fours", "one", "singletons"]


@pytest.mark.parametrize("with_variance", [False, True])
@pytest.mark.parametrize("grouping", GROUPINGS)
def test_closed_form_value_matches_refits(grouping, with_variance):
    x, y, s = _problem(40, with_variance)
    K, _ = se_gram(x, PARAMS)
    groups = groupings(40)[grouping]
    value, _, _, _, _, terms = logo_marginal_closed_form(K + np.diag(s), y, s, groups)
    want = logo_marginal_brute_force(K + np.diag(s), y, s, groups)
    assert abs(value - want) <= 1e-12 * abs(want), (value, want)
    assert len(terms) == len(groups)


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
    u = logo_marginal_closed_form(K, t - theta * x[:, 0], s, groups)[2]
    h = 1e-5
    fd = (logo_marginal_brute_force(K, t - (theta + h) * x[:, 0], s, groups)
          - logo_marginal_brute_force(K, t - (theta - h) * x[:, 0], s, groups)) / (2 * h)
    assert abs(-u @ x[:, 0] - fd) <= 1e-7 * max(1., abs(fd))


@pytest.mark.parametrize("with_variance", [False, True])
@pytest.mark.parametrize("grouping", GROUPINGS)
def test_indefinite_problem_value_and_gradient(grouping, with_variance):
    x, y, s = indefinite_problem(40)
    if not with_variance:
        s = np.zeros(40)
    groups = groupings(40)[grouping]
    K, _ = se_gram(x, PARAMS)
    value = logo_marginal_closed_form(K + np.diag(s), y, s, groups)[0]
    want = logo_marginal_brute_force(K + np.diag(s), y, s, groups)
    assert abs(value - want) <= 1e-12 * abs(want), (value, want)
    _check_gradient(x, y, s, groups)


def test_indefinite_blocks_keep_the_gradient_exact():
    """w_i = 1/2 (1 / v_i - q_i^2) < 0 wherever d_i^2 > v_i: B_g = Sigma diag(w) Sigma + sym(a d^T) has negative
    eigenvalues, no root of w or factor of B_g exists, and the formula still holds"""
    x, y, s = indefinite_problem(40)
    groups = groupings(40)["ragged"]
    K, _ = se_gram(x, PARAMS)
    blocks = logo_marginal_closed_form(K + np.diag(s), y, s, groups)[4]
    assert min(np.linalg.eigvalsh(b).min() for b in blocks) < -0.1
    _check_gradient(x, y, s, groups)


@pytest.mark.parametrize("with_variance", [False, True])
def test_singleton_groups_reproduce_the_leave_one_out_weight(with_variance):
    x, y, s = _problem(40, with_variance, seed=6)
    K, _ = se_gram(x, PARAMS)
    K = K + np.diag(s)
    value, W, u, _, _, _ = logo_marginal_closed_form(K, y, s, groupings(40)["singletons"])
    loo_value, loo_W, loo_u, _, _ = loo_closed_form(K, y, s)
    assert abs(value - loo_value) <= 1e-13 * abs(loo_value)
    assert np.abs(W - loo_W).max() <= 1e-12 * np.abs(loo_W).max()
    assert np.abs(u - loo_u).max() <= 1e-12 * np.abs(loo_u).max()


def test_header_declares_the_typed_entry_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    assert re.search(r"^#define AGP_PREDICT_JOINT 0$", text, re.M)
    assert re.search(r"^#define AGP_PREDICT_MARGINAL 1$", text, re.M)
    assert re.search(r"AGP_API int agp_logo_nll_gradient_typed\(agp_context \*ctx, const agp_kernel \*k, const agp_features \*x,"
                     r"\s*const double \*y, const double \*y_var,\s*int64_t n_groups, const int64_t \*offsets,"
                     r"\s*const int64_t \*indices,\s*int predict_type,\s*int n_slots, const agp_gradient_slot \*slots,"
                     r"\s*const double \*tangents, int64_t ldt,\s*double \*logo_nll, double \*grad_logo_nll,"
                     r"\s*double \*mean_weights,\s*double \*group_nll\);", text)
    assert "is not built" not in text
    assert (capi.PREDICT_JOINT, capi.PREDICT_MARGINAL) == (0, 1)
    exports = {name: (res, args) for name, res, args in capi.EXPORTS}
    assert "agp_logo_nll_gradient_typed" in exports
    logo = exports["agp_logo_nll_gradient"][1]
    assert exports["agp_logo_nll_gradient_typed"][1] == logo[:8] + [capi.C.c_int] + logo[8:] + [logo[0]]
    assert hasattr(capi.load(), "agp_logo_nll_gradient_typed")
