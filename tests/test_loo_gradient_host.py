"""CPU tests (no GPU) of the leave-one-out likelihood metric and its gradient (agp_loo_nll_gradient).

The closed form that agp_loo_nll_gradient evaluates, restated in numpy, is checked against brute force: n refits that
each leave one point out, predict it and score it with the truth's variance added (LeaveOneOutLikelihood,
evaluation/model_metrics.hpp:59-72; prediction_metrics.hpp:113-119), and central differences of those refits.  The
GPU tests use the same restatement as their reference, so this checks the test reference itself.  Also: the header
declares the entry and _capi binds it."""
import os
import re

import numpy as np
import pytest

from albatross_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_2PI = np.log(2 * np.pi)


def se_gram(x, params):
    """k(x, x) of SE(length_scale, sigma) + IndependentNoise(sigma_noise) on 2-D points, and dk / dparams"""
    ls, sg, sn = params
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    e = np.exp(-d2 / ls ** 2)
    K = sg ** 2 * e + sn ** 2 * np.eye(len(x))
    return K, [sg ** 2 * e * 2 * d2 / ls ** 3, 2 * sg * e, 2 * sn * np.eye(len(x))]


def loo_closed_form(K, y, s):
    """(LOO metric, W, u, alpha) from K = k(x, x) + diag(s): the formulas of include/albatross_amd.h"""
    C = np.linalg.inv(K)
    C = 0.5 * (C + C.T)
    alpha = C @ y
    c = np.diag(C)
    v = 1. / c + s
    d = alpha / c
    value = 0.5 * np.sum(np.log(v) + d * d / v + LOG_2PI)
    b = (1. - d * d / v + 2. * alpha * d) / (2. * v * c * c)
    a = d / (v * c)
    u = C @ a
    W = C @ np.diag(b) @ C - 0.5 * (np.outer(u, alpha) + np.outer(alpha, u))
    return value, W, u, alpha, b


def loo_brute_force(K, y, s):
    """sum_i NLL_i of the prediction of point i from a fit on the other n - 1, scored with v_i = var_i + s_i"""
    n = len(y)
    total = 0.
    for i in range(n):
        rest = np.arange(n) != i
        Kr = K[np.ix_(rest, rest)]
        k = K[rest, i]
        w = np.linalg.solve(Kr, k)
        mean = w @ y[rest]
        var = K[i, i] - w @ k  # the held-out measurement's variance (s_i included: K carries diag(s))
        v = var + s[i]
        dev = y[i] - mean
        total += 0.5 * (np.log(v) + dev * dev / v + LOG_2PI)
    return total


def _problem(n, with_variance, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0., 5., (n, 2))
    y = np.sin(x).sum(axis=1) + 0.1 * rng.standard_normal(n)
    s = rng.uniform(0.01, 0.2, n) if with_variance else np.zeros(n)
    return x, y, s


@pytest.mark.parametrize("with_variance", [False, True])
def test_closed_form_value_matches_refits(with_variance):
    x, y, s = _problem(40, with_variance)
    K, _ = se_gram(x, (1.3, 0.9, 0.2))
    value, _, _, _, b = loo_closed_form(K + np.diag(s), y, s)
    assert np.all(b > 0)
    want = loo_brute_force(K + np.diag(s), y, s)
    assert abs(value - want) <= 1e-12 * abs(want), (value, want)


@pytest.mark.parametrize("with_variance", [False, True])
def test_closed_form_gradient_matches_central_differences_of_refits(with_variance):
    x, y, s = _problem(40, with_variance, seed=4)
    params = np.array([1.3, 0.9, 0.2])
    K, dK = se_gram(x, params)
    _, W, _, _, _ = loo_closed_form(K + np.diag(s), y, s)
    for p in range(len(params)):
        h = 1e-5 * max(1., abs(params[p]))
        up, down = params.copy(), params.copy()
        up[p] += h
        down[p] -= h
        fd = (loo_brute_force(se_gram(x, up)[0] + np.diag(s), y, s)
              - loo_brute_force(se_gram(x, down)[0] + np.diag(s), y, s)) / (2 * h)
        g = np.sum(W * dK[p])
        assert abs(g - fd) <= 1e-7 * max(1., abs(fd)), (p, g, fd)


def test_closed_form_mean_gradient():
    """d LOO / d theta = -u^T dm / dtheta for a mean m = theta * x_0: y = targets - m"""
    x, t, s = _problem(40, True, seed=5)
    K, _ = se_gram(x, (1.3, 0.9, 0.2))
    K = K + np.diag(s)
    theta = 0.3
    _, _, u, _, _ = loo_closed_form(K, t - theta * x[:, 0], s)
    h = 1e-5
    fd = (loo_brute_force(K, t - (theta + h) * x[:, 0], s) - loo_brute_force(K, t - (theta - h) * x[:, 0], s)) / (2 * h)
    assert abs(-u @ x[:, 0] - fd) <= 1e-7 * max(1., abs(fd))


def test_header_declares_loo_gradient_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    assert re.search(r"AGP_API int agp_loo_nll_gradient\(agp_context \*ctx, const agp_kernel \*k, const agp_features \*x,"
                     r"\s*const double \*y, const double \*y_var,\s*int n_slots, const agp_gradient_slot \*slots,"
                     r"\s*const double \*tangents, int64_t ldt,\s*double \*loo_nll, double \*grad_loo_nll,"
                     r"\s*double \*mean_weights\);", text)
    exports = {name: (res, args) for name, res, args in capi.EXPORTS}
    assert "agp_loo_nll_gradient" in exports
    assert exports["agp_loo_nll_gradient"][1] == exports["agp_nll_gradient"][1]
    assert hasattr(capi.load(), "agp_loo_nll_gradient")
