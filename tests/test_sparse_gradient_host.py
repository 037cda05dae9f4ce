"""Host tests of the sparse GP's exact gradient (agp_sparse_nll_gradient): the numpy restatement of its structured
formulas (tests/sparse_gradient_cases.py - through A, Sigma and V, no n x n inverse) against the plain dense gradient
1/2 <Kt^-1 - alpha alpha^T, dKt> and central differences of the dense NLL of Kt; and the entry's presence in the header,
the ctypes table and the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

from sparse_gradient_cases import (assemble_dkt, assemble_kt, dense_gradient, dense_nll, structured_gradient,
                                   structured_weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def se(a, b, length, sigma):
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return sigma * sigma * np.exp(-d2 / (length * length))


def matrices(theta, x, u, yvar):
    """K_ff (measurement pairs: SE + noise on the diagonal), K_fu, K_uu + inducing nugget, d = y_var + measurement nugget"""
    length, sigma, noise, mn, inn = theta
    Kff = se(x, x, length, sigma) + noise * noise * np.eye(len(x))
    return Kff, se(x, u, length, sigma), se(u, u, length, sigma) + inn * np.eye(len(u)), yvar + mn


@pytest.mark.parametrize("layout", ["uniform", "ragged", "singletons"])
@pytest.mark.parametrize("with_yvar", [False, True])
def test_structured_formulas_match_dense_gradient_and_central_differences(layout, with_yvar):
    rng = np.random.default_rng(3)
    n, m = 96, 11
    x = rng.uniform(0., 10., (n, 2))
    u = rng.uniform(0., 10., (m, 2))
    y = np.sin(x).sum(axis=1) + 0.1 * rng.standard_normal(n)
    yvar = rng.uniform(0.01, 0.05, n) if with_yvar else np.zeros(n)
    offsets = {"uniform": np.arange(0, n + 1, 16), "ragged": np.array([0, 7, 30, 31, 60, 96]), "singletons": np.arange(n + 1)}[layout]
    theta = np.array([2.0, 1.0, 0.3, 1e-3, 1e-4])  # length scale, sigma, noise, measurement nugget, inducing nugget

    def nll(t):
        Kff, Kfu, Kuu, d = matrices(t, x, u, yvar)
        return dense_nll(assemble_kt(Kff, Kfu, Kuu, d, offsets), y)

    Kff, Kfu, Kuu, d = matrices(theta, x, u, yvar)
    Kt = assemble_kt(Kff, Kfu, Kuu, d, offsets)
    weights = structured_weights(Kff, Kfu, Kuu, d, offsets, y)
    assert np.abs(weights[3] - np.linalg.solve(Kt, y)).max() <= 1e-9 * np.abs(weights[3]).max()
    for p in range(len(theta)):
        h = 1e-5 * max(1e-2, abs(theta[p]))
        up, down = theta.copy(), theta.copy()
        up[p] += h
        down[p] -= h
        mats_up, mats_down = matrices(up, x, u, yvar), matrices(down, x, u, yvar)
        dKff, dKfu, dKuu, dd = [(a - b) / (2 * h) for a, b in zip(mats_up, mats_down)]
        g, s = structured_gradient(weights, dKff, dKfu, dKuu, dd)
        g_dense = dense_gradient(Kt, y, assemble_dkt(Kfu, Kuu, offsets, dKff, dKfu, dKuu, dd))
        g_fd = (nll(up) - nll(down)) / (2 * h)
        assert abs(g - g_dense) <= 1e-9 * s, (p, g, g_dense, s)
        assert abs(g - g_fd) <= 1e-6 * max(1., abs(g_fd)), (p, g, g_fd)
    # the nuggets are traces of the weights
    assert abs(0.5 * np.trace(weights[0]) - (nll(theta + [0, 0, 0, 1e-7, 0]) - nll(theta - [0, 0, 0, 1e-7, 0])) / 2e-7) <= 1e-5 * abs(np.trace(weights[0]))


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    assert re.search(r"AGP_API int agp_sparse_nll_gradient\(", header)
    from albatross_amd import _capi
    assert "agp_sparse_nll_gradient" in [e[0] for e in _capi.EXPORTS]
    lib = os.path.join(ROOT, "albatross_amd", "libalbatross_amd.so")
    symbols = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bagp_sparse_nll_gradient\b", symbols)
