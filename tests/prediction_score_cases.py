"""numpy restatement of the reference's prediction scores (include/albatross/src/evaluation/prediction_metrics.hpp)
and of the library's counter-based normal generator, shared by tests/test_prediction_scores_host.py (which pins it)
and tests/test_prediction_scores_gpu.py (which compares the device entries against it).  Plain fp64 numpy, no GPU."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).
    counter: four arrays of 32-bit words, key: two 32-bit words; returns the four output words (uint64 arrays < 2^32)."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def standard_normal(seed, m, first_column, n_columns):
    """what agp_standard_normal documents (include/albatross_amd.h): key = the halves of the seed, counter =
    (row, column, 0, 0), two 53-bit uniforms centred in their cells, the cosine branch of Box-Muller"""
    rows = np.arange(m, dtype=np.uint64)[:, None]
    cols = (np.arange(n_columns, dtype=np.uint64) + np.uint64(first_column))[None, :]
    zero = np.zeros((1, 1), dtype=np.uint64)
    r = philox4x32_10((rows, cols, zero, zero), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = (((r[0] | (r[1] << np.uint64(32))) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = (((r[2] | (r[3] << np.uint64(32))) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return np.sqrt(-2. * np.log(u1)) * np.cos((2. * math.pi) * u2)


def crps_normal(mu, sigma, y):
    """score::crps_normal, prediction_metrics.hpp:349-364"""
    if not (math.isfinite(mu) and math.isfinite(sigma) and math.isfinite(y)):
        return math.nan
    if sigma <= 0.:
        return abs(y - mu)
    z = (y - mu) / sigma
    return sigma * (z * math.erf(z / math.sqrt(2.)) + 2. * math.exp(-0.5 * z * z) / math.sqrt(2. * math.pi) - 1. / math.sqrt(math.pi))


def expected_abs_normal_1(mu, sigma):
    """detail::expected_abs_normal_1, prediction_metrics.hpp:287-301"""
    if not (math.isfinite(mu) and math.isfinite(sigma)):
        return math.nan
    if sigma <= 0.:
        return abs(mu)
    normalized = abs(mu) / max(1.0e-16, sigma)
    return sigma * math.sqrt(2. / math.pi) * math.exp(-0.5 * normalized * normalized) + abs(mu) * math.erf(normalized / math.sqrt(2.))


def energy_score_terms(mean, cov, truth, weights, z, truth_var=None):
    """score::energy_score, prediction_metrics.hpp:387-435, with the normals supplied: z is m x 2k, k = num_samples / 2 + 1;
    the draws go through the LL^T of cov (+ diag(truth_var)) as the library's do (the reference: pivoted LDL^T, :200-217).
    Returns (term1, paired) = (the mean of the two mean_err_norms, pairwise_errors_paired)."""
    mean, truth = np.asarray(mean, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    m = mean.shape[0]
    c = np.array(cov, dtype=np.float64).reshape(m, m)
    if truth_var is not None:
        c[np.diag_indices(m)] += truth_var                     # :431-432
    w = np.ones(m) if weights is None else np.asarray(weights, dtype=np.float64)
    L = np.linalg.cholesky(c)
    k = z.shape[1] // 2

    def antithetic(zs):                                        # :258-277
        left = mean[:, None] + L @ zs                          # draw_mvn
        return np.concatenate([left, 2. * mean[:, None] - left], axis=1)

    def mean_err_norms(samples):                               # :221-234
        return np.sqrt((((samples - truth[:, None]) ** 2) * w[:, None]).sum(axis=0)).mean()

    a, b = antithetic(z[:, :k]), antithetic(z[:, k:])
    paired = np.sqrt((((a - b) * w[:, None]) ** 2).sum(axis=0)).mean()   # :244-256
    return 0.5 * (mean_err_norms(a) + mean_err_norms(b)), paired


def energy_score(mean, cov, truth, weights, z, truth_var=None):
    term1, paired = energy_score_terms(mean, cov, truth, weights, z, truth_var)
    return max(0., term1 - 0.5 * paired)                       # :415-421


def variogram_score(mean, cov, truth, weights=None, order=1, truth_var=None):
    """score::variogram_score, prediction_metrics.hpp:465-520 (order 1: madogram, 2: variogram)"""
    mean, truth = np.asarray(mean, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    m = mean.shape[0]
    c = np.asarray(cov, dtype=np.float64)
    d = np.diag(c) + (0. if truth_var is None else np.asarray(truth_var, dtype=np.float64))   # :517-518
    total = 0.
    for row in range(m - 1):
        mu = mean[row + 1:] - mean[row]
        sigma = np.sqrt(d[row] + d[row + 1:] - 2. * c[row, row + 1:])
        if order == 2:
            expectation = mu * mu + sigma * sigma
        else:
            expectation = np.array([expected_abs_normal_1(a, b) for a, b in zip(mu, sigma)])
        diff = np.abs(truth[row] - truth[row + 1:]) ** order - expectation
        w = 1. if weights is None else weights[row, row + 1:]
        total += (w * diff * diff).sum()
    return total


def random_covariance(rng, m):
    """A A^T / m + I: well conditioned, off-diagonal correlations far below 0.9, so c_ii + c_jj - 2 c_ij has no
    cancellation"""
    a = rng.standard_normal((m, m))
    return a @ a.T / m + np.eye(m)


def max_offdiagonal_correlation(c):
    s = np.sqrt(np.diag(c))
    r = c / np.outer(s, s)
    return np.abs(r - np.diag(np.diag(r))).max() if c.shape[0] > 1 else 0.
