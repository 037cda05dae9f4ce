"""CPU tests that pin tests/prediction_score_cases.py, the numpy restatement the GPU tests of the prediction scores
compare against: the Philox4x32-10 generator behind agp_standard_normal and the reference's crps_normal,
expected_abs_normal_1 and energy_score (include/albatross/src/evaluation/prediction_metrics.hpp)."""
import math

import numpy as np

import prediction_score_cases as pc


def words(counter, key):
    c = [np.array([v], dtype=np.uint64) for v in counter]
    return [int(w[0]) for w in pc.philox4x32_10(c, key)]


def test_philox_known_answers():
    """The known-answer vectors Random123 publishes for philox4x32_10 (its kat_vectors file: counter and key all zero, all
    ones, and the digits of pi).  No copy of that file and no other Philox4x32 implementation that runs on a CPU is
    installed beside this project (numpy's Philox is the 4x64 variant), so the vectors are quoted from the publication
    and, beyond them, three counters of the shape the library uses - (row, column, 0, 0) under key (22, 0) - are pinned
    as regression constants of this helper."""
    assert words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert words((f, f, f, f), (f, f)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    assert words((1, 2, 0, 0), (22, 0)) == [0x730bec2c, 0x6c7f5929, 0x6ac6b321, 0xd3a42dce]
    assert words((129, 17, 0, 0), (22, 0)) == [0xf7b63298, 0x43cd801f, 0xb3c87789, 0x287547da]
    assert words((4000000000, 7, 0, 0), (22, 0)) == [0xd5cb884a, 0xa49896db, 0xa6f27a30, 0x95f8edf0]


def test_standard_normal_is_a_function_of_seed_row_and_column():
    a, b = pc.standard_normal(22, 50, 0, 64), pc.standard_normal(22, 50, 32, 64)
    assert np.array_equal(a[:, 32:], b[:, :32])
    assert np.array_equal(pc.standard_normal(22, 20, 7, 3), pc.standard_normal(22, 50, 0, 64)[:20, 7:10])
    assert not np.array_equal(a, pc.standard_normal(1 << 32 | 22, 50, 0, 64))  # the high word of the seed is the second key word
    assert np.isfinite(a).all() and np.abs(a).max() <= 8.6


def test_standard_normal_moments_of_the_seed_the_gpu_test_uses():
    z = pc.standard_normal(22, 256, 0, 1024)
    n = z.size
    assert abs(z.mean()) <= 5. / math.sqrt(n) and abs(z.var() - 1.) <= 5. * math.sqrt(2. / n)


def test_crps_normal():
    assert pc.crps_normal(5., 0., 3.) == 2. and pc.crps_normal(5., 0., 5.) == 0. and pc.crps_normal(5., -1., 3.) == 2.
    for bad in (math.nan, math.inf, -math.inf):
        assert math.isnan(pc.crps_normal(bad, 1., 0.)) and math.isnan(pc.crps_normal(0., bad, 0.)) and math.isnan(pc.crps_normal(0., 1., bad))
    # the closed form at y = mu: sigma (sqrt(2) - 1) / sqrt(pi)
    assert abs(pc.crps_normal(1., 2., 1.) - 2. * (math.sqrt(2.) - 1.) / math.sqrt(math.pi)) <= 1e-15


def test_expected_abs_normal_1():
    for sigma in (1e-3, 0.7, 1., 42.):
        assert abs(pc.expected_abs_normal_1(0., sigma) - sigma * math.sqrt(2. / math.pi)) <= 1e-12
    assert pc.expected_abs_normal_1(-3., 0.) == 3. and pc.expected_abs_normal_1(-3., -1.) == 3.
    assert math.isnan(pc.expected_abs_normal_1(math.nan, 1.)) and math.isnan(pc.expected_abs_normal_1(0., math.inf))


def test_energy_score_matches_crps_in_one_dimension():
    """tests/test_stats_scores.cc:215-250 with this project's generator: 500 samples, |ES - CRPS| <= 2 sqrt(2 sigma^2 / 500);
    the same draws of (mu, sigma, truth) and the same seed as the GPU test of the device entry"""
    rng = np.random.default_rng(9999)
    k = 500 // 2 + 1
    z = pc.standard_normal(444, 1, 0, 2 * k)
    for _ in range(40):
        mu, sigma, truth = rng.uniform(-10., 10.), rng.uniform(0.1, 5.), rng.uniform(-10., 10.)
        es = pc.energy_score(np.array([mu]), np.array([[sigma * sigma]]), np.array([truth]), None, z)
        assert abs(es - pc.crps_normal(mu, sigma, truth)) <= 2. * math.sqrt(2. * sigma * sigma / 500.)


def test_variogram_score_restatement_against_a_double_loop():
    rng = np.random.default_rng(1)
    m = 7
    c = pc.random_covariance(rng, m)
    assert pc.max_offdiagonal_correlation(c) <= 0.9
    mean, truth, w = rng.standard_normal(m), rng.standard_normal(m), rng.uniform(0.1, 2., (m, m))
    for order in (1, 2):
        total = 0.
        for i in range(m):
            for j in range(i + 1, m):
                sigma = math.sqrt(c[i, i] + c[j, j] - 2. * c[i, j])
                e = pc.expected_abs_normal_1(mean[j] - mean[i], sigma) if order == 1 else (mean[j] - mean[i]) ** 2 + sigma * sigma
                total += w[i, j] * (abs(truth[i] - truth[j]) ** order - e) ** 2
        assert abs(pc.variogram_score(mean, c, truth, w, order) - total) <= 1e-12 * total
    assert pc.variogram_score(mean[:1], c[:1, :1], truth[:1]) == 0.
