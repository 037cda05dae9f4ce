"""The premises of tests/test_gram_paths_gpu.py, checked without a GPU: the case tables are not empty, every planted
duplicate / near-duplicate / id construction gives the noise pattern its comment claims (evaluated with the oracle), and
the reference and the bound of the predictive mean are consistent with each other - a plain fp64 numpy evaluation of the
sum in the tiled kernel's order meets the bound at every (N, M) of the table, and no test point's bound is zero."""
import numpy as np
import pytest

import albatross_amd as ab
import gram_path_cases as gc
from oracle import oracle_py as orc

NOISE = ab.IndependentNoise(gc.NOISE_SIGMA)
NV = gc.NOISE_SIGMA * gc.NOISE_SIGMA


def noise_pattern(fx, fy=None):
    """the (i, j) at which the oracle's noise term is non-zero, and that it is sigma^2 there"""
    K = orc.gram(NOISE, fx) if fy is None else orc.gram(NOISE, fx, fy)
    i, j = np.nonzero(K)
    assert np.all(K[i, j] == NV)
    return sorted(zip(i.tolist(), j.tolist()))


def test_case_tables_are_not_empty():
    assert gc.FAST_CROSS_SHAPES and gc.FAST_NOISE_KINDS and gc.LOWER_SIZES and gc.PAIR2_TREES and gc.GENERIC_DIMS
    assert gc.BLOCK_ROWS and gc.BLOCK_COUNTS and gc.PM_M and gc.PM_N and gc.FAST_COMBOS
    shapes = gc.predict_mean_shapes()
    assert len(shapes) == len(gc.PM_M) + 2 * len(gc.PM_N) - 2  # (257, 1027) and (257, 5) are in the first list already
    assert all((257, m) in shapes for m in gc.PM_M) and all((n, 1027) in shapes and (n, 5) in shapes for n in gc.PM_N)
    cases = gc.predict_mean_fast_cases()
    assert {(c[0], c[1]) for c in cases} >= set(shapes)
    # every (op, dim) pair on each of the three fast kernels
    for path in (gc.TILED8, gc.TILED4, gc.FAST_WAVE):
        assert {(c[2], c[3]) for c in cases if gc.expected_fast_pm_path(c[1]) == path} == set(gc.FAST_COMBOS)
    # each one-sided id mode on each fast kernel, with plain noise under both measurement flags of the test points
    for path in (gc.TILED8, gc.TILED4, gc.FAST_WAVE):
        for mode in ("x", "xs"):
            assert {c[5] for c in cases if gc.expected_fast_pm_path(c[1]) == path and c[6] == mode and c[4] == "noise"} == {False, True}
        assert any(c[6] == "both" for c in cases if gc.expected_fast_pm_path(c[1]) == path)
    assert {("noise", False), ("noise", True), ("meas", False), ("meas", True)} <= {(c[4], c[5]) for c in cases}
    # the (EUCLID, ANGULAR) written beside each pair-2 tree is what its program's radial leaves say
    for name, build, _, claim in gc.PAIR2_TREES:
        assert gc.tree_metrics(build()) == claim, name
    # all four (EUCLID, ANGULAR) instantiations of the pair-2 kernel at every dimension they allow
    seen = {(e, a, d) for _, _, dims, (e, a) in gc.PAIR2_TREES for d in dims}
    assert seen == {(e, a, d) for e in (False, True) for a in (False, True) for d in (1, 2, 3) if not (a and d == 1)}
    # both parities of the leading dimension at every cross shape
    assert all({ld % 2 for ld in gc.cross_lds(r)} == {0, 1} for r, _ in gc.FAST_CROSS_SHAPES)


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("rows,cols", gc.FAST_CROSS_SHAPES)
def test_planted_cross_pairs(rows, cols, dim):
    x, y, pairs = gc.planted_cross(rows, cols, dim, 7 * rows + cols + dim)
    assert noise_pattern(x, y) == sorted(pairs["equal"])
    for i, j in pairs["near"]:
        assert np.array_equal(x[i, :-1], y[j, :-1]) and x[i, -1] != y[j, -1]
    for i, j in pairs["underflow"]:
        assert ((x[i] - y[j]) ** 2).sum() == 0. and abs(x[i, 0] - y[j, 0]) == 1e-170 and np.array_equal(x[i, 1:], y[j, 1:])
    if cols > 9:
        assert pairs["underflow"] and (dim == 1 or pairs["near"]) and len(pairs["equal"]) == 3
    # a squared exponential sees sigma^2 at the underflow pair, which therefore reaches the kernels' `maybe` test
    K = orc.gram(gc.fast_cov(0, "noise"), x, y)
    for i, j in pairs["underflow"]:
        assert K[i, j] == 1.3 * 1.3
    for i, j in pairs["equal"]:
        assert K[i, j] == 1.3 * 1.3 + NV


@pytest.mark.parametrize("n", gc.LOWER_SIZES + [gc.PAIR2_SHAPE[0]])
def test_planted_symmetric_pairs(n):
    x, equal = gc.planted_symmetric(n, 3, n)
    assert noise_pattern(x) == sorted(equal)
    assert n <= 4 or len(equal) > n


@pytest.mark.parametrize("rows,cols", [gc.PAIR2_SHAPE, (129, 129)])
def test_planted_id_pairs(rows, cols):
    x, y, xi, yi, pairs = gc.planted_ids(rows, cols, 3, 5)
    fx, fy = gc.features(NOISE, x, ids=xi), gc.features(NOISE, y, ids=yi)
    assert noise_pattern(fx, fy) == sorted(pairs["equal_ids"])
    # one side without ids: the comparison falls back to the coordinates
    assert noise_pattern(gc.features(NOISE, x), fy) == sorted(pairs["equal_coords"])
    assert noise_pattern(fx, gc.features(NOISE, y)) == sorted(pairs["equal_coords"])
    assert set(pairs["equal_ids"]) - set(pairs["equal_coords"]) and set(pairs["equal_coords"]) - set(pairs["equal_ids"])


def test_planted_predict_mean_pairs():
    for n, m in [(257, 1027), (1, 5), (513, 5), (257, 1), (257, 16391)]:
        x, xs, _, pairs, _, _ = gc.predict_mean_points(n, m, 2, n + m)
        assert noise_pattern(x, xs) == sorted(pairs)
        assert (n - 1, m - 1) in pairs
        assert len({j for _, j in pairs}) == len(pairs)  # a test point is the copy of at most one training point
        x2, xs2, _, id_pairs, xi, si = gc.predict_mean_points(n, m, 2, n + m, ids="both")
        assert np.array_equal(x2, x) and np.array_equal(xs2, xs) and xi is not None and si is not None
        assert noise_pattern(gc.features(NOISE, x, ids=xi), gc.features(NOISE, xs, ids=si)) == sorted(id_pairs)
        assert m < 3 or (set(id_pairs) - set(pairs) and set(pairs) - set(id_pairs))  # ids and coordinates disagree somewhere
        # ids on one side only: the noise appears by coordinates, exactly where it does without ids - and not where the
        # ids of the 'both' construction would put it
        for mode in ("x", "xs"):
            _, _, _, one_pairs, oi, osi = gc.predict_mean_points(n, m, 2, n + m, ids=mode)
            assert (oi is None) != (osi is None) and (oi is not None) == (mode == "x")
            assert one_pairs == pairs
            assert noise_pattern(gc.features(NOISE, x, ids=oi), gc.features(NOISE, xs, ids=osi)) == sorted(pairs)
    # the partial last tile of both tile widths holds a planted pair
    assert 1027 % 4 and 16391 % 8


def test_predict_mean_bound_and_reference_are_consistent():
    """every case of the table: the fp64 sum in the tiled kernel's order is within the bound of the longdouble reference,
    and the bound is positive at every test point"""
    assert gc.HAVE_LONGDOUBLE
    for n, m, op, dim, kind, xs_meas, ids in gc.predict_mean_fast_cases():
        cov = gc.fast_cov(op, kind)
        x, xs, alpha, _, xi, si = gc.predict_mean_points(n, m, dim, 31 * n + m, ids)
        fx, fxs = gc.features(cov, x, True, xi), gc.features(cov, xs, xs_meas, si)
        r, S, K = gc.predict_mean_reference(cov, fx, fxs, alpha)
        assert np.all(S > 0.), (n, m)
        assert np.all(gc.predict_mean_bound(n, S) > 0.)
        got = gc.predict_mean_tiled_numpy(K, alpha)
        assert gc.predict_mean_ok(got, r, S, n), (n, m, op, dim)
        # ... and a wrong tile edge is not: the last test point evaluated at its neighbour's position
        if m > 1:
            bad = got.copy()
            bad[m - 1] = got[m - 2]
            assert not gc.predict_mean_ok(bad, r, S, n)
