"""No GPU: a float64 numpy restatement of agp_gram_matvec's summation order (tests/gram_matvec_cases.py: restatement) meets
the bound of that module on the very inputs of tests/test_gram_matvec_gpu.py, with K from the CPU restatement of the
covariance functions - so the bound asks nothing of the kernel that plain double arithmetic in the defined order does
not give - and reproduces the columns of the matrix bit for bit from columns of the identity.  Also pins the Python
restatement of the slice rule to the values the cases file quotes."""
import numpy as np
import pytest

import albatross_amd as ab  # noqa: F401  (the package must import without a GPU)
from oracle import oracle_py as orc

import gram_matvec_cases as mc


def host_matrix(cov, fs, y_var):
    K = orc.gram(cov, fs, None, x_meas=fs.is_measurement)
    return mc.system_matrix(K, y_var)


def test_slice_rule():
    assert mc.slices(1) == (1, 64) and mc.slices(mc.LARGEST_UNSPLIT) == (1, 256)
    assert mc.slices(mc.FIRST_SPLIT) == (2, 192)      # last slice: 65 columns
    assert mc.slices(513) == (3, 192) and mc.slices(777) == (4, 256)
    assert mc.slices(4096) == (16, 256) and mc.slices(65536) == (4, 16384) and mc.slices(262144) == (1, 262144)
    for n in list(range(1, 1200)) + [4095, 4096, 4097, 16384, 65536, 100000, 262144, 1 << 20]:
        S, cps = mc.slices(n)
        assert cps % mc.MV_COLS == 0 and (S - 1) * cps < n <= S * cps
        assert S == 1 or cps >= mc.MV_MIN_SLICE - mc.MV_COLS
    assert [mc.chunk_widths(r) for r in (1, 2, 3, 8, 17, 33)] == [[(1, 1)], [(4, 2)], [(4, 3)], [(16, 8)], [(16, 16), (1, 1)],
                                                                 [(16, 16), (16, 16), (1, 1)]]


@pytest.mark.parametrize("n", mc.SIZES)
def test_restatement_meets_the_bound(n):
    cov = mc.gp.fast_cov(0, "noise")
    fs = mc.make_features(cov, mc.points(n, 3, 11 + n), False, False)
    y_var = mc.variances(n, n)
    Am = host_matrix(cov, fs, y_var)
    worst = 0.
    for nrhs in mc.NRHS:
        V = mc.right_hand_sides(n, nrhs, 100 * n + nrhs)
        ok, frac = mc.within_bound(mc.restatement(Am, V), Am, V)
        assert ok, (n, nrhs, frac)
        worst = max(worst, frac)
    print(n, "worst fraction of the bound", worst)


@pytest.mark.parametrize("name,dim", mc.tree_cases())
def test_restatement_on_every_tree(name, dim):
    cov, _ = mc.tree(name)
    n = mc.PATH_N
    x = mc.points(n, dim, 7 * dim + len(name))
    for k, (meas, ids) in enumerate(mc.FEATURE_VARIANTS):
        fs = mc.make_features(cov, x, meas, ids)
        y_var = mc.variances(n, 3) if k % 2 == 0 else None
        Am = host_matrix(cov, fs, y_var)
        V = mc.right_hand_sides(n, mc.PATH_NRHS, 31 + k)
        ok, frac = mc.within_bound(mc.restatement(Am, V), Am, V)
        assert ok, (name, dim, meas, ids, frac)
        first = n - mc.PATH_NRHS
        got = mc.restatement(Am, mc.identity_block(n, first, mc.PATH_NRHS))
        assert np.array_equal(got, Am[:, first:first + mc.PATH_NRHS])
