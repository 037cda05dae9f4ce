"""No GPU: the float64 numpy restatement of the matrix-free fit (tests/iterative_fit_cases.py: Preconditioner, pcg) meets, on
the inputs of tests/test_iterative_fit_gpu.py and with K from the CPU restatement of the covariance functions, every
condition that file asserts of the library - so they ask nothing that the definition in plain double arithmetic does not
give."""
import numpy as np
import pytest

import albatross_amd as ab  # noqa: F401  (the package must import without a GPU)
from oracle import oracle_py as orc

import iterative_fit_cases as ic


def host_system(name, with_var):
    cov, x, y, y_var = ic.inputs(name)
    return ic.system(orc.gram(cov, x), y_var if with_var else None), y


@pytest.mark.parametrize("name", sorted(ic.CASES))
def test_restatement_against_the_dense_solve(name):
    n = ic.CASES[name][0]
    for with_var in (False, True):
        A, y = host_system(name, with_var)
        dense = np.linalg.solve(A, y)
        for r in ic.RANKS:
            st, a, its, res, rank = ic.pcg(A, y, ic.rank_of(r, n))
            assert st == ic.OK and res <= ic.TOL and rank == ic.rank_of(r, n)
            worst = ic.check_information(A, a, dense, y)
            if r == "n":
                assert its <= 6, its
            print(name, "y_var" if with_var else "no y_var", "rank", rank, "iterations", its, worst)


def test_preconditioner_halves_the_iterations():
    A, y = host_system(ic.ONE_D, False)
    it0, it64 = ic.pcg(A, y, 0)[2], ic.pcg(A, y, 64)[2]
    print("iterations: rank 0", it0, "rank 64", it64)
    assert 2 * it64 < it0


def test_duplicates_stop_the_preconditioner_early():
    A, y = host_system("duplicates", True)
    st, a, its, res, rank = ic.pcg(A, y, ic.DUPLICATE_RANK_ASKED, rel_tol=ic.DUPLICATE_REL_TOL)
    assert st == ic.OK and 0 < rank <= ic.DUPLICATE_DISTINCT < ic.DUPLICATE_RANK_ASKED
    ic.check_information(A, a, np.linalg.solve(A, y), y)
    print("duplicates: rank", rank, "iterations", its)


def test_iteration_count_is_the_first_that_meets_the_criterion():
    A, y = host_system("n777_2d", True)
    st, a, its, res, _ = ic.pcg(A, y, 64)
    assert st == ic.OK and res <= ic.TOL
    st2, _, its2, res2, _ = ic.pcg(A, y, 64, max_iterations=its - 1)
    assert st2 == ic.NOT_CONVERGED and its2 == its - 1 and res2 > ic.TOL


def test_solve_columns_and_zero_column():
    A, _ = host_system("n777_2d", True)
    B = np.random.default_rng(3).standard_normal((777, 3))
    B[:, 1] = 0.
    for c in range(3):
        st, x, its, res, _ = ic.pcg(A, B[:, c], 64)
        assert st == ic.OK
        if c == 1:
            assert its == 0 and not x.any()
        else:
            assert np.abs(x - np.linalg.solve(A, B[:, c])).max() <= ic.PARITY * np.abs(np.linalg.solve(A, B[:, c])).max()


def test_status_codes():
    cov, x, y, _ = ic.inputs(ic.ONE_D)
    K = orc.gram(cov, x)
    st, _, its, res, _ = ic.pcg(K, y, 0, max_iterations=3)
    assert st == ic.NOT_CONVERGED and its == 3 and np.isfinite(res) and res > ic.TOL
    n = 777
    x7 = x[:n]
    K7 = orc.gram(cov, x7)
    indefinite = ic.system(K7, np.full(n, -0.5))
    assert np.diag(indefinite).min() > 0.
    for rank in (0, 16):
        st, _, its, _, _ = ic.pcg(indefinite, y[:n], rank)
        assert st == ic.NOT_POSITIVE_DEFINITE, (rank, st)
        print("indefinite: rank", rank, "detected at iteration", its)
    st, _, its, _, _ = ic.pcg(ic.system(K7, np.full(n, -5.)), y[:n], 0)
    assert st == ic.NOT_POSITIVE_DEFINITE and its == 0
    bad = y[:n].copy()
    bad[5] = np.nan
    assert ic.pcg(K7, bad, 0)[0] == ic.NAN_INPUT
