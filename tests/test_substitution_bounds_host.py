"""The residual bound of tests/substitution_cases.py can be met: a plain fp64 restatement of every substitution path of
csrc/solve.hip (block rows of width b, explicit inverses of the diagonal blocks obtained by substitution, products in
numpy) stays at or below it on every matrix, shape and right-hand side that tests/test_substitutions_gpu.py and
test_forward_solve_wide (tests/test_kernels_gpu.py) give to the kernels.  So a correct kernel can pass those tests, and
the inputs are not ones on which the bound is out of reach.  No GPU."""
import numpy as np
import pytest

import substitution_cases as sc

CASES = sc.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restated_substitution_meets_bound(case):
    kind = case["kind"]
    b, transposed = sc.BLOCK_WIDTH[kind], kind in sc.TRANSPOSED
    worst = 0.0
    for p, K in enumerate(sc.case_matrices(case)):
        L = np.linalg.cholesky(K)
        B = sc.case_rhs(case, p)
        X = sc.blocked_substitution(L, B, b, transposed)
        worst = max(worst, sc.residual_ratio(L, X, B, b, transposed))
        if case["lower"]:  # a lower-triangular right-hand side has a lower-triangular solution
            assert np.all(X[np.triu_indices(X.shape[0], 1, X.shape[1])] == 0.0)
    print(f"{case['id']}: residual / bound {worst:.3g}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n,ncols", sc.WIDE_SHAPES)
def test_restated_wide_solve_meets_bound(n, ncols):
    """forward_solve_wide: b = 512, the matrix and right-hand side of test_forward_solve_wide."""
    K, B = sc.wide_problem(n, ncols)
    L = np.linalg.cholesky(K)
    X = sc.blocked_substitution(L, B, sc.WIDE_BW, False)
    ratio = sc.residual_ratio(L, X, B, sc.WIDE_BW, False)
    print(f"forward_solve_wide {n} x {ncols}: residual / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio


WIDE_SWEEPS = sc.wide_sweep_cases()


@pytest.mark.parametrize("case", WIDE_SWEEPS, ids=[c["id"] for c in WIDE_SWEEPS])
def test_restated_wide_sweep_meets_bound(case):
    """The wide vector sweeps and the two sweeps of the mixed fit's preconditioner (tests/test_reduce_kernels_gpu.py):
    b = 512 and 1024, against the fp64 factor and against the factor whose off-diagonal blocks are rounded to fp32; the
    backward sweep of the preconditioner starts from the forward sweep's result."""
    n, bw = case["n"], case["bw"]
    L = np.linalg.cholesky(sc.spd_matrix(case["family"], n))
    B = sc.wide_sweep_rhs(case)
    for T in (L, sc.fp32_off_diagonal(L, bw)):
        t2 = sc.blocked_substitution(T, B, bw, False)
        fwd = sc.residual_ratio(T, t2, B, bw, False)
        bwd = sc.residual_ratio(T, sc.blocked_substitution(T, B, bw, True), B, bw, True)
        pre = sc.residual_ratio(T, sc.blocked_substitution(T, t2, bw, True), t2, bw, True)
        print(f"wide sweeps {case['id']}: residual / bound forward {fwd:.3g}, backward {bwd:.3g}, preconditioner's backward {pre:.3g}")
        assert max(fwd, bwd, pre) <= 1.0, (fwd, bwd, pre)


@pytest.mark.parametrize("n,k0", sc.BACK_UPDATE_SHAPES)
def test_restated_back_update_meets_bound(n, k0):
    """back_update_kernel is a product, z -= L[k0 : k0 + nbk, : k0]^T x: its bound is that of a dot product of length
    nbk plus the subtraction, c (nbk + 1) u (|z| + |L|^T |x|)."""
    for fam in ("rand", "gram"):
        L = np.linalg.cholesky(sc.spd_matrix(fam, n))
        z, x = sc.back_update_vectors(n, k0)
        got = z - L[k0:k0 + sc.NB, :k0].T @ x
        ratio = sc.back_update_ratio(L, k0, z, x, got)
        assert ratio <= 1.0, ratio


def test_bound_is_not_slack_for_a_wrong_solve():
    """The bound refuses what the GPU tests are there to catch: one right-hand-side entry left unsolved, one update
    skipped, a solution column taken from the wrong problem."""
    n, m = 300, 40
    L = np.linalg.cholesky(sc.spd_matrix("gram", n))
    B = sc.rhs_matrix(n, m, 5)
    X = sc.blocked_substitution(L, B, sc.MB, False)
    assert sc.residual_ratio(L, X, B, sc.MB, False) <= 1.0
    bad = X.copy()
    bad[n - 1, m - 1] = B[n - 1, m - 1]  # last row of the last column not stored
    assert sc.residual_ratio(L, bad, B, sc.MB, False) > 1.0
    bad = X.copy()
    bad[200, 3] *= 1.0 + 1e-10
    assert sc.residual_ratio(L, bad, B, sc.MB, False) > 1.0
    L2 = np.linalg.cholesky(sc.spd_matrix("gram", n, 1))
    assert sc.residual_ratio(L2, X, B, sc.MB, False) > 1.0
