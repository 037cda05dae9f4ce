"""No GPU: the float64 restatement of the greedy pivoted Cholesky factorisation (tests/pivoted_chol_cases.py) meets every
bound of that module on the very inputs of tests/test_pivoted_chol_gpu.py, with K from the CPU restatement of the
covariance functions - so the bounds ask nothing of the kernel that plain double arithmetic in the defined order does
not give.  Worst fractions of the bounds measured over all cases (float64 restatement): pivot slack 0.063 (rows128),
pivot rows 0.27 (rank8), residual 0.15 and trace 0.16 (both rank1, where the bound is 4 u Kmax against one division
and one subtraction)."""
import numpy as np
import pytest

import albatross_amd as ab  # noqa: F401  (the package must import without a GPU)
from oracle import oracle_py as orc

import pivoted_chol_cases as pc


def host_gram(cov, xs, ys=None):
    return orc.gram(cov, xs, ys)


def run_restatement(name, dtype=np.float64):
    cov, x = pc.inputs(name)
    n, _, _, max_rank, rel_tol, _ = pc.CASES[name]
    if name in pc.BIG:
        kdiag, _, _ = pc.gram_parts(host_gram, name, [])
        kcol = lambda p: host_gram(cov, x, pc.subset(x, np.array([p])))[:, 0]  # noqa: E731
    else:
        K = host_gram(cov, x)
        kdiag, kcol = np.diag(K).copy(), (lambda p: K[:, p])
    return (kdiag,) + pc.restatement(kdiag, kcol, max_rank, rel_tol, dtype)


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_float64_restatement_meets_every_bound(name):
    n, _, _, max_rank, rel_tol, _ = pc.CASES[name]
    kdiag, pivots, rank, L, d, trace = run_restatement(name)
    _, krows, _ = pc.gram_parts(host_gram, name, pivots)
    worst = pc.check(kdiag, krows, max_rank, rel_tol, pivots, rank, L, d, float(trace))
    print(name, rank, worst)
    if name.startswith("duplicates"):
        assert rank == pc.DUPLICATE_RANK
        x = pc.coords_of(pc.inputs(name)[1])
        assert len({x[p].tobytes() for p in pivots}) == rank, "two copies of one point were selected"
    elif name == "early_stop":
        assert 0 < rank < max_rank  # (34 in this restatement; the stop RULE is what `check` asserts)
    elif name == "ties":
        assert pivots.tolist() == [0]
    else:
        assert rank == max_rank


@pytest.mark.parametrize("name", ["duplicates_exp", "duplicates_m32", "early_stop"])
def test_longdouble_restatement_agrees_on_the_rank(name):
    """where the stop rule decides, it decides with digits to spare: the longdouble run stops at the same rank as the
    float64 run on the duplicates (exactly 200: the smallest accepted pivot is ~7e-3, the largest rejected residual
    ~4e-16 against a threshold of 1e-12) and within one step of it on the early stop"""
    _, _, r64, _, _, _ = run_restatement(name)
    _, _, rld, _, dld, _ = run_restatement(name, np.longdouble)
    if name.startswith("duplicates"):
        assert r64 == rld == pc.DUPLICATE_RANK
    else:
        assert abs(r64 - rld) <= 1


def test_duplicates_margin():
    """the numbers behind the duplicates case: accepted pivots and rejected residuals are thirteen digits apart"""
    kdiag, pivots, rank, L, d, _ = run_restatement("duplicates_exp")
    accepted = np.array([L[p, j] ** 2 for j, p in enumerate(pivots)])
    assert accepted.min() > 1e-3 and d.max() < 1e-14


def test_free_running_pivots_are_not_comparable():
    """why no test compares pivots with a reference run: float64 and longdouble part ways within a few steps"""
    cov, x = pc.inputs("rows1000")
    K = host_gram(cov, x)
    a = pc.restatement(np.diag(K).copy(), lambda p: K[:, p], 40, 0., np.float64)[0]
    b = pc.restatement(np.diag(K).copy(), lambda p: K[:, p], 40, 0., np.longdouble)[0]
    assert a[0] == b[0] == 0  # the constant diagonal: the lowest index in both
    print("agreeing pivots:", int((a == b).sum()), "of 40")
