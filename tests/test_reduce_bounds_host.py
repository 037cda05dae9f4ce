"""The bounds of tests/reduce_cases.py can be met and are not slack: on every input that tests/test_reduce_kernels_gpu.py
gives to the reductions of csrc/reduce.hip a plain fp64 evaluation - numpy's own summation, and term after term from the
left - stays within the bound, and a result with its last term dropped, a term counted twice or a column taken from the
neighbour does not.  So a correct kernel can pass the GPU tests and a subtly wrong one cannot.  No GPU."""
import numpy as np
import pytest

import reduce_cases as rc

REDUCTIONS = rc.reduction_cases()
KERNELS = sorted({c["kernel"] for c in REDUCTIONS})
CONTRACTS = rc.contract_cases()


@pytest.mark.parametrize("kernel", KERNELS)
def test_plain_evaluation_meets_the_reduction_bound(kernel):
    worst = 0.0
    for case in [c for c in REDUCTIONS if c["kernel"] == kernel]:
        p = rc.reduction_problem(case)
        ref, bound = rc.canonical_bound(p)
        for plain in (rc.plain_dot, rc.plain_loop):
            got = plain(p["F"], p["alpha"], p["beta"], p["base"])
            ratio = rc.error_ratio(np.asarray(got, dtype=np.float64) + np.zeros(len(bound)), ref, bound)
            assert ratio <= 1.0, (case["id"], plain.__name__, ratio)
            worst = max(worst, ratio)
    print(f"{kernel}: plain fp64 evaluations, worst error / bound {worst:.3g}")


def wrong_results(p):
    """The three results the GPU tests are there to refuse, from the canonical form of a case with at least two terms."""
    F0, F1 = p["F"][0], np.array(p["F"][1])
    args = (p["alpha"], p["beta"], p["base"])
    last = p["alpha"] * F0[:, -1] * F1[:, -1]
    return {"last term dropped": rc.plain_dot([F0[:, :-1], F1[:, :-1]], *args),
            "a term counted twice": rc.plain_dot([F0, F1], *args) + last,
            "column shifted by one": rc.plain_dot([np.roll(F0, 1, axis=1), F1], *args)}


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_wrong_reduction_exceeds_the_bound(kernel):
    """One case per kernel family with more than one term and, where there are several, more terms than a workgroup's
    stride - the wrong results miss the bound by orders of magnitude, not by a rounding."""
    cases = [c for c in REDUCTIONS if c["kernel"] == kernel]
    case = max(cases, key=lambda c: rc.reduction_problem(c)["F"][0].shape[1])
    p = rc.reduction_problem(case)
    assert p["F"][0].shape[1] >= 2
    ref, bound = rc.canonical_bound(p)
    for what, got in wrong_results(p).items():
        ratio = rc.error_ratio(got, ref, bound)
        print(f"{case['id']}: {what}: error / bound {ratio:.3g}")
        assert ratio > 1e3, (case["id"], what, ratio)


def test_plain_contraction_meets_its_bound():
    """contract_combinations: numpy's xc . (K yc) and the kernel's two nested loops in plain fp64."""
    def nested(ca, Kab, cb):
        acc = 0.0
        for i in range(len(ca)):
            t = 0.0
            for j in range(len(cb)):
                t += Kab[i, j] * cb[j]
            acc += ca[i] * t
        return acc

    worst = 0.0
    for case in CONTRACTS:
        p = rc.contract_problem(case)
        for evaluate in (lambda ca, Kab, cb: float(ca @ (Kab @ cb)) if Kab.size else 0.0, nested):
            ref, bound, plain = rc.contract_reference(case, p, evaluate)
            ratio = rc.error_ratio(plain.reshape(-1), ref.reshape(-1), bound.reshape(-1))
            assert ratio <= 1.0, (case["id"], ratio)
            worst = max(worst, ratio)
    print(f"contract_combinations: plain fp64 evaluations, worst error / bound {worst:.3g}")


def test_a_wrong_contraction_exceeds_the_bound():
    """A member dropped from the inner sum, one counted twice, and the coefficients of the neighbouring combination."""
    case = next(c for c in CONTRACTS if c["offsets"] and c["coefficients"] and not c["symmetric"] and c["na"] == 33 and c["nb"] >= 16)
    p = rc.contract_problem(case)
    wrong = {"last member dropped": lambda ca, Kab, cb: float(ca @ (Kab[:, :-1] @ cb[:-1])) if Kab.size else 0.0,
             "a member counted twice": lambda ca, Kab, cb: float(ca @ (Kab @ cb) + ca[-1] * Kab[-1, -1] * cb[-1]) if Kab.size else 0.0,
             "coefficients shifted by one": lambda ca, Kab, cb: float(np.roll(ca, 1) @ (Kab @ cb)) if Kab.size else 0.0}
    for what, evaluate in wrong.items():
        ref, bound, plain = rc.contract_reference(case, p, evaluate)
        ratio = rc.error_ratio(plain.reshape(-1), ref.reshape(-1), bound.reshape(-1))
        print(f"{case['id']}: {what}: error / bound {ratio:.3g}")
        assert ratio > 1e3, (what, ratio)


@pytest.mark.parametrize("n", rc.COLUMN_ROWS)
def test_plain_loo_and_axpby_meet_their_bounds(n):
    p = rc.loo_problem(n)
    (mean_ref, mean_bound), (var_ref, var_bound) = rc.loo_reference(p)
    assert rc.error_ratio(p["y"] - p["info"] / p["d"], mean_ref, mean_bound) <= 1.0
    assert rc.error_ratio(1.0 / p["d"], var_ref, var_bound) <= 1.0
    assert rc.error_ratio(p["y"] - p["info"] / np.roll(p["d"], 1), mean_ref, mean_bound) > 1e3 or n == 1  # the neighbour's d
    for mode in ("both", "x_null", "y_null"):
        q = rc.axpby_problem(n, mode)
        ref, bound = rc.axpby_reference(q, n)
        ax = q["a"] * q["x"] if q["x"] is not None else 0.0
        by = q["b"] * (q["y"] if q["y"] is not None else 1.0)
        assert rc.error_ratio(ax + by + np.zeros(n), ref, bound) <= 1.0
        assert rc.error_ratio(ax + by * (1.0 + 1e-12) + np.zeros(n), ref, bound) > 1e3


def test_movers_restated():
    """The helpers the bit-exact GPU tests lean on: the leading dimension of a factor, the entries the pair kernels may
    write, the places a NaN is put."""
    assert [rc.factor_ld(n) for n in (1, 8, 9, 511, 512, 513, 2048, 2049)] == [8, 8, 16, 520, 520, 520, 2056, 2056]
    mask = rc.pair_written_mask(5)
    assert mask.sum() == 15 + 2 and mask[0, 1] and mask[2, 3] and not mask[1, 2] and not mask[0, 2]
    for n in (2, 3, 513, 2049, 2050):
        pos = rc.nan_positions(n)
        assert all(r >= c for r, c, _ in pos), "a flag is expected only on and below the diagonal"
        assert (n - 1, 0) in [(r, c) for r, c, _ in pos] and (n - 1, n - 1) in [(r, c) for r, c, _ in pos]
        if n > 2048:
            assert (2048, 2048) in [(r, c) for r, c, _ in pos]
    assert any("scalar tail" in what for _, _, what in rc.nan_positions(2049))
    off = rc.group_offsets(8)
    assert list(np.diff(off)) == [8, 1, 0, 7]
