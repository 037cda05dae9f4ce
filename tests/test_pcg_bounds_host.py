"""The bounds of tests/pcg_kernel_cases.py can be met and are not slack: on every input that tests/test_pcg_kernels_gpu.py
gives to the kernels of csrc/iterative.hip a plain fp64 evaluation - in the kernel's summation order where there is a sum -
stays within the bound, and a result with its last element or its last block of 256 / 1024 dropped, a term counted twice
or a column taken from the neighbour does not.  So a correct kernel can pass the GPU tests and a subtly wrong one cannot.
The same for the whole preconditioner application, on preconditioners that the float64 restatement of
tests/iterative_fit_cases.py builds from the CPU restatement of the covariance functions; and the iteration counts that
the independence tests of the GPU file lean on have room.  No GPU."""
import numpy as np
import pytest

import albatross_amd as ab  # noqa: F401  (the package must import without a GPU)
from oracle import oracle_py as orc

import iterative_fit_cases as ic
import pcg_kernel_cases as kc


def test_longdouble_is_wider_than_double():
    assert kc.HAVE_LONGDOUBLE


def test_control_block_mirror():
    """the mirror of PcgCtrl: C's layout rules for ints and doubles (the GPU file asserts it against the library's)"""
    assert kc.CTRL.itemsize == 16 + 2 * 4 * kc.PCG_COLS + 6 * 8 * kc.PCG_COLS
    lay = kc.ctrl_layout()
    assert lay[1:5] == [0, 4, 8, 12] and lay[5] == 16 and lay[6] == 16 + 64 and lay[7] == 16 + 128
    assert lay[8] - lay[7] == 128 and lay[9] - lay[8] == 256 and lay[-1] == 1 << 20
    c, raw = kc.fresh_ctrl(kc.rng_of(1), 16, kc.ERROR_ACTIVE, stopped=(1, 15))
    assert int(c["active"][0]) == 3 - (1 << 20) and list(np.nonzero(c["stopped"][0])[0]) == [1, 15]
    assert np.all(raw[kc.CTRL.itemsize:] == 0xA5) and np.all(c["bb"] > 0)


def _check_sum(name, F0, F1, ref, bound, threads, final, worst):
    ratio = kc.error_ratio(kc.kernel_sum(F0, F1, threads, final), ref, bound)
    assert ratio <= 1.0, (name, ratio)
    return max(worst, ratio)


def _check_wrong(name, F0, F1, ref, bound, block):
    wrong = kc.wrong_sums(F0, F1, block)
    assert any("block" in what for what in wrong), name
    for what, got in wrong.items():
        ratio = kc.error_ratio(got, ref, bound)
        print(f"{name}: {what}: error / bound {ratio:.3g}")
        assert ratio > 1e3, (name, what, ratio)


@pytest.mark.parametrize("mode", range(4), ids=kc.DOT_NAMES)
def test_plain_dot_meets_the_bound(mode):
    worst = 0.0
    for case in kc.dot_cases():
        p = kc.dot_problem(mode, case)
        worst = _check_sum(case["id"], p["a"].T, p["b"].T, p["ref"], p["bound"], 1024, "waves_left", worst)
        if mode == kc.DOT_PQ:
            assert np.all(p["ref"] > 0)
    print(f"dot {kc.DOT_NAMES[mode]}: plain fp64 in the kernel's order, worst error / bound {worst:.3g}")


@pytest.mark.parametrize("mode", [kc.DOT_RZ, kc.DOT_RR], ids=["rz", "rr"])
def test_a_wrong_dot_exceeds_the_bound(mode):
    """(a sum of squares, DOT_RR, has no cancellation: the bound is relative to the result there, and still orders away)"""
    for n in (1025, 3000):
        p = kc.dot_problem(mode, dict(n=n, t=16))
        _check_wrong(f"dot {kc.DOT_NAMES[mode]} n{n}", p["a"].T, p["b"].T, p["ref"], p["bound"], 1024)


def test_derived_scalars_of_the_dot():
    """the tolerances of alpha and of the residual norm in plain fp64, and the stop cases' distance from the edge"""
    worst_a = worst_r = 0.0
    for case in kc.dot_cases():
        p = kc.dot_problem(kc.DOT_PQ, case)
        rz = kc.rng_of(case["n"], 3).standard_normal(case["t"])
        s = kc.kernel_sum(p["a"].T, p["b"].T, 1024, "waves_left")
        ref = rz.astype(kc.LD) / p["ref"]
        tol = (p["bound"] / np.abs(p["ref"]).astype(np.float64) + 2 * kc.U) * np.abs(ref).astype(np.float64)
        worst_a = max(worst_a, kc.error_ratio(rz / s, ref, tol))
        q = kc.dot_problem(kc.DOT_RR, case)
        bb = 1.7
        s = kc.kernel_sum(q["a"].T, q["a"].T, 1024, "waves_left")
        ref = np.sqrt(q["ref"] / kc.LD(bb))
        tol = (q["bound"] / (2 * q["ref"].astype(np.float64)) + 4 * kc.U) * ref.astype(np.float64)
        worst_r = max(worst_r, kc.error_ratio(np.sqrt(s) / np.sqrt(bb), ref, tol))
    assert worst_a <= 1.0 and worst_r <= 1.0
    print(f"alpha: worst error / tolerance {worst_a:.3g}; residual norm: {worst_r:.3g}")
    # a factor 2 on either side of tol ||b|| is orders of magnitude more than the error of s
    assert kc.gamma(kc.dot_counts(max(kc.DOT_N))) < 1e-3 * 0.5


def test_plain_lt_r_meets_the_bound():
    worst = 0.0
    for case in kc.lt_r_cases():
        p = kc.lt_r_problem(case)
        got = kc.kernel_sum(*kc.lt_r_canonical(p), 256, "waves_pairs").reshape(p["ref"].shape, order="F")
        ratio = kc.error_ratio(got, p["ref"], p["bound"])
        assert ratio <= 1.0, (case["id"], ratio)
        worst = max(worst, ratio)
    print(f"lt_r: plain fp64 in the kernel's order, worst error / bound {worst:.3g}")


def test_a_wrong_lt_r_exceeds_the_bound():
    p = kc.lt_r_problem(dict(n=1025, m=65, t=16))
    F0, F1 = kc.lt_r_canonical(p)
    _check_wrong("lt_r n1025-m65-t16", F0, F1, p["ref"].reshape(-1, order="F"), p["bound"].reshape(-1, order="F"), 256)
    # the right-hand side of the neighbour, and the column of L of the neighbour
    assert kc.error_ratio(p["L"].T @ np.roll(p["R"], 1, axis=1), p["ref"], p["bound"]) > 1e3
    assert kc.error_ratio(np.roll(p["L"], 1, axis=1).T @ p["R"], p["ref"], p["bound"]) > 1e3


def test_plain_precond_meets_the_bound_and_a_wrong_one_does_not():
    worst = 0.0
    for case in kc.precond_cases():
        p = kc.precond_problem(case)
        got = (p["R"] - p["L"] @ p["U"]) / p["delta"]
        ratio = kc.error_ratio(got, p["ref"], p["bound"])
        assert ratio <= 1.0, (case["id"], ratio)
        worst = max(worst, ratio)
        if case["m"] == 0:
            assert np.array_equal(got, p["R"] / p["delta"])
    print(f"precond: plain fp64 evaluation, worst error / bound {worst:.3g}")
    p = kc.precond_problem(dict(n=513, m=65, t=16))
    L, Um, R, d = p["L"], p["U"], p["R"], p["delta"]
    unwritten = (R - L @ Um) / d
    unwritten[512:] = np.nan  # the last block of 256 rows (one row here) never written
    wrong = {"last column of L dropped": (R - L[:, :-1] @ Um[:-1]) / d,
             "a term counted twice": (R - L @ Um - L[:, -1:] * Um[-1:]) / d,
             "U of the neighbouring right-hand side": (R - L @ np.roll(Um, 1, axis=1)) / d,
             "rows of U shifted by one": (R - L @ np.roll(Um, 1, axis=0)) / d,
             "last block of rows not written": unwritten}
    for what, got in wrong.items():
        ratio = kc.error_ratio(got, p["ref"], p["bound"])
        print(f"precond n513-m65-t16: {what}: error / bound {ratio:.3g}")
        assert ratio > 1e3, (what, ratio)


def test_plain_sweeps_meet_their_bounds():
    worst = 0.0
    for case in kc.sweep_cases():
        p = kc.sweep_problem(case)
        for x, a, v, sign in ((p["Z"], p["beta"], p["P"], 1.), (p["X"], p["alpha"], p["P"], 1.), (p["R"], p["alpha"], p["Q"], -1.)):
            ref, bound = kc.axpy_reference(x, sign * a, v)
            ratio = kc.error_ratio(x + (sign * a)[None, :] * v, ref, bound)
            assert ratio <= 1.0, (case["id"], ratio)
            worst = max(worst, ratio)
            if case["t"] > 1:  # the scalar of the neighbouring column
                assert kc.error_ratio(x + np.roll(sign * a, 1)[None, :] * v, ref, bound) > 1e3
            assert kc.error_ratio(x + (sign * a)[None, :] * v * (1. + 1e-12), ref, bound) > 1e2
    print(f"p / xr: plain fp64 evaluation, worst error / bound {worst:.3g}")


def test_plain_diag_stats_meet_the_bound_and_a_wrong_sum_does_not():
    worst = 0.0
    for case in kc.stats_cases():
        p = kc.stats_problem(case)
        assert p["v"][case["pmax"]] == p["max"] and (case["n"] == 1 or p["v"][case["pmin"]] == p["min"]) and p["min"] > 0
        assert np.sum(p["v"] == p["max"]) == 1 and np.sum(p["v"] == p["min"]) == 1
        got = kc.kernel_sum(p["v"][None, :], np.ones((1, case["n"])), 1024, "tree")
        ratio = kc.error_ratio(got, np.array([p["ref"]]), np.array([p["bound"]]))
        assert ratio <= 1.0, (case["id"], ratio)
        worst = max(worst, ratio)
    print(f"diag_stats: plain fp64 in the kernel's order, worst error / bound {worst:.3g}")
    p = kc.stats_problem(dict(n=3000, yvar=True, pmax=1024, pmin=2999))
    v = p["v"]
    for what, got in {"last element dropped": v[:-1].sum(), "last block of 1024 dropped": v[:2048].sum(),
                      "a term counted twice": v.sum() + v[-1], "yvar forgotten": p["d"].sum()}.items():
        ratio = kc.error_ratio(np.array([got]), np.array([p["ref"]]), np.array([p["bound"]]))
        print(f"diag_stats n3000: {what}: error / bound {ratio:.3g}")
        assert ratio > 1e3, (what, ratio)


def test_plain_variance_meets_the_bound_and_a_wrong_one_does_not():
    worst = 0.0
    for case in kc.variance_cases():
        p = kc.variance_problem(case)
        ratio = kc.error_ratio(p["prior"] - kc.kernel_sum(p["Kc"].T, p["S"].T, 256, "waves_pairs"), p["ref"], p["bound"])
        assert ratio <= 1.0, (case["id"], ratio)
        worst = max(worst, ratio)
    print(f"variance: plain fp64 in the kernel's order, worst error / bound {worst:.3g}")
    p = kc.variance_problem(dict(n=1025, t=16))
    for what, s in kc.wrong_sums(p["Kc"].T, p["S"].T, 256).items():
        ratio = kc.error_ratio(p["prior"] - s, p["ref"], p["bound"])
        print(f"variance n1025-t16: {what}: error / bound {ratio:.3g}")
        assert ratio > 1e3, (what, ratio)
    assert kc.error_ratio(np.roll(p["prior"], 1) - kc.plain_sum(p["Kc"].T, p["S"].T), p["ref"], p["bound"]) > 1e3


def test_shift_restated():
    for m in kc.SHIFT_M:
        p = kc.shift_problem(m)
        assert np.array_equal(np.diag(p["want"]), p["delta"] - np.diag(p["C"]))
        off = ~np.eye(m, dtype=bool)
        assert np.array_equal(p["want"][off], -p["C"][off])
        assert p["want"][0, 0] == p["delta"] and (m == 1 or not np.signbit(p["want"][1, 0]))  # delta - 0, and 0 - 0 = +0


# ---- the whole application ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_preconditioners():
    made = {}

    def get(case):
        key = case["id"]
        if key not in made:
            cov, x, y, y_var = ic.inputs(case["name"])
            A = ic.system(orc.gram(cov, x), y_var if case["with_var"] else None)
            P = ic.Preconditioner(A, case["rank"], kc.PRECOND_REL_TOL)
            made[key] = (A, P, kc.Application(P.L, P.delta))
        return made[key]
    return get


@pytest.mark.parametrize("case", kc.live_cases(), ids=lambda c: c["id"])
def test_plain_application_meets_the_bound(case, host_preconditioners):
    A, P, app = host_preconditioners(case)
    n, m = P.L.shape
    assert m == case["rank"] == P.rank
    ref, bound = kc.delta_reference(np.diag(A).copy(), P.L)
    assert abs(P.delta - ref) <= bound, (P.delta, ref, bound)
    for t in kc.LIVE_T:
        R = kc.live_rhs(n, t, m)
        Z, E = app.reference(R)
        ratio = kc.error_ratio(kc.plain_application(P.L, P.delta, R), Z, E)
        sharp = float(E.max() / np.abs(Z).max())
        print(f"{case['id']} t{t}: plain fp64 application, error / bound {ratio:.3g}; E / max|Z| {sharp:.3g}")
        assert ratio <= 1.0, (case["id"], t, ratio)
        assert sharp < (1e-3 if m == n else 1e-10), sharp  # (m = n: the formula's own cancellation - the module docstring)
    chol = np.linalg.cholesky(P.delta * np.eye(m) + P.L.T @ P.L)
    M, fb = app.factor_bound()
    assert kc.error_ratio(np.tril(chol @ chol.T), np.tril(M), np.tril(fb) + np.triu(np.ones((m, m)), 1)) <= 1.0


@pytest.mark.parametrize("name,rank", [("n777_2d", 1), ("n777_2d", 64), ("n65_3d", 64)])
def test_a_wrong_application_exceeds_the_bound(name, rank, host_preconditioners):
    """partial ranks: what a dropped row tile of pcg_lt_r_kernel, a missed tail of L^T L, a wrong ldt or a delta from the
    wrong trace would give.  The single row that is dropped or doubled is the largest of the last block of 256: at rank 1
    the one column of L is a bump around the first pivot and its very last row is zero to rounding - nothing to miss."""
    A, P, app = host_preconditioners(dict(id=f"{name}-rank{rank}-var", name=name, rank=rank, with_var=True))
    L, d = P.L, P.delta
    n, m = L.shape
    R = kc.live_rhs(n, 16, m)
    Z, E = app.reference(R)
    cut = (n - 1) // 256 * 256
    Mw = d * np.eye(m) + L[:cut].T @ L[:cut]
    i = cut + int(np.argmax(np.abs(L[cut:]).max(axis=1)))
    keep = np.arange(n) != i

    def apply(t1, M=None, delta=d):
        chol = np.linalg.cholesky(delta * np.eye(m) + L.T @ L if M is None else M)
        return (R - L @ np.linalg.solve(chol.T, np.linalg.solve(chol, t1))) / delta

    wrong = {"a row of the last block of L^T R dropped": apply(L[keep].T @ R[keep]),
             "last block of 256 rows of L^T R dropped": apply(L[:cut].T @ R[:cut]),
             "last block of rows missed by the GEMM of L^T L": apply(L.T @ R, Mw),
             "a term counted twice": apply(L.T @ R + np.outer(L[i], R[i])),
             "right-hand sides shifted by one in L^T R": apply(L.T @ np.roll(R, 1, axis=1)),
             "delta from the trace of A, not of A - L L^T": apply(L.T @ R, delta=np.diag(A).sum() / (n - m))}
    if m > 1:
        wrong["rows of u shifted by one"] = (R - L @ np.roll(np.linalg.solve(d * np.eye(m) + L.T @ L, L.T @ R), 1, axis=0)) / d
    for what, got in wrong.items():
        ratio = kc.error_ratio(got, Z, E)
        print(f"{name} rank {rank}: {what}: error / bound {ratio:.3g}")
        assert ratio > 1e3, (what, ratio)


# ---- the columns of a chunk -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", kc.INDEPENDENCE_RANKS)
def test_iteration_gaps_of_the_independence_inputs(rank):
    """The GPU test asserts, on the device's counts, that a neighbour stops at least 16 iterations before the column under
    test and another runs at least 16 longer.  In the float64 restatement the two gaps are at least 20, and every
    neighbour is on its side of the column under test by more than two looks of the host."""
    cov, x, y, y_var = ic.inputs(kc.INDEPENDENCE_FIT)
    A = ic.system(orc.gram(cov, x), y_var)
    vs = kc.independence_vectors(A, rank)

    def its(b):
        st, _, k, _, r = ic.pcg(A, b, rank, rel_tol=kc.PRECOND_REL_TOL)
        assert st == ic.OK and r == rank
        return k

    mid = its(vs["test"])
    early, late = [its(b) for b in vs["early"]], [its(b) for b in vs["late"]]
    print(f"rank {rank}: the column under test {mid} iterations, early neighbours {early}, late neighbours {late}")
    assert min(early) + kc.HOST_GAP <= mid <= max(late) - kc.HOST_GAP
    assert max(early) + kc.DEVICE_GAP < mid < min(late) - kc.DEVICE_GAP
    for c in kc.POSITIONS:
        for variant in (0, 1):
            B = kc.chunk_around(vs, c, variant)
            assert np.array_equal(B[:, c], vs["test"])
            others = [k for k in range(kc.PCG_COLS) if k != c]
            assert any(any(np.array_equal(B[:, k], e) for e in vs["early"]) for k in others)
            assert any(any(np.array_equal(B[:, k], e) for e in vs["late"]) for k in others)
        assert not np.array_equal(np.delete(kc.chunk_around(vs, c, 0), c, axis=1), np.delete(kc.chunk_around(vs, c, 1), c, axis=1))
