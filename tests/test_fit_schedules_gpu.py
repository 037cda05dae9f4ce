"""The fp64 factorisation and fit at the edges of their schedules (csrc/chol.hip: factor_lower, panel_phase; csrc/api.hip:
fit_create_impl), checked with componentwise backward-error bounds, and with the schedule record of the context
(agp_debug_schedule, csrc/debug_api.hip) proving which path each case took.

The factorisation is not one algorithm: the outer block width, the merged / throttled / CU-masked bulk updates, the step
launches, the fused and the two-launch panels and the single-stream end each switch on the number of REMAINING rows, and
the back substitution of a fit has four paths of its own.  Every size below is derived from the thresholds so that the
first outer steps fall on either side of one of them; `expected_schedule` (tests/fit_schedule_cases.py) restates the
branch conditions independently of the library and each case checks the record against it.  The library decides the
schedule in csrc/factor_plan.h; tests/test_fit_schedule_host.py compares that plan with the same restatement at every n
without a device, and this module stays the proof that what a real factorisation RAN is the plan.

Bounds (u = 2^-53, G = |L| |L|^T, c = 4):
  factor       |K - L L^T| <= c n u G elementwise (Higham, Thm 10.3: gamma_{n+1}, plus the check's own product)
  z = L^-1 y   |y - L z| <= c n u |L| |z| (backward error of the substitution, Thm 8.5)
  information  |K a - y| <= c n u G |a| (Thm 10.4: gamma_{3n+1}), + u |K| |a| for a fit (its K is recomputed by ctx.gram)
  log det      |ld - 2 sum log L_ii| <= 2 n u sum |log L_ii| + n u (the sum on the device), and against LAPACK's
               to first order |tr(K^-1 dK)| <= n ||K^-1||_2 ||dK||_2 <= c n^2 u kappa(K) n for both factors
None of them depends on the conditioning except the last, which states kappa from a rigorous upper bound.
Memory safety: the NaN padding rows of lda > n come back bit-identical, and so does the strict upper triangle outside
the 128 x 128 diagonal blocks (the diagonal tiles store their upper half: gemm_tiles.h guards only row < M, col < N).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from conftest import synthetic_3d
from fit_schedule_cases import (INV_EARLY, INV_LAST_STEP, INV_TAIL, MASKED, MERGED, NB, SCHED_HEADER, SCHED_STEPS, SINGLE, STEP,
                                THROTTLED, expected_schedule, step_fits)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CB = 4.0  # c of the bounds above
FULL_CHECK_MAX = 4700  # above: whole 128-row block rows only

# ---- the schedule record (csrc/debug_api.hip: agp_debug_schedule, which documents the layout) -----------------------
BS_NONE, BS_COOP_DIRECT, BS_COOP_FLAGS, BS_WIDE, BS_CHAIN = 0, 1, 2, 3, 4
_HEADER_FIELDS = ("n", "steps", "steps_dropped", "panels_step", "panels_fused", "panels_split", "backsub", "bs_done",
                  "inv", "handover_timeout", "demotions", "step_slots", "cus", "masked_stream", "step_below",
                  "panel_fused", "merge_above", "backsub_coop", "fp64_nbo")


def schedule(ctx):
    """The schedule record of a context (debug library): header fields by name, and `outer` = [(end column, bits)] of
    the outer steps of its last factorisation."""
    fn = capi.load_debug().agp_debug_schedule
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    w = np.zeros(SCHED_HEADER + 2 * SCHED_STEPS, np.int64)
    assert fn(ctx._h, C.c_void_p(w.ctypes.data), w.size) == 0
    rec = {name: int(w[i]) for i, name in enumerate(_HEADER_FIELDS)}
    rec["outer"] = [(int(w[SCHED_HEADER + 2 * i]), int(w[SCHED_HEADER + 2 * i + 1])) for i in range(rec["steps"])]
    return rec


def count_steps(rec, bit):
    return sum(1 for _, b in rec["outer"] if b & bit)


def check_schedule(rec, n):
    """The record shows the schedule factor_lower's conditions give for n, no hand-over timed out, no demotion."""
    assert rec["n"] == n and rec["steps_dropped"] == 0, rec
    assert rec["handover_timeout"] == 0 and rec["demotions"] == 0, rec
    outer, panels = expected_schedule(n, rec)
    assert rec["outer"] == outer, (rec, outer)
    assert (rec["panels_step"], rec["panels_fused"], rec["panels_split"]) == (panels["step"], panels["fused"],
                                                                                panels["split"]), (rec, panels)
    assert all(e % NB == 0 or e == n for e, _ in rec["outer"]), rec  # outer edges on panel edges


def require_step_fits(rec, rows):
    if rec["step_below"] > 0 and rows <= rec["step_below"] and not step_fits(rec, rows):
        pytest.skip(f"this device holds {rec['step_slots']} step-kernel workgroups, fewer than the "
                    f"{10 + rows // 64 + 64} a step launch over {rows} rows needs (chol.hip: step_fits)")


# ---- matrices -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def spd_matrix(kind, n):
    """(K, lambda_min lower bound, ||K||_inf).  'rand': B B^T / r + I like the factor tests (B n x r Gaussian; r = n + 5 up
    to FULL_CHECK_MAX, 512 above: a full-rank product there is minutes of host time); 'gram': SE Gram matrix of
    synthetic_3d points plus the noise that puts cond(K) near 1e6."""
    rng = np.random.default_rng(1000 + n)
    if kind == "rand":
        r = n + 5 if n <= FULL_CHECK_MAX else 512
        B = rng.standard_normal((n, r))
        K = B @ B.T
        K /= r
        K[np.diag_indices(n)] += 1.0
        lam_min = 1.0
    else:
        x, _ = synthetic_3d(n, 7 + n)
        sq = (x * x).sum(axis=1)
        K = x @ x.T
        K *= -2.0
        K += sq[:, None]
        K += sq[None, :]
        np.maximum(K, 0.0, out=K)
        K *= -1.0 / (2 * 1.5 ** 2)
        np.exp(K, out=K)
        v = rng.standard_normal(n)
        for _ in range(30):  # power iteration: lambda_max to a few digits
            v = K @ v
            v /= np.linalg.norm(v)
        lam_min = float(v @ (K @ v)) / 1e6  # cond(K) <= (lambda_max + s) / s ~ 1e6
        K[np.diag_indices(n)] += lam_min
    return K, lam_min, float(np.abs(K).sum(axis=1).max())


def check_block_rows(K, L, rows_from, rows_to):
    """max over the lower triangle of rows [rows_from, rows_to) of |K - L L^T| / (c n u G)."""
    n = K.shape[0]
    r1 = rows_to
    Lr = L[rows_from:r1, :r1]
    R = K[rows_from:r1, :r1] - Lr @ L[:r1, :r1].T
    G = np.abs(Lr) @ np.abs(L[:r1, :r1]).T
    low = np.arange(rows_from, r1)[:, None] >= np.arange(r1)[None, :]
    return float((np.abs(R)[low] / (CB * n * U * G[low])).max())


def factor_ratio(K, L, block_rows):
    n = K.shape[0]
    if n <= FULL_CHECK_MAX:
        return check_block_rows(K, L, 0, n)
    return max(check_block_rows(K, L, b * NB, min(n, b * NB + NB)) for b in sorted(block_rows))


def edge_block_rows(rec, n, seed):
    """Block rows that start or end an outer step of the record, the last (ragged) one, and 16 at random."""
    nblk = -(-n // NB)
    rows = {nblk - 1}
    for e, _ in rec["outer"]:
        for i in (e - 1, e):
            if 0 <= i < n:
                rows.add(i // NB)
    rows.update(np.random.default_rng(seed).choice(nblk, size=min(16, nblk), replace=False).tolist())
    return rows


def debug_factor(ctx, K, y):
    """agp_debug_factor with lda > n: NaN padding rows, a pattern in the strict upper triangle."""
    n = K.shape[0]
    lib = capi.load_debug()
    lib.agp_debug_factor.restype = C.c_int
    lib.agp_debug_factor.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_double),
                                     C.POINTER(C.c_int64)]
    lda = n + 3
    Ad = np.full((lda, n), np.nan, order="F")
    Ad[:n] = K
    for c0 in range(0, n, NB):  # (column block by column block: index arrays of the whole triangle are GBs at n = 12289)
        c1 = min(n, c0 + NB)
        Ad[:c0, c0:c1] = 7.5
        Ad[c0:c1, c0:c1][np.triu_indices(c1 - c0, 1)] = 7.5
    yd = y.copy()
    logdet, bad = C.c_double(), C.c_int64()
    assert lib.agp_debug_factor(ctx._h, C.c_void_p(Ad.ctypes.data), n, lda, C.c_void_p(yd.ctypes.data), C.byref(logdet),
                                C.byref(bad)) == 0
    assert bad.value == -1
    # padding rows bit-identical; strict upper triangle outside the diagonal 128 x 128 blocks unchanged
    assert np.all(np.ascontiguousarray(Ad[n:]).view(np.uint64) == np.array(np.nan).view(np.uint64))
    assert all(np.all(Ad[:c0, c0:c0 + NB] == 7.5) for c0 in range(NB, n, NB))
    L = np.tril(Ad[:n])
    return L, yd, logdet.value


def check_logdet(ld, L, n, kappa, ld_ref):
    dg = np.log(np.diag(L))
    assert abs(ld - 2 * dg.sum()) <= 2 * n * U * np.abs(dg).sum() + n * U * 2 * np.abs(dg).sum() + 1e-300
    # both factors are exact for K + dK with |dK| <= c n u G, ||G||_2 <= n ||K||_2
    assert abs(ld - ld_ref) <= 2 * CB * n * U * n * kappa, (ld, ld_ref)


def reference_logdet(K):
    s, ld = np.linalg.slogdet(K) if K.shape[0] <= FULL_CHECK_MAX else (1.0, 2 * np.log(np.diag(np.linalg.cholesky(K))).sum())
    assert s > 0
    return ld


# ---- factor cases -------------------------------------------------------------------------------------------------
# (n, switches, intent): `intent` names what the case is there for, checked on the record besides the full schedule.
FACTOR_CASES = [
    # SINGLE_BELOW = 1536: n = 1792 ends with exactly 1536 rows after its first 256-wide block, 1793 with 1537
    (1792, {}, "all_step"), (1793, {}, "all_step"),
    (1792, {"AGP_STEP_BELOW": "0"}, "single_after_first"), (1793, {"AGP_STEP_BELOW": "0"}, "single_after_second"),
    # pick_nbo: 512-wide first block above 2048 rows (all step launches by default)
    (2049, {}, "all_step"),
    # AGP_STEP_BELOW = 4608 (and FUSED_BELOW): every panel a step launch at 4608; at 4609 a first 512 block of
    # POTRF + TRSM panels, then the step tail over 4097 rows
    (4608, {}, "all_step"), (4609, {}, "step_tail"),
    (4609, {"AGP_STEP_BELOW": "0", "AGP_PANEL_FUSED": "0"}, "two_launch"),
    # INNER_LEFT_ABOVE = 6144: the first block of 6145 is left-looking (6145 > 6144 rows from its start)
    (6145, {}, "step_tail"),
    # THROTTLE_BELOW = 8192: 8704 - 512 = 8192 rows after the first step (throttled), 8705 - 512 = 8193 (not)
    (8704, {}, "first_throttled"), (8705, {}, "first_not_throttled"),
    # MASK_BELOW / AGP_MERGE_ABOVE = 8704: 9216 leaves exactly 8704 (masked, not merged), 9217 leaves 8705 (merged)
    (9216, {}, "no_merged"), (9217, {}, "one_merged"),
    (9217, {"AGP_STEP_BELOW": "0", "AGP_PANEL_FUSED": "0"}, "two_launch"),
    (9217, {"AGP_MERGE_ABOVE": "0"}, "no_merged"),
    (9217, {"AGP_FP64_NBO": "700"}, "one_merged"),  # not a multiple of 128: ignored
    (12289, {}, "seven_merged"), (12289, {"AGP_MERGE_ABOVE": "0"}, "no_merged"),
    (12289, {"AGP_FP64_NBO": "1024"}, "merged_1024"),
]


def _case_id(c):
    (n, sw, _), kind = c
    return f"{n}-{kind}-" + ("default" if not sw else "-".join(f"{k[4:].lower()}{v}" for k, v in sw.items()))


# both matrices for the default switches; the switched cases above FULL_CHECK_MAX on the Gram matrix only (host time)
# (ordered by matrix, so that the cases of one matrix run one after the other: spd_matrix keeps the last one)
FACTOR_RUNS = sorted([(c, kind) for c in FACTOR_CASES for kind in ("rand", "gram") if kind == "gram" or not c[1] or c[0] <= FULL_CHECK_MAX],
                     key=lambda r: (r[1], r[0][0]))


def check_intent(rec, n, intent):
    steps = rec["outer"]
    if intent == "all_step":
        assert steps == [(n, STEP)], rec
    elif intent == "single_after_first":
        assert len(steps) == 2 and steps[1][1] & SINGLE, rec
    elif intent == "single_after_second":
        assert len(steps) == 3 and steps[2][1] & SINGLE and not steps[1][1] & SINGLE, rec
    elif intent == "step_tail":
        assert steps[-1][1] & STEP and rec["panels_step"] > 0 and rec["panels_split"] > 0, rec
    elif intent == "two_launch":
        assert rec["panels_step"] == 0 and rec["panels_fused"] == 0 and count_steps(rec, MERGED | STEP) == 0, rec
    elif intent == "first_throttled":
        assert steps[1][1] & THROTTLED and count_steps(rec, MERGED) == 0, rec
    elif intent == "first_not_throttled":
        assert not steps[1][1] & THROTTLED and steps[2][1] & THROTTLED and count_steps(rec, MERGED) == 0, rec
    elif intent == "no_merged":
        assert count_steps(rec, MERGED) == 0, rec
    elif intent == "one_merged":
        assert count_steps(rec, MERGED) == 1 and steps[1][1] == MERGED, rec
    elif intent == "seven_merged":
        assert count_steps(rec, MERGED) == 7, rec
    elif intent == "merged_1024":
        assert count_steps(rec, MERGED) == 3 and [e for e, _ in steps[:4]] == [1024, 2048, 3072, 4096], rec
    if rec["masked_stream"] and n > 8704 and intent != "two_launch":
        assert count_steps(rec, MASKED) > 0, rec


@pytest.mark.parametrize("run", FACTOR_RUNS, ids=_case_id)
def test_factor_schedule_edges(make_ctx, monkeypatch, run):
    (n, switches, intent), kind = run
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    ctx = make_ctx()
    K, lam_min, norm_inf = spd_matrix(kind, n)
    y = np.random.default_rng(n + 1).standard_normal(n)
    L, z, ld = debug_factor(ctx, K, y)
    rec = schedule(ctx)
    if rec["step_below"] > 0 and rec["panel_fused"] == 1:
        require_step_fits(rec, min(n, rec["step_below"]))
    if "AGP_FP64_NBO" in switches:
        assert rec["fp64_nbo"] == (int(switches["AGP_FP64_NBO"]) if int(switches["AGP_FP64_NBO"]) % NB == 0 else 0)
    check_schedule(rec, n)
    check_intent(rec, n, intent)
    ratio = factor_ratio(K, L, edge_block_rows(rec, n, n))
    rz = float((np.abs(y - L @ z) / (CB * n * U * (np.abs(L) @ np.abs(z)))).max())
    kappa = norm_inf / lam_min
    check_logdet(ld, L, n, kappa, reference_logdet(K))
    print(f"n={n} {kind} {switches}: factor error / bound {ratio:.3g}, z residual / bound {rz:.3g}")
    assert ratio <= 1.0, ratio
    assert rz <= 1.0, rz


# ---- fit cases ----------------------------------------------------------------------------------------------------
COVS = {
    "se": lambda: ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1),
    "matern": lambda: ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1),
}
# (n, switches, back substitution, wide inverses computed under the factorisation: (bs_done, inversion bits))
FIT_CASES = [
    (1000, {}, BS_COOP_DIRECT, (0, 0)), (2047, {}, BS_COOP_DIRECT, (0, 0)),  # <= 16 blocks: the output as hand-over
    (2048, {}, BS_WIDE, (3, INV_EARLY)),            # all step launches: early inversion of the first three 512 blocks
    (2049, {}, BS_CHAIN, (0, 0)),
    (4608, {}, BS_WIDE, (8, INV_EARLY)),
    (5120, {}, BS_WIDE, (9, INV_LAST_STEP | INV_TAIL)),  # one block at the last outer step, the rest under the step tail
    (9216, {}, BS_WIDE, (17, INV_LAST_STEP | INV_TAIL)),
    (12289, {}, BS_CHAIN, (0, 0)),
    (1000, {"AGP_BACKSUB_COOP": "0"}, BS_CHAIN, (0, 0)), (2047, {"AGP_BACKSUB_COOP": "0"}, BS_CHAIN, (0, 0)),
    (3000, {"AGP_BACKSUB_COOP_MAX": "4096"}, BS_COOP_FLAGS, (0, 0)),  # > 16 blocks: per-block flags
    (4096, {"AGP_BACKSUB_COOP_MAX": "4096"}, BS_COOP_FLAGS, (0, 0)),
]


def _fit_id(c):
    (n, sw, _, _), cov = c
    return f"{n}-{cov}-" + ("default" if not sw else "-".join(f"{k[4:].lower()}{v}" for k, v in sw.items()))


# both covariances for the default switches, SE for the switched cases
FIT_RUNS = [(c, cov) for c in FIT_CASES for cov in sorted(COVS) if cov == "se" or not c[1]]


@pytest.mark.parametrize("run", FIT_RUNS, ids=_fit_id)
def test_fit_schedule_edges(make_ctx, monkeypatch, run):
    (n, switches, backsub, (bs_done, inv)), cov = run
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    ctx = make_ctx()
    x, y = synthetic_3d(n, 300 + n)
    cf = COVS[cov]()
    fit = ab.gp_from_covariance(cf, context=ctx).fit(ab.RegressionDataset(x, y)).get_fit()
    rec = schedule(ctx)
    require_step_fits(rec, min(n, rec["step_below"]))
    check_schedule(rec, n)
    assert rec["backsub"] == backsub, rec
    assert (rec["bs_done"], rec["inv"]) == (bs_done, inv), rec
    a = np.array(fit.information)
    L = np.tril(fit.factor())
    K = ctx.gram(cf, ab.Measurement(x))
    Ga = np.abs(L) @ (np.abs(L).T @ np.abs(a))
    bound = CB * n * U * Ga + U * (np.abs(K) @ np.abs(a))
    ratio = float((np.abs(K @ a - y) / bound).max())
    # the factor of the fit itself, on the block rows at the edges of its outer steps
    fratio = factor_ratio(K, L, edge_block_rows(rec, n, n))
    print(f"fit n={n} {cov} {switches}: information residual / bound {ratio:.3g}, factor error / bound {fratio:.3g}")
    assert ratio <= 1.0, ratio
    assert fratio <= 1.0, fratio
    dg = np.log(np.diag(L))
    assert abs(fit.log_determinant - 2 * dg.sum()) <= 4 * n * U * np.abs(dg).sum()


# (n of the fp64 fit, n of the mixed fits, back substitution and (bs_done, inversion bits) of the fp64 fit)
# 2304 is not a multiple of 512: its substitution runs the 128-row chain and no wide block is inverted anywhere.  5120 is
# the FIT_CASES size whose fit asks for the early inversion AND has a bulk update (the hand-over to its step tail), which a
# low-precision variant left behind by a mixed fit would run on the fp32 products; 4736 is the smallest mixed fit with a
# split-plane update on every device (4608: all step launches where the device holds them).
SEQUENCE_CASES = [(2304, 4608, BS_CHAIN, (0, 0)),
                  (5120, 4736) + next((c[2], c[3]) for c in FIT_CASES if c[0] == 5120 and not c[1])]


@pytest.mark.parametrize("n,n_mixed,backsub,inverted", SEQUENCE_CASES, ids=["2304-4608", "5120-4736"])
def test_nothing_of_a_factorisation_survives_into_the_next(make_ctx, n, n_mixed, backsub, inverted):
    """Four fits in sequence on ONE context: (a) an fp64 fit, (b) a mixed fit, (c) a mixed fit that fails with
    AGP_ERR_NOT_POSITIVE_DEFINITE (the construction of test_mixed_fit_reports_failures), (d) the fit of (a) again.  What a
    fit asks of its factorisation - the low-precision bulk update, the wide outer blocks, the early inversion of the wide
    diagonal blocks - is an argument of that call (factor_plan.h: FactorRequest), so (d) returns the factor, information
    vector and log-determinant of (a) bit for bit and leaves the same schedule record."""
    ctx = make_ctx()
    cov = COVS["se"]()
    x, y = synthetic_3d(n, 300 + n)

    def fp64_fit():
        fit = ab.gp_from_covariance(cov, context=ctx).fit(ab.RegressionDataset(x, y)).get_fit()
        rec = schedule(ctx)
        return np.tril(fit.factor()), np.array(fit.information), fit.log_determinant, rec

    La, aa, lda, rec_a = fp64_fit()
    require_step_fits(rec_a, min(n, rec_a["step_below"]))
    check_schedule(rec_a, n)
    assert rec_a["backsub"] == backsub and (rec_a["bs_done"], rec_a["inv"]) == inverted, rec_a

    xm, ym = synthetic_3d(n_mixed, 300 + n_mixed)
    mixed = ab.gp_from_covariance(cov, context=ctx)
    mixed.precision = "mixed"
    mixed.fit(ab.RegressionDataset(xm, ym))
    xm[17] = xm[3]  # duplicate point and no noise: singular
    failing = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0), context=ctx)
    failing.precision = "mixed"
    failing.pivoted_fallback = False
    with pytest.raises(ab.NotPositiveDefiniteError):
        failing.fit(ab.RegressionDataset(xm, ym))

    Ld, ad, ldd, rec_d = fp64_fit()
    assert np.array_equal(La, Ld)
    assert np.array_equal(aa, ad)
    assert lda == ldd
    assert rec_d == rec_a, (rec_a, rec_d)
