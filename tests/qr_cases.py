"""Shared by tests/test_qr_bounds_host.py and tests/test_qr_gpu.py: the shapes, inputs, bounds and the numpy restatement
of the column-pivoted Householder QR of csrc/qr.hip and of the substitutions against its R factor.

The restatement (colpiv_qr, back_solve, sqrt_solve below) is the algorithm of oracle/oracle.c's colpiv_qr, qr_solve and
qr_sqrt_solve in numpy, parameterised by dtype: the squared column norms are recomputed over rows k and below at every
step, the FIRST index of the largest one is the pivot, the reflector is makeHouseholderInPlace with its
`tail <= DBL_MIN` branch (tau = 0, essential part zeroed), nonzero_pivots is the first step whose largest squared norm
falls below threshold_helper * (rows - k), rank counts |R_kk| > maxpivot * eps * steps.  It runs in np.longdouble as the
reference and in float64 to show (tests/test_qr_bounds_host.py) that a plain double implementation meets every bound on
these very inputs.  Where the longdouble run would take many seconds (rows * cols^2 > LONGDOUBLE_WORK: 1040 x 1030 and
the 1030-wide back_solve input) the float64 run is the reference and the bounds that compare against it are doubled;
the backward error of that case is then formed in float64 too, against the doubled bound.

Inputs.  G (rows x cols, Gaussian) with its columns scaled by a shuffled np.geomspace(0.1, 10, cols): every step has a
clear winner, and the winner is rarely the column already in place.  With extra = 1 a Gaussian y rides along.
Special cases: `zeros` ([T; 0], T 20 x 50, 80 rows: exact rank 20, all-zero norms from step 20 on), `zerocol` (one
exactly zero column), `tie` (90 x 70, column 40 a bitwise copy of column 2, both of the largest norm), `lowrank`
(G (200 x 37) H (37 x 90)).

Conditions on the inputs (asserted by the host test, so that a reseeded or resized case cannot lose them unnoticed):
  * pivot gap: in the reference run the relative gap (largest - second) / largest of the remaining squared norms is at
    least PIVOT_GAP = 1e-8 at every determined step, or exactly 0 between bitwise equal columns (the tie and the
    all-zero remainders, where the first index wins).  1e-8 is ~1e8 u: no rounding of a sum of squares closes it.
    Smallest measured: 3.4e-06 (257x257) and 3.7e-06 (1040x1030); the float64 and reference pivots agree on every
    case.  A case that misses the condition gets another seed (SEEDS).
  * determined steps: every step, except for `tie` (69 of 70: after the first step the copy of the pivot column is
    rounding noise, so the last reflector is arbitrary) and `lowrank` (37 of 90).  Pivots, rows of R and of Q^T y are
    compared on the determined steps only; the rows of R below them must be small (forward bound).
  * rank margin: in both runs no |R_kk| lies within a factor RANK_MARGIN = 4 of maxpivot * eps * steps.  Smallest
    measured: 27 (lowrank), 146 (tie); exact zeros count as infinitely far.
  * nonzero_pivots: state[2] is compared where both runs agree on it and every decisive comparison
    best_sq < threshold_helper * (rows - k) has a factor NP_MARGIN = 16 (4 in the norm) to spare: every case (smallest
    margin 82, lowrank, whose count is 90: its noise columns stay above that threshold) except `tie`, where the noise
    column trips the threshold in longdouble (69) and not in double (70).

Bounds.  u = 2^-53, eps = 2 u, c = CB = 4 as in tests/substitution_cases.py.  None depends on the conditioning of the
matrix or on what the kernels were seen to give.  "Restatement" is the float64 run of this module on these inputs.
  * threshold helper, state[0] = (max_j ||a_j|| eps / rows)^2: a sum of `rows` squares carries a relative error of at
    most rows u in any order, which the root halves and the square doubles; c rows u relative.  Restatement: at most
    0.084 of it.
  * reflectors: tau_k v_k^T v_k = 2 for v_k = [1; essential] when tau_k != 0; |tau_k v_k^T v_k - 2| <= c len u with
    len = rows - k covers the rounding of tail (a sum of len squares), of beta, of the division and of tau.
    Restatement: at most 0.21 of it (257x257).
  * backward error (Higham, Accuracy and Stability of Numerical Algorithms, Thm 19.4: A + dA = Q R with
    ||da_j|| <= gamma~_{steps rows} ||a_j||): with Q the product of the RETURNED reflectors, formed in longdouble, every
    column of [A P | y] obeys ||a_j - Q r_j||_2 <= c steps rows u ||a_j||_2.  An exactly zero column admits only a
    zero residual.  Restatement: 0.026 of it on 5x3, at most 0.002 elsewhere (the theorem's worst case is far from a
    Gaussian matrix).
  * forward agreement with the reference, elementwise on R (columns mapped back through perm) and on Q^T y:
    FWD_C eps sqrt(rows) max|[A | y]| with FWD_C = 2.  A QR has no forward bound free of the conditioning; this one is
    calibrated on the restatement, which must stay within a QUARTER of it on every case (RESTATEMENT_SLACK, asserted
    by the host test), so that a kernel that sums in another order has a factor 4 left.  Measured at FWD_C = 2, with
    the products of the restatement summed in three different orders (BLAS, einsum, numpy's pairwise sum - the
    committed one, because it gives the same bits in every run): at most 0.16 of the bound on the ten shapes and the
    two zero cases.  Two cases missed the quarter in one of the orders, and get four times their measured worst
    (FWD_C_OF): `tie` 0.60 eps sqrt(rows) max|A| -> 2.4, and `lowrank`, whose rows of R below the determined ones
    reached 1.03 eps sqrt(rows) max|A| -> 4.1, rounded up to 4.2 (they hold the rounding noise of the product G H
    itself, which no order of summation removes).  Committed restatement: 0.14 (tie), 0.22 (lowrank) of those.
  * sqrt_solve (W = R^-T P^T X, Higham Thm 8.5): |P^T X - R^T W| <= c m u |R^T| |W| elementwise, the residual in
    longdouble.  The 64-wide diagonal blocks are solved by substitution and the hand-over between them is a product
    whose terms the same sum covers, so there is no term for an explicit inverse.  Restatement: 0.20 at m = 1 (one
    division against 4 u), at most 0.007 beyond.
  * back_solve (out = P [R11^-1 c[:np]; 0]): |R11 z - c[:np]| <= c np u |R11| |z|; out[perm[i]] = z[i] and
    out[perm[i]] = +0 for i >= np are exact.  Restatement: 0.099 at m = 1, at most 0.011 beyond.

Tried on a copy of the restatement, outside the repository: the last index instead of the first on a tie; the last row
of a column longer than 256 left out of the update, or of the dot product, or of the initial norms; the pivot search
confined to 1024 columns; the reflector's last row beyond 1024 not scaled; `tail < 0` for the DBL_MIN branch; the
scatter of back_solve with i <= np; the hand-over between two 64-blocks of sqrt_solve skipped.  Each fails at least one
check of tests/test_qr_gpu.py.
"""
import functools

import numpy as np

U = 2.0 ** -53
EPS = 2.0 * U
DBL_MIN = 2.2250738585072014e-308
CB = 4.0
FWD_C = 2.0
FWD_C_OF = {"tie": 2.4, "lowrank": 4.2}  # per case, where the restatement misses a quarter of the bound at FWD_C (docstring)
PIVOT_GAP = 1e-8
RANK_MARGIN = 4.0
NP_MARGIN = 16.0
RESTATEMENT_SLACK = 0.25  # the float64 restatement stays within this fraction of the forward bound
LONGDOUBLE_WORK = 2.0e8   # rows * cols^2 up to which the reference runs in np.longdouble
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 2.0 ** -60
LD = np.longdouble if HAVE_LONGDOUBLE else np.float64


# ---- the algorithm, restated --------------------------------------------------------------------------------------
def colpiv_qr(M, cols, dtype):
    """Column-pivoted Householder QR of the first `cols` columns of M (rows x (cols + extra)); the extra columns are
    carried along un-pivoted.  Returns a dict: qr (R above, essential parts below), tau, perm, threshold_helper,
    nonzero_pivots, rank,
    maxpivot, gap (per step: relative gap of the two largest squared norms; inf with one column left), np_margin."""
    A = np.array(M, dtype=dtype, order="F")
    rows, _ = A.shape
    steps = min(rows, cols)
    eps, tiny = dtype(EPS), dtype(DBL_MIN)
    perm = np.arange(cols, dtype=np.int64)
    tau = np.zeros(cols, dtype=dtype)
    max_norm = np.sqrt((A[:, :cols] ** 2).sum(axis=0)).max()
    t = max_norm * eps / dtype(rows)
    helper = t * t
    nonzero_pivots, maxpivot = cols, dtype(0)
    gap = np.full(steps, np.inf)
    np_margin = np.inf
    for k in range(steps):
        sq = (A[k:, k:cols] ** 2).sum(axis=0)      # recomputed over rows k and below
        b = int(np.argmax(sq))                      # the first index of the largest
        best, best_sq = k + b, sq[b]
        if sq.size > 1:
            second = np.delete(sq, b).max()
            gap[k] = float((best_sq - second) / best_sq) if best_sq > 0 else 0.0
        if nonzero_pivots == cols:
            thr = helper * dtype(rows - k)
            lo, hi = (best_sq, thr) if best_sq < thr else (thr, best_sq)
            np_margin = min(np_margin, float(hi / lo) if lo > 0 else np.inf)
            if best_sq < thr:
                nonzero_pivots = k
        if best != k:
            A[:, [k, best]] = A[:, [best, k]]
            perm[[k, best]] = perm[[best, k]]
        x = A[k:, k]                                # makeHouseholderInPlace
        x0 = x[0]
        tail = (x[1:] ** 2).sum() if x.size > 1 else dtype(0)
        if tail <= tiny:
            tk, beta = dtype(0), x0
            x[1:] = 0
        else:
            beta = np.sqrt(x0 * x0 + tail)
            if x0 >= 0:
                beta = -beta
            x[1:] /= x0 - beta
            tk = (beta - x0) / beta
        x[0] = beta
        tau[k] = tk
        if k + 1 < A.shape[1]:                      # I - tau v v^T on the columns behind, v = [1; essential]
            v = x.copy()
            v[0] = 1
            C = A[k:, k + 1:]
            C -= np.outer(v, tk * (v[:, None] * C).sum(axis=0))  # (numpy's pairwise sums: the same in every run)
        maxpivot = max(maxpivot, abs(beta))
    d = np.abs(np.diagonal(A)[:steps])
    thr = maxpivot * eps * dtype(steps)
    rank = int((d > thr).sum())
    nz = d[d > 0]
    rank_margin = float(np.where(nz > thr, nz / thr, thr / nz).min()) if nz.size and thr > 0 else np.inf
    return dict(qr=A, tau=tau, perm=perm, threshold_helper=helper, nonzero_pivots=nonzero_pivots, rank=rank, maxpivot=maxpivot, gap=gap,
                np_margin=np_margin, rank_margin=rank_margin)


def apply_q(qr, tau, steps, B, dtype):
    """Q B for Q = H_0 H_1 ... H_{steps-1} of the stored reflectors; column j of B must be zero below row j where
    j < steps (an upper-trapezoidal R beside full columns), which lets H_k skip the columns before k."""
    B = np.array(B, dtype=dtype, order="F")
    for k in reversed(range(steps)):
        if tau[k] == 0:
            continue
        v = qr[k:, k].astype(dtype)
        v[0] = 1
        C = B[k:, k:]
        C -= np.outer(v, dtype(tau[k]) * (v[:, None] * C).sum(axis=0))
    return B


def back_solve(R, perm, npv, c, dtype=np.float64):
    """ColPivHouseholderQR::solve after Q^T: (out = P [R11^-1 c[:np]; 0], z = R11^-1 c[:np]) by column-oriented back
    substitution."""
    z = np.array(c[:npv], dtype=dtype)
    for i in range(npv - 1, -1, -1):
        z[i] = z[i] / dtype(R[i, i])
        z[:i] -= R[:i, i].astype(dtype) * z[i]
    out = np.zeros(len(perm), dtype=dtype)
    out[perm[:npv]] = z
    return out, z


def sqrt_solve(R, perm, X, dtype=np.float64):
    """sqrt_solve(R, P, X) = R^-T P^T X: forward substitution against the lower-triangular R^T, row by row."""
    W = np.array(X[perm], dtype=dtype)
    for i in range(len(perm)):
        W[i] = (W[i] - R[:i, i].astype(dtype) @ W[:i]) / dtype(R[i, i])
    return W


# ---- inputs -------------------------------------------------------------------------------------------------------
# rows x cols: the 256-wide strided loops of qr_norms_kernel / qr_apply_kernel with 1, 2 and 3 trips and ragged tails
# (257, 300, 520 rows), the 1024-wide loops of qr_pivot_kernel over rows (1100, 2100) and over columns (1030)
SHAPES = [(1, 1), (5, 3), (64, 64), (65, 64), (257, 257), (300, 129), (520, 300), (1100, 40), (2100, 33), (1040, 1030)]
SPECIAL = ["zeros", "zerocol", "tie", "lowrank"]
LOWRANK = (200, 37, 90)  # G (200 x 37) H (37 x 90)
NP_EXEMPT = ("tie",)
SEEDS = {}  # name -> seed, for a case that misses the pivot-gap condition with seed 0


def scaled_gaussian(rng, rows, cols):
    """Gaussian columns scaled by a shuffled geomspace(0.1, 10).  Beyond 1024 columns the largest scale goes to column
    cols - 3: the first pivot is then found in the second trip of qr_pivot_kernel's 1024-wide search."""
    scale = rng.permutation(np.geomspace(0.1, 10.0, cols))
    if cols > 1024:
        j = int(np.argmax(scale))
        scale[[j, cols - 3]] = scale[[cols - 3, j]]
    return rng.standard_normal((rows, cols)) * scale


@functools.lru_cache(maxsize=None)
def qr_input(name):
    """(A, y, determined steps) of a case: `name` is 'ROWSxCOLS' or one of SPECIAL."""
    seed = SEEDS.get(name, 0)
    if name in SPECIAL:
        rng = np.random.default_rng(5000 + 101 * SPECIAL.index(name) + seed)
        if name == "zeros":       # [T; 0]: exact rank 20, every later norm exactly zero
            A = np.zeros((80, 50))
            A[:20] = rng.standard_normal((20, 50))
            det = 50
        elif name == "zerocol":   # one exactly zero column: it is the last pivot, with tau = 0
            A = scaled_gaussian(rng, 30, 12)
            A[:, 5] = 0.0
            det = 12
        elif name == "tie":       # column 40 a bitwise copy of column 2, both of the largest norm
            A = scaled_gaussian(rng, 90, 70)
            A[:, 2] *= 1.5 * np.sqrt((A * A).sum(axis=0).max() / (A[:, 2] @ A[:, 2]))
            A[:, 40] = A[:, 2]
            det = 69              # the copy is rounding noise after the first step: the last reflector is arbitrary
        else:                     # rank 37 up to rounding noise
            r, k, c = LOWRANK
            A = rng.standard_normal((r, k)) @ rng.standard_normal((k, c))
            det = k
    else:
        rows, cols = (int(v) for v in name.split("x"))
        rng = np.random.default_rng(4000 + 13 * rows + cols + 7919 * seed)
        A = scaled_gaussian(rng, rows, cols)
        det = cols
    y = rng.standard_normal(A.shape[0])
    A.setflags(write=False)
    y.setflags(write=False)
    return A, y, det


def reference_dtype(rows, cols):
    return LD if float(rows) * cols * cols <= LONGDOUBLE_WORK else np.float64


@functools.lru_cache(maxsize=None)
def restated(name, which):
    """The restatement on [A | y] of a case (the factorisation of A alone is its first `cols` columns: a carried column
    changes nothing before it).  which = 'ref': in the case's reference dtype; 'f64': in float64."""
    A, y, _ = qr_input(name)
    dtype = reference_dtype(*A.shape) if which == "ref" else np.float64
    if which == "ref" and dtype is np.float64:
        return restated(name, "f64")
    return colpiv_qr(np.column_stack([A, y]), A.shape[1], dtype)


def ref_factor(name):
    """2 where the float64 restatement stands in for the longdouble reference (the doubled bounds), else 1."""
    return 2.0 if reference_dtype(*qr_input(name)[0].shape) is np.float64 else 1.0


def qr_cases():
    out = []
    for rows, cols in SHAPES:
        for extra in (0, 1):
            out.append(dict(name=f"{rows}x{cols}", extra=extra, id=f"{rows}x{cols}-extra{extra}"))
    for name in SPECIAL:
        out.append(dict(name=name, extra=1, id=f"{name}-extra1"))
    return out


def pick_ld(rows):
    """A leading dimension > rows that is no multiple of 8 (the factor's own, api.hip: factor_ld, always is)."""
    ld = rows + 3
    return ld + 2 if ld % 8 == 0 else ld


# ---- the checks ---------------------------------------------------------------------------------------------------
def ratio_of(R, bound):
    """max |R| / bound; a zero bound admits only a zero residual."""
    R, bound = np.asarray(R, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if R.size == 0:
        return 0.0
    zero = bound == 0.0
    if np.any(R[zero] != 0.0) or not np.all(np.isfinite(R)):
        return np.inf
    if np.all(zero):
        return 0.0
    return float((np.abs(R[~zero]) / bound[~zero]).max())


def tau_ratio(qr, tau, cols):
    """max |tau_k v_k^T v_k - 2| / (c len u) over the steps with tau_k != 0, in longdouble."""
    rows = qr.shape[0]
    worst = 0.0
    for k in np.flatnonzero(np.asarray(tau[:cols]) != 0):
        v = qr[k + 1:, k].astype(LD)
        vv = LD(1) + v @ v
        worst = max(worst, float(abs(LD(tau[k]) * vv - 2)) / (CB * (rows - k) * U))
    return worst


def backward_ratio(name, extra, qr, tau, perm):
    """max_j ||a_j - Q r_j||_2 / (c steps rows u ||a_j||_2) over the columns of [A P | y], Q from the given reflectors.
    Formed in longdouble; where the float64 restatement is the reference, in float64 against the doubled bound (the
    rounding of forming Q R in double is of the size of the bound itself)."""
    A, y, _ = qr_input(name)
    rows, cols = A.shape
    steps = min(rows, cols)
    f = ref_factor(name)
    dtype = np.float64 if f > 1.0 else LD
    M = np.column_stack([A[:, perm]] + ([y] if extra else []))
    B = np.zeros(M.shape, dtype=dtype, order="F")
    B[:, :cols] = np.triu(qr[:, :cols])
    B[:, cols:] = qr[:, cols:cols + extra]
    QR = apply_q(qr, tau, steps, B, dtype)
    res = np.sqrt(((M.astype(dtype) - QR) ** 2).sum(axis=0)).astype(np.float64)
    return ratio_of(res, f * CB * steps * rows * U * np.sqrt((M * M).sum(axis=0)))


def forward_bound(name, extra):
    A, y, _ = qr_input(name)
    top = max(np.abs(A).max(), np.abs(y).max() if extra else 0.0)
    return ref_factor(name) * FWD_C_OF.get(name, FWD_C) * EPS * np.sqrt(A.shape[0]) * top


def unpermuted_r(qr, perm, cols, det):
    """R[:det, :] with its columns back in their original order."""
    R = np.zeros((det, cols), dtype=qr.dtype)
    R[:, perm] = np.triu(qr[:cols, :cols])[:det]
    return R


def forward_ratios(name, extra, qr, perm):
    """(agreement of R[:det] and of Q^T y with the reference, max|R[det:, :]|), each over the forward bound.  Only the
    determined rows are compared; with every step determined the whole carried column is."""
    A, _, det = qr_input(name)
    rows, cols = A.shape
    ref = restated(name, "ref")
    bound = forward_bound(name, extra)
    diff = np.abs(unpermuted_r(qr, perm, cols, det).astype(LD) - unpermuted_r(ref["qr"], ref["perm"], cols, det).astype(LD)).max()
    if extra:
        top = rows if det == cols else det
        diff = max(diff, np.abs(qr[:top, cols].astype(LD) - ref["qr"][:top, cols].astype(LD)).max())
    below = np.abs(np.triu(qr[:cols, :cols])[det:]).max() if det < cols else 0.0
    return float(diff) / bound, float(below) / bound


def helper_ratio(name, got):
    """|state[0] - threshold_helper| over c rows u threshold_helper: the helper is (max_j ||a_j|| eps / rows)^2, and a sum
    of `rows` squares carries a relative error of at most rows u in any order (the square root halves it, the square
    doubles it again; c covers the three roundings around it)."""
    want = restated(name, "ref")["threshold_helper"]
    rows = qr_input(name)[0].shape[0]
    return float(abs(LD(got) - want) / (ref_factor(name) * CB * rows * U * want))


def after_swaps(perm, k):
    """The permutation the first k pivot swaps alone leave: what perm must be when no later step swaps (every later
    tie won by the column already in place).  Not ascending behind k: a swap parks the displaced column at the pivot's
    old place."""
    out = np.arange(len(perm), dtype=np.int64)
    for i in range(k):
        j = int(np.flatnonzero(out == perm[i])[0])
        out[[i, j]] = out[[j, i]]
    return out


def pivot_gap_ok(name):
    """(holds, smallest non-zero gap) over the determined steps of the reference run."""
    g = restated(name, "ref")["gap"][:qr_input(name)[2]]
    nz = g[g != 0.0]
    return bool(np.all(nz >= PIVOT_GAP)), float(nz.min()) if nz.size else np.inf


def counts_determined(name):
    """nonzero_pivots is compared: both runs agree on it with NP_MARGIN to spare at every decisive step."""
    r, f = restated(name, "ref"), restated(name, "f64")
    return r["nonzero_pivots"] == f["nonzero_pivots"] and min(r["np_margin"], f["np_margin"]) >= NP_MARGIN


# ---- the substitutions against R ----------------------------------------------------------------------------------
# m: one block, the 63 / 64 / 65 edge of a block, two blocks and one row more, a ragged fourth block, nine blocks;
# nrhs: around the four right-hand sides of a workgroup
SQRT_M = [1, 63, 64, 65, 128, 129, 200, 520]
SQRT_NRHS = [1, 3, 4, 5, 37]
SQRT_SHAPES = [(m, r) for m in SQRT_M for r in SQRT_NRHS] + [(65, 4100)]  # 4100: past the 4096 rows of the permutation grid
BACK_SHAPES = [(m, npv) for m in (1, 64, 300, 1030) for npv in sorted({m, m // 2})]


@functools.lru_cache(maxsize=None)
def square_factor(m):
    """(R, perm) in float64 from the reference QR of an m x m scaled Gaussian; R upper triangular, zeros below."""
    rng = np.random.default_rng(9000 + m)
    f = colpiv_qr(scaled_gaussian(rng, m, m), m, reference_dtype(m, m))
    R = np.asfortranarray(np.triu(f["qr"]).astype(np.float64))
    R.setflags(write=False)
    f["perm"].setflags(write=False)
    return R, f["perm"]


def solve_rhs(m, nrhs):
    return np.asfortranarray(np.random.default_rng(31 * m + nrhs).standard_normal((m, nrhs)))


def sqrt_solve_ratio(R, perm, X, W):
    m = R.shape[0]
    res = X[perm].astype(LD) - R.T.astype(LD) @ W.astype(LD)
    return ratio_of(res, CB * m * U * (np.abs(R.T) @ np.abs(W)))


def back_solve_ratio(R, npv, c, z):
    if npv == 0:
        return 0.0
    R11 = R[:npv, :npv]
    res = R11.astype(LD) @ z.astype(LD) - c[:npv].astype(LD)
    return ratio_of(res, CB * npv * U * (np.abs(R11) @ np.abs(z)))
