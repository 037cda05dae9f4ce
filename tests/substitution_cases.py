"""Shared by tests/test_substitution_bounds_host.py and tests/test_substitutions_gpu.py: the shapes, matrices, right-hand
sides and the residual bound of the triangular substitutions of csrc/solve.hip, and their numpy restatement.

The bound.  u = 2^-53, c = 4 (CB of tests/test_fit_schedules_gpu.py).  Every path solves T X = B (T = L, or L^T for the
backward forms; the right-hand forms X L^T = B are the forward form of X^T) block row by block row over diagonal blocks
of width b whose inverses are formed EXPLICITLY and applied as products: b = 16 for the MFMA micro-substitution
(trsm_micro_kernel, backsub_coop_kernel), 128 for the vector chains, 512 for forward_solve_wide.  For block row I

    |B - T X|_I  <=  c n u (|T| |X|)_I  +  2 c b u |T_II| |T_II^-1| |T_II| |X_I|

The first term is the backward error of a substitution (Higham, Thm 8.5: gamma_n |T| |X|, here with the sums in the order
the kernels take them - c covers the constant).  The second is the price of X_I = Y t with Y = fl(T_II^-1) instead of a
substitution against T_II: t = B_I - sum T_IJ X_J is T_II X_I up to the first term, the product Y t rounds with
b u |Y| |t| <= b u |T_II^-1| |T_II| |X_I|, and an inverse obtained by substitution has the residual |T_II Y - I| <=
b u |T_II| |T_II^-1|, which t multiplies - both times |T_II| from the left gives the term above.
T is the factor the device solved against (the debug entry point returns it: the error of the factorisation itself is
the business of tests/test_fit_schedules_gpu.py and would enter with the condition number); T_II^-1 and all products of
the bound are numpy's / scipy's.  The residual is computed in np.longdouble where that takes seconds; for the large
shapes in fp64, with the rounding of that product, n u |T| |X|, added to the bound.  Above n = FULL_CHECK_MAX only the
128-row block rows at the edges of the 512-wide outer steps, the last one and 16 at random are checked.
No tolerance here depends on the conditioning of the matrix or on what the kernels were seen to give.
"""
import functools

import numpy as np
from scipy.linalg import solve_triangular

U = 2.0 ** -53
CB = 4.0
MB, NB, NBO, WIDE_BW = 16, 128, 512, 512
FULL_CHECK_MAX = 2200
LONGDOUBLE_MACS = 2.0e7  # residuals up to this many multiply-adds are computed in np.longdouble
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 2.0 ** -60

# kinds of agp_debug_substitute (csrc/debug_api.hip)
(FWD_MAT, FWD_MAT_LOOKAHEAD, FWD_MAT_BATCHED, BWD_MAT, RIGHT_LT, RIGHT_LT_BATCHED, FWD_VEC, BWD_VEC, BWD_VEC_BATCHED,
 COOP_DIRECT, COOP_FLAGS, COOP_BATCHED, BACK_UPDATE) = range(13)
BLOCK_WIDTH = {FWD_MAT: MB, FWD_MAT_LOOKAHEAD: MB, FWD_MAT_BATCHED: MB, BWD_MAT: MB, RIGHT_LT: MB, RIGHT_LT_BATCHED: MB,
               FWD_VEC: NB, BWD_VEC: NB, BWD_VEC_BATCHED: MB, COOP_DIRECT: MB, COOP_FLAGS: MB, COOP_BATCHED: MB}
TRANSPOSED = {BWD_MAT, BWD_VEC, BWD_VEC_BATCHED, COOP_DIRECT, COOP_FLAGS, COOP_BATCHED}


# ---- matrices and right-hand sides --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def spd_matrix(family, n, seed=0):
    """'rand': B B^T / r + I (B n x (n + 5) Gaussian); 'gram': the squared-exponential Gram matrix of n points uniform in
    [0, 10]^3 (length scale 1.5) plus the noise that puts cond(K) near 1e6.  Different seeds give different matrices."""
    rng = np.random.default_rng(1000 + 7919 * seed + n)
    if family == "rand":
        r = n + 5
        B = rng.standard_normal((n, r))
        K = B @ B.T
        K /= r
        K[np.diag_indices(n)] += 1.0
    else:
        x = rng.uniform(0.0, 10.0, (n, 3))
        sq = (x * x).sum(axis=1)
        K = x @ x.T
        K *= -2.0
        K += sq[:, None]
        K += sq[None, :]
        np.maximum(K, 0.0, out=K)
        K *= -1.0 / (2 * 1.5 ** 2)
        np.exp(K, out=K)
        K = 0.5 * (K + K.T)
        v = rng.standard_normal(n)
        for _ in range(30):  # power iteration: lambda_max to a few digits
            v = K @ v
            v /= np.linalg.norm(v)
        K[np.diag_indices(n)] += float(v @ (K @ v)) / 1e6
    return np.asfortranarray(K)


def family_of(index):
    return "rand" if index % 2 == 0 else "gram"


def rhs_matrix(rows, cols, seed, lower=None):
    """Gaussian right-hand side; lower = 'eye': the identity, 'rand': Gaussian on and below the diagonal."""
    rng = np.random.default_rng(seed)
    if lower == "eye":
        return np.asfortranarray(np.eye(rows, cols))
    B = rng.standard_normal((rows, cols))
    if lower == "rand":
        B = np.tril(B)
    return np.asfortranarray(B)


def untouched_above(n, m, outer=NB):
    """Masks of an n x m right-hand side under rhs_lower: (never read nor written, read as zeros but never written).
    Block row k (128 rows) is solved and applied in its first k + nbk columns only (m_act); forward_solve_mat and its
    look-ahead (outer = NBO) then apply a whole 512-row outer block [K0, kend) at once in the first kend columns, which
    reads the zeros between k + nbk and kend; the batched form (outer = NB) never does."""
    never = np.zeros((n, m), dtype=bool)
    zeros = np.zeros((n, m), dtype=bool)
    for k in range(0, n, NB):
        kend = min(n, (k // outer + 1) * outer)
        never[k:k + NB, kend:] = True
        zeros[k:k + NB, min(n, k + NB):kend] = True
    return never, zeros


# ---- the bound ----------------------------------------------------------------------------------------------------
def check_rows(n, seed=0):
    """All rows up to FULL_CHECK_MAX; above: the 128-row block rows on both sides of every 512-wide outer step, the last
    (ragged) one and 16 at random."""
    if n <= FULL_CHECK_MAX:
        return np.arange(n)
    nblk = -(-n // NB)
    blocks = {nblk - 1}
    for e in range(NBO, n, NBO):
        blocks.update(((e - 1) // NB, e // NB))
    blocks.update(np.random.default_rng(seed + n).choice(nblk, size=min(16, nblk), replace=False).tolist())
    return np.concatenate([np.arange(b * NB, min(n, b * NB + NB)) for b in sorted(blocks)])


def diag_block_term(T, X, b, lower):
    """|T_II| |T_II^-1| |T_II| |X_I| for the b-wide diagonal blocks (rows of all blocks stacked)."""
    n = T.shape[0]
    out = np.empty_like(X)
    aX = np.abs(X)
    for i in range(0, n, b):
        Tii = T[i:i + b, i:i + b]
        inv = solve_triangular(Tii, np.eye(Tii.shape[0]), lower=lower)
        aT = np.abs(Tii)
        out[i:i + b] = aT @ (np.abs(inv) @ (aT @ aX[i:i + b]))
    return out


def residual_bound(L, X, B, b, transposed, rows=None):
    """(|B - T X|, bound) on `rows` (default check_rows) for T = L^T if transposed else L; X, B n x m."""
    n = L.shape[0]
    X = X.reshape(n, -1)
    B = B.reshape(n, -1)
    T = L.T if transposed else L
    rows = check_rows(n) if rows is None else rows
    Tr = T[rows]
    first = np.abs(Tr) @ np.abs(X)
    bound = CB * n * U * first + 2 * CB * b * U * diag_block_term(T, X, b, not transposed)[rows]
    if HAVE_LONGDOUBLE and float(len(rows)) * n * X.shape[1] <= LONGDOUBLE_MACS:
        R = np.abs(B[rows].astype(np.longdouble) - Tr.astype(np.longdouble) @ X.astype(np.longdouble)).astype(np.float64)
    else:
        R = np.abs(B[rows] - Tr @ X)
        bound = bound + n * U * first  # the rounding of this product
    return R, bound


def ratio_of(R, bound):
    """max |R| / bound; a zero bound admits only a zero residual."""
    zero = bound == 0.0
    if np.any(R[zero] != 0.0) or not np.all(np.isfinite(R)):
        return np.inf
    if np.all(zero):
        return 0.0
    return float((R[~zero] / bound[~zero]).max())


def residual_ratio(L, X, B, b, transposed, rows=None):
    return ratio_of(*residual_bound(L, X, B, b, transposed, rows))


def agreement_ratio(L, X1, X2, B, b, transposed, rows=None, b2=None):
    """Two solutions of the same system agree within the bound: |T (X1 - X2)| <= bound(X1) + bound(X2) (each meets it
    against the same B)."""
    n = L.shape[0]
    rows = check_rows(n) if rows is None else rows
    _, bd1 = residual_bound(L, X1, B, b, transposed, rows)
    _, bd2 = residual_bound(L, X2, B, b if b2 is None else b2, transposed, rows)
    T = (L.T if transposed else L)[rows]
    D = X1.reshape(n, -1) - X2.reshape(n, -1)
    R = np.abs(T @ D)
    return ratio_of(R, bd1 + bd2 + n * U * (np.abs(T) @ np.abs(D)))


# ---- the algorithms, restated -------------------------------------------------------------------------------------
def blocked_substitution(L, B, b, transposed):
    """T X = B in fp64 by block rows of width b with EXPLICIT inverses of the diagonal blocks (themselves obtained by
    substitution), the way every path of solve.hip works: X_I = fl(T_II^-1) (B_I - sum_J T_IJ X_J)."""
    n = L.shape[0]
    X = np.array(B, dtype=np.float64, order="F").reshape(n, -1)
    starts = list(range(0, n, b))
    if not transposed:
        for i in starts:
            j = min(n, i + b)
            inv = solve_triangular(L[i:j, i:j], np.eye(j - i), lower=True)
            X[i:j] = inv @ (X[i:j] - L[i:j, :i] @ X[:i])
    else:
        for i in reversed(starts):
            j = min(n, i + b)
            inv = solve_triangular(L[i:j, i:j].T, np.eye(j - i), lower=False)
            X[i:j] = inv @ (X[i:j] - L[j:, i:j].T @ X[j:])
    return X


# ---- shapes -------------------------------------------------------------------------------------------------------
# Derived from the constants: MB = 16 rows of a micro block, 16 columns per wave and 64 per workgroup of
# trsm_micro_kernel, NB = 128, NBO = 512, the look-ahead's switches n > 2 NBO and m >= 64.
# forward_solve_mat / backward_solve_mat: (n, m)
MAT_SHAPES = [(1, 1), (15, 17), (16, 16), (17, 15), (127, 63), (128, 64), (129, 65), (511, 200), (512, 1), (513, 1000),
              (1024, 17), (1025, 64), (1537, 65), (2177, 200)]
# rhs_lower = 1 (forward_solve_mat): (n, m); m < n, m = n and m > n (m_act reaches m before the last block row)
LOWER_SHAPES = [(17, 17), (129, 129), (129, 65), (513, 513), (513, 1000), (1025, 1025), (1537, 200)]
# forward_solve_mat_lookahead: (n, m, rhs_lower, two streams expected).  One stream for n <= 2 NBO or m < 64; three outer
# blocks at 1025 (the first U2), four at 1537, five at 2177 (ev_b waited on from the third on), six at 2700.
LOOKAHEAD_SHAPES = [(1024, 64, 0, False), (1025, 63, 0, False), (1025, 64, 0, True), (1537, 200, 0, True),
                    (2177, 65, 0, True), (2700, 1000, 0, True), (1025, 1025, 1, True), (1537, 200, 1, True),
                    (2177, 2177, 1, True)]
# forward_solve_mat_batched: (n, m, count, rhs_lower); (512, 512, 3, 1) is invert_wide_blocks' call
FWD_BATCHED_SHAPES = [(16, 17, 3, 0), (129, 65, 4, 0), (300, 200, 5, 0), (513, 64, 2, 0), (129, 129, 2, 1), (512, 512, 3, 1)]
# right_solve_lt: (n, nrows);  right_solve_lt_batched: (n, nrows, count)
RIGHT_SHAPES = [(1, 1), (15, 17), (17, 16), (128, 63), (129, 64), (129, 65), (513, 200), (1025, 15), (1537, 1000)]
RIGHT_BATCHED_SHAPES = [(17, 15, 3), (129, 65, 4), (300, 200, 3), (513, 64, 2)]
# the vector chains: n, each at an odd and an even leading dimension of the factor (the double2 selection of
# back_step_kernel) and on the factor's own buffer
VEC_SIZES = [1, 15, 16, 17, 127, 128, 129, 511, 513, 1025, 1537]
# back_update_kernel: (n, k0); nbk = min(128, n - k0) ragged, 1 and full
BACK_UPDATE_SHAPES = [(300, 128), (300, 256), (257, 256), (512, 384)]
# backward_solve_vec_batched: (n, count)
BWD_VEC_BATCHED_SHAPES = [(1, 2), (100, 3), (129, 4), (512, 8), (700, 5), (1300, 4)]
# backward_solve_coop.  Direct hand-over: at most 16 blocks (2047: 16 blocks, the last ragged).  Flags: more than 16
# blocks, dispatched only under AGP_BACKSUB_COOP_MAX (here 4096).  Batched: the (n, count) of tests/test_fit_batch_gpu.py
# that the product sends down this path.
COOP_DIRECT_SIZES = [1, 17, 128, 129, 513, 1000, 2047]
COOP_FLAGS_SIZES = [2049, 2177, 3000]
COOP_BATCHED_SHAPES = [(100, 3), (512, 8), (700, 5), (1300, 4), (256, 40), (520, 24), (1100, 50), (200, 12)]
# forward_solve_wide (tests/test_kernels_gpu.py: test_forward_solve_wide)
WIDE_SHAPES = [(1024, 8192), (1536, 12289), (1024, 9000)]


def odd_even_lda(n):
    """An odd and an even leading dimension >= n + 1."""
    odd = n + 1 if n % 2 == 0 else n + 2
    return odd, odd + 1


def families(n, index):
    """Both families up to n = 600, alternating above (host time)."""
    return ("rand", "gram") if n <= 600 else (family_of(index),)


# ---- the cases, as both test files see them -------------------------------------------------------------------------
def make_case(kind, name, n, cols, family, count=1, lower=None, **extra):
    c = dict(kind=kind, name=name, n=n, cols=cols, family=family, count=count, lower=lower)
    c.update(extra)
    c["id"] = "-".join(str(v) for v in [name, n, cols, family] + ([f"x{count}"] if count > 1 else [])
                       + ([f"lower_{lower}"] if lower else []) + [f"{k}{v}" for k, v in sorted(extra.items())])
    return c


def all_cases():
    """Every (kind, shape, matrix family, right-hand side) the GPU tests run; `cols` is the number of right-hand sides
    (the rows of X for the right-hand forms)."""
    out = []
    for i, (n, m) in enumerate(MAT_SHAPES):
        for fam in families(n, i):
            out.append(make_case(FWD_MAT, "forward_solve_mat", n, m, fam))
            out.append(make_case(BWD_MAT, "backward_solve_mat", n, m, fam))
    for i, (n, m) in enumerate(LOWER_SHAPES):
        for fam in families(n, i):
            for low in ("eye", "rand"):
                out.append(make_case(FWD_MAT, "forward_solve_mat", n, m, fam, lower=low))
    for i, (n, m, low, two) in enumerate(LOOKAHEAD_SHAPES):
        for lw in (("eye", "rand") if low else (None,)):
            out.append(make_case(FWD_MAT_LOOKAHEAD, "forward_solve_mat_lookahead", n, m, family_of(i), lower=lw, two=int(two)))
    for i, (n, m, count, low) in enumerate(FWD_BATCHED_SHAPES):
        for lw in (("eye", "rand") if low else (None,)):
            out.append(make_case(FWD_MAT_BATCHED, "forward_solve_mat_batched", n, m, family_of(i), count=count, lower=lw))
    for i, (n, r) in enumerate(RIGHT_SHAPES):
        for fam in families(n, i):
            out.append(make_case(RIGHT_LT, "right_solve_lt", n, r, fam))
    for i, (n, r, count) in enumerate(RIGHT_BATCHED_SHAPES):
        out.append(make_case(RIGHT_LT_BATCHED, "right_solve_lt_batched", n, r, family_of(i), count=count))
    for i, n in enumerate(VEC_SIZES):
        for kind, name in ((FWD_VEC, "forward_solve_vec"), (BWD_VEC, "backward_solve_vec")):
            for j, lda in enumerate((0,) + odd_even_lda(n)):
                out.append(make_case(kind, name, n, 1, family_of(i + j), lda=lda))
    for i, (n, count) in enumerate(BWD_VEC_BATCHED_SHAPES):
        out.append(make_case(BWD_VEC_BATCHED, "backward_solve_vec_batched", n, 1, family_of(i), count=count))
    for i, n in enumerate(COOP_DIRECT_SIZES):
        for fam in families(n, i):
            out.append(make_case(COOP_DIRECT, "backward_solve_coop_direct", n, 1, fam))
    for i, n in enumerate(COOP_FLAGS_SIZES):
        out.append(make_case(COOP_FLAGS, "backward_solve_coop_flags", n, 1, family_of(i)))
    for i, (n, count) in enumerate(COOP_BATCHED_SHAPES):
        out.append(make_case(COOP_BATCHED, "backward_solve_coop_batched", n, 1, family_of(i), count=count))
    return out


def case_matrices(case):
    """The `count` SPD matrices of a case: a different one per problem of a batch."""
    return [spd_matrix(case["family"], case["n"], p) for p in range(case["count"])]


def case_rhs(case, p=0):
    """Right-hand side of problem p as the n x cols matrix of the equivalent left solve T X = B (the right-hand forms
    store its transpose)."""
    return rhs_matrix(case["n"], case["cols"], 17 + 31 * p + case["n"] + case["cols"], case["lower"])


# ---- the wide vector sweeps and the mixed fit's preconditioner (csrc/api.hip; tests/test_reduce_kernels_gpu.py) ------
# forward_solve_vec_wide, backward_solve_vec_wide, the wide branch of backward_solve_vec_any and mixed_precondition_apply:
# one right-hand side through explicitly inverted BW x BW diagonal blocks, b = BW in the bound (512, and 1024 as the mixed
# fit takes it from n = 8192 - here at n = 2048).  The variants that read the fp32 copy of the factor solve EXACTLY the
# system of Lt = fp32_off_diagonal(L): the fp32 entries are widened and multiplied in fp64, so the bound holds against Lt
# with nothing added, and no fp32 tolerance appears.
WIDE_SWEEP_SHAPES = [(2048, 512), (2560, 512), (2048, 1024)]


def fp32_off_diagonal(L, bw):
    """L with everything below its bw-wide diagonal blocks replaced by its fp32 rounding (the matrix the sweeps with the
    fp32 copy of a factor solve against)."""
    n = L.shape[0]
    T = np.tril(L).astype(np.float32).astype(np.float64)
    for i in range(0, n, bw):
        T[i:i + bw, i:i + bw] = np.tril(L[i:i + bw, i:i + bw])
    return T


def wide_sweep_cases():
    """(n, BW, family) of the sweeps: every shape on both matrix families."""
    return [dict(n=n, bw=bw, family=fam, id=f"{n}-bw{bw}-{fam}") for n, bw in WIDE_SWEEP_SHAPES for fam in ("rand", "gram")]


def wide_sweep_rhs(case):
    return rhs_matrix(case["n"], 1, 91 + case["n"] + case["bw"])


def wide_problem(n, ncols):
    """The matrix and right-hand side of test_forward_solve_wide (tests/test_kernels_gpu.py)."""
    rng = np.random.default_rng(n + ncols)
    G = rng.standard_normal((n, n))
    K = np.asfortranarray(G @ G.T / n + np.eye(n))
    return K, np.asfortranarray(rng.standard_normal((n, ncols)))


def back_update_vectors(n, k0):
    rng = np.random.default_rng(n + k0)
    return rng.standard_normal(k0), rng.standard_normal(min(NB, n - k0))


def back_update_ratio(L, k0, z, x, got):
    """|got - (z - L[k0 : k0 + nbk, : k0]^T x)| against c (nbk + 1) u (|z| + |L|^T |x|), the reference in longdouble."""
    P = L[k0:k0 + NB, :k0]
    ld = np.longdouble if HAVE_LONGDOUBLE else np.float64
    want = z.astype(ld) - P.T.astype(ld) @ x.astype(ld)
    bound = CB * (len(x) + 1) * U * (np.abs(z) + np.abs(P).T @ np.abs(x))
    return ratio_of(np.abs(got - want).astype(np.float64), bound)
