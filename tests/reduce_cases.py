"""Shared by tests/test_reduce_bounds_host.py and tests/test_reduce_kernels_gpu.py: the shapes, inputs, references and
bounds of the small kernels of csrc/reduce.hip, each run on its own through agp_debug_reduce (csrc/debug_api.hip).

Every launcher of reduce.hip and the GPU test that names it (tests/test_reduce_kernels_gpu.py unless stated):
    launch_coldot                  test_coldot
    launch_dot                     test_dot
    launch_matvec                  test_matvec
    launch_tall_matvec             test_tall_matvec
    launch_tall_matvec_f32         test_tall_matvec_f32
    launch_colvec_dot              test_colvec_dot
    launch_colvec_dot_strided      test_colvec_dot_strided
    launch_colvec_dot_batched      test_colvec_dot_batched
    launch_colvec_dot_f32          test_colvec_dot_f32
    launch_symv_lower              tests/test_kernels_gpu.py: test_symv_lower
    launch_symv_lower_batched      test_symv_lower_batched
    launch_contract_combinations   test_contract_combinations
    launch_symmetrize              test_symmetrize
    launch_upper_to_lower          test_upper_to_lower
    launch_transpose_blocks        test_transpose_blocks
    launch_zero_upper              test_zero_upper
    launch_set_identity            test_set_identity
    launch_set_identity_batched    test_set_identity_batched
    launch_negate                  test_negate
    launch_nan_scan_lower          test_nan_scan_lower
    launch_copy_lower              test_copy_lower, test_copy_lower_nan_flag
    launch_convert_lower_f32       test_convert_lower_f32
    launch_loo                     test_loo
    launch_gather_cols             test_gather_cols
    launch_gather_vec              test_gather_vec
    launch_pad_columns             test_pad_columns
    launch_pad_identity            test_pad_identity
    launch_compact_blocks          test_compact_blocks
    launch_axpby                   test_axpby

The bounds.  u = 2^-53.  No tolerance here comes from what the kernels were seen to give.

Reductions.  out = alpha sum_k a_k b_k + beta base over k terms summed in ANY order (threads, waves, chunks): every
product carries one rounding, a term passes through at most k - 1 additions, and alpha * (sum), beta * base and their
addition add three roundings of which each operand sees two - (1 + u)^(k + 2) on every term at the most, so to first
order

    |got - ref|  <=  (k + 2) u (|alpha| sum_k |a_k| |b_k| + |beta| |base|)

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; a fused multiply-add drops a rounding and only
helps).  The bound is relative to sum |a| |b|, not to the result: a dropped term, one counted twice or a column taken from
the neighbour misses it by orders of magnitude (tests/test_reduce_bounds_host.py shows both directions).  The kernels
that read an fp32 matrix multiply in fp64: against the fp32-ROUNDED matrix widened to fp64 the bound is the same one, and
no fp32 tolerance appears anywhere.  ref is computed in np.longdouble (u = 2^-64: its own error is 2^-11 of the bound) and,
where that type is no wider than a double, exactly in rationals.

contract_combinations nests two sums, out(a, b) = sum_i xc_i (sum_j K_ij yc_j) over ka and kb members: the inner sum is a
reduction of kb terms, the outer one of ka terms whose second factor carries the inner error, together
(ka + kb + 2) u sum_i sum_j |xc_i| |K_ij| |yc_j|.

loo and axpby have no sum.  mean = y - information / d is a correctly rounded division q (1 + d1) and a subtraction
(1 + d2): |got - ref| <= u (1 + u) |q| + u |y - q| <= u (2 + u) (|y| + |q|); variance = 1 / d is one rounding, u |1 / d|.
axpby = a x + b y: two products and an addition, |got - ref| <= u (1 + u) (|a x| + |b y|) + u |a x + b y| <=
u (2 + u) (|a x| + |b y|).

Where a kernel takes an optional `base` (null, its own buffer, the buffer of out), tall_matvec*, matvec and colvec_dot8 do
not run every shape with all three: the mode CYCLES over the shape grid (reduction_cases), so that every row count, every
column count - each loop body - and every mode meet several times, at a third of the launches.  That is intended.

Movers and packers (symmetrize, upper_to_lower, transpose_blocks, zero_upper, set_identity*, negate, copy_lower,
convert_lower_f32, gather_*, pad_*, compact_blocks) are bit-exact: the expected buffer is the buffer that went in with the
numpy restatement applied, compared as bit patterns over its WHOLE length - padding rows, the other triangle, rows above
row0 and the gaps between batch entries included.
"""
import fractions
import functools

import numpy as np

U = 2.0 ** -53
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 2.0 ** -60
TALL_MATVEC_MAX_COLS = 2048  # csrc/common.h

# ops of agp_debug_reduce (csrc/debug_api.hip)
(COLDOT, DOT, MATVEC, TALL_MATVEC, TALL_MATVEC_F32, COLVEC_DOT, COLVEC_DOT_STRIDED, COLVEC_DOT_BATCHED, COLVEC_DOT_F32,
 SYMV_LOWER_BATCHED, CONTRACT, SYMMETRIZE, UPPER_TO_LOWER, TRANSPOSE_BLOCKS, ZERO_UPPER, SET_IDENTITY, SET_IDENTITY_BATCHED,
 NEGATE, NAN_SCAN_LOWER, COPY_LOWER, CONVERT_LOWER_F32, LOO, GATHER_COLS, GATHER_VEC, PAD_COLUMNS, PAD_IDENTITY, COMPACT_BLOCKS,
 AXPBY) = range(28)
# kinds of agp_debug_wide_sweep
FWD_VEC_WIDE, BWD_VEC_WIDE, BWD_VEC_ANY_WIDE, MIXED_PRECONDITION = range(4)

# ---- shapes (derived from the kernels' strides: 256 threads per column, 1024 per dot, 64 rows x 4 waves x 16 / 8 / 1
# columns of tall_matvec, 8 columns x 512 rows of colvec_dot8, 32 x 32 tiles, 16 x 16 outputs of contract_combinations,
# pairs of rows and relaunches every 2048 columns of the lower-triangle copies) ----------------------------------------
TILE_SIZES = [1, 31, 32, 33, 65, 100]
COLUMN_ROWS = [1, 255, 256, 257, 1000]
DOT_SIZES = [1, 1023, 1024, 1025, 5000]
MATVEC_M = [1, 255, 256, 257]
MATVEC_N = [1, 2, 1023, 1024, 1025, 2049]
TALL_ROWS = [1, 63, 64, 65, 200]
TALL_COLS = [1, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65, 100, 512, 1024, 2047, 2048]
DOT8_N = [1, 2, 7, 8, 9, 17]
DOT8_M = [1, 63, 64, 65, 511, 512, 513, 1025]
LOWER_SIZES = [1, 2, 3, 511, 512, 513, 2048, 2049, 2050]
SYMV_SIZES = [1, 31, 32, 33, 100, 257]
CONTRACT_SIZES = [1, 15, 16, 17, 33]
GROUP_SMAX = [8, 33]
GROUP_ROWS = [1, 257]
BASE_MODES = ("null", "distinct", "alias")


def factor_ld(n):
    """csrc/api.hip: factor_ld."""
    ld = (n + 7) // 8 * 8
    return ld + 8 if ld % 256 == 0 else ld


def group_offsets(smax):
    """Groups of sizes {smax, 1, 0, 7}."""
    return np.concatenate([[0], np.cumsum([smax, 1, 0, 7])]).astype(np.int64)


def rng_of(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


# ---- the reduction bound ------------------------------------------------------------------------------------------
def _exact_dot(F):
    """sum_k prod_f F[f][o, k] for every output o, rounded once: longdouble, or rationals where that is no wider."""
    if HAVE_LONGDOUBLE:
        P = F[0].astype(np.longdouble)
        for f in F[1:]:
            P = P * f.astype(np.longdouble)
        return P.sum(axis=1)
    out = np.empty(F[0].shape[0])
    for o in range(F[0].shape[0]):
        acc = fractions.Fraction(0)
        for k in range(F[0].shape[1]):
            t = fractions.Fraction(1)
            for f in F:
                t *= fractions.Fraction(float(f[o, k]))
            acc += t
        out[o] = float(acc)
    return out


def reference_and_bound(F, k, alpha=1.0, beta=0.0, base=None):
    """(ref, bound) of out = alpha sum_k prod_f F[f][:, k] + beta base; F: factor arrays (outputs x terms, broadcast
    before the call); k: the terms of one output (a number or one per output)."""
    outputs = F[0].shape[0]
    ld = np.longdouble if HAVE_LONGDOUBLE else np.float64
    s = _exact_dot(F) if F[0].shape[1] else np.zeros(outputs, dtype=ld)
    a = np.ones(F[0].shape)
    for f in F:
        a = a * np.abs(f)
    mag = abs(alpha) * a.sum(axis=1)
    ref = ld(alpha) * s
    if base is not None:
        ref = ref + ld(beta) * base.astype(ld)
        mag = mag + abs(beta) * np.abs(base)
    return ref, (np.asarray(k, dtype=np.float64) + 2.0) * U * mag


def error_ratio(got, ref, bound):
    """max |got - ref| / bound; a zero bound admits only an exact result."""
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    if not np.all(np.isfinite(err)):
        return np.inf
    zero = bound == 0.0
    if np.any(err[zero] != 0.0):
        return np.inf
    return float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0


def plain_dot(F, alpha=1.0, beta=0.0, base=None):
    """The same in plain fp64 with numpy's own summation."""
    s = np.einsum("ok,ok->o", F[0], F[1]) if F[0].shape[1] else np.zeros(F[0].shape[0])
    return alpha * s + (beta * base if base is not None else 0.0)


def plain_loop(F, alpha=1.0, beta=0.0, base=None):
    """... and term after term from the left."""
    s = np.zeros(F[0].shape[0])
    for k in range(F[0].shape[1]):
        s = s + F[0][:, k] * F[1][:, k]
    return alpha * s + (beta * base if base is not None else 0.0)


# ---- reduction cases: the inputs as the kernels see them, and their canonical form ---------------------------------
def nan_padded(M, ld, extra=0):
    """Column-major rows x cols M in a NaN-filled buffer of leading dimension ld and `extra` further words: (flat, view)."""
    rows, cols = M.shape
    flat = np.full(ld * cols + extra, np.nan, dtype=M.dtype)
    view = flat[:ld * cols].reshape((ld, cols), order="F")
    view[:rows] = M
    return flat, view


def base_of(mode, rng, n):
    return None if mode == "null" else rng.standard_normal(n)


def reduction_cases():
    """Every reduction case of the GPU file: dict(kernel, id, shape parameters)."""
    out = []

    def add(kernel, **kw):
        kw["kernel"] = kernel
        kw["id"] = kernel + "-" + "-".join(f"{k}{v}" for k, v in kw.items() if k != "kernel")
        out.append(kw)

    for i, rows in enumerate(COLUMN_ROWS):
        add("coldot", n=rows, m=3, base=BASE_MODES[i % 2])
        for j, mode in enumerate(BASE_MODES):
            add("colvec_dot", m=rows, n=3 + j, base=mode)
        add("colvec_dot_strided", m=rows, n=3, count=3, base=BASE_MODES[i % 3])
        add("colvec_dot_batched", m=rows, count=3)
    for n in DOT_SIZES:
        add("dot", n=n)
    for i, m in enumerate(MATVEC_M):
        for j, n in enumerate(MATVEC_N):
            add("matvec", m=m, n=n, base=BASE_MODES[(i + j) % 3])
        add("matvec", m=m, n=0, base="distinct")
    for kernel in ("tall_matvec", "tall_matvec_f32"):
        for i, rows in enumerate(TALL_ROWS):
            for j, ncols in enumerate(TALL_COLS):
                add(kernel, rows=rows, ncols=ncols, base=BASE_MODES[(i + j) % 3])
    for i, n in enumerate(DOT8_N):
        for j, m in enumerate(DOT8_M):
            add("colvec_dot_f32", m=m, n=n, base=("alias", "null", "alias", "distinct")[(i + j) % 4])
    for n in SYMV_SIZES:
        add("symv_lower_batched", n=n, count=3)
    return out


def reduction_problem(case):
    """The inputs of a reduction case and its canonical form: dict(F = [outputs x terms, outputs x terms], k, alpha, beta,
    base (per output, or None)) plus the arrays the kernel is given."""
    kern = case["kernel"]
    rng = rng_of(*[v for v in case.values() if isinstance(v, int)], len(kern))
    p = dict(alpha=1.0, beta=0.0, base=None)
    mode = case.get("base", "null")
    if kern == "coldot":
        n, m = case["n"], case["m"]
        p["A"], p["B"] = rng.standard_normal((n, m)), rng.standard_normal((n, m))
        p["alpha"], p["beta"], p["base"] = -0.75, (0.0 if mode == "null" else 1.0), base_of(mode, rng, m)
        p["F"], p["k"] = [p["A"].T.copy(), p["B"].T.copy()], n
    elif kern == "dot":
        n = case["n"]
        p["a"], p["b"] = rng.standard_normal(n), rng.standard_normal(n)
        p["F"], p["k"] = [p["a"][None, :], p["b"][None, :]], n
    elif kern in ("matvec", "tall_matvec", "tall_matvec_f32"):
        rows, cols = (case["m"], case["n"]) if kern == "matvec" else (case["rows"], case["ncols"])
        W = rng.standard_normal((rows, cols))
        if kern == "tall_matvec_f32":
            W = W.astype(np.float32)
        p["W"], p["x"] = W, rng.standard_normal(cols)
        p["alpha"], p["beta"], p["base"] = -1.25, (0.0 if mode == "null" else 0.5), base_of(mode, rng, rows)
        p["F"], p["k"] = [W.astype(np.float64), np.broadcast_to(p["x"], (rows, cols))], cols
    elif kern in ("colvec_dot", "colvec_dot_f32"):
        m, n = case["m"], case["n"]
        W = rng.standard_normal((m, n))
        if kern == "colvec_dot_f32":
            W = W.astype(np.float32)
        p["W"], p["v"] = W, rng.standard_normal(m)
        p["alpha"], p["beta"], p["base"] = -1.0, (0.0 if mode == "null" else 1.0), base_of(mode, rng, n)
        p["F"], p["k"] = [W.T.astype(np.float64), np.broadcast_to(p["v"], (n, m))], m
    elif kern == "colvec_dot_strided":
        m, n, count = case["m"], case["n"], case["count"]
        p["W"], p["v"] = rng.standard_normal((count, m, n)), rng.standard_normal((count, m))
        p["alpha"], p["beta"] = 0.5, (0.0 if mode == "null" else -1.0)
        p["base"] = None if mode == "null" else rng.standard_normal(count * n)
        p["F"] = [np.concatenate([w.T for w in p["W"]]), np.concatenate([np.broadcast_to(v, (n, m)) for v in p["v"]])]
        p["k"] = m
    elif kern == "colvec_dot_batched":
        m, count = case["m"], case["count"]
        p["Q"], p["z"] = rng.standard_normal((count, m, m)), rng.standard_normal((count, m))
        p["F"] = [np.concatenate([q.T for q in p["Q"]]), np.concatenate([np.broadcast_to(z, (m, m)) for z in p["z"]])]
        p["k"] = m
    elif kern == "symv_lower_batched":
        n, count = case["n"], case["count"]
        G = rng.standard_normal((count, n, n))
        p["K"] = np.stack([np.tril(g) + np.tril(g, -1).T for g in G])  # symmetric; the kernel is given the lower triangle
        p["p"] = rng.standard_normal((count, n))
        p["F"] = [np.concatenate(list(p["K"])), np.concatenate([np.broadcast_to(v, (n, n)) for v in p["p"]])]
        p["k"] = n
    else:
        raise ValueError(kern)
    return p


def canonical_bound(p):
    return reference_and_bound(p["F"], p["k"], p["alpha"], p["beta"], p["base"])


# ---- contract_combinations ----------------------------------------------------------------------------------------
def contract_cases():
    """(na, nb, symmetric, offsets, coefficients): every pair of sizes, the four input modes in turn; symmetric (na = nb,
    one member list for both sides) with and without lists."""
    out = []
    for i, na in enumerate(CONTRACT_SIZES):
        for j, nb in enumerate(CONTRACT_SIZES):
            mode = (i + j) % 4
            out.append(dict(na=na, nb=nb, symmetric=0, offsets=mode & 1, coefficients=(mode >> 1) & 1))
        out.append(dict(na=na, nb=na, symmetric=1, offsets=i % 2, coefficients=i % 2))
        out.append(dict(na=na, nb=na, symmetric=1, offsets=1 - i % 2, coefficients=1))
    for c in out:
        c["id"] = "contract-" + "-".join(f"{k}{v}" for k, v in c.items())
    return out


def member_offsets(rng, count):
    """Member lists of 0 .. 4 points, an empty one among them (the first of a single list has one point)."""
    sizes = rng.integers(0, 5, count)
    sizes[count // 2] = 0
    if sizes.sum() == 0:
        sizes[0] = 1
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def contract_problem(case):
    na, nb, sym = case["na"], case["nb"], case["symmetric"]
    rng = rng_of(na, nb, sym, case["offsets"], case["coefficients"])
    xoff = member_offsets(rng, na) if case["offsets"] else None
    yoff = xoff if sym else (member_offsets(rng, nb) if case["offsets"] else None)
    nx = int(xoff[-1]) if xoff is not None else na
    ny = int(yoff[-1]) if yoff is not None else nb
    K = rng.standard_normal((nx, ny))
    if sym:
        K = np.tril(K) + np.tril(K, -1).T
    xc = rng.standard_normal(nx) if case["coefficients"] else None
    yc = xc if (sym and xc is not None) else (rng.standard_normal(ny) if case["coefficients"] else None)
    return dict(K=K, xoff=xoff, yoff=yoff, xc=xc, yc=yc, nx=nx, ny=ny)


def contract_reference(case, p, evaluate=None):
    """(ref, bound) as na x nb arrays; evaluate(xc_a, K_ab, yc_b) (optional) gives a plain fp64 result to compare instead."""
    na, nb = case["na"], case["nb"]
    xoff = p["xoff"] if p["xoff"] is not None else np.arange(na + 1)
    yoff = p["yoff"] if p["yoff"] is not None else np.arange(nb + 1)
    xc = p["xc"] if p["xc"] is not None else np.ones(p["nx"])
    yc = p["yc"] if p["yc"] is not None else np.ones(p["ny"])
    ld = np.longdouble if HAVE_LONGDOUBLE else np.float64
    ref, bound, plain = np.zeros((na, nb), dtype=ld), np.zeros((na, nb)), np.zeros((na, nb))
    for a in range(na):
        ca = xc[xoff[a]:xoff[a + 1]]
        for b in range(nb):
            cb = yc[yoff[b]:yoff[b + 1]]
            Kab = p["K"][xoff[a]:xoff[a + 1], yoff[b]:yoff[b + 1]]
            if Kab.size:
                F = [(ca[:, None] * np.ones(len(cb))).reshape(1, -1), Kab.reshape(1, -1), (np.ones(len(ca))[:, None] * cb).reshape(1, -1)]
                r, bd = reference_and_bound(F, len(ca) + len(cb))
                ref[a, b], bound[a, b] = r[0], bd[0]
            if evaluate is not None:
                plain[a, b] = evaluate(ca, Kab, cb)
    return (ref, bound, plain) if evaluate is not None else (ref, bound)


# ---- loo and axpby ------------------------------------------------------------------------------------------------
def loo_problem(n):
    rng = rng_of(n, 77)
    return dict(d=rng.uniform(0.5, 4.0, n) * rng.choice([-1.0, 1.0], n), y=rng.standard_normal(n), info=rng.standard_normal(n))


def loo_reference(p):
    """((mean, bound), (variance, bound))."""
    ld = np.longdouble if HAVE_LONGDOUBLE else np.float64
    q = p["info"].astype(ld) / p["d"].astype(ld)
    var = ld(1.0) / p["d"].astype(ld)
    mean_bound = U * (2.0 + U) * (np.abs(p["y"]) + np.abs(q).astype(np.float64))
    return (p["y"].astype(ld) - q, mean_bound), (var, U * np.abs(var).astype(np.float64))


def axpby_problem(n, mode):
    """mode: 'both', 'x_null' (out = b y), 'y_null' (out = a x + b)."""
    rng = rng_of(n, len(mode))
    return dict(a=1.75, b=-0.3, x=None if mode == "x_null" else rng.standard_normal(n),
                y=None if mode == "y_null" else rng.standard_normal(n))


def axpby_reference(p, n):
    ld = np.longdouble if HAVE_LONGDOUBLE else np.float64
    ax = ld(p["a"]) * p["x"].astype(ld) if p["x"] is not None else np.zeros(n, dtype=ld)
    by = ld(p["b"]) * (p["y"].astype(ld) if p["y"] is not None else np.ones(n, dtype=ld))
    return ax + by, U * (2.0 + U) * (np.abs(ax) + np.abs(by)).astype(np.float64)


# ---- movers: numpy restatements on the buffers' views ---------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def lower_source(n):
    """A random n x n matrix (every entry finite) at the factor's leading dimension, NaN padding rows: (flat, view)."""
    rng = rng_of(n, 5)
    return nan_padded(rng.standard_normal((n, n)), factor_ld(n))


def pair_written_mask(n):
    """What copy_lower / convert_lower_f32 may write: the lower triangle and the entry above the diagonal of odd columns."""
    mask = np.tril(np.ones((n, n), dtype=bool))
    j = np.arange(1, n, 2)
    mask[j - 1, j] = True
    return mask


def nan_positions(n):
    """(row, column, what) at which a NaN must raise the flag of copy_lower / nan_scan_lower.  At an odd n the last row
    of every column is copy_lower_kernel's scalar tail (a pair starts at an even row), at an even n the second of a pair."""
    last = n - 1
    tail = "scalar tail" if n % 2 else "second of the last pair"
    pos = {(last, 0): "last row, " + tail, (last, last): "diagonal of the last column"}
    if n > 2048:
        pos[(2048, 2048)] = "first column of the relaunch, its diagonal"
        pos[(last, 2048)] = "first column of the relaunch, last row, " + tail
    if n >= 2:
        pos.setdefault((1, 1), "diagonal of an odd column")
        pos.setdefault((last, 1), "last row of an odd column, " + tail)
    if n >= 4:
        pos.setdefault((2, 1), "first of a pair below the diagonal")
    return [(r, c, what) for (r, c), what in sorted(pos.items())]
