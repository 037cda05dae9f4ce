"""Shared by tests/test_gram_matvec_host.py and tests/test_gram_matvec_gpu.py: the shapes, the covariance trees, the bound and a
float64 restatement of agp_gram_matvec (csrc/gram_matvec.hip):  out[:, c] = (k(x, x) + diag(y_var)) V[:, c].

The bound.  With A = K + diag(y_var) formed in float64 from K = ctx.gram(cov, x) - the kernel's entries are these bits,
and it adds y_var_i to K_ii with the same single rounding before the product - and r = A V in np.longdouble:

    |out_ic - r_ic|  <=  gamma(L + S) sum_j |A_ij| |V_jc|,      gamma(m) = m u / (1 - m u),  u = 2^-53

from the kernel's summation structure, nothing measured:
  * one lane owns row i and walks the columns of its slice in order, acc = fma(A_ij, V_jc, acc): one rounding per step,
    so a term passes through at most L roundings, L = the columns of the longest slice (the slots past the end of a
    ragged tile multiply a zero of V: fma(a, 0, acc) = acc exactly).  There is no LDS or shuffle tree: a row never leaves
    its lane.
  * the S partial sums of an entry are added one after the other in slice order: at most S - 1 further roundings.
  * one more u covers the conversion of the longdouble reference (its own error is n 2^-64 of the same sum).
V is standard normal with signs, so the sums cancel and the bound stays relative to sum |A| |V|.

Entry parity: with V = columns of the identity, out is the corresponding columns of A bit for bit - fma(a, 1, 0) = a and
fma(a, 0, acc) = acc are exact, and so is the sum of one value and zeros over the slices.
"""
import ctypes as C
import functools

import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi

import gram_path_cases as gp
from gram_path_cases import canaries, all_canary, radial, noise, E, R, A  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -53
# csrc/gram_matvec.h
MV_ROWS, MV_COLS, MV_MAX_RHS, MV_MIN_SLICE, MV_TARGET_WGS = 256, 64, 16, 256, 1024
FAST, SOP, INTERP = 0, 1, 2
PATH_NAMES = ["FAST", "SOP", "INTERP"]
HAVE_LONGDOUBLE = gp.HAVE_LONGDOUBLE


def slices(n):
    """(S, columns per slice): csrc/gram_matvec.hip: gram_matvec_slices"""
    row_tiles = -(-n // MV_ROWS)
    want = max(1, min(-(-MV_TARGET_WGS // row_tiles), -(-n // MV_MIN_SLICE)))
    cps = -(-(-(-n // want)) // MV_COLS) * MV_COLS
    return -(-n // cps), cps


def chunk_widths(nrhs):
    """the kernel widths (1, 4 or 16) of the chunks a call with nrhs right-hand sides makes, and their column counts"""
    out, left = [], nrhs
    while left > 0:
        t = MV_MAX_RHS if left >= 5 else (4 if left >= 2 else 1)
        out.append((t, min(left, t)))
        left -= min(left, t)
    return out


def gamma(m):
    return m * U / (1. - m * U)


def bound_factor(n):
    S, cps = slices(n)
    return gamma(min(cps, n) + S)


# ---- shapes -------------------------------------------------------------------------------------------------------------
# 1, 2; the column tile - 1, the tile, + 1; the row tile - 1, the row tile = the largest n that runs unsplit, + 1 = the first n
# that splits (two slices of 192 columns, the last one ragged: 65 = one tile and one column); three row tiles and three
# slices (513: last slice 129 columns); four slices of 256 whose last holds 9 columns (777)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 513, 777]
NRHS = [1, 2, 3, 8, 15, 16, 17, 33]
LARGEST_UNSPLIT, FIRST_SPLIT = 256, 257
PATH_N = 257     # every path: two row tiles, two slices, a ragged last tile
PATH_NRHS = 17   # a chunk of 16 and a chunk of 1


def points(n, dim, seed):
    """uniform in [0.5, 10)^dim with a duplicated point when there is room (the noise term off the diagonal)"""
    x, _ = gp.planted_symmetric(n, dim, seed)
    return x


def right_hand_sides(n, nrhs, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, nrhs)))


def variances(n, seed):
    return np.random.default_rng(seed).uniform(0.01, 0.5, n)


# ---- covariance trees: (name, builder, dims, expected path) ----------------------------------------------------------------
def _interp_tree():
    """a sum inside a product: not a sum of products, the postfix interpreter keeps it"""
    return (radial(0, 2.0, 1.1, E) + radial(1, 5.0, 0.9, E)) * radial(3, 3.0, 0.7, E) + noise()


TREES = [(f"fast_{gp.RADIAL_IDS[op]}_{kind}", functools.partial(gp.fast_cov, op, kind), (1, 2, 3), FAST)
         for op in range(4) for kind in ("none", "noise")]
TREES += [
    ("fast_m52_meas", functools.partial(gp.fast_cov, 3, "meas"), (1, 2, 3), FAST),
    ("fast_se_4d", functools.partial(gp.fast_cov, 0, "noise"), (4,), SOP),           # dim > 3: off the fast path
    ("sop_generic", gp.generic_cov, (3, 5, 8), SOP),
    ("sop_generic_noise", gp.generic_noise_cov, (3,), SOP),
    ("sop_radial_metric", lambda: radial(0, 4.0, 1.2, R), (1, 3), SOP),              # non-Euclidean: a pair-2 tree of agp_gram
    ("sop_angular_metric", lambda: radial(1, 1.1, 1.0, A) * radial(3, 4.0, 1.2, E), (2, 3), SOP),
    ("sop_scaling", lambda: gp._rank1() + noise() + radial(1, 1.1, 1.0, A) * radial(0, 6.0, 3.7, R), (2, 3), SOP),
    ("interp_sum_in_product", _interp_tree, (1, 3, 4), INTERP),
    ("interp_scaling", lambda: (gp._rank1() + radial(0, 2.0, 1.0, E)) * radial(2, 3.0, 0.8, R) + noise(), (3,), INTERP),
]


def tree_cases():
    return [(name, dim) for name, _, dims, _ in TREES for dim in dims]


def tree(name):
    for nm, build, _, path in TREES:
        if nm == name:
            return build(), path
    raise KeyError(name)


# (measurement flag, ids): the feature variants every noise-carrying tree is run with
FEATURE_VARIANTS = [(False, False), (True, False), (False, True), (True, True)]


def make_features(cov, x, meas, ids, seed=5):
    """FeatureSet of x; ids: explicit equality ids under which point 0 and point n - 1 are ONE feature although
    planted_symmetric made n - 1 a copy of 0 only for n > 8, and points 1 and 3 (equal coordinates for n > 4) are two"""
    if not ids:
        return gp.features(cov, x, meas=meas)
    n = len(x)
    eq = np.arange(n, dtype=np.int64) + 100
    if n > 1:
        eq[n - 1] = eq[0]
    return gp.features(cov, x, meas=meas, ids=eq)


def gram_argument(fs):
    """what Context.gram / ab.gram_matvec take for this FeatureSet (the Measurement tag keeps its flag)"""
    return ab.Measurement(fs) if fs.is_measurement else fs


# ---- reference, bound, restatement -------------------------------------------------------------------------------------------
def system_matrix(K, y_var):
    Am = np.array(K, dtype=np.float64, order="F")
    if y_var is not None:
        Am[np.diag_indices_from(Am)] = np.diag(Am) + y_var  # one float64 rounding, as the kernel's
    return Am


def reference(Am, V):
    """(r in longdouble, sum_j |A_ij| |V_jc|)"""
    r = Am.astype(np.longdouble) @ np.asarray(V, dtype=np.float64).astype(np.longdouble)
    return r, np.abs(Am) @ np.abs(V)


def within_bound(out, Am, V):
    """(ok, worst fraction of the bound)"""
    n = Am.shape[0]
    r, Sabs = reference(Am, V)
    err = np.abs(out.astype(np.longdouble) - r).astype(np.float64)
    bound = bound_factor(n) * Sabs
    frac = float(np.max(err / np.where(bound > 0., bound, 1.))) if err.size else 0.
    return bool(np.all(np.isfinite(out)) and np.all(err <= bound)), frac


def restatement(Am, V):
    """float64, the kernel's order: per slice the columns one after the other (a rounded product, a rounded sum: one more
    rounding per step than the kernel's fma, within the same count of roundings per term), then the slices in order"""
    n = Am.shape[0]
    V = np.asarray(V, dtype=np.float64).reshape(n, -1)
    S, cps = slices(n)
    total = None
    for s in range(S):
        acc = np.zeros((n, V.shape[1]))
        for j in range(s * cps, min(n, (s + 1) * cps)):
            acc = acc + Am[:, j:j + 1] * V[j:j + 1, :]
        total = acc if total is None else total + acc
    return total


def identity_block(n, first, count):
    """columns first .. first + count - 1 of the n x n identity"""
    Vm = np.zeros((n, count), order="F")
    for c in range(count):
        Vm[first + c, c] = 1.
    return Vm


# ---- the C-ABI call with canaries -------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def call(ctx, cov, fs, V, y_var=None, ldv=None, ldo=None, extra_cols=0):
    """agp_gram_matvec on host arrays: (status, out (n x nrhs), the padding rows of out, the columns beyond nrhs).  V is
    copied into a block of leading dimension ldv whose padding rows are canaries; out goes in full of canaries."""
    n, nrhs = V.shape
    ldv = n if ldv is None else ldv
    ldo = n if ldo is None else ldo
    Vb = canaries(ldv * nrhs).reshape(ldv, nrhs, order="F")
    Vb[:n] = V
    ob = canaries(ldo * (nrhs + extra_cols)).reshape(ldo, nrhs + extra_cols, order="F")
    s = fs.as_struct()
    yv = None if y_var is None else np.ascontiguousarray(y_var, dtype=np.float64)
    st = ctx._lib.agp_gram_matvec(ctx._h, ctx.kernel(cov), C.byref(s), _p(yv), _p(Vb), ldv, nrhs, _p(ob), ldo, capi.HOST)
    return st, ob[:n, :nrhs], ob[n:, :nrhs], ob[:, nrhs:]


@functools.lru_cache(maxsize=1)
def debug_lib():
    lib = capi.load_debug()
    lib.agp_debug_gram_matvec_plan.restype = C.c_int
    lib.agp_debug_gram_matvec_plan.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.Features), C.c_int64, C.c_void_p]
    return lib


def plan(ctx, cov, fs, nrhs=1):
    """agp_debug_gram_matvec_plan: [path, S, columns per slice, rows of a workgroup, columns of a tile, width of the first chunk]"""
    out = np.full(6, -1, dtype=np.int64)
    s = fs.as_struct()
    st = debug_lib().agp_debug_gram_matvec_plan(ctx._h, ctx.kernel(cov), C.byref(s), nrhs, _p(out))
    assert st == 0, st
    return out.tolist()
