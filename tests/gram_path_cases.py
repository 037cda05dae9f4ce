"""Shared by tests/test_gram_paths_host.py and tests/test_gram_paths_gpu.py: the case tables, the feature constructions, the
ctypes prototypes of the three debug entry points (csrc/debug_api.hip: agp_debug_gram, agp_debug_gram_blocks,
agp_debug_predict_mean), the canary fill and the reference of the predictive mean for the kernels of csrc/gram.hip and
csrc/gram_fast.h.

Every launch reports the path its dispatcher chose (csrc/common.h: GramPath, PredictMeanPath; the launcher switches on the
same gram_select_path / predict_mean_select_path call), and every case asserts that path first.

Gram entries: oracle_py.gram (the C restatement in the reference's own operation order) under the bar of
tests/test_gram_gpu.py, 4e-16 max|K| + 2e-14 |value| (derived in that file's header; csrc/gram_fast.h states its 10x margin).

Predictive mean: r_j = sum_i K[i, j] alpha_i with K from oracle_py.gram and the products and the sum in np.longdouble;

    |got_j - r_j|  <=  ((ceil(N / 64) + 12) eps + 2e-14) sum_i |K[i, j]| |alpha_i|

ceil(N / 64) fp64 additions in one lane's chain, 6 of the shuffle tree, 2 of the LDS tree of the 256-thread kernel, one
rounding of each product and of the reference's conversion (12 covers them; the tiled kernel's chains are four times
shorter); 2e-14 is the per-entry bar of K above.  alpha is standard normal with signs, so the sums cancel and the bound
stays relative to sum |K| |alpha|.  Nothing here is measured.

Canaries: NaN with all 64 bits set, compared as uint64 (tests/test_kernels_gpu.py: test_forward_solve_wide).
"""
import ctypes as C
import functools

import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi
from oracle import oracle_py as orc

EPS = float(np.finfo(np.float64).eps)
TM, TN = 128, 32  # csrc/gram_fast.h

# csrc/common.h
FAST_TRI, FAST_RECT, PAIR2, SOP, INTERP = range(5)
GRAM_PATH_NAMES = ["FAST_TRI", "FAST_RECT", "PAIR2", "SOP", "INTERP"]
TILED8, TILED4, FAST_WAVE, PM_SOP, PM_INTERP = range(5)
PM_PATH_NAMES = ["TILED8", "TILED4", "FAST_WAVE", "SOP", "INTERP"]

RADIALS = [ab.SquaredExponential, ab.Exponential, ab.Matern32, ab.Matern52]
RADIAL_IDS = ["se", "exp", "m32", "m52"]
NOISE_SIGMA = 0.3
MEAS_COMBOS = [(False, False), (False, True), (True, False), (True, True)]


# ---- canaries --------------------------------------------------------------------------------------------------------
CANARY_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def canaries(count):
    return np.full(int(count), CANARY_BITS, dtype=np.uint64).view(np.float64)


def all_canary(a):
    a = np.ascontiguousarray(a)
    return bool(np.all(a.view(np.uint64) == CANARY_BITS))


def close(got, want):
    """the bar of tests/test_gram_gpu.py"""
    scale = np.abs(want).max() if want.size else 1.
    return bool(np.all(np.abs(got - want) <= 4e-16 * scale + 2e-14 * np.abs(want)))


def close_nan(got, want):
    """close() where the reference is finite, NaN exactly where it is NaN"""
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    if nan.all():
        return True
    scale = np.abs(want[~nan]).max()
    return bool(np.all(np.abs(got[~nan] - want[~nan]) <= 4e-16 * scale + 2e-14 * np.abs(want[~nan])))


# ---- the debug entry points --------------------------------------------------------------------------------------------
_P, _PF = C.c_void_p, C.POINTER(capi.Features)


@functools.lru_cache(maxsize=1)
def debug_lib():
    lib = capi.load_debug()
    lib.agp_debug_gram.restype = C.c_int
    lib.agp_debug_gram.argtypes = [_P, _P, _PF, _PF, C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]
    lib.agp_debug_gram_blocks.restype = C.c_int
    lib.agp_debug_gram_blocks.argtypes = [_P, _P, _PF, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P, C.POINTER(C.c_int)]
    lib.agp_debug_predict_mean.restype = C.c_int
    lib.agp_debug_predict_mean.argtypes = [_P, _P, _PF, _PF, _P, _P, C.POINTER(C.c_int)]
    return lib


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def features(cov, coords, meas=False, ids=None):
    """FeatureSet of `coords` (n x dim) for `cov` (its ScalingTerm columns evaluated), optionally with explicit equality ids"""
    fs = cov.features(np.asarray(coords, dtype=np.float64), is_measurement=meas)
    if ids is None:
        return fs
    return ab.FeatureSet(fs.coords, None if fs.scales is None else list(fs.scales.T), np.asarray(ids, dtype=np.int64), meas)


def run_gram(ctx, cov, fx, fy=None, lower_only=False, ld=None, offset=0, diag_add=None):
    """agp_debug_gram: (K, rest, before, flag, path) - K the rows x cols matrix as stored, `rest` the padding rows
    (ld - rows) x cols, `before` the `offset` elements in front of the matrix.  The buffer goes in full of canaries."""
    rows, cols = fx.n, (fx.n if fy is None else fy.n)
    ld = rows if ld is None else ld
    buf = canaries(offset + ld * cols)
    sx = fx.as_struct()
    sy = None if fy is None else fy.as_struct()
    d = None if diag_add is None else np.ascontiguousarray(diag_add, dtype=np.float64)
    assert d is None or d.shape == (cols,)
    flag, path = C.c_int(-1), C.c_int(-1)
    st = debug_lib().agp_debug_gram(ctx._h, ctx.kernel(cov), C.byref(sx), None if sy is None else C.byref(sy),
                                    1 if fy is None else 0, 1 if lower_only else 0, ld, offset, _ptr(d), _ptr(buf),
                                    C.byref(flag), C.byref(path))
    assert st == 0, st
    M = buf[offset:].reshape(ld, cols, order="F")
    return M[:rows], M[rows:], buf[:offset], flag.value, path.value


def run_gram_blocks(ctx, cov, fx, rows, count, ld, stride, diag_add):
    """agp_debug_gram_blocks: (the whole buffer, launched)"""
    buf = canaries((count - 1) * stride + ld * rows)
    sx = fx.as_struct()
    d = None if diag_add is None else np.ascontiguousarray(diag_add, dtype=np.float64)
    assert d is None or d.shape == (rows * count,)
    launched = C.c_int(-1)
    st = debug_lib().agp_debug_gram_blocks(ctx._h, ctx.kernel(cov), C.byref(sx), rows, count, ld, stride, _ptr(d), _ptr(buf),
                                           C.byref(launched))
    assert st == 0, st
    return buf, launched.value


def run_predict_mean(ctx, cov, fx, fxs, alpha):
    """agp_debug_predict_mean: (mean (M), the two trailing elements, path)"""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    assert alpha.shape == (fx.n,)
    buf = canaries(fxs.n + 2)
    sx, sxs = fx.as_struct(), fxs.as_struct()
    path = C.c_int(-1)
    st = debug_lib().agp_debug_predict_mean(ctx._h, ctx.kernel(cov), C.byref(sx), C.byref(sxs), _ptr(alpha), _ptr(buf),
                                            C.byref(path))
    assert st == 0, st
    return buf[:fxs.n], buf[fxs.n:], path.value


# ---- covariance functions ----------------------------------------------------------------------------------------------
class Elevation(ab.ScalingFunction):
    """the temperature example's scaling, on the first coordinate"""
    _params = {"center": 4.0, "factor": 0.3}

    def _call_impl(self, c):
        return 1. + self._params["factor"] * np.maximum(self._params["center"] - np.asarray(c)[:, 0], 0.)


def radial(op, length_scale=2.5, sigma=1.3, metric=None):
    return RADIALS[op](length_scale, sigma, metric() if metric else None)


def noise():
    return ab.IndependentNoise(NOISE_SIGMA)


def fast_cov(op, kind, length_scale=2.5):
    """the fast shapes (csrc/gram.hip: match_fast): radial<Euclidean> alone ('none'), + noise ('noise'), + measurement-only
    noise ('meas'); the nugget has the noise's node shape ('nugget')"""
    r = radial(op, length_scale)
    if kind == "none":
        return r
    if kind == "noise":
        return r + noise()
    if kind == "nugget":
        return r + ab.Nugget(NOISE_SIGMA)
    assert kind == "meas"
    return r + ab.measurement_only(noise())


E, R, A = ab.EuclideanDistance, ab.RadialDistance, ab.AngularDistance


def _rank1():
    return ab.ScalingTerm(Elevation()) * ab.Constant(0.8)


# (name, builder, dims, (EUCLID, ANGULAR) of the gram_pair2_kernel instantiation): csrc/gram.hip: match_pair2
PAIR2_TREES = [
    # one radial leaf
    ("const+m32_e", lambda: ab.Constant(0.7) + radial(2, 3.0, 1.1, E), (1, 2, 3), (True, False)),
    ("se_r", lambda: radial(0, 4.0, 1.2, R), (1, 2, 3), (False, False)),
    ("exp_a", lambda: radial(1, 1.1, 1.0, A), (2, 3), (False, True)),
    # two radial leaves
    ("m32_e*exp_e+nugget", lambda: radial(2, 3.0, 2.0, E) * radial(1, 5.0, 1.5, E) + ab.Nugget(NOISE_SIGMA), (1, 2, 3), (True, False)),
    ("m52_r*se_r+noise", lambda: radial(3, 3.0, 0.9, R) * radial(0, 6.0, 1.4, R) + noise(), (1, 2, 3), (False, False)),
    ("exp_a*m52_e", lambda: radial(1, 1.1, 1.0, A) * radial(3, 4.0, 1.2, E), (2, 3), (True, True)),
    ("m32_a*exp_a+noise", lambda: radial(2, 0.9, 1.0, A) * radial(1, 1.7, 0.8, A) + noise(), (2, 3), (False, True)),
    # the temperature example's shape (examples/temperature_example/temperature_example.cc:34-85)
    ("temperature", lambda: _rank1() + noise() + radial(1, 1.1, 1.0, A) * radial(0, 6.0, 3.7, R), (2, 3), (False, True)),
    ("scaling_only+se_e*exp_a", lambda: ab.ScalingTerm(Elevation()) + radial(0, 4.0, 1.0, E) * radial(1, 1.3, 1.1, A), (2, 3), (True, True)),
    ("const*scaling+m52_e", lambda: ab.Constant(0.8) * ab.ScalingTerm(Elevation()) + radial(3, 2.0, 1.0, E), (1, 3), (True, False)),
    # the three positions of the noise term in the sum
    ("noise,rad,rank1", lambda: noise() + radial(2, 3.0, 1.1, E) + _rank1(), (1, 2, 3), (True, False)),
    ("rad,noise,rank1", lambda: radial(2, 3.0, 1.1, E) + noise() + _rank1(), (1, 2, 3), (True, False)),
    ("rad,rank1,noise", lambda: radial(2, 3.0, 1.1, E) + _rank1() + noise(), (1, 2, 3), (True, False)),
    # each term measurement-only in turn
    ("meas(rad)", lambda: ab.measurement_only(radial(1, 3.0, 1.1, R)) + _rank1() + noise(), (1, 2, 3), (False, False)),
    ("meas(rank1)", lambda: radial(1, 3.0, 1.1, R) + ab.measurement_only(_rank1()) + noise(), (1, 2, 3), (False, False)),
    ("meas(noise)", lambda: radial(1, 3.0, 1.1, R) + _rank1() + ab.measurement_only(noise()), (1, 2, 3), (False, False)),
]


def generic_cov():
    """three terms, the first of three factors: a sum of products that matches neither fast shape at any dimension"""
    return (radial(0, 2.0, 1.1, E) * radial(1, 5.0, 0.9, R) * ab.Constant(1.2) + radial(3, 3.0, 0.7, A)
            + ab.measurement_only(noise()))


def generic_noise_cov():
    """the same with plain noise: the equality branches of the generic evaluators"""
    return radial(0, 2.0, 1.1, E) * radial(1, 5.0, 0.9, R) * ab.Constant(1.2) + radial(3, 3.0, 0.7, A) + noise()


def generic_radial_cov():
    """a product of three factors plus noise without the angular metric: the generic evaluators at dim 1 and 2"""
    return radial(0, 2.0, 1.1, E) * radial(1, 5.0, 0.9, R) * ab.Constant(1.2) + radial(2, 3.0, 0.7, R) + noise()


FAST_KINDS = ["none", "noise", "meas", "nugget"]


# ---- feature vectors with planted pairs -----------------------------------------------------------------------------------
def planted_cross(rows, cols, dim, seed):
    """x (rows x dim), y (cols x dim) uniform in [0.5, 10) and the pairs planted in them:
        equal      (i, j) with y[j] == x[i] in every coordinate: the noise term appears there
        near       (i, j) equal in all but the last coordinate (dim >= 2): no noise
        underflow  (i, j) 1e-170 apart in the first coordinate, equal in the others: the squared distance underflows to
                   exactly 0 but the features differ: no noise
    Every other pair differs (continuous draws)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 10., (rows, dim))
    y = rng.uniform(0.5, 10., (cols, dim))
    equal, near, underflow = [], [], []
    big = cols > 9
    u = min(3, rows - 1)
    if big:
        x[u, 0] = 0.
    y[0] = x[rows - 1]  # the last row: in the edge tile, and the single-row store of an odd row count
    equal.append((rows - 1, 0))
    if cols >= 2:
        y[cols - 1] = x[0]  # the last column: the second of a pair, or the `two` guard of an odd column count
        equal.append((0, cols - 1))
    if big:
        y[9] = x[u]
        y[9, 0] = 1e-170
        underflow.append((u, 9))
        v = min(7, rows - 1)
        y[6] = x[v]  # equal pair in the middle of a tile
        equal.append((v, 6))
        if dim >= 2:
            y[5] = x[v]
            y[5, dim - 1] += 0.25
            near.append((v, 5))
    return x, y, dict(equal=equal, near=near, underflow=underflow)


def planted_symmetric(n, dim, seed):
    """x (n x dim) with x[3] = x[1] when n > 4 and the last point a copy of point 0 when n > 8 (off-diagonal noise)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 10., (n, dim))
    equal = [(i, i) for i in range(n)]
    if n > 4:
        x[3] = x[1]
        equal += [(3, 1), (1, 3)]
    if n > 8:
        x[n - 1] = x[0]
        equal += [(n - 1, 0), (0, n - 1)]
    return x, equal


def planted_ids(rows, cols, dim, seed):
    """x, y, x_ids, y_ids and the pairs: `equal_ids` - the ids agree (noise whenever both sides carry ids), some of them at
    different coordinates; `equal_coords` - the coordinates agree (noise whenever a side has no ids), some of them under
    different ids."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 10., (rows, dim))
    y = rng.uniform(0.5, 10., (cols, dim))
    xi = np.arange(rows, dtype=np.int64)
    yi = 1000000 + np.arange(cols, dtype=np.int64)
    a, b, c = rows - 1, min(2, rows - 1), 0
    ja, jb, jc = cols - 1, min(1, cols - 1), 0
    equal_ids, equal_coords = [], []
    y[ja] = x[a]; yi[ja] = xi[a]          # same point, same id
    equal_ids.append((a, ja)); equal_coords.append((a, ja))
    if cols >= 3 and rows >= 3:
        yi[jb] = xi[b]                    # different point, same id: noise
        equal_ids.append((b, jb))
        y[jc] = x[c]                      # same point, different id: no noise
        equal_coords.append((c, jc))
    return x, y, xi, yi, dict(equal_ids=equal_ids, equal_coords=equal_coords)


# ---- shapes ----------------------------------------------------------------------------------------------------------------
# (a) the fast rectangular kernel on a cross Gram: one column, 31 / 32 / 33 columns (the `two` guard, a full tile, one
# column in a second tile), odd and even row counts past one tile (the single-row store), two columns of tiles
FAST_CROSS_SHAPES = [(1, 1), (129, 1), (129, 31), (130, 32), (130, 33), (257, 63), (2, 65)]
FAST_NOISE_KINDS = [("none", (False, False)), ("noise", (False, False))] + [("meas", m) for m in MEAS_COMBOS]


def cross_lds(rows):
    return [rows, rows + 1, rows + 3]


# (b) lower_only, diag_add
LOWER_SIZES = [1, 2, 127, 128, 129, 257]
TRI_LARGE = 2049  # 17 row tiles: the sqrt inversion of the workgroup index, with its two correction loops
# (c) / (e) / (f)
PAIR2_SHAPE = (129, 33)
# (d) the generic evaluators at DIMP 4 and 8
GENERIC_DIMS = [4, 5, 8]
# (g) launch_gram_blocks
BLOCK_ROWS = [1, 31, 128, 129, 200]
BLOCK_COUNTS = [1, 3]
# (h) predict mean
PM_M = [1, 3, 4, 5, 1023, 1024, 1025, 1026, 1027, 16383, 16384, 16385, 16391]
PM_N = [1, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 513]


def predict_mean_shapes():
    """(N, M): every M with N = 257, every N with M = 1027, every N with M = 5"""
    out = [(257, m) for m in PM_M]
    out += [(n, 1027) for n in PM_N if (n, 1027) not in out]
    out += [(n, 5) for n in PM_N if (n, 5) not in out]
    return out


def expected_fast_pm_path(m, length_scale=1.0):
    """csrc/gram.hip: predict_mean_select_path for a fast tree"""
    if m >= 1024 and length_scale > 0.:
        return TILED8 if m >= 16384 else TILED4
    return FAST_WAVE


FAST_COMBOS = [(op, dim) for op in range(4) for dim in (1, 2, 3)]
# (kind, xs measurement): plain and measurement-only noise under both flags (the nugget has the noise's node shape)
PM_NOISE_KINDS = [("noise", False), ("meas", True), ("meas", False), ("none", False), ("nugget", True), ("noise", True)]
# which side carries equality ids: both (the ids decide), the training points only / the test points only (one pointer
# null: the comparison falls back to the coordinates, as in planted_ids), neither
ID_MODES = ["both", "x", "xs"]


def predict_mean_fast_cases():
    """(N, M, op, dim, noise kind, xs_meas, id mode or None): the (op, dim) pairs, the noise kinds and the id modes rotate
    over the shapes (the tile edges do not depend on them); every pair runs on each of the three fast kernels at one shape of
    its own, and each one-sided id mode runs on each of them with plain noise under both measurement flags."""
    out = []
    for k, (n, m) in enumerate(predict_mean_shapes()):
        op, dim = FAST_COMBOS[k % len(FAST_COMBOS)]
        kind, xs_meas = PM_NOISE_KINDS[k % len(PM_NOISE_KINDS)]
        out.append((n, m, op, dim, kind, xs_meas, ID_MODES[(k // 3) % 3] if k % 3 == 2 else None))
    for k, (op, dim) in enumerate(FAST_COMBOS):
        kind, xs_meas = PM_NOISE_KINDS[(k + 1) % len(PM_NOISE_KINDS)]
        for n, m in ((193, 16385), (257, 1026), (65, 7)):
            out.append((n, m, op, dim, kind, xs_meas, "both" if k % 4 == 1 else None))
    k = 0
    for n, m in ((193, 16391), (257, 1027), (129, 5)):  # TILED8, TILED4 (partial last tiles), FAST_WAVE
        for mode in ("x", "xs"):
            for xs_meas in (False, True):
                op, dim = FAST_COMBOS[(5 * k + 2) % len(FAST_COMBOS)]
                out.append((n, m, op, dim, "noise", xs_meas, mode))
                k += 1
    return out


def predict_mean_points(n, m, dim, seed, ids=None):
    """x (n x dim), xs (m x dim), alpha (n, standard normal), the pairs (i, j) at which the noise term appears, and the
    ids of both sides (None where a side has none).  Planted copies: xs[j] == x[i] for the last test point (of a partial
    tile whenever m is no multiple of the tile) and training point n - 1, the first test point and point 0, one in the
    middle.  ids (ID_MODES): ids are drawn as in planted_ids - the last pair under one id, xs[0] == x[0] under two ids,
    xs[1] != x[2] under one id - and handed to both sides ('both': the pairs are the equal ids) or to one side only ('x',
    'xs': the pairs are the equal coordinates, as without ids)."""
    assert ids in (None, "both", "x", "xs")
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 10., (n, dim))
    xs = rng.uniform(0.5, 10., (m, dim))
    alpha = rng.standard_normal(n)
    pairs = [(n - 1, m - 1)]
    xs[m - 1] = x[n - 1]
    if m >= 3:
        xs[0] = x[0]
        pairs.append((0, 0))
        xs[m // 2] = x[n // 2]
        pairs.append((n // 2, m // 2))
    if ids is None:
        return x, xs, alpha, pairs, None, None
    xi = np.arange(n, dtype=np.int64)
    si = 1000000 + np.arange(m, dtype=np.int64)
    si[m - 1] = xi[n - 1]          # same point, same id: noise
    id_pairs = [(n - 1, m - 1)]
    if m >= 3:                     # xs[0] == x[0] under different ids: no noise; xs[1] != x[..] under the same id: noise
        si[1] = xi[min(2, n - 1)]
        id_pairs.append((min(2, n - 1), 1))
    if ids == "both":
        return x, xs, alpha, id_pairs, xi, si
    return x, xs, alpha, pairs, (xi if ids == "x" else None), (si if ids == "xs" else None)


def tree_metrics(cov):
    """(EUCLID, ANGULAR) of the gram_pair2_kernel instantiation a tree takes, read off its program the way
    csrc/gram.hip: match_pair2 builds metric_mask: the metrics of the radial leaves"""
    metrics = {nd.metric for nd in cov.program_nodes() if nd.op <= capi.OP_MATERN52}
    return (capi.METRIC_EUCLIDEAN in metrics, capi.METRIC_ANGULAR in metrics)


# ---- the reference of the predictive mean -----------------------------------------------------------------------------------
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 2.0 ** -60


def predict_mean_reference(cov, fx, fxs, alpha):
    """(r, S, K): r_j = sum_i K[i, j] alpha_i in np.longdouble, S_j = sum_i |K[i, j]| |alpha_i|, K = oracle_py.gram"""
    K = orc.gram(cov, fx, fxs, x_meas=fx.is_measurement, y_meas=fxs.is_measurement, threads=8 if fx.n * fxs.n > 200000 else 0)
    a = np.asarray(alpha, dtype=np.float64)
    r = np.einsum("ij,i->j", K.astype(np.longdouble), a.astype(np.longdouble))
    S = np.abs(K).T @ np.abs(a)
    return r, S, K


def predict_mean_bound(n, S):
    return ((-(-n // 64) + 12) * EPS + 2e-14) * S


def predict_mean_ok(got, r, S, n):
    err = np.abs(got.astype(np.longdouble) - r).astype(np.float64)
    return bool(np.all(np.isfinite(got)) and np.all(err <= predict_mean_bound(n, S)))


def predict_mean_tiled_numpy(K, alpha):
    """The same sum in plain fp64 in the order of predict_mean_tiled_kernel: thread t of 256 adds the products of the
    training points t, t + 256, ... one after the other, a shuffle tree over the 64 lanes of each wave, then
    (w0 + w1) + (w2 + w3)."""
    n, m = K.shape
    chunks = -(-n // 256)
    P = np.zeros((chunks * 256, m))
    P[:n] = K * alpha[:, None]
    acc = np.zeros((256, m))
    for c in range(chunks):
        acc = acc + P[c * 256:(c + 1) * 256]
    r = acc.reshape(4, 64, m)
    off = 32
    while off > 0:
        r = r[:, :off] + r[:, off:2 * off]
        off //= 2
    r = r[:, 0]
    return (r[0] + r[1]) + (r[2] + r[3])
