"""Every kernel path of csrc/gram.hip and csrc/gram_fast.h, one launch at a time, at its tile edges.

The launches go through agp_debug_gram, agp_debug_gram_blocks and agp_debug_predict_mean (csrc/debug_api.hip), which hand
the caller's whole output buffer - padding rows, gaps and the elements in front included, all canaries - to launch_gram,
launch_gram_blocks and launch_predict_mean and report the path the dispatcher chose.  Every case asserts that path
first, then the values against the oracle under the bars of tests/gram_path_cases.py (none of them measured), then that
nothing outside the matrix was stored, then the NaN flag.  tests/test_gram_paths_host.py checks the premises (planted
pairs, reference and bound) without a GPU."""
import numpy as np
import pytest

import albatross_amd as ab
import gram_path_cases as gc
from oracle import oracle_py as orc

pytestmark = pytest.mark.gpu


@pytest.fixture
def interp_ctx(make_ctx, monkeypatch):
    """A context under AGP_GRAM_SOP=0 (the switch is read when a context is created and holds for the launchers of the
    whole process); afterwards a context under the default puts the switch back for the tests that follow."""
    monkeypatch.setenv("AGP_GRAM_SOP", "0")
    yield make_ctx()
    monkeypatch.setenv("AGP_GRAM_SOP", "1")
    make_ctx()


def check_gram(result, want, expect_path, lower=False, what=""):
    K, rest, before, flag, path = result
    assert path == expect_path, (what, gc.GRAM_PATH_NAMES[path], gc.GRAM_PATH_NAMES[expect_path])
    if lower:
        assert gc.close_nan(np.tril(K), np.tril(want)), what
    else:
        assert gc.close_nan(K, want), what
    assert gc.all_canary(rest), what      # the padding rows of the leading dimension
    assert gc.all_canary(before), what    # the elements in front of a misaligned output
    assert flag == int(np.isnan(np.tril(want) if lower else want).any()), what


# ---- (a) the fast rectangular kernel on a cross Gram ----------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("op", range(4), ids=gc.RADIAL_IDS)
def test_fast_rect_cross(ctx, op, dim):
    """gram_fast_kernel<dim, op>: one / odd / even column counts (the `two` guard), odd row counts (the single-row
    store), both parities of ld and an output one element off its 16-byte alignment (the scalar store pair), equal
    pairs off the diagonal, pairs that only look equal (all but the last coordinate; a squared distance that underflows)."""
    for rows, cols in gc.FAST_CROSS_SHAPES:
        x, y, pairs = gc.planted_cross(rows, cols, dim, 7 * rows + cols + dim)
        for kind, (xm, ym) in gc.FAST_NOISE_KINDS:
            cov = gc.fast_cov(op, kind)
            fx, fy = gc.features(cov, x, xm), gc.features(cov, y, ym)
            want = orc.gram(cov, x, y, x_meas=xm, y_meas=ym)
            for ld in gc.cross_lds(rows):
                for offset in (0, 1):
                    what = (rows, cols, kind, xm, ym, ld, offset)
                    res = gc.run_gram(ctx, cov, fx, fy, ld=ld, offset=offset)
                    check_gram(res, want, gc.FAST_RECT, what=what)
                    if (ld, offset) != (rows, 0):
                        continue
                    # the planted pairs, exactly: noise where the features are equal and the term is on, none elsewhere
                    K = res[0]
                    on = kind == "noise" or (kind == "meas" and xm and ym)
                    Kn = K if kind == "none" else gc.run_gram(ctx, gc.fast_cov(op, "none"), fx, fy)[0]
                    diff = np.argwhere(K != Kn)
                    assert sorted(map(tuple, diff.tolist())) == (sorted(pairs["equal"]) if on else []), what
                    for i, j in pairs["equal"]:
                        assert K[i, j] == Kn[i, j] + (gc.NOISE_SIGMA * gc.NOISE_SIGMA if on else 0.), what


# ---- (b) lower_only and diag_add --------------------------------------------------------------------------------------------
def lower_trees():
    """(id, builder, dim, expected path of a lower_only symmetric launch with AGP_GRAM_SOP=1)"""
    by_name = {t[0]: t[1] for t in gc.PAIR2_TREES}
    fast = [(f"{gc.RADIAL_IDS[op]}{dim}+{gc.FAST_KINDS[k % 4]}", (lambda op=op, k=k: gc.fast_cov(op, gc.FAST_KINDS[k % 4])), dim, gc.FAST_TRI)
            for k, (op, dim) in enumerate(gc.FAST_COMBOS)]  # every gram_fast_tri_kernel<dim, op>
    return fast + [("temperature", by_name["temperature"], 3, gc.PAIR2), ("rad,noise,rank1", by_name["rad,noise,rank1"], 1, gc.PAIR2),
                   ("generic1", gc.generic_radial_cov, 1, gc.SOP), ("generic2", gc.generic_radial_cov, 2, gc.SOP),
                   ("generic3", gc.generic_noise_cov, 3, gc.SOP), ("generic5", gc.generic_noise_cov, 5, gc.SOP)]


def run_lower_and_diag(ctx, cov, dim, expect_path):
    for n in gc.LOWER_SIZES:
        x, _ = gc.planted_symmetric(n, dim, 100 + n)
        fx = gc.features(cov, x, True)
        want = orc.gram(cov, x, x_meas=True)
        d = np.random.default_rng(n).uniform(0., 0.05, n)
        for ld in (n + 1, n + 2):
            what = (n, ld)
            plain = gc.run_gram(ctx, cov, fx, lower_only=True, ld=ld)
            check_gram(plain, want, expect_path, lower=True, what=what)
            added = gc.run_gram(ctx, cov, fx, lower_only=True, ld=ld, diag_add=d)
            check_gram(added, want + np.diag(d), expect_path, lower=True, what=what)
            K0, K1 = plain[0], added[0]
            assert np.array_equal(np.tril(K1, -1), np.tril(K0, -1)), what      # added once, and on the diagonal only
            assert np.array_equal(np.diag(K1), np.diag(K0) + d), what
        # both triangles (lower_only = 0): the rectangular launch of the same path
        full = gc.run_gram(ctx, cov, fx, ld=n + 1)
        check_gram(full, want, gc.FAST_RECT if expect_path == gc.FAST_TRI else expect_path, what=n)
        assert np.array_equal(full[0], full[0].T)
        assert np.array_equal(np.tril(full[0]), np.tril(plain[0]))


@pytest.mark.parametrize("name,build,dim,path", lower_trees(), ids=[t[0] for t in lower_trees()])
def test_lower_only_and_diag_add(ctx, name, build, dim, path):
    """gram_fast_tri_kernel (the workgroup index inverted into a tile) and the lower_only early return of the other
    kernels, with and without diag_add, at one tile, a tile edge and three row tiles"""
    run_lower_and_diag(ctx, build(), dim, path)


@pytest.mark.parametrize("dim", [1, 2, 8])
def test_lower_only_and_diag_add_interpreter(interp_ctx, dim):
    """gram_kernel<1 | 2 | 8, false>; the fast and the pair-2 shapes go there too under AGP_GRAM_SOP=0"""
    cov = {1: lambda: gc.fast_cov(0, "noise"), 2: dict((t[0], t[1]) for t in gc.PAIR2_TREES)["rad,noise,rank1"], 8: gc.generic_noise_cov}[dim]()
    run_lower_and_diag(interp_ctx, cov, dim, gc.INTERP)


def test_fast_tri_many_row_tiles(ctx):
    """17 row tiles: every (r, c) of the triangular launch against the rectangular launch of the same data, bit for bit,
    and 300 rows of it against the oracle"""
    n = gc.TRI_LARGE
    cov = gc.fast_cov(0, "noise")
    x, _ = gc.planted_symmetric(n, 3, n)
    fx = gc.features(cov, x)
    tri = gc.run_gram(ctx, cov, fx, lower_only=True, ld=n + 1)
    rect = gc.run_gram(ctx, cov, fx, lower_only=False, ld=n + 1)
    assert tri[4] == gc.FAST_TRI and rect[4] == gc.FAST_RECT
    assert tri[3] == 0 and rect[3] == 0
    assert gc.all_canary(tri[1]) and gc.all_canary(rect[1])
    assert np.array_equal(np.tril(tri[0]), np.tril(rect[0]))
    # above the diagonal the triangular launch stores only inside the tiles that touch it
    r, c = np.indices((n, n), sparse=True)
    assert gc.all_canary(tri[0][(c // gc.TN) * gc.TN > (r // gc.TM) * gc.TM + gc.TM - 1])
    idx = np.unique(np.concatenate([[0, 127, 128, n - 2, n - 1], np.random.default_rng(0).choice(n, 295, replace=False)]))
    want = orc.gram(cov, x[idx], x, threads=8)
    mask = np.arange(n)[None, :] <= idx[:, None]
    assert gc.close(np.where(mask, tri[0][idx], 0.), np.where(mask, want, 0.))


# ---- (c) the pair-2 kernel ----------------------------------------------------------------------------------------------------
PAIR2_CASES = [(name, build, dim) for name, build, dims, _ in gc.PAIR2_TREES for dim in dims]


@pytest.mark.parametrize("name,build,dim", PAIR2_CASES, ids=[f"{c[0]}-{c[2]}" for c in PAIR2_CASES])
def test_pair2(ctx, name, build, dim):
    """gram_pair2_kernel<dim, EUCLID, ANGULAR>: one and two radial leaves over every metric, the rank-1 term in its
    forms, the noise term in each position of the sum, each term measurement-only in turn"""
    cov = build()
    rows, cols = gc.PAIR2_SHAPE
    x, y, _ = gc.planted_cross(rows, cols, dim, 3 * rows + dim)
    xsym, _ = gc.planted_symmetric(rows, dim, 5 * rows + dim)
    for xm, ym in [(False, False), (True, True), (True, False)]:
        want = orc.gram(cov, x, y, x_meas=xm, y_meas=ym)
        fx, fy = gc.features(cov, x, xm), gc.features(cov, y, ym)
        for ld in (rows, rows + 1):
            check_gram(gc.run_gram(ctx, cov, fx, fy, ld=ld), want, gc.PAIR2, what=(xm, ym, ld))
        if xm == ym:
            fs = gc.features(cov, xsym, xm)
            ws = orc.gram(cov, xsym, x_meas=xm)
            for ld in (rows, rows + 1):
                res = gc.run_gram(ctx, cov, fs, ld=ld)
                check_gram(res, ws, gc.PAIR2, what=(xm, ld))
                assert np.array_equal(res[0], res[0].T)


# ---- (d) the generic evaluators at DIMP 4 and 8 -------------------------------------------------------------------------------
def run_generic(ctx, dim, expect_path):
    rows, cols = gc.PAIR2_SHAPE
    x, y, _ = gc.planted_cross(rows, cols, dim, 11 * rows + dim)
    xsym, _ = gc.planted_symmetric(rows, dim, 13 * rows + dim)
    for cov in (gc.generic_cov(), gc.generic_noise_cov()):
        for xm, ym in [(True, True), (False, True)]:
            want = orc.gram(cov, x, y, x_meas=xm, y_meas=ym)
            for ld in (rows, rows + 1):
                check_gram(gc.run_gram(ctx, cov, gc.features(cov, x, xm), gc.features(cov, y, ym), ld=ld), want, expect_path,
                           what=(xm, ym, ld))
        res = gc.run_gram(ctx, cov, gc.features(cov, xsym, True), ld=rows + 1)
        check_gram(res, orc.gram(cov, xsym, x_meas=True), expect_path)
        assert np.array_equal(res[0], res[0].T)


@pytest.mark.parametrize("dim", gc.GENERIC_DIMS)
def test_generic_sum_of_products(ctx, dim):
    """gram_kernel<4, true> (dim 4) and gram_kernel<8, true> (dim 5 and 8)"""
    run_generic(ctx, dim, gc.SOP)


@pytest.mark.parametrize("dim", gc.GENERIC_DIMS)
def test_generic_interpreter(interp_ctx, dim):
    """gram_kernel<4, false> and gram_kernel<8, false>"""
    run_generic(interp_ctx, dim, gc.INTERP)


# ---- (e) equality ids -----------------------------------------------------------------------------------------------------------
def id_trees():
    by_name = {t[0]: t[1] for t in gc.PAIR2_TREES}
    return [("fast", lambda: gc.fast_cov(0, "noise"), 3, gc.FAST_RECT, gc.FAST_TRI), ("fast1", lambda: gc.fast_cov(2, "nugget"), 1, gc.FAST_RECT, gc.FAST_TRI),
            ("pair2", by_name["rad,noise,rank1"], 2, gc.PAIR2, gc.PAIR2), ("sop", gc.generic_noise_cov, 3, gc.SOP, gc.SOP),
            ("sop8", gc.generic_noise_cov, 8, gc.SOP, gc.SOP)]


def run_ids(ctx, cov, dim, cross_path, lower_path):
    rows, cols = gc.PAIR2_SHAPE
    x, y, xi, yi, _ = gc.planted_ids(rows, cols, dim, 17 + dim)
    for ix, iy in [(xi, yi), (xi, None), (None, yi)]:  # one side without ids: the comparison falls back to coordinates
        fx, fy = gc.features(cov, x, ids=ix), gc.features(cov, y, ids=iy)
        check_gram(gc.run_gram(ctx, cov, fx, fy, ld=rows + 1), orc.gram(cov, fx, fy), cross_path, what=(ix is None, iy is None))
    # symmetric: two points under one id (noise off the diagonal), one point twice under two ids (none)
    xs, si = x.copy(), xi.copy()
    si[5] = si[9]
    xs[7] = xs[11]
    xs[rows - 1] = xs[0]
    si[rows - 1] = si[0]
    fs = gc.features(cov, xs, ids=si)
    want = orc.gram(cov, fs)
    noise_only = orc.gram(ab.IndependentNoise(gc.NOISE_SIGMA), gc.features(ab.IndependentNoise(gc.NOISE_SIGMA), xs, ids=si))
    assert noise_only[9, 5] > 0. and noise_only[11, 7] == 0. and noise_only[rows - 1, 0] > 0.
    check_gram(gc.run_gram(ctx, cov, fs, lower_only=True, ld=rows + 1), want, lower_path, lower=True)
    res = gc.run_gram(ctx, cov, fs, ld=rows)
    check_gram(res, want, cross_path)
    assert np.array_equal(res[0], res[0].T)


@pytest.mark.parametrize("name,build,dim,cross_path,lower_path", id_trees(), ids=[t[0] for t in id_trees()])
def test_equality_ids(ctx, name, build, dim, cross_path, lower_path):
    """the have_ids branches of gram_fast_body, gram_pair2_kernel and gram_kernel<., true>"""
    run_ids(ctx, build(), dim, cross_path, lower_path)


def test_equality_ids_interpreter(interp_ctx):
    run_ids(interp_ctx, gc.generic_noise_cov(), 3, gc.INTERP, gc.INTERP)


# ---- (f) the NaN flag ------------------------------------------------------------------------------------------------------------
def nan_trees():
    by_name = {t[0]: t[1] for t in gc.PAIR2_TREES}
    return [("pair2_angular", by_name["exp_a"], gc.PAIR2, gc.PAIR2, True), ("temperature", by_name["temperature"], gc.PAIR2, gc.PAIR2, True),
            ("sop_angular", gc.generic_cov, gc.SOP, gc.SOP, True), ("fast", lambda: gc.fast_cov(0, "noise"), gc.FAST_RECT, gc.FAST_TRI, False)]


@pytest.mark.parametrize("name,build,cross_path,lower_path,angular", nan_trees(), ids=[t[0] for t in nan_trees()])
def test_nan_flag_counts_stored_entries_only(ctx, name, build, cross_path, lower_path, angular):
    """n = 129 and 129 x 33: the second row tile holds one real row and 127 zero vectors, of which the angular metric makes
    NaN - not stored, not flagged.  A NaN coordinate in the last row, or (angular metric) one all-zero point, is."""
    cov = build()
    rows, cols = gc.PAIR2_SHAPE
    rng = np.random.default_rng(3)
    x = rng.uniform(0.5, 10., (rows, 3))
    y = rng.uniform(0.5, 10., (cols, 3))
    x_nan, x_zero = x.copy(), x.copy()
    x_nan[rows - 1, 0] = np.nan
    x_zero[64] = 0.
    for xv, flagged in [(x, False), (x_nan, True), (x_zero, angular)]:
        fx = gc.features(cov, xv)
        want = orc.gram(cov, xv, y)
        assert bool(np.isnan(want).any()) == flagged
        check_gram(gc.run_gram(ctx, cov, fx, gc.features(cov, y), ld=rows + 1), want, cross_path, what=flagged)
        ws = orc.gram(cov, xv)
        assert bool(np.isnan(ws).any()) == flagged
        check_gram(gc.run_gram(ctx, cov, fx, ld=rows + 1), ws, cross_path, what=flagged)
        check_gram(gc.run_gram(ctx, cov, fx, lower_only=True, ld=rows + 1), ws, lower_path, lower=True, what=flagged)


def test_nan_flag_interpreter(interp_ctx):
    cov = gc.generic_cov()
    x = np.random.default_rng(3).uniform(0.5, 10., (129, 3))
    check_gram(gc.run_gram(interp_ctx, cov, gc.features(cov, x), ld=130), orc.gram(cov, x), gc.INTERP)
    x[64] = 0.
    check_gram(gc.run_gram(interp_ctx, cov, gc.features(cov, x), ld=130), orc.gram(cov, x), gc.INTERP)


# ---- (g) launch_gram_blocks --------------------------------------------------------------------------------------------------------
BLOCK_TREES = [(0, 3, "noise", False), (1, 1, "meas", False), (3, 2, "none", False), (2, 3, "nugget", True)]  # op, dim, noise kind, ids


@pytest.mark.parametrize("count", gc.BLOCK_COUNTS)
@pytest.mark.parametrize("rows", gc.BLOCK_ROWS)
def test_gram_blocks(ctx, rows, count):
    """gram_fast_kernel with blk_rows / blk_stride / blockIdx.z: block g is the Gram matrix of ITS rows (duplicates in
    another block do not show), with its own slice of diag_add, at out + g * stride - even and odd strides, so that
    blocks land off their 16-byte alignment - and nothing is stored between the blocks or below them"""
    n = rows * count
    for op, dim, kind, with_ids in BLOCK_TREES:
        cov = gc.fast_cov(op, kind)
        rng = np.random.default_rng(rows + 1000 * count + dim)
        x = rng.uniform(0.5, 10., (n, dim))
        ids = np.arange(n, dtype=np.int64) if with_ids else None
        for g in range(count):
            if rows > 1:
                x[g * rows + rows - 1] = x[g * rows]      # equal pair inside every block (under different ids)
            if rows > 2 and with_ids:
                ids[g * rows + 1] = ids[g * rows + 2]     # one id on two points
        if count > 1:
            x[rows] = x[0]                                # equal pair across blocks
        fx = gc.features(cov, x, True, ids)
        d = rng.uniform(0., 0.05, n)
        for ld in (rows + 1, rows + 2):
            for stride in (ld * rows + 3, ld * rows + 4):
                what = (op, dim, kind, ld, stride)
                buf, launched = gc.run_gram_blocks(ctx, cov, fx, rows, count, ld, stride, d)
                assert launched == 1, what
                for g in range(count):
                    sl = slice(g * rows, (g + 1) * rows)
                    M = buf[g * stride:g * stride + ld * rows].reshape(ld, rows, order="F")
                    fg = gc.features(cov, x[sl], True, None if ids is None else ids[sl])
                    want = orc.gram(cov, fg, x_meas=True) + np.diag(d[sl])
                    assert gc.close(np.tril(M[:rows]), np.tril(want)), (what, g)
                    assert gc.all_canary(M[rows:]), (what, g)
                    if g + 1 < count:
                        assert gc.all_canary(buf[g * stride + ld * rows:(g + 1) * stride]), (what, g)


def test_gram_blocks_declines_other_trees(ctx):
    """a tree outside the fast shapes: nothing launched, the buffer untouched"""
    cov = dict((t[0], t[1]) for t in gc.PAIR2_TREES)["const+m32_e"]()
    x = np.random.default_rng(0).uniform(0.5, 10., (93, 3))
    buf, launched = gc.run_gram_blocks(ctx, cov, gc.features(cov, x, True), 31, 3, 32, 32 * 31 + 3, np.zeros(93))
    assert launched == 0 and gc.all_canary(buf)
    cov = gc.fast_cov(0, "noise")  # ... and a fast tree above three dimensions
    x = np.random.default_rng(0).uniform(0.5, 10., (93, 4))
    buf, launched = gc.run_gram_blocks(ctx, cov, gc.features(cov, x, True), 31, 3, 32, 32 * 31 + 3, np.zeros(93))
    assert launched == 0 and gc.all_canary(buf)


# ---- (h) the predictive mean ---------------------------------------------------------------------------------------------------------
def check_predict_mean(ctx, cov, fx, fxs, alpha, expect_path, what=""):
    mean, tail, path = gc.run_predict_mean(ctx, cov, fx, fxs, alpha)
    assert path == expect_path, (what, gc.PM_PATH_NAMES[path], gc.PM_PATH_NAMES[expect_path])
    r, S, _ = gc.predict_mean_reference(cov, fx, fxs, alpha)
    assert np.all(S > 0.)
    err = np.abs(mean.astype(np.longdouble) - r).astype(np.float64)
    bound = gc.predict_mean_bound(fx.n, S)
    print(f"predict mean {what}: max error / bound {float((err / bound).max()):.3g}")
    assert gc.predict_mean_ok(mean, r, S, fx.n), what
    assert gc.all_canary(tail), what  # nothing stored past the last test point
    return mean


PM_FAST_CASES = gc.predict_mean_fast_cases()


@pytest.mark.parametrize("n,m,op,dim,kind,xs_meas,ids", PM_FAST_CASES,
                         ids=[f"{c[0]}x{c[1]}-{gc.RADIAL_IDS[c[2]]}{c[3]}-{c[4]}{int(c[5])}{'-ids_' + c[6] if c[6] else ''}" for c in PM_FAST_CASES])
def test_predict_mean_fast_paths(ctx, n, m, op, dim, kind, xs_meas, ids):
    """predict_mean_tiled_kernel<dim, op, 8 | 4> and predict_mean_fast_kernel<dim, op>: the thresholds 1024 and 16384 from
    both sides, partial last tiles of every length, fewer training points than threads (the clamp) and one more than a
    multiple of 256 (the prefetch that re-reads), test points that are training points (the `__any` branch; the last test
    point of a partial tile against training point N - 1); equality ids on both sides (the ids decide) and on one side only
    (`have_ids` false with one pointer set: the coordinates decide, and none of the guarded id loads may run)"""
    cov = gc.fast_cov(op, kind)
    x, xs, alpha, _, xi, si = gc.predict_mean_points(n, m, dim, 31 * n + m, ids)
    fx, fxs = gc.features(cov, x, True, xi), gc.features(cov, xs, xs_meas, si)
    check_predict_mean(ctx, cov, fx, fxs, alpha, gc.expected_fast_pm_path(m), what=(n, m))


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("op", range(4), ids=gc.RADIAL_IDS)
def test_predict_mean_dead_length_scale(ctx, op, dim):
    """a non-positive length scale (radial.hpp: the covariance is 0) goes back to the one-wave kernel at any M, and the mean
    is exactly the noise term: sigma^2 alpha_i at the copy of training point i, 0 elsewhere - by ids where both sides carry
    them, by coordinates where neither or only one does"""
    n, m = 257, 1027
    for ids in [None] + gc.ID_MODES:
        x, xs, alpha, pairs, xi, si = gc.predict_mean_points(n, m, dim, 5 + dim, ids)
        for ls in (0., -1.):
            cov = gc.fast_cov(op, "noise", length_scale=ls)
            mean, tail, path = gc.run_predict_mean(ctx, cov, gc.features(cov, x, True, xi), gc.features(cov, xs, True, si), alpha)
            assert path == gc.FAST_WAVE
            want = np.zeros(m)
            for i, j in pairs:
                want[j] = gc.NOISE_SIGMA * gc.NOISE_SIGMA * alpha[i]
            assert np.array_equal(mean, want) and gc.all_canary(tail), (ids, ls)
    assert gc.expected_fast_pm_path(m, 2.5) == gc.TILED4


def run_predict_mean_generic(ctx, dim, expect_path):
    cov = gc.generic_radial_cov() if dim <= 2 else (gc.generic_noise_cov() if dim % 2 else gc.generic_cov())
    for k, (n, m) in enumerate([(n, 5) for n in gc.PM_N] + [(257, 1027), (193, 3)]):
        ids = gc.ID_MODES[(k // 4) % 3] if k % 4 == 3 else None  # k = 3: both sides, 7: training points only, 11: test points only
        x, xs, alpha, _, xi, si = gc.predict_mean_points(n, m, dim, 77 * n + m + dim, ids)
        # (with ids the test points are measurements too: the measurement-only noise of generic_cov is on, the equality counts)
        fx, fxs = gc.features(cov, x, True, xi), gc.features(cov, xs, k % 2 == 0 or ids is not None, si)
        check_predict_mean(ctx, cov, fx, fxs, alpha, expect_path, what=(n, m, dim, ids))


@pytest.mark.parametrize("dim", [1, 2, 3] + gc.GENERIC_DIMS)
def test_predict_mean_sum_of_products(ctx, dim):
    """predict_mean_kernel<DIMP, true>: the two-points-per-trip loop `i + 64 < N` and its remainder at every N of the table,
    every DIMP"""
    run_predict_mean_generic(ctx, dim, gc.PM_SOP)


@pytest.mark.parametrize("dim", [1, 2, 3] + gc.GENERIC_DIMS)
def test_predict_mean_interpreter(interp_ctx, dim):
    """predict_mean_kernel<DIMP, false>; a fast tree goes there too under AGP_GRAM_SOP=0"""
    run_predict_mean_generic(interp_ctx, dim, gc.PM_INTERP)
    if dim == 3:
        cov = gc.fast_cov(0, "noise")
        x, xs, alpha, _, _, _ = gc.predict_mean_points(257, 1027, dim, 9)
        check_predict_mean(interp_ctx, cov, gc.features(cov, x, True), gc.features(cov, xs, True), alpha, gc.PM_INTERP, what="fast tree")
