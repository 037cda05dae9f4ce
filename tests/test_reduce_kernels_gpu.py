"""Every small kernel of csrc/reduce.hip on its own through agp_debug_reduce, and the wide vector sweeps and the mixed fit's
preconditioner of csrc/api.hip through agp_debug_wide_sweep (csrc/debug_api.hip).

Shapes, inputs, references and bounds are tests/reduce_cases.py's (its docstring derives the bounds and lists which test
names which launcher; tests/test_reduce_bounds_host.py shows that plain fp64 evaluations meet them on these inputs and
that a dropped, doubled or shifted term does not).  Reductions assert error / bound <= 1 against a longdouble reference;
movers and packers are compared bit for bit over the WHOLE buffer that went in - NaN padding rows, the other triangle,
rows above row0 and the gaps between batch entries come back as they were; the sweeps assert the componentwise residual
bound of tests/substitution_cases.py against the matrix the device solved with.  Each test prints its worst ratio."""
import ctypes as C

import numpy as np
import pytest

from albatross_amd import _capi as capi
import reduce_cases as rc
import substitution_cases as sc

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 1  # include/albatross_amd.h: AGP_ERR_INVALID_ARGUMENT
REDUCTIONS = rc.reduction_cases()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def reduce_call(ctx, op, ip, dp, bufs):
    """agp_debug_reduce: bufs are flat numpy arrays (run in place) or None; the same array twice shares a device buffer."""
    fn = capi.load_debug().agp_debug_reduce
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    for b in bufs:
        assert b is None or (b.flags.c_contiguous and b.flags.writeable and b.ndim == 1)
    ipa = np.asarray(ip, dtype=np.int64)
    dpa = np.asarray(dp, dtype=np.float64)
    ptrs = (C.c_void_p * len(bufs))(*[None if b is None else b.ctypes.data for b in bufs])
    sizes = np.asarray([0 if b is None else b.nbytes for b in bufs], dtype=np.int64)
    return fn(ctx._h, op, ipa.ctypes.data, len(ipa), dpa.ctypes.data if len(dpa) else None, len(dpa), ptrs, sizes.ctypes.data, len(bufs))


def nan_vector(v, extra=3):
    """v followed by `extra` NaN words: (flat, view of the first len(v))."""
    flat = np.full(len(v) + extra, np.nan)
    flat[:len(v)] = v
    return flat, flat[:len(v)]


def base_and_out(mode, base, n):
    """(base buffer, out buffer) for the three modes of `base`: none, its own buffer, the buffer of out."""
    if mode == "alias":
        flat, _ = nan_vector(base)
        return flat, flat
    out = np.full(n + 3, np.nan)
    return (None if mode == "null" else nan_vector(base)[0]), out


def tail_untouched(out, n):
    return np.all(_bits(out[n:]) == _bits(np.array([np.nan]))[0])


def slabs(mats, ld, stride):
    """Column-major matrices in NaN-filled slabs `stride` apart, leading dimension ld: flat buffer."""
    flat = np.full(stride * (len(mats) - 1) + ld * mats[0].shape[1] + 2, np.nan)
    for b, M in enumerate(mats):
        flat[b * stride:b * stride + ld * M.shape[1]].reshape((ld, M.shape[1]), order="F")[:M.shape[0]] = M
    return flat


def slab_view(flat, b, rows, cols, ld, stride):
    return flat[b * stride:b * stride + ld * cols].reshape((ld, cols), order="F")[:rows]


def vectors(vs, stride):
    flat = np.full(stride * (len(vs) - 1) + len(vs[0]) + 2, np.nan)
    for b, v in enumerate(vs):
        flat[b * stride:b * stride + len(v)] = v
    return flat


# ---- reductions ---------------------------------------------------------------------------------------------------
def run_reduction(ctx, case, p):
    """Runs the kernel of one reduction case; returns its outputs in the order of the canonical form.  Asserts that the
    read-only inputs and every word around the outputs came back as they went in."""
    kern, mode = case["kernel"], case.get("base", "null")
    if kern == "coldot":
        n, m = case["n"], case["m"]
        A, _ = rc.nan_padded(p["A"], n + 3)
        B, _ = rc.nan_padded(p["B"], n + 6)
        base, out = base_and_out(mode, p["base"], m)
        keep = [A.copy(), B.copy()]
        assert reduce_call(ctx, rc.COLDOT, [n + 3, n + 6, n, m], [-p["alpha"]], [A, B, out, base]) == 0
        assert same_bits(A, keep[0]) and same_bits(B, keep[1]) and tail_untouched(out, m)
        return out[:m].copy()
    if kern == "dot":
        n = case["n"]
        a, b, out = nan_vector(p["a"])[0], nan_vector(p["b"])[0], np.full(4, np.nan)
        assert reduce_call(ctx, rc.DOT, [n], [], [a, b, out]) == 0
        assert tail_untouched(out, 1)
        return out[:1].copy()
    if kern in ("matvec", "tall_matvec", "tall_matvec_f32", "colvec_dot", "colvec_dot_f32"):
        W = p["W"]
        rows, cols = W.shape
        ld = rows + 3
        Wf, _ = rc.nan_padded(W, ld, extra=2) if cols else (None, None)
        vec = p["x"] if "x" in p else p["v"]
        vf = nan_vector(vec)[0] if len(vec) else None
        nout = rows if "x" in p else cols
        base, out = base_and_out(mode, p["base"], nout)
        keepW = None if Wf is None else Wf.copy()
        if kern == "matvec":
            partial = np.full(max(1, -(-cols // 1024)) * rows + 3, np.nan)
            st = reduce_call(ctx, rc.MATVEC, [ld, rows, cols], [p["alpha"], p["beta"]], [Wf, vf, partial, base, out])
        else:
            op = {"tall_matvec": rc.TALL_MATVEC, "tall_matvec_f32": rc.TALL_MATVEC_F32, "colvec_dot": rc.COLVEC_DOT,
                  "colvec_dot_f32": rc.COLVEC_DOT_F32}[kern]
            st = reduce_call(ctx, op, [ld, rows, cols], [p["alpha"], p["beta"]], [Wf, vf, base, out])
        assert st == 0, st
        assert (keepW is None or same_bits(Wf, keepW)) and tail_untouched(out, nout)
        if mode == "distinct":
            assert np.array_equal(base[:nout], p["base"])
        return out[:nout].copy()
    if kern == "colvec_dot_strided":
        m, n, count = case["m"], case["n"], case["count"]
        ld = m + 3
        stride_W, stride_v = ld * n + 11, max(m, n) + 5
        W = slabs(list(p["W"]), ld, stride_W)
        v = vectors(list(p["v"]), stride_v)
        out = np.full(stride_v * count, np.nan)
        if mode == "alias":
            for b in range(count):
                out[b * stride_v:b * stride_v + n] = p["base"][b * n:(b + 1) * n]
            base = out
        else:
            base = None if mode == "null" else vectors(list(p["base"].reshape(count, n)), stride_v)
        assert reduce_call(ctx, rc.COLVEC_DOT_STRIDED, [ld, stride_W, m, n, stride_v, count], [p["alpha"], p["beta"]], [W, v, base, out]) == 0
        got = out.reshape(count, stride_v)
        assert np.all(np.isnan(got[:, n:])), "gaps between the outputs written"
        return got[:, :n].reshape(-1).copy()
    if kern == "colvec_dot_batched":
        m, count = case["m"], case["count"]
        ld = m + 3
        stride_Q, stride_z = ld * m + 11, m + 5
        Q = slabs(list(p["Q"]), ld, stride_Q)
        z = vectors(list(p["z"]), stride_z)
        out = np.full(count * m + 3, np.nan)
        assert reduce_call(ctx, rc.COLVEC_DOT_BATCHED, [ld, stride_Q, m, stride_z, count], [], [Q, z, out]) == 0
        assert tail_untouched(out, count * m)
        return out[:count * m].copy()
    if kern == "symv_lower_batched":
        n, count = case["n"], case["count"]
        ld = n + 3
        stride_K, stride_v = ld * n + 9, n + 5
        lower = [np.where(np.tril(np.ones((n, n), dtype=bool)), K, np.nan) for K in p["K"]]  # the upper triangle is NaN
        K = slabs(lower, ld, stride_K)
        v = vectors(list(p["p"]), stride_v)
        out = np.full(stride_v * count, np.nan)
        assert reduce_call(ctx, rc.SYMV_LOWER_BATCHED, [ld, stride_K, n, stride_v, count], [], [K, v, out]) == 0
        got = out.reshape(count, stride_v)
        assert np.all(np.isnan(got[:, n:])), "gaps between the outputs written"
        return got[:, :n].reshape(-1).copy()
    raise ValueError(kern)


def reduction_family(ctx, kernel):
    worst, where = 0.0, None
    cases = [c for c in REDUCTIONS if c["kernel"] == kernel]
    assert cases
    for case in cases:
        p = rc.reduction_problem(case)
        got = run_reduction(ctx, case, p)
        ratio = rc.error_ratio(got, *rc.canonical_bound(p))
        if ratio >= worst:
            worst, where = ratio, case["id"]
        assert ratio <= 1.0, (case["id"], ratio)
    print(f"{kernel}: {len(cases)} cases, worst error / bound {worst:.3g} ({where})")


def test_coldot(ctx):
    reduction_family(ctx, "coldot")


def test_dot(ctx):
    reduction_family(ctx, "dot")


def test_matvec(ctx):
    """Odd and even column counts inside a 1024-column chunk, a last chunk of one column, and n = 0 with a base: the
    reduce launch alone."""
    reduction_family(ctx, "matvec")


def test_tall_matvec(ctx):
    """The 16-, 8- and 1-column loop bodies on each of the four waves' column ranges; base null, distinct, aliasing out."""
    reduction_family(ctx, "tall_matvec")


def test_tall_matvec_f32(ctx):
    reduction_family(ctx, "tall_matvec_f32")


def test_colvec_dot(ctx):
    reduction_family(ctx, "colvec_dot")


def test_colvec_dot_strided(ctx):
    reduction_family(ctx, "colvec_dot_strided")


def test_colvec_dot_batched(ctx):
    reduction_family(ctx, "colvec_dot_batched")


def test_colvec_dot_f32(ctx):
    """colvec_dot8_kernel<float>: the guarded row tail (m no multiple of 512), an odd last column, fewer columns than a
    workgroup's eight, base aliasing out."""
    reduction_family(ctx, "colvec_dot_f32")


def test_symv_lower_batched(ctx):
    reduction_family(ctx, "symv_lower_batched")


def test_tall_matvec_refuses_more_columns_than_it_stages(ctx):
    """launch_tall_matvec* launches nothing beyond TALL_MATVEC_MAX_COLS columns; the callers check their widths where they
    choose them (csrc/api.hip) and the debug entry reports the call instead of returning a stale vector."""
    rows, ncols = 4, rc.TALL_MATVEC_MAX_COLS + 1
    for op, dtype in ((rc.TALL_MATVEC, np.float64), (rc.TALL_MATVEC_F32, np.float32)):
        W, x, out = np.ones(rows * ncols, dtype=dtype), np.ones(ncols), np.full(rows, 7.0)
        assert reduce_call(ctx, op, [rows, rows, ncols], [1.0, 0.0], [W, x, None, out]) == INVALID_ARGUMENT
        assert np.all(out == 7.0)
        assert reduce_call(ctx, op, [rows, rows, ncols - 1], [1.0, 0.0], [W, x, None, out]) == 0
        assert np.all(out == ncols - 1)


CONTRACTS = rc.contract_cases()


def test_contract_combinations(ctx):
    worst, where = 0.0, None
    for case in CONTRACTS:
        na, nb = case["na"], case["nb"]
        p = rc.contract_problem(case)
        ldk, ldo = max(p["nx"], 1) + 3, na + 3
        K, _ = rc.nan_padded(p["K"], ldk, extra=2) if p["K"].size else (np.full(4, np.nan), None)
        out, view = rc.nan_padded(np.full((na, nb), np.nan), ldo, extra=2)
        before = out.copy()
        lists = [None if a is None else a.copy() for a in (p["xoff"], p["xc"], p["yoff"], p["yc"])]
        st = reduce_call(ctx, rc.CONTRACT, [ldk, na, nb, case["symmetric"], ldo], [], [K, lists[0], lists[1], lists[2], lists[3], out])
        assert st == 0, (case["id"], st)
        got = view[:na].copy()
        view[:na] = np.nan
        assert same_bits(out, before), (case["id"], "padding of out written")
        ref, bound = rc.contract_reference(case, p)
        if case["symmetric"]:
            assert same_bits(got, got.T.copy()), (case["id"], "the mirrored half differs")
        ratio = rc.error_ratio(got.reshape(-1), ref.reshape(-1), bound.reshape(-1))
        if ratio >= worst:
            worst, where = ratio, case["id"]
        assert ratio <= 1.0, (case["id"], ratio)
    print(f"contract_combinations: {len(CONTRACTS)} cases, worst error / bound {worst:.3g} ({where})")


@pytest.mark.parametrize("n", rc.COLUMN_ROWS)
def test_loo(ctx, n):
    p = rc.loo_problem(n)
    (mean_ref, mean_bound), (var_ref, var_bound) = rc.loo_reference(p)
    worst = 0.0
    for alias in (False, True):
        d, y, info = nan_vector(p["d"])[0], nan_vector(p["y"])[0], nan_vector(p["info"])[0]
        mean = np.full(n + 3, np.nan)
        var = d if alias else np.full(n + 3, np.nan)
        assert reduce_call(ctx, rc.LOO, [n], [], [d, y, info, mean, var]) == 0
        assert tail_untouched(mean, n) and tail_untouched(var, n)
        assert np.array_equal(y[:n], p["y"]) and np.array_equal(info[:n], p["info"]) and (alias or np.array_equal(d[:n], p["d"]))
        worst = max(worst, rc.error_ratio(mean[:n], mean_ref, mean_bound), rc.error_ratio(var[:n], var_ref, var_bound))
    print(f"loo n={n}: worst error / bound {worst:.3g}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n", rc.COLUMN_ROWS)
def test_axpby(ctx, n):
    worst = 0.0
    for mode in ("both", "x_null", "y_null", "in_place"):
        p = rc.axpby_problem(n, "both" if mode == "in_place" else mode)
        ref, bound = rc.axpby_reference(p, n)
        x = None if p["x"] is None else nan_vector(p["x"])[0]
        y = None if p["y"] is None else nan_vector(p["y"])[0]
        out = y if mode == "in_place" else np.full(n + 3, np.nan)  # (refine_information updates its vectors in place)
        assert reduce_call(ctx, rc.AXPBY, [n], [p["a"], p["b"]], [x, y, out]) == 0
        assert tail_untouched(out, n)
        worst = max(worst, rc.error_ratio(out[:n], ref, bound))
    print(f"axpby n={n}: worst error / bound {worst:.3g}")
    assert worst <= 1.0, worst


# ---- movers and packers: bit for bit ------------------------------------------------------------------------------
def lower_mask(n):
    return np.tril(np.ones((n, n), dtype=bool))


@pytest.mark.parametrize("n", rc.TILE_SIZES)
def test_symmetrize(ctx, n):
    M = np.where(lower_mask(n), rc.rng_of(n, 1).standard_normal((n, n)), np.nan)
    flat, view = rc.nan_padded(M, n + 3, extra=2)
    want = flat.copy()
    wv = want[:(n + 3) * n].reshape((n + 3, n), order="F")
    wv[:n] = np.tril(M) + np.tril(M, -1).T
    assert reduce_call(ctx, rc.SYMMETRIZE, [n + 3, n], [], [flat]) == 0
    assert same_bits(flat, want)


@pytest.mark.parametrize("n", rc.TILE_SIZES)
def test_upper_to_lower(ctx, n):
    rng = rc.rng_of(n, 2)
    S = np.where(lower_mask(n).T, rng.standard_normal((n, n)), np.nan)  # the upper triangle; the strict lower one NaN
    src, _ = rc.nan_padded(S, n + 3, extra=2)
    D0 = np.where(lower_mask(n), rng.standard_normal((n, n)), np.nan)   # the destination's other triangle is NaN and stays
    dst, _ = rc.nan_padded(D0, n + 5, extra=2)
    want = dst.copy()
    wv = want[:(n + 5) * n].reshape((n + 5, n), order="F")
    wv[:n] = np.where(lower_mask(n), S.T, D0)
    keep = src.copy()
    assert reduce_call(ctx, rc.UPPER_TO_LOWER, [n + 3, n + 5, n], [], [src, dst]) == 0
    assert same_bits(dst, want) and same_bits(src, keep)


@pytest.mark.parametrize("m", rc.TILE_SIZES)
def test_transpose_blocks(ctx, m):
    count = 3
    blocks = rc.rng_of(m, 3).standard_normal((count, m, m))
    src = np.concatenate([b.ravel(order="F") for b in blocks] + [np.full(5, np.nan)])
    dst = np.full_like(src, np.nan)
    want = np.concatenate([b.T.ravel(order="F") for b in blocks] + [np.full(5, np.nan)])
    keep = src.copy()
    assert reduce_call(ctx, rc.TRANSPOSE_BLOCKS, [m, count], [], [src, dst]) == 0
    assert same_bits(dst, want) and same_bits(src, keep)


@pytest.mark.parametrize("n", rc.COLUMN_ROWS)
def test_zero_upper(ctx, n):
    M = rc.rng_of(n, 4).standard_normal((n, n))
    M[np.triu_indices(n, 1)] = np.nan
    flat, _ = rc.nan_padded(M, n + 3, extra=2)
    want = flat.copy()
    want[:(n + 3) * n].reshape((n + 3, n), order="F")[:n] = np.tril(M)
    assert reduce_call(ctx, rc.ZERO_UPPER, [n + 3, n], [], [flat]) == 0
    assert same_bits(flat, want)


@pytest.mark.parametrize("n", rc.COLUMN_ROWS)
def test_set_identity(ctx, n):
    flat, _ = rc.nan_padded(np.full((n, n), np.nan), n + 3, extra=2)
    want = flat.copy()
    want[:(n + 3) * n].reshape((n + 3, n), order="F")[:n] = np.eye(n)
    assert reduce_call(ctx, rc.SET_IDENTITY, [n + 3, n], [], [flat]) == 0
    assert same_bits(flat, want)


@pytest.mark.parametrize("m", rc.COLUMN_ROWS)
def test_set_identity_batched(ctx, m):
    count, ld = 3, m + 3
    stride = ld * m + 7
    flat = np.full(stride * count, np.nan)
    want = flat.copy()
    for b in range(count):
        slab_view(want, b, m, m, ld, stride)[:] = np.eye(m)
    assert reduce_call(ctx, rc.SET_IDENTITY_BATCHED, [ld, stride, m, count], [], [flat]) == 0
    assert same_bits(flat, want)


@pytest.mark.parametrize("m", rc.COLUMN_ROWS)
@pytest.mark.parametrize("with_diag", [False, True])
def test_negate(ctx, m, with_diag):
    M = rc.rng_of(m, 6).standard_normal((m, m))
    flat, _ = rc.nan_padded(M, m + 3, extra=2)
    want = flat.copy()
    want[:(m + 3) * m].reshape((m + 3, m), order="F")[:m] = -M
    diag = np.full(m + 3, np.nan) if with_diag else None
    assert reduce_call(ctx, rc.NEGATE, [m + 3, m], [], [flat, diag]) == 0
    assert same_bits(flat, want)
    if with_diag:
        assert same_bits(diag, np.concatenate([-np.diag(M), np.full(3, np.nan)]))


@pytest.mark.parametrize("n", rc.LOWER_SIZES)
def test_convert_lower_f32(ctx, n):
    """The fp32 copy equals L.astype(float32) on the lower triangle; besides it only the entry above the diagonal of an odd
    column is written (with the rounding of what stood there), nothing else - neither the rest of the upper triangle nor a
    padding row."""
    ld = rc.factor_ld(n)
    src, sview = rc.lower_source(n)
    src = src.copy()
    keep = src.copy()
    dst = np.full(ld * n, np.nan, dtype=np.float32)
    dst.view(np.uint32)[:] = 0xFFFFFFFF
    want = dst.copy()
    mask = rc.pair_written_mask(n)
    wv = want.reshape((ld, n), order="F")
    wv[:n][mask] = sview[:n].astype(np.float32)[mask]
    assert reduce_call(ctx, rc.CONVERT_LOWER_F32, [ld, n], [], [src, dst]) == 0
    got = dst.reshape((ld, n), order="F")
    assert np.array_equal(got[:n][lower_mask(n)], sview[:n].astype(np.float32)[lower_mask(n)])
    assert same_bits(dst, want) and same_bits(src, keep)


@pytest.mark.parametrize("n", rc.LOWER_SIZES)
@pytest.mark.parametrize("with_flag", [True, False])
def test_copy_lower(ctx, n, with_flag):
    """The copy of the lower triangle, bit for bit; the strict upper triangle of the SOURCE is NaN throughout - the pair
    (j - 1, j) of every odd column included - and must neither raise the flag nor be copied anywhere but to (j - 1, j)."""
    ld = rc.factor_ld(n)
    _, sview = rc.lower_source(n)
    S = np.where(lower_mask(n), sview[:n], np.nan)
    src, _ = rc.nan_padded(S, ld)
    keep = src.copy()
    dst = np.full(ld * n, np.nan)
    dst.view(np.uint64)[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    want = dst.copy()
    mask = rc.pair_written_mask(n)
    want.reshape((ld, n), order="F")[:n][mask] = S[mask]
    flag = np.zeros(1, dtype=np.int32) if with_flag else None
    assert reduce_call(ctx, rc.COPY_LOWER, [ld, n], [], [src, dst, flag]) == 0
    assert same_bits(dst, want) and same_bits(src, keep)
    assert flag is None or flag[0] == 0, "a NaN above the diagonal raised the flag"


@pytest.mark.parametrize("n", [2, 3, 513, 2049, 2050])
def test_copy_lower_nan_flag(ctx, n):
    """One NaN at a time in the lower triangle raises the flag wherever it lies."""
    ld = rc.factor_ld(n)
    src, sview = rc.lower_source(n)
    src = src.copy()
    sv = src.reshape((ld, n), order="F")
    dst = np.empty(ld * n)
    for r, c, what in rc.nan_positions(n):
        saved = sv[r, c]
        sv[r, c] = np.nan
        flag = np.zeros(1, dtype=np.int32)
        assert reduce_call(ctx, rc.COPY_LOWER, [ld, n], [], [src, dst, flag]) == 0
        assert flag[0] == 1, (n, r, c, what)
        sv[r, c] = saved


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1000, 2049, 2050])
def test_nan_scan_lower(ctx, n):
    """No flag for a clean lower triangle under an all-NaN strict upper one; a flag for one NaN at each of the places of
    tests/reduce_cases.py: nan_positions."""
    ld = n + 3
    M = np.where(lower_mask(n), rc.rng_of(n, 8).standard_normal((n, n)), np.nan)
    flat, view = rc.nan_padded(M, ld, extra=2)
    keep = flat.copy()
    flag = np.zeros(1, dtype=np.int32)
    assert reduce_call(ctx, rc.NAN_SCAN_LOWER, [ld, n], [], [flat, flag]) == 0
    assert flag[0] == 0 and same_bits(flat, keep)
    for r, c, what in rc.nan_positions(n):
        saved = view[r, c]
        view[r, c] = np.nan
        flag = np.zeros(1, dtype=np.int32)
        assert reduce_call(ctx, rc.NAN_SCAN_LOWER, [ld, n], [], [flat, flag]) == 0
        assert flag[0] == 1, (n, r, c, what)
        view[r, c] = saved


@pytest.mark.parametrize("n,m,cols,row0", [(300, 4, 6, 0), (300, 4, 6, 5), (1, 1, 1, 0), (257, 3, 2, 5),
                                           (64 * 256 + 300, 2, 3, 0), (64 * 256 + 300 + 5, 2, 3, 5)])
def test_gather_cols(ctx, n, m, cols, row0):
    """Padding (negative) indices give zero columns, rows above row0 stay as they were; n - row0 > 64 * 256 rows: the
    grid-stride loop's second pass."""
    rng = rc.rng_of(n, m, row0)
    R, rview = rc.nan_padded(rng.standard_normal((n, cols)), n + 3, extra=2)
    idx = rng.integers(0, cols, m).astype(np.int64)
    idx[m // 2] = -1 if m > 1 else idx[0]
    G, _ = rc.nan_padded(np.full((n, m), np.nan), n + 5, extra=2)
    want = G.copy()
    wv = want[:(n + 5) * m].reshape((n + 5, m), order="F")
    for a, j in enumerate(idx):
        wv[row0:n, a] = 0.0 if j < 0 else rview[row0:n, j]
    keep = R.copy()
    assert reduce_call(ctx, rc.GATHER_COLS, [n + 3, m, row0, n, n + 5, cols], [], [R, idx, G]) == 0
    assert same_bits(G, want) and same_bits(R, keep)


@pytest.mark.parametrize("m", rc.COLUMN_ROWS)
@pytest.mark.parametrize("with_sub", [False, True])
def test_gather_vec(ctx, m, with_sub):
    rng = rc.rng_of(m, 9)
    nsrc = m + 7
    src = rng.standard_normal(nsrc)
    idx = rng.integers(0, nsrc, m).astype(np.int64)
    idx[::5] = -1
    sub = rng.standard_normal(m) if with_sub else None
    out = np.full(m + 3, np.nan)
    want = out.copy()
    v = np.where(idx < 0, 0.0, src[np.maximum(idx, 0)])
    want[:m] = v - sub if with_sub else v
    assert reduce_call(ctx, rc.GATHER_VEC, [m, nsrc], [], [src.copy(), idx, None if sub is None else sub.copy(), out]) == 0
    assert same_bits(out, want)


GROUPS = [(smax, rows) for smax in rc.GROUP_SMAX for rows in rc.GROUP_ROWS]


@pytest.mark.parametrize("smax,rows", GROUPS)
def test_pad_columns(ctx, smax, rows):
    """Compact -> padded zero-fills the columns beyond a group's size; padded -> compact drops them (whatever they hold)
    and writes nothing for the empty group."""
    off = rc.group_offsets(smax)
    groups, total = len(off) - 1, int(off[-1])
    rng = rc.rng_of(smax, rows)
    compact, cview = rc.nan_padded(rng.standard_normal((rows, total)), rows + 3, extra=2)
    padded, _ = rc.nan_padded(np.full((rows, smax * groups), np.nan), rows + 5, extra=2)
    want = padded.copy()
    wv = want[:(rows + 5) * smax * groups].reshape((rows + 5, smax * groups), order="F")
    wv[:rows] = 0.0
    for g in range(groups):
        sg = off[g + 1] - off[g]
        wv[:rows, g * smax:g * smax + sg] = cview[:rows, off[g]:off[g + 1]]
    assert reduce_call(ctx, rc.PAD_COLUMNS, [rows + 3, smax, groups, rows, rows + 5, 0], [], [compact, off.copy(), padded]) == 0
    assert same_bits(padded, want)
    # back: the padding columns hold NaN now and must not travel
    src = padded.copy()
    sv = src[:(rows + 5) * smax * groups].reshape((rows + 5, smax * groups), order="F")
    for g in range(groups):
        sv[:rows, g * smax + (off[g + 1] - off[g]):(g + 1) * smax] = np.nan
    back, _ = rc.nan_padded(np.full((rows, total), np.nan), rows + 3, extra=2)
    assert reduce_call(ctx, rc.PAD_COLUMNS, [rows + 5, smax, groups, rows, rows + 3, 1], [], [src, off.copy(), back]) == 0
    assert same_bits(back, compact)


@pytest.mark.parametrize("smax", rc.GROUP_SMAX)
def test_pad_identity(ctx, smax):
    """Rows and columns beyond a group's size become identity in the LOWER part; the group's own block, the upper triangle,
    padding rows and gaps stay."""
    off = rc.group_offsets(smax)
    groups, ld = len(off) - 1, smax + 3
    stride = ld * smax + 7
    rng = rc.rng_of(smax, 11)
    flat = slabs([rng.standard_normal((smax, smax)) for _ in range(groups)], ld, stride)
    want = flat.copy()
    for g in range(groups):
        sg = int(off[g + 1] - off[g])
        v = slab_view(want, g, smax, smax, ld, stride)
        r, c = np.tril_indices(smax)
        pad = (r >= sg) | (c >= sg)
        v[r[pad], c[pad]] = (r[pad] == c[pad]).astype(np.float64)
    assert reduce_call(ctx, rc.PAD_IDENTITY, [ld, stride, smax, groups], [], [flat, off.copy()]) == 0
    assert same_bits(flat, want)


@pytest.mark.parametrize("smax", rc.GROUP_SMAX)
def test_compact_blocks(ctx, smax):
    off = rc.group_offsets(smax)
    groups, ld = len(off) - 1, smax + 3
    stride = ld * smax + 7
    rng = rc.rng_of(smax, 12)
    mats = [rng.standard_normal((smax, smax)) for _ in range(groups)]
    flat = slabs(mats, ld, stride)
    sizes = np.diff(off)
    boff = np.concatenate([[0], np.cumsum(sizes * sizes + 2)])[:groups].astype(np.int64)  # two words between the blocks
    out = np.full(int(boff[-1] + sizes[-1] ** 2 + 3), np.nan)
    want = out.copy()
    for g in range(groups):
        sg = int(sizes[g])
        want[boff[g]:boff[g] + sg * sg] = mats[g][:sg, :sg].ravel(order="F")
    keep = flat.copy()
    assert reduce_call(ctx, rc.COMPACT_BLOCKS, [ld, stride, smax, groups], [], [flat, off.copy(), boff, out]) == 0
    assert same_bits(out, want) and same_bits(flat, keep)


# ---- the wide vector sweeps and the mixed fit's preconditioner ------------------------------------------------------
SWEEPS = sc.wide_sweep_cases()
NAN_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def wide_sweep(ctx, kind, K, bw, rhs, a32):
    """agp_debug_wide_sweep: (status, solution, t2, L, the fp32 copy or None); the vector's padding enters as all-ones NaN
    and is checked to come back whole."""
    fn = capi.load_debug().agp_debug_wide_sweep
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 3
    n = K.shape[0]
    z = np.empty(n + 5)
    z.view(np.uint64)[:] = NAN_BITS
    z[:n] = rhs
    t2 = np.zeros(n + 5)
    L = np.zeros((n, n), order="F")
    want32 = a32 or kind == rc.MIXED_PRECONDITION
    L32 = np.zeros((n, n), dtype=np.float32, order="F") if want32 else None
    st = fn(ctx._h, kind, K.ctypes.data, n, bw, int(a32), z.ctypes.data, z.size, t2.ctypes.data, L.ctypes.data,
            None if L32 is None else L32.ctypes.data)
    if st == 0:
        assert np.all(z.view(np.uint64)[n:] == NAN_BITS), "padding behind the vector written"
        if kind == rc.MIXED_PRECONDITION:
            assert np.all(t2.view(np.uint64)[n:] == NAN_BITS), "padding behind the work vector written"
    return st, z[:n].copy(), t2[:n].copy(), np.tril(L), L32


def solved_matrix(L, L32, bw):
    """The matrix the device solved with: the returned factor, its blocks below the bw-wide diagonal ones rounded to fp32 -
    checked bit for bit against the fp32 copy the device made (lower triangle; above it only the pairs' entries)."""
    if L32 is None:
        return L
    n = L.shape[0]
    low = lower_mask(n)
    assert np.array_equal(L32[low], L.astype(np.float32)[low]), "the fp32 copy is not the rounded factor"
    untouched = L32.view(np.uint32) == np.uint32(0xFFFFFFFF)
    assert np.all(untouched[~rc.pair_written_mask(n)]), "the fp32 copy was written above the pairs of the diagonal"
    T = sc.fp32_off_diagonal(L, bw)
    for i in range(0, n, bw):  # the off-diagonal blocks of T are the device's fp32 entries, bit for bit
        assert np.array_equal(T[i + bw:, i:i + bw], L32[i + bw:, i:i + bw].astype(np.float64))
    return T


@pytest.mark.parametrize("case", SWEEPS, ids=[c["id"] for c in SWEEPS])
def test_wide_vector_sweeps(ctx, case):
    """forward_solve_vec_wide and backward_solve_vec_wide, on the fp64 factor and with the fp32 copy of its off-diagonal
    blocks, and the wide branch of backward_solve_vec_any where the product takes it (BW = 512)."""
    n, bw = case["n"], case["bw"]
    K, B = sc.spd_matrix(case["family"], n), sc.wide_sweep_rhs(case)
    runs = [(rc.FWD_VEC_WIDE, False, False), (rc.FWD_VEC_WIDE, True, False), (rc.BWD_VEC_WIDE, False, True), (rc.BWD_VEC_WIDE, True, True)]
    if bw == 512:
        runs.append((rc.BWD_VEC_ANY_WIDE, False, True))
    worst = 0.0
    for kind, a32, transposed in runs:
        st, x, _, L, L32 = wide_sweep(ctx, kind, K, bw, B[:, 0], a32)
        assert st == 0, (kind, a32, st)
        ratio = sc.residual_ratio(solved_matrix(L, L32, bw), x, B, bw, transposed)
        print(f"wide sweep {case['id']} kind {kind} fp32 copy {a32}: residual / bound {ratio:.3g}")
        assert ratio <= 1.0, (kind, a32, ratio)
        worst = max(worst, ratio)
    print(f"wide sweeps {case['id']}: worst residual / bound {worst:.3g}")


@pytest.mark.parametrize("case", SWEEPS, ids=[c["id"] for c in SWEEPS])
def test_mixed_preconditioner(ctx, case):
    """One application out = Lt^-T Lt^-1 in, each sweep on its own: |in - Lt t2| and |t2 - Lt^T out| against the bound, Lt
    the factor with its off-diagonal blocks in fp32."""
    n, bw = case["n"], case["bw"]
    K, B = sc.spd_matrix(case["family"], n), sc.wide_sweep_rhs(case)
    st, out, t2, L, L32 = wide_sweep(ctx, rc.MIXED_PRECONDITION, K, bw, B[:, 0], False)
    assert st == 0, st
    T = solved_matrix(L, L32, bw)
    fwd = sc.residual_ratio(T, t2, B, bw, False)
    bwd = sc.residual_ratio(T, out, t2.reshape(n, 1), bw, True)
    print(f"mixed preconditioner {case['id']}: residual / bound forward {fwd:.3g}, backward {bwd:.3g}")
    assert fwd <= 1.0 and bwd <= 1.0, (fwd, bwd)


def test_wide_sweep_refuses_other_widths(ctx):
    """BW is 512 or 1024 and divides n; backward_solve_vec_any only at the width the product gives it."""
    K = np.asfortranarray(np.eye(1024))
    for kind, n, bw in ((rc.FWD_VEC_WIDE, 1024, 256), (rc.MIXED_PRECONDITION, 1024, 4096), (rc.BWD_VEC_WIDE, 768, 512),
                        (rc.BWD_VEC_ANY_WIDE, 1024, 512), (rc.BWD_VEC_ANY_WIDE, 1024, 1024)):
        st, _, _, _, _ = wide_sweep(ctx, kind, np.asfortranarray(K[:n, :n]), bw, np.ones(n), False)
        assert st == INVALID_ARGUMENT, (kind, n, bw, st)
