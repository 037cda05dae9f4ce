"""The low-precision products of the mixed fit (csrc/gemm_split_planes.hip, the fp32 copy of csrc/gemm.hip), staged and
applied through the fit's own PanelStager / StagedPanel (agp_debug_split_plane_step), against the numpy restatement of
tests/split_plane_cases.py:

  A  the conversions bit for bit - every byte of the planes, layout and padding included, the fp32 copy, the row scales;
  B  the products bit for bit on panels whose partial products add exactly in fp32 in any order (B1 plain integers over
     every shape and the tile-order table, B2 panels that occupy the small planes, B3 an fp16 second plane of
     subnormals);
  C  dense panels within the derived componentwise bound of the cases module, worst error / bound printed.

tests/test_split_plane_bounds_host.py shows on an emulation that these cases catch a dropped, doubled or misplaced term
and the addressing faults a tile kernel can have.

Measured on an MI355X: the 16-bit matrix pipe keeps subnormal fp16 inputs (test_b3_subnormal_second_plane); worst error /
bound of part C 0.03-0.06 for the fp32 copy, 0.004-0.008 for bf16 x 3, 0.006-0.011 for fp16 x 2."""
import ctypes as C

import numpy as np
import pytest

from albatross_amd import _capi as capi

import split_plane_cases as sc

pytestmark = pytest.mark.gpu


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def dbg(ctx):
    lib = capi.load_debug()
    lib.agp_debug_split_plane_step.restype = C.c_int
    lib.agp_debug_split_plane_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                               C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture
def context_for(ctx, make_ctx, monkeypatch):
    """the context whose fp16 x 2 settings are the variant's: the session's for the defaults, a new one otherwise"""
    def get(variant):
        if variant.default_context:
            return ctx
        monkeypatch.setenv("AGP_F16X2_TERMS", str(variant.terms))
        monkeypatch.setenv("AGP_F16X2_CHUNK", str(variant.chunk))
        return make_ctx()
    return get


def stage(c, dbg, variant, P, rows, K, diag, first_row, copy_bytes=0, scales=False):
    """the conversion alone: (status, the copy as bytes, ld32, rs, irs)"""
    copy = np.zeros(copy_bytes, np.uint8) if copy_bytes else None
    n = first_row + rows
    rs, irs = (np.zeros(n), np.zeros(n)) if scales else (None, None)
    ld32 = C.c_int64(-1)
    st = dbg.agp_debug_split_plane_step(c._h, variant.products, _p(P), P.shape[0], rows, K, _p(diag), first_row, None, 0, 0, 0, 0,
                                        _p(copy), copy_bytes, C.byref(ld32), _p(rs), _p(irs))
    return st, copy, ld32.value, rs, irs


def apply(c, dbg, variant, case):
    """the staged update of a case: (status, C as it came back)"""
    got = case.C0.copy(order="F")
    st = dbg.agp_debug_split_plane_step(c._h, variant.products, _p(case.P), case.ldp, case.rows, case.K, _p(case.diag), case.first_row,
                                        _p(got), case.ldc, case.row_offset, case.M, case.N, None, 0, None, None, None)
    return st, got


def run_cases(c, dbg, variant, cases):
    """every case through the kernel; all the verdicts at once"""
    failures = []
    for case in cases:
        st, got = apply(c, dbg, variant, case)
        if st != 0:
            failures.append(f"{case.name}: status {st}")
            continue
        ok, why, _ = sc.check(case, variant, got)
        if not ok:
            failures.append(f"{case.name}: {why}")
    assert not failures, f"{variant.name}: " + " | ".join(failures)


# ---- A: conversions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_row", sc.FIRST_ROWS)
def test_row_scales(ctx, dbg, first_row):
    """r = 2^(14 - e) and 1 / r for the whole diagonal handed to PanelStager::begin: sqrt(d) at a power of two and one ulp
    either side, the clamp at 2^+-200 (1e-130, 1e130, a subnormal), and r = 1 / r = 1 for 0, negative, NaN, inf and >= 1e300."""
    rows, K = 257, 32
    _, P16, diag, _ = sc.conversion_panel(rows, K, first_row)
    st, _, _, rs, irs = stage(ctx, dbg, sc.V_F16, P16, rows, K, diag, first_row, scales=True)
    assert st == 0
    want_r, want_ir = sc.row_scales(diag)
    assert sc.same_bits(rs, want_r) and sc.same_bits(irs, want_ir)
    assert set(np.log2(want_r).astype(int)) >= {214, -186} and (want_r == 1.).sum() >= 7   # the clamp and the rejects are there


@pytest.mark.parametrize("K", sc.CONVERSION_K)
def test_convert_bf16x3_bit_for_bit(ctx, dbg, K):
    """Three bf16 planes [plane][k / 32][rows_pad][k % 32], every byte: ties of each of the three roundings in both parities,
    values whose (float) rounding changes the bf16 result, -0.0, padding rows of zero bits, nothing written behind the
    third plane (K = 96: the buffer is sized for K rounded up to 64)."""
    for rows in sc.CONVERSION_ROWS:
        _, _, diag, P = sc.conversion_panel(rows, K, 0)
        nbytes = sc.split_planes_bytes(3, rows, K)
        st, copy, _, _, _ = stage(ctx, dbg, sc.V_BF16, P, rows, K, diag, 0, nbytes)
        assert st == 0
        want = sc.plane_image(sc.split_bf16x3(P[:rows]), K, 32)
        assert np.array_equal(copy.view(np.uint16), want), f"rows = {rows}"


@pytest.mark.parametrize("K", sc.CONVERSION_K + (16, 48))
def test_convert_fp32_bit_for_bit(ctx, dbg, K):
    """The fp32 copy: (float) x at k ld32 + row, nothing else written."""
    for rows in sc.CONVERSION_ROWS + (505, 512):   # (ld32 = 512 + 8: no multiple of 512)
        _, _, diag, P = sc.conversion_panel(rows, K, 0)
        want = sc.fp32_image(P, rows, K)
        st, copy, ld32, _, _ = stage(ctx, dbg, sc.V_FP32, P, rows, K, diag, 0, want.nbytes)
        assert st == 0 and ld32 == want.shape[1]
        assert np.array_equal(copy.view(np.uint32).reshape(want.shape), want), f"rows = {rows}"


@pytest.mark.parametrize("first_row", sc.FIRST_ROWS)
@pytest.mark.parametrize("K", sc.CONVERSION_K)
@pytest.mark.parametrize("chunk", [32, 64])
def test_convert_f16x2_bit_for_bit(context_for, dbg, chunk, K, first_row):
    """Two fp16 planes [plane][k / CH][rows_pad][k % CH] of the rows scaled by the scales of diag[first_row ..], every byte:
    ties of both roundings, values a double -> float -> half conversion would round differently, -0.0, second planes that
    are subnormal, that tie at 2^-25 and that vanish.  K = 96 with CH = 64 is no whole number of chunks: not staged, and
    reported as such."""
    variant = sc.Variant(sc.F16X2, 4, chunk)
    c = context_for(variant)
    for rows in sc.CONVERSION_ROWS:
        X, P16, diag, _ = sc.conversion_panel(rows, K, first_row)
        nbytes = sc.split_planes_bytes(2, rows, K)
        st, copy, _, _, _ = stage(c, dbg, variant, P16, rows, K, diag, first_row, nbytes)
        if not variant.stages(K):
            assert st == sc.NOT_STAGED
            continue
        assert st == 0
        rs, _ = sc.row_scales(diag)
        bits = sc.split_f16x2(P16[:rows], rs[first_row:])
        assert np.array_equal(bits, sc.split_f16x2(X, np.ones(rows)))   # (the panel was made so that r x = X)
        assert np.array_equal(copy.view(np.uint16), sc.plane_image(bits, K, chunk)), f"rows = {rows}"


# ---- B: exactly summable panels ----------------------------------------------------------------------------------------
def _staging(variants, depths):
    return [pytest.param(v, K, id=f"{v.name}-K{K}") for v in variants for K in depths if v.stages(K)]


@pytest.mark.parametrize("variant,K", _staging(sc.ALL_VARIANTS, sc.B1_K) + _staging([sc.V_FP32], sc.B1_K_FP32_ONLY))
def test_b1_plain_integers(context_for, dbg, variant, K):
    """Integers in [-2, 2]: whole, ragged and single tiles, the next-block-column shape (N < M, N = 1), row offsets that are
    and are not multiples of the tile, the last whole tile of the panel; one and several K chunks.  Equal to the last bit
    on the lower tiles, and not a bit changed in the padding rows, the guard columns and the strict upper tiles."""
    run_cases(context_for(variant), dbg, variant, [sc.b1_case(*shape, K) for shape in sc.B1_SHAPES])


@pytest.mark.parametrize("variant", sc.ALL_VARIANTS, ids=lambda v: v.name)
def test_b1_rows_scaled_by_powers_of_two(context_for, dbg, variant):
    """The rows times 2^-30 .. 2^30 with the matching diagonal, the panel at first_row = 37 of it: the fp16 scales undo the
    powers exactly (those of the ROW for the rows, of the COLUMN for the columns), bf16 x 3 and fp32 take them unchanged."""
    run_cases(context_for(variant), dbg, variant, [sc.b1_case(129, 0, 129, 129, 64, True), sc.b1_case(700, 128, 572, 572, 64, True)])


@pytest.mark.parametrize("variant", [sc.V_FP32, sc.V_BF16, sc.V_F16], ids=lambda v: v.name)
def test_b1_bulk_tile_order(ctx, dbg, variant):
    """M = N = 5761: 1081 tiles, so StagedPanel::apply takes them in the order of the table - every tile once, its -1
    fillers none - with a ragged last tile row."""
    run_cases(ctx, dbg, variant, [sc.b1_bulk_case()])


@pytest.mark.parametrize("K", sc.B2_K)
@pytest.mark.parametrize("kind", ["bf16-rich", "bf16-cross"])
def test_b2_bf16_small_terms(ctx, dbg, kind, K):
    """All three planes occupied and every one of the six products exact: a lost lo*hi, hi*lo or mid*mid, a swapped pair or
    a wrong stride of the third plane changes bits."""
    run_cases(ctx, dbg, sc.V_BF16, [sc.b2_case(kind, K)])


@pytest.mark.parametrize("variant,K", _staging(sc.F16_VARIANTS, sc.B2_K))
def test_b2_f16_cross_terms(context_for, dbg, variant, K):
    """h2*h1 and h1*h2, each alone beside h1*h1, exact (TERMS 3 and 4 agree on these entries: h2*h2 is zero there)."""
    run_cases(context_for(variant), dbg, variant, [sc.b2_case("f16-cross", K)])


@pytest.mark.parametrize("variant,K", _staging(sc.F16_VARIANTS, sc.B2_K))
def test_b2_f16_all_four_terms(context_for, dbg, variant, K):
    """Three non-zeros per row: h2*h2 beside h2*h1, h1*h2 and h1*h1, all four exact - with TERMS = 4 the fourth product is
    there to the last bit, with TERMS = 3 it is absent to the last bit."""
    run_cases(context_for(variant), dbg, variant, [sc.b2_case("f16-pair", K)])


@pytest.mark.parametrize("variant,K", _staging(sc.F16_VARIANTS, sc.B3_K))
def test_b3_subnormal_second_plane(context_for, dbg, variant, K):
    """A second plane of fp16 SUBNORMALS (b 2^-24) against integer rows: v_mfma_f32_16x16x32_f16 takes subnormal inputs at
    their value - the result holds h2*h1 to the last bit and differs from what a pipe that flushed them would leave."""
    case = sc.b3_case(K)
    st, got = apply(context_for(variant), dbg, variant, case)
    assert st == 0
    kept, _, _ = sc.check(case, variant, got)
    flushed, _, _ = sc.check(case, variant, got, want=sc.flushed_expected(case, variant))
    print(f"{case.name} {variant.name}: subnormal inputs kept {kept}, flushed {flushed}")
    assert kept and not flushed


# ---- C: dense panels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.C_SHAPES, ids=lambda s: f"M{s[2]}")
@pytest.mark.parametrize("data", sc.C_DATA)
@pytest.mark.parametrize("variant,K", _staging(sc.C_VARIANTS, sc.C_K))
def test_dense_panel_within_bound(context_for, dbg, variant, data, shape, K):
    """|got - ref| <= T 2^-23 sum|partial products| / (r_i r_j) + 2^-53 |ref| on every entry of the lower tiles, ref from the
    included partial products of the restated planes in longdouble; nothing else written."""
    case = sc.c_case(data, *shape, K)
    st, got = apply(context_for(variant), dbg, variant, case)
    assert st == 0
    ok, why, ratio = sc.check(case, variant, got)
    print(f"{case.name} {variant.name}: worst error / bound = {ratio:.3g}")
    assert ok, why
