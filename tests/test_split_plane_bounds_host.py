"""The checks of tests/test_split_plane_kernels_gpu.py are sound and they bite, before any GPU is involved.

  * The restatement obeys the statements of the header of csrc/gemm_split_planes.hip: |x - hi - mid - lo| <= 2^-25 |x|;
    |r x - h1 - h2| <= 2^-22 |r x| where |r x| >= 2^-2 and <= 2^-25 below; and the included partial products lie within
    the distance of P P^T that follows from them (split_plane_cases.distance_allowed).
  * Every part B case adds exactly: split_plane_cases.exact_need stays below 24 bits (asserted where a case is built).
  * An emulation of the kernels from the plane image - tile by tile, chunk by chunk, instruction by instruction; exact
    sums for part B, fp32 accumulators in kernel order for part C - passes every case of the GPU module unmutated.
  * Each fault below, put into that emulation, fails at least one named case:
        drop / double     each partial product left out / taken twice
        swap_planes       the first two planes exchanged (fp16 x 2 with four products: the SAME sum, caught by the plane
                          bytes of part A only)
        third_stride      the third bf16 plane read at the second's stride
        chunk_off         K chunk c + 1 read for chunk c
        rowab             the row and the column operand exchanged (a transposed tile: shows where N < M or bi != bj)
        scales_first0     the scales of diag[0 ..] instead of diag[first_row ..], in the conversion and the epilogue / in
                          the conversion alone
        irs_row_for_col   1 / r of the row used for the column
        ragged_past_M     a ragged tile written below row M (the padding rows are signalling NaNs: any write shows)
        tile_twice        a tile of the order table done twice
  * Which faults only part B catches: a dropped or doubled lo*hi, hi*lo, mid*mid (bf16 x 3) and h2*h2 (fp16 x 2) pass the
    bound of part C on every dense case - as they must, their size is that of the fp32 accumulation noise - and fail
    part B.  mid*hi, hi*mid, h2*h1, h1*h2 and the leading products fail part C too (K = 32, 64).
  * h2*h2 beside h1*h1 on rows of 16 non-zeros is beyond an exact check (32 bits), so on such rows
    test_split_plane_settings_belong_to_the_context ("B must differ from A") stays the only witness; the f16-pair panel of
    3 non-zeros per row holds all four products in 23.6 bits and is the exact witness of the fourth.
No GPU."""
import numpy as np
import pytest

import albatross_amd as ab  # noqa: F401  (the package must import without a GPU)

import split_plane_cases as sc


def test_longdouble_is_wider_than_double():
    assert sc.HAVE_LONGDOUBLE


def test_bound_constants():
    """the counts of the derivation, spelled out"""
    assert sc.V_BF16.roundings(64) == 33 * 6 * 2 and sc.V_F16.roundings(64) == 33 * 4 * 2
    assert sc.Variant(sc.F16X2, 3, 64).roundings(64) == 33 * 3 * 2 and sc.V_FP32.roundings(64) == 5 * 16
    assert sc.rows_pad(1) == 256 and sc.rows_pad(128) == 256 and sc.rows_pad(129) == 384
    assert sc.split_planes_bytes(3, 129, 96) == 2 * 3 * 384 * 128 and sc.fp32_ld(505) == 520 and sc.fp32_ld(129) == 136


@pytest.mark.parametrize("rows,K", [(257, 512), (129, 96), (1, 32)])
def test_split_statements_of_the_header(rows, K):
    X, P16, diag, P = sc.conversion_panel(rows, K, 37)
    x = P[:rows]
    V = sc.bf16_val(sc.split_bf16x3(x))
    assert np.all(np.abs(x - V[0] - V[1] - V[2]) <= 2. ** -25 * np.abs(x))
    rs, _ = sc.row_scales(diag)
    H = sc.plane_values(sc.F16X2, sc.split_f16x2(P16[:rows], rs[37:]))
    err = np.abs(X - H[0] - H[1])
    big = np.abs(X) >= 2. ** -2
    assert np.all(err[big] <= 2. ** -22 * np.abs(X[big])) and np.all(err[~big] <= 2. ** -25)
    assert np.all(np.abs(H[1]) <= 2. ** -11 * np.abs(X) + 2. ** -25)   # (what distance_allowed takes for a dropped h2*h2)
    assert np.all(np.abs(V[1]) <= 2. ** -8 * np.abs(x)) and np.all(np.abs(V[2]) <= 2. ** -16 * np.abs(x))


def test_special_values_hit_their_roundings():
    """the panel of part A holds what its docstrings promise"""
    v = sc.special_values()
    h1 = v.astype(np.float16).astype(np.float64)
    assert (np.abs(v - h1) == 2. ** -11).sum() >= 8                                     # fp16 ties in [1, 2)
    assert (v.astype(np.float32).astype(np.float16) != v.astype(np.float16)).sum() >= 4  # double rounding would differ
    h2 = (v - h1).astype(np.float16)
    sub = h2.view(np.uint16) & 0x7fff
    assert ((sub > 0) & (sub < 0x400)).sum() >= 6 and ((v != h1) & (h2 == 0)).sum() >= 4  # subnormal / vanishing residuals
    f = v.astype(np.float32).astype(np.float64)
    m, e = np.frexp(f)
    assert np.array_equal(sc.bf16_val(sc.bf16_rn_bits(f)), np.ldexp(np.round(np.ldexp(m, 8)), e - 8))  # the bit trick rounds to even
    assert (np.abs(f - sc.bf16_val(sc.bf16_rn_bits(f))) == 2. ** -8).sum() >= 8                         # bf16 ties in [1, 2)
    m64, e64 = np.frexp(v)
    once = np.ldexp(np.round(np.ldexp(m64, 8)), e64 - 8)   # x rounded to bf16 ONCE
    assert (once != sc.bf16_val(sc.bf16_rn_bits(f))).sum() >= 4   # ... is not what the two roundings of the kernel give
    assert np.signbit(v[v == 0]).any()
    r, ir = sc.row_scales(sc.special_diagonals())
    assert np.array_equal(r * ir, np.ones_like(r)) and r[0] == 2. ** 10 and r[1] == 2. ** 11 and r[2] == 2. ** 10


def _variants_of(cases):
    return sorted({v for c in cases for v in c.variants if v.stages(c.K)}, key=lambda v: v.name)


@pytest.mark.parametrize("variant", sc.ALL_VARIANTS, ids=lambda v: v.name)
def test_unmutated_emulation_passes_every_case(variant):
    b, c = sc.named_gpu_cases(variant)
    assert b
    for case in b:
        ok, why, _ = sc.check(case, variant, sc.emulate(case, variant))
        assert ok, (case.name, why)
    worst = 0.
    for case in c:
        if case.M > 300 and (case.K != 64 or case.name.startswith("C-badly")):
            continue   # (one large dense case is enough here)
        ok, why, ratio = sc.check(case, variant, sc.emulate(case, variant, arith="fp32"))
        assert ok, (case.name, why)
        worst = max(worst, ratio)
    if c:
        print(f"{variant.name}: sequential fp32 emulation reaches {worst:.3g} of the bound")
    assert worst <= 0.5


@pytest.mark.parametrize("variant", sc.C_VARIANTS, ids=lambda v: v.name)
def test_included_terms_near_the_full_product(variant):
    for case in sc.named_gpu_cases(variant)[1]:
        if case.M > 300:
            continue
        S, _, _ = sc.products_ld(case, variant)
        o = case.row_offset
        Pi = case.P[o:o + case.M, :case.K].astype(np.longdouble)
        full = Pi @ case.P[o:o + case.N, :case.K].astype(np.longdouble).T
        dist = np.abs(S * sc.pair_scale(case, variant) - full).astype(np.float64)
        assert np.all(dist <= sc.distance_allowed(case, variant)), case.name


def test_exact_need_of_the_designs():
    """the margins measured when the designs were made: below 24 bits each (asserted for EVERY case where it is built)"""
    need = {k: sc.exact_need(sc.b2_case(k, 64), v) for k, v in [("bf16-rich", sc.V_BF16), ("bf16-cross", sc.V_BF16), ("f16-cross", sc.V_F16),
                                                               ("f16-pair", sc.V_F16)]}
    need["B3"] = sc.exact_need(sc.b3_case(64), sc.V_F16)
    need["B1 K = 512"] = sc.exact_need(sc.b1_case(700, 128, 572, 572, 512), sc.V_BF16)
    need["bulk (upper bound)"] = sc.exact_need(sc.b1_bulk_case(), sc.V_F16)
    print({k: round(float(v), 1) for k, v in need.items()})
    assert all(v < 24. for v in need.values()) and 22.9 < need["bf16-rich"] < 23.1 and 23.5 < need["f16-pair"] < 23.7


def SMALL_B(v):
    """the part B cases a fault is looked for in: the shallow ones, and one of eight K chunks"""
    return [c for c in sc.named_gpu_cases(v)[0] if (c.K <= 96 and c.rows <= 400) or (c.K == 512 and c.rows <= 129)]


def caught_by(variant, fault, cases, arith="exact"):
    """the names of the cases whose check fails on the emulation with the fault"""
    return [c.name for c in cases if not sc.check(c, variant, sc.emulate(c, variant, fault, arith))[0]]


def term_faults(variant):
    return [(kind, pair) for kind in ("drop", "double") for pair in variant.pairs]


# pairs whose loss part C cannot see (their size is that of the accumulation noise): part B is their only witness
ONLY_B = {sc.BF16X3: {(2, 0), (0, 2), (1, 1)}, sc.F16X2: {(1, 1)}, sc.FP32: set()}


@pytest.mark.parametrize("variant", [sc.V_FP32, sc.V_BF16, sc.Variant(sc.F16X2, 4, 32), sc.Variant(sc.F16X2, 3, 32), sc.Variant(sc.F16X2, 4, 64)],
                         ids=lambda v: v.name)
def test_every_term_fault_is_caught(variant):
    b = SMALL_B(variant)
    dense = [c for c in sc.named_gpu_cases(variant)[1] if c.M < 300]
    for fault in term_faults(variant):
        hit_b = caught_by(variant, fault, b)
        hit_c = caught_by(variant, fault, dense, "fp32")
        name = sc.PAIR_NAMES[variant.products][fault[1]]
        print(f"{variant.name} {fault[0]} {name}: part B {hit_b[:3]}{'...' if len(hit_b) > 3 else ''}, part C {hit_c}")
        assert hit_b, (variant.name, fault)
        if fault[1] in ONLY_B[variant.products]:
            assert not hit_c, (variant.name, fault, hit_c)
        else:
            assert hit_c, (variant.name, fault)


@pytest.mark.parametrize("variant", [sc.V_FP32, sc.V_BF16, sc.Variant(sc.F16X2, 4, 32), sc.Variant(sc.F16X2, 3, 64)], ids=lambda v: v.name)
def test_every_addressing_fault_is_caught(variant):
    b = SMALL_B(variant)
    f16, bf16, planes = variant.products == sc.F16X2, variant.products == sc.BF16X3, variant.products != sc.FP32
    faults = ["rowab", "ragged_past_M", "tile_twice"]
    faults += ["chunk_off"] if planes else []
    faults += ["third_stride"] if bf16 else []
    faults += ["swap_planes"] if bf16 or (f16 and variant.terms == 3) else []
    faults += ["scales_first0", "scales_first0_convert", "irs_row_for_col"] if f16 else []
    for fault in faults:
        hit = caught_by(variant, fault, b)
        print(f"{variant.name} {fault}: {hit[:4]}{'...' if len(hit) > 4 else ''}")
        assert hit, (variant.name, fault)
    if f16 and variant.terms == 4:   # all four products: exchanging the planes exchanges terms of the same sum
        assert not caught_by(variant, "swap_planes", b)
        case = sc.b2_case("f16-cross", 64)
        bits = sc.staged_bits(variant, case.P, case.rows, case.K, case.scales()[0])
        assert not np.array_equal(sc.plane_image(bits, 64, 32), sc.plane_image(bits[::-1], 64, 32))   # ... part A sees it


def test_tile_done_twice_in_the_bulk_case():
    case = sc.b1_bulk_case()
    assert len(sc.lower_tiles(case.M, case.N)) == 1081
    want = sc.expected(case, sc.V_F16)
    assert sc.check(case, sc.V_F16, sc.emulate(case, sc.V_F16), want)[0]
    assert not sc.check(case, sc.V_F16, sc.emulate(case, sc.V_F16, "tile_twice"), want)[0]
