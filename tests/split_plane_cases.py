"""The split-plane kernels of the mixed fit (csrc/gemm_split_planes.hip, reached through PanelStager / StagedPanel of
csrc/chol.hip) restated in numpy, and the cases tests/test_split_plane_kernels_gpu.py runs them on.

The conversions are restated bit for bit.  The products are checked on panels whose partial products can be added in fp32
IN ANY ORDER without a rounding: every partial product of a checked entry is a multiple of a granularity g, and the sum of
their absolute values stays below 2^24 g, so every partial sum is one of the 2^25 multiples of g that fp32 holds exactly.
The result is then known to the last bit whatever the matrix instruction does inside, and a lost, doubled or misplaced
term shows.  exact_need() computes that margin per entry and every case builder asserts it.

A dense panel cannot be exact; part C holds it to a componentwise bound instead:
    |got - ref| <= T 2^-23 sum|partial products| / (r_i r_j) + 2^-53 |ref|,    T = (k of an instruction + 1) x instructions
with ref = C - (the included partial products of the restated planes, in longdouble) - the kernel's contract, not P P^T.
T counts one faithful rounding (< one ulp = 2^-23 of the partial sum, itself <= sum|partial products|) per product added
and one per accumulator handed from instruction to instruction, whatever the order inside the instruction: 33 per
v_mfma_f32_16x16x32_{f16,bf16}, 5 per v_mfma_f32_16x16x4_f32; the last term is the fp64 subtraction of the epilogue."""
import functools
from dataclasses import dataclass

import numpy as np

GT = 128            # tile of the kernels
GUARD_COLS = 128    # agp_debug_split_plane_step: columns of C behind the N updated ones that travel to the device and back
FP32, BF16X3, F16X2 = 3, 4, 5   # factor_plan.h: BulkProducts
SCALE_EXP = 14
NOT_STAGED, OTHER_PRODUCTS = 100, 101   # debug_api.hip: AGP_DEBUG_NOT_STAGED, AGP_DEBUG_OTHER_PRODUCTS
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63

# (plane of the C-COLUMN operand, plane of the C-ROW operand) of every matrix instruction of a K chunk, in kernel order
BF16_PAIRS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # lo hi, hi lo, mid mid, mid hi, hi mid, hi hi
F16_PAIRS = ((1, 1), (1, 0), (0, 1), (0, 0))                    # h2 h2 (TERMS = 4 only), h2 h1, h1 h2, h1 h1
PAIR_NAMES = {BF16X3: {(2, 0): "lo*hi", (0, 2): "hi*lo", (1, 1): "mid*mid", (1, 0): "mid*hi", (0, 1): "hi*mid", (0, 0): "hi*hi"},
              F16X2: {(1, 1): "h2*h2", (1, 0): "h2*h1", (0, 1): "h1*h2", (0, 0): "h1*h1"}, FP32: {(0, 0): "f32*f32"}}


@dataclass(frozen=True)
class Variant:
    """which kernel runs: the products, and for fp16 x 2 the context's AGP_F16X2_TERMS / AGP_F16X2_CHUNK"""
    products: int
    terms: int = 4
    chunk: int = 32

    @property
    def name(self):
        return {FP32: "fp32", BF16X3: "bf16x3"}.get(self.products, f"f16x2-t{self.terms}-ch{self.chunk}")

    @property
    def ch(self):
        """k per chunk of the plane layout"""
        return self.chunk if self.products == F16X2 else 32

    @property
    def pairs(self):
        if self.products == BF16X3:
            return BF16_PAIRS
        if self.products == F16X2:
            return F16_PAIRS if self.terms == 4 else F16_PAIRS[1:]
        return ((0, 0),)

    @property
    def default_context(self):
        return self.products != F16X2 or (self.terms == 4 and self.chunk == 32)

    def stages(self, K):
        """PanelStager::stage makes a copy at this depth"""
        return K > 0 and (self.products == FP32 or K % self.ch == 0)

    def roundings(self, K):
        """T of the bound: (k of one matrix instruction + 1) x the instructions accumulated into an entry"""
        if self.products == FP32:
            return 5 * ((K + 3) // 4)
        return 33 * len(self.pairs) * (K // 32)


V_FP32, V_BF16, V_F16 = Variant(FP32), Variant(BF16X3), Variant(F16X2)
F16_VARIANTS = tuple(Variant(F16X2, t, c) for c in (32, 64) for t in (4, 3))
ALL_VARIANTS = (V_FP32, V_BF16) + F16_VARIANTS


# ---- the conversions, bit for bit ---------------------------------------------------------------------------------------
def rows_pad(rows):
    return (rows + GT - 1) // GT * GT + GT


def split_planes_bytes(planes, rows, K):
    return 2 * planes * rows_pad(rows) * ((K + 63) // 64 * 64)


def fp32_ld(rows):
    """PanelStager::stage: whole groups of 8 rows and no multiple of 512"""
    ld = (rows + 7) // 8 * 8
    return ld + 8 if ld % 512 == 0 else ld


def bf16_rn_bits(f32):
    """bf16_rn of the kernel file: round to nearest even on the bits of a float"""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7fff + ((u >> 16) & 1)
    return ((u >> 16) & 0xffff).astype(np.uint16)


def bf16_val(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def split_bf16x3(P):
    """(3, rows, K) uint16: hi = rn((float) x), mid = rn((float)(x - hi)), lo = rn((float)(x - hi - mid)), residuals in fp64"""
    out = np.empty((3,) + P.shape, np.uint16)
    r = np.array(P, dtype=np.float64)
    for p in range(3):
        out[p] = bf16_rn_bits(r.astype(np.float32))
        r = r - bf16_val(out[p])
    return out


def row_scales(diag):
    """f16x2_row_scales_kernel: r = 2^(14 - e), sqrt(d) = m 2^e with 0.5 <= m < 1, e clamped to +-200; r = 1 / r = 1 for a
    diagonal that is not a positive number below 1e300"""
    d = np.asarray(diag, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (d > 0.) & (d < 1e300)
        _, e = np.frexp(np.sqrt(np.where(ok, d, 1.)))
    e = np.clip(e, -200, 200)
    r = np.where(ok, np.ldexp(1., SCALE_EXP - e), 1.)
    ir = np.where(ok, np.ldexp(1., e - SCALE_EXP), 1.)
    return r, ir


def split_f16x2(P, rs):
    """(2, rows, K) uint16: h1 = fp16(r x), h2 = fp16(r x - h1), each ONE rounding from fp64 (as astype is)"""
    with np.errstate(over="ignore", invalid="ignore"):
        x = rs[:, None] * np.asarray(P, dtype=np.float64)
        h1 = x.astype(np.float16)
        h2 = (x - h1.astype(np.float64)).astype(np.float16)
    return np.stack([h1.view(np.uint16), h2.view(np.uint16)])


def plane_values(products, bits):
    if products == BF16X3:
        return bf16_val(bits)
    return bits.view(np.float16).astype(np.float64)


def plane_image(bits, K, ch, total_bytes=None):
    """The planes as they lie in memory, uint16: [plane][k / ch][rows_pad][k % ch], padding rows all zero bits, and 0xffff
    (what the debug entry fills the buffer with) behind the last plane up to split_planes_bytes."""
    planes, rows, _ = bits.shape
    rp = rows_pad(rows)
    img = np.zeros((planes, K // ch, rp, ch), np.uint16)
    img[:, :, :rows, :] = bits.reshape(planes, rows, K // ch, ch).transpose(0, 2, 1, 3)
    total = (split_planes_bytes(planes, rows, K) if total_bytes is None else total_bytes) // 2
    out = np.full(total, 0xffff, np.uint16)
    out[:img.size] = img.reshape(-1)
    return out


def fp32_image(P, rows, K):
    """the fp32 copy as uint32 (K, ld32): column k at k ld32, 0xffffffff where nothing is written"""
    ld = fp32_ld(rows)
    img = np.full((K, ld), 0xffffffff, np.uint32)
    img[:, :rows] = np.asarray(P[:rows, :K], dtype=np.float64).T.astype(np.float32).view(np.uint32)
    return img


def staged_bits(variant, P, rows, K, rs):
    """(planes, rows, K) uint16 of the copy (fp32: None)"""
    if variant.products == BF16X3:
        return split_bf16x3(P[:rows, :K])
    if variant.products == F16X2:
        return split_f16x2(P[:rows, :K], rs)
    return None


def staged_values(variant, P, rows, K, rs):
    """(planes, rows, K) float64: what the matrix instructions multiply (fp16 x 2: in scaled units)"""
    if variant.products == FP32:
        return np.asarray(P[:rows, :K], dtype=np.float64).astype(np.float32).astype(np.float64)[None]
    return plane_values(variant.products, staged_bits(variant, P, rows, K, rs))


# ---- part A: panels that hit every rounding ------------------------------------------------------------------------------
CONVERSION_ROWS = (1, 127, 128, 129, 255, 256, 257)
CONVERSION_K = (32, 64, 96, 512)
FIRST_ROWS = (0, 37)


def special_values():
    """Scaled-unit values at the edges of each rounding (and their negatives)."""
    v = [0.0]
    for m in (0, 1, 2, 3):   # exact ties, both parities of the kept mantissa
        v += [1 + (m + .5) * 2.**-10,                              # fp16 h1
              1 + (m + .5) * 2.**-7,                               # bf16 hi
              1 + 2.**-10 * (1 + (m + .5) * 2.**-7),               # bf16 mid (hi = 1)
              1 + 2.**-10 + 2.**-19 * (1 + (m + .5) * 2.**-7),     # bf16 lo (hi = 1, mid = 2^-10)
              1 + 2.**-12 * (1 + (m + .5) * 2.**-10)]              # fp16 h2 (h1 = 1)
    # double rounding: (float) x lands on a bf16 tie that x itself is off (the kernel rounds twice, and so does the restatement)
    v += [1 + 2.**-8 + 2.**-40, 1 + 3 * 2.**-8 - 2.**-40, 1 + 2.**-8 - 2.**-40, 1 + 3 * 2.**-8 + 2.**-40]
    # ... and a double -> float -> half conversion would land on an fp16 tie that x is off (the kernel rounds ONCE)
    v += [1 + 2.**-11 + 2.**-40, 1 + 3 * 2.**-11 - 2.**-40, 1 + 2.**-11 - 2.**-40, 1 + 3 * 2.**-11 + 2.**-40]
    # fp16 residuals that are subnormal, that tie at half the smallest subnormal, and that vanish
    v += [1 + b * 2.**-24 for b in (1, 3, 5, 100)] + [1 + 2.**-25, 1 + 3 * 2.**-25, 1 + 2.**-26, 1 + 3 * 2.**-26, 1 + 2.**-30]
    # small and large magnitudes: h1 itself subnormal or zero, the top of the scaled range
    v += [2.**-2, 1.2345 * 2.**-3, 2.**-14 * 1.001, 2.**-20 * 1.3, 2.**-24, 2.**-25, 3 * 2.**-25, 2.**-26, 2.**14 - 8., 16383.5, 12345.678]
    v = np.array(v)
    return np.concatenate([v, -v])   # (-0.0 among them)


def special_diagonals():
    d = []
    for e in (3, -5, 0, 13):   # sqrt(d) at a power of two exactly, and one ulp either side
        x = 4.**e
        d += [x, np.nextafter(x, 0.), np.nextafter(x, np.inf)]
    d += [1e-130, 1e130, 0., -1., np.nan, np.inf, -np.inf, 1e300, np.nextafter(1e300, 0.), 5e-324, 2.**26, 1e-300]
    return np.array(d)


@functools.lru_cache(maxsize=None)
def conversion_panel(rows, K, first_row):
    """(X, P16, diag, P) read-only.  X (rows x K): the values in scaled units.  diag (first_row + rows) and P16 = X / r, exact,
    for fp16 x 2, so that r x = X.  P = X times a power of two per row for the bf16 and fp32 copies."""
    rng = np.random.default_rng(1000 * rows + 10 * K + first_row)
    X = rng.standard_normal((rows, K)) * 2. ** rng.integers(-12, 12, (rows, K))
    sp = special_values()
    where = rng.permutation(rows * K)[:min(rows * K, 3 * sp.size)]
    X.reshape(-1)[where] = np.roll(sp, rows + K)[np.arange(where.size) % sp.size]
    n = first_row + rows
    diag = 10. ** rng.uniform(-12, 12, n)
    sd = special_diagonals()
    at = rng.permutation(n)[:min(n, sd.size)]
    diag[at] = np.roll(sd, rows)[:at.size]
    rs, _ = row_scales(diag)
    P16 = X / rs[first_row:, None]
    P = X * 2. ** ((np.arange(rows) * 7) % 41 - 20)[:, None]
    assert np.array_equal(P16 * rs[first_row:, None], X) and np.all(np.isfinite(P16))
    ldp = rows + 10
    out = []
    for a in (P16, P):
        b = np.zeros((ldp, K), order="F")
        b[:rows] = a
        out.append(b)
    for a in [X, diag] + out:
        a.setflags(write=False)
    return X, out[0], diag, out[1]


# ---- exactly summable panels -----------------------------------------------------------------------------------------
def lowbit(v):
    """the weight of the lowest set bit of each number (inf for 0)"""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    mi = np.ldexp(np.abs(m), 53).astype(np.int64)
    lb = np.ldexp((mi & -mi).astype(np.float64), e - 53)
    return np.where(mi == 0, np.inf, lb)


def tile_lower(M, N):
    """entries of the lower 128 x 128 TILES: what the kernels update"""
    return (np.arange(M)[:, None] // GT) >= (np.arange(N)[None, :] // GT)


def snan_rows(shape, seed):
    """signalling NaNs with distinct payloads: any arithmetic on one sets its quiet bit, so a write shows"""
    n = int(np.prod(shape))
    bits = np.uint64(0x7ff0000000000000) + (np.arange(n, dtype=np.uint64) + np.uint64(1 + seed))
    return bits.view(np.float64).reshape(shape)


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    part: str            # "B": bit for bit, "C": the bound
    rows: int
    row_offset: int
    M: int
    N: int
    K: int
    first_row: int
    P: np.ndarray        # ldp x K, column-major
    diag: np.ndarray     # first_row + rows
    C0: np.ndarray       # ldc x (N + GUARD_COLS), column-major: ldc = M + 3, padding rows signalling NaNs
    variants: tuple
    free: object = None  # (M x N) bool or None: lower-tile entries NOT compared (beyond an exact check)

    @property
    def ldc(self):
        return self.C0.shape[0]

    @property
    def ldp(self):
        return self.P.shape[0]

    def scales(self):
        rs, irs = row_scales(self.diag)
        return rs[self.first_row:], irs[self.first_row:]

    def checked(self):
        m = tile_lower(self.M, self.N)
        return m & ~self.free if self.free is not None else m


def products_of(case, variant, longdouble=False, r0=0, r1=None):
    """(S, A, g) for the rows r0 .. r1 of C (all M by default): the included partial products of the restated planes summed
    per entry, the sum of their absolute values, and the finest granularity of a partial product of the entry - all in
    scaled units for fp16 x 2"""
    r1 = case.M if r1 is None else r1
    rs, _ = case.scales()
    V = staged_values(variant, case.P, case.rows, case.K, rs)
    o = case.row_offset
    Vi, Vj = V[:, o + r0:o + r1], V[:, o:o + case.N]
    dt = np.longdouble if longdouble else np.float64
    S = np.zeros((r1 - r0, case.N), dt)
    A = np.zeros((r1 - r0, case.N))
    g = np.full((r1 - r0, case.N), np.inf)
    gran = lowbit(V).min(axis=2)   # per plane and row
    used = V.any(axis=(1, 2))
    for pa, pb in variant.pairs:   # pa: of the column's row j, pb: of the row i
        if not (used[pa] and used[pb]):
            continue
        S += Vi[pb].astype(dt) @ Vj[pa].astype(dt).T
        A += np.abs(Vi[pb]) @ np.abs(Vj[pa]).T
        g = np.fmin(g, gran[pb, o + r0:o + r1, None] * gran[pa, None, o:o + case.N])
    return S, A, g


@functools.lru_cache(maxsize=8)
def products_ld(case, variant):
    """products_of in longdouble, kept: the reference and the bound of a part C case are shared by its tests"""
    return products_of(case, variant, longdouble=True)


def pair_scale(case, variant, r0=0, r1=None):
    """1 / (r_i r_j) of the entries of C (fp16 x 2; otherwise 1)"""
    if variant.products != F16X2:
        return 1.
    _, irs = case.scales()
    o = case.row_offset
    return irs[o + r0:o + (case.M if r1 is None else r1), None] * irs[None, o:o + case.N]


def exact_need(case, variant):
    """Bits the fp32 accumulators need on the checked entries: log2 of max sum|partial products| / granularity.  Below 24
    every partial sum in any order is an fp32 number.  Also asserts that the fp64 epilogue is exact."""
    if case.M * case.N > 4_000_000:
        # the bulk case, by a sufficient condition that costs nothing: sum|products| <= sum over the pairs of the largest
        # row 1-norm of one plane times the largest entry of the other, against the finest granularity of any product
        rs, _ = case.scales()
        V = np.abs(staged_values(variant, case.P, case.rows, case.K, rs))
        A = sum(V[pb].sum(axis=1).max() * V[pa].max() for pa, pb in variant.pairs)
        gran = lowbit(V).min(axis=(1, 2))
        g = min(gran[pa] * gran[pb] for pa, pb in variant.pairs if np.isfinite(gran[pa] * gran[pb]))
        irs = case.scales()[1] if variant.products == F16X2 else np.ones(case.rows)
        C = case.C0[:case.M, :case.N]
        assert (np.abs(C).max() + A * irs.max() ** 2) / min(g * irs.min() ** 2, lowbit(C).min()) < 2. ** 52
        return np.log2(A / g)
    chk_all = case.checked()
    need = 0.
    for r0 in range(0, case.M, 1024):   # (block rows: the bulk case is 5761 x 5761)
        r1 = min(case.M, r0 + 1024)
        _, A, g = products_of(case, variant, r0=r0, r1=r1)
        chk = chk_all[r0:r1]
        if not chk.any():
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            need = max(need, np.where(np.isfinite(g) & (A > 0), A / g, 0.)[chk].max())
        sc = pair_scale(case, variant, r0, r1)
        C = case.C0[r0:r1, :case.N]
        fine = np.fmin(np.where(np.isfinite(g), g * sc, np.inf), lowbit(C))
        with np.errstate(invalid="ignore"):
            width = np.where(np.isfinite(fine), (np.abs(C) + A * sc) / fine, 0.)[chk].max()
        assert width < 2. ** 52, (case.name, variant.name, np.log2(width))
    return np.log2(need) if need > 0 else 0.


def expected(case, variant):
    """Part B: what the call must leave in C (ldc x (N + guard)): C - sum(included partial products) / (r_i r_j) on the
    entries of the lower tiles, every other bit as it came."""
    S, _, _ = products_of(case, variant)
    S *= pair_scale(case, variant)   # powers of two: exact
    want = case.C0.copy(order="F")
    low = tile_lower(case.M, case.N)
    want[:case.M, :case.N][low] = (case.C0[:case.M, :case.N] - S)[low]
    return want


def reference_and_bound(case, variant):
    """Part C, per entry of C (M x N): the reference in longdouble and the bound"""
    S, A, _ = products_ld(case, variant)
    sc = pair_scale(case, variant)
    ref = case.C0[:case.M, :case.N] - S * sc
    return ref, variant.roundings(case.K) * 2. ** -23 * A * sc + 2. ** -53 * np.abs(ref).astype(np.float64)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check(case, variant, got, want=None):
    """(ok, text, ratio): the verdict on a buffer that came back.  Outside the lower tiles every bit must be the input's;
    on the checked entries part B asks for equality with `want` (expected() by default) and part C for the bound
    (ratio = worst error / bound)."""
    M, N = case.M, case.N
    low = tile_lower(M, N)
    why = []
    if not same_bits(got[M:], case.C0[M:]):
        why.append("padding rows written")
    if not same_bits(got[:, N:], case.C0[:, N:]):
        why.append("guard columns written")
    if not same_bits(got[:M, :N][~low], case.C0[:M, :N][~low]):
        why.append("strict upper tiles written")
    chk = case.checked()
    g = got[:M, :N][chk]
    ratio = 0.
    if case.part == "B":
        want = expected(case, variant) if want is None else want
        w = want[:M, :N][chk]
        bad = g != w
        if bad.any():
            i, j = np.argwhere(chk)[np.flatnonzero(bad)[0]]
            why.append(f"{int(bad.sum())} of {bad.size} checked entries differ, first C[{i}, {j}] = {got[i, j]!r}, want {want[i, j]!r}")
    else:
        ref, b = reference_and_bound(case, variant)
        err = np.abs(g.astype(np.longdouble) - ref[chk]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(b[chk] > 0, err / b[chk], np.where(err == 0, 0., np.inf))
        ratio = float(np.max(np.where(np.isnan(r), np.inf, r)))
        if not ratio <= 1.:
            why.append(f"worst error / bound = {ratio:.3g}")
    return not why, "; ".join(why), ratio


def _finish(name, part, rows, row_offset, M, N, K, first_row, X, p, m, cg, variants, free=None, seed=0):
    """X (rows x K) in scaled units, p (rows) the exponents of the rows' scales: P = X 2^p, diag = 2^26 4^p (r = 2^-p);
    C = m cg 2^(p_i + p_j) on the tiles with integers m (M x N), signalling NaNs in the padding rows, finite guards."""
    rng = np.random.default_rng(seed + 17)
    ldp, ldc = rows + 10, M + 3
    P = np.zeros((ldp, K), order="F")
    P[:rows] = np.ldexp(X, p[:, None])
    diag = np.concatenate([10. ** rng.uniform(-3, 3, first_row), np.ldexp(2. ** 26, 2 * p)])
    C0 = np.asfortranarray(rng.standard_normal((ldc, N + GUARD_COLS)))
    C0[:M, :N] = np.ldexp(m * cg, p[row_offset:row_offset + M, None] + p[None, row_offset:row_offset + N])
    C0[M:] = snan_rows((ldc - M, N + GUARD_COLS), seed)
    for a in (P, diag, C0):
        a.setflags(write=False)
    case = Case(name, part, rows, row_offset, M, N, K, first_row, P, diag, C0, tuple(variants), free)
    if part == "B":
        for v in variants:
            if v.stages(K):
                need = exact_need(case, v)
                assert need < 24., (name, v.name, need)
    return case


B1_SHAPES = ((129, 0, 129, 129), (128, 0, 128, 128), (127, 0, 127, 127), (385, 0, 385, 128), (700, 128, 572, 572),
             (700, 200, 500, 500), (384, 256, 128, 128), (300, 171, 129, 1))   # (rows, row_offset, M, N)
B1_K = (32, 64, 512)
B1_K_FP32_ONLY = (16, 48)
BULK_VARIANTS = (V_FP32, V_BF16, V_F16)
BULK_M = 5761   # 46 tile rows, 1081 >= 1024 tiles: the tile-order table and its -1 fillers; a ragged last tile row


@functools.lru_cache(maxsize=None)
def b1_case(rows, row_offset, M, N, K, scaled=False, only=None):
    """B1: integers in [-2, 2], all of them in the first plane.  scaled: the rows times powers of two between 2^-30 and
    2^30 with a matching diagonal - the fp16 scales undo them exactly, bf16 x 3 and fp32 take them as they are."""
    seed = rows + 3 * row_offset + 5 * M + 7 * N + 11 * K + scaled
    rng = np.random.default_rng(seed)
    X = rng.integers(-2, 3, (rows, K)).astype(np.float64)
    p = ((np.arange(rows) * 7) % 61 - 30) if scaled else np.zeros(rows, np.int64)
    m = rng.integers(-1000, 1001, (M, N)).astype(np.float64)
    first_row = 37 if (scaled or row_offset in (128, 171)) else 0
    variants = only or (ALL_VARIANTS if K % 32 == 0 else (V_FP32,))
    return _finish(f"B1{'s' if scaled else ''}-{rows}-{row_offset}-{M}-{N}-K{K}", "B", rows, row_offset, M, N, K, first_row, X, p, m, 1.,
                   variants, seed=seed)


@functools.lru_cache(maxsize=1)
def b1_bulk_case():
    return b1_case(BULK_M, 0, BULK_M, BULK_M, 32, only=BULK_VARIANTS)


B2_SHAPE = (257, 0, 257, 257)   # three tile rows, the last one ragged
B2_K = (32, 64, 96)


def _sparse_rows(rng, rows, K, nnz):
    mask = np.zeros((rows, K), bool)
    for i in range(rows):
        mask[i, rng.choice(K, nnz, replace=False)] = True
    return mask


@functools.lru_cache(maxsize=None)
def b2_case(kind, K):
    """B2: panels that occupy the small planes and still add exactly.
      bf16-rich    every row 8 non-zeros s (1 + b 2^-10 + c 2^-19), s = +-1, b in 1..3, c in -1..1: hi = s, mid = s b 2^-10,
                   lo = s c 2^-19 - all three planes occupied, finest product mid*mid = 2^-20, sums <= 8.1: 23.0 bits.
                   (The magnitude must not fall below 1 - b and s of one sign: below 1 bf16 rounds hi to 1 - 2^-8 and lo*hi
                   gets a granularity of 2^-27; and b = 0 would put c 2^-19 into the MID plane, mid*mid = 2^-38.)
      bf16-cross   even rows rich, odd rows integers in [-2, 2]: in an even row x odd column entry only the ROW operand has
                   mid and lo, so hi*lo and lo*hi (hi*mid and mid*hi) are told apart
      f16-cross    even rows 16 non-zeros a + b 2^-12, a in [-4, 4] non-zero, b in [-3, 3]; odd rows integers.  Even x odd
                   and odd x even entries hold h2*h1 or h1*h2 alone next to h1*h1 and add exactly; even x even entries hold
                   h2*h2 = 2^-24 beside h1*h1 of order 2^4 and are left out (free): they belong to part C.
      f16-pair     every row 3 non-zeros s (1 + b 2^-11), s = +-1, b in {1, 3}: h1 = s or s (1 + 2^-9), h2 = +-2^-11 (ties, to
                   even).  An entry is a sum of at most three products x_i x_j = 1 + ... + b b' 2^-22 below 4 in all, so ALL
                   four partial products add exactly (23.6 bits), h2*h2 = 2^-22 among them: the exact witness of the
                   fourth product that rows of 16 non-zeros cannot give."""
    rows, o, M, N = B2_SHAPE
    seed = 100 * K + len(kind)
    rng = np.random.default_rng(seed)
    even = (np.arange(rows) % 2 == 0)[:, None]
    ints = rng.integers(-4, 5, (rows, K)).astype(np.float64)
    free = None
    if kind == "f16-pair":
        nz = _sparse_rows(rng, rows, K, 3)
        X = np.where(nz, rng.choice([-1., 1.], (rows, K)) * (1. + rng.choice([1., 3.], (rows, K)) * 2. ** -11), 0.)
        variants, cg = F16_VARIANTS, 2. ** -10
    elif kind.startswith("bf16"):
        nz = _sparse_rows(rng, rows, K, 8)
        s = rng.choice([-1., 1.], (rows, K))
        rich = s * (1. + rng.integers(1, 4, (rows, K)) * 2. ** -10 + rng.integers(-1, 2, (rows, K)) * 2. ** -19)
        X = np.where(nz, rich if kind == "bf16-rich" else np.where(even, rich, np.clip(ints, -2, 2)), 0.)
        variants, cg = (V_BF16,), 2. ** -10
    else:
        nz = _sparse_rows(rng, rows, K, 16)
        a = rng.integers(1, 5, (rows, K)) * rng.choice([-1., 1.], (rows, K))
        rich = a + rng.integers(-3, 4, (rows, K)) * 2. ** -12
        X = np.where(nz, np.where(even, rich, ints), 0.)
        variants, cg = F16_VARIANTS, 2. ** -6
        par = np.arange(o, o + M) % 2 == 0
        free = par[:, None] & par[None, :N]
    variants = tuple(v for v in variants if v.stages(K))
    m = rng.integers(-4096, 4097, (M, N)).astype(np.float64)
    case = _finish(f"B2-{kind}-K{K}", "B", rows, o, M, N, K, 0, X, np.zeros(rows, np.int64), m, cg, variants, free, seed)
    if kind == "bf16-rich":   # all three planes are occupied and the reconstruction is exact
        V = staged_values(V_BF16, case.P, rows, K, None)
        assert all((V[q] != 0).sum() > K for q in range(3)) and np.array_equal(V.sum(axis=0), X)
    if kind == "f16-cross":
        V = staged_values(V_F16, case.P, rows, K, case.scales()[0])
        assert (V[1][::2] != 0).sum() > K and not V[1][1::2].any() and np.array_equal(V.sum(axis=0), X)
    return case


B3_K = (32, 64)


@functools.lru_cache(maxsize=None)
def b3_case(K):
    """B3: even rows a 2^-10 + b 2^-24 (a in [-4, 4], b in [-3, 3], both non-zero): h1 = a 2^-10 and h2 = b 2^-24, an fp16
    SUBNORMAL; odd rows integers in [-4, 4].  16 non-zeros per row.  Even x odd entries hold h2*h1 (multiples of 2^-24)
    beside h1*h1 (multiples of 2^-10, sums <= 2^-2): 22 bits.  Even x even entries (h2*h2 = 2^-48) are left out."""
    rows, o, M, N = B2_SHAPE
    seed = 7000 + K
    rng = np.random.default_rng(seed)
    even = (np.arange(rows) % 2 == 0)[:, None]
    nz = _sparse_rows(rng, rows, K, 16)
    sgn = lambda: rng.choice([-1., 1.], (rows, K))
    rich = rng.integers(1, 5, (rows, K)) * sgn() * 2. ** -10 + rng.integers(1, 4, (rows, K)) * sgn() * 2. ** -24
    X = np.where(nz, np.where(even, rich, rng.integers(-4, 5, (rows, K)).astype(np.float64)), 0.)
    par = np.arange(o, o + M) % 2 == 0
    m = rng.integers(-4096, 4097, (M, N)).astype(np.float64)
    case = _finish(f"B3-K{K}", "B", rows, o, M, N, K, 0, X, np.zeros(rows, np.int64), m, 2. ** -12,
                   tuple(v for v in F16_VARIANTS if v.stages(K)), par[:, None] & par[None, :N], seed)
    h2 = staged_bits(V_F16, case.P, rows, K, case.scales()[0])[1]
    assert np.all((h2[::2][nz[::2]] & 0x7c00) == 0) and np.all((h2[::2][nz[::2]] & 0x3ff) != 0) and not h2[1::2].any()
    return case


def flushed_expected(case, variant):
    """B3 if the matrix pipe took subnormal inputs as zero: the h2 plane contributes nothing"""
    h1 = staged_values(variant, case.P, case.rows, case.K, case.scales()[0])[0]
    o = case.row_offset
    S = h1[o:o + case.M] @ h1[o:o + case.N].T
    want = case.C0.copy(order="F")
    low = tile_lower(case.M, case.N)
    want[:case.M, :case.N][low] = (case.C0[:case.M, :case.N] - S)[low]
    return want


C_SHAPES = ((385, 128, 257, 257), (828, 128, 700, 700))   # M = 257 and 700 at row_offset 128
C_K = (32, 64)
C_DATA = ("normal", "badly-scaled")
C_VARIANTS = (V_FP32, V_BF16, Variant(F16X2, 4, 32), Variant(F16X2, 3, 32), Variant(F16X2, 4, 64))


@functools.lru_cache(maxsize=None)
def c_case(data, rows, row_offset, M, N, K):
    """Part C: a dense N(0, 1) panel; badly-scaled: the rows times 10^U(-9, 9) and every fourth column 1e-5 of the others
    (tests/test_kernels_gpu.py: test_trailing_update_split_planes_badly_scaled_rows).  The diagonal is the rows' squared
    norms - the bound a Cholesky factor's rows obey - behind first_row = 37 entries of another matrix."""
    seed = rows + 3 * M + 5 * K + len(data)
    rng = np.random.default_rng(seed)
    ldp, ldc, first_row = rows + 10, M + 3, 37
    P = np.zeros((ldp, K), order="F")
    P[:rows] = rng.standard_normal((rows, K))
    rowscale = np.ones(rows)
    if data == "badly-scaled":
        rowscale = 10. ** rng.uniform(-9., 9., rows)
        P[:rows] *= rowscale[:, None]
        P[:, ::4] *= 1e-5
    diag = np.concatenate([10. ** rng.uniform(-3, 3, first_row), (P[:rows] ** 2).sum(axis=1)])
    C0 = np.asfortranarray(rng.standard_normal((ldc, N + GUARD_COLS)))
    rsc = rowscale[row_offset:row_offset + M]
    C0[:M, :N] *= np.outer(rsc, rsc[:N])
    C0[M:] = snan_rows((ldc - M, N + GUARD_COLS), seed)
    for a in (P, diag, C0):
        a.setflags(write=False)
    return Case(f"C-{data}-M{M}-K{K}", "C", rows, row_offset, M, N, K, first_row, P, diag, C0,
                tuple(v for v in C_VARIANTS if v.stages(K)))


def distance_allowed(case, variant):
    """How far the included terms may lie from P P^T by the statements of the kernel file's header, per entry (M x N).
    Every factor carries the error of its split - bf16 x 3: 2^-25 |x|; fp16 x 2: 2^-22 |x|, and 2^-25 in scaled units where
    |r x| < 2^-2; fp32: 2^-24 |x| - and the products left out are bounded by the planes' sizes: |mid| <= 2^-8 |x|,
    |lo| <= 2^-16 |x|, |h2| <= 2^-11 |x| (and 2^-25 + 2^-11 |x| at most below 2^-2)."""
    rs, irs = case.scales()
    o = case.row_offset
    X = np.abs(case.P[:case.rows, :case.K])
    if variant.products == F16X2:
        X = X * rs[:, None]
    if variant.products == FP32:
        E, drop = 2. ** -24 * X, 0.
    elif variant.products == BF16X3:
        E = 2. ** -25 * X
        mid, lo = 2. ** -8 * X, 2. ** -16 * X
        drop = mid[o:o + case.M] @ lo[o:o + case.N].T + lo[o:o + case.M] @ mid[o:o + case.N].T + lo[o:o + case.M] @ lo[o:o + case.N].T
    else:
        E = np.where(X >= 2. ** -2, 2. ** -22 * X, 2. ** -25)
        h2 = 2. ** -11 * X + 2. ** -25
        drop = h2[o:o + case.M] @ h2[o:o + case.N].T if variant.terms == 3 else 0.
    Xi, Xj, Ei, Ej = X[o:o + case.M], X[o:o + case.N], E[o:o + case.M], E[o:o + case.N]
    d = Ei @ Xj.T + Xi @ Ej.T + Ei @ Ej.T + drop
    if variant.products == F16X2:
        d = d * (irs[o:o + case.M, None] * irs[None, o:o + case.N])
    return d * (1 + 2. ** -40)   # (the fp64 evaluation of this very bound)


# ---- the kernels emulated tile by tile from the plane image, with faults --------------------------------------------------
FAULTS = ("swap_planes", "third_stride", "chunk_off", "rowab", "scales_first0", "scales_first0_convert", "irs_row_for_col",
          "ragged_past_M", "tile_twice")


def lower_tiles(M, N):
    ntr, ntc = (M + GT - 1) // GT, min((N + GT - 1) // GT, (M + GT - 1) // GT)
    return [(bi, bj) for bj in range(ntc) for bi in range(bj, ntr)]


def emulate(case, variant, fault=None, arith="exact"):
    """What the staged update leaves in C, by the kernels' own addressing of the plane image: per tile, per K chunk, per
    matrix instruction.  arith 'exact': fp64 sums (exact on part B panels); 'fp32': every product added to an fp32
    accumulator one after the other, k ascending inside an instruction.  fault: one of FAULTS, ('drop', pair) or
    ('double', pair) - what a subtly wrong kernel would do."""
    rows, K, o, M, N = case.rows, case.K, case.row_offset, case.M, case.N
    ch, rp = variant.ch, rows_pad(case.rows)
    rs_all, irs_all = row_scales(case.diag)
    first_c = 0 if fault in ("scales_first0", "scales_first0_convert") else case.first_row
    first_e = 0 if fault == "scales_first0" else case.first_row
    irs = irs_all[first_e:first_e + rows]
    if variant.products == FP32:
        vals = np.zeros((1, 1, rp, K))
        vals[0, 0, :rows] = staged_values(variant, case.P, rows, K, None)[0]
        vals = vals.reshape(-1)
        ch, nk = K, 1
    else:
        bits = staged_bits(variant, case.P, rows, K, rs_all[first_c:first_c + rows])
        img = plane_image(bits, K, ch)
        with np.errstate(invalid="ignore"):
            vals = bf16_val(img) if variant.products == BF16X3 else img.view(np.float16).astype(np.float64)
        nk = K // ch
    plane_stride = rp * K

    def fetch(plane, row0, c):
        if fault == "swap_planes" and plane < 2:
            plane = 1 - plane
        stride = plane_stride if (fault == "third_stride" and plane == 2) else plane * plane_stride
        if fault == "chunk_off":
            c = min(c + 1, nk - 1)
        off = stride + c * rp * ch + row0 * ch
        return vals[off:off + GT * ch].reshape(GT, ch)

    pairs = list(variant.pairs)
    if isinstance(fault, tuple):
        pairs = [q for q in pairs if q != fault[1]] if fault[0] == "drop" else pairs + [fault[1]]
    tiles = lower_tiles(M, N)
    if fault == "tile_twice":
        tiles = tiles + [tiles[len(tiles) // 2]]
    got = case.C0.copy(order="F")
    flat = got.reshape(-1, order="F")   # (a view: got is column-major)
    assert np.shares_memory(flat, got)
    for bi, bj in tiles:
        i0, j0 = bi * GT, bj * GT
        ri, rj = (j0, i0) if fault == "rowab" else (i0, j0)
        acc = np.zeros((GT, GT), np.float32 if arith == "fp32" else np.float64)
        for c in range(nk):
            for pa, pb in pairs:
                Bi, Aj = fetch(pb, o + ri, c), fetch(pa, o + rj, c)
                if arith == "fp32":
                    for k in range(ch):
                        acc += (Bi[:, k, None] * Aj[None, :, k]).astype(np.float32)
                else:
                    with np.errstate(invalid="ignore"):
                        acc += Bi @ Aj.T
        upd = acc.astype(np.float64)
        ii, jj = np.arange(i0, i0 + GT), np.arange(j0, j0 + GT)
        if variant.products == F16X2:
            ir_i = np.where(ii < M, irs[np.minimum(o + ii, rows - 1)], 0.)
            ir_j = irs[np.minimum(o + (ii if fault == "irs_row_for_col" else jj), rows - 1)]
            upd = upd * (ir_i[:, None] * (ir_j[:, None] if fault == "irs_row_for_col" else ir_j[None, :]))
        row_ok = ii < (i0 + GT if fault == "ragged_past_M" else M)
        idx = ii[:, None] + jj[None, :] * case.ldc
        ok = row_ok[:, None] & (jj < N)[None, :] & (idx < flat.size)
        with np.errstate(invalid="ignore"):
            flat[idx[ok]] = flat[idx[ok]] - upd[ok]
    return got


def named_gpu_cases(variant, with_bulk=False):
    """every (part B, part C) case the GPU module runs with this variant"""
    b = [b1_case(*shape, K) for K in B1_K + B1_K_FP32_ONLY for shape in B1_SHAPES]
    b += [b1_case(129, 0, 129, 129, 64, True), b1_case(700, 128, 572, 572, 64, True)]
    b += [b2_case(kind, K) for kind in ("bf16-rich", "bf16-cross", "f16-cross", "f16-pair") for K in B2_K] + [b3_case(K) for K in B3_K]
    if with_bulk:
        b.append(b1_bulk_case())
    c = [c_case(data, *shape, K) for data in C_DATA for shape in C_SHAPES for K in C_K]
    keep = lambda cases: [x for x in cases if variant in x.variants and variant.stages(x.K)]
    return keep(b), keep(c)
