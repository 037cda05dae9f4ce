"""The ring tile of the fp64 bulk update (csrc/gemm_tiles.h: gemm_nt_sub_tile_ring - both panels loaded global -> LDS
directly into a ring of stages, counted waits, raw barriers) against the register-staged tile it replaces in the whole
interior tiles (gemm_nt_sub_tile_cpf), through the two launch variants that exist for this comparison
(csrc/gemm.hip, launch_trailing_update_planned): 30 = every tile a whole 128 x 128 workgroup on the ring loop where the
tile is eligible, 31 = the same launch on the register-staged loop.  The shapes are small - three or four tile rows -
which the product launch would hand to 64 x 64 quadrants.

Both loops run the same MFMAs in the same order over k and take the eight parts of C in at the same k; the ring keeps
the negative of the other's accumulators (nothing is negated while staging), which rounds the same way.  So the two
must agree exactly; `same` compares values (an entry that comes out exactly zero may differ in the sign of the zero,
and NaN - the padding rows - equals NaN)."""
import ctypes as C
import functools

import numpy as np
import pytest

from albatross_amd import _capi as capi

pytestmark = pytest.mark.gpu

RING, STAGED = 30, 31

# (M, K, ldp - M)
#   M = 384: three tile rows, diagonal and off-diagonal whole tiles.  K = 128: eight chunks of 16, the shallowest
#   eligible product; 144, 272: a last part of C longer than the others and an odd chunk count against the ring length;
#   512: the depth of the fit.  M = 400: the last tile row and column are ragged and stay on the guarded body beside
#   ring tiles.  K = 136: not a multiple of 16, nothing is eligible.  ldp = M + 9: odd, the panel's columns are not
#   16-byte aligned, nothing is eligible.
CASES = [(384, 128, 10), (384, 144, 10), (384, 272, 10), (384, 512, 10), (400, 256, 10), (384, 136, 10), (384, 256, 9)]


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def dbg(ctx):
    lib = capi.load_debug()
    lib.agp_debug_trailing_update.restype = C.c_int
    lib.agp_debug_trailing_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int]
    return lib


@functools.lru_cache(maxsize=None)
def problem(M, K, pad_p):
    """C (ldc x M) and P (ldp x K), random as in test_trailing_update_variants, NaN in the padding rows of both."""
    rng = np.random.default_rng(1000 * M + K + pad_p)
    ldc, ldp = M + 8, M + pad_p
    Cm = np.asfortranarray(rng.standard_normal((ldc, M)))
    P = np.asfortranarray(rng.standard_normal((ldp, K)))
    Cm[M:] = np.nan
    P[M:] = np.nan
    Cm.setflags(write=False)
    P.setflags(write=False)
    return Cm, P


_results = {}


def updated(ctx, dbg, M, K, pad_p, variant):
    """The whole buffer after the update by `variant`; computed once per case and variant."""
    key = (M, K, pad_p, variant)
    if key not in _results:
        Cm, P = problem(M, K, pad_p)
        got = Cm.copy(order="F")
        assert dbg.agp_debug_trailing_update(ctx._h, _p(got), got.shape[0], _p(P), P.shape[0], M, K, variant) == 0
        got.setflags(write=False)
        _results[key] = got
    return _results[key]


@pytest.mark.parametrize("M,K,pad_p", CASES)
def test_ring_equals_register_staged(ctx, dbg, M, K, pad_p):
    """Variant 30 and variant 31 return the same buffer: every tile, the padding rows, and the strict upper triangle
    outside the diagonal tiles, which neither may touch."""
    ring = updated(ctx, dbg, M, K, pad_p, RING)
    staged = updated(ctx, dbg, M, K, pad_p, STAGED)
    assert same(ring, staged)
    Cm, _ = problem(M, K, pad_p)
    nt = (M + 127) // 128
    for bj in range(1, nt):  # tiles strictly above the diagonal: as they came in
        assert np.array_equal(_bits(ring[:128 * bj, 128 * bj:128 * (bj + 1)]), _bits(Cm[:128 * bj, 128 * bj:128 * (bj + 1)]))


@pytest.mark.parametrize("M,K,pad_p", CASES)
def test_ring_against_numpy(ctx, dbg, M, K, pad_p):
    """Variant 30 against the numpy product on the lower triangle, the bar and the scale of test_trailing_update_variants;
    the padding rows come back bit for bit."""
    Cm, P = problem(M, K, pad_p)
    got = updated(ctx, dbg, M, K, pad_p, RING)
    want = Cm[:M] - P[:M] @ P[:M].T
    low = np.tril_indices(M)
    scale = np.abs(P[:M]).sum(axis=1).max() ** 2
    err = np.abs(got[:M][low] - want[low]).max()
    print(f"M={M} K={K} ldp=M+{pad_p}: max error {err:.3e}, bar {1e-14 * scale:.3e}")
    assert err <= 1e-14 * scale
    assert np.array_equal(_bits(got[M:]), _bits(Cm[M:]))


def test_merged_head_publishes_ring_tiles(ctx, dbg):
    """The merged update with a head of four tile columns (variant 20 + 4) at M = 1418, K = 512: the head's counted
    128 x 128 tiles run the product kernel's loop; the debug entry point checks their count and the gate.  On the tiles
    that are whole workgroup tiles in both launches - tile columns 0 .. 3, the eleven whole tile rows - the result equals
    variant 31's."""
    M, K, head = 1418, 512, 4
    merged = updated(ctx, dbg, M, K, 10, 20 + head)
    staged = updated(ctx, dbg, M, K, 10, STAGED)
    whole = M // 128
    for bj in range(head):
        for bi in range(bj, whole):
            r, c = slice(128 * bi, 128 * (bi + 1)), slice(128 * bj, 128 * (bj + 1))
            assert same(merged[r, c], staged[r, c]), (bi, bj)
    Cm, _ = problem(M, K, 10)
    assert np.array_equal(_bits(merged[M:]), _bits(Cm[M:]))
