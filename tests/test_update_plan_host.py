"""The tiling of the MFMA update launches, checked without a GPU: csrc/update_plan.h decides the tile edge of every product,
the cut of a bulk update into whole tiles and quadrants, the grid, the order table of the whole tiles and the decode from
a workgroup number to its tile from plain integers, and agp_debug_update_plan (csrc/debug_api.hip) shows those decisions
with no context and no device.  Here they are compared with the independent restatement in tests/update_plan_cases.py at
every size up to 160 tile rows (M = 20480) and checked for the structure every plan must have.  The kernel tests
(test_kernels_gpu.py, test_bulk_ring_tiles_gpu.py, test_split_plane_kernels_gpu.py) prove on the device that the launches
compute what the plans say."""
import functools
import hashlib

import numpy as np
import pytest

import update_plan_cases as uc
from update_plan_cases import QUADRANTS_ONLY, WHOLE_AND_QUADRANTS, XCDS

NTR_MAX = 160
SLOTS = (512, 208, 64)  # 2 per CU: an MI355X, a partition of 104 CUs, a small CU mask
HEAD_COLS = (0, 1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def bulk_plans(slots):
    """{(nth, head_cols): plan of the library}, each already equal to the restatement."""
    plans = {}
    for nth in range(1, NTR_MAX + 1):
        for h in HEAD_COLS:
            plans[nth, h] = uc.planned_bulk(nth, h, slots)
            assert plans[nth, h] == uc.bulk_plan(nth, h, slots), (nth, h, slots)
    return plans


@pytest.mark.parametrize("slots", SLOTS)
def test_bulk_plan_equals_restatement(slots):
    bulk_plans(slots)


def nt_sub_edge_shapes():
    """(M, N, K, tri, count) on both sides of every rule of plan_nt_sub at small_limit = 512."""
    shapes = []
    for count in (1, 7):
        # 128-tiles * count = 511 / 512 (count 1: 7 x 73 and 8 x 64 tiles; count 7: 73 and 74 tiles per problem)
        shapes += [(7 * 128, 73 * 128, 256, False, 1), (8 * 128, 64 * 128, 256, False, 1)] if count == 1 else \
                  [(128, 73 * 128, 256, False, 7), (128, 74 * 128 - 5, 256, False, 7)]
        # lower tiles: 31 rows = 496 tiles, 32 rows = 528 (count 1); 11 rows = 66 tiles (462), 12 rows = 78 (546) (count 7)
        shapes += [(31 * 128, 31 * 128, 300, True, 1), (32 * 128 - 3, 32 * 128 - 3, 300, True, 1)] if count == 1 else \
                  [(11 * 128, 11 * 128, 300, True, 7), (12 * 128, 12 * 128, 300, True, 7)]
        # 64-tiles * count = 255 / 256, K = 255 / 256 on each side of them
        for K in (255, 256):
            shapes += [(15 * 64, 17 * 64, K, False, 1), (16 * 64, 16 * 64, K, False, 1)] if count == 1 else \
                      [(4 * 64, 9 * 64, K, False, 7), (64, 37 * 64 - 1, K, False, 7)]
            # ... and of a lower grid: 22 tile rows of 64 = 253, 23 = 276 (count 1); 8 = 36 (252), 9 = 45 (315) (count 7)
            shapes += [(22 * 64, 22 * 64, K, True, 1), (23 * 64 - 1, 23 * 64 - 1, K, True, 1)] if count == 1 else \
                      [(8 * 64, 8 * 64, K, True, 7), (9 * 64, 9 * 64, K, True, 7)]
    # wider than tall with tri (the tile columns stop at the diagonal), ragged and tiny
    shapes += [(300, 1000, 512, True, 1), (300, 1000, 512, True, 7), (1, 1, 1, False, 1), (33, 65, 256, False, 1), (129, 129, 256, True, 7)]
    return shapes


def test_nt_sub_plan_equals_restatement():
    # the shapes do sit on the edges: 511 / 512 large tiles and 255 / 256 small ones in all (seven problems cannot make
    # 512, 255 or 256, and lower grids only triangular numbers: the nearest on either side)
    def total(M, N, tri, count, edge):
        ntr, ntc = uc.ceil_div(M, edge), uc.ceil_div(N, edge)
        return count * len(uc.tiles_in_order(ntr, min(ntc, ntr) if tri else ntc, tri))
    large = {total(M, N, tri, count, 128) for M, N, _, tri, count in nt_sub_edge_shapes()}
    small = {total(M, N, tri, count, 64) for M, N, _, tri, count in nt_sub_edge_shapes()}
    assert {511, 512, 496, 528, 518, 462, 546} <= large and {255, 256, 253, 276, 252, 259, 315} <= small
    seen = set()
    for M, N, K, tri, count in nt_sub_edge_shapes():
        for a_kmajor in (False, True):
            for b_kmajor in (False, True):
                want = uc.nt_sub_plan(M, N, K, tri, a_kmajor, b_kmajor, count)
                got = uc.planned_nt_sub(M, N, K, tri, a_kmajor, b_kmajor, count)
                assert got == want, (M, N, K, tri, a_kmajor, b_kmajor, count)
                assert got["grid"] == len(uc.tiles_in_order(got["ntr"], got["ntc"], tri and not got["transposed"]))
                seen.add((got["edge"], got["transposed"]))
    assert seen == {(128, 0), (64, 0), (64, 1), (32, 0)}
    # the limit is the caller's: nothing is small at 0, a 128-tile launch of 600 tiles is at 601
    assert uc.planned_nt_sub(64, 64, 512, False, False, False, 1, small_limit=0)["edge"] == 128
    assert uc.planned_nt_sub(128 * 20, 128 * 30, 512, False, False, False, 1, small_limit=601)["edge"] == 64


@pytest.mark.parametrize("slots", SLOTS)
def test_stair_plan_equals_restatement(slots):
    block = 1536  # 12 tile rows of 128 per row block
    sides = set()
    for blocks, cols in ((1, 1), (2, 5), (4, 16), (6, 40), (8, 80), (16, 160), (24, 240)):
        M, N = blocks * block, cols * 128
        for c0 in (0, 384, 128 * 57):
            want = uc.stair_plan(M, N, block, c0, slots)
            assert uc.planned_stair(M, N, block, c0, slots) == want, (M, N, c0, slots)
            sides.add(want["edge"])
    # exactly at the switch: 4 * slots rounds of owned (half of all) large tiles
    rows = 16
    cols = 8 * slots // rows
    assert uc.planned_stair(rows * 128, cols * 128, 128, 0, slots)["edge"] == 128
    assert uc.planned_stair(rows * 128, (cols - 1) * 128 + 1, 128, 0, slots)["edge"] == 128  # (a ragged last tile column counts)
    assert uc.planned_stair(rows * 128, (cols - 1) * 128, 128, 0, slots)["edge"] == 64
    assert sides == {64, 128}


@pytest.mark.parametrize("slots", SLOTS)
def test_bulk_plan_structure(slots):
    plans = bulk_plans(slots)
    for (nth, h), p in plans.items():
        ntr, tiles, full, rem = p["ntr"], p["tiles"], p["full"], p["rem"]
        assert ntr == nth - min(h, nth) and tiles == len(uc.tiles_in_order(ntr, ntr, True))
        # every tile of the sub-triangle exactly once: [0, full) whole, [full, tiles) as quadrants
        assert 0 <= full and 0 <= rem and full + rem == tiles
        assert full % slots == 0 or full == tiles
        assert rem < slots or full == 0
        assert p["order_len"] == (XCDS * uc.ceil_div(full, XCDS) if full else 0)
        assert p["grid"] == p["head_count"] + p["order_len"] + 4 * rem
        assert p["kernel"] == (QUADRANTS_ONLY if full == 0 and h == 0 else WHOLE_AND_QUADRANTS)
        # the head: the first head_cols tile columns of the whole trailing matrix, column by column
        assert p["head_count"] == len(uc.tiles_in_order(nth, min(h, nth), True))
        if h:
            # merged and plain launch of the same triangle differ in the all-quadrants kernel and the head only
            plain = plans[ntr, 0] if ntr else None
            if plain:
                same = ("ntr", "tiles", "full", "rem", "order_len")
                assert {k: p[k] for k in same} == {k: plain[k] for k in same}
                assert plain["kernel"] == p["kernel"] or (full == 0 and plain["kernel"] == QUADRANTS_ONLY)
                assert p["grid"] - p["head_count"] == plain["grid"]
    # every branch is met at this slot count
    assert {p["kernel"] for p in plans.values()} == {QUADRANTS_ONLY, WHOLE_AND_QUADRANTS}
    assert any(p["full"] and p["rem"] for p in plans.values()) and any(p["full"] == p["tiles"] > 0 and p["tiles"] % slots for p in plans.values())


@pytest.mark.parametrize("slots", SLOTS)
def test_bulk_plan_head_and_quadrant_workgroups(slots):
    """The workgroups of every planned launch, laid out as trailing_update_kernel reads its grid - head, quadrants, whole
    tiles through the table - cover the lower triangle of the whole trailing matrix exactly once: counted in quadrants, four
    for every tile, three for a diagonal tile that runs as quadrants.  The head's tiles come first, column by column."""
    for (nth, h), p in bulk_plans(slots).items():
        h = min(h, nth)
        covered = np.zeros((nth, nth), np.int64)
        if p["head_count"]:
            head = uc.planned_tiles(0, p["head_count"], nth, h, True)
            assert head[:, 0].all() and np.array_equal(head[:, 1:], np.array(uc.tiles_in_order(nth, h, True), np.int64)), (nth, h)
            np.add.at(covered, (head[:, 1], head[:, 2]), 4)
        expected = 4 * np.tril(np.ones((nth, nth), np.int64))
        if p["rem"]:
            quads = uc.planned_tiles(p["full"], p["rem"], p["ntr"], p["ntr"], True)
            assert quads[:, 0].all(), (nth, h)
            bi, bj = quads[:, 1] + h, quads[:, 2] + h
            parts = [sum(1 for q in range(4) if not (i == j and (q >> 1) > (q & 1))) for i, j in zip(bi.tolist(), bj.tolist())]
            np.add.at(covered, (bi, bj), parts)
            expected[bi[bi == bj], bj[bi == bj]] = 3  # nothing of a diagonal tile's upper quadrant is in the lower triangle
        if p["full"]:
            table = uc.planned_order(p["ntr"], p["full"])
            assert table.size == p["order_len"]
            tiles = table[table >= 0]
            np.add.at(covered, ((tiles >> 16) + h, (tiles & 0xffff) + h), 4)
        assert np.array_equal(covered, expected), (nth, h, slots)


@pytest.mark.parametrize("tri", [True, False])
def test_lower_tile_of_is_a_bijection(tri):
    for ntr in range(1, NTR_MAX + 1):
        for ntc in sorted({1, (ntr + 1) // 2, max(ntr - 1, 1), ntr}):
            want = uc.tiles_in_order(ntr, ntc, tri)
            got = uc.planned_tiles(0, len(want) + 3, ntr, ntc, tri)
            assert got[:len(want), 0].all() and not got[len(want):, 0].any(), (ntr, ntc)
            assert np.array_equal(got[:len(want), 1:], np.array(want, np.int64).reshape(-1, 2)), (ntr, ntc)
            assert (got[len(want):, 1:] == -1).all()
    # far beyond the grid, and a window in the middle of a large one
    assert not uc.planned_tiles(1 << 40, 2, 160, 160, tri)[:, 0].any()
    want = uc.tiles_in_order(160, 160, tri)
    assert [tuple(r) for r in uc.planned_tiles(9000, 50, 160, 160, tri)[:, 1:].tolist()] == want[9000:9050]


def test_order_table_structure():
    shapes = sorted({(p["ntr"], p["full"]) for slots in SLOTS for p in bulk_plans(slots).values() if p["full"]})
    shapes += [(46, 1081), (124, 7750), (1, 1), (9, 45), (160, 1)]
    assert len(shapes) > 300  # (not vacuous)
    for ntr, full in shapes:
        table = uc.planned_order(ntr, full)
        assert table.size == XCDS * uc.ceil_div(full, XCDS), (ntr, full)
        assert (table[:-XCDS] >= 0).all(), (ntr, full)  # -1 only in the last row of eight
        tiles = table[table >= 0]
        bi, bj = tiles >> 16, tiles & 0xffff
        assert ((bj <= bi) & (bi < ntr)).all()
        index = bj * ntr - bj * (bj - 1) // 2 + (bi - bj)  # number of the tile in the column-major lower order
        assert np.array_equal(np.sort(index), np.arange(full)), (ntr, full)
        per_xcd = (table.reshape(-1, XCDS) >= 0).sum(axis=0)
        assert per_xcd.max() - per_xcd.min() <= 1, (ntr, full)


# sha256 of the table as little-endian int32.  Made ONCE from the commit before csrc/update_plan.h existed: the lines of
# gemm.hip's xcd_order that built the table, compiled as they stood into a scratch program that wrote the two tables
# out.  A change of these digests is a change of the tile-to-workgroup assignment of every large bulk update.
ORDER_DIGESTS = {
    (46, 1081): "28e31bfa565c9ac7cb7011081af5896a8235918870ca4f943f6eebeb8601f376",    # M = 5761 (split_plane_cases.BULK_M)
    (124, 7750): "f1a24e2febefa359db9c3e14772e6219ab6d25a12bbe8360232ebf2e4665a937",  # M = 15872, every tile whole
}


@pytest.mark.parametrize("shape", sorted(ORDER_DIGESTS))
def test_order_table_did_not_move(shape):
    table = uc.planned_order(*shape)
    assert hashlib.sha256(table.astype("<i4").tobytes()).hexdigest() == ORDER_DIGESTS[shape]


def test_update_plan_rejects_bad_requests():
    fn = uc.capi.load_debug().agp_debug_update_plan
    import ctypes as C
    n = C.c_int64(0)
    out = np.zeros(8, np.int64)
    for words in ([5, 1, 1], [0, 4, 0], [0, 0, 0, 512], [0, 4, 0, 0], [1, 128, 128, 0, 0, 0, 0, 1, 512], [3, 0, 1, 0, 1, 1], [-1]):
        w = np.array(words, np.int64)
        assert fn(C.c_void_p(w.ctypes.data), w.size, C.c_void_p(out.ctypes.data), out.size, C.byref(n)) != 0, words
