"""The tiling of the MFMA update launches restated in Python, independently of csrc/update_plan.h: which tile edge a
product C -= A B^T gets, how a bulk trailing update is cut into whole 128 x 128 tiles and 64 x 64 quadrants, how its grid
is laid out and in which order tiles are numbered.  tests/test_update_plan_host.py compares the plans of
agp_debug_update_plan (csrc/debug_api.hip) with these at every size, without a device.

The restatements follow what the launches have to achieve (csrc/gemm.hip: launch_trailing_update_as,
launch_trailing_update_merged, launch_gemm_nt_sub_batched, launch_gemm_nt_sub_stair), in Python's own terms and NOT
transcribed from the plan header; they are the reference, so a change of a rule changes BOTH sides on purpose.
"""
import ctypes as C

import numpy as np

from albatross_amd import _capi as capi

WHOLE_AND_QUADRANTS, QUADRANTS_ONLY = 0, 1  # trailing_update_kernel / trailing_update_tail_kernel
XCDS = 8                                    # workgroup i of a launch runs on XCD i % 8


def ceil_div(a, b):
    return -(-a // b)


def tiles_in_order(ntr, ntc, tri):
    """The tiles (bi, bj) of an ntr x ntc tile grid in launch order: column by column, top to bottom; tri: only the
    tiles on or below the diagonal."""
    return [(bi, bj) for bj in range(ntc) for bi in range(bj if tri else 0, ntr)]


def bulk_plan(nth, head_cols, slots):
    """The bulk update of a trailing matrix of nth tile rows on a device with `slots` workgroup slots for large tiles.
    head_cols > 0: the merged launch, whose first workgroups are the tiles of the first head_cols tile columns; the
    rest of the plan describes the triangle right of them.

    Whole rounds of large tiles run at full occupancy; what is left over would hold a fraction of the chip for a whole
    round, so it runs as quadrants, four workgroups a tile, IN FRONT of the whole tiles.  Below two rounds everything
    runs as quadrants; a remainder of three quarters of a round or more is not worth cutting up."""
    head_cols = min(head_cols, nth)
    ntr = nth - head_cols
    tiles = ntr * (ntr + 1) // 2
    rounds, left = divmod(tiles, slots)
    if rounds < 2:
        whole, quads = 0, tiles
    elif 4 * left >= 3 * slots:
        whole, quads = tiles, 0
    else:
        whole, quads = rounds * slots, left
    # a launch of quadrants alone has a kernel of its own (twice the workgroups per CU) - unless a head has to run too
    kernel = QUADRANTS_ONLY if whole == 0 and head_cols == 0 else WHOLE_AND_QUADRANTS
    head_count = sum(nth - c for c in range(head_cols))
    # the whole tiles are handed out through a table of one row per eight workgroups (one per XCD)
    order_len = XCDS * ceil_div(whole, XCDS)
    return {"ntr": ntr, "tiles": tiles, "full": whole, "rem": quads, "kernel": kernel, "head_count": head_count,
            "order_len": order_len, "grid": head_count + order_len + 4 * quads}


def nt_sub_plan(M, N, K, tri, a_kmajor, b_kmajor, count, small_limit=512):
    """C (M x N) -= A B^T for `count` problems: 128 x 128 tiles when they fill the chip; otherwise 64 x 64 tiles - for a
    transposed second operand (and a full grid) the kernel with the transposed loaders, for two plain operands the plain
    one, and 32 x 32 tiles when even those are fewer than the CUs and the product is deep; every other layout has only
    the 128-tile kernel."""
    def cut(edge, lower):
        ntr, ntc = ceil_div(M, edge), ceil_div(N, edge)
        if lower:
            ntc = min(ntc, ntr)
        return ntr, ntc, len(tiles_in_order(ntr, ntc, lower))

    def plan(edge, lower, transposed=False):
        ntr, ntc, grid = cut(edge, lower)
        return {"edge": edge, "transposed": int(transposed), "ntr": ntr, "ntc": ntc, "grid": grid}

    if cut(128, tri)[2] * count >= small_limit:
        return plan(128, tri)
    if b_kmajor and not tri:
        return plan(64, False, transposed=True)
    if not a_kmajor and not b_kmajor:
        if cut(64, tri)[2] * count < 256 and K >= 256:
            return plan(32, tri)
        return plan(64, tri)
    return plan(128, tri)


def stair_plan(M, N, block, c0, slots):
    """A staircase product of the sharded fit (about half of the M x N tile grid is owned): 64 x 64 tiles below four
    rounds of large ones; the rows per row block and the first column in units of the tile edge."""
    large = ceil_div(M, 128) * ceil_div(N, 128)
    edge = 64 if large // 2 < 4 * slots else 128
    return {"edge": edge, "ntr": ceil_div(M, edge), "ntc": ceil_div(N, edge), "st_tpb": block // edge, "st_c0t": c0 // edge}


# ---- the plans of the library, without a device (csrc/debug_api.hip: agp_debug_update_plan) ---------------------------
def _ask(words, cap):
    fn = capi.load_debug().agp_debug_update_plan
    w = np.array(words, np.int64)
    out = np.zeros(max(cap, 1), np.int64)
    n = C.c_int64(0)
    assert fn(C.c_void_p(w.ctypes.data), w.size, C.c_void_p(out.ctypes.data), cap, C.byref(n)) == 0, words
    assert n.value <= cap, (words, n.value, cap)
    return out[:n.value]


BULK_FIELDS = ("ntr", "tiles", "full", "rem", "kernel", "head_count", "order_len", "grid")
NT_SUB_FIELDS = ("edge", "transposed", "ntr", "ntc", "grid")
STAIR_FIELDS = ("edge", "ntr", "ntc", "st_tpb", "st_c0t")


def planned_bulk(nth, head_cols, slots):
    return dict(zip(BULK_FIELDS, _ask([0, nth, head_cols, slots], 8).tolist()))


def planned_nt_sub(M, N, K, tri, a_kmajor, b_kmajor, count, small_limit=512):
    return dict(zip(NT_SUB_FIELDS, _ask([1, M, N, K, int(tri), int(a_kmajor), int(b_kmajor), count, small_limit], 5).tolist()))


def planned_stair(M, N, block, c0, slots):
    return dict(zip(STAIR_FIELDS, _ask([2, M, N, block, c0, slots], 5).tolist()))


def planned_tiles(first, count, ntr, ntc, tri):
    """lower_tile_of for the ids first .. first + count - 1: rows of (found, bi, bj)."""
    return _ask([3, first, count, ntr, ntc, int(tri)], 3 * count).reshape(count, 3)


def planned_order(ntr, full):
    """xcd_tile_order(ntr, full): the table, entry = bi << 16 | bj or -1."""
    return _ask([4, ntr, full], XCDS * (ceil_div(full, XCDS) + 1))
