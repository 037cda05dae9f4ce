// update_plan.h — how every MFMA update launch (C -= A B^T: gemm.hip, gemm_split_planes.hip) is tiled, as plain C++
// (no HIP; g++ -std=c++17 compiles it): which tile edge a product gets, how a bulk update is cut into whole tiles and
// quadrants, in which order the whole tiles are handed out, how large the grid is - and the ONE decode from a workgroup
// number to its tile, which the kernels of gemm.hip call too (AGP_HD).  Integer arithmetic only.  gemm.hip carries the plans out;
// agp_debug_update_plan (debug_api.hip) shows them to tests/test_update_plan_host.py without a device.  Every switch
// point of these launches lives HERE, with the measurement that set it.
#pragma once
#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define AGP_HD __host__ __device__ __attribute__((always_inline))
#else
#define AGP_HD
#endif

namespace agp {

// (gemm.hip asserts that these equal the tile edges GT, ST and TT of gemm_tiles.h)
constexpr int PLAN_GT = 128, PLAN_ST = 64, PLAN_TT = 32;

// Which kernel a bulk trailing update runs on (launch_trailing_update_as).  The debug entries take integers
// (debug_api.hip: bulk_kernel_of is the one place that maps them).
enum class BulkKernel {
  Fp64,                     // the product launch: plan_bulk_update below
  Fp32Products,             // trailing_update_f32_kernel (mixed precision), every tile whole
  Fp64WholeRing,            // the fp64 kernel with whole tiles only, however few: on the ring loop ...
  Fp64WholeRegisterStaged,  // ... on the register-staged loop (the same-build comparison of the two)
};

// ---- tile order arithmetic ------------------------------------------------------------------------------------------
// The tiles of C are numbered column by column, top to bottom; tri: only those on or below the diagonal (column bj
// holds the rows bi >= bj), of the first ntc <= ntr tile columns.
inline int tile_rows(long long rows, int edge = PLAN_GT) { return (int)((rows + edge - 1) / edge); }
AGP_HD inline long long lower_tile_count(int ntr, int ntc, int tri) {
  if (ntr <= 0 || ntc <= 0) return 0;
  if (!tri) return (long long)ntr * ntc;
  const long long c = ntc < ntr ? ntc : ntr;
  return c * ntr - c * (c - 1) / 2;
}
// number of tile (bi, bj) in the lower-triangular order: the tiles before column bj + (bi - bj)
inline long long lower_tile_index(int bi, int bj, int ntr) { return (long long)bj * ntr - (long long)bj * (bj - 1) / 2 + (bi - bj); }

// entries on or below the diagonal of C (M x M) covered by the first `count` lower 128 x 128 tiles
inline double lower_entries(long long M, int ntr, long long count) {
  double e = 0.;
  for (int bj = 0; bj < ntr && count > 0; ++bj) {
    const long long w = (M - (long long)bj * PLAN_GT < PLAN_GT) ? M - (long long)bj * PLAN_GT : PLAN_GT;  // tile column width
    for (int bi = bj; bi < ntr && count > 0; ++bi, --count) {
      const long long h = (M - (long long)bi * PLAN_GT < PLAN_GT) ? M - (long long)bi * PLAN_GT : PLAN_GT;
      e += (bi == bj) ? 0.5 * (double)w * (double)(w + 1) : (double)h * (double)w;
    }
  }
  return e;
}

// THE decode: tile number `id` -> (bi, bj).  A subtraction per tile column, no square root: at most ntc scalar iterations
// in front of a tile of thousands of MFMAs.  One loop, two entries:
//   lower_tile_of   stops once the column reaches ntc and returns false from lower_tile_count(ntr, ntc, tri) on
//   lower_tile_at   the walk without that bound, for 0 <= id < lower_tile_count ONLY: the fp64 kernels, whose grids the
//                   plans below make exactly that long, never had the bound, and the compare in the loop moves the
//                   register allocation of their whole tile bodies (profiles/r08/update_plan_resources.txt)
template <bool CHECKED>
AGP_HD inline bool lower_tile_walk(long long id, int ntr, int ntc, int tri, int &bi, int &bj) {
  int col = 0;
  while (true) {
    const int cnt = tri ? ntr - col : ntr;  // tri: column `col` holds the row tiles bi >= col
    if ((CHECKED && col >= ntc) || id < cnt) break;
    id -= cnt;
    ++col;
  }
  if (CHECKED && col >= ntc) return false;
  bj = col;
  bi = (tri ? col : 0) + (int)id;
  return true;
}
AGP_HD inline void lower_tile_at(long long id, int ntr, int tri, int &bi, int &bj) { (void)lower_tile_walk<false>(id, ntr, 0, tri, bi, bj); }
AGP_HD inline bool lower_tile_of(long long id, int ntr, int ntc, int tri, int &bi, int &bj) {
  return lower_tile_walk<true>(id, ntr, ntc, tri, bi, bj);
}

// ---- quadrants and staircase ----------------------------------------------------------------------------------------
// A 128-tile as four 64 x 64 workgroups: quadrant q = 0 .. 3 covers rows 64 qi.., columns 64 qj.. of the tile, qi = q & 1,
// qj = q >> 1; the upper quadrant of a diagonal tile has nothing to compute.
AGP_HD inline bool quadrant_skipped(int bi, int bj, int qi, int qj) { return bi == bj && qj > qi; }

// Staircase launches of the row-block-sharded fit (GemmArgs::stair): C is the stacked local row blocks of one rank, tpb
// tile rows each.  The row tile bi belongs to local block lb0 + bi / tpb = global block gi (snake deal over `world`
// ranks) and owns the tile columns up to its own diagonal tile; c0t: the tile column of the matrix that C's column 0 is.
AGP_HD inline bool stair_tile_owned(int bi, int bj, long long lb0, int tpb, int world, int rank, long long c0t) {
  const long long lb = lb0 + bi / tpb;
  const long long gi = lb * world + ((lb & 1) ? world - 1 - rank : rank);
  return bj <= gi * tpb - c0t + (bi % tpb);
}

// ---- the bulk trailing update (trailing_update_kernel) --------------------------------------------------------------
// A launch of T tiles runs floor(T / slots) full rounds of 128 x 128 workgroups (slots = 2 per CU); the T mod slots tiles
// left over would occupy a fraction of the chip for a whole further round.  They go FIRST, as four 64 x 64 workgroups
// each, so that the launch ends with full rounds.
// Fewer than BULK_WHOLE_FROM_ROUNDS rounds of large tiles: 64 x 64 workgroups throughout balance the CUs better (M = 4096,
// K = 512: 0.196 ms instead of 0.272; with the store-only epilogue of the large tiles two rounds are enough: M = 6144
// 448 -> 424 us, M = 7680 707 -> 670 us).
constexpr long long BULK_WHOLE_FROM_ROUNDS = 2;
// An almost full last round - from 3/4 of the slots on - is left to the large tiles.
constexpr long long BULK_ROUND_WHOLE_NUM = 3, BULK_ROUND_WHOLE_DEN = 4;

enum class SplitKernel {
  WholeAndQuadrants,  // trailing_update_kernel: [head,] 4 * rem quadrant workgroups, then `full` whole tiles
  QuadrantsOnly,      // trailing_update_tail_kernel: every tile as quadrants, four workgroups per CU
};
struct BulkSplit {
  long long full = 0, rem = 0;  // tiles [0, full) whole, [full, full + rem) as quadrants (column-major lower-tile order)
  SplitKernel kernel = SplitKernel::WholeAndQuadrants;
};

// tiles: of the sub-triangle right of the head (all of them without a head); merged: the launch begins with a head
inline BulkSplit plan_bulk_update(long long tiles, long long slots, bool merged) {
  BulkSplit sp;
  sp.rem = tiles;
  if (tiles >= BULK_WHOLE_FROM_ROUNDS * slots) {
    sp.full = tiles / slots * slots;
    sp.rem = tiles - sp.full;
    if (BULK_ROUND_WHOLE_DEN * sp.rem >= BULK_ROUND_WHOLE_NUM * slots) { sp.full = tiles; sp.rem = 0; }
  }
  // The one difference between the merged and the plain launch: all quadrants behind a head stay on
  // trailing_update_kernel, which runs the head; without one they go to the kernel that holds four workgroups per CU.
  if (sp.full == 0 && !merged) sp.kernel = SplitKernel::QuadrantsOnly;
  return sp;
}
// head_count: workgroups of the head; order_len: length of the whole tiles' order table (0: none, column-major order)
inline long long bulk_grid(const BulkSplit &sp, long long head_count, long long order_len) {
  return head_count + (order_len > 0 ? order_len : sp.full) + 4 * sp.rem;
}

// ---- C (M x N) -= A B^T, batched `count` times (launch_gemm_nt_sub_batched) --------------------------------------------
// Fewer than small_limit 128-tiles (AGP_GEMM_SMALL_LIMIT, default 512 = the workgroup slots, 2 per CU): 64 x 64 tiles
// instead (128 ... 512: flat, profiles/r03).
// With a transposed second operand, not triangular - launches that cannot fill the chip with 128 x 128 tiles (few
// right-hand sides, or the inner updates of a substitution with few rows) - the 64-tile kernel with the
// transposed-operand loader(s).  N = 16384, predict marginal: M = 64: 10.5 -> 5.0 ms, M = 1024: 12.3 -> 8.9 ms,
// M = 4096: 25.8 -> 24.8 ms.
// Fewer 64-tiles than CUs and a deep product: every wave would carry K / 4 x 4 MFMAs one behind the other on a mostly
// idle chip - 32 x 32 tiles (1536 x 512 x 512: 58 -> 2x us next to a bulk update).
constexpr long long NT_SUB_TINY_BELOW_TILES = 256, NT_SUB_TINY_FROM_K = 256;

struct NtSubPlan {
  int edge = PLAN_GT;       // 128: gemm_nt_sub_kernel<a_kmajor, b_kmajor>, 64: gemm64_nt_sub_kernel, 32: gemm32_nt_sub_kernel
  bool transposed = false;  // edge 64 only: gemm64_nt_sub_bk_kernel, all ntr x ntc tiles
  int ntr = 0, ntc = 0;     // in tiles of `edge`; tri: ntc <= ntr
  long long grid = 0;       // workgroups per problem (0: nothing to launch)
};

inline void cut_tiles(NtSubPlan &p, long long M, long long N, int edge, bool tri) {
  p.edge = edge;
  p.ntr = tile_rows(M, edge);
  p.ntc = tile_rows(N, edge);
  if (tri && p.ntc > p.ntr) p.ntc = p.ntr;
  p.grid = lower_tile_count(p.ntr, p.ntc, tri ? 1 : 0);
}

inline NtSubPlan plan_nt_sub(long long M, long long N, long long K, bool tri, bool a_kmajor, bool b_kmajor, long long count,
                             long long small_limit) {
  NtSubPlan p;
  cut_tiles(p, M, N, PLAN_GT, tri);
  if (p.grid <= 0 || p.grid * count >= small_limit) return p;
  if (b_kmajor && !tri) {
    cut_tiles(p, M, N, PLAN_ST, false);
    p.transposed = true;
  } else if (!a_kmajor && !b_kmajor) {
    cut_tiles(p, M, N, PLAN_ST, tri);
    if (p.grid * count < NT_SUB_TINY_BELOW_TILES && K >= NT_SUB_TINY_FROM_K) cut_tiles(p, M, N, PLAN_TT, tri);
  }
  return p;
}

// ---- staircase products of the sharded fit (launch_gemm_nt_sub_stair) -------------------------------------------------
// Few rounds of 128 x 128 tiles (a rank's share of a sharded fit: 12 tile rows): the last round is mostly idle slots -
// 64 x 64 tiles balance the CUs better.  (The staircase owns about half of the ntr x ntc grid; the single-GPU bulk update
// makes the same switch below BULK_WHOLE_FROM_ROUNDS = two rounds.)
constexpr long long STAIR_LARGE_FROM_ROUNDS = 4;

struct StairPlan {
  int edge = PLAN_GT;  // 128: gemm_nt_sub_kernel<false, false>, 64: gemm64_nt_sub_kernel; the grid is ntr * ntc
  int ntr = 0, ntc = 0;
  int st_tpb = 0;      // tile rows per row block
  long long st_c0t = 0;  // tile column of C's column 0
};

// block: rows per row block (a multiple of 128); c0: global column of C's column 0 (a multiple of 128)
inline StairPlan plan_stair(long long M, long long N, long long block, long long c0, long long slots) {
  const long long large = (long long)tile_rows(M) * tile_rows(N);
  StairPlan p;
  p.edge = large / 2 < STAIR_LARGE_FROM_ROUNDS * slots ? PLAN_ST : PLAN_GT;
  p.ntr = tile_rows(M, p.edge);
  p.ntc = tile_rows(N, p.edge);
  p.st_tpb = (int)(block / p.edge);
  p.st_c0t = c0 / p.edge;
  return p;
}

// ---- the order of the whole tiles -------------------------------------------------------------------------------------
// Bulk updates of the mixed fit (every tile whole): the XCD-aware order from this many tiles on
constexpr long long ORDERED_FROM_TILES = 1024;
inline bool mixed_bulk_ordered(long long tiles) { return tiles >= ORDERED_FROM_TILES; }

// The order in which the whole tiles [0, full) of a bulk update are handed out, for a part whose workgroup i runs on XCD
// i % 8: the lower-triangular tile grid is cut into 8 x 8 blocks of tiles; every XCD gets whole blocks (longest first to
// the least loaded XCD, then single tiles moved until the XCDs differ by at most one tile), so that the 64 workgroups
// resident on an XCD at a time read 16 panel strips between them instead of 65 - the strips are what the update fetches
// from the Infinity Cache / HBM (measured: FETCH_SIZE 5.8 -> 2.95 GB per launch at M = 15872, the launch 2 % faster, the
// fit 30.4 -> 30.05 ms; profiles/r04/bulk_update_vs_k.txt).
// Entry i of the table is the tile of workgroup i, bi << 16 | bj, or -1: no tile (only in the last row of XCDS).
constexpr int ORDER_BLOCK = 8;  // tiles a side (blocks of 4 ... 16 tiles a side measure the same)
constexpr int XCDS = 8;

inline std::vector<int> xcd_tile_order(int ntr, long long full) {
  constexpr int SB = ORDER_BLOCK;
  const int nsb = (ntr + SB - 1) / SB;
  std::vector<std::vector<int>> blocks;
  for (int SJ = 0; SJ < nsb; ++SJ)
    for (int SI = SJ; SI < nsb; ++SI) {
      std::vector<int> t;
      for (int tj = 0; tj < SB; ++tj)
        for (int ti = 0; ti < SB; ++ti) {
          const int bi = SI * SB + ti, bj = SJ * SB + tj;
          if (bi < ntr && bj <= bi && lower_tile_index(bi, bj, ntr) < full) t.push_back((bi << 16) | bj);
        }
      if (!t.empty()) blocks.push_back(std::move(t));
    }
  std::stable_sort(blocks.begin(), blocks.end(), [](const std::vector<int> &a, const std::vector<int> &b) { return a.size() > b.size(); });
  std::vector<std::vector<int>> per(XCDS);
  for (auto &b : blocks) {
    int best = 0;
    for (int x = 1; x < XCDS; ++x) if (per[x].size() < per[best].size()) best = x;
    per[best].insert(per[best].end(), b.begin(), b.end());
  }
  while (true) {  // single tiles from the longest list to the shortest
    int lo = 0, hi = 0;
    for (int x = 1; x < XCDS; ++x) { if (per[x].size() < per[lo].size()) lo = x; if (per[x].size() > per[hi].size()) hi = x; }
    if (per[hi].size() <= per[lo].size() + 1) break;
    per[lo].push_back(per[hi].back());
    per[hi].pop_back();
  }
  size_t L = 0;
  for (auto &v : per) L = std::max(L, v.size());
  std::vector<int> table(L * XCDS, -1);
  for (int x = 0; x < XCDS; ++x)
    for (size_t q = 0; q < per[x].size(); ++q) table[q * XCDS + x] = per[x][q];
  return table;
}

}  // namespace agp
