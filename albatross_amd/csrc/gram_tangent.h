// gram_tangent.h — the tangent bilinear forms forms[c, p] = U[:, c]^T (dk(x, x) / dslot_p) V[:, c] of gram_tangent.hip as the
// other translation units see them (iterative.hip: the probe gradient of the matrix-free fit; debug_api.hip: the plan a
// test reads).
#pragma once
#include "common.h"
#include "contract.h"

namespace agp {

constexpr int TF_ROWS = 256;            // rows of a row block, one per lane
constexpr int TF_COLS = 64;             // columns of an LDS tile
constexpr int TF_MAX_PAIRS = 8;         // column pairs (U[:, c], V[:, c]) of a chunk: TF_MAX_PAIRS x GRAD_GROUP accumulators per lane
static_assert(TF_MAX_PAIRS == AGP_TANGENT_FORMS_MAX_PAIRS, "the chunk width include/albatross_amd.h documents");
constexpr int TF_MIN_SLICE_TILES = 4;   // column tiles of a slice at least
constexpr int TF_TARGET_WGS = 1024;     // workgroups the slicing aims at (four per CU)

// A workgroup (unit q, slice s) owns the row blocks q and nb - 1 - q (the same block once in the middle of an odd nb) and
// walks tiles [s * tiles_per_slice, (s + 1) * tiles_per_slice) of the unit's list: the column tiles 0 .. of row block q up
// to its diagonal, then those of row block nb - 1 - q.  Depends on n alone.
struct TfPlan {
  long long row_blocks, units, slices, tiles_per_slice, max_tiles;  // max_tiles: the longest list of a unit
};
TfPlan gram_tangent_plan(long long n);
// column pairs the next chunk's kernel holds (1, 4 or TF_MAX_PAIRS) when `remaining` are left
int gram_tangent_chunk_width(long long remaining);
// doubles of scratch launch_gram_tangent_forms needs for n rows: one TF_MAX_PAIRS x GRAD_GROUP block per workgroup
size_t gram_tangent_ws_elems(long long n);
// forms[c + p * ldf] = sum_ij U[i, c] (dk(x_i, x_j) / dslot_p) V[j, c], c < ncols, p < n_slots, everything on the device;
// tang / ldt: the tangent columns of the AGP_OP_SCALING slots (or nullptr); the slot table has passed check_slots.  nan_flag
// is raised when an evaluated tangent is NaN; go (optional): a device word, the launches return at once when it holds a
// value <= 0.  Launches only: no allocation, no synchronisation.
void launch_gram_tangent_forms(hipStream_t s, const DevProgram *P, const agp_kernel *k, const FeatView &X, int n_slots,
                               const agp_gradient_slot *slots, const double *tang, long long ldt, const double *U, long long ldu,
                               const double *V, long long ldv, long long ncols, double *forms, long long ldf, double *ws,
                               int *nan_flag, const int *go = nullptr);

}  // namespace agp
