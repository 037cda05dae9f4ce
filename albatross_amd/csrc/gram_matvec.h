// gram_matvec.h — the fused product (k(x, x) + diag(y_var)) V of gram_matvec.hip as the other translation units see it
// (iterative.hip: the conjugate-gradient solve; debug_api.hip: the plan a test asserts).
#pragma once
#include "common.h"

namespace agp {

constexpr int MV_ROWS = 256;          // rows of a workgroup, one per lane
constexpr int MV_COLS = 64;           // columns of an LDS tile
constexpr int MV_MAX_RHS = 16;        // AGP_MATVEC_MAX_RHS: right-hand sides of a chunk (accumulators of a lane)
constexpr int MV_MIN_SLICE = 256;     // columns of a slice at least
constexpr int MV_TARGET_WGS = 1024;   // workgroups the column split aims at (four per CU)

// which evaluator forms K_ij (the pair-2 trees of gram.hip take SOP: the same arithmetic)
constexpr int MV_PATH_FAST = 0, MV_PATH_SOP = 1, MV_PATH_INTERP = 2;

struct MvPlan {
  int path;
  long long slices, cols_per_slice;
};

// what launch_gram_matvec will run for these features (it switches on the same choice)
MvPlan gram_matvec_plan(const DevProgram *host_program, const FeatView &X);
void gram_matvec_slices(long long n, long long *slices, long long *cols_per_slice);
// right-hand sides the next chunk's kernel holds (1, 4 or MV_MAX_RHS) when `remaining` are left
int gram_matvec_chunk_width(long long remaining);
// doubles of scratch launch_gram_matvec needs for n rows (0: one slice, no partial sums)
size_t gram_matvec_ws_elems(long long n);
// out[:, c] = (k(x, x) + diag(yvar)) V[:, c], c < nrhs, everything on the device; yvar may be nullptr; nan_flag is raised
// when an evaluated entry is NaN.  V and out must not overlap.  go (optional): a device word; the launches return at once when it
// holds a value <= 0.  Launches only: no allocation, no synchronisation.
void launch_gram_matvec(hipStream_t s, const DevProgram *P, const DevProgram *host_program, const FeatView &X, const double *yvar,
                        const double *V, long long ldv, long long nrhs, double *out, long long ldo, double *ws, int *nan_flag,
                        const int *go = nullptr);

}  // namespace agp
