// batch_front.h — the front end the batched fits share (agp_nll_batch and agp_fit_create_batch in api.hip,
// gradient_batch_begin in gradient.hip): "count Gram matrices into slabs, factored in lock step".  Host code only; the
// kernels it launches stay in gram.hip and chol.hip.  What differs between the entries - where the memory comes from,
// the status words, whether the look-ahead schedule may be used, what follows the factor - is an argument at the call.
#pragma once
#include <vector>

#include "api_internal.h"
#include "batch_layout.h"
#include "pub.h"

namespace agp {

constexpr int BATCH_MAX_PROBLEMS = 65535;  // gridDim.y of every batched launch

BatchGeometry batch_geometry(long long n, long long count);

// The argument checks of a batch, all made before anything is written or launched: count in 1 .. BATCH_MAX_PROBLEMS,
// every kernel and feature view there and valid, one n > 0 (-> *n), one location, ldy and (with y_var) ldv 0 or >= n.
int check_batch_problems(int count, const agp_kernel *const *kernels, const agp_features *const *features, int64_t ldy,
                         const double *y_var, int64_t ldv, long long *n);

// n x columns values (targets, variances) at `location`, leading dimension ld, into dst with leading dimension ld_dst:
// one pitched copy, or with ld = 0 the one shared vector into every column.  Enqueued on the context's stream.
int upload_problem_columns(agp_context *ctx, const double *src, int64_t ld, long long n, long long columns, int location,
                           double *dst, long long ld_dst);

// The per-problem tables of the Gram launches.  Problem b writes slab b of A, adds yvar + b * stride_yvar to its
// diagonal (yvar may be null) and reports NaN in flags + b * stride_flags (flags may be null).
struct BatchGramTables {
  std::vector<FeatView> views;
  std::vector<const DevProgram *> hprogs;
  std::vector<double *> outs;
  std::vector<const double *> diag;
  std::vector<int *> nanf;
  std::vector<DeviceFeatures> uploads;  // what upload_features made; released with the tables
  BatchGramTables(const BatchGeometry &g, const agp_kernel *const *kernels, double *A, const double *yvar, long long stride_yvar,
                  int *flags, long long stride_flags);
  // problem b's features as the Gram reads them: as_measurements(features), gp.hpp:288
  void set_view(int b, FeatView v) { v.meas = 1; views[(size_t)b] = v; }
  // every view through to_device; an array shared with the previous problem (parameter vectors of one model) goes up once
  int upload_features(agp_context *ctx, const agp_features *const *features);
};

// All Gram matrices in ONE launch when the trees share a fast path (gram.hip; the descriptor table goes to table_dev
// through table_pinned, see common.h), else - or with one problem, or without a table - a launch each.
int launch_batch_grams(agp_context *ctx, const BatchGeometry &g, const BatchGramTables &t, const agp_kernel *const *kernels,
                       void *table_dev, void *table_pinned);

// The schedule of the factorisation.  Two streams once the trailing updates of the batch are long enough to hide the
// panel chain behind; otherwise one, with fused POTRF + TRSM panel launches for batches whose workgroups fit on the chip
// at once - those publish z through a slab of their own (zpub) and read the tile images as hand-over buffers.
bool batched_lookahead(long long count, long long n);
bool batched_fused_panels(agp_context *ctx, const BatchGeometry &g, bool allow_lookahead);
// `prep` plus the sentinel fill of the hand-over buffers of the fused panel launches (zpub null: none), launched
void launch_batch_prep(hipStream_t s, PrepArgs &prep, const BatchGeometry &g, double *invd, double *zpub);
// L_b and z_b = L_b^-1 y_b in place, log sums and status words (flags + b * stride_flags) as factor_lower_batched documents
void factor_batch(agp_context *ctx, const BatchGeometry &g, bool allow_lookahead, double *A, double *invd, double *z, int *flags,
                  long long stride_flags, double *logsum, double *zpub);

}  // namespace agp
