// batch_front.h — the front end the batched fits share (agp_nll_batch, agp_fit_create_batch and agp_fit_create_batch_ragged
// in api.hip, gradient_batch_begin in gradient.hip): "count Gram matrices into slabs, factored in lock step".  Host code
// only; the kernels it launches stay in gram.hip, chol.hip and ragged_batch.hip.  What differs between the entries - where the memory comes from,
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
// The same for problems of unequal sizes (agp_fit_create_batch_ragged): every n_b > 0, *n = the largest of them - the
// padded size of the call, which ldy and ldv are held to -, *equal = all sizes are that size.
int check_batch_problems_ragged(int count, const agp_kernel *const *kernels, const agp_features *const *features, int64_t ldy,
                                const double *y_var, int64_t ldv, long long *n, bool *equal);

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

// ---- fits of unequal sizes in one batch (ragged_batch.hip) -------------------------------------------------------------
// A fit of n_b points in a batch of padded size n carries the trailing phantom rows [n_b, n) (common.h: agp_fit::phantom).
// One problem of the pad launch that runs behind the Gram launches, which work on views of n_b rows: the phantom rows of
// the lower triangle of slab b become e_i^T, z_b is zeroed there, and the phantom rows of the training features become
// copies of the problem's first feature (ids: -2 - k, which no caller's id equals).  An item with dim = 0, nsc = 0 and
// ids = nullptr (the batched gradients, which keep no features) has the slab and z written and nothing else touched.
struct RaggedPadItem {
  double *A, *z;       // slab b (ld = lda) and its targets
  double *coords;      // n rows
  long long *ids;      // n ids or null
  double *scales;      // nsc columns at stride n, or null
  long long nb;        // real rows
  int dim, nsc;
};
void launch_ragged_pad(hipStream_t s, const RaggedPadItem *table_dev, long long count, long long n, long long lda);

// Half-open ranges of phantom rows per problem, for the table-driven zero fills: problem b owns the `count` ranges from
// `first` on in an array of (begin, end) pairs.  In device memory the items come first, then the pairs.
struct RangeItem {
  long long first, count;
};
struct RangeTable {
  std::vector<RangeItem> items;
  std::vector<long long> pairs;
  void begin_problem() { items.push_back(RangeItem{(long long)pairs.size() / 2, 0}); }
  void add(long long r0, long long r1) {
    if (r1 <= r0) return;
    pairs.push_back(r0);
    pairs.push_back(r1);
    ++items.back().count;
  }
  bool any() const { return !pairs.empty(); }
  size_t item_bytes() const { return sizeof(RangeItem) * items.size(); }
  size_t bytes() const { return item_bytes() + sizeof(long long) * pairs.size(); }
  void write(void *dst) const;  // items | pairs, as the kernels read them
};
// table_dev holds a table of `total` problems; the launches below work on the `count` problems from `first` on, whose
// matrices lie at one stride from the pointer given (blockIdx.y = problem - first).
// rows [r0, r1) of all m columns of V_b (ld = ldv) <- 0 for every range (r0, r1) of problem b
void launch_zero_row_ranges(hipStream_t s, const void *table_dev, long long total, long long first, long long count, double *V,
                            long long stride_V, long long ldv, long long m);
// rows 0 .. m of the columns [c0, c1) of X_b (ld) <- 0 for every range (c0, c1) of problem b
void launch_zero_column_ranges(hipStream_t s, const void *table_dev, long long total, long long first, long long count, double *X,
                               long long stride_X, long long ld, long long m);

// agp_fit_create_batch and agp_fit_create_batch_ragged (api.hip): one body; `ragged` admits unequal sizes
int fit_create_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features, const double *y,
                     int64_t ldy, const double *y_var, int64_t ldv, agp_fit **out, double *information, int64_t ldi, double *log_det,
                     int *status, bool ragged);

}  // namespace agp
