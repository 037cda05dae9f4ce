// predict_batch.hip — agp_predict_batch: the predictions of `count` small fits in lock step (gp.hpp:305-366, 82-113 for
// every problem at once).  A fit of a few hundred points predicts in a handful of launches that are all latency-bound
// (N = 512, M = 512: 0.05 / 0.18 / 0.51 ms for mean / marginal / joint); a batch of fits whose factors lie at one
// stride - the handles of one agp_fit_create_batch call, or any evenly spaced subset of them - runs each of those launches
// ONCE for all problems (one grid dimension = problem, per-problem pointers and parameters in a table in device memory):
//
//   K*_b  = cov(train_b, xs_b)          cross_fast_batch_kernel (the tile body of gram.hip) -> V_b (n x m)
//   mean_b = K*_b^T alpha_b             colvec_batch_kernel<false>, before V is overwritten
//   V_b   <- L_b^-1 V_b                 forward_solve_mat_batched (solve.hip)
//   marginal:  prior_b = diag cov(xs_b)           prior_fast_batch_kernel
//              var_b = prior_b - colsum(V_b o V_b)  colvec_batch_kernel<true>
//   joint:     P_b = cov(xs_b, xs_b), lower tiles   launch_gram_batch (gram.hip)
//              P_b -= V_b^T V_b, lower tiles        launch_gemm_nt_sub_batched (gemm.hip)
//              cov_b = full symmetric P_b, ld = m   symmetrize_pack_batch_kernel
//   mean only: mean_b = K*_b^T alpha_b without K*   mean_fast_batch_kernel
//
// Fits with phantom rows (agp_fit_create_batch_ragged, agp_fit_update_batch; common.h: agp_fit::phantom) run in lock step
// like any other: every kernel works on the padded size.  The covariance with a phantom row is zero by definition, but
// its feature row holds a copy of a real feature, so the phantom rows of K*_b are zeroed by ONE table-driven launch per
// sub-batch (any number of ranges per problem; ragged_batch.hip) right behind the cross covariance.  The mean-only kernel
// needs nothing of the kind: alpha_b is exactly zero on phantom rows and the covariance there is finite.
//
// The table-driven covariance launches cover the radial<Euclidean> [+ noise] trees (gram_fast.h).  When every problem of
// a run has such a tree with one operator and one dimension they are one launch; otherwise every problem gets a launch
// of its own - the SAME kernel on its table entry when its tree has the shape, the generic program launchers of gram.hip
// when not.  Either way a problem is evaluated by the same code with the same arguments: its bits do not depend on its
// neighbours.  Every reduction has a fixed order; there are no floating-point atomics.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "batch_front.h"
#include "gram_fast.h"

namespace agp {

// One problem of a lock-step launch.  The covariance kernels read fp / X / Y, the reductions the pointers.
struct PredictBatchItem {
  FastParams fp;
  FeatView X;           // training features of the fit
  FeatView Y;           // test features
  const double *alpha;  // information vector (n)
  double *V;            // n x m slab: K*, then L^-1 K*
  double *prior;        // marginal: m prior variances; joint: m x m prior covariance (ld = round_up(m, 2))
  double *mean;         // where the m means go
  double *second;       // where the m variances / the m x m covariance (ld = m) go
};

// K*_b into V_b: blockIdx = (row tile, column tile, problem) of 128 x 32 tiles, partial tiles masked in the body
template <int DIMP, int OP>
__global__ __launch_bounds__(GRAM_THREADS) void cross_fast_batch_kernel(const PredictBatchItem *__restrict__ items, long long ldv) {
  const PredictBatchItem it = items[blockIdx.z];
  if ((long long)blockIdx.x * TM >= it.X.n || (long long)blockIdx.y * TN >= it.Y.n) return;
  gram_fast_body<DIMP, OP>(it.fp, it.X, it.Y, 0, it.V, ldv, nullptr, nullptr, 0, 0, blockIdx.x, blockIdx.y);
}

// mean_b[j] = sum_i k(x_i, xs_j) alpha_i without the cross covariance: a wave per test point, the training points over
// its lanes (the arithmetic of gram.hip's predict_mean_fast_kernel), blockIdx.y = problem
constexpr int PB_WAVES = 4;
template <int DIMP, int OP>
__global__ __launch_bounds__(64 * PB_WAVES) void mean_fast_batch_kernel(const PredictBatchItem *__restrict__ items) {
  const PredictBatchItem it = items[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * PB_WAVES + wave;
  if (j >= it.Y.n) return;
  double y[DIMP];
#pragma unroll
  for (int d = 0; d < DIMP; ++d) y[d] = it.Y.coords[j * DIMP + d];
  const bool have_ids = it.X.ids != nullptr && it.Y.ids != nullptr;
  const long long yid = have_ids ? it.Y.ids[j] : -1;
  const bool noise_on = it.fp.has_noise && (!it.fp.noise_meas_only || (it.X.meas && it.Y.meas));
  double acc = 0.;
  for (long long i = lane; i < it.X.n; i += 64) {
    bool eq = true;
    double s = 0.;
#pragma unroll
    for (int d = 0; d < DIMP; ++d) {
      const double xd = it.X.coords[i * DIMP + d];
      const double t = xd - y[d];
      s += t * t;
      eq = eq && (xd == y[d]);
    }
    if (have_ids) eq = it.X.ids[i] == yid;
    double v = radial_fast<OP>(s, it.fp);
    if (it.fp.has_noise) v = v + ((noise_on && eq) ? it.fp.noise_var : 0.);
    acc += v * it.alpha[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) it.mean[j] = acc;
}

// prior_b[j] = k(xs_j, xs_j) (gp.hpp:339-343): the pair arithmetic of the tile body for a point and itself
template <int DIMP, int OP>
__global__ __launch_bounds__(256) void prior_fast_batch_kernel(const PredictBatchItem *__restrict__ items) {
  const PredictBatchItem it = items[blockIdx.y];
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= it.Y.n) return;
  double s = 0.;
  bool eq = true;
#pragma unroll
  for (int d = 0; d < DIMP; ++d) {
    const double yd = it.Y.coords[j * DIMP + d];
    const double t = yd - yd;  // (NaN coordinates stay NaN)
    s += t * t;
    eq = eq && (yd == yd);
  }
  if (it.Y.ids) eq = true;
  const bool noise_on = it.fp.has_noise && (!it.fp.noise_meas_only || it.Y.meas);
  double v = radial_fast<OP>(s, it.fp);
  if (it.fp.has_noise) v = v + ((noise_on && eq) ? it.fp.noise_var : 0.);
  it.prior[j] = v;
}

// One workgroup per (column j, problem): 256 threads stride over the n rows of V_b[:, j], shuffle reduction per wave, the
// four wave sums added as (0 + 1) + (2 + 3) - the order of reduce.hip's column reductions.
//   SQUARE = false: mean_b[j]   = sum_i V_b[i, j] alpha_b[i]          (gp.hpp:82-85, on K* before the substitution)
//   SQUARE = true:  second_b[j] = prior_b[j] - sum_i V_b[i, j]^2      (gp.hpp:96-99, on L^-1 K*)
template <bool SQUARE>
__global__ __launch_bounds__(256) void colvec_batch_kernel(const PredictBatchItem *__restrict__ items, long long ldv, long long n) {
  __shared__ double red[4];
  const PredictBatchItem &it = items[blockIdx.y];
  const long long j = blockIdx.x;
  const double *v = it.V + j * ldv;
  const double *a = it.alpha;
  double acc = 0.;
  for (long long i = threadIdx.x; i < n; i += 256) acc += SQUARE ? v[i] * v[i] : v[i] * a[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    if (SQUARE) it.second[j] = it.prior[j] - s;
    else it.mean[j] = s;
  }
}

// second_b (m x m, ld = m, full) = the symmetric matrix whose lower triangle is prior_b (ld = ldp): 32 x 32 tiles on or
// below the diagonal, each written once as it is and once mirrored (reduce.hip: symmetrize_kernel), blockIdx.z = problem
__global__ __launch_bounds__(256) void symmetrize_pack_batch_kernel(const PredictBatchItem *__restrict__ items, long long ldp, long long m) {
  __shared__ double tile[32][33];
  const long long bi = blockIdx.x, bj = blockIdx.y;
  if (bj > bi) return;
  const double *S = items[blockIdx.z].prior;
  double *D = items[blockIdx.z].second;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const long long row = bi * 32 + tx, col = bj * 32 + r;
    const bool in = row < m && col < m;
    const double v = in ? S[col * ldp + row] : 0.;
    tile[r][tx] = v;
    if (in && row >= col) D[col * m + row] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const long long row = bj * 32 + tx, col = bi * 32 + r;  // D[row, col] = S[col, row]
    if (row < m && col < m && row < col) D[col * m + row] = tile[tx][r];
  }
}

__global__ __launch_bounds__(256) void fill_nan_kernel(double *p, long long count) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) p[i] = __longlong_as_double(0x7ff8000000000000LL);
}

#define AGP_PB_OPS(LAUNCH, D)                                                     \
  switch (op) {                                                                   \
  case AGP_OP_SQUARED_EXPONENTIAL: LAUNCH(D, AGP_OP_SQUARED_EXPONENTIAL); break;  \
  case AGP_OP_EXPONENTIAL: LAUNCH(D, AGP_OP_EXPONENTIAL); break;                  \
  case AGP_OP_MATERN32: LAUNCH(D, AGP_OP_MATERN32); break;                        \
  default: LAUNCH(D, AGP_OP_MATERN52); break;                                     \
  }
#define AGP_PB_DIMS(LAUNCH)                  \
  do {                                       \
    if (dim == 1) { AGP_PB_OPS(LAUNCH, 1) }  \
    else if (dim == 2) { AGP_PB_OPS(LAUNCH, 2) } \
    else { AGP_PB_OPS(LAUNCH, 3) }           \
  } while (0)

// `count` table entries from `tab` on: their cross covariances / means / prior variances (op, dim: of all of them)
static void launch_cross_fast_batch(hipStream_t s, const PredictBatchItem *tab, long long count, int op, int dim, long long n, long long m,
                                    long long ldv) {
  dim3 grid((unsigned)((n + TM - 1) / TM), (unsigned)((m + TN - 1) / TN), (unsigned)count), block(GRAM_THREADS);
#define AGP_PB_CROSS(D, O) hipLaunchKernelGGL((cross_fast_batch_kernel<D, O>), grid, block, 0, s, tab, ldv)
  AGP_PB_DIMS(AGP_PB_CROSS);
#undef AGP_PB_CROSS
}
static void launch_mean_fast_batch(hipStream_t s, const PredictBatchItem *tab, long long count, int op, int dim, long long m) {
  dim3 grid((unsigned)((m + PB_WAVES - 1) / PB_WAVES), (unsigned)count), block(64 * PB_WAVES);
#define AGP_PB_MEAN(D, O) hipLaunchKernelGGL((mean_fast_batch_kernel<D, O>), grid, block, 0, s, tab)
  AGP_PB_DIMS(AGP_PB_MEAN);
#undef AGP_PB_MEAN
}
static void launch_prior_fast_batch(hipStream_t s, const PredictBatchItem *tab, long long count, int op, int dim, long long m) {
  dim3 grid((unsigned)((m + 255) / 256), (unsigned)count), block(256);
#define AGP_PB_PRIOR(D, O) hipLaunchKernelGGL((prior_fast_batch_kernel<D, O>), grid, block, 0, s, tab)
  AGP_PB_DIMS(AGP_PB_PRIOR);
#undef AGP_PB_PRIOR
}
#undef AGP_PB_DIMS
#undef AGP_PB_OPS

// Problems per lock-step launch chain: the V slabs (round_up(n, 2) x m each) and, for a joint prediction, the prior slabs
// (round_up(m, 2) x m each) of one sub-batch stay within 2^28 doubles = 2 GiB, the bound of a single marginal prediction
// (api.hip: marginal_chunk); at least one problem, at most what a grid dimension holds.
// AGP_PREDICT_CHUNK=<points> (the test points per slice of agp_predict_marginal) counts the columns of all V slabs here:
// a sub-batch holds max(1, floor(points / m)) problems.
static long long predict_batch_cap(const agp_context *ctx, long long n, long long m, int mode) {
  if (ctx->tune.predict_chunk > 0) {
    const long long c = ctx->tune.predict_chunk / (m > 0 ? m : 1);
    return c < 1 ? 1 : (c > 65535 ? 65535 : c);
  }
  const double per = (mode == 0 ? 0. : (double)round_up(n, 2) * (double)m) + (mode == 2 ? (double)round_up(m, 2) * (double)m : 0.);
  if (per <= 0.) return 65535;
  const double c = std::floor((double)(1LL << 28) / per);
  return c < 1. ? 1 : (c > 65535. ? 65535 : (long long)c);
}

}  // namespace agp

using namespace agp;

namespace {
struct Run {
  int first = 0, count = 0;
  long long dA = 0, dI = 0, dAl = 0;
  bool uniform = false;  // every tree has the radial fast-path shape, with one operator and one dimension
  int op = 0, dim = 0;
};
}  // namespace

extern "C" {

int agp_predict_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_fit *const *fits,
                      const agp_features *const *xs, int mode, double *mean, int64_t ldm, double *second, int64_t lds,
                      int out_location, int *status) {
  if (!c || count <= 0 || !kernels || !fits || !xs || !mean || !status || mode < 0 || mode > 2 || (mode != 0 && !second))
    return AGP_ERR_INVALID_ARGUMENT;
  if (out_location != AGP_HOST && out_location != AGP_DEVICE) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  if (!kernels[0] || !fits[0] || !xs[0]) return AGP_ERR_INVALID_ARGUMENT;
  const long long m = xs[0]->n, n_pad = fits[0]->n;
  const int loc = xs[0]->location;
  for (int b = 0; b < count; ++b) {
    const agp_fit *f = fits[b];
    if (!kernels[b] || !f || !xs[b] || validate_features(xs[b]) != AGP_OK) return AGP_ERR_INVALID_ARGUMENT;
    if (xs[b]->n != m || xs[b]->location != loc || f->ctx != c || f->mixed || f->n != n_pad) return AGP_ERR_INVALID_ARGUMENT;
    // a fit without training features (agp_factor_create), or whose features have another dimension than the test points
    if (f->fail_status == AGP_OK && (!f->A || !f->invd || !f->alpha || !f->train.v.coords)) return AGP_ERR_INVALID_ARGUMENT;
    if (f->train.v.coords && xs[b]->dim != f->train.v.dim) return AGP_ERR_INVALID_ARGUMENT;
  }
  if (ldm < m || (mode == 1 && lds < m) || (mode == 2 && lds < m * m)) return AGP_ERR_INVALID_ARGUMENT;
  for (int b = 0; b < count; ++b) status[b] = fits[b]->fail_status;
  if (m == 0) return AGP_OK;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const long long second_elems = mode == 1 ? m : m * m;  // per problem

  // ---- the runs: maximal stretches of good fits whose factors, tile images and information vectors lie at one stride
  auto lockstep_ok = [&](int b) {
    const agp_fit *f = fits[b];
    return f->fail_status == AGP_OK;
  };
  std::vector<Run> runs;
  for (int b = 0; b < count;) {
    Run r;
    r.first = b;
    r.count = 1;
    if (lockstep_ok(b)) {
      const agp_fit *f0 = fits[b];
      while (b + r.count < count && lockstep_ok(b + r.count)) {
        const agp_fit *p = fits[b + r.count - 1], *q = fits[b + r.count];
        if (q->n != f0->n || q->lda != f0->lda) break;
        // (the handles may belong to unrelated allocations: compare addresses, not pointers)
        auto step = [](const double *to, const double *from, long long *d) {
          const uintptr_t a = reinterpret_cast<uintptr_t>(to), b = reinterpret_cast<uintptr_t>(from);
          if (a < b || (a - b) % sizeof(double) != 0) return false;
          *d = (long long)((a - b) / sizeof(double));
          return true;
        };
        long long dA = 0, dI = 0, dAl = 0;
        if (!step(q->A, p->A, &dA) || !step(q->invd, p->invd, &dI) || !step(q->alpha, p->alpha, &dAl)) break;
        if (r.count == 1) { r.dA = dA; r.dI = dI; r.dAl = dAl; }
        else if (dA != r.dA || dI != r.dI || dAl != r.dAl) break;
        ++r.count;
      }
    }
    runs.push_back(r);
    b += r.count;
  }
  // every tree of a lock-step run is matched against the fast-path shapes ONCE: fast[b], ops[b], fps[b]
  bool any_lockstep = false;
  std::vector<char> fast((size_t)count, 0);
  std::vector<int> ops((size_t)count, 0);
  std::vector<FastParams> fps((size_t)count);
  for (Run &r : runs) {
    if (r.count < 2) continue;
    any_lockstep = true;
    r.uniform = true;
    for (int i = 0; i < r.count; ++i) {
      const int b = r.first + i, dim = fits[b]->train.v.dim;
      fast[(size_t)b] = dim <= 3 && gram_match_fast(kernels[b]->prog, &fps[(size_t)b], &ops[(size_t)b]);
      if (i == 0) { r.op = ops[(size_t)b]; r.dim = dim; }
      if (!fast[(size_t)b] || ops[(size_t)b] != r.op || dim != r.dim) r.uniform = false;
    }
  }

  // the phantom ranges of the fits in lock-step runs (modes that form V only)
  RangeTable phantoms;
  if (any_lockstep && mode != 0) {
    std::vector<char> in_run((size_t)count, 0);
    for (const Run &r : runs)
      for (int i = 0; r.count > 1 && i < r.count; ++i) in_run[(size_t)(r.first + i)] = 1;
    for (int b = 0; b < count; ++b) {
      phantoms.begin_problem();
      if (in_run[(size_t)b])
        for (const auto &ph : fits[b]->phantom) phantoms.add(ph.first, ph.second);
    }
  }
  // ---- descriptor tables of the whole call: device scratch + the context's pinned staging area, entry b = problem b
  const size_t item_bytes = (sizeof(PredictBatchItem) * (size_t)count + 15) / 16 * 16;
  const size_t gram_bytes = mode == 2 ? (gram_batch_table_bytes(count) + 15) / 16 * 16 : 0;
  const size_t range_off = item_bytes + gram_bytes, range_bytes = phantoms.any() ? phantoms.bytes() : 0;
  DevMem<void> tables;
  char *pinned = nullptr;
  std::vector<PredictBatchItem> pageable;
  if (any_lockstep) {
    if (tables.alloc_cached(range_off + range_bytes) != 0) {
      (void)hipGetLastError();
      ctx->last_error = "agp_predict_batch: descriptor tables";
      return AGP_ERR_HIP;
    }
    pinned = static_cast<char *>(host_stage(ctx, range_off + range_bytes));
    if (!pinned) pageable.resize((size_t)count);
  }
  PredictBatchItem *h_items = pinned ? reinterpret_cast<PredictBatchItem *>(pinned) : pageable.data();
  PredictBatchItem *d_items = static_cast<PredictBatchItem *>(tables.get());
  const size_t gram_item = mode == 2 ? gram_batch_table_bytes(1) : 0;

  int st = AGP_OK;
  auto finish = [&](int code) {
    (void)hipStreamSynchronize(s);
    return code;
  };
  std::vector<char> pageable_ranges;
  if (range_bytes > 0) {  // one upload for the whole call
    char *src = pinned ? pinned + range_off : nullptr;
    if (!src) { pageable_ranges.resize(range_bytes); src = pageable_ranges.data(); }
    phantoms.write(src);
    if (hipMemcpyAsync(static_cast<char *>(tables.get()) + range_off, src, range_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
      ctx->last_error = "agp_predict_batch: phantom range table";
      return finish(AGP_ERR_HIP);
    }
    if (!pinned) (void)hipStreamSynchronize(s);  // (pageable source)
  }
  // Test features of the lock-step runs on the device.  Device-resident arrays are used where they are.  Host arrays go
  // into ONE allocation for the whole call (coordinates | equality ids | scale columns per problem; consecutive problems
  // that share their arrays share the copy) with ONE synchronisation behind the uploads, as agp_fit_create_batch stages
  // its training features: no allocation and no synchronisation per problem.
  std::vector<FeatView> yv((size_t)count);
  DevMem<double> xbuf;
  if (any_lockstep) {
    auto same_arrays = [&](int a, int b) {
      return xs[a]->coords == xs[b]->coords && xs[a]->scales == xs[b]->scales && xs[a]->eq_id == xs[b]->eq_id && xs[a]->dim == xs[b]->dim &&
             xs[a]->n_scale_columns == xs[b]->n_scale_columns;
    };
    auto words = [&](const agp_features *f) { return (size_t)m * ((size_t)f->dim + (f->eq_id ? 1 : 0) + (size_t)f->n_scale_columns); };
    size_t total = 0;
    if (loc == AGP_HOST)
      for (const Run &r : runs)
        for (int i = 0; r.count > 1 && i < r.count; ++i)
          if (i == 0 || !same_arrays(r.first + i, r.first + i - 1)) total += words(xs[r.first + i]);
    if (total > 0 && xbuf.alloc_cached(sizeof(double) * total) != 0) {
      (void)hipGetLastError();
      ctx->last_error = "agp_predict_batch: test feature staging";
      return AGP_ERR_HIP;
    }
    double *cur = xbuf;
    for (const Run &r : runs)
      for (int i = 0; r.count > 1 && i < r.count; ++i) {
        const int b = r.first + i;
        const agp_features *f = xs[b];
        FeatView v;
        if (i > 0 && same_arrays(b, b - 1)) {
          v = yv[(size_t)b - 1];
        } else {
          v.n = m; v.dim = f->dim; v.nsc = f->n_scale_columns; v.sstride = 0;
          v.coords = f->coords;
          v.ids = reinterpret_cast<const long long *>(f->eq_id);
          v.scales = f->n_scale_columns > 0 ? f->scales : nullptr;
          if (loc == AGP_HOST) {
            auto up = [&](const void *src, size_t n_words) -> const double * {
              double *dst = cur;
              cur += n_words;
              if (hipMemcpyAsync(dst, src, sizeof(double) * n_words, hipMemcpyHostToDevice, s) != hipSuccess) st = AGP_ERR_HIP;
              return dst;
            };
            v.coords = up(f->coords, (size_t)m * (size_t)f->dim);
            if (f->eq_id) v.ids = reinterpret_cast<const long long *>(up(f->eq_id, (size_t)m));
            if (f->n_scale_columns > 0) v.scales = up(f->scales, (size_t)m * (size_t)f->n_scale_columns);
          }
        }
        v.meas = f->is_measurement;
        yv[(size_t)b] = v;
      }
    if (st != AGP_OK) {
      ctx->last_error = "agp_predict_batch: test feature upload";
      return finish(st);
    }
    if (loc == AGP_HOST && total > 0) AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // (pageable sources: the one wait of the host path)
  }

  const long long ldv = round_up(n_pad, 2), ldc = round_up(m, 2);  // (V has the padded rows of the fits)
  for (const Run &r : runs) {
    if (r.count == 1) {
      const int b = r.first;
      if (fits[b]->fail_status != AGP_OK) continue;  // its outputs are NaN-filled below
      // today's path, unchanged (a fit grown by agp_fit_update, a fit of its own allocation, a leftover of a cut)
      if (mode == 0) st = agp_predict_mean(c, kernels[b], fits[b], xs[b], mean + (size_t)b * (size_t)ldm, out_location);
      else if (mode == 1)
        st = agp_predict_marginal(c, kernels[b], fits[b], xs[b], mean + (size_t)b * (size_t)ldm, second + (size_t)b * (size_t)lds, out_location);
      else
        st = agp_predict_joint(c, kernels[b], fits[b], xs[b], mean + (size_t)b * (size_t)ldm, second + (size_t)b * (size_t)lds, out_location);
      if (st != AGP_OK) return finish(st);
      continue;
    }
    const agp_fit *f0 = fits[r.first];
    const long long rn = f0->n;  // (the padded size)
    const long long cap = predict_batch_cap(ctx, rn, m, mode);
    for (int p0 = 0; p0 < r.count; p0 += (int)cap) {
      const int first = r.first + p0;
      const long long cnt = std::min<long long>(cap, r.count - p0);
      // workspace: V slabs | prior slabs | (host outputs) mean and second staging
      const size_t v_elems = mode == 0 ? 0 : (size_t)ldv * (size_t)m, p_elems = mode == 0 ? 0 : (mode == 1 ? (size_t)ldc : (size_t)ldc * (size_t)m);
      const bool stage_out = out_location == AGP_HOST;
      const size_t so_elems = stage_out ? (size_t)ldc + (mode == 0 ? 0 : (size_t)round_up(second_elems, 2)) : 0;
      if ((st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (size_t)cnt * (v_elems + p_elems + so_elems))) != AGP_OK)
        return finish(st);
      double *V = ctx->ws_aux, *prior = V + (size_t)cnt * v_elems, *mean_s = prior + (size_t)cnt * p_elems;
      double *second_s = mean_s + (size_t)cnt * (size_t)ldc;
      const size_t second_stride = (size_t)round_up(second_elems, 2);
      for (long long i = 0; i < cnt; ++i) {
        const int b = first + (int)i;
        PredictBatchItem &it = h_items[(size_t)b];
        std::memset(&it, 0, sizeof(it));
        it.fp = fps[(size_t)b];
        it.X = fits[b]->train.v;
        it.Y = yv[(size_t)b];
        it.alpha = fits[b]->alpha;
        it.V = mode == 0 ? nullptr : V + (size_t)i * v_elems;
        it.prior = mode == 0 ? nullptr : prior + (size_t)i * p_elems;
        it.mean = stage_out ? mean_s + (size_t)i * (size_t)ldc : mean + (size_t)b * (size_t)ldm;
        it.second = mode == 0 ? nullptr : (stage_out ? second_s + (size_t)i * second_stride : second + (size_t)b * (size_t)lds);
      }
      const PredictBatchItem *tab = d_items + first;
      if (hipMemcpyAsync(d_items + first, h_items + first, sizeof(PredictBatchItem) * (size_t)cnt, hipMemcpyHostToDevice, s) != hipSuccess) {
        ctx->last_error = "agp_predict_batch: table upload";
        return finish(AGP_ERR_HIP);
      }
      if (!pinned) (void)hipStreamSynchronize(s);  // (pageable source)
      // per problem where the trees differ: the table-driven kernel on one entry, or the generic program launchers
      auto each = [&](auto &&fast_launch, auto &&generic_launch) -> int {
        for (long long i = 0; i < cnt; ++i) {
          const int b = first + (int)i;
          if (fast[(size_t)b]) {
            fast_launch(tab + i, 1, ops[(size_t)b], fits[b]->train.v.dim);
          } else {
            const DevProgram *dprog = nullptr;
            const int e = device_program(ctx, kernels[b], &dprog);
            if (e != AGP_OK) return e;
            generic_launch(b, h_items[(size_t)b], dprog);
          }
        }
        return AGP_OK;
      };
      if (mode == 0) {
        // mean = cross_cov^T information without the cross covariance (gp.hpp:361-363)
        if (r.uniform) launch_mean_fast_batch(s, tab, cnt, r.op, r.dim, m);
        else
          st = each([&](const PredictBatchItem *t, long long k, int op, int dim) { launch_mean_fast_batch(s, t, k, op, dim, m); },
                    [&](int b, const PredictBatchItem &it, const DevProgram *dprog) {
                      launch_predict_mean(s, dprog, it.X, it.Y, it.alpha, it.mean, &kernels[b]->prog);
                    });
        if (st != AGP_OK) return finish(st);
      } else {
        // cross_cov = cov(train_features, features) (gp.hpp:316,337)
        if (r.uniform) launch_cross_fast_batch(s, tab, cnt, r.op, r.dim, rn, m, ldv);
        else
          st = each([&](const PredictBatchItem *t, long long k, int op, int dim) { launch_cross_fast_batch(s, t, k, op, dim, rn, m, ldv); },
                    [&](int b, const PredictBatchItem &it, const DevProgram *dprog) {
                      launch_gram(s, dprog, it.X, it.Y, false, false, it.V, ldv, nullptr, nullptr, &kernels[b]->prog);
                    });
        if (st != AGP_OK) return finish(st);
        bool chunk_phantoms = false;
        for (long long i = 0; i < cnt && !chunk_phantoms; ++i) chunk_phantoms = !fits[first + (int)i]->phantom.empty();
        if (chunk_phantoms)
          launch_zero_row_ranges(s, static_cast<const char *>(tables.get()) + range_off, count, first, cnt, V, (long long)v_elems, ldv, m);
        // mean = cross_cov^T information (gp.hpp:82-85), then V = L^-1 K* (gp.hpp:96,111)
        hipLaunchKernelGGL((colvec_batch_kernel<false>), dim3((unsigned)m, (unsigned)cnt), dim3(256), 0, s, tab, ldv, rn);
        forward_solve_mat_batched(s, f0->A + (size_t)p0 * (size_t)r.dA, r.dA, rn, f0->lda, f0->invd + (size_t)p0 * (size_t)r.dI, r.dI, V,
                                  (long long)v_elems, m, ldv, false, cnt);
        if (mode == 1) {
          // prior variances (gp.hpp:339-343), then variance = prior - colsum(V o V) (gp.hpp:97-99)
          if (r.uniform) launch_prior_fast_batch(s, tab, cnt, r.op, r.dim, m);
          else
            st = each([&](const PredictBatchItem *t, long long k, int op, int dim) { launch_prior_fast_batch(s, t, k, op, dim, m); },
                      [&](int, const PredictBatchItem &it, const DevProgram *dprog) { launch_gram_diagonal(s, dprog, it.Y, it.prior); });
          if (st != AGP_OK) return finish(st);
          hipLaunchKernelGGL((colvec_batch_kernel<true>), dim3((unsigned)m, (unsigned)cnt), dim3(256), 0, s, tab, ldv, rn);
        } else {
          // prior covariance (gp.hpp:317), lower tiles: one table-driven launch where the trees allow it
          bool gram_done = false;
          if (r.uniform) {
            std::vector<const DevProgram *> hprogs((size_t)cnt);
            std::vector<double *> outs((size_t)cnt);
            for (long long i = 0; i < cnt; ++i) {
              hprogs[(size_t)i] = &kernels[first + i]->prog;
              outs[(size_t)i] = h_items[(size_t)(first + i)].prior;
            }
            gram_done = launch_gram_batch(s, cnt, hprogs.data(), &yv[(size_t)first], outs.data(), ldc, nullptr, nullptr,
                                          static_cast<char *>(tables.get()) + item_bytes + gram_item * (size_t)first,
                                          pinned ? pinned + item_bytes + gram_item * (size_t)first : nullptr);
          }
          for (long long i = 0; i < cnt && !gram_done; ++i) {
            const int b = first + (int)i;
            const DevProgram *dprog = nullptr;
            if ((st = device_program(ctx, kernels[b], &dprog)) != AGP_OK) return finish(st);
            const PredictBatchItem &it = h_items[(size_t)b];
            launch_gram(s, dprog, it.Y, it.Y, true, false, it.prior, ldc, nullptr, nullptr, &kernels[b]->prog);
          }
          // covariance = prior - V^T V on the lower tiles (gp.hpp:111-112), then the full symmetric matrix with ld = m
          launch_gemm_nt_sub_batched(s, prior, ldc, (long long)p_elems, V, ldv, true, (long long)v_elems, V, ldv, true, (long long)v_elems, m,
                                     m, rn, true, cnt);
          const unsigned nb = (unsigned)((m + 31) / 32);
          hipLaunchKernelGGL(symmetrize_pack_batch_kernel, dim3(nb, nb, (unsigned)cnt), dim3(256), 0, s, tab, ldc, m);
        }
      }
      if (stage_out) {
        hipError_t e = hipMemcpy2DAsync(mean + (size_t)first * (size_t)ldm, sizeof(double) * (size_t)ldm, mean_s, sizeof(double) * (size_t)ldc,
                                        sizeof(double) * (size_t)m, (size_t)cnt, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && mode != 0)
          e = hipMemcpy2DAsync(second + (size_t)first * (size_t)lds, sizeof(double) * (size_t)lds, second_s, sizeof(double) * second_stride,
                               sizeof(double) * (size_t)second_elems, (size_t)cnt, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) {
          ctx->last_error = std::string("agp_predict_batch: copy out: ") + hipGetErrorString(e);
          return finish(AGP_ERR_HIP);
        }
      }
    }
  }
  // failed fits: NaN-filled outputs
  for (int b = 0; b < count; ++b) {
    if (fits[b]->fail_status == AGP_OK) continue;
    double *mb = mean + (size_t)b * (size_t)ldm, *sb = mode == 0 ? nullptr : second + (size_t)b * (size_t)lds;
    if (out_location == AGP_HOST) {
      std::fill(mb, mb + m, std::numeric_limits<double>::quiet_NaN());
      if (sb) std::fill(sb, sb + second_elems, std::numeric_limits<double>::quiet_NaN());
    } else {
      hipLaunchKernelGGL(fill_nan_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, mb, m);
      if (sb) hipLaunchKernelGGL(fill_nan_kernel, dim3((unsigned)((second_elems + 255) / 256)), dim3(256), 0, s, sb, second_elems);
    }
  }
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    ctx->last_error = std::string("agp_predict_batch: ") + hipGetErrorString(e);
    return AGP_ERR_HIP;
  }
  return AGP_OK;
}

}  // extern "C"
