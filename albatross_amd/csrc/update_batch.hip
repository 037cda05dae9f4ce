// update_batch.hip — agp_fit_update_batch: FitModel::update (gp.hpp:384-414) for `count` small fits in lock step.
// One agp_fit_update of a few hundred points is six allocations, up to three synchronisations and about fifteen launches
// that are all far too small to fill the chip; a caller who keeps many small models and conditions each on every new
// epoch of observations pays that per model.  Here the grown fits are slices of ONE allocation (agp_fit_slab) and every
// stage of update_api.hip's algebra is ONE launch or launch chain for the whole batch (one grid dimension = problem):
//
//   grow      old factor (lda0 -> lda1), tile images, z, features -> slab b; phantom identity rows     update_grow_kernel
//   cross     B_b^T = cov(new_b, train_b) into rows n_pad.. of slab b (m x n_pad, ld = lda1)            update_cross_fast_kernel
//             phantom columns <- 0 (per-problem ranges: the old fits may differ in them)                 zero_column_ranges_kernel
//   V_b^T     = B_b^T L_b^-T                                                                            right_solve_lt_batched
//   S_b       = cov(new_b, new_b) + diag(y_var_b), lower tiles                                          launch_gram_batch
//   S_b      -= V_b^T V_b                                                                               launch_gemm_nt_sub_batched
//   z_new_b   = y_new_b - V_b^T z_old_b                                                                 update_matvec_kernel
//   L_S L_S^T = S_b, z_new_b <- L_S^-1 z_new_b (fused), log sums, status words                          factor_lower_batched
//   alpha_b   = L_1^-T z_b over the grown factor                                                        backward_solve_vec_batched
//
// The old fits may lie anywhere (handles of several agp_fit_create_batch calls, of agp_fit_create, of earlier updates):
// the grow kernel gathers them through a descriptor table; behind it everything lies at the constant strides of the
// slab.  The covariance launches are table-driven for the radial<Euclidean> [+ noise] trees (gram_fast.h) when every
// problem has one operator and one dimension; otherwise every problem gets the launch agp_fit_update makes.  Either way a
// problem is evaluated by the same code with the same arguments whatever its neighbours are.  Every reduction has a
// fixed order; there are no floating-point atomics.  Synchronisations: one behind the uploads of host-resident inputs,
// and the closing one, where status words, log sums (and the information vectors, when asked for) come down together.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "batch_front.h"
#include "gram_fast.h"

namespace agp {

// One problem of the grow launch.  Sizes that all problems share are kernel arguments.
struct UpdateGrowItem {
  const double *A0;         // old factor, ld = lda0
  const double *invd0, *z0;
  const double *coords0;    // old features (n0 rows)
  const long long *ids0;
  const double *scales0;
  long long lda0, sstride0;
  const double *coords_new;  // the m further features (device)
  const long long *ids_new;
  const double *scales_new;  // m x nsc, column-major
  double *A1, *invd1, *z1, *alpha1;
  double *coords1;           // features of the grown fit (n1 rows; scale columns at stride n1)
  long long *ids1;
  double *scales1;
  double *logsum;
  int *flags;
  int dim, nsc;
};

// One problem of the table-driven cross covariance
struct UpdateCrossItem {
  FastParams fp;
  FeatView Xnew, Xold;  // views of the grown fit's features: rows n_pad.. and rows 0 .. n_pad
  double *X;            // rows n_pad.. of slab b
  int *flags;
};

// blockIdx.y = problem.  Columns of the factor are dealt to the workgroups round-robin; a column moves as 16-byte pairs
// of rows (lda0, lda1 and the first row of a column's range are even, the slabs 16-byte aligned).  Only the tiles the
// factorisation ever wrote are copied: rows from the 128-row block of the column's diagonal element on.  Rows n0 .. n_pad
// are the phantom rows e_i^T.  The small arrays (tile images, z, features, status words) follow, spread over all threads
// of the problem.
__global__ __launch_bounds__(256) void update_grow_kernel(const UpdateGrowItem *__restrict__ items, long long n0, long long n_pad,
                                                         long long m, long long lda1, long long img_words) {
  const UpdateGrowItem it = items[blockIdx.y];
  const long long n1 = n_pad + m;
  const bool pairs = ((reinterpret_cast<uintptr_t>(it.A0) & 15) == 0) && ((it.lda0 & 1) == 0);
  for (long long c = blockIdx.x; c < n_pad; c += gridDim.x) {
    const long long r0 = c / NB * NB;
    const double *src = it.A0 + c * it.lda0;
    double *dst = it.A1 + c * lda1;
    for (long long r = r0 + 2 * (long long)threadIdx.x; r < n_pad; r += 2 * 256) {
      double va, vb;
      if (c < n0 && r + 1 < n0 && pairs) {
        const double2 v = *reinterpret_cast<const double2 *>(src + r);
        va = v.x; vb = v.y;
      } else {
        va = (c < n0 && r < n0) ? src[r] : (r == c ? 1. : 0.);
        vb = (c < n0 && r + 1 < n0) ? src[r + 1] : (r + 1 == c ? 1. : 0.);
      }
      *reinterpret_cast<double2 *>(dst + r) = make_double2(va, vb);  // (n_pad is even: r + 1 < n_pad)
    }
  }
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  if ((reinterpret_cast<uintptr_t>(it.invd0) & 15) == 0) {
    for (long long i = t0; i < img_words / 2; i += step)  // (a tile image is an even number of doubles)
      reinterpret_cast<double2 *>(it.invd1)[i] = reinterpret_cast<const double2 *>(it.invd0)[i];
  } else {
    for (long long i = t0; i < img_words; i += step) it.invd1[i] = it.invd0[i];
  }
  for (long long i = t0; i < n1; i += step) {
    const double v = i < n0 ? it.z0[i] : 0.;
    it.z1[i] = v;
    it.alpha1[i] = v;
  }
  // train_features = concatenate(fit.train_features, features) (gp.hpp:387); a phantom row carries a copy of the first
  // new feature and an id no caller's (non-negative) id equals
  const int dim = it.dim;
  for (long long i = t0; i < n1 * dim; i += step) {
    const long long row = i / dim, d = i - row * dim;
    it.coords1[i] = row < n0 ? it.coords0[i] : it.coords_new[(row < n_pad ? 0 : row - n_pad) * dim + d];
  }
  if (it.ids1)
    for (long long i = t0; i < n1; i += step) it.ids1[i] = i < n0 ? it.ids0[i] : (i < n_pad ? -2 - (i - n0) : it.ids_new[i - n_pad]);
  for (int k = 0; k < it.nsc; ++k)
    for (long long i = t0; i < n1; i += step)
      it.scales1[(long long)k * n1 + i] =
          i < n0 ? it.scales0[(long long)k * it.sstride0 + i] : it.scales_new[(long long)k * m + (i < n_pad ? 0 : i - n_pad)];
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) *it.logsum = 0.;
    if (threadIdx.x < 4) it.flags[threadIdx.x] = 0;
  }
}

// B_b^T into rows n_pad.. of slab b: blockIdx = (row tile of new points, column tile of old points, problem)
template <int DIMP, int OP>
__global__ __launch_bounds__(GRAM_THREADS) void update_cross_fast_kernel(const UpdateCrossItem *__restrict__ items, long long ld) {
  const UpdateCrossItem it = items[blockIdx.z];
  if ((long long)blockIdx.x * TM >= it.Xnew.n || (long long)blockIdx.y * TN >= it.Xold.n) return;
  gram_fast_body<DIMP, OP>(it.fp, it.Xnew, it.Xold, 0, it.X, ld, nullptr, it.flags, 0, 0, blockIdx.x, blockIdx.y);
}

// z_b[n_pad + i] = y_b[i] - sum_j X_b[i, j] z_b[j], j < n_pad: blockIdx = (128 rows, problem).  Lane l of every wave owns
// the rows 2 l, 2 l + 1 (one 16-byte load per column: a wave reads 1 KiB of a column), wave w the columns j = w (mod 4);
// the four partial sums are added as (0 + 1) + (2 + 3).
__global__ __launch_bounds__(256) void update_matvec_kernel(const double *__restrict__ X, long long stride_X, long long ld, long long m,
                                                           long long n_pad, double *z, long long stride_z,
                                                           const double *__restrict__ y, long long stride_y) {
  __shared__ double red[4][128];
  const double *Xb = X + (long long)blockIdx.y * stride_X;
  double *zb = z + (long long)blockIdx.y * stride_z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 128 + 2 * lane;
  double a0 = 0., a1 = 0.;
  if (r + 1 < m) {
    for (long long j = wave; j < n_pad; j += 4) {
      const double2 v = *reinterpret_cast<const double2 *>(Xb + j * ld + r);
      const double zj = zb[j];
      a0 += v.x * zj;
      a1 += v.y * zj;
    }
  } else if (r < m) {
    for (long long j = wave; j < n_pad; j += 4) a0 += Xb[j * ld + r] * zb[j];
  }
  red[wave][2 * lane] = a0;
  red[wave][2 * lane + 1] = a1;
  __syncthreads();
  if (threadIdx.x < 128) {
    const long long i = (long long)blockIdx.x * 128 + threadIdx.x;
    if (i < m) {
      const int t = threadIdx.x;
      zb[n_pad + i] = y[(long long)blockIdx.y * stride_y + i] - ((red[0][t] + red[1][t]) + (red[2][t] + red[3][t]));
    }
  }
}

// alpha_b <- z_b (n values per problem, both at stride_v)
__global__ __launch_bounds__(256) void update_copy_vectors_kernel(const double *__restrict__ z, double *alpha, long long stride_v,
                                                                 long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) alpha[(long long)blockIdx.y * stride_v + i] = z[(long long)blockIdx.y * stride_v + i];
}

static void launch_update_cross_fast(hipStream_t s, const UpdateCrossItem *tab, long long count, int op, int dim, long long m,
                                     long long n_pad, long long ld) {
  dim3 grid((unsigned)((m + TM - 1) / TM), (unsigned)((n_pad + TN - 1) / TN), (unsigned)count), block(GRAM_THREADS);
#define AGP_UB_CROSS(D, O) hipLaunchKernelGGL((update_cross_fast_kernel<D, O>), grid, block, 0, s, tab, ld)
#define AGP_UB_OPS(D)                                                                  \
  switch (op) {                                                                        \
  case AGP_OP_SQUARED_EXPONENTIAL: AGP_UB_CROSS(D, AGP_OP_SQUARED_EXPONENTIAL); break;  \
  case AGP_OP_EXPONENTIAL: AGP_UB_CROSS(D, AGP_OP_EXPONENTIAL); break;                  \
  case AGP_OP_MATERN32: AGP_UB_CROSS(D, AGP_OP_MATERN32); break;                        \
  default: AGP_UB_CROSS(D, AGP_OP_MATERN52); break;                                     \
  }
  if (dim == 1) { AGP_UB_OPS(1) }
  else if (dim == 2) { AGP_UB_OPS(2) }
  else { AGP_UB_OPS(3) }
#undef AGP_UB_OPS
#undef AGP_UB_CROSS
}

// problem's training features inside the slab of its batch: coordinates, equality ids, scale columns (n1 rows)
static FeatView carve_grown_features(WsLayout &ws, long long n1, int dim, bool ids, int nsc) {
  FeatView v;
  v.n = n1; v.dim = dim; v.nsc = nsc; v.meas = 0; v.sstride = 0;
  v.coords = ws.take<double>((size_t)n1 * (size_t)dim);
  v.ids = ids ? ws.take<long long>((size_t)n1) : nullptr;
  v.scales = nsc > 0 ? ws.take<double>((size_t)n1 * (size_t)nsc) : nullptr;
  return v;
}

}  // namespace agp

using namespace agp;

extern "C" {

int agp_fit_update_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_fit *const *olds,
                         const agp_features *const *x_new, const double *y_new, int64_t ldy, const double *y_var_new, int64_t ldv,
                         agp_fit **out, double *information, int64_t ldi, double *log_det, int *status) {
  if (!c || !olds || !y_new || !out || !status) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  // ---- every check before anything is written or launched ----
  long long m = 0;
  int st = check_batch_problems(count, kernels, x_new, ldy, y_var_new, ldv, &m);
  if (st != AGP_OK) return st;
  bool no_z = false;
  for (int b = 0; b < count; ++b) {
    const agp_fit *f = olds[b], *f0 = olds[0];
    if (!f || f->ctx != c || f->mixed || !f->A || !f->alpha || !f->invd || f->failed_pivot >= 0 || f->fail_status != AGP_OK)
      return AGP_ERR_INVALID_ARGUMENT;
    if (!f->z) { no_z = true; continue; }  // (agp_factor_create, replicated fits)
    const FeatView &ov = f->train.v;
    if (!ov.coords || ov.n != f->n) return AGP_ERR_INVALID_ARGUMENT;
    if (f->n != f0->n) return AGP_ERR_INVALID_ARGUMENT;  // (one padded size; real rows and phantom ranges may differ)
    if (x_new[b]->dim != ov.dim || x_new[b]->n_scale_columns != ov.nsc) return AGP_ERR_INVALID_ARGUMENT;
    if ((ov.ids != nullptr) != (x_new[b]->eq_id != nullptr)) return AGP_ERR_INVALID_ARGUMENT;  // equality by id on one side only
  }
  if (no_z) return AGP_ERR_UNSUPPORTED;
  const long long n0 = olds[0]->n, n_pad = round_up(n0, NB), n1 = n_pad + m;
  if (information)
    for (int b = 0; b < count; ++b)
      if (ldi < fit_real_rows(olds[b]) + m) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const BatchGeometry g = batch_geometry(n1, count);
  const long long lda = g.lda, nblk0 = (n0 + NB - 1) / NB, mp2 = round_up(m, 2);
  const int loc = x_new[0]->location;
  const bool prof = ctx->profiling;

  // ---- the slab the grown fits keep: factors | tile images | information | z | log sums | status words | features ----
  WsLayout size;
  carve_update_batch(size, g);
  for (int b = 0; b < count; ++b) carve_grown_features(size, n1, x_new[b]->dim, x_new[b]->eq_id != nullptr, x_new[b]->n_scale_columns);
  const size_t bytes = size.bytes();
  DevMem<double> base;
  base.adopt(static_cast<double *>(ctx->pool_batch.take(bytes)));
  if (!base) AGP_HIP_CHECK(ctx, base.alloc_plain(bytes));
  WsLayout ws(base.get());
  const UpdateBatchRegions r = carve_update_batch(ws, g);
  // ---- the scratch of the call: targets, variances, staged host features, the three descriptor tables ----
  size_t stage_words = 0;  // host-resident new features go through one staging region
  if (loc == AGP_HOST)
    for (int b = 0; b < count; ++b)
      stage_words += (size_t)m * ((size_t)x_new[b]->dim + (x_new[b]->eq_id ? 1 : 0) + (size_t)x_new[b]->n_scale_columns);
  // the phantom columns of every problem's cross covariance: those of its old fit and the pad to n_pad (the table follows
  // the Gram table in its region)
  RangeTable phantoms;
  for (int b = 0; b < count; ++b) {
    phantoms.begin_problem();
    for (const auto &ph : olds[b]->phantom) phantoms.add(ph.first, ph.second);
    phantoms.add(n0, n_pad);
  }
  const size_t range_off = phantoms.any() ? (gram_batch_table_bytes(count) + 15) / 16 * 16 : gram_batch_table_bytes(count);
  const size_t grow_bytes = sizeof(UpdateGrowItem) * (size_t)count, cross_bytes = sizeof(UpdateCrossItem) * (size_t)count,
               gram_bytes = range_off + (phantoms.any() ? phantoms.bytes() : 0);
  WsLayout tsize;
  carve_update_batch_scratch(tsize, g, mp2, y_var_new != nullptr, stage_words, grow_bytes, cross_bytes, gram_bytes);
  DevMem<void> scratch;
  if (scratch.alloc_cached(tsize.bytes()) != 0) {
    (void)hipGetLastError();
    ctx->last_error = "agp_fit_update_batch: scratch";
    return AGP_ERR_HIP;
  }
  WsLayout tws(scratch.get());
  const UpdateBatchScratch t =
      carve_update_batch_scratch(tws, g, mp2, y_var_new != nullptr, stage_words, grow_bytes, cross_bytes, gram_bytes);
  const size_t table_off = (size_t)(static_cast<char *>(t.grow_table) - static_cast<char *>(scratch.get()));
  const size_t cross_off = (size_t)(static_cast<char *>(t.cross_table) - static_cast<char *>(t.grow_table));
  const size_t gram_off = (size_t)(static_cast<char *>(t.gram_table) - static_cast<char *>(t.grow_table));
  const size_t tables_bytes = tsize.bytes() - table_off;  // (the tables are the tail of the scratch, laid out alike in the pinned stage)
  char *pinned = static_cast<char *>(host_stage(ctx, tables_bytes));
  std::vector<char> pageable;
  if (!pinned) pageable.resize(tables_bytes);
  char *h_tables = pinned ? pinned : pageable.data();

  std::vector<agp_fit *> fits((size_t)count, nullptr);
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(s);
    for (auto *f : fits)
      if (f) delete f;
    base.reset();
    return code;
  };
#define UPB_CHECK(expr)                                                      \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);   \
      return fail(AGP_ERR_HIP);                                              \
    }                                                                        \
  } while (0)
  if (prof) UPB_CHECK(hipEventRecord(ctx->stage_ev[0], s));
  if ((st = upload_problem_columns(ctx, y_new, ldy, m, count, loc, t.ynew, mp2)) != AGP_OK) return fail(st);
  if (y_var_new && (st = upload_problem_columns(ctx, y_var_new, ldv, m, count, loc, t.yvar, mp2)) != AGP_OK) return fail(st);

  // ---- the descriptor tables; every tree is matched against the fast-path shapes once ----
  UpdateGrowItem *h_grow = reinterpret_cast<UpdateGrowItem *>(h_tables);
  UpdateCrossItem *h_cross = reinterpret_cast<UpdateCrossItem *>(h_tables + cross_off);
  std::vector<FeatView> vnew((size_t)count), vold((size_t)count);
  std::vector<const DevProgram *> hprogs((size_t)count);
  std::vector<double *> S((size_t)count);
  std::vector<const double *> diag((size_t)count, nullptr);
  std::vector<int *> nanf((size_t)count);
  bool uniform = true;
  int op0 = 0, dim0 = 0;
  double *cur = t.xstage;
  for (int b = 0; b < count; ++b) {
    agp_fit *fit = new (std::nothrow) agp_fit();
    if (!fit) return fail(AGP_ERR_INVALID_ARGUMENT);
    fits[(size_t)b] = fit;
    const agp_fit *old = olds[b];
    const agp_features *f = x_new[b];
    const FeatView &ov = old->train.v;
    const int dim = ov.dim, nsc = ov.nsc;
    const FeatView v = carve_grown_features(ws, n1, dim, ov.ids != nullptr, nsc);
    fit->train.v = v;  // (not owned: DeviceFeatures::release has nothing to free)
    UpdateGrowItem &gi = h_grow[b];
    std::memset(&gi, 0, sizeof(gi));
    gi.A0 = old->A; gi.invd0 = old->invd; gi.z0 = old->z; gi.lda0 = old->lda;
    gi.coords0 = ov.coords; gi.ids0 = ov.ids; gi.scales0 = ov.scales; gi.sstride0 = scale_stride(ov);
    gi.coords_new = f->coords;
    gi.ids_new = reinterpret_cast<const long long *>(f->eq_id);
    gi.scales_new = nsc > 0 ? f->scales : nullptr;
    if (loc == AGP_HOST) {
      auto up = [&](const void *src, size_t words) -> const double * {
        double *dst = cur;
        cur += words;
        if (hipMemcpyAsync(dst, src, sizeof(double) * words, hipMemcpyHostToDevice, s) != hipSuccess) st = AGP_ERR_HIP;
        return dst;
      };
      gi.coords_new = up(f->coords, (size_t)m * (size_t)dim);
      if (f->eq_id) gi.ids_new = reinterpret_cast<const long long *>(up(f->eq_id, (size_t)m));
      if (nsc > 0) gi.scales_new = up(f->scales, (size_t)m * (size_t)nsc);
    }
    gi.A1 = r.A + (size_t)b * (size_t)g.stride_A;
    gi.invd1 = r.invd + (size_t)b * (size_t)g.stride_I;
    gi.z1 = r.z + (size_t)b * (size_t)g.np2;
    gi.alpha1 = r.alpha + (size_t)b * (size_t)g.np2;
    gi.coords1 = const_cast<double *>(v.coords);
    gi.ids1 = const_cast<long long *>(v.ids);
    gi.scales1 = const_cast<double *>(v.scales);
    gi.logsum = r.logsum + b;
    gi.flags = r.flags + 4 * (size_t)b;
    gi.dim = dim; gi.nsc = nsc;
    // cross = k(train_features, features) and prior = k(features, features) on PLAIN features (gp.hpp:388-396)
    FeatView vn = v, vo = v;
    vn.coords = v.coords + n_pad * dim; vn.ids = v.ids ? v.ids + n_pad : nullptr; vn.scales = v.scales ? v.scales + n_pad : nullptr;
    vn.n = m; vn.sstride = n1;
    vo.n = n_pad; vo.sstride = n1;
    vnew[(size_t)b] = vn;
    vold[(size_t)b] = vo;
    UpdateCrossItem &ci = h_cross[b];
    std::memset(&ci, 0, sizeof(ci));
    int op = 0;
    const bool fast = dim <= 3 && gram_match_fast(kernels[b]->prog, &ci.fp, &op);
    if (b == 0) { op0 = op; dim0 = dim; }
    if (!fast || op != op0 || dim != dim0) uniform = false;
    ci.Xnew = vn; ci.Xold = vo;
    ci.X = gi.A1 + n_pad;
    ci.flags = gi.flags;
    hprogs[(size_t)b] = &kernels[b]->prog;
    S[(size_t)b] = gi.A1 + n_pad * (lda + 1);
    if (y_var_new) diag[(size_t)b] = t.yvar + (size_t)b * (size_t)mp2;
    nanf[(size_t)b] = gi.flags;
  }
  if (st != AGP_OK) {
    ctx->last_error = "agp_fit_update_batch: feature upload";
    return fail(st);
  }
  UPB_CHECK(hipMemcpyAsync(t.grow_table, h_tables, gram_off, hipMemcpyHostToDevice, s));  // grow and cross tables
  if (phantoms.any()) {
    phantoms.write(h_tables + gram_off + range_off);
    UPB_CHECK(hipMemcpyAsync(static_cast<char *>(t.gram_table) + range_off, h_tables + gram_off + range_off, phantoms.bytes(),
                             hipMemcpyHostToDevice, s));
  }
  if (loc == AGP_HOST || !pinned) UPB_CHECK(hipStreamSynchronize(s));  // (pageable sources: the one wait for host-resident inputs)

  // ---- grow: old factor, tile images, z and features into the slab, phantom rows, zeroed status ----
  hipLaunchKernelGGL(update_grow_kernel, dim3((unsigned)(n_pad < 1024 ? n_pad : 1024), (unsigned)count), dim3(256), 0, s,
                     static_cast<const UpdateGrowItem *>(t.grow_table), n0, n_pad, m, lda, nblk0 * (long long)(36 * MB * MB));
  // ---- cross covariance, written transposed where V^T belongs: rows n_pad.., columns 0 .. n_pad ----
  double *X = r.A + n_pad;  // m x n_pad, ld = lda, of problem 0
  if (uniform) {
    launch_update_cross_fast(s, static_cast<const UpdateCrossItem *>(t.cross_table), count, op0, dim0, m, n_pad, lda);
  } else {
    for (int b = 0; b < count; ++b) {
      const DevProgram *dprog = nullptr;
      if ((st = device_program(ctx, kernels[b], &dprog)) != AGP_OK) return fail(st);
      launch_gram(s, dprog, vnew[(size_t)b], vold[(size_t)b], false, false, X + (size_t)b * (size_t)g.stride_A, lda, nullptr,
                  nanf[(size_t)b], &kernels[b]->prog);
    }
  }
  // (the covariance with a phantom row is zero by definition)
  if (phantoms.any()) launch_zero_column_ranges(s, static_cast<const char *>(t.gram_table) + range_off, count, 0, count, X, g.stride_A, lda, m);
  // ---- X <- X L^-T (the block row V^T of the grown factor; block_symmetric.hpp:51) ----
  right_solve_lt_batched(s, r.A, g.stride_A, n_pad, lda, r.invd, g.stride_I, X, g.stride_A, m, lda, count);
  if (prof) UPB_CHECK(hipEventRecord(ctx->stage_ev[1], s));
  // ---- S = prior(features) + targets.covariance - V^T V (gp.hpp:389-392 folded into one Schur complement) ----
  if (!(uniform && launch_gram_batch(s, count, hprogs.data(), vnew.data(), S.data(), lda, diag.data(), nanf.data(), t.gram_table,
                                     pinned ? pinned + gram_off : nullptr))) {
    for (int b = 0; b < count; ++b) {
      const DevProgram *dprog = nullptr;
      if ((st = device_program(ctx, kernels[b], &dprog)) != AGP_OK) return fail(st);
      launch_gram(s, dprog, vnew[(size_t)b], vnew[(size_t)b], true, true, S[(size_t)b], lda, diag[(size_t)b], nanf[(size_t)b],
                  &kernels[b]->prog);
    }
  }
  launch_gemm_nt_sub_batched(s, S[0], lda, g.stride_A, X, lda, false, g.stride_A, X, lda, false, g.stride_A, m, m, n_pad, true, count);
  // ---- forward substitution of the new targets: y_new - V^T z_old, then through L_S (fused into its factorisation) ----
  hipLaunchKernelGGL(update_matvec_kernel, dim3((unsigned)((m + 127) / 128), (unsigned)count), dim3(256), 0, s, X, g.stride_A, lda, m,
                     n_pad, r.z, g.np2, t.ynew, mp2);
  // ---- LL^T of S in place (the sub-matrix is addressed as a matrix of its own: its 128-blocks start at n_pad) ----
  factor_lower_batched(s, S[0], g.stride_A, m, lda, r.invd + (n_pad / NB) * (long long)(36 * MB * MB), g.stride_I, r.z + n_pad, g.np2,
                       count, r.flags, r.logsum, 4);
  if (prof) UPB_CHECK(hipEventRecord(ctx->stage_ev[2], s));
  // ---- information = L^-T z over the whole grown factor; a failed problem only spoils its own vector ----
  hipLaunchKernelGGL(update_copy_vectors_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)count), dim3(256), 0, s, r.z + n_pad,
                     r.alpha + n_pad, g.np2, m);
  backward_solve_vec_batched(s, r.A, g.stride_A, n1, lda, r.invd, g.stride_I, r.alpha, g.np2, count);
  if (prof) UPB_CHECK(hipEventRecord(ctx->stage_ev[3], s));
  // ---- the closing synchronisation: log sums, status words and (when asked for) the information vectors together ----
  std::vector<double> h_status(3 * (size_t)g.cp2);  // [logsum | flags]
  std::vector<double> h_alpha(information ? (size_t)count * (size_t)g.np2 : 0);
  UPB_CHECK(hipMemcpyAsync(h_status.data(), r.logsum, sizeof(double) * h_status.size(), hipMemcpyDeviceToHost, s));
  if (information) UPB_CHECK(hipMemcpyAsync(h_alpha.data(), r.alpha, sizeof(double) * h_alpha.size(), hipMemcpyDeviceToHost, s));
  UPB_CHECK(hipStreamSynchronize(s));
  UPB_CHECK(hipGetLastError());
#undef UPB_CHECK
  if (prof) {
    for (int i = 0; i < 3; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ctx->stage_ev[i], ctx->stage_ev[i + 1]) == hipSuccess) ctx->stage_ms[i] = ms;
    }
  }
  const int *h_flags = reinterpret_cast<const int *>(h_status.data() + g.cp2);
  agp_fit_slab *slab = new (std::nothrow) agp_fit_slab();
  if (!slab) return fail(AGP_ERR_INVALID_ARGUMENT);
  slab->base = std::move(base);
  slab->bytes = bytes;
  slab->refs = count;
  for (int b = 0; b < count; ++b) {
    agp_fit *fit = fits[(size_t)b];
    const agp_fit *old = olds[b];
    fit->ctx = ctx;
    fit->slab = slab;
    fit->device = ctx->device;
    fit->n = n1;
    fit->lda = lda;
    fit->A_bytes = sizeof(double) * (size_t)g.stride_A;
    fit->A = r.A + (size_t)b * (size_t)g.stride_A;
    fit->invd = r.invd + (size_t)b * (size_t)g.stride_I;
    fit->alpha = r.alpha + (size_t)b * (size_t)g.np2;
    fit->z = r.z + (size_t)b * (size_t)g.np2;
    fit->phantom = old->phantom;
    if (n_pad > n0) fit->phantom.emplace_back(n0, n_pad);
    const long long real0 = fit_real_rows(old);
    fit->n_real = real0 + m;
    const int *fl = h_flags + 4 * (size_t)b;
    fit->failed_pivot = (!fl[0] && fl[1]) ? real0 + (int64_t)fl[1] - 1 : -1;  // real rows of the old fit + local pivot
    fit->log_det = old->log_det + 2. * h_status[(size_t)b];
    status[b] = fl[0] ? AGP_ERR_NAN_INPUT : (fl[1] ? AGP_ERR_NOT_POSITIVE_DEFINITE : AGP_OK);
    fit->fail_status = status[b];
    if (status[b] == AGP_OK) {
      if (information) {  // the real rows: the old observations first, then the new ones
        double *dst = information + (size_t)b * (size_t)ldi;
        const double *src = h_alpha.data() + (size_t)b * (size_t)g.np2;
        long long pad = 0;
        for (const auto &ph : fit->phantom) {
          dst = std::copy(src + pad, src + ph.first, dst);
          pad = ph.second;
        }
        std::copy(src + pad, src + n1, dst);
      }
      if (log_det) log_det[b] = fit->log_det;
    }
    out[b] = fit;
  }
  return AGP_OK;
}

}  // extern "C"
