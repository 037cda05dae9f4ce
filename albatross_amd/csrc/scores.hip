// scores.hip — scoring a joint prediction against held-out truth on the device (the reference's
// evaluation/prediction_metrics.hpp): counter-based standard normals, draws S = mean 1^T + L Z from a resident LL^T
// factor on the fp64 MFMA, the Monte-Carlo energy score, the variogram score and the elementwise CRPS.
//
// Every reduction here has a fixed order (per-thread strided sums, a fixed LDS tree per workgroup, a fixed tree over the
// workgroups' partials) and there are no floating-point atomics: two identical calls give identical bits.
#include <cmath>
#include <new>

#include "api_internal.h"
#include "gemm_tiles.h"

namespace agp {
namespace {

// ---- standard normals -------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): key = the two halves of the seed,
// counter = (row, column, 0, 0).  One normal per counter, so entry (row, column) depends on nothing but the seed.
__device__ __forceinline__ double standard_normal(unsigned k0, unsigned k1, unsigned row, unsigned col) {
  unsigned c0 = row, c1 = col, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  // 53 random bits each, centred in their cell: u in (0, 1), never 0 or 1
  const double u1 = ((double)((((unsigned long long)c1 << 32) | c0) >> 11) + 0.5) * 0x1p-53;
  const double u2 = ((double)((((unsigned long long)c3 << 32) | c2) >> 11) + 0.5) * 0x1p-53;
  return sqrt(-2. * log(u1)) * cos((2. * M_PI) * u2);  // Box-Muller, the cosine branch only
}

__global__ void standard_normal_kernel(unsigned k0, unsigned k1, long long m, long long first_column, long long n_columns,
                                       double *__restrict__ out, long long ldo) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  for (long long j = blockIdx.y; j < n_columns; j += gridDim.y)
    out[i + j * ldo] = standard_normal(k0, k1, (unsigned)i, (unsigned)(first_column + j));
}

// the Rademacher probes of agp_iterative_nll_gradient: +1 where the normal of the same (seed, row, column) is >= 0, else -1
__global__ void rademacher_kernel(unsigned k0, unsigned k1, long long m, long long first_column, long long n_columns,
                                  double *__restrict__ out, long long ldo) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  for (long long j = blockIdx.y; j < n_columns; j += gridDim.y)
    out[i + j * ldo] = standard_normal(k0, k1, (unsigned)i, (unsigned)(first_column + j)) >= 0. ? 1. : -1.;
}

// ---- S = mean 1^T + L Z -------------------------------------------------------------------------------------------------
// One 64 x 64 tile of S per workgroup of 256 threads (four waves, 32 x 32 each: the operand layout, the LDS pitch and the
// lane maps of gemm64_body, gemm_tiles.h).  L is lower triangular: the K loop of row tile bi ends at that tile's diagonal
// block, and the four chunks of the diagonal block are masked to k <= row while they are staged - whatever the factor
// buffer holds above the diagonal (the input's upper triangle, as the factorisation leaves it) never reaches a product.
struct DrawArgs {
  const double *L;
  long long ldl, m;
  const double *Z;  // m x n, element (k, col) at Z[k + col * ldz]
  long long ldz, n;
  const double *mean;  // or nullptr: S = L Z
  double *S;
  long long lds_;
};

__global__ __launch_bounds__(GEMM_THREADS) void draw_kernel(DrawArgs g) {
  __shared__ double lds[2 * 2 * GK * SLD];
  // the deepest row tiles first: their K loops are the longest
  const long long bi = (long long)gridDim.x - 1 - blockIdx.x, bj = blockIdx.y;
  const long long i0 = bi * ST, j0 = bj * ST;
  const long long K = (i0 + ST < g.m) ? i0 + ST : g.m;  // columns of L this row tile can see
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int ln = lane & 15, lg = lane >> 4;
  const bool l_vec = ((reinterpret_cast<uintptr_t>(g.L) & 15) == 0) && ((g.ldl & 1) == 0);
  const bool z_vec = ((reinterpret_cast<uintptr_t>(g.Z) & 15) == 0) && ((g.ldz & 1) == 0);
  const long long nk = (K + GK - 1) / GK;

  auto load_l = [&](long long kc, double (&r)[4]) {
    const long long k0 = kc * GK;
    load_chunk64(g.L, g.ldl, i0, g.m, k0, K, l_vec, r);
    if (k0 + GK > i0 + 1) {  // a chunk of the diagonal block: keep k <= row
      const long long k = k0 + (threadIdx.x >> 4), row = i0 + (threadIdx.x & 15) * 2;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k > row + 32 * (q >> 1) + (q & 1)) r[q] = 0.;
    }
  };
  auto load_z = [&](long long kc, double (&r)[4]) { load_chunk64_kmajor(g.Z, g.ldz, j0, g.n, kc * GK, K, z_vec, r); };

  v4d acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4zero();

  double ra[4], rb[4];
  load_l(0, ra);
  load_z(0, rb);
  store_chunk64<false>(lds, ra);
  store_chunk64_kmajor<false>(lds + GK * SLD, rb);
  __syncthreads();
  for (long long kc = 0; kc < nk; ++kc) {
    const int cur = (int)(kc & 1);
    const double *As = lds + cur * (2 * GK * SLD);
    const double *Bs = As + GK * SLD;
    const bool more = kc + 1 < nk;
    if (more) {
      load_l(kc + 1, ra);
      load_z(kc + 1, rb);
    }
#pragma unroll
    for (int s = 0; s < GK / 4; ++s) {
      const int krow = (4 * s + lg) * SLD;
      double fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fa[t] = Bs[krow + 32 * wc + 16 * t + ln];  // MFMA A operand: the columns of S (draws)
        fb[t] = As[krow + 32 * wr + 16 * t + ln];  // MFMA B operand: the rows of S
      }
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) acc[tj][ti] = mfma16(fa[tj], fb[ti], acc[tj][ti]);
    }
    if (more) {  // the other stage: nobody reads it before the barrier below
      double *An = lds + (cur ^ 1) * (2 * GK * SLD);
      store_chunk64<false>(An, ra);
      store_chunk64_kmajor<false>(An + GK * SLD, rb);
    }
    __syncthreads();
  }
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const long long row = i0 + 32 * wr + 16 * ti + ln;
      if (row >= g.m) continue;
      const double mu = g.mean ? g.mean[row] : 0.;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long col = j0 + 32 * wc + 16 * tj + lg + 4 * r;
        if (col < g.n) g.S[row + col * g.lds_] = mu + acc[tj][ti][r];
      }
    }
}

// ---- fixed-order reductions ----------------------------------------------------------------------------------------------
constexpr int RED_THREADS = 256;

// sum of the workgroup's values, the same tree whatever the values are; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double *sh) {
  __syncthreads();  // (sh may still be read from the previous call)
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int w = RED_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// Energy score, per pair of matched columns j (prediction_metrics.hpp:221-256, :258-277): V = L Z without the mean,
// va = V[:, j] of set A, vb = V[:, k + j] of set B.  The samples are mean + v and - the antithetic half, never stored -
// mean - v; cols[j] = the four weighted error norms and the paired distance || w o (va - vb) ||, which is the same number
// for the antithetic pair (mean - va) - (mean - vb).
__global__ __launch_bounds__(RED_THREADS) void energy_columns_kernel(const double *__restrict__ V, long long ldv, long long m,
                                                                     long long k, const double *__restrict__ mean,
                                                                     const double *__restrict__ truth,
                                                                     const double *__restrict__ weights, double *__restrict__ cols) {
  __shared__ double sh[RED_THREADS];
  const long long j = blockIdx.x;
  const double *va = V + j * ldv, *vb = V + (k + j) * ldv;
  double s[5] = {0., 0., 0., 0., 0.};
  for (long long i = threadIdx.x; i < m; i += RED_THREADS) {
    const double w = weights ? weights[i] : 1., d = mean[i] - truth[i], a = va[i], b = vb[i];
    const double ap = d + a, am = d - a, bp = d + b, bm = d - b, pr = w * (a - b);
    s[0] += w * (ap * ap);  // the weights enter unsquared here ...
    s[1] += w * (am * am);
    s[2] += w * (bp * bp);
    s[3] += w * (bm * bm);
    s[4] += pr * pr;        // ... and squared here, as in the reference
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const double t = block_sum(s[q], sh);
    if (threadIdx.x == 0) cols[5 * j + q] = sqrt(t);
  }
}

// out[0] = sum of the error norms of set A (both halves), out[1] = of set B, out[2] = sum of the paired distances
__global__ __launch_bounds__(RED_THREADS) void energy_finish_kernel(const double *__restrict__ cols, long long k,
                                                                    double *__restrict__ out) {
  __shared__ double sh[RED_THREADS];
  double s[3] = {0., 0., 0.};
  for (long long j = threadIdx.x; j < k; j += RED_THREADS) {
    s[0] += cols[5 * j] + cols[5 * j + 1];
    s[1] += cols[5 * j + 2] + cols[5 * j + 3];
    s[2] += cols[5 * j + 4];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double t = block_sum(s[q], sh);
    if (threadIdx.x == 0) out[q] = t;
  }
}

__global__ __launch_bounds__(RED_THREADS) void sum_partials_kernel(const double *__restrict__ partial, long long count,
                                                                   double *__restrict__ out) {
  __shared__ double sh[RED_THREADS];
  double s = 0.;
  for (long long t = threadIdx.x; t < count; t += RED_THREADS) s += partial[t];
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = t;
}

// ---- variogram score -------------------------------------------------------------------------------------------------------
// E|N(mu, sigma^2)| (prediction_metrics.hpp:287-301; Winkelbauer, arXiv:1209.4340, eq. 17)
__device__ __forceinline__ double expected_abs_normal_1(double mu, double sigma) {
  if (!isfinite(mu) || !isfinite(sigma)) return nan("");
  if (sigma <= 0.) return fabs(mu);
  const double normalized = fabs(mu) / fmax(1.0e-16, sigma);
  return sigma * sqrt(2. / M_PI) * exp(-0.5 * normalized * normalized) + fabs(mu) * erf(normalized / sqrt(2.));
}

// One 64 x 64 tile of pairs (i, j), i < j, per workgroup: tile t of the upper triangle in column-major tile order.  Thread
// (t & 63, t >> 6) walks the pairs (i0 + (t & 63), j0 + (t >> 6) + 4 s), s = 0 .. 15: the loads of c and w run along a
// column, and j is uniform over a wave.  ORDER2: p = 2.
template <bool ORDER2>
__global__ __launch_bounds__(RED_THREADS) void variogram_kernel(const double *__restrict__ mean, const double *__restrict__ c,
                                                                long long ldc, long long m, const double *__restrict__ truth,
                                                                const double *__restrict__ truth_var,
                                                                const double *__restrict__ w, long long ldw,
                                                                double *__restrict__ partial) {
  __shared__ double sh[RED_THREADS];
  const long long t = blockIdx.x;
  long long bj = (long long)((sqrt(8. * (double)t + 1.) - 1.) * 0.5);
  while (bj * (bj + 1) / 2 > t) --bj;
  while ((bj + 1) * (bj + 2) / 2 <= t) ++bj;
  const long long bi = t - bj * (bj + 1) / 2;
  const long long i = bi * 64 + (threadIdx.x & 63), jw = bj * 64 + (threadIdx.x >> 6);
  double sum = 0.;
  if (i < m) {
    const double mu_i = mean[i], y_i = truth[i];
    const double d_i = c[i + i * ldc] + (truth_var ? truth_var[i] : 0.);  // the truth's variance joins the diagonal here
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const long long j = jw + 4 * s;
      if (j >= m || j <= i) continue;
      const double d_j = c[j + j * ldc] + (truth_var ? truth_var[j] : 0.);
      const double sigma = sqrt(d_i + d_j - 2. * c[i + j * ldc]);
      const double mu = mean[j] - mu_i, ty = fabs(y_i - truth[j]);
      const double diff = ORDER2 ? ty * ty - (mu * mu + sigma * sigma) : ty - expected_abs_normal_1(mu, sigma);
      sum += (w ? w[i + j * ldw] * diff : diff) * diff;
    }
  }
  const double total = block_sum(sum, sh);
  if (threadIdx.x == 0) partial[t] = total;
}

// ---- CRPS of univariate normals (prediction_metrics.hpp:349-364) ---------------------------------------------------------
__global__ void crps_normal_kernel(const double *__restrict__ mu, const double *__restrict__ sigma, const double *__restrict__ y,
                                   long long n, double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double m = mu[i], s = sigma[i], v = y[i];
  double r;
  if (!isfinite(m) || !isfinite(s) || !isfinite(v)) {
    r = nan("");
  } else if (s <= 0.) {
    r = fabs(v - m);
  } else {
    const double z = (v - m) / s;
    const double erfz = erf(z / sqrt(2.));
    const double phi = exp(-0.5 * z * z) / sqrt(2. * M_PI);
    r = s * (z * erfz + 2. * phi - 1. / sqrt(M_PI));
  }
  out[i] = r;
}

__global__ void add_diagonal_kernel(double *__restrict__ A, long long lda, long long n, const double *__restrict__ d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[i + i * lda] += d[i];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// `src` (n doubles at `location`, may be nullptr) as a device pointer: itself, or a copy in `buf`
int device_vector(agp_context *ctx, const double *src, long long n, int location, DevMem<double> *buf, const double **out) {
  *out = src;
  if (!src || location == AGP_DEVICE) return AGP_OK;
  AGP_HIP_CHECK(ctx, alloc_doubles(*buf, (size_t)n));
  *out = buf->get();
  return vector_to_device(ctx, src, n, AGP_HOST, buf->get());
}

// the same for a rows x cols matrix with leading dimension ld; the copy keeps ld
int device_matrix(agp_context *ctx, const double *src, long long rows, long long cols, long long ld, int location, DevMem<double> *buf,
                  const double **out) {
  *out = src;
  if (!src || location == AGP_DEVICE) return AGP_OK;
  const size_t elems = (size_t)ld * (size_t)(cols - 1) + (size_t)rows;
  AGP_HIP_CHECK(ctx, alloc_doubles(*buf, elems));
  *out = buf->get();
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(buf->get(), src, sizeof(double) * elems, hipMemcpyHostToDevice, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

// rows x cols from the device (ld_dev) into the caller's HOST matrix (ld_dst), touching nothing but those entries: the
// rows between two columns of a wider destination - a block of a larger matrix - stay as they are
int copy_out_block(agp_context *ctx, const double *dev, long long ld_dev, long long rows, long long cols, double *dst,
                   long long ld_dst) {
  AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, sizeof(double) * (size_t)ld_dst, dev, sizeof(double) * (size_t)ld_dev,
                                      sizeof(double) * (size_t)rows, (size_t)cols, hipMemcpyDeviceToHost, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

void launch_draw(hipStream_t s, const double *L, long long ldl, long long m, const double *Z, long long ldz, long long n,
                 const double *mean, double *S, long long lds_) {
  DrawArgs g{L, ldl, m, Z, ldz, n, mean, S, lds_};
  draw_kernel<<<dim3((unsigned)((m + ST - 1) / ST), (unsigned)((n + ST - 1) / ST)), GEMM_THREADS, 0, s>>>(g);
}

bool usable_factor(const agp_fit *fit) { return fit && fit->A && fit->failed_pivot < 0; }

}  // namespace

void launch_standard_normal(hipStream_t s, unsigned long long seed, long long m, long long first_column, long long n_columns,
                            double *out, long long ldo) {
  const long long gy = n_columns < 1024 ? n_columns : 1024;
  standard_normal_kernel<<<dim3((unsigned)((m + 255) / 256), (unsigned)gy), 256, 0, s>>>(
      (unsigned)seed, (unsigned)(seed >> 32), m, first_column, n_columns, out, ldo);
}

void launch_rademacher(hipStream_t s, unsigned long long seed, long long m, long long first_column, long long n_columns, double *out,
                       long long ldo) {
  const long long gy = n_columns < 1024 ? n_columns : 1024;
  rademacher_kernel<<<dim3((unsigned)((m + 255) / 256), (unsigned)gy), 256, 0, s>>>((unsigned)seed, (unsigned)(seed >> 32), m, first_column,
                                                                                    n_columns, out, ldo);
}

void launch_add_diagonal(hipStream_t s, double *A, long long lda, long long n, const double *d) {
  add_diagonal_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(A, lda, n, d);
}

}  // namespace agp

using namespace agp;

extern "C" {

int agp_standard_normal(agp_context *ctx, uint64_t seed, int64_t m, int64_t first_column, int64_t n_columns, double *out,
                        int64_t ldo, int location) {
  if (!ctx || !out || m <= 0 || n_columns <= 0 || first_column < 0 || ldo < m) return AGP_ERR_INVALID_ARGUMENT;
  if (m > 0xffffffffll || first_column + n_columns > 0xffffffffll) return AGP_ERR_INVALID_ARGUMENT;  // 32-bit counter words
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (location == AGP_DEVICE) {
    launch_standard_normal(ctx->stream, seed, m, first_column, n_columns, out, ldo);
    AGP_HIP_CHECK(ctx, hipGetLastError());
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return AGP_OK;
  }
  const long long ld = round_up(m, 2);
  DevMem<double> buf;
  AGP_HIP_CHECK(ctx, alloc_doubles(buf, (size_t)ld * (size_t)n_columns));
  launch_standard_normal(ctx->stream, seed, m, first_column, n_columns, buf.get(), ld);
  AGP_HIP_CHECK(ctx, hipGetLastError());
  return copy_out_block(ctx, buf.get(), ld, m, n_columns, out, ldo);
}

int agp_draw_mvn(agp_context *ctx, const agp_fit *fit, const double *mean, int64_t n_draws, uint64_t seed, const double *z,
                 int64_t ldz, double *out, int64_t ldo, int location) {
  if (!ctx || !fit || !mean || !out || n_draws <= 0 || !usable_factor(fit)) return AGP_ERR_INVALID_ARGUMENT;
  if (!fit->phantom.empty()) return AGP_ERR_UNSUPPORTED;  // a fit grown by agp_fit_update: factor the joint covariance instead
  const long long m = fit->n;
  if (ldo < m || (z && ldz < m) || n_draws > 0xffffffffll) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const long long ld = round_up(m, 2);
  DevMem<double> mean_b, z_b, out_b;
  const double *mean_d = nullptr, *z_d = nullptr;
  int st = device_vector(ctx, mean, m, location, &mean_b, &mean_d);
  if (st != AGP_OK) return st;
  long long ldz_d = ldz;
  if (z) {
    if ((st = device_matrix(ctx, z, m, n_draws, ldz, location, &z_b, &z_d)) != AGP_OK) return st;
  } else {
    AGP_HIP_CHECK(ctx, alloc_doubles(z_b, (size_t)ld * (size_t)n_draws));
    launch_standard_normal(s, seed, m, 0, n_draws, z_b.get(), ld);
    z_d = z_b.get();
    ldz_d = ld;
  }
  if (location == AGP_DEVICE) {
    launch_draw(s, fit->A, fit->lda, m, z_d, ldz_d, n_draws, mean_d, out, ldo);
    AGP_HIP_CHECK(ctx, hipGetLastError());
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return AGP_OK;
  }
  AGP_HIP_CHECK(ctx, alloc_doubles(out_b, (size_t)ld * (size_t)n_draws));
  launch_draw(s, fit->A, fit->lda, m, z_d, ldz_d, n_draws, mean_d, out_b.get(), ld);
  AGP_HIP_CHECK(ctx, hipGetLastError());
  return copy_out_block(ctx, out_b.get(), ld, m, n_draws, out, ldo);
}

int agp_energy_score(agp_context *ctx, const double *mean, const double *cov, int64_t ldc, int64_t m, const double *truth,
                     const double *truth_var, const double *weights, uint64_t seed, int64_t num_samples, const double *z,
                     int64_t ldz, int location, double *out) {
  if (!ctx || !mean || !cov || !truth || !out || m <= 0 || ldc < m || num_samples <= 1 || (z && ldz < m))
    return AGP_ERR_INVALID_ARGUMENT;
  if (num_samples > 0x7fffffffll) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const long long k = num_samples / 2 + 1, ncols = 2 * k, ld = round_up(m, 2);  // antithetic_sample, :265
  DevMem<double> mean_b, truth_b, var_b, w_b, z_b, v_b, cols_b;
  const double *mean_d = nullptr, *truth_d = nullptr, *var_d = nullptr, *w_d = nullptr, *z_d = nullptr;
  int st;
  if ((st = device_vector(ctx, mean, m, location, &mean_b, &mean_d)) != AGP_OK) return st;
  if ((st = device_vector(ctx, truth, m, location, &truth_b, &truth_d)) != AGP_OK) return st;
  if ((st = device_vector(ctx, truth_var, m, location, &var_b, &var_d)) != AGP_OK) return st;
  if ((st = device_vector(ctx, weights, m, location, &w_b, &w_d)) != AGP_OK) return st;
  // LL^T of cov + diag(truth_var) on a copy (the reference: Eigen::LDLT of the combined covariance, :407, :431-432)
  agp_fit *fit = new (std::nothrow) agp_fit();
  if (!fit) return AGP_ERR_INVALID_ARGUMENT;
  st = factor_dense(ctx, cov, m, ldc, /*uplo=*/0, location, fit, nullptr, var_d);
  if (st != AGP_OK) { agp_fit_destroy(fit); return st; }
  long long ldz_d = ldz;
  hipError_t e = hipSuccess;
  if (z) {
    st = device_matrix(ctx, z, m, ncols, ldz, location, &z_b, &z_d);
  } else if ((e = alloc_doubles(z_b, (size_t)ld * (size_t)ncols)) == hipSuccess) {
    launch_standard_normal(s, seed, m, 0, ncols, z_b.get(), ld);  // set A: columns 0 .. k - 1, set B: k .. 2 k - 1
    z_d = z_b.get();
    ldz_d = ld;
  }
  if (st == AGP_OK && e == hipSuccess) e = alloc_doubles(v_b, (size_t)ld * (size_t)ncols);
  if (st == AGP_OK && e == hipSuccess) e = alloc_doubles(cols_b, (size_t)(5 * k + 4));
  if (st == AGP_OK && e == hipSuccess) {
    launch_draw(s, fit->A, fit->lda, m, z_d, ldz_d, ncols, nullptr, v_b.get(), ld);
    energy_columns_kernel<<<(unsigned)k, RED_THREADS, 0, s>>>(v_b.get(), ld, m, k, mean_d, truth_d, w_d, cols_b.get());
    energy_finish_kernel<<<1, RED_THREADS, 0, s>>>(cols_b.get(), k, cols_b.get() + 5 * k);
    e = hipGetLastError();
  }
  double sums[3] = {0., 0., 0.};
  if (st == AGP_OK && e == hipSuccess) e = hipMemcpyAsync(sums, cols_b.get() + 5 * k, sizeof(sums), hipMemcpyDeviceToHost, s);
  if (st == AGP_OK && e == hipSuccess) e = hipStreamSynchronize(s);
  agp_fit_destroy(fit);
  if (st != AGP_OK) return st;
  if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return AGP_ERR_HIP; }
  const double term_a = sums[0] / (double)ncols, term_b = sums[1] / (double)ncols, paired = sums[2] / (double)k;
  const double es = 0.5 * (term_a + term_b) - 0.5 * paired;  // :415-418
  *out = es > 0. ? es : (es == es ? 0. : es);                // std::max(0.0, es), a NaN shown as one
  return AGP_OK;
}

int agp_variogram_score(agp_context *ctx, const double *mean, const double *cov, int64_t ldc, int64_t m, const double *truth,
                        const double *truth_var, const double *weights, int64_t ldw, int order, int location, double *out) {
  if (!ctx || !mean || !cov || !truth || !out || m <= 0 || ldc < m || (weights && ldw < m) || (order != 1 && order != 2))
    return AGP_ERR_INVALID_ARGUMENT;
  if (m == 1) { *out = 0.; return AGP_OK; }  // no pair
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevMem<double> mean_b, truth_b, var_b, c_b, w_b, part_b;
  const double *mean_d = nullptr, *truth_d = nullptr, *var_d = nullptr, *c_d = nullptr, *w_d = nullptr;
  int st;
  if ((st = device_vector(ctx, mean, m, location, &mean_b, &mean_d)) != AGP_OK) return st;
  if ((st = device_vector(ctx, truth, m, location, &truth_b, &truth_d)) != AGP_OK) return st;
  if ((st = device_vector(ctx, truth_var, m, location, &var_b, &var_d)) != AGP_OK) return st;
  if ((st = device_matrix(ctx, cov, m, m, ldc, location, &c_b, &c_d)) != AGP_OK) return st;
  if ((st = device_matrix(ctx, weights, m, m, ldw, location, &w_b, &w_d)) != AGP_OK) return st;
  const long long nt = (m + 63) / 64, tiles = nt * (nt + 1) / 2;
  AGP_HIP_CHECK(ctx, alloc_doubles(part_b, (size_t)tiles + 1));
  if (order == 2)
    variogram_kernel<true><<<(unsigned)tiles, RED_THREADS, 0, s>>>(mean_d, c_d, ldc, m, truth_d, var_d, w_d, ldw, part_b.get());
  else
    variogram_kernel<false><<<(unsigned)tiles, RED_THREADS, 0, s>>>(mean_d, c_d, ldc, m, truth_d, var_d, w_d, ldw, part_b.get());
  sum_partials_kernel<<<1, RED_THREADS, 0, s>>>(part_b.get(), tiles, part_b.get() + tiles);
  AGP_HIP_CHECK(ctx, hipGetLastError());
  double total = 0.;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(&total, part_b.get() + tiles, sizeof(double), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  *out = total;
  return AGP_OK;
}

int agp_crps_normal(agp_context *ctx, const double *mu, const double *sigma, const double *y, int64_t n, double *out,
                    int location) {
  if (!ctx || !mu || !sigma || !y || !out || n < 0) return AGP_ERR_INVALID_ARGUMENT;
  if (n == 0) return AGP_OK;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DevMem<double> mu_b, sigma_b, y_b, out_b;
  const double *mu_d = nullptr, *sigma_d = nullptr, *y_d = nullptr;
  int st;
  if ((st = device_vector(ctx, mu, n, location, &mu_b, &mu_d)) != AGP_OK) return st;
  if ((st = device_vector(ctx, sigma, n, location, &sigma_b, &sigma_d)) != AGP_OK) return st;
  if ((st = device_vector(ctx, y, n, location, &y_b, &y_d)) != AGP_OK) return st;
  double *out_d = out;
  if (location == AGP_HOST) {
    AGP_HIP_CHECK(ctx, alloc_doubles(out_b, (size_t)n));
    out_d = out_b.get();
  }
  crps_normal_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(mu_d, sigma_d, y_d, n, out_d);
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (location == AGP_HOST) return copy_out(ctx, out_d, n, out, AGP_HOST);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

}  // extern "C"
