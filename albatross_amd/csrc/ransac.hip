// ransac.hip — GP RANSAC: the trials of one run scored in lock step (include/albatross_amd.h: agp_ransac_score_trials,
// agp_ransac_draw_candidates).  The reference (models/ransac.hpp:172-257 around models/ransac_gp.hpp and
// models/conditional_gaussian.hpp) fits and predicts once per trial on the host; here the prior covariance is built
// once and T trials are one batch:
//   1  the Gram of the measurement features, full N x N, without y_var (launch_gram)
//   2  gather: every trial's A_t = Sigma_cc + R_c into a slab and d_c beside it, padded to the trial's size class with a
//      unit diagonal (ransac_gather_kernel)
//   3  the shared batched front end: L_t, z_t = L_t^-1 d_c and the log sums (batch_front.h: factor_batch, the plain
//      schedule: no look-ahead, no fused panel launches, so a problem's result does not depend on the batch around it)
//   4  one launch over (tile of groups, trial): ransac_score_kernel below
//   5  one workgroup per trial: q_c = z_t^T z_t and the accept counts in a fixed order (ransac_count_kernel)
// Trials are sorted into size classes (16, 32, 64, 128, 256 candidate points) and a class runs stages 2-5 in chunks of
// bounded workspace, so the padding - and with it every bit of a trial's results - depends on the trial alone, never on
// n_trials or on the other trials of the call.
//
// The scoring kernel.  A workgroup owns one trial t and one tile of consecutive groups of at most 64 points in all (a
// group has at most 64 points, so a tile holds at least one).  It gathers W = Sigma_cg for its columns from the
// resident Gram (for one candidate row the tile's columns are the entries K[p_j, c_a] of ONE column of K: contiguous
// where a group's points are), and forward-substitutes against L_t, which is streamed through LDS in panels of 8
// columns: the 8 x 8 triangle is solved in registers by every wave for its 64 columns, the rows below are updated from
// the panel in LDS.  W (s x 64 doubles) is what bounds the sizes: with s = 256 it takes 128 KiB of the CU's 160 KiB,
// the panel 16 KiB - hence RANSAC_MAX_CANDIDATE_POINTS = 256 and RANSAC_MAX_GROUP_POINTS = 64, and one instantiation
// per size class so that small trials keep several workgroups per CU.  Then r = W^T z - d_g, P = Sigma_gg - W^T W + R_g
// for the pairs of one group (in registers, then over W in LDS), and the tile's block-diagonal P is eliminated in
// place column by column (P = L D L^T; r rides along), which yields log|P| and r^T P^-1 r per group; NLL_MARGINAL
// forms and reads the diagonal only, a singleton group is the m = 1 case of the same code.  No workgroup waits for
// another one; fp64 on the vector pipe throughout.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/albatross_amd/chi_squared.h"
#include "api_internal.h"
#include "batch_front.h"

using namespace agp;

namespace {

constexpr int RANSAC_MAX_CANDIDATE_POINTS = AGP_RANSAC_MAX_CANDIDATE_POINTS;  // 256: W in LDS (above)
constexpr int RANSAC_MAX_GROUP_POINTS = AGP_RANSAC_MAX_GROUP_POINTS;          // 64: the columns of one tile
constexpr int NC = RANSAC_MAX_GROUP_POINTS;
constexpr int PW = 8;         // columns of L_t per LDS panel
constexpr int PLD = NC + 1;   // leading dimension of P over W
constexpr size_t RANSAC_CHUNK_BYTES = 512ull << 20;  // slabs + tile images + z of the trials in flight

static_assert(RANSAC_MAX_CANDIDATE_POINTS == 256 && RANSAC_MAX_GROUP_POINTS == 64, "the size classes and the tile below");

struct RansacArgs {
  const double *K;          // N x N Gram, both triangles
  long long ldk;
  const double *d, *yvar;   // deviation, y_var (may be null)
  const long long *goff, *gidx;    // the grouping
  const int *tiles;         // first group of every tile, n_tiles + 1
  const long long *cpo, *cpts;     // candidate points per trial: offsets (n_trials + 1) and point ids
  const long long *cgo, *cgr;      // candidate groups per trial: offsets and group ids
  const int *order;         // problem b of this launch is trial order[b]
  double *A;                // the slabs: L_t after the factor
  long long lda, stride_A;
  double *z;                // z_t, stride np2
  long long np2;
  const double *logsum;     // per problem
  const int *flags;         // 4 per problem: [0] NaN, [1] first bad pivot + 1
  double *metric;           // n_groups x n_trials, ld ldm, column = trial
  long long ldm, n_groups;
  int S;                    // padded size of the class
  int inlier_metric;
  double threshold;
  // per trial, indexed by the trial: q_c, log|A|, failed, accepted groups / points
  double *quad, *logdet;
  int *failed;
  long long *counts;
};

__device__ __forceinline__ bool trial_failed(const RansacArgs &a, long long b) {
  const double ls = a.logsum[b];
  return a.flags[4 * b] != 0 || a.flags[4 * b + 1] != 0 || !(fabs(ls) <= 1.7976931348623157e308);
}

// grid (S, problems): column `col` of problem b's slab, and with col == 0 its right-hand side
__global__ __launch_bounds__(256) void ransac_gather_kernel(RansacArgs a) {
  const long long b = blockIdx.y;
  const int col = (int)blockIdx.x, S = a.S;
  const int t = a.order[b];
  const long long p0 = a.cpo[t];
  const int s = (int)(a.cpo[t + 1] - p0);
  const long long pc = col < s ? a.cpts[p0 + col] : 0;
  double *dst = a.A + b * a.stride_A + (long long)col * a.lda;
  for (int row = (int)threadIdx.x; row < S; row += 256) {
    double v = row == col ? 1. : 0.;
    const long long pr = row < s ? a.cpts[p0 + row] : 0;
    if (row < s && col < s) {
      v = a.K[pr + pc * a.ldk];
      if (row == col && a.yvar) v += a.yvar[pr];
    }
    dst[row] = v;
    if (col == 0) a.z[b * a.np2 + row] = row < s ? a.d[pr] : 0.;
  }
}

template <int SMAX>
__global__ __launch_bounds__(256) void ransac_score_kernel(RansacArgs a) {
  constexpr int WP = SMAX * NC > NC * PLD ? SMAX * NC : NC * PLD;
  __shared__ double Wl[WP];        // W (row a, column c at a * NC + c), later P (i, j at i * PLD + j, j <= i)
  __shared__ double Lp[PW * SMAX]; // panel column j, row kk (from the panel's first row) at j * SMAX + kk
  __shared__ double zl[SMAX];
  __shared__ double rl[NC];
  __shared__ long long colpt[NC];
  __shared__ int colgrp[NC];
  __shared__ int gcand[NC];
  __shared__ int gfirst[NC + 1];

  const int tid = (int)threadIdx.x;
  const long long b = blockIdx.y;
  const int t = a.order[b];
  const int g0 = a.tiles[blockIdx.x], ng = a.tiles[blockIdx.x + 1] - g0;
  const long long c0 = a.goff[g0];
  const int ncol = (int)(a.goff[g0 + ng] - c0);
  double *mcol = a.metric + (long long)t * a.ldm + g0;
  if (trial_failed(a, b)) {  // A_t did not factor: every metric of the trial is NaN
    if (tid < ng) mcol[tid] = nan("");
    return;
  }
  const long long p0 = a.cpo[t];
  const int s = (int)(a.cpo[t + 1] - p0);
  const long long *cand = a.cpts + p0;
  const double *Lb = a.A + b * a.stride_A;

  if (tid < NC) {
    colpt[tid] = tid < ncol ? a.gidx[c0 + tid] : 0;
    colgrp[tid] = -1;
  }
  if (tid < ng) {
    gcand[tid] = 0;
    gfirst[tid] = (int)(a.goff[g0 + tid] - c0);
  }
  if (tid == 0) gfirst[ng] = ncol;
  for (int e = tid; e < s; e += 256) zl[e] = a.z[b * a.np2 + e];
  __syncthreads();
  if (tid < ng)
    for (int c = gfirst[tid]; c < gfirst[tid + 1]; ++c) colgrp[c] = tid;
  {
    const long long q0 = a.cgo[t];
    const int ncg = (int)(a.cgo[t + 1] - q0);
    for (int e = tid; e < ncg; e += 256) {
      const long long g = a.cgr[q0 + e];
      if (g >= g0 && g < g0 + ng) gcand[(int)(g - g0)] = 1;
    }
  }
  for (int e = tid; e < s * NC; e += 256) {  // W = Sigma_cg: row e / NC is a run of ONE column of K
    const int row = e / NC, c = e % NC;
    Wl[e] = c < ncol ? a.K[colpt[c] + cand[row] * a.ldk] : 0.;
  }
  __syncthreads();

  // W <- L^-1 W, a panel of PW columns of L at a time
  const int c = tid & (NC - 1), r = tid / NC;  // a wave = one r, 64 columns
  for (int i0 = 0; i0 < s; i0 += PW) {
    const int pw = s - i0 < PW ? s - i0 : PW, rows = s - i0;
    double w[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) w[j] = j < pw ? Wl[(i0 + j) * NC + c] : 0.;
    for (int e = tid; e < pw * rows; e += 256) {
      const int j = e / rows, kk = e - j * rows;
      Lp[j * SMAX + kk] = Lb[(long long)(i0 + j) * a.lda + (i0 + kk)];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      if (j < pw) {
        double v = w[j];
#pragma unroll
        for (int i = 0; i < j; ++i) v -= Lp[i * SMAX + j] * w[i];
        w[j] = v / Lp[j * SMAX + j];
      }
    }
    if (r == 0) {
#pragma unroll
      for (int j = 0; j < PW; ++j)
        if (j < pw) Wl[(i0 + j) * NC + c] = w[j];
    }
    for (int k = i0 + PW + r; k < s; k += 256 / NC) {  // (a short last panel has no rows below it)
      double v = Wl[k * NC + c];
#pragma unroll
      for (int j = 0; j < PW; ++j) v -= Lp[j * SMAX + (k - i0)] * w[j];
      Wl[k * NC + c] = v;
    }
    __syncthreads();
  }

  // r = W^T z - d_g
  if (tid < NC) {
    double acc = 0.;
    for (int i = 0; i < s; ++i) acc += Wl[i * NC + tid] * zl[i];
    rl[tid] = tid < ncol ? acc - a.d[colpt[tid]] : 0.;
  }
  // P = Sigma_gg - W^T W + R_g for the pairs (i, j <= i) of one group; the diagonal alone for NLL_MARGINAL
  const bool marginal = a.inlier_metric == AGP_RANSAC_NLL_MARGINAL;
  constexpr int PER = NC * NC / 256;
  double acc[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int e = tid + 256 * q, i = e % NC, j = e / NC;
    const bool valid = i < ncol && j <= i && colgrp[i] == colgrp[j] && (!marginal || i == j);
    double v = 0.;
    if (valid) {
      v = a.K[colpt[i] + colpt[j] * a.ldk];
      double ww = 0.;
      for (int k = 0; k < s; ++k) ww += Wl[k * NC + i] * Wl[k * NC + j];
      v -= ww;
      if (i == j && a.yvar) v += a.yvar[colpt[i]];
    }
    acc[q] = v;
  }
  __syncthreads();  // W is dead
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int e = tid + 256 * q, i = e % NC, j = e / NC;
    if (i < ncol && j <= i && colgrp[i] == colgrp[j] && (!marginal || i == j)) Wl[i * PLD + j] = acc[q];
  }
  __syncthreads();
  // P = L D L^T in place, one column per step, inside the column's group; r <- L^-1 r
  if (!marginal) {
    for (int k = 0; k < ncol; ++k) {
      const int kend = gfirst[colgrp[k] + 1];
      if (c > k && c < kend) {
        const double f = Wl[c * PLD + k] / Wl[k * PLD + k];
        for (int j = k + 1 + r; j <= c; j += 256 / NC) Wl[c * PLD + j] -= f * Wl[j * PLD + k];
        if (r == 0) rl[c] -= f * rl[k];
      }
      __syncthreads();
    }
  }
  if (tid < ng) {
    double m = nan("");
    if (!gcand[tid]) {
      double logdet = 0., quad = 0.;
      bool bad = false;
      const int first = gfirst[tid], last = gfirst[tid + 1];
      for (int k = first; k < last; ++k) {
        const double piv = Wl[k * PLD + k];
        if (!(piv > 0.)) bad = true;
        logdet += log(piv);
        quad += rl[k] * rl[k] / piv;
      }
      const double dof = (double)(last - first);
      if (!bad)
        m = a.inlier_metric == AGP_RANSAC_CHI_SQUARED_CDF ? albatross_amd_stats::chi_squared_cdf(quad, dof)
                                                          : 0.5 * (logdet + quad + dof * 1.8378770664093453);
    }
    mcol[tid] = m;
  }
}

// one workgroup per problem: q_c = z^T z, log|A|, and the accepted groups / points of the trial's metric column, summed
// by thread in a strided order and then over the threads in a fixed tree
__global__ __launch_bounds__(256) void ransac_count_kernel(RansacArgs a) {
  __shared__ double sq[256];
  __shared__ long long sg[256], sp[256];
  const int tid = (int)threadIdx.x;
  const long long b = blockIdx.x;
  const int t = a.order[b];
  const bool failed = trial_failed(a, b);
  const int s = (int)(a.cpo[t + 1] - a.cpo[t]);
  double q = 0.;
  long long ngr = 0, npt = 0;
  if (!failed) {
    for (int e = tid; e < s; e += 256) {
      const double v = a.z[b * a.np2 + e];
      q += v * v;
    }
    const double *mcol = a.metric + (long long)t * a.ldm;
    for (long long g = tid; g < a.n_groups; g += 256)
      if (mcol[g] <= a.threshold) {  // NaN: not an inlier
        ngr += 1;
        npt += a.goff[g + 1] - a.goff[g];
      }
  }
  sq[tid] = q; sg[tid] = ngr; sp[tid] = npt;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) { sq[tid] += sq[tid + h]; sg[tid] += sg[tid + h]; sp[tid] += sp[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    a.failed[t] = failed ? 1 : 0;
    a.quad[t] = failed ? nan("") : sq[0];
    a.logdet[t] = failed ? nan("") : 2. * a.logsum[b];
    a.counts[2 * t] = sg[0];
    a.counts[2 * t + 1] = sp[0];
  }
}

void launch_score(hipStream_t s, int S, unsigned n_tiles, unsigned count, const RansacArgs &a) {
  const dim3 grid(n_tiles, count), block(256);
  switch (S) {
    case 16: hipLaunchKernelGGL(ransac_score_kernel<16>, grid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL(ransac_score_kernel<32>, grid, block, 0, s, a); break;
    case 64: hipLaunchKernelGGL(ransac_score_kernel<64>, grid, block, 0, s, a); break;
    case 128: hipLaunchKernelGGL(ransac_score_kernel<128>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(ransac_score_kernel<256>, grid, block, 0, s, a); break;
  }
}

int size_class(long long s) {
  int S = 16;
  while (S < s) S *= 2;
  return S;
}

struct ChunkRegions {
  double *A, *img, *z, *logsum;
  int *flags;
};
ChunkRegions carve_chunk(WsLayout &ws, const BatchGeometry &g) {
  return {ws.take<double>(g.slabs()), ws.take<double>(g.images()), ws.take<double>(g.vectors()), ws.take<double>((size_t)g.cp2),
          ws.take<int>(4 * (size_t)g.cp2)};
}
size_t problem_bytes(int S) {
  const BatchGeometry one = batch_geometry(S, 1);
  return sizeof(double) * (size_t)(one.stride_A + one.stride_I + one.np2 + 1) + 4 * sizeof(int);
}
long long chunk_trials(int S) {
  const long long fit = (long long)(RANSAC_CHUNK_BYTES / problem_bytes(S));
  return fit < 1 ? 1 : (fit > BATCH_MAX_PROBLEMS ? BATCH_MAX_PROBLEMS : fit);
}

struct FixedRegions {
  double *K, *d, *yvar, *metric, *quad, *logdet;
  long long *goff, *gidx, *cpo, *cpts, *cgo, *cgr, *counts;
  int *tiles, *order, *failed;
};
FixedRegions carve_fixed(WsLayout &ws, long long n, long long ldk, bool has_yvar, long long G, long long total, long long T,
                         long long cand_points, long long cand_groups, long long n_tiles) {
  FixedRegions r;
  r.K = ws.take<double>((size_t)ldk * (size_t)n);
  r.d = ws.take<double>((size_t)n);
  r.yvar = has_yvar ? ws.take<double>((size_t)n) : nullptr;
  r.metric = ws.take<double>((size_t)G * (size_t)T);
  r.quad = ws.take<double>((size_t)T);
  r.logdet = ws.take<double>((size_t)T);
  r.goff = ws.take<long long>((size_t)G + 1);
  r.gidx = ws.take<long long>((size_t)total);
  r.cpo = ws.take<long long>((size_t)T + 1);
  r.cpts = ws.take<long long>((size_t)cand_points);
  r.cgo = ws.take<long long>((size_t)T + 1);
  r.cgr = ws.take<long long>((size_t)cand_groups);
  r.counts = ws.take<long long>(2 * (size_t)T);
  r.tiles = ws.take<int>((size_t)n_tiles + 1);
  r.order = ws.take<int>((size_t)T);
  r.failed = ws.take<int>((size_t)T);
  return r;
}

// the project's own generator of the draws: splitmix64 (Steele, Lea and Flood, OOPSLA 2014)
inline unsigned long long splitmix64(unsigned long long &state) {
  unsigned long long v = (state += 0x9E3779B97F4A7C15ull);
  v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
  v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
  return v ^ (v >> 31);
}
// uniform in [0, bound), bound >= 1, by rejection
inline unsigned long long uniform_below(unsigned long long &state, unsigned long long bound) {
  const unsigned long long limit = ~0ull - (~0ull % bound + 1) % bound;  // largest v with v % bound unbiased
  for (;;) {
    const unsigned long long v = splitmix64(state);
    if (v <= limit) return v % bound;
  }
}

}  // namespace

extern "C" {

int agp_ransac_draw_candidates(uint64_t seed, int64_t n_groups, int64_t sample_size, int64_t n_trials, int64_t *out) {
  if (n_groups <= 0 || sample_size < 0 || sample_size > n_groups || n_trials < 0 || (!out && n_trials * sample_size > 0))
    return AGP_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> chosen;
  for (int64_t t = 0; t < n_trials; ++t) {
    // trial t has a stream of its own, so a trial's draw does not depend on n_trials
    unsigned long long state = (unsigned long long)seed ^ (0xD1B54A32D192ED03ull * (unsigned long long)(t + 1));
    chosen.clear();
    for (int64_t j = n_groups - sample_size; j < n_groups; ++j) {  // Floyd's sampling without replacement
      const int64_t v = (int64_t)uniform_below(state, (unsigned long long)j + 1);
      chosen.push_back(std::find(chosen.begin(), chosen.end(), v) == chosen.end() ? v : j);
    }
    std::sort(chosen.begin(), chosen.end());
    std::copy(chosen.begin(), chosen.end(), out + t * sample_size);
  }
  return AGP_OK;
}

int agp_ransac_score_trials(agp_context *c, const agp_kernel *k, const agp_features *x, const double *deviation, const double *y_var,
                            int64_t n_groups, const int64_t *offsets, const int64_t *indices, int64_t n_trials,
                            const int64_t *cand_offsets, const int64_t *cand_groups, int inlier_metric, double inlier_threshold,
                            double *metric, int64_t ld_metric, int metric_location, int64_t *inlier_groups,
                            int64_t *inlier_points, double *candidate_quadratic, double *candidate_log_det, int *status) {
  // ---- every check before anything is written or launched ----
  if (!c || !k || !x || !deviation || !offsets || !indices || !cand_offsets || !cand_groups || !inlier_groups || !inlier_points ||
      !candidate_quadratic || !candidate_log_det || !status)
    return AGP_ERR_INVALID_ARGUMENT;
  if (inlier_metric != AGP_RANSAC_NLL_JOINT && inlier_metric != AGP_RANSAC_NLL_MARGINAL && inlier_metric != AGP_RANSAC_CHI_SQUARED_CDF)
    return AGP_ERR_INVALID_ARGUMENT;
  if (metric_location != AGP_HOST && metric_location != AGP_DEVICE) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n, G = n_groups, T = n_trials;
  if (n <= 0 || G <= 0 || G > INT32_MAX / 2 || T <= 0 || T > BATCH_MAX_PROBLEMS || offsets[0] != 0 || cand_offsets[0] != 0)
    return AGP_ERR_INVALID_ARGUMENT;
  if (metric && ld_metric < G) return AGP_ERR_INVALID_ARGUMENT;
  for (long long g = 0; g < G; ++g) {
    const long long m = offsets[g + 1] - offsets[g];
    if (m < 1 || m > RANSAC_MAX_GROUP_POINTS) return AGP_ERR_INVALID_ARGUMENT;
  }
  const long long total = offsets[G];
  if (total > n) return AGP_ERR_INVALID_ARGUMENT;
  {
    std::vector<char> seen((size_t)n, 0);
    for (long long i = 0; i < total; ++i) {
      if (indices[i] < 0 || indices[i] >= n || seen[(size_t)indices[i]]) return AGP_ERR_INVALID_ARGUMENT;
      seen[(size_t)indices[i]] = 1;
    }
  }
  std::vector<long long> cpo((size_t)T + 1, 0), cpts;
  {
    std::vector<long long> stamp((size_t)G, -1);
    for (long long t = 0; t < T; ++t) {
      const long long q0 = cand_offsets[t], q1 = cand_offsets[t + 1];
      if (q1 <= q0 || q1 - q0 > RANSAC_MAX_CANDIDATE_POINTS) return AGP_ERR_INVALID_ARGUMENT;
      long long s = 0;
      for (long long q = q0; q < q1; ++q) {
        const long long g = cand_groups[q];
        if (g < 0 || g >= G || stamp[(size_t)g] == t) return AGP_ERR_INVALID_ARGUMENT;
        stamp[(size_t)g] = t;
        s += offsets[g + 1] - offsets[g];
        if (s > RANSAC_MAX_CANDIDATE_POINTS) return AGP_ERR_INVALID_ARGUMENT;
        for (long long i = offsets[g]; i < offsets[g + 1]; ++i) cpts.push_back(indices[i]);
      }
      cpo[(size_t)t + 1] = cpo[(size_t)t] + s;
    }
  }
  const long long n_cand_groups = cand_offsets[T];
  // tiles: consecutive groups, at most NC points
  std::vector<int> tiles;
  {
    long long cols = 0;
    tiles.push_back(0);
    for (long long g = 0; g < G; ++g) {
      const long long m = offsets[g + 1] - offsets[g];
      if (cols + m > NC) { tiles.push_back((int)g); cols = 0; }
      cols += m;
    }
    tiles.push_back((int)G);
  }
  const long long n_tiles = (long long)tiles.size() - 1;
  // trials by size class, in the caller's order inside a class
  std::vector<int> order((size_t)T);
  std::vector<long long> class_first;  // into order, per class 16 .. 256, + end
  std::vector<int> class_size;
  {
    long long pos = 0;
    for (int S = 16; S <= RANSAC_MAX_CANDIDATE_POINTS; S *= 2) {
      const long long first = pos;
      for (long long t = 0; t < T; ++t)
        if (size_class(cpo[(size_t)t + 1] - cpo[(size_t)t]) == S) order[(size_t)pos++] = (int)t;
      if (pos > first) { class_first.push_back(first); class_size.push_back(S); }
    }
    class_first.push_back(pos);
  }
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));

  // ---- workspaces: ws_aux holds what the whole call reads, ws_A the slabs of the chunk in flight ----
  const long long ldk = round_up(n, 2);
  auto fixed = [&](WsLayout &w) {
    return carve_fixed(w, n, ldk, y_var != nullptr, G, total, T, (long long)cpts.size(), n_cand_groups, n_tiles);
  };
  WsLayout size_fixed, size_chunk;
  fixed(size_fixed);
  size_t chunk_bytes = 0;
  for (size_t ci = 0; ci < class_size.size(); ++ci) {
    const long long cnt = std::min(class_first[ci + 1] - class_first[ci], chunk_trials(class_size[ci]));
    WsLayout w;
    carve_chunk(w, batch_geometry(class_size[ci], cnt));
    chunk_bytes = std::max(chunk_bytes, w.bytes());
  }
  if ((st = reserve_ws(ctx, ctx->ws_aux, size_fixed.bytes())) != AGP_OK) return st;
  if ((st = reserve_ws(ctx, ctx->ws_A, chunk_bytes)) != AGP_OK) return st;
  WsLayout ws_fixed(ctx->ws_aux);
  const FixedRegions f = fixed(ws_fixed);
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling;
  static_assert(sizeof(long long) == sizeof(int64_t), "index width");

  // ---- uploads (pageable sources: synchronised before the host vectors go) ----
  const hipMemcpyKind in_kind = x->location == AGP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.d, deviation, sizeof(double) * (size_t)n, in_kind, s));
  if (y_var) AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.yvar, y_var, sizeof(double) * (size_t)n, in_kind, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.goff, offsets, sizeof(long long) * (size_t)(G + 1), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.gidx, indices, sizeof(long long) * (size_t)total, hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.cpo, cpo.data(), sizeof(long long) * cpo.size(), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.cpts, cpts.data(), sizeof(long long) * cpts.size(), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.cgo, cand_offsets, sizeof(long long) * (size_t)(T + 1), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.cgr, cand_groups, sizeof(long long) * (size_t)n_cand_groups, hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.tiles, tiles.data(), sizeof(int) * tiles.size(), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f.order, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));

  // ---- 1: the prior covariance of the measurements, once ----
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  FeatView xm = dx.v;
  xm.meas = 1;  // as_measurements(x), gp.hpp:421-425
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[0], s));
  launch_gram(s, dprog, xm, xm, true, false, f.K, ldk, nullptr, nullptr, &k->prog);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));

  RansacArgs a;
  a.K = f.K; a.ldk = ldk; a.d = f.d; a.yvar = f.yvar; a.goff = f.goff; a.gidx = f.gidx; a.tiles = f.tiles;
  a.cpo = f.cpo; a.cpts = f.cpts; a.cgo = f.cgo; a.cgr = f.cgr;
  a.metric = f.metric; a.ldm = G; a.n_groups = G; a.inlier_metric = inlier_metric; a.threshold = inlier_threshold;
  a.quad = f.quad; a.logdet = f.logdet; a.failed = f.failed; a.counts = f.counts;
  // ---- 2-5 per size class, in chunks of bounded workspace ----
  float ms_gather = 0.f, ms_factor = 0.f, ms_score = 0.f;
  for (size_t ci = 0; ci < class_size.size(); ++ci) {
    const int S = class_size[ci];
    const long long cap = chunk_trials(S);
    for (long long first = class_first[ci]; first < class_first[ci + 1]; first += cap) {
      const long long cnt = std::min(cap, class_first[ci + 1] - first);
      const BatchGeometry geo = batch_geometry(S, cnt);
      WsLayout ws(ctx->ws_A);
      const ChunkRegions r = carve_chunk(ws, geo);
      a.order = f.order + first;
      a.A = r.A; a.lda = geo.lda; a.stride_A = geo.stride_A; a.z = r.z; a.np2 = geo.np2; a.logsum = r.logsum; a.flags = r.flags;
      a.S = S;
      AGP_HIP_CHECK(ctx, hipMemsetAsync(r.logsum, 0, sizeof(double) * (size_t)geo.cp2, s));
      AGP_HIP_CHECK(ctx, hipMemsetAsync(r.flags, 0, sizeof(int) * 4 * (size_t)geo.cp2, s));
      if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
      hipLaunchKernelGGL(ransac_gather_kernel, dim3((unsigned)S, (unsigned)cnt), dim3(256), 0, s, a);
      if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[3], s));
      factor_batch(ctx, geo, /*allow_lookahead=*/false, r.A, r.img, r.z, r.flags, 4, r.logsum, nullptr);
      if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[4], s));
      launch_score(s, S, (unsigned)n_tiles, (unsigned)cnt, a);
      hipLaunchKernelGGL(ransac_count_kernel, dim3((unsigned)cnt), dim3(256), 0, s, a);
      if (prof) {
        AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
        AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->stage_ev[2], ctx->stage_ev[3]) == hipSuccess) ms_gather += ms;
        if (hipEventElapsedTime(&ms, ctx->stage_ev[3], ctx->stage_ev[4]) == hipSuccess) ms_factor += ms;
        if (hipEventElapsedTime(&ms, ctx->stage_ev[4], ctx->stage_ev[5]) == hipSuccess) ms_score += ms;
      }
    }
  }
  AGP_HIP_CHECK(ctx, hipGetLastError());

  // ---- download; the caller's arrays are written only when everything has run ----
  std::vector<double> h_quad((size_t)T), h_logdet((size_t)T);
  std::vector<long long> h_counts(2 * (size_t)T);
  std::vector<int> h_failed((size_t)T);
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_quad.data(), f.quad, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_logdet.data(), f.logdet, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_counts.data(), f.counts, sizeof(long long) * 2 * (size_t)T, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_failed.data(), f.failed, sizeof(int) * (size_t)T, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  if (metric && (st = copy_out_2d(ctx, f.metric, G, G, T, metric, ld_metric, metric_location)) != AGP_OK) return st;
  for (long long t = 0; t < T; ++t) {
    status[t] = h_failed[(size_t)t] ? AGP_ERR_NOT_POSITIVE_DEFINITE : AGP_OK;
    candidate_quadratic[t] = h_quad[(size_t)t];
    candidate_log_det[t] = h_logdet[(size_t)t];
    inlier_groups[t] = h_counts[2 * (size_t)t];
    inlier_points[t] = h_counts[2 * (size_t)t + 1];
  }
  if (prof) {
    float ms = 0.f;
    for (double &v : ctx->stage_ms) v = 0.;
    if (hipEventElapsedTime(&ms, ctx->stage_ev[0], ctx->stage_ev[1]) == hipSuccess) ctx->stage_ms[0] = ms;
    ctx->stage_ms[1] = ms_factor;
    ctx->stage_ms[2] = ms_gather;
    ctx->stage_ms[8] = ms_score;
  }
  return AGP_OK;
}

}  // extern "C"
