// sparse_gradient.hip — agp_sparse_nll_gradient: exact gradient of the sparse GP's (FITC / PITC) negative log-likelihood.
//
// Notation of sparse_api.hip: n observations in groups g, m inducing points u, D = diag(y_var) + measurement_nugget I,
// K_uu = k(u, u) + inducing_nugget I, Q = K_fu K_uu^-1 K_uf, A = blockdiag_g(k(x_g, x_g) + D_g - Q_gg), Kt = A + Q,
// NLL = 1/2 (log|Kt| + y^T Kt^-1 y + n log 2 pi).  With alpha = Kt^-1 y, G = Kt^-1 - alpha alpha^T, bd(.) the group-block
// diagonal part, H = G - bd(G), E = K_fu K_uu^-1:
//
//   2 dNLL / dtheta = sum_g <bd(G)_g, dk(x_g, x_g)> + <2 H E, dk(x, u)> + <-E^T H E, dk(u, u)>
//   dNLL / d measurement_nugget = 1/2 trace(bd(G)),   dNLL / d inducing_nugget = 1/2 trace(-E^T H E)
//
// Everything is formed from what the fit leaves behind (sparse_internal.h: the scratch of sparse_fit_fast), as m x n
// matrices whose column blocks are the groups - no n x n matrix anywhere:
//   aw = y_w - W^T v,   alpha_g = R_g^T aw_g                         R_g = L_g^-1 (the block factors of A)
//   Z = Lacc^-1 W = L2^-1 Q1_W,   N_g = -Z_g R_g = -(A^-1 K_fu Lacc^-T)_g^T
//   -bd(G)_g = alpha_g alpha_g^T + N_g^T N_g - R_g^T R_g              (s_g x s_g slabs, both triangles)
//   E^T = L_u^-T P,   q = E^T alpha
//   -(H E)^T = L1^-T L2^-T N + [E_g^T bd(G)_g]_g + q alpha^T          (in place over N)
//   -W_uu = E^T (H E)                                                 (split-K slabs over the observations)
// followed by three contractions of those weights against the tangent form of the covariance program (contract.h:
// contract_tile, the body shared with gradient.hip) with the measurement / equality semantics of the Gram call that
// built each matrix: group blocks (measurement, measurement), k(u, x) (plain, measurement), k(u, u) (plain, plain).
//
// Workspace beyond the fit's pool (K_uf | P | slabs): ONE more ldk x (n + m) slab (Q1^T no longer shares P's region),
// two sets of s_g x s_g group slabs (R_g and bd(G)_g: n * s doubles each for groups of s) and O(n + m^2) vectors.
//
// agp_sparse_held_out (leave-one-group-out cross validation from one fit, include/albatross_amd.h) shares the stages up to
// bd(Kt^-1)_g with the gradient (inverse_blocks_begin / inverse_blocks_run) and then runs the value chain of the dense
// leave-one-group-out metric (gradient.hip: logo_chunk_sigma, logo_chunk_terms) on those blocks, chunk by chunk.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "api_internal.h"
#include "batch_layout.h"
#include "sparse_internal.h"
#include "contract.h"
#include "contract_internal.h"
#include "cov_eval.h"

using namespace agp;

namespace {

// group of global point i: off[g] <= i < off[g + 1]  (off has G + 1 entries)
__device__ __forceinline__ long long find_group(const long long *__restrict__ off, long long G, long long i) {
  long long lo = 0, hi = G;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// alpha_g = R_g^T aw_g: one wave per point i (lanes over the rows k >= i of column i of R_g: coalesced), butterfly sum
__global__ __launch_bounds__(256) void group_rt_vec_kernel(const double *__restrict__ R, const long long *__restrict__ off,
                                                           const long long *__restrict__ roff, const long long *__restrict__ rld,
                                                           long long G, long long n, const double *__restrict__ aw,
                                                           double *__restrict__ alpha) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= n) return;
  const long long g = find_group(off, G, i), o = off[g], sg = off[g + 1] - o, il = i - o;
  const double *col = R + roff[g] + il * rld[g];
  double acc = 0.;
  for (long long k = il + lane; k < sg; k += 64) acc += col[k] * aw[o + k];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane == 0) alpha[i] = acc;
}

// The group slabs hold the lower triangle of bd(Kt^-1)_g = R_g^T R_g - N_g^T N_g.  Overwrite them, BOTH triangles, with
// -bd(G)_g = alpha_g alpha_g^T - bd(Kt^-1)_g and keep the diagonal of bd(G) in diag[].  One workgroup per column.
__global__ __launch_bounds__(256) void group_weight_kernel(double *__restrict__ B, const long long *__restrict__ off,
                                                           const long long *__restrict__ boff, const long long *__restrict__ bld,
                                                           long long G, const double *__restrict__ alpha,
                                                           double *__restrict__ diag) {
  const long long j = blockIdx.x;
  const long long g = find_group(off, G, j), o = off[g], sg = off[g + 1] - o, jl = j - o, ld = bld[g];
  double *b = B + boff[g];
  const double aj = alpha[j];
  for (long long il = jl + threadIdx.x; il < sg; il += 256) {
    const double v = aj * alpha[o + il] - b[il + jl * ld];
    b[il + jl * ld] = v;
    if (il == jl) diag[j] = -v;
    else b[jl + il * ld] = v;
  }
}

// M (m x n, ldm) += q alpha^T
__global__ __launch_bounds__(256) void rank_one_add_kernel(double *__restrict__ M, long long ld, long long m,
                                                           const double *__restrict__ q, const double *__restrict__ alpha) {
  const long long c = (long long)blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;  // (the long dimension in grid x)
  if (c < m) M[c + i * ld] += q[c] * alpha[i];
}

// out[0] = scale * sum_i v[i * stride]   (one workgroup, fixed order)
__global__ __launch_bounds__(1024) void strided_sum_kernel(const double *__restrict__ v, long long n, long long stride, double scale,
                                                           double *__restrict__ out) {
  __shared__ double red[1024];
  double acc = 0.;
  for (long long i = threadIdx.x; i < n; i += 1024) acc += v[i * stride];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = scale * red[0];
}

// ---- the contractions: partial[tile][g] = sum over the tile's pairs of mult * w(row, col) dk(row, col) / dslot_g -----
// One kernel, three shapes (SparseContractArgs::mode, contract_internal.h).

template <int DIMP>
__global__ __launch_bounds__(CT_THREADS) void sparse_contract_kernel(const DevProgram *__restrict__ P, FeatView R, FeatView C,
                                                                     SparseContractArgs a) {
  const long long id = blockIdx.x;
  ContractTile t;
  t.rbase = t.cbase = 0;
  t.lower = a.mode != 0;
  MatrixWeight w{a.W, a.ldw};
  if (a.mode == 0) {
    t.bi = (int)(id % a.tiles_r);
    t.bj = (int)(id / a.tiles_r);
    t.nrl = R.n; t.ncl = C.n;
  } else if (a.mode == 1) {
    lower_tile(id, t.bi, t.bj);
    t.nrl = t.ncl = R.n;
  } else {
    const long long g = find_group(a.tstart, a.G, id);
    lower_tile(id - a.tstart[g], t.bi, t.bj);
    t.rbase = t.cbase = a.off[g];
    t.nrl = t.ncl = a.off[g + 1] - a.off[g];
    w = MatrixWeight{a.W + a.woff[g], a.wld[g]};
  }
  contract_tile<DIMP>(P, a.slots, R, C, t, a.tr, a.tc, w, id, a.partial);
}

}  // namespace

void agp::launch_sparse_contract(hipStream_t s, const DevProgram *P, const FeatView &R, const FeatView &C, const SparseContractArgs &a,
                            long long tiles) {
  if (tiles <= 0) return;
  dispatch_dim(R.dim, [&](auto D) {
    hipLaunchKernelGGL(sparse_contract_kernel<decltype(D)::value>, dim3((unsigned)tiles), dim3(CT_THREADS), 0, s, P, R, C, a);
  });
}

namespace {

// out[g] = -1/2 S_blocks[g] - S_fu[g] - 1/2 S_uu[g], every S the sum of its tiles' partials in a fixed order
// (reduce_partials); one workgroup per slot of the group.  The signs: the weights held are -bd(G), -(H E)^T, -W_uu.
__global__ __launch_bounds__(256) void sparse_grad_reduce_kernel(const double *__restrict__ p0, long long t0,
                                                                 const double *__restrict__ p1, long long t1,
                                                                 const double *__restrict__ p2, long long t2, int count,
                                                                 double *__restrict__ out) {
  const int g = blockIdx.x;
  if (g >= count) return;
  const double *parts[3] = {p0, p1, p2};
  const long long tiles[3] = {t0, t1, t2};
  const double scale[3] = {-0.5, -1.0, -0.5};
  double total = 0.;
  for (int q = 0; q < 3; ++q) {
    total += scale[q] * reduce_partials(parts[q], tiles[q], g);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[g] = total;
}

}  // namespace

void agp::launch_sparse_grad_reduce(hipStream_t s, const double *p0, long long t0, const double *p1, long long t1, const double *p2,
                               long long t2, int count, double *out) {
  hipLaunchKernelGGL(sparse_grad_reduce_kernel, dim3(GRAD_GROUP), dim3(256), 0, s, p0, t0, p1, t1, p2, t2, count, out);
}

namespace {

// ---- what agp_sparse_nll_gradient and agp_sparse_held_out share: the group tables and, per group, R_g = L_g^-1 and the
// lower triangle of bd(Kt^-1)_g = R_g^T R_g - N_g^T N_g in s_g x s_g slabs (h_roff / h_rld), for all three layouts of the
// fit's blocks (SparseScratch::layout) --------------------------------------------------------------------------------
struct InverseBlocks {
  std::vector<long long> tab;  // off | roff | rld | tstart, G + 1 entries each
  long long *h_off = nullptr, *h_roff = nullptr, *h_rld = nullptr, *h_tstart = nullptr;
  DevMem<long long> d_tab;
  const long long *d_off = nullptr, *d_roff = nullptr, *d_rld = nullptr, *d_tstart = nullptr;
  DevMem<double> Rg, Bg;
  long long smax = 0, lda_b = 0, stride_A = 0, stride_I = 0, r_elems = 0, tiles_blocks = 0;
  bool uniform = false, slabbed = false;
  double *Nm = nullptr;  // N (m x n, ld round_up(m, 2)): in the fit's pool
};

// group tables: offsets, where each group's s_g x s_g slab starts and its leading dimension, first tile; the slabs; the
// upload of the tables (asynchronous, from b.tab: the caller synchronises before b goes away)
int inverse_blocks_begin(agp_context_impl *ctx, const SparseScratch &w, long long G, const int64_t *offsets, long long n,
                         InverseBlocks &b) {
  hipStream_t s = ctx->stream;
  for (long long g = 0; g < G; ++g) b.smax = std::max<long long>(b.smax, offsets[g + 1] - offsets[g]);
  const long long smax = b.smax;
  b.uniform = w.layout == 0;
  b.slabbed = w.layout != 2;
  b.lda_b = factor_ld(smax);
  b.stride_A = b.lda_b * smax;
  b.stride_I = ((smax + NB - 1) / NB) * (36 * MB * MB);
  b.tab.resize(4 * (size_t)(G + 1));
  b.h_off = b.tab.data(); b.h_roff = b.h_off + (G + 1); b.h_rld = b.h_roff + (G + 1); b.h_tstart = b.h_rld + (G + 1);
  for (long long g = 0; g < G; ++g) {
    const long long sg = offsets[g + 1] - offsets[g];
    b.h_off[g] = offsets[g];
    b.h_rld[g] = b.slabbed ? b.lda_b : factor_ld(sg);
    b.h_roff[g] = b.slabbed ? g * b.stride_A : b.r_elems;
    b.r_elems = b.slabbed ? (g + 1) * b.stride_A : b.r_elems + b.h_rld[g] * sg;
    b.h_tstart[g] = b.tiles_blocks;
    b.tiles_blocks += lower_tiles(sg);
  }
  b.h_off[G] = n; b.h_roff[G] = b.r_elems; b.h_rld[G] = 0; b.h_tstart[G] = b.tiles_blocks;
  AGP_HIP_CHECK(ctx, b.d_tab.alloc_cached(sizeof(long long) * b.tab.size()));
  b.d_off = b.d_tab; b.d_roff = b.d_off + (G + 1); b.d_rld = b.d_roff + (G + 1); b.d_tstart = b.d_rld + (G + 1);
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(b.d_tab, b.tab.data(), sizeof(long long) * b.tab.size(), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, b.Rg.alloc_cached(sizeof(double) * (size_t)round_up(b.r_elems, 2)));
  AGP_HIP_CHECK(ctx, b.Bg.alloc_cached(sizeof(double) * (size_t)round_up(b.r_elems, 2)));
  return AGP_OK;
}

// R_g = L_g^-1, aw = y_w - W^T v, alpha_g = R_g^T aw_g, Z = Lacc^-1 W, N_g = -Z_g R_g and the lower triangle of
// bd(Kt^-1)_g = R_g^T R_g - N_g^T N_g into b.Bg.  aw, alpha: n doubles each.  Stops before the E^T backward solve.
int inverse_blocks_run(agp_context_impl *ctx, SparseScratch &w, const agp_sparse_fit *fit, const int64_t *offsets, long long G,
                       long long n, long long m, const double *yw, double *aw, double *alpha, InverseBlocks &b, StageTimer &stage) {
  hipStream_t s = ctx->stream;
  const long long ldk = round_up(m, 2), smax = b.smax, lda_b = b.lda_b, stride_A = b.stride_A, stride_I = b.stride_I;
  const long long *h_roff = b.h_roff, *h_rld = b.h_rld;
  double *Rg = b.Rg.get(), *Bg = b.Bg.get();
  // once per group, or once for all groups when they advance in lock step (blockIdx.y = group)
  auto per_group = [&](auto &&fn) {
    if (b.uniform) { fn(0LL, smax, G); return; }
    for (long long g = 0; g < G; ++g) fn(g, offsets[g + 1] - offsets[g], 1LL);
  };

  // ---- R_g = L_g^-1 for every block of A ----
  if (b.slabbed) {
    launch_set_identity_batched(s, Rg, lda_b, stride_A, smax, G);
    forward_solve_mat_batched(s, w.Ag, stride_A, smax, lda_b, w.Pimg, stride_I, Rg, stride_A, smax, lda_b, /*rhs_lower=*/true, G);
  } else {
    for (long long g = 0; g < G; ++g) {
      const long long sg = offsets[g + 1] - offsets[g];
      const agp_fit *blk = w.blocks[(size_t)g];
      launch_set_identity(s, Rg + h_roff[g], h_rld[g], sg);
      forward_solve_mat(s, blk->A, sg, blk->lda, blk->invd, Rg + h_roff[g], sg, h_rld[g], /*rhs_lower=*/true);
    }
  }
  // ---- alpha = A^-1 (y - K_fu v) = L^-T (y_w - W^T v) ----
  launch_colvec_dot(s, w.Kuf, ldk, m, n, fit->v, -1.0, 1.0, yw, aw);
  hipLaunchKernelGGL(group_rt_vec_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, Rg, b.d_off, b.d_roff, b.d_rld, G, n, aw, alpha);
  stage("gradient: R_g, alpha");

  // ---- Z = Lacc^-1 W = L2^-1 Q1_W, then N_g = -Z_g R_g ----
  const agp_fit *L2 = fit->sigma2;
  double *Q1W = w.Q1T + (size_t)ldk * (size_t)m, *Z = nullptr, *Nm = nullptr;
  if (forward_solve_wide_ok(m, n)) {  // out of place into W's buffer (W is dead: aw has been formed)
    if (!w.Winv) AGP_HIP_CHECK(ctx, w.Winv.alloc_cached(sizeof(double) * (size_t)m * (size_t)WIDE_BW));
    invert_wide_blocks(s, L2->A, m, L2->lda, L2->invd, WIDE_BW, w.Winv);
    forward_solve_wide(s, L2->A, m, L2->lda, w.Winv, Q1W, ldk, w.Kuf, ldk, n);
    Z = w.Kuf; Nm = w.Q1T;
  } else {
    forward_solve_mat(s, L2->A, m, L2->lda, L2->invd, Q1W, n, ldk);
    Z = Q1W; Nm = w.Kuf;
  }
  AGP_HIP_CHECK(ctx, hipMemsetAsync(Nm, 0, sizeof(double) * (size_t)ldk * (size_t)n, s));
  per_group([&](long long g, long long sg, long long cnt) {
    const size_t o = (size_t)offsets[g] * (size_t)ldk;
    launch_gemm_nt_sub_batched(s, Nm + o, ldk, sg * ldk, Z + o, ldk, false, sg * ldk, Rg + h_roff[g], h_rld[g], true, stride_A, m, sg, sg,
                               false, cnt);
  });
  stage("gradient: Z, N = -Z R");

  // ---- bd(Kt^-1)_g = R_g^T R_g - N_g^T N_g (lower triangle) ----
  per_group([&](long long g, long long sg, long long cnt) {
    const size_t o = (size_t)offsets[g] * (size_t)ldk;
    launch_rtr_lower_batched(s, Rg + h_roff[g], h_rld[g], stride_A, sg, Bg + h_roff[g], h_rld[g], stride_A, cnt);
    launch_gemm_nt_sub_batched(s, Bg + h_roff[g], h_rld[g], stride_A, Nm + o, ldk, true, sg * ldk, Nm + o, ldk, true, sg * ldk, sg, sg, m,
                               true, cnt);
  });
  b.Nm = Nm;
  return AGP_OK;
}

// ---- agp_sparse_held_out: the kernels around the value chain of a chunk of groups (gradient.hip: logo_chunk_sigma,
// logo_chunk_terms).  A chunk holds `count` groups padded to m points; the points of chunk group q are the grouped
// positions idx[q * m] .. idx[q * m] + sizes[q] - 1 (the held-out groups are the fit's own: contiguous). --------------------

// X0_q = [B_g 0; 0 I], B_g = bd(Kt^-1)_g mirrored from the lower triangle of the group's slab: column blockIdx.x of chunk
// group blockIdx.y.  Stands where logo_gather_blocks_kernel stands in the dense chain.
__global__ __launch_bounds__(256) void held_out_load_kernel(const double *__restrict__ Bg, const long long *__restrict__ off,
                                                            const long long *__restrict__ roff, const long long *__restrict__ rld,
                                                            long long G, const long long *__restrict__ idx,
                                                            const long long *__restrict__ sizes, long long m,
                                                            double *__restrict__ X0, long long ldb, long long stride) {
  const long long c = blockIdx.x, q = blockIdx.y, sz = sizes[q];
  const long long g = find_group(off, G, idx[q * m]), ld = rld[g];
  const double *b = Bg + roff[g];
  double *out = X0 + q * stride + c * ldb;
  for (long long r = threadIdx.x; r < m; r += 256)
    out[r] = (r < sz && c < sz) ? (r >= c ? b[r + c * ld] : b[c + r * ld]) : (r == c ? 1. : 0.);
}

// Mn_q = M_g + nugget I, M_g = k(Measurement x_g, Measurement x_g) - k(x_g, x_g): the part of the covariance function that
// only measurements carry, pair by pair with the argument order of the symmetric Gram call that built the blocks of A
// (k(x_i, x_j) for i >= j, mirrored).  Zero in the padding.  Column blockIdx.x of chunk group blockIdx.y.
template <int DIMP>
__global__ __launch_bounds__(256) void held_out_correction_kernel(const DevProgram *__restrict__ P, FeatView X,
                                                                  const long long *__restrict__ idx,
                                                                  const long long *__restrict__ sizes, long long m, double nugget,
                                                                  double *__restrict__ Mn, long long ldb, long long stride) {
  const long long c = blockIdx.x, q = blockIdx.y, sz = sizes[q], base = idx[q * m];
  double *out = Mn + q * stride + c * ldb;
  if (c >= sz) {  // (the whole workgroup)
    for (long long r = threadIdx.x; r < m; r += 256) out[r] = 0.;
    return;
  }
  const bool need_norm = (P->metric_mask & ((1 << AGP_METRIC_RADIAL) | (1 << AGP_METRIC_ANGULAR))) != 0;
  const bool have_ids = X.ids != nullptr;
  Point<DIMP> pc;
  load_point<DIMP>(X, base + c, need_norm, pc);
  for (long long r = threadIdx.x; r < m; r += 256) {
    double v = 0.;
    if (r < sz) {
      Point<DIMP> pr;
      load_point<DIMP>(X, base + r, need_norm, pr);
      const bool swapped = r < c;
      v = eval_pair<DIMP>(P, pr, pc, swapped, have_ids, true) - eval_pair<DIMP>(P, pr, pc, swapped, have_ids, false);
      if (r == c) v += nugget;
    }
    out[r] = v;
  }
}

// fixed-order sum of one value per thread over a workgroup of 256 (every thread receives it)
__device__ __forceinline__ double block_sum_256(double acc, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// X2_q holds -Sigma_q (Sigma = B^-1; the identity in the padding).  Column c of chunk group q:
//   d_c = (Sigma alpha_g)_c,   V_q = Sigma_q - Mn_q  (= cov_g + diag(y_var_g); the identity in the padding)
// Joint (MARGINAL = false): V into X0 and d into d and z, for the second LL^T with z riding along.
// Marginal: v_c = V_cc, the column's share log v_c + d_c^2 / v_c of 2 NLL_g into t.
// Both, where the pointer is given: mean = y - d, variance = V_cc - y_var, the column of cov_g = V_g - diag(y_var_g) into
// the group's block of joint (joff[q]: where it starts).
template <bool MARGINAL>
__global__ __launch_bounds__(256) void held_out_sigma_kernel(const double *__restrict__ X2, const double *__restrict__ Mn,
                                                             const long long *__restrict__ idx, const long long *__restrict__ sizes,
                                                             long long m, long long ldb, long long stride,
                                                             const double *__restrict__ alpha, const double *__restrict__ y,
                                                             const double *__restrict__ yvar, double *__restrict__ X0,
                                                             double *__restrict__ d, double *__restrict__ z, double *__restrict__ t,
                                                             double *__restrict__ mean, double *__restrict__ variance,
                                                             double *__restrict__ joint, const long long *__restrict__ joff) {
  __shared__ double red[4];
  const long long c = blockIdx.x, q = blockIdx.y, sz = sizes[q], base = idx[q * m];
  const long long off = q * stride + c * ldb;
  const bool valid = c < sz;
  const double sc = (yvar && valid) ? yvar[base + c] : 0.;
  double *jcol = (joint && valid) ? joint + joff[q] + c * sz : nullptr;
  double acc = 0.;
  for (long long r = threadIdx.x; r < m; r += 256) {
    const double sg = -X2[off + r];
    acc += sg * (r < sz ? alpha[base + r] : 0.);
    const double v = sg - Mn[off + r];
    if (!MARGINAL) X0[off + r] = v;
    if (jcol && r < sz) jcol[r] = r == c ? v - sc : v;
  }
  const double dc = block_sum_256(acc, red);
  if (threadIdx.x != 0) return;
  const double vc = -X2[off + c] - Mn[off + c];
  d[q * m + c] = dc;
  if (MARGINAL) t[q * m + c] = log(vc) + dc * (dc / vc);
  else z[q * m + c] = dc;
  if (!valid) return;
  if (mean) mean[base + c] = y[base + c] - dc;
  if (variance) variance[base + c] = vc - sc;
}

}  // namespace

extern "C" {

int agp_sparse_nll_gradient(agp_context *c, const agp_kernel *k, const agp_features *x, int64_t n_groups,
                            const int64_t *offsets, const double *y, const double *y_var, const agp_features *u,
                            double measurement_nugget, double inducing_nugget, int n_slots, const agp_gradient_slot *slots,
                            const double *tangents_x, int64_t ldtx, const double *tangents_u, int64_t ldtu, double *nll,
                            double *grad_nll, double *grad_nuggets, double *alpha_out) {
  if (!c || !k || !x || !u || !y || !offsets || !nll || n_groups <= 0) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && (!slots || !grad_nll))) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto fail = [&](int code) {
    *nll = nan;
    for (int j = 0; j < n_slots; ++j) grad_nll[j] = nan;
    if (grad_nuggets) grad_nuggets[0] = grad_nuggets[1] = nan;
    return code;
  };
  int st = AGP_OK, ntc = 0;
  if ((st = check_slots(k, n_slots, slots, &ntc)) != AGP_OK) return st;
  if (ntc > 0 && (!tangents_x || ldtx < x->n || !tangents_u || ldtu < u->n)) return AGP_ERR_INVALID_ARGUMENT;

  // ---- the fit, exactly as agp_sparse_nll makes it on the LL^T / CholeskyQR2 path (no pivoted fallback: the gradient
  // of a pseudo-inverse is not what a tuner wants) ----
  SparseScratch w;
  w.keep_P = true;
  agp_sparse_fit *fit_raw = nullptr;
  double *yw = nullptr, nll_v = 0.;
  st = sparse_fit_fast(ctx, k, x, n_groups, offsets, y, y_var, u, measurement_nugget, inducing_nugget, &fit_raw, &nll_v, &w, &yw);
  std::unique_ptr<agp_sparse_fit, void (*)(agp_sparse_fit *)> fit(fit_raw, agp_sparse_fit_destroy);
  if (st == AGP_ERR_INVALID_ARGUMENT) return st;
  if (st != AGP_OK) return fail(st);

  hipStream_t s = ctx->stream;
  StageTimer stage(s, getenv("AGP_SPARSE_TIMING") != nullptr);
  const long long n = x->n, m = u->n, G = n_groups;
  const long long ldk = round_up(m, 2), ldm = factor_ld(m), np2 = round_up(n, 2), mp2 = round_up(m, 2);
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return fail(st);
  FeatView xm = w.dx.v;
  xm.meas = 1;
  const FeatView uv = fit->u->v;

  // ---- group tables, R_g and bd(Kt^-1)_g slabs ----
  InverseBlocks ib;
  if ((st = inverse_blocks_begin(ctx, w, G, offsets, n, ib)) != AGP_OK) return st;
  const long long tiles_blocks = ib.tiles_blocks;
  const long long *d_off = ib.d_off, *d_roff = ib.d_roff, *d_rld = ib.d_rld, *d_tstart = ib.d_tstart;
  double *Bg = ib.Bg.get();
  const long long tiles_r = (m + CT - 1) / CT, tiles_fu = tiles_r * ((n + CT - 1) / CT), tiles_uu = lower_tiles(m);
  if (tiles_blocks > 0x7fffffffLL || tiles_fu > 0x7fffffffLL) return fail(AGP_ERR_INVALID_ARGUMENT);

  // ---- device buffers beyond the pool ----
  DevMem<double> Wn, vec;
  AGP_HIP_CHECK(ctx, Wn.alloc_cached(sizeof(double) * (size_t)ldm * (size_t)m));
  const bool tx_copy = ntc > 0 && x->location == AGP_HOST, tu_copy = ntc > 0 && u->location == AGP_HOST;
  const size_t part_elems = (size_t)(tiles_blocks + tiles_fu + tiles_uu) * GRAD_GROUP;
  const size_t vec_elems = 3 * (size_t)np2 + (size_t)mp2 + 8 + (size_t)round_up(AGP_MAX_GRADIENT_SLOTS, 2) + part_elems +
                           (tx_copy ? (size_t)np2 * (size_t)ntc : 0) + (tu_copy ? (size_t)mp2 * (size_t)ntc : 0);
  AGP_HIP_CHECK(ctx, vec.alloc_cached(sizeof(double) * vec_elems));
  double *aw = vec, *alpha = aw + np2, *diag = alpha + np2, *q = diag + np2, *scal = q + mp2, *grad_d = scal + 8;
  double *part_blocks = grad_d + round_up(AGP_MAX_GRADIENT_SLOTS, 2), *part_fu = part_blocks + (size_t)tiles_blocks * GRAD_GROUP,
         *part_uu = part_fu + (size_t)tiles_fu * GRAD_GROUP, *tcopy = part_uu + (size_t)tiles_uu * GRAD_GROUP;
  const double *tang_x = nullptr, *tang_u = nullptr;
  long long ld_tx = 0, ld_tu = 0;
  if ((st = stage_tangents(ctx, s, tangents_x, ldtx, x->location, n, ntc, &tcopy, &tang_x, &ld_tx)) != AGP_OK) return st;
  if ((st = stage_tangents(ctx, s, tangents_u, ldtu, u->location, m, ntc, &tcopy, &tang_u, &ld_tu)) != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // (pageable sources)

  // ---- R_g, alpha, Z, N_g and the lower triangles of bd(Kt^-1)_g ----
  if ((st = inverse_blocks_run(ctx, w, fit.get(), offsets, G, n, m, yw, aw, alpha, ib, stage)) != AGP_OK) return st;
  double *Nm = ib.Nm;
  const long long stride_A = ib.stride_A;
  const long long *h_roff = ib.h_roff, *h_rld = ib.h_rld;
  const bool uniform = ib.uniform;
  const long long smax = ib.smax;
  auto per_group = [&](auto &&fn) {
    if (uniform) { fn(0LL, smax, G); return; }
    for (long long g = 0; g < G; ++g) fn(g, offsets[g + 1] - offsets[g], 1LL);
  };
  // ---- -bd(G)_g = alpha_g alpha_g^T - bd(Kt^-1)_g (both triangles) and the diagonal of bd(G) ----
  hipLaunchKernelGGL(group_weight_kernel, dim3((unsigned)n), dim3(256), 0, s, Bg, d_off, d_roff, d_rld, G, alpha, diag);
  stage("gradient: bd(G) slabs");

  // ---- E^T = K_uu^-1 K_uf = L_u^-T P in place, q = E^T alpha ----
  double *Et = w.Pbuf;
  backward_solve_mat(s, fit->kuu->A, m, fit->kuu->lda, fit->kuu->invd, Et, n, ldk);
  launch_matvec(s, Et, ldk, m, n, alpha, w.partial, 1.0, 0.0, nullptr, q);
  stage("gradient: E^T = L_u^-T P");

  // ---- -(H E)^T = Lacc^-T N + [E_g^T bd(G)_g]_g + q alpha^T, in place over N (Lacc^-T = L1^-T L2^-T) ----
  const agp_fit *L1 = fit->sigma, *L2 = fit->sigma2;
  backward_solve_mat(s, L2->A, m, L2->lda, L2->invd, Nm, n, ldk);
  backward_solve_mat(s, L1->A, m, L1->lda, L1->invd, Nm, n, ldk);
  stage("gradient: Lacc^-T N");
  per_group([&](long long g, long long sg, long long cnt) {
    const size_t o = (size_t)offsets[g] * (size_t)ldk;
    launch_gemm_nt_sub_batched(s, Nm + o, ldk, sg * ldk, Et + o, ldk, false, sg * ldk, Bg + h_roff[g], h_rld[g], false, stride_A, m, sg, sg,
                               false, cnt);
  });
  hipLaunchKernelGGL(rank_one_add_kernel, dim3((unsigned)n, (unsigned)((m + 255) / 256)), dim3(256), 0, s, Nm, ldk, m, q, alpha);
  stage("gradient: (H E)^T");

  // ---- -W_uu = E^T (H E): lower tiles, summed over the observations through the fit's split-K slabs ----
  AGP_HIP_CHECK(ctx, hipMemsetAsync(Wn, 0, sizeof(double) * (size_t)ldm * (size_t)m, s));
  gemm_over_observations(s, w, Wn, ldm, Et, Nm, ldk, m, n);
  hipLaunchKernelGGL(strided_sum_kernel, dim3(1), dim3(1024), 0, s, diag, n, 1LL, 0.5, scal);           // 1/2 trace(bd(G))
  hipLaunchKernelGGL(strided_sum_kernel, dim3(1), dim3(1024), 0, s, Wn, m, ldm + 1, -0.5, scal + 1);    // 1/2 trace(W_uu)
  stage("gradient: W_uu = -E^T H E");

  // ---- the three contractions, GRAD_GROUP slots per pass ----
  for (int g0 = 0; g0 < n_slots; g0 += GRAD_GROUP) {
    SparseContractArgs ca;
    std::memset(static_cast<void *>(&ca), 0, sizeof(ca));
    bool scaling[GRAD_GROUP];
    const int cnt = fill_slot_group(k, n_slots, slots, g0, ca.slots, scaling);
    const double *col_x[GRAD_GROUP], *col_u[GRAD_GROUP];
    for (int j = 0; j < GRAD_GROUP; ++j) {
      col_x[j] = scaling[j] ? tang_x + (size_t)ca.slots.param[j] * (size_t)ld_tx : nullptr;
      col_u[j] = scaling[j] ? tang_u + (size_t)ca.slots.param[j] * (size_t)ld_tu : nullptr;
    }
    ca.off = d_off; ca.woff = d_roff; ca.wld = d_rld; ca.tstart = d_tstart; ca.G = G; ca.tiles_r = tiles_r;
    // group blocks: (measurement, measurement) pairs of the observations
    for (int j = 0; j < GRAD_GROUP; ++j) ca.tr[j] = ca.tc[j] = col_x[j];
    ca.W = Bg; ca.ldw = 0; ca.partial = part_blocks; ca.mode = 2;
    launch_sparse_contract(s, dprog, xm, xm, ca, tiles_blocks);
    // k(u, x): (plain, measurement)
    for (int j = 0; j < GRAD_GROUP; ++j) { ca.tr[j] = col_u[j]; ca.tc[j] = col_x[j]; }
    ca.W = Nm; ca.ldw = ldk; ca.partial = part_fu; ca.mode = 0;
    launch_sparse_contract(s, dprog, uv, xm, ca, tiles_fu);
    // k(u, u): (plain, plain)
    for (int j = 0; j < GRAD_GROUP; ++j) ca.tr[j] = ca.tc[j] = col_u[j];
    ca.W = Wn; ca.ldw = ldm; ca.partial = part_uu; ca.mode = 1;
    launch_sparse_contract(s, dprog, uv, uv, ca, tiles_uu);
    launch_sparse_grad_reduce(s, part_blocks, tiles_blocks, part_fu, tiles_fu, part_uu, tiles_uu, cnt, grad_d + g0);
  }
  stage("gradient: contractions");

  AGP_HIP_CHECK(ctx, hipGetLastError());
  double h_scal[2] = {nan, nan};
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_scal, scal, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_slots > 0) AGP_HIP_CHECK(ctx, hipMemcpyAsync(grad_nll, grad_d, sizeof(double) * (size_t)n_slots, hipMemcpyDeviceToHost, s));
  if (alpha_out) AGP_HIP_CHECK(ctx, hipMemcpyAsync(alpha_out, alpha, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (grad_nuggets) { grad_nuggets[0] = h_scal[0]; grad_nuggets[1] = h_scal[1]; }
  *nll = nll_v;
  return AGP_OK;
}

int agp_sparse_held_out(agp_context *c, const agp_kernel *k, const agp_features *x, int64_t n_groups, const int64_t *offsets,
                        const double *y, const double *y_var, const agp_features *u, double measurement_nugget,
                        double inducing_nugget, int predict_type, double *logo_nll, double *group_nll, double *mean,
                        double *variance, double *joint) {
  if (!c || !k || !x || !u || !y || !offsets || n_groups <= 0) return AGP_ERR_INVALID_ARGUMENT;
  if (predict_type != AGP_PREDICT_JOINT && predict_type != AGP_PREDICT_MARGINAL) return AGP_ERR_INVALID_ARGUMENT;
  const bool marginal = predict_type == AGP_PREDICT_MARGINAL;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  const long long n = x->n, m = u->n, G = n_groups;
  // the offsets as the fit checks them, here so that nothing has been written when they are malformed
  if (n <= 0 || m <= 0 || offsets[0] != 0 || offsets[G] != n) return AGP_ERR_INVALID_ARGUMENT;
  size_t joint_total = 0;
  for (long long g = 0; g < G; ++g) {
    const long long sg = offsets[g + 1] - offsets[g];
    if (sg <= 0 || offsets[g + 1] > n) return AGP_ERR_INVALID_ARGUMENT;
    joint_total += (size_t)sg * (size_t)sg;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const bool on_host = x->location == AGP_HOST;
  hipStream_t s = ctx->stream;
  auto fill_nan = [&](double *out, size_t count) {
    if (!out) return;
    if (on_host) std::fill(out, out + count, nan);
    else launch_axpby(s, (long long)count, 0., nullptr, nan, nullptr, out);
  };
  auto fail = [&](int code) {
    if (logo_nll) *logo_nll = nan;
    if (group_nll) std::fill(group_nll, group_nll + G, nan);
    fill_nan(mean, (size_t)n);
    fill_nan(variance, (size_t)n);
    fill_nan(joint, joint_total);
    if (!on_host) (void)hipStreamSynchronize(s);
    return code;
  };

  // ---- the fit, on the LL^T / CholeskyQR2 path only, as agp_sparse_nll_gradient makes it ----
  SparseScratch w;
  w.keep_P = true;
  agp_sparse_fit *fit_raw = nullptr;
  double *yw = nullptr, nll_v = 0.;
  int st = sparse_fit_fast(ctx, k, x, n_groups, offsets, y, y_var, u, measurement_nugget, inducing_nugget, &fit_raw, &nll_v, &w, &yw);
  std::unique_ptr<agp_sparse_fit, void (*)(agp_sparse_fit *)> fit(fit_raw, agp_sparse_fit_destroy);
  if (st == AGP_ERR_INVALID_ARGUMENT) return st;
  if (st != AGP_OK) return fail(st);

  StageTimer stage(s, getenv("AGP_SPARSE_TIMING") != nullptr);
  const long long np2 = round_up(n, 2);
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return fail(st);
  FeatView xm = w.dx.v;
  xm.meas = 1;

  // ---- the chunks of groups (the indices are the grouped positions themselves) and the workspace ----
  LogoPlan plan;
  {
    std::vector<int64_t> identity((size_t)n);
    for (long long i = 0; i < n; ++i) identity[(size_t)i] = i;
    if ((st = logo_plan(n, n_groups, offsets, identity.data(), plan)) != AGP_OK) return st;
  }
  std::vector<long long> joff;  // term q (the plan's order): where the block of its group starts in joint
  if (joint) {
    std::vector<long long> start((size_t)G);
    long long at = 0;
    for (long long g = 0; g < G; ++g) { start[(size_t)g] = at; at += (offsets[g + 1] - offsets[g]) * (offsets[g + 1] - offsets[g]); }
    for (long long q = 0; q < plan.terms; ++q) joff.push_back(start[(size_t)plan.group[(size_t)q]]);
  }
  const size_t term_elems = (size_t)round_up(plan.terms, 2);
  auto carve = [&](WsLayout &ws) {
    return carve_sparse_held_out(ws, (size_t)np2, plan.block_elems, plan.img_elems, plan.vec_elems, plan.count_elems, term_elems,
                                 plan.meta.size(), mean != nullptr, y_var && (variance || joint), mean != nullptr,
                                 variance != nullptr, joint ? joint_total : 0);
  };
  WsLayout size_own;
  carve(size_own);
  DevMem<void> own_mem;
  AGP_HIP_CHECK(ctx, own_mem.alloc_cached(size_own.bytes()));
  WsLayout own(own_mem.get());
  const SparseHeldOutRegions r = carve(own);
  InverseBlocks ib;
  if ((st = inverse_blocks_begin(ctx, w, G, offsets, n, ib)) != AGP_OK) return st;
  const hipMemcpyKind in_kind = on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(r.chain.meta, plan.meta.data(), sizeof(long long) * plan.meta.size(), hipMemcpyHostToDevice, s));
  if (r.joff) AGP_HIP_CHECK(ctx, hipMemcpyAsync(r.joff, joff.data(), sizeof(long long) * joff.size(), hipMemcpyHostToDevice, s));
  if (r.y) AGP_HIP_CHECK(ctx, hipMemcpyAsync(r.y, y, sizeof(double) * (size_t)n, in_kind, s));
  if (r.yvar) AGP_HIP_CHECK(ctx, hipMemcpyAsync(r.yvar, y_var, sizeof(double) * (size_t)n, in_kind, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // (pageable sources)

  // ---- R_g, alpha, Z, N_g and B_g = bd(Kt^-1)_g ----
  if ((st = inverse_blocks_run(ctx, w, fit.get(), offsets, G, n, m, yw, r.aw, r.alpha, ib, stage)) != AGP_OK) return st;
  stage("held out: bd(Kt^-1) slabs");

  // ---- per chunk: B_g -> Sigma_g = B_g^-1 -> V_g = Sigma_g - nugget I - M_g -> the NLL terms and the predictions ----
  AGP_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), s));
  for (const LogoChunk &ch : plan.chunks) {
    const long long cm = ch.m, ldb = factor_ld(cm), stride_B = ldb * cm;
    const long long *idx = r.chain.meta + ch.idx_off, *sizes = r.chain.meta + ch.size_off;
    const dim3 cols((unsigned)cm, (unsigned)ch.count);
    hipLaunchKernelGGL(held_out_load_kernel, cols, dim3(256), 0, s, ib.Bg.get(), ib.d_off, ib.d_roff, ib.d_rld, G, idx, sizes, cm,
                       r.chain.X0, ldb, stride_B);
    logo_chunk_sigma(ctx, r.chain, ch);
    dispatch_dim(xm.dim, [&](auto D) {
      hipLaunchKernelGGL(held_out_correction_kernel<decltype(D)::value>, cols, dim3(256), 0, s, dprog, xm, idx, sizes, cm,
                         measurement_nugget, r.M, ldb, stride_B);
    });
    const long long *jo = r.joff ? r.joff + ch.term_off : nullptr;
    if (marginal)
      hipLaunchKernelGGL(held_out_sigma_kernel<true>, cols, dim3(256), 0, s, r.chain.X2, r.M, idx, sizes, cm, ldb, stride_B, r.alpha, r.y,
                         r.yvar, r.chain.X0, r.chain.d, r.chain.z, r.chain.a_pad, r.mean, r.variance, r.joint, jo);
    else
      hipLaunchKernelGGL(held_out_sigma_kernel<false>, cols, dim3(256), 0, s, r.chain.X2, r.M, idx, sizes, cm, ldb, stride_B, r.alpha, r.y,
                         r.yvar, r.chain.X0, r.chain.d, r.chain.z, r.chain.a_pad, r.mean, r.variance, r.joint, jo);
    logo_chunk_terms(ctx, r.chain, ch, marginal);
  }
  launch_logo_sum(s, r.chain.term, plan.terms, ctx->d_scalars + 2);
  stage("held out: group chains");

  AGP_HIP_CHECK(ctx, hipGetLastError());
  const hipMemcpyKind out_kind = on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  std::vector<double> h_term(group_nll ? (size_t)plan.terms : 0);
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_flags, ctx->d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (!h_term.empty()) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_term.data(), r.chain.term, sizeof(double) * h_term.size(), hipMemcpyDeviceToHost, s));
  if (mean) AGP_HIP_CHECK(ctx, hipMemcpyAsync(mean, r.mean, sizeof(double) * (size_t)n, out_kind, s));
  if (variance) AGP_HIP_CHECK(ctx, hipMemcpyAsync(variance, r.variance, sizeof(double) * (size_t)n, out_kind, s));
  if (joint) AGP_HIP_CHECK(ctx, hipMemcpyAsync(joint, r.joint, sizeof(double) * joint_total, out_kind, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if ((st = status_from_flags(ctx)) != AGP_OK) return fail(st);  // a B_g or (Joint) a V_g that is not positive definite
  if (logo_nll) *logo_nll = ctx->h_scalars[2];
  if (group_nll)  // the terms are in the plan's order (by size) and hold 2 NLL_g
    for (size_t q = 0; q < h_term.size(); ++q) group_nll[plan.group[q]] = 0.5 * h_term[q];
  return AGP_OK;
}

}  // extern "C"
