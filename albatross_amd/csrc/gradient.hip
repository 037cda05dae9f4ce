// gradient.hip — exact gradients of the tuner's objectives with respect to the covariance parameters.
//
// agp_nll_gradient, the negative log-likelihood:
//
//   dNLL / dtheta = 1/2 sum_ij W_ij dK_ij / dtheta,   W = K^-1 - alpha alpha^T,   alpha = K^-1 y
//
// The reference's tuner gets the gradient by forward differences of the log-likelihood (compute_gradient,
// tune/finite_difference.hpp:37-90): P + 1 evaluations for P parameters, accurate to the likelihood's error over eps.
// Here: one fit (build_and_factor, api.hip), R = L^-1 (forward_solve_mat_lookahead on a triangular right-hand side,
// as inverse_diagonal_device does), K^-1 = R^T R into the factor's buffer (rtr_lower_kernel below), and one contraction
// of W's lower triangle against the tangent form of the covariance program (contract.h: contract_tile, the body shared
// with sparse_gradient.hip).  Cost: a fit plus ~2 N^3 / 3 flop, whatever P is.
//
// agp_loo_nll_gradient, the leave-one-out likelihood metric (LeaveOneOutLikelihood, evaluation/model_metrics.hpp:59-72)
// and its gradient (GPML 5.4.2, eqs. 5.10-5.13, with the truth's variance s added as prediction_metrics.hpp:113-119 does):
// with C = K^-1 (K including diag(s)), c_i = C_ii, v_i = 1/c_i + s_i, d_i = alpha_i / c_i,
//
//   LOO = sum_i 1/2 (log v_i + d_i^2 / v_i + log 2 pi),   dLOO / dtheta = sum_ij W_ij dK_ij / dtheta,
//   W = C diag(b) C - 1/2 (u alpha^T + alpha u^T),   b_i = (1 - d_i^2/v_i + 2 alpha_i d_i) / (2 v_i c_i^2),
//   u = C a,   a_i = d_i / (v_i c_i).
//
// The same fit, alpha, R and C = R^T R; then loo_terms_kernel (per point: the NLL term, a, sqrt(b)), u by
// launch_symv_lower, G = diag(b)^1/2 sym(C) over R (loo_form_g_kernel), S = G^T G = C diag(b) C over C (gtg_lower_kernel:
// N^3 flop, the only O(N^3) work beyond agp_nll_gradient) and the contraction of W = S - sym(u alpha^T).
//
// agp_logo_nll_gradient, the leave-one-GROUP-out likelihood metric (LeaveOneGroupOutLikelihood, Joint predict type,
// evaluation/model_metrics.hpp:74-93) and its gradient: per group with index set I, A = C[I, I], Sigma = A^-1,
// d = Sigma alpha_I, V = Sigma + diag(s_I), NLL_g = 1/2 (log |V| + d^T V^-1 d + |I| log 2 pi), and with a_I = Sigma V^-1 d
//
//   W = C B C - 1/2 (u alpha^T + alpha u^T),   B = blockdiag(B_g),   u = C a,
//   B_g = 1/2 Sigma V^-1 Sigma - 1/2 a_I a_I^T + 1/2 (a_I d^T + d a_I^T).
//
// B_g is indefinite in general, so there is no G with G^T G = C B C: H = sym(C) B (logo_h_kernel), then S = H C^T
// (hct_lower_kernel, the N^3 product again, into a third slab).  The front end and the contraction are those of
// agp_loo_nll_gradient; the group blocks go through the batched LL^T / solve / product launches that
// agp_held_out_predictions uses (cv_api.hip), the groups sorted by size and cut into chunks of comparable size that
// advance in lock step (logo_plan, logo_chunk), with the small kernels below around them.
// agp_logo_nll_gradient_typed is the same entry with the score's predict type as an argument: AGP_PREDICT_MARGINAL scores
// each held-out group against the diagonal of V only (v_i = Sigma_ii + s_i, q_i = d_i / v_i, w_i = 1/2 (1 / v_i - q_i^2),
// a_I = Sigma q, B_g = Sigma diag(w) Sigma + 1/2 (a_I d^T + d a_I^T)): the chain up to Sigma_g is shared, then a per-column
// kernel and ONE two-operand block product replace the second LL^T, the second solve and T^T T.
//
// agp_nll_gradient_batch and agp_loo_nll_gradient_batch run the same steps for `count` problems of one size in lock step:
// every kernel below takes the problem from blockIdx.y (blockIdx.z where y is a tile index) and per-problem strides, and
// the single-problem calls are its count = 1 case.  Their checks, uploads, Gram and factor are the front end the batched
// fits share (batch_front.h); every workspace here is carved by a layout of batch_layout.h.
// agp_nll_gradient_batch_ragged and agp_loo_nll_gradient_batch_ragged are the same two bodies for problems of UNEQUAL sizes:
// problem b is diag(K_b, I) at the padded size of the call (ragged_batch.hip; gradient_batch_begin says what changes).
// agp_logo_nll_gradient_batch is agp_logo_nll_gradient_typed for problems of any mix of sizes on that front end: the group
// blocks of ALL problems go through ONE chain per size class of groups (the pooled plan of logo_batch_plan.h; the kernels
// around the chain take every group's problem from a table, LogoProblems).
#include <algorithm>
#include <climits>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "api_internal.h"
#include "batch_front.h"
#include "contract.h"
#include "contract_internal.h"
#include "cov_eval.h"
#include "gemm_tiles.h"
#include "logo_batch_plan.h"
#include "pub.h"

namespace agp {

// ---- C = R^T R, lower tiles, R lower triangular -----------------------------------------------------------------
// Tile (bi, bj), bi >= bj, of C sums R(k, i) R(k, j) over k >= i0 = bi * 128 only: R(k, i) = 0 for k < i.  Both
// operands are read k-major (element (row, k) at R[k + row * ldr], the TN product) through gemm_nt_sub_tile's 128 x 128
// body, with the operand pointers moved to row i0 of R and K = n - i0.  The workgroups of the first tile rows (the
// deepest products) are launched first.  Flop: N^3 / 3.  The whole diagonal tile is written; nothing reads its upper
// half.
__global__ __launch_bounds__(GEMM_THREADS, 2) void rtr_lower_kernel(GemmArgs g) {
  __shared__ double lds[2 * 2 * GK * GLD];
  int bi, bj;
  lower_tile(blockIdx.x, bi, bj);
  const long long k0 = (long long)bi * GT;
  const long long b = blockIdx.y;  // problem of a batched launch (batch_* = 0: one problem)
  GemmArgs t = g;
  t.C = g.C + b * g.batch_C;
  t.A = g.A + b * g.batch_A + k0;
  t.B = g.B + b * g.batch_B + k0;
  t.K = g.K - k0;
  gemm_nt_sub_tile<true, true, true>(t, bi, bj, lds);
}

// C_b = R_b^T R_b for `count` problems (blockIdx.y = problem): R_b = R + b * stride_R, C_b = C + b * stride_C.  Within
// each problem the deepest tile rows go first, as for one problem; count = 1 is launch_rtr_lower.
void launch_rtr_lower_batched(hipStream_t s, const double *R, long long ldr, long long stride_R, long long n, double *C,
                              long long ldc, long long stride_C, long long count) {
  if (n <= 0 || count <= 0) return;
  GemmArgs g;
  g.C = C; g.ldc = ldc; g.A = R; g.lda = ldr; g.B = R; g.ldb = ldr;
  g.M = n; g.N = n; g.K = n; g.tri = 1;
  g.ntr = g.ntc = (int)((n + GT - 1) / GT);
  g.assign = 1;  // C = + A B^T, C not read
  g.batch_C = stride_C; g.batch_A = g.batch_B = stride_R;
  const long long tiles = (long long)g.ntr * (g.ntr + 1) / 2;
  hipLaunchKernelGGL(rtr_lower_kernel, dim3((unsigned)tiles, (unsigned)count), dim3(GEMM_THREADS), 0, s, g);
}

void launch_rtr_lower(hipStream_t s, const double *R, long long ldr, long long n, double *C, long long ldc) {
  launch_rtr_lower_batched(s, R, ldr, 0, n, C, ldc, 0, 1);
}

// ---- contraction of a weight's lower triangle (contract.h): tile blockIdx.x of the row-major lower enumeration ----
// (ContractArgs: contract_internal.h)

// The body of both the single-problem kernel and the batched one.  LOO: the weight of agp_loo_nll_gradient in place of
// K^-1_ij - alpha_i alpha_j.
// The pairs are those of X.n points, whatever the grid was sized for: a problem of n_b rows in a batch of padded size n
// (ragged_batch.hip) hands in its view of n_b rows and so contracts no phantom pair - a phantom diagonal pair would carry
// the weight 1/2 against dK_ii / dtheta of whatever feature the row is read as.  A tile wholly behind X.n (bi CT >= X.n;
// bj <= bi) writes its zero partial, which the reduction sums with the rest, and leaves before it loads a point.
template <int DIMP, bool LOO>
__device__ __forceinline__ void contract_lower(const DevProgram *__restrict__ P, const FeatView &X, const ContractArgs &a) {
  ContractTile t;
  lower_tile(blockIdx.x, t.bi, t.bj);
  if ((long long)t.bi * CT >= X.n) {  // (the whole workgroup)
    if (threadIdx.x < GRAD_GROUP) a.partial[(long long)blockIdx.x * GRAD_GROUP + threadIdx.x] = 0.;
    return;
  }
  t.rbase = t.cbase = 0;
  t.nrl = t.ncl = X.n;
  t.lower = true;
  if constexpr (LOO) contract_tile<DIMP>(P, a.slots, X, X, t, a.tang, a.tang, LooWeight{a.C, a.ldc, a.alpha, a.u}, blockIdx.x, a.partial);
  else contract_tile<DIMP>(P, a.slots, X, X, t, a.tang, a.tang, NllWeight{a.C, a.ldc, a.alpha}, blockIdx.x, a.partial);
}

template <int DIMP, bool LOO = false>
__global__ __launch_bounds__(CT_THREADS) void nll_grad_contract_kernel(const DevProgram *__restrict__ P, FeatView X,
                                                                       ContractArgs a) {
  contract_lower<DIMP, LOO>(P, X, a);
}

// out[base + g] = scale * sum over tiles of partial[tile][g], in a fixed order; one workgroup per slot of the group
__global__ __launch_bounds__(256) void nll_grad_reduce_kernel(const double *__restrict__ partial, long long tiles, int count,
                                                              double scale, double *__restrict__ out) {
  const int g = blockIdx.x;
  if (g >= count) return;
  const double v = reduce_partials(partial, tiles, g);
  if (threadIdx.x == 0) out[g] = scale * v;
}

// ---- the batched contraction (agp_nll_gradient_batch, agp_loo_nll_gradient_batch) -----------------------------------
// One descriptor per problem, ContractDesc (contract_internal.h), built on the host for the call and uploaded with it.

// grid: x = tile, y = problem, z = slot group.  DIMP covers the batch's largest dimension (load_point zero-pads);
// problems with fewer slot groups leave their unused z-slices at once.  LOO: the weight of agp_loo_nll_gradient.
template <int DIMP, bool LOO = false>
__global__ __launch_bounds__(CT_THREADS) void nll_grad_contract_batched_kernel(const ContractDesc *__restrict__ D, long long tiles) {
  const ContractDesc &d = D[blockIdx.y];
  const int grp = blockIdx.z;
  if (grp * GRAD_GROUP >= d.n_slots) return;  // (the whole workgroup)
  ContractArgs a;
  a.slots = d.slots[grp];
#pragma unroll
  for (int g = 0; g < GRAD_GROUP; ++g) a.tang[g] = d.tang[grp * GRAD_GROUP + g];
  a.C = d.C; a.ldc = d.ldc; a.alpha = d.alpha; a.u = d.u;
  a.partial = d.partial + (long long)grp * tiles * GRAD_GROUP;
  const FeatView X = d.X;
  contract_lower<DIMP, LOO>(&d.prog, X, a);
}

// out[b * ldo + slot] = scale * sum over tiles of problem b's partials of that slot (one workgroup per (slot, problem))
__global__ __launch_bounds__(256) void nll_grad_reduce_batched_kernel(const ContractDesc *__restrict__ D, long long tiles,
                                                                      double scale, double *__restrict__ out, long long ldo) {
  const int slot = blockIdx.x;
  const long long b = blockIdx.y;
  const ContractDesc &d = D[b];
  if (slot >= d.n_slots) return;
  const double v = reduce_partials(d.partial + (long long)(slot / GRAD_GROUP) * tiles * GRAD_GROUP, tiles, slot % GRAD_GROUP);
  if (threadIdx.x == 0) out[b * ldo + slot] = scale * v;
}

template <bool LOO>
void launch_contract(hipStream_t s, const DevProgram *P, const FeatView &X, const ContractArgs &a, long long tiles) {
  dispatch_dim(X.dim, [&](auto D) {
    hipLaunchKernelGGL((nll_grad_contract_kernel<decltype(D)::value, LOO>), dim3((unsigned)tiles), dim3(CT_THREADS), 0, s, P, X, a);
  });
}
template void launch_contract<false>(hipStream_t, const DevProgram *, const FeatView &, const ContractArgs &, long long);
template void launch_contract<true>(hipStream_t, const DevProgram *, const FeatView &, const ContractArgs &, long long);

void launch_grad_reduce(hipStream_t s, const double *partial, long long tiles, int count, double scale, double *out) {
  hipLaunchKernelGGL(nll_grad_reduce_kernel, dim3(GRAD_GROUP), dim3(256), 0, s, partial, tiles, count, scale, out);
}

template <bool LOO>
void launch_contract_batched(hipStream_t s, int dim_max, const ContractDesc *D, long long tiles, long long count, int groups) {
  dispatch_dim(dim_max, [&](auto DIMP) {
    hipLaunchKernelGGL((nll_grad_contract_batched_kernel<decltype(DIMP)::value, LOO>), dim3((unsigned)tiles, (unsigned)count, (unsigned)groups),
                       dim3(CT_THREADS), 0, s, D, tiles);
  });
}
template void launch_contract_batched<false>(hipStream_t, int, const ContractDesc *, long long, long long, int);
template void launch_contract_batched<true>(hipStream_t, int, const ContractDesc *, long long, long long, int);

void launch_grad_reduce_batched(hipStream_t s, const ContractDesc *D, long long tiles, long long count, int groups, double scale,
                                double *out, long long ldo) {
  hipLaunchKernelGGL(nll_grad_reduce_batched_kernel, dim3((unsigned)(groups * GRAD_GROUP), (unsigned)count), dim3(256), 0, s, D, tiles, scale,
                     out, ldo);
}

// ---- leave-one-out terms -----------------------------------------------------------------------------------------
// Per point i, from c_i = cdiag[i * cstride] (C's diagonal in place, stride ldc + 1, or R's squared column norms) and
// alpha_i: term[i] = log v_i + d_i^2 / v_i (the NLL term without 1/2 and log 2 pi), a[i] = d_i / (v_i c_i) and
// sqrt_b[i] = sqrt(b_i); b_i > 0 always (c_i v_i >= 1).  a and sqrt_b may be nullptr (value only).  blockIdx.y = problem:
// its c starts at cdiag + b * cbatch, its vectors at b * vbatch (one problem: a grid of height 1).
// rows: the descriptors of a batch of unequal sizes, whose problem b has rows[b].X.n real rows of the n (nullptr: n for
// everybody).  A phantom row gets term = a = sqrt_b = 0 - the sum, the product C a and G read all n rows - and neither its
// c (1, from diag(C_b, I)) nor its target variance (never written) is looked at.
__device__ __forceinline__ long long real_rows(const ContractDesc *__restrict__ rows, long long n) {
  return rows ? rows[blockIdx.y].X.n : n;
}

__global__ __launch_bounds__(256) void loo_terms_kernel(const double *__restrict__ cdiag, long long cstride, long long cbatch,
                                                        const double *__restrict__ alpha, const double *__restrict__ yvar,
                                                        long long n, long long vbatch, double *__restrict__ term,
                                                        double *__restrict__ a, double *__restrict__ sqrt_b,
                                                        const ContractDesc *__restrict__ rows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long vb = (long long)blockIdx.y * vbatch;
  cdiag += (long long)blockIdx.y * cbatch;
  alpha += vb; term += vb;
  if (yvar) yvar += vb;
  if (a) a += vb;
  if (sqrt_b) sqrt_b += vb;
  if (i >= real_rows(rows, n)) {
    term[i] = 0.;
    if (a) a[i] = 0.;
    if (sqrt_b) sqrt_b[i] = 0.;
    return;
  }
  const double c = cdiag[i * cstride], al = alpha[i];
  const double v = 1. / c + (yvar ? yvar[i] : 0.);  // the LOO variance plus the truth's (prediction_metrics.hpp:113-119)
  const double d = al / c;                           // cross_validation_utils.hpp:146-163
  const double dv = d * d / v;
  term[i] = log(v) + dv;
  if (a) a[i] = d / (v * c);
  if (sqrt_b) sqrt_b[i] = sqrt((1. - dv + 2. * al * d) / (2. * v * c * c));
}

// out[b] = 1/2 (sum_i term_b[i] + n log 2 pi), term_b = term + b * tbatch, b = blockIdx.y   (one workgroup per problem,
// fixed order).  rows as in loo_terms_kernel: problem b sums its rows[b].X.n real terms and its n is that number.
__global__ __launch_bounds__(1024) void loo_sum_kernel(const double *__restrict__ term, long long n, long long tbatch,
                                                       double *__restrict__ out, const ContractDesc *__restrict__ rows) {
  __shared__ double red[16];
  n = real_rows(rows, n);
  term += (long long)blockIdx.y * tbatch;
  double acc = 0.;
  for (long long i = threadIdx.x; i < n; i += 1024) acc += term[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.;
    for (int w = 0; w < 16; ++w) s += red[w];
    out[blockIdx.y] = 0.5 * (s + (double)n * log(2. * M_PI));
  }
}

// G (n x n, ldg) = diag(sqrt_b) sym(C), C given by its lower triangle (ldc): G(k, i) = sqrt_b[k] C(max(k, i), min(k, i)).
// One 32 x 32 tile of G per workgroup, staged through LDS from the lower tile of C it mirrors, so both the reads and the
// writes are coalesced.  Only C's lower triangle is read, the diagonal tile's included.  blockIdx.z = problem: C and G
// at b * batch_M, sqrt_b at b * batch_v.
constexpr int GF_T = 32;
__global__ __launch_bounds__(256) void loo_form_g_kernel(const double *__restrict__ C, long long ldc,
                                                         const double *__restrict__ sqrt_b, long long n,
                                                         double *__restrict__ G, long long ldg, long long batch_M,
                                                         long long batch_v) {
  __shared__ double tile[GF_T][GF_T + 1];
  C += (long long)blockIdx.z * batch_M;
  G += (long long)blockIdx.z * batch_M;
  sqrt_b += (long long)blockIdx.z * batch_v;
  const long long bi = blockIdx.x, bj = blockIdx.y;  // rows k of tile bi, columns i of tile bj
  const long long rb = bi > bj ? bi : bj, cb = bi > bj ? bj : bi;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < GF_T; r += 8) {  // tile[r][tx] = C(rb * 32 + r, cb * 32 + tx), lower part only
    const long long row = rb * GF_T + r, col = cb * GF_T + tx;
    tile[r][tx] = (row < n && col < n && row >= col) ? C[row + col * ldc] : 0.;
  }
  __syncthreads();
  for (int c = ty; c < GF_T; c += 8) {  // G(k, i), k = bi * 32 + tx (coalesced), i = bj * 32 + c
    const long long k = bi * GF_T + tx, i = bj * GF_T + c;
    if (k >= n || i >= n) continue;
    double v;
    if (bi > bj) v = tile[tx][c];
    else if (bi < bj) v = tile[c][tx];
    else v = tx >= c ? tile[tx][c] : tile[c][tx];
    G[k + i * ldg] = sqrt_b[k] * v;
  }
}

// ---- S = G^T G, lower tiles, G full ------------------------------------------------------------------------------
// rtr_lower_kernel's product without its k >= i0 restriction: tile (bi, bj), bi >= bj, sums G(k, i) G(k, j) over all
// k < K through the same gemm_nt_sub_tile body, both operands k-major.  Every tile is K deep, so the launch order does
// not matter.  Flop: N^3.  The whole diagonal tile is written.
__global__ __launch_bounds__(GEMM_THREADS, 2) void gtg_lower_kernel(GemmArgs g) {
  __shared__ double lds[2 * 2 * GK * GLD];
  int bi, bj;
  lower_tile(blockIdx.x, bi, bj);
  const long long b = blockIdx.y;  // problem of a batched launch (batch_* = 0: one problem)
  GemmArgs t = g;
  t.C = g.C + b * g.batch_C;
  t.A = g.A + b * g.batch_A;
  t.B = g.B + b * g.batch_B;
  gemm_nt_sub_tile<true, true, true>(t, bi, bj, lds);
}

// S_b = G_b^T G_b for `count` problems (blockIdx.y = problem): G_b = G + b * stride_G, S_b = S + b * stride_S; count = 1 is
// launch_gtg_lower.
void launch_gtg_lower_batched(hipStream_t s, const double *G, long long ldg, long long stride_G, long long n, double *S,
                              long long lds_, long long stride_S, long long count) {
  if (n <= 0 || count <= 0) return;
  GemmArgs g;
  g.C = S; g.ldc = lds_; g.A = G; g.lda = ldg; g.B = G; g.ldb = ldg;
  g.M = n; g.N = n; g.K = n; g.tri = 1;
  g.ntr = g.ntc = (int)((n + GT - 1) / GT);
  g.assign = 1;  // S = + G^T G, S not read
  g.batch_C = stride_S; g.batch_A = g.batch_B = stride_G;
  const long long tiles = (long long)g.ntr * (g.ntr + 1) / 2;
  hipLaunchKernelGGL(gtg_lower_kernel, dim3((unsigned)tiles, (unsigned)count), dim3(GEMM_THREADS), 0, s, g);
}

void launch_gtg_lower(hipStream_t s, const double *G, long long ldg, long long n, double *S, long long lds_) {
  launch_gtg_lower_batched(s, G, ldg, 0, n, S, lds_, 0, 1);
}

// ---- leave-one-group-out: the kernels around the batched factor / solve / product chain ---------------------------
// A chunk of `count` groups padded to one size m: group g of the chunk owns idx[g * m .. (g + 1) * m) (point indices,
// -1 = padding) and an m x m slab (ld ldb, stride) of each of X0 / X1 / X2; sizes[g] is its real size.  Padded rows and
// columns of every slab are those of [X 0; 0 I], so they pass through the factorisations, inverses and products as
// identity blocks: log 1 = 0 in the log sums, zeros in d, z and a.  blockIdx.y (z where y is a tile index) = group;
// blockIdx.z of mirror_lower_kernel = problem.

// C(j, i) = C(i, j) for i > j, in place: rtr_lower_kernel writes the lower tiles only, the group blocks and the
// product sym(C) B sym(C) read both.  One 32 x 32 lower tile per workgroup through LDS, reads and writes coalesced.
__global__ __launch_bounds__(256) void mirror_lower_kernel(double *__restrict__ C, long long ldc, long long n, long long batch_C) {
  __shared__ double tile[GF_T][GF_T + 1];
  const long long bi = blockIdx.x, bj = blockIdx.y;
  if (bi < bj) return;  // (the whole workgroup)
  C += (long long)blockIdx.z * batch_C;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int c = ty; c < GF_T; c += 8) {  // tile[c][tx] = C(bi * 32 + tx, bj * 32 + c)
    const long long row = bi * GF_T + tx, col = bj * GF_T + c;
    tile[c][tx] = (row < n && col < n && row >= col) ? C[row + col * ldc] : 0.;
  }
  __syncthreads();
  for (int c = ty; c < GF_T; c += 8) {  // C(bj * 32 + tx, bi * 32 + c) = C(bi * 32 + c, bj * 32 + tx)
    const long long row = bj * GF_T + tx, col = bi * GF_T + c;
    if (row < n && col < n && row < col) C[row + col * ldc] = tile[tx][c];
  }
}

// The problems of a POOLED chunk (agp_logo_nll_gradient_batch: the groups of all problems of a batch in one chain).  Group g
// of the chunk belongs to problem prob[g]: its indices are row numbers of that problem, whose slabs (C, H) start stride_M
// and whose vectors (alpha, y_var, a) stride_v doubles behind those of problem 0.  flags: the problems' status words (4
// each: NaN input, failed pivot, ...) as the front end left them.  The plan is built before any status is known, so the
// groups of a FAILED problem run with the rest: the gather hands the chain an identity block in place of whatever the
// failed factor left in C_b and the sigma kernels take zeros for its alpha and variances, so nothing NaN enters the block
// chain and every launch keeps its trip counts; the problem's results are discarded at the end.
// prob == nullptr: one problem (the single-problem entries), nothing is offset and no status is read.
struct LogoProblems {
  const long long *prob = nullptr;
  long long stride_M = 0, stride_v = 0;
  const int *flags = nullptr;
};
__device__ __forceinline__ long long logo_problem(const LogoProblems &P, long long g) { return P.prob ? P.prob[g] : 0; }
__device__ __forceinline__ bool logo_problem_failed(const LogoProblems &P, long long b) {
  return P.prob && P.flags && (P.flags[4 * b] != 0 || P.flags[4 * b + 1] != 0);
}

// X0_g = [C[I_g, I_g] 0; 0 I] from the full symmetric C: column blockIdx.x of group blockIdx.y
__global__ __launch_bounds__(256) void logo_gather_blocks_kernel(const double *__restrict__ C, long long ldc,
                                                                 const long long *__restrict__ idx, long long m,
                                                                 double *__restrict__ X0, long long ldb, long long stride,
                                                                 LogoProblems P) {
  const long long c = blockIdx.x, g = blockIdx.y;
  const long long b = logo_problem(P, g);
  C += b * P.stride_M;
  const long long *ig = idx + g * m;
  const long long ic = logo_problem_failed(P, b) ? -1 : ig[c];
  double *out = X0 + g * stride + c * ldb;
  for (long long r = threadIdx.x; r < m; r += 256) {
    const long long ir = ig[r];
    out[r] = (ic >= 0 && ir >= 0) ? C[ir + ic * ldc] : (r == c ? 1. : 0.);
  }
}

// value only: X0_g holds -G_g^T G_g of the gathered columns of R (padding columns of G are zero): negate it and put
// the identity into the padding
__global__ __launch_bounds__(256) void logo_fix_blocks_kernel(const long long *__restrict__ idx, long long m,
                                                              double *__restrict__ X0, long long ldb, long long stride) {
  const long long c = blockIdx.x, g = blockIdx.y;
  const long long *ig = idx + g * m;
  const bool cv = ig[c] >= 0;
  double *x = X0 + g * stride + c * ldb;
  for (long long r = threadIdx.x; r < m; r += 256) x[r] = (cv && ig[r] >= 0) ? -x[r] : (r == c ? 1. : 0.);
}

// fixed-order sum of one value per thread over a workgroup of 256 (every thread receives it)
__device__ __forceinline__ double logo_block_sum(double acc, double *red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// X2_g holds -Sigma_g (Sigma_g = A_g^-1 = Q^T Q, Q = L_A^-1).  Column c of group g: V_g = Sigma_g + diag(s_I) into X0,
// T_g = Sigma_g into X1 (nullptr: value only), d_c = (Sigma_g alpha_I)_c into d and z.
__global__ __launch_bounds__(256) void logo_sigma_kernel(const double *__restrict__ X2, const long long *__restrict__ idx,
                                                         long long m, long long ldb, long long stride,
                                                         const double *__restrict__ alpha, const double *__restrict__ yvar,
                                                         double *__restrict__ X0, double *__restrict__ X1,
                                                         double *__restrict__ d, double *__restrict__ z, LogoProblems P) {
  __shared__ double red[4];
  const long long c = blockIdx.x, g = blockIdx.y;
  const long long b = logo_problem(P, g);
  if (logo_problem_failed(P, b)) { alpha = nullptr; yvar = nullptr; }
  else { alpha += b * P.stride_v; if (yvar) yvar += b * P.stride_v; }
  const long long *ig = idx + g * m;
  const long long off = g * stride + c * ldb, ic = ig[c];
  const double sc = (yvar && ic >= 0) ? yvar[ic] : 0.;
  double acc = 0.;
  for (long long r = threadIdx.x; r < m; r += 256) {
    const double sg = -X2[off + r];
    const long long ir = ig[r];
    acc += sg * ((ir >= 0 && alpha) ? alpha[ir] : 0.);
    X0[off + r] = r == c ? sg + sc : sg;
    if (X1) X1[off + r] = sg;
  }
  const double dc = logo_block_sum(acc, red);
  if (threadIdx.x == 0) d[g * m + c] = z[g * m + c] = dc;
}

// term[g] = log |V_g| + d_g^T V_g^-1 d_g + |I_g| log 2 pi = 2 logs_V[g] + z_g^T z_g + ..., z_g = L_V^-1 d_g
__global__ __launch_bounds__(256) void logo_term_kernel(const double *__restrict__ z, long long m,
                                                        const double *__restrict__ logs_V, const long long *__restrict__ sizes,
                                                        double *__restrict__ term) {
  __shared__ double red[4];
  const long long g = blockIdx.x;
  double acc = 0.;
  for (long long r = threadIdx.x; r < m; r += 256) acc += z[g * m + r] * z[g * m + r];
  const double zz = logo_block_sum(acc, red);
  if (threadIdx.x == 0) term[g] = 2. * logs_V[g] + zz + (double)sizes[g] * log(2. * M_PI);
}

// X2_g holds -T_g^T T_g = -Sigma_g V_g^-1 Sigma_g.  Column c of group g:
//   B_g = 1/2 Sigma V^-1 Sigma - 1/2 a a^T + 1/2 (a d^T + d a^T)   (symmetric, in general INDEFINITE: nothing may take its root)
// with zero rows and columns in the padding, and a[I_g[c]] = a_pad[c] (no scatter from the padding).
__global__ __launch_bounds__(256) void logo_assemble_kernel(const long long *__restrict__ idx, long long m, long long ldb,
                                                            long long stride, const double *__restrict__ a_pad,
                                                            const double *__restrict__ d, double *__restrict__ X2,
                                                            double *__restrict__ a, LogoProblems P) {
  const long long c = blockIdx.x, g = blockIdx.y;
  a += logo_problem(P, g) * P.stride_v;
  const long long *ig = idx + g * m;
  const long long ic = ig[c];
  const double ac = a_pad[g * m + c], dc = d[g * m + c];
  double *x = X2 + g * stride + c * ldb;
  for (long long r = threadIdx.x; r < m; r += 256) {
    const double ar = a_pad[g * m + r], dr = d[g * m + r];
    x[r] = (ic >= 0 && ig[r] >= 0) ? -0.5 * x[r] - 0.5 * ar * ac + 0.5 * (ar * dc + dr * ac) : 0.;
  }
  if (threadIdx.x == 0 && ic >= 0) a[ic] = ac;
}

// Marginal predict type.  X2_g holds -Sigma_g.  Column c of group g: d_c = (Sigma_g alpha_I)_c, v_c = Sigma_cc + s_c,
// q_c = d_c / v_c, and the column's share log v_c + d_c q_c of 2 NLL_g into t.  Gradient calls (X0 != nullptr): Sigma_g into
// X0 and Sigma_g diag(w) into X1 (this column scaled by w_c = 1/2 (1 / v_c - q_c^2), which is NEGATIVE whenever
// d_c^2 > v_c).  A padding column is e_c: d_c = q_c = 0, log v_c = log 1 = 0, and w_c is set to 0.
__global__ __launch_bounds__(256) void logo_marginal_sigma_kernel(const double *__restrict__ X2, const long long *__restrict__ idx,
                                                                  long long m, long long ldb, long long stride,
                                                                  const double *__restrict__ alpha, const double *__restrict__ yvar,
                                                                  double *__restrict__ X0, double *__restrict__ X1,
                                                                  double *__restrict__ d, double *__restrict__ q,
                                                                  double *__restrict__ t, LogoProblems P) {
  __shared__ double red[4];
  const long long c = blockIdx.x, g = blockIdx.y;
  const long long b = logo_problem(P, g);
  if (logo_problem_failed(P, b)) { alpha = nullptr; yvar = nullptr; }
  else { alpha += b * P.stride_v; if (yvar) yvar += b * P.stride_v; }
  const long long *ig = idx + g * m;
  const long long off = g * stride + c * ldb, ic = ig[c];
  double acc = 0.;
  for (long long r = threadIdx.x; r < m; r += 256) {
    const long long ir = ig[r];
    acc += -X2[off + r] * ((ir >= 0 && alpha) ? alpha[ir] : 0.);
  }
  const double dc = logo_block_sum(acc, red);
  const double vc = -X2[off + c] + ((yvar && ic >= 0) ? yvar[ic] : 0.);
  const double qc = dc / vc;
  if (threadIdx.x == 0) {
    d[g * m + c] = dc;
    q[g * m + c] = qc;
    t[g * m + c] = log(vc) + dc * qc;
  }
  if (!X0) return;
  const double wc = ic >= 0 ? 0.5 * (1. / vc - qc * qc) : 0.;
  for (long long r = threadIdx.x; r < m; r += 256) {
    const double sg = -X2[off + r];
    X0[off + r] = sg;
    X1[off + r] = sg * wc;
  }
}

// Marginal predict type: term[g] = sum_c (log v_c + d_c q_c) + |I_g| log 2 pi = 2 NLL_g, the scale of logo_term_kernel
__global__ __launch_bounds__(256) void logo_marginal_term_kernel(const double *__restrict__ t, long long m,
                                                                 const long long *__restrict__ sizes, double *__restrict__ term) {
  __shared__ double red[4];
  const long long g = blockIdx.x;
  double acc = 0.;
  for (long long r = threadIdx.x; r < m; r += 256) acc += t[g * m + r];
  const double sum = logo_block_sum(acc, red);
  if (threadIdx.x == 0) term[g] = sum + (double)sizes[g] * log(2. * M_PI);
}

// Marginal predict type.  X2_g holds -(Sigma_g diag(w)) Sigma_g^T.  Column c of group g:
//   B_g = Sigma diag(w) Sigma + 1/2 (a d^T + d a^T)   (symmetric, INDEFINITE wherever some w_c < 0)
// with zero rows and columns in the padding, and a[I_g[c]] = a_pad[c] (no scatter from the padding).
__global__ __launch_bounds__(256) void logo_marginal_assemble_kernel(const long long *__restrict__ idx, long long m, long long ldb,
                                                                     long long stride, const double *__restrict__ a_pad,
                                                                     const double *__restrict__ d, double *__restrict__ X2,
                                                                     double *__restrict__ a, LogoProblems P) {
  const long long c = blockIdx.x, g = blockIdx.y;
  a += logo_problem(P, g) * P.stride_v;
  const long long *ig = idx + g * m;
  const long long ic = ig[c];
  const double ac = a_pad[g * m + c], dc = d[g * m + c];
  double *x = X2 + g * stride + c * ldb;
  for (long long r = threadIdx.x; r < m; r += 256) {
    const double ar = a_pad[g * m + r], dr = d[g * m + r];
    x[r] = (ic >= 0 && ig[r] >= 0) ? -x[r] + 0.5 * (ar * dc + dr * ac) : 0.;
  }
  if (threadIdx.x == 0 && ic >= 0) a[ic] = ac;
}

// H = sym(C) B (n x n, ldh): column I_g[r] of H is sum_c B_g(c, r) C[:, I_g[c]]; the columns of points in no group
// stay zero (the caller zero-fills H).  One workgroup: 256 rows j, LOGO_HR columns r of group blockIdx.z; every C(j, I_c)
// is loaded once for the LOGO_HR columns.  Flop: 2 n sum_g |I_g|^2.
constexpr int LOGO_HR = 8;
__global__ __launch_bounds__(256) void logo_h_kernel(const double *__restrict__ C, long long ldc, long long n,
                                                     const long long *__restrict__ idx, const long long *__restrict__ sizes,
                                                     long long m, const double *__restrict__ X2, long long ldb, long long stride,
                                                     double *__restrict__ H, long long ldh, LogoProblems P) {
  const long long g = blockIdx.z, r0 = (long long)blockIdx.y * LOGO_HR, sz = sizes[g];
  if (r0 >= sz) return;  // (the whole workgroup)
  const long long pb = logo_problem(P, g);
  C += pb * P.stride_M;
  H += pb * P.stride_M;
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long *ig = idx + g * m;
  const double *B = X2 + g * stride;
  double acc[LOGO_HR];
#pragma unroll
  for (int t = 0; t < LOGO_HR; ++t) acc[t] = 0.;
  for (long long c = 0; c < sz; ++c) {
    const double x = j < n ? C[j + ig[c] * ldc] : 0.;
#pragma unroll
    for (int t = 0; t < LOGO_HR; ++t) acc[t] += (r0 + t < sz ? B[c + (r0 + t) * ldb] : 0.) * x;
  }
  if (j >= n) return;
#pragma unroll
  for (int t = 0; t < LOGO_HR; ++t)
    if (r0 + t < sz) H[j + ig[r0 + t] * ldh] = acc[t];
}

// out = 1/2 sum_g term[g]   (one workgroup, fixed order)
__global__ __launch_bounds__(1024) void logo_sum_kernel(const double *__restrict__ term, long long count, double *__restrict__ out) {
  __shared__ double red[16];
  double acc = 0.;
  for (long long i = threadIdx.x; i < count; i += 1024) acc += term[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.;
    for (int w = 0; w < 16; ++w) s += red[w];
    *out = 0.5 * s;
  }
}

// agp_logo_nll_gradient_batch: the terms lie in the pooled order of the plan (by size, across problems).  Workgroup b walks
// problem b's own terms - list[off[b] .. off[b + 1]), ascending term indices, built on the host - in a fixed order:
// out[b] = 1/2 sum of them (0 for a problem without a non-empty group), and a group block that did not factor
// (gflags[4 q + 1], written by the block factorisations) becomes the problem's failed pivot in flags[4 b + 1].
// The front end reports NaN in the features and variances only (the Gram sees them); a NaN TARGET reaches alpha_b and from
// there this problem's own terms and columns, nobody else's: the n_b real values of alpha_b (D[b].X.n of them, at
// alpha + b * stride_v) are looked through here, and a NaN among them of a problem that did factor becomes flags[4 b].
__global__ __launch_bounds__(256) void logo_problem_sum_kernel(const double *__restrict__ term, const int *__restrict__ gflags,
                                                               const long long *__restrict__ off, const long long *__restrict__ list,
                                                               const double *__restrict__ alpha, long long stride_v,
                                                               const ContractDesc *__restrict__ D, double *__restrict__ out,
                                                               int *__restrict__ flags) {
  __shared__ double red[4];
  const long long b = blockIdx.x;
  int nan_alpha = 0;
  for (long long i = threadIdx.x; i < D[b].X.n; i += 256) nan_alpha |= isnan(alpha[b * stride_v + i]);
  nan_alpha = __syncthreads_or(nan_alpha);
  double acc = 0.;
  int bad = 0;
  for (long long i = off[b] + threadIdx.x; i < off[b + 1]; i += 256) {
    const long long q = list[i];
    acc += term[q];
    bad |= gflags[4 * q + 1] != 0 || gflags[4 * q] != 0;
  }
  const double sum = logo_block_sum(acc, red);
  const int any_bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    out[b] = 0.5 * sum;
    if (nan_alpha && flags[4 * b] == 0 && flags[4 * b + 1] == 0) flags[4 * b] = 1;
    if (any_bad && flags[4 * b + 1] == 0) flags[4 * b + 1] = 1;
  }
}

// ---- S = H C^T = sym(C) B sym(C), lower tiles, H and C full -----------------------------------------------------------
// gtg_lower_kernel's product with two different operands, both stored like the matrix (C is symmetric): tile (bi, bj),
// bi >= bj, sums H(i, k) C(j, k) over all k through the same gemm_nt_sub_tile body.  Flop: N^3.  S is neither operand.
__global__ __launch_bounds__(GEMM_THREADS, 2) void hct_lower_kernel(GemmArgs g) {
  __shared__ double lds[2 * 2 * GK * GLD];
  int bi, bj;
  lower_tile(blockIdx.x, bi, bj);
  const long long b = blockIdx.y;  // problem of a batched launch (batch_* = 0: one problem)
  GemmArgs t = g;
  t.C = g.C + b * g.batch_C;
  t.A = g.A + b * g.batch_A;
  t.B = g.B + b * g.batch_B;
  gemm_nt_sub_tile<false, false, true>(t, bi, bj, lds);
}

void launch_hct_lower_batched(hipStream_t s, const double *H, long long ldh, long long stride_H, const double *C, long long ldc,
                              long long stride_C, long long n, double *S, long long lds_, long long stride_S, long long count) {
  if (n <= 0 || count <= 0) return;
  GemmArgs g;
  g.C = S; g.ldc = lds_; g.A = H; g.lda = ldh; g.B = C; g.ldb = ldc;
  g.M = n; g.N = n; g.K = n; g.tri = 1;
  g.ntr = g.ntc = (int)((n + GT - 1) / GT);
  g.assign = 1;  // S = + H C^T, S not read
  g.batch_C = stride_S; g.batch_A = stride_H; g.batch_B = stride_C;
  const long long tiles = (long long)g.ntr * (g.ntr + 1) / 2;
  hipLaunchKernelGGL(hct_lower_kernel, dim3((unsigned)tiles, (unsigned)count), dim3(GEMM_THREADS), 0, s, g);
}

}  // namespace agp

using namespace agp;

// ---- slot validation: a leaf node and a parameter index the leaf has ----------------------------------------------
int check_slots(const agp_kernel *k, int n_slots, const agp_gradient_slot *slots, int *n_tangent_columns) {
  int ntc = 0;
  for (int s = 0; s < n_slots; ++s) {
    const int node = slots[s].node, param = slots[s].param;
    if (node < 0 || node >= k->prog.n_nodes || param < 0) return AGP_ERR_INVALID_ARGUMENT;
    const agp_kernel_node &nd = k->prog.nodes[node];
    int n_params;
    if (nd.op >= AGP_OP_SQUARED_EXPONENTIAL && nd.op <= AGP_OP_MATERN52) n_params = 2;
    else if (nd.op == AGP_OP_CONSTANT || nd.op == AGP_OP_INDEPENDENT_NOISE || nd.op == AGP_OP_NUGGET) n_params = 1;
    else if (nd.op == AGP_OP_POLYNOMIAL) n_params = nd.order + 1;
    else if (nd.op == AGP_OP_SCALING) n_params = -1;  // any tangent column
    else return AGP_ERR_INVALID_ARGUMENT;             // not a leaf
    if (n_params >= 0 && param >= n_params) return AGP_ERR_INVALID_ARGUMENT;
    if (n_params < 0 && param + 1 > ntc) ntc = param + 1;
  }
  *n_tangent_columns = ntc;
  return AGP_OK;
}

int fill_slot_group(const agp_kernel *k, int n_slots, const agp_gradient_slot *slots, int g0, TangentSlots<GRAD_GROUP> &group,
                    bool (&scaling)[GRAD_GROUP]) {
  const int cnt = n_slots - g0 < GRAD_GROUP ? n_slots - g0 : GRAD_GROUP;
  for (int j = 0; j < GRAD_GROUP; ++j) {
    const bool used = j < cnt;
    group.node[j] = used ? slots[g0 + j].node : -1;
    group.param[j] = used ? slots[g0 + j].param : 0;
    scaling[j] = used && k->prog.nodes[group.node[j]].op == AGP_OP_SCALING;
  }
  return cnt > 0 ? cnt : 0;
}

void fill_contract_desc(ContractDesc &d, const agp_kernel *k, const FeatView &X, const double *C, long long ldc, const double *alpha,
                        const double *u, double *partial, int n_slots, const agp_gradient_slot *slots, const double *tcol, long long tld) {
  std::memset(static_cast<void *>(&d), 0, sizeof(ContractDesc));
  d.prog = k->prog;
  d.X = X;
  d.C = C;
  d.ldc = ldc;
  d.alpha = alpha;
  d.u = u;
  d.partial = partial;
  d.n_slots = n_slots;
  for (int grp = 0; grp < GRAD_GROUPS_MAX; ++grp) {
    bool scaling[GRAD_GROUP];
    fill_slot_group(k, n_slots, slots, grp * GRAD_GROUP, d.slots[grp], scaling);
    for (int j = 0; j < GRAD_GROUP; ++j)
      d.tang[grp * GRAD_GROUP + j] = scaling[j] ? tcol + (size_t)d.slots[grp].param[j] * (size_t)tld : nullptr;
  }
}

int stage_tangents(agp_context *ctx, hipStream_t s, const double *tangents, long long ld, int location, long long n, int ntc,
                   double **cursor, const double **dev, long long *ld_dev) {
  *dev = tangents;
  *ld_dev = ld;
  if (ntc <= 0 || location != AGP_HOST) return AGP_OK;
  const long long np2 = round_up(n, 2);
  AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(*cursor, sizeof(double) * (size_t)np2, tangents, sizeof(double) * (size_t)ld,
                                      sizeof(double) * (size_t)n, (size_t)ntc, hipMemcpyHostToDevice, s));
  *dev = *cursor;
  *ld_dev = np2;
  *cursor += (size_t)np2 * (size_t)ntc;
  return AGP_OK;
}

// ---- the steps both gradients share ------------------------------------------------------------------------------
// Everything agp_nll_gradient and agp_loo_nll_gradient do up to and including the fit.  Workspaces (batch_layout.h):
// ws_A as agp_nll (carve_fit), ws_aux by carve_gradient_aux with extra_elems doubles of the entry's own at its end.
struct GradientCall {
  long long n = 0, lda = 0, tiles = 0, ldt_d = 0;
  double *A = nullptr, *invd = nullptr, *z = nullptr, *yvar_d = nullptr;
  double *R = nullptr, *bs_ws = nullptr, *partial = nullptr, *grad_d = nullptr, *extra = nullptr;
  const double *tang_d = nullptr;
  const DevProgram *dprog = nullptr;
  DeviceFeatures dx;
  FeatView xm{};
};

static int gradient_setup(agp_context_impl *ctx, const agp_kernel *k, const agp_features *x, const double *y,
                          const double *y_var, int n_slots, const agp_gradient_slot *slots, const double *tangents,
                          int64_t ldt, size_t extra_elems, GradientCall &g) {
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  int ntc = 0;
  if ((st = check_slots(k, n_slots, slots, &ntc)) != AGP_OK) return st;
  if (ntc > 0 && (!tangents || ldt < n)) return AGP_ERR_INVALID_ARGUMENT;
  if ((st = device_program(ctx, k, &g.dprog)) != AGP_OK) return st;
  hipStream_t s = ctx->stream;

  g.n = n;
  const BatchGeometry geo = batch_geometry(n, 1);
  const long long lda = g.lda = geo.lda;
  g.tiles = lower_tiles(n);
  const size_t tang_elems = ntc > 0 && x->location == AGP_HOST ? (size_t)geo.np2 * (size_t)ntc : 0;
  auto carve_aux = [&](WsLayout &w) {
    return carve_gradient_aux(w, geo, backsolve_ws_elems(n), (size_t)g.tiles * GRAD_GROUP, (size_t)round_up(AGP_MAX_GRADIENT_SLOTS, 2),
                              tang_elems, extra_elems);
  };
  WsLayout size_A, size_aux;
  carve_fit(size_A, geo);
  carve_aux(size_aux);
  if ((st = reserve_ws(ctx, ctx->ws_A, size_A.bytes())) != AGP_OK) return st;
  if ((st = reserve_ws(ctx, ctx->ws_aux, size_aux.bytes())) != AGP_OK) return st;
  WsLayout ws_A(ctx->ws_A), ws_aux(ctx->ws_aux);
  const FitRegions r = carve_fit(ws_A, geo);
  const GradientAuxRegions a = carve_aux(ws_aux);
  g.A = r.A; g.invd = r.invd; g.z = r.z; g.yvar_d = y_var ? r.yvar : nullptr;
  g.R = a.R; g.bs_ws = a.bs_ws; g.partial = a.partial; g.grad_d = a.grad; g.extra = a.extra;
  double *tcur = a.tang;
  if ((st = stage_tangents(ctx, s, tangents, ldt, x->location, n, ntc, &tcur, &g.tang_d, &g.ldt_d)) != AGP_OK) return st;

  if ((st = to_device(ctx, x, false, &g.dx)) != AGP_OK) return st;
  if ((st = vector_to_device(ctx, y, n, x->location, g.z)) != AGP_OK) return st;
  if (y_var && (st = vector_to_device(ctx, y_var, n, x->location, g.yvar_d)) != AGP_OK) return st;
  g.xm = g.dx.v;
  g.xm.meas = 1;
  // the fit: A = L, z = L^-1 y, flags and log det (api.hip: build_and_factor via agp_nll's path)
  st = build_and_factor_nll(ctx, g.dprog, &k->prog, g.xm, g.A, lda, g.invd, g.z, g.yvar_d);
  if (st == AGP_OK) st = status_from_flags(ctx);
  return st;
}

// alpha = L^-T z in place, then R = L^-1 (triangular right-hand side); stage event 3 at the end
static int alpha_and_inverse_factor(agp_context_impl *ctx, GradientCall &g) {
  hipStream_t s = ctx->stream;
  backward_solve_vec_any(s, g.A, g.n, g.lda, g.invd, g.z, g.bs_ws);
  launch_set_identity(s, g.R, g.lda, g.n);
  forward_solve_mat_lookahead(ctx, g.A, g.n, g.lda, g.invd, g.R, g.n, g.lda, /*rhs_lower=*/true);
  if (ctx->profiling) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[3], s));
  return AGP_OK;
}

// the contraction of W's lower triangle (g.A, or the slab `weight` with the same leading dimension) against dK / dslot,
// GRAD_GROUP slots per pass, into g.grad_d
template <bool LOO>
static void contract_slots(hipStream_t s, const agp_kernel *k, int n_slots, const agp_gradient_slot *slots,
                           const GradientCall &g, const double *u, double scale, const double *weight = nullptr) {
  for (int g0 = 0; g0 < n_slots; g0 += GRAD_GROUP) {
    ContractArgs ca;
    ca.C = weight ? weight : g.A; ca.ldc = g.lda; ca.alpha = g.z; ca.u = u; ca.partial = g.partial;
    bool scaling[GRAD_GROUP];
    const int cnt = fill_slot_group(k, n_slots, slots, g0, ca.slots, scaling);
    for (int j = 0; j < GRAD_GROUP; ++j) ca.tang[j] = scaling[j] ? g.tang_d + (size_t)ca.slots.param[j] * (size_t)g.ldt_d : nullptr;
    launch_contract<LOO>(s, g.dprog, g.xm, ca, g.tiles);
    launch_grad_reduce(s, g.partial, g.tiles, cnt, scale, g.grad_d + g0);
  }
}

// ---- leave-one-group-out: the chunks of groups that advance in lock step (LogoChunk, LogoPlan: api_internal.h) --------
constexpr long long LOGO_CHUNK_GROUPS_MAX = 16384;
constexpr long long LOGO_CHUNK_IMG_ELEMS_MAX = 32ll << 20;  // 256 MiB of tile images per chunk
long long logo_img_stride(long long m) { return (m + NB - 1) / NB * (36ll * MB * MB); }
long long logo_chunk_groups_max() { return LOGO_CHUNK_GROUPS_MAX; }
long long logo_chunk_img_elems_max() { return LOGO_CHUNK_IMG_ELEMS_MAX; }

int logo_plan(long long n, int64_t n_groups, const int64_t *offsets, const int64_t *indices, LogoPlan &p) {
  if (n_groups < 0 || (n_groups > 0 && (!offsets || offsets[0] != 0))) return AGP_ERR_INVALID_ARGUMENT;
  std::vector<std::pair<long long, long long>> order;  // (size, group), non-empty groups
  for (int64_t g = 0; g < n_groups; ++g) {
    const long long m = offsets[g + 1] - offsets[g];
    if (m < 0) return AGP_ERR_INVALID_ARGUMENT;
    if (m > 0) order.emplace_back(m, (long long)g);
  }
  const long long total = n_groups > 0 ? offsets[n_groups] : 0;
  if (total > n || (total > 0 && !indices)) return AGP_ERR_INVALID_ARGUMENT;  // (more than n indices: one occurs twice)
  std::vector<char> seen((size_t)n, 0);
  for (long long i = 0; i < total; ++i) {
    const long long j = indices[i];
    if (j < 0 || j >= n || seen[(size_t)j]) return AGP_ERR_INVALID_ARGUMENT;
    seen[(size_t)j] = 1;
  }
  std::sort(order.begin(), order.end());
  p.terms = (long long)order.size();
  for (const auto &o : order) p.group.push_back(o.second);
  size_t at = 0;
  while (at < order.size()) {
    const long long m0 = order[at].first;
    size_t end = at + 1;
    while (end < order.size()) {
      const long long m = order[end].first, cnt = (long long)(end - at) + 1;
      if (m > 2 * m0 || cnt > LOGO_CHUNK_GROUPS_MAX || cnt * m > n || cnt * logo_img_stride(m) > LOGO_CHUNK_IMG_ELEMS_MAX) break;
      ++end;
    }
    LogoChunk ch;
    ch.m = order[end - 1].first;
    ch.count = (long long)(end - at);
    ch.term_off = (long long)at;
    ch.idx_off = (long long)p.meta.size();
    p.meta.resize(p.meta.size() + (size_t)(ch.count * ch.m), -1);
    for (size_t q = at; q < end; ++q) {
      const long long g = order[q].second, sz = order[q].first;
      for (long long a = 0; a < sz; ++a) p.meta[(size_t)ch.idx_off + (size_t)((long long)(q - at) * ch.m + a)] = indices[offsets[g] + a];
    }
    ch.size_off = (long long)p.meta.size();
    for (size_t q = at; q < end; ++q) p.meta.push_back(order[q].first);
    p.chunks.push_back(ch);
    const size_t blocks = (size_t)ch.count * (size_t)(factor_ld(ch.m) * ch.m), imgs = (size_t)ch.count * (size_t)logo_img_stride(ch.m);
    const size_t vec = (size_t)round_up(ch.count * ch.m, 2), cnt2 = (size_t)round_up(ch.count, 2);
    if (blocks > p.block_elems) p.block_elems = blocks;
    if (imgs > p.img_elems) p.img_elems = imgs;
    if (vec > p.vec_elems) p.vec_elems = vec;
    if (cnt2 > p.count_elems) p.count_elems = cnt2;
    at = end;
  }
  return AGP_OK;
}

// The two halves of a chunk's value chain that do not depend on where the blocks come from (logo_chunk below; the sparse
// model's held-out groups, sparse_gradient.hip).  logo_chunk_sigma: X0 = [A_g 0; 0 I] -> L_A (logs_A), X1 = L_A^-1,
// X2 = -Sigma_g = -X1^T X1.  The caller's sigma kernel then puts V_g into X0 and d into d / z (Joint), or the columns'
// shares of 2 NLL_g into a_pad (Marginal).  logo_chunk_terms: Joint V_g = L_V L_V^T with z = L_V^-1 d riding along, then
// term[g] = 2 NLL_g; Marginal: the sum of the shares.
void logo_chunk_sigma(agp_context_impl *ctx, const LogoRegions &r, const LogoChunk &ch, int *group_flags) {
  hipStream_t s = ctx->stream;
  const long long m = ch.m, count = ch.count;
  const long long ldb = factor_ld(m), stride_B = ldb * m, stride_I = logo_img_stride(m);
  const size_t slab_bytes = sizeof(double) * (size_t)stride_B * (size_t)count;
  (void)hipMemsetAsync(r.logs_A, 0, sizeof(double) * (size_t)round_up(count, 2), s);
  (void)hipMemsetAsync(r.logs_V, 0, sizeof(double) * (size_t)round_up(count, 2), s);
  factor_lower_batched(s, r.X0, stride_B, m, ldb, r.img, stride_I, nullptr, 0, count, group_flags ? group_flags : ctx->d_flags, r.logs_A,
                       group_flags ? 4 : 0);
  launch_set_identity_batched(s, r.X1, ldb, stride_B, m, count);
  forward_solve_mat_batched(s, r.X0, stride_B, m, ldb, r.img, stride_I, r.X1, stride_B, m, ldb, /*rhs_lower=*/true, count);
  (void)hipMemsetAsync(r.X2, 0, slab_bytes, s);
  launch_gemm_nt_sub_batched(s, r.X2, ldb, stride_B, r.X1, ldb, true, stride_B, r.X1, ldb, true, stride_B, m, m, m, false, count);  // -Sigma
}

void logo_chunk_terms(agp_context_impl *ctx, const LogoRegions &r, const LogoChunk &ch, bool marginal, int *group_flags) {
  hipStream_t s = ctx->stream;
  const long long m = ch.m, count = ch.count;
  const long long ldb = factor_ld(m), stride_B = ldb * m, stride_I = logo_img_stride(m);
  const long long *sizes = r.meta + ch.size_off;
  if (marginal) {
    hipLaunchKernelGGL(logo_marginal_term_kernel, dim3((unsigned)count), dim3(256), 0, s, r.a_pad, m, sizes, r.term + ch.term_off);
  } else {
    factor_lower_batched(s, r.X0, stride_B, m, ldb, r.img, stride_I, r.z, m, count, group_flags ? group_flags : ctx->d_flags, r.logs_V,
                         group_flags ? 4 : 0);
    hipLaunchKernelGGL(logo_term_kernel, dim3((unsigned)count), dim3(256), 0, s, r.z, m, r.logs_V, sizes, r.term + ch.term_off);
  }
}

void launch_logo_sum(hipStream_t s, const double *term, long long count, double *out) {
  hipLaunchKernelGGL(logo_sum_kernel, dim3(1), dim3(1024), 0, s, term, count, out);
}

// One chunk through its chain.  X0 enters as [A_g 0; 0 I], A_g = C[I_g, I_g]: from the full C (gradient calls), or from
// the gathered columns of R, A_g = R[:, I_g]^T R[:, I_g] (value only; the columns go where L was).  Then, all groups at
// once: A_g = L_A L_A^T, Q = L_A^-1, Sigma_g = Q^T Q, d = Sigma alpha_I, V_g = Sigma_g + diag(s_I) = L_V L_V^T with
// z = L_V^-1 d riding along, the NLL term; and for the gradient T = L_V^-1 Sigma, a_I = T^T z = Sigma V^-1 d,
// T^T T = Sigma V^-1 Sigma, B_g and (with slots) the columns I_g of H = sym(C) B.
// marginal (AGP_PREDICT_MARGINAL): the same up to -Sigma_g in X2; then d, q = d / v and the terms per column (the shares of
// 2 NLL_g wait in a_pad until the term kernel has summed them), and for the gradient Sigma into X0, Sigma diag(w) into X1,
// a_I = Sigma q, -(Sigma diag(w)) Sigma^T as a product of two different operands, B_g, H.  No second LL^T, no T.
// The pooled chunks of agp_logo_nll_gradient_batch run the same chain through logo_chunk_run with P naming every group's
// problem: the blocks always come from C_b there (from_c), need_c means "the gradient's half of the chain", group_flags are
// its per-group status words.
struct LogoChainArgs {
  long long n, lda;
  double *C, *H, *a;
  const double *R, *alpha, *yvar;
};
static void logo_chunk_run(agp_context_impl *ctx, const LogoChainArgs &g, const LogoRegions &r, const LogoChunk &ch, bool from_c,
                           bool need_c, bool need_h, bool marginal, const LogoProblems &P, int *group_flags);

static void logo_chunk(agp_context_impl *ctx, const GradientCall &g, const LogoRegions &r, const LogoChunk &ch, bool need_c,
                       bool need_h, bool marginal) {
  const LogoChainArgs a{g.n, g.lda, g.A, g.R, r.a, g.R, g.z, g.yvar_d};
  logo_chunk_run(ctx, a, r, ch, need_c, need_c, need_h, marginal, LogoProblems{}, nullptr);
}

static void logo_chunk_run(agp_context_impl *ctx, const LogoChainArgs &g, const LogoRegions &r, const LogoChunk &ch, bool from_c,
                           bool need_c, bool need_h, bool marginal, const LogoProblems &P, int *group_flags) {
  hipStream_t s = ctx->stream;
  const long long m = ch.m, count = ch.count, n = g.n;
  const long long ldb = factor_ld(m), stride_B = ldb * m, stride_I = logo_img_stride(m);
  const long long *idx = r.meta + ch.idx_off, *sizes = r.meta + ch.size_off;
  const size_t slab_bytes = sizeof(double) * (size_t)stride_B * (size_t)count;
  const dim3 cols((unsigned)m, (unsigned)count);
  if (from_c) {
    hipLaunchKernelGGL(logo_gather_blocks_kernel, cols, dim3(256), 0, s, g.C, g.lda, idx, m, r.X0, ldb, stride_B, P);
  } else {
    for (long long c0 = 0; c0 < count * m; c0 += 32768)  // (grid limit of the gather: 65535 columns per launch)
      launch_gather_cols(s, g.R, g.lda, idx + c0, count * m - c0 < 32768 ? count * m - c0 : 32768, 0, n, g.C + c0 * g.lda, g.lda);
    (void)hipMemsetAsync(r.X0, 0, slab_bytes, s);
    launch_gemm_nt_sub_batched(s, r.X0, ldb, stride_B, g.C, g.lda, true, m * g.lda, g.C, g.lda, true, m * g.lda, m, m, n, false, count);
    hipLaunchKernelGGL(logo_fix_blocks_kernel, cols, dim3(256), 0, s, idx, m, r.X0, ldb, stride_B);
  }
  logo_chunk_sigma(ctx, r, ch, group_flags);
  if (marginal) {
    hipLaunchKernelGGL(logo_marginal_sigma_kernel, cols, dim3(256), 0, s, r.X2, idx, m, ldb, stride_B, g.alpha, g.yvar,
                       need_c ? r.X0 : nullptr, need_c ? r.X1 : nullptr, r.d, r.z, r.a_pad, P);
    logo_chunk_terms(ctx, r, ch, true, group_flags);
    if (!need_c) return;
    launch_colvec_dot_batched(s, r.X0, ldb, stride_B, m, r.z, m, count, r.a_pad);  // a_I = Sigma q (Sigma symmetric)
    (void)hipMemsetAsync(r.X2, 0, slab_bytes, s);
    launch_gemm_nt_sub_batched(s, r.X2, ldb, stride_B, r.X1, ldb, false, stride_B, r.X0, ldb, false, stride_B, m, m, m, false, count);
    hipLaunchKernelGGL(logo_marginal_assemble_kernel, cols, dim3(256), 0, s, idx, m, ldb, stride_B, r.a_pad, r.d, r.X2, g.a, P);
  } else {
    hipLaunchKernelGGL(logo_sigma_kernel, cols, dim3(256), 0, s, r.X2, idx, m, ldb, stride_B, g.alpha, g.yvar, r.X0, need_c ? r.X1 : nullptr,
                       r.d, r.z, P);
    logo_chunk_terms(ctx, r, ch, false, group_flags);
    if (!need_c) return;
    forward_solve_mat_batched(s, r.X0, stride_B, m, ldb, r.img, stride_I, r.X1, stride_B, m, ldb, /*rhs_lower=*/false, count);  // T
    launch_colvec_dot_batched(s, r.X1, ldb, stride_B, m, r.z, m, count, r.a_pad);
    (void)hipMemsetAsync(r.X2, 0, slab_bytes, s);
    launch_gemm_nt_sub_batched(s, r.X2, ldb, stride_B, r.X1, ldb, true, stride_B, r.X1, ldb, true, stride_B, m, m, m, false, count);  // -T^T T
    hipLaunchKernelGGL(logo_assemble_kernel, cols, dim3(256), 0, s, idx, m, ldb, stride_B, r.a_pad, r.d, r.X2, g.a, P);
  }
  if (need_h)
    hipLaunchKernelGGL(logo_h_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((m + LOGO_HR - 1) / LOGO_HR), (unsigned)count), dim3(256),
                       0, s, g.C, g.lda, n, idx, sizes, m, r.X2, ldb, stride_B, g.H, g.lda, P);
}

static float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  return ms;
}

extern "C" {

int agp_nll_gradient(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                     int n_slots, const agp_gradient_slot *slots, const double *tangents, int64_t ldt, double *nll,
                     double *grad_nll, double *information) {
  if (!c || !k || !x || !y || !nll) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && (!slots || !grad_nll))) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  GradientCall g;
  int st = gradient_setup(ctx, k, x, y, y_var, n_slots, slots, tangents, ldt, 0, g);
  if (st != AGP_OK) return st;
  hipStream_t s = ctx->stream;
  const long long n = g.n;
  const bool prof = ctx->profiling;
  // y^T K^-1 y = z^T z, then alpha = L^-T z in place; R = L^-1, K^-1 = R^T R over L
  launch_dot(s, g.z, g.z, n, ctx->d_scalars + 1);
  if ((st = alpha_and_inverse_factor(ctx, g)) != AGP_OK) return st;
  const double *alpha = g.z;
  launch_rtr_lower(s, g.R, g.lda, n, g.A, g.lda);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[4], s));
  contract_slots<false>(s, k, n_slots, slots, g, nullptr, 0.5);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_slots > 0) AGP_HIP_CHECK(ctx, hipMemcpyAsync(grad_nll, g.grad_d, sizeof(double) * (size_t)n_slots, hipMemcpyDeviceToHost, s));
  if (information) AGP_HIP_CHECK(ctx, hipMemcpyAsync(information, alpha, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  *nll = 0.5 * (2. * ctx->h_scalars[0] + ctx->h_scalars[1] + (double)n * std::log(2 * M_PI));  // likelihood.hpp:46
  if (prof) {
    // stage 2: alpha and R = L^-1 (from the end of the factorisation), 6: R^T R, 7: contraction
    ctx->stage_ms[2] = elapsed(ctx->stage_ev[2], ctx->stage_ev[3]);
    ctx->stage_ms[6] = elapsed(ctx->stage_ev[3], ctx->stage_ev[4]);
    ctx->stage_ms[7] = elapsed(ctx->stage_ev[4], ctx->stage_ev[5]);
  }
  return AGP_OK;
}

int agp_loo_nll_gradient(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                         int n_slots, const agp_gradient_slot *slots, const double *tangents, int64_t ldt, double *loo_nll,
                         double *grad_loo_nll, double *mean_weights) {
  if (!c || !k || !x || !y || !loo_nll) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && (!slots || !grad_loo_nll)))
    return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  // extra: [term | a | sqrt_b | u | c | symv scratch], n (rounded up) each but the scratch
  const long long n = x->n, n2 = round_up(n > 0 ? n : 1, 2);
  const size_t extra = 5 * (size_t)n2 + symv_ws_elems(n > 0 ? n : 1);
  GradientCall g;
  int st = gradient_setup(ctx, k, x, y, y_var, n_slots, slots, tangents, ldt, extra, g);
  if (st != AGP_OK) return st;
  hipStream_t s = ctx->stream;
  double *term = g.extra, *a = term + n2, *sqrt_b = a + n2, *u = sqrt_b + n2, *cdiag = u + n2, *symv_ws = cdiag + n2;
  const bool prof = ctx->profiling;
  const bool need_c = n_slots > 0 || mean_weights;  // u = C a needs C = R^T R; the value alone needs only diag(C)
  if ((st = alpha_and_inverse_factor(ctx, g)) != AGP_OK) return st;
  const double *alpha = g.z;
  const unsigned eblocks = (unsigned)((n + 255) / 256);
  if (!need_c) {
    // c_i = ||R[:, i]||^2, as agp_fit_inverse_diagonal
    launch_coldot(s, g.R, g.lda, g.R, g.lda, n, n, cdiag, -1.0, nullptr);
    hipLaunchKernelGGL(loo_terms_kernel, dim3(eblocks), dim3(256), 0, s, cdiag, 1LL, 0LL, alpha, g.yvar_d, n, 0LL, term, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(loo_sum_kernel, dim3(1), dim3(1024), 0, s, term, n, 0LL, ctx->d_scalars + 2, nullptr);
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
  } else {
    launch_rtr_lower(s, g.R, g.lda, n, g.A, g.lda);  // C = K^-1 over L
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[4], s));
    hipLaunchKernelGGL(loo_terms_kernel, dim3(eblocks), dim3(256), 0, s, g.A, g.lda + 1, 0LL, alpha, g.yvar_d, n, 0LL, term, a, sqrt_b, nullptr);
    hipLaunchKernelGGL(loo_sum_kernel, dim3(1), dim3(1024), 0, s, term, n, 0LL, ctx->d_scalars + 2, nullptr);
    launch_symv_lower(s, g.A, g.lda, n, a, 1., 0., nullptr, u, symv_ws);  // u = C a
    if (n_slots > 0) {
      const unsigned gt = (unsigned)((n + GF_T - 1) / GF_T);
      hipLaunchKernelGGL(loo_form_g_kernel, dim3(gt, gt), dim3(256), 0, s, g.A, g.lda, sqrt_b, n, g.R, g.lda, 0LL, 0LL);  // G over R
    }
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
    if (n_slots > 0) {
      launch_gtg_lower(s, g.R, g.lda, n, g.A, g.lda);  // S = C diag(b) C over C
      if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[6], s));
      contract_slots<true>(s, k, n_slots, slots, g, u, 1.0);
      if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[7], s));
    }
  }
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_slots > 0)
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(grad_loo_nll, g.grad_d, sizeof(double) * (size_t)n_slots, hipMemcpyDeviceToHost, s));
  if (mean_weights) AGP_HIP_CHECK(ctx, hipMemcpyAsync(mean_weights, u, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  *loo_nll = ctx->h_scalars[2];
  if (prof) {
    // 2: alpha and R = L^-1; value only: 8 the column norms and the LOO terms; otherwise 6 R^T R, 8 the LOO terms, u
    // and G, 9 G^T G, 7 the contraction
    ctx->stage_ms[6] = ctx->stage_ms[7] = ctx->stage_ms[8] = ctx->stage_ms[9] = 0.;
    ctx->stage_ms[2] = elapsed(ctx->stage_ev[2], ctx->stage_ev[3]);
    if (!need_c) {
      ctx->stage_ms[8] = elapsed(ctx->stage_ev[3], ctx->stage_ev[5]);
    } else {
      ctx->stage_ms[6] = elapsed(ctx->stage_ev[3], ctx->stage_ev[4]);
      ctx->stage_ms[8] = elapsed(ctx->stage_ev[4], ctx->stage_ev[5]);
      if (n_slots > 0) {
        ctx->stage_ms[9] = elapsed(ctx->stage_ev[5], ctx->stage_ev[6]);
        ctx->stage_ms[7] = elapsed(ctx->stage_ev[6], ctx->stage_ev[7]);
      }
    }
  }
  return AGP_OK;
}

int agp_logo_nll_gradient(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                          int64_t n_groups, const int64_t *offsets, const int64_t *indices, int n_slots,
                          const agp_gradient_slot *slots, const double *tangents, int64_t ldt, double *logo_nll,
                          double *grad_logo_nll, double *mean_weights) {
  return agp_logo_nll_gradient_typed(c, k, x, y, y_var, n_groups, offsets, indices, AGP_PREDICT_JOINT, n_slots, slots, tangents, ldt,
                                     logo_nll, grad_logo_nll, mean_weights, nullptr);
}

int agp_logo_nll_gradient_typed(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                                int64_t n_groups, const int64_t *offsets, const int64_t *indices, int predict_type, int n_slots,
                                const agp_gradient_slot *slots, const double *tangents, int64_t ldt, double *logo_nll,
                                double *grad_logo_nll, double *mean_weights, double *group_nll) {
  if (!c || !k || !x || !y || !logo_nll) return AGP_ERR_INVALID_ARGUMENT;
  if (predict_type != AGP_PREDICT_JOINT && predict_type != AGP_PREDICT_MARGINAL) return AGP_ERR_INVALID_ARGUMENT;
  const bool marginal = predict_type == AGP_PREDICT_MARGINAL;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && (!slots || !grad_logo_nll)))
    return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  LogoPlan plan;
  if ((st = logo_plan(n, n_groups, offsets, indices, plan)) != AGP_OK) return st;
  const bool need_c = n_slots > 0 || mean_weights;  // value only: the blocks from gathered columns of R, no C, H or S
  const bool need_h = n_slots > 0;
  const BatchGeometry geo = batch_geometry(n, 1);
  auto carve = [&](WsLayout &w) {
    return carve_logo(w, geo, need_h, plan.block_elems, plan.img_elems, plan.vec_elems, plan.count_elems,
                      (size_t)round_up(plan.terms > 0 ? plan.terms : 1, 2), symv_ws_elems(n), plan.meta.size());
  };
  WsLayout size_own;
  carve(size_own);
  GradientCall g;
  st = gradient_setup(ctx, k, x, y, y_var, n_slots, slots, tangents, ldt, size_own.bytes() / sizeof(double), g);
  if (st != AGP_OK) return st;
  WsLayout own(g.extra);
  const LogoRegions r = carve(own);
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling;
  if (!plan.meta.empty()) {
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(r.meta, plan.meta.data(), sizeof(long long) * plan.meta.size(), hipMemcpyHostToDevice, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // (pageable source)
  }
  if ((st = alpha_and_inverse_factor(ctx, g)) != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), s));
  if (need_c) {
    launch_rtr_lower(s, g.R, g.lda, n, g.A, g.lda);  // C = K^-1 over L
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[4], s));
    const unsigned mt = (unsigned)((n + GF_T - 1) / GF_T);
    hipLaunchKernelGGL(mirror_lower_kernel, dim3(mt, mt), dim3(256), 0, s, g.A, g.lda, n, 0LL);
    AGP_HIP_CHECK(ctx, hipMemsetAsync(r.a, 0, sizeof(double) * (size_t)geo.np2, s));
    if (need_h) AGP_HIP_CHECK(ctx, hipMemsetAsync(g.R, 0, sizeof(double) * geo.slabs(), s));  // H over R
  }
  for (const LogoChunk &ch : plan.chunks) logo_chunk(ctx, g, r, ch, need_c, need_h, marginal);
  launch_logo_sum(s, r.term, plan.terms, ctx->d_scalars + 2);
  if (need_c) launch_symv_lower(s, g.A, g.lda, n, r.a, 1., 0., nullptr, r.u, r.symv);  // u = C a
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
  if (need_h) {
    launch_hct_lower_batched(s, g.R, g.lda, 0, g.A, g.lda, 0, n, r.S, g.lda, 0, 1);  // S = C B C
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[6], s));
    contract_slots<true>(s, k, n_slots, slots, g, r.u, 1.0, r.S);
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[7], s));
  }
  AGP_HIP_CHECK(ctx, hipGetLastError());
  std::vector<double> h_grad((size_t)n_slots), h_u(mean_weights ? (size_t)n : 0), h_term(group_nll ? (size_t)plan.terms : 0);
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_flags, ctx->d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  if (!h_term.empty()) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_term.data(), r.term, sizeof(double) * h_term.size(), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_slots > 0) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_grad.data(), g.grad_d, sizeof(double) * (size_t)n_slots, hipMemcpyDeviceToHost, s));
  if (mean_weights) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_u.data(), r.u, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  if ((st = status_from_flags(ctx)) != AGP_OK) return st;  // a group block that did not factor: nothing is written
  *logo_nll = ctx->h_scalars[2];
  if (n_slots > 0) std::memcpy(grad_logo_nll, h_grad.data(), sizeof(double) * (size_t)n_slots);
  if (mean_weights) std::memcpy(mean_weights, h_u.data(), sizeof(double) * (size_t)n);
  if (group_nll) {  // the terms are in the plan's order (by size) and hold 2 NLL_g; an empty group has none
    std::fill(group_nll, group_nll + n_groups, 0.);
    for (size_t q = 0; q < h_term.size(); ++q) group_nll[plan.group[q]] = 0.5 * h_term[q];
  }
  if (prof) {
    // 2: alpha and R = L^-1; value only: 8 the group blocks and terms; otherwise 6 R^T R, 8 the mirror, the group blocks,
    // u and H, 9 the product, 7 the contraction
    ctx->stage_ms[6] = ctx->stage_ms[7] = ctx->stage_ms[8] = ctx->stage_ms[9] = 0.;
    ctx->stage_ms[2] = elapsed(ctx->stage_ev[2], ctx->stage_ev[3]);
    if (!need_c) {
      ctx->stage_ms[8] = elapsed(ctx->stage_ev[3], ctx->stage_ev[5]);
    } else {
      ctx->stage_ms[6] = elapsed(ctx->stage_ev[3], ctx->stage_ev[4]);
      ctx->stage_ms[8] = elapsed(ctx->stage_ev[4], ctx->stage_ev[5]);
      if (need_h) {
        ctx->stage_ms[9] = elapsed(ctx->stage_ev[5], ctx->stage_ev[6]);
        ctx->stage_ms[7] = elapsed(ctx->stage_ev[6], ctx->stage_ev[7]);
      }
    }
  }
  return AGP_OK;
}

}  // extern "C"

// ---- the steps both batched gradients share ----------------------------------------------------------------------
// Everything agp_nll_gradient_batch and agp_loo_nll_gradient_batch do up to and including C_b = R_b^T R_b, and the
// download at the end.  Workspaces (batch_layout.h): ws_A by carve_gradient_batch, ws_aux by carve_gradient_batch_aux.
struct GradientBatch {
  long long n = 0, lda = 0, np2 = 0, cp2 = 0, stride_A = 0, tiles = 0, ldgd = 0;
  int groups = 0, max_slots = 0, dim_max = 1;
  double *A = nullptr, *z = nullptr, *yvar_d = nullptr;
  double *logsum = nullptr;  // [logsum | quad | flags]: what gradient_batch_finish downloads
  double *quad = nullptr;    // one scalar per problem: z_b^T z_b (NLL) or the leave-one-out sum
  int *flags = nullptr;      // 4 status words per problem
  double *R = nullptr, *grad_d = nullptr, *extra = nullptr;
  ContractDesc *desc_d = nullptr;
  const ContractDesc *rows_d = nullptr;  // desc_d when some problem has phantom rows (loo_terms_kernel: rows), else null
  std::vector<long long> nb;             // the real rows of every problem
  long long count = 0;
  double *vector(int k) const { return extra + (size_t)k * (size_t)count * (size_t)np2; }  // extra array k (np2 x count)
};

// The argument checks of both entries (every problem is checked before anything is written or launched), then the
// shared front end (batch_front.h) - memory from ws_A and ws_aux, status words per problem, the look-ahead schedule where
// the predicate asks for it - and after the factor alpha_b in place and R_b = L_b^-1 into the second slab (stage event
// 3), then with `rtr` K_b^-1 = R_b^T R_b over L_b (stage event 4).
// vec / ldvec: the entry's n x count host output, checked only.  quad: z_b^T z_b before alpha overwrites z.
// extra_vectors: further np2 x count arrays behind the descriptors, laid out like z (GradientBatch::vector(k): array k,
// problem b's vector at + b * np2); u_vector >= 0: the array that holds every problem's u, for the descriptors;
// weight_vector >= 0: the contraction's weight slabs (ld lda, stride_A apart) start at that array instead of at A.
//
// `ragged` (the _ragged entries) admits problems of unequal sizes n_b, as fit_create_batch does (api.hip).  The padded size
// n of the call is the largest of them and problem b is diag(K_b, I): column b of the targets, the variances and the
// tangents holds n_b values that go up in copies of their own (device inputs: one table-driven copy launch), the Gram
// launches run on the views of n_b rows, and ONE pad launch behind them writes the phantom rows of slab b as identity rows
// and z_b[n_b .. n) = 0.  No covariance is ever evaluated on a phantom row, so the pad items carry no features.  The
// factor, alpha, R and R^T R then run at size n on diag(L_b, I), diag(R_b, I) and diag(C_b, I).  The descriptors hold the
// views of n_b rows, which is what masks the phantom pairs of the contraction (contract_lower) and tells the leave-one-out
// kernels the real rows (GradientBatch::rows_d).  With all sizes equal nothing of this runs: the launches and the bits
// are those of the equal-size call.
static int gradient_batch_begin(agp_context_impl *ctx, int count, const agp_kernel *const *kernels,
                                const agp_features *const *features, const double *y, int64_t ldy, const double *y_var,
                                int64_t ldv, const int *n_slots, const agp_gradient_slot *const *slots,
                                const double *const *tangents, int64_t ldt, const double *grad, int64_t ldg, const double *vec,
                                int64_t ldvec, bool quad, bool rtr, int extra_vectors, int u_vector, bool ragged,
                                int weight_vector, GradientBatch &g) {
  long long n = 0;
  bool equal = true;
  int st = ragged ? check_batch_problems_ragged(count, kernels, features, ldy, y_var, ldv, &n, &equal)
                  : check_batch_problems(count, kernels, features, ldy, y_var, ldv, &n);
  if (st != AGP_OK) return st;
  const bool padded = !equal;  // some problem has phantom rows
  if (vec && ldvec < n) return AGP_ERR_INVALID_ARGUMENT;
  int max_slots = 0, dim_max = 1;
  std::vector<int> ntc((size_t)count, 0);
  for (int b = 0; b < count; ++b) {
    const int ns = n_slots[b];
    if (ns < 0 || ns > AGP_MAX_GRADIENT_SLOTS || (ns > 0 && (!slots || !slots[b]))) return AGP_ERR_INVALID_ARGUMENT;
    if ((st = check_slots(kernels[b], ns, ns > 0 ? slots[b] : nullptr, &ntc[(size_t)b])) != AGP_OK) return st;
    if (ntc[(size_t)b] > 0 && (!tangents || !tangents[b] || ldt < n)) return AGP_ERR_INVALID_ARGUMENT;
    if (ns > max_slots) max_slots = ns;
    if (features[b]->dim > dim_max) dim_max = features[b]->dim;
  }
  if (max_slots > 0 && (!grad || ldg < max_slots)) return AGP_ERR_INVALID_ARGUMENT;
  const long long tiles = lower_tiles(n), rtr_tiles = ((n + GT - 1) / GT) * ((n + GT - 1) / GT + 1) / 2;
  const int groups = (max_slots + GRAD_GROUP - 1) / GRAD_GROUP;
  if (tiles * CT_THREADS > (long long)UINT_MAX || rtr_tiles * GEMM_THREADS > (long long)UINT_MAX ||
      tiles * count > (long long)UINT_MAX || rtr_tiles * count > (long long)UINT_MAX)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));

  const BatchGeometry geo = batch_geometry(n, count);
  const long long lda = geo.lda, np2 = geo.np2, cp2 = geo.cp2, stride_A = geo.stride_A, stride_I = geo.stride_I;
  const long long ldgd = round_up(max_slots > 0 ? max_slots : 1, 2);  // device gradient: [count][ldgd]
  const long long part_per = (long long)groups * tiles * GRAD_GROUP;  // partials per problem
  const int loc = features[0]->location;
  const bool fused_panels = batched_fused_panels(ctx, geo, /*allow_lookahead=*/true);
  long long tang_elems = 0;
  if (loc == AGP_HOST)
    for (int b = 0; b < count; ++b) tang_elems += (long long)ntc[(size_t)b] * np2;
  const size_t gram_bytes = gram_batch_table_bytes(count), desc_bytes = sizeof(ContractDesc) * (size_t)count;
  // a padded call: behind the descriptors, in the same region and the same upload, the pad table and (device inputs) the
  // copy table of the targets and variances
  const size_t pad_off = (desc_bytes + 15) / 16 * 16, pad_bytes = padded ? sizeof(RaggedPadItem) * (size_t)count : 0;
  const size_t copy_off = pad_off + pad_bytes;
  const size_t copy_cap = padded && loc != AGP_HOST ? sizeof(CopyItem) * (size_t)count * (y_var ? 2 : 1) : 0;
  const size_t tables_bytes = padded ? copy_off + copy_cap : desc_bytes;
  auto carve_aux = [&](WsLayout &w) {
    return carve_gradient_batch_aux(w, geo, (size_t)tang_elems, (size_t)part_per, (size_t)ldgd, gram_bytes, tables_bytes, (size_t)extra_vectors);
  };
  WsLayout size_A, size_aux;
  carve_gradient_batch(size_A, geo, y_var != nullptr, fused_panels);
  carve_aux(size_aux);
  if ((st = reserve_ws(ctx, ctx->ws_A, size_A.bytes())) != AGP_OK) return st;
  if ((st = reserve_ws(ctx, ctx->ws_aux, size_aux.bytes())) != AGP_OK) return st;
  WsLayout ws_A(ctx->ws_A), ws_aux(ctx->ws_aux);
  const GradientBatchRegions r = carve_gradient_batch(ws_A, geo, y_var != nullptr, fused_panels);
  const GradientBatchAuxRegions a = carve_aux(ws_aux);
  double *A = r.A, *invd = r.invd, *z = r.z, *R = a.R;
  ContractDesc *desc_d = static_cast<ContractDesc *>(a.desc);
  g.count = count; g.n = n; g.lda = lda; g.np2 = np2; g.cp2 = cp2; g.stride_A = stride_A; g.tiles = tiles; g.ldgd = ldgd;
  g.groups = groups; g.max_slots = max_slots; g.dim_max = dim_max;
  g.A = A; g.z = z; g.yvar_d = r.yvar; g.logsum = r.logsum; g.quad = r.quad; g.flags = r.flags; g.R = R; g.grad_d = a.grad; g.desc_d = desc_d;
  g.extra = a.extra;
  g.rows_d = padded ? desc_d : nullptr;
  g.nb.resize((size_t)count);
  for (int b = 0; b < count; ++b) g.nb[(size_t)b] = features[b]->n;
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling;

  std::vector<CopyItem> copies;  // (a padded call with device inputs)
  long long copy_max = 0;
  if (!padded) {
    if ((st = upload_problem_columns(ctx, y, ldy, n, count, loc, z, np2)) != AGP_OK) return st;
    if (y_var && (st = upload_problem_columns(ctx, y_var, ldv, n, count, loc, r.yvar, np2)) != AGP_OK) return st;
  } else {
    // the n_b values of column b; what follows them in the column is never read
    for (int b = 0; b < count; ++b) {
      const long long nb = g.nb[(size_t)b];
      const double *src[2] = {y + (size_t)b * (size_t)ldy, y_var ? y_var + (size_t)b * (size_t)ldv : nullptr};
      double *dst[2] = {z + (size_t)b * (size_t)np2, y_var ? r.yvar + (size_t)b * (size_t)np2 : nullptr};
      for (int k = 0; k < 2; ++k) {
        if (!src[k]) continue;
        if (loc == AGP_HOST) {
          AGP_HIP_CHECK(ctx, hipMemcpyAsync(dst[k], src[k], sizeof(double) * (size_t)nb, hipMemcpyHostToDevice, s));
        } else {
          copies.push_back(CopyItem{reinterpret_cast<unsigned long long *>(dst[k]), reinterpret_cast<const unsigned long long *>(src[k]), nb});
          if (nb > copy_max) copy_max = nb;
        }
      }
    }
  }
  // tangent columns: host columns are copied into the workspace (leading dimension np2), device ones are read in place
  std::vector<const double *> tcol((size_t)count, nullptr);
  std::vector<long long> tld((size_t)count, 0);
  {
    double *tcur = a.tang;
    for (int b = 0; b < count; ++b) {
      if (ntc[(size_t)b] == 0) continue;
      if ((st = stage_tangents(ctx, s, tangents[b], ldt, loc, g.nb[(size_t)b], ntc[(size_t)b], &tcur, &tcol[(size_t)b], &tld[(size_t)b])) != AGP_OK)
        return st;
    }
  }
  BatchGramTables gram(geo, kernels, A, r.yvar, np2, r.flags, 4);
  if ((st = gram.upload_features(ctx, features)) != AGP_OK) return st;
  if (loc == AGP_HOST) AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // (pageable sources)
  {  // log sums, quadratic terms and flags zeroed; the hand-over buffers of the fused panel launches sentinel-filled
    PrepArgs prep;
    prep.fill(r.logsum, 0ull, 4 * cp2);
    launch_batch_prep(s, prep, geo, invd, r.zpub);
  }
  // the contraction's descriptors, built in the pinned staging area behind the Gram table's, as they lie on the device
  const size_t desc_off = (size_t)(static_cast<char *>(a.desc) - static_cast<char *>(a.gram_table));
  char *pinned = static_cast<char *>(host_stage(ctx, desc_off + tables_bytes));
  std::vector<double> desc_pageable;  // (doubles: aligned as the tables need it)
  char *tables_h = nullptr;
  if (pinned) tables_h = pinned + desc_off;
  else { desc_pageable.resize((tables_bytes + sizeof(double) - 1) / sizeof(double)); tables_h = reinterpret_cast<char *>(desc_pageable.data()); }
  ContractDesc *desc_h = reinterpret_cast<ContractDesc *>(tables_h);
  for (int b = 0; b < count; ++b) {
    fill_contract_desc(desc_h[b], kernels[b], gram.views[(size_t)b],
                       (weight_vector >= 0 ? g.vector(weight_vector) : A) + (size_t)b * (size_t)stride_A, lda, z + (size_t)b * (size_t)np2,
                       u_vector >= 0 ? g.vector(u_vector) + (size_t)b * (size_t)np2 : nullptr, a.partial + (size_t)b * (size_t)part_per,
                       n_slots[b], n_slots[b] > 0 ? slots[b] : nullptr, tcol[(size_t)b], tld[(size_t)b]);
  }
  const size_t copy_bytes = sizeof(CopyItem) * copies.size();
  if (padded) {
    RaggedPadItem *pads = reinterpret_cast<RaggedPadItem *>(tables_h + pad_off);
    for (int b = 0; b < count; ++b) {  // the slab and z only: no phantom feature rows (dim = nsc = 0, no ids)
      RaggedPadItem &pi = pads[b];
      std::memset(static_cast<void *>(&pi), 0, sizeof(RaggedPadItem));
      pi.A = A + (size_t)b * (size_t)stride_A;
      pi.z = z + (size_t)b * (size_t)np2;
      pi.nb = g.nb[(size_t)b];
    }
    if (copy_bytes > 0) std::memcpy(tables_h + copy_off, copies.data(), copy_bytes);
  }
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(desc_d, tables_h, padded ? copy_off + copy_bytes : desc_bytes, hipMemcpyHostToDevice, s));
  if (!pinned) AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // (pageable source)
  const char *tables_d = reinterpret_cast<const char *>(desc_d);
  if (!copies.empty()) launch_copy_table(s, reinterpret_cast<const CopyItem *>(tables_d + copy_off), (long long)copies.size(), copy_max);

  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[0], s));
  if ((st = launch_batch_grams(ctx, geo, gram, kernels, a.gram_table, pinned)) != AGP_OK) return st;
  if (padded) launch_ragged_pad(s, reinterpret_cast<const RaggedPadItem *>(tables_d + pad_off), count, n, lda);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
  factor_batch(ctx, geo, /*allow_lookahead=*/true, A, invd, z, r.flags, 4, r.logsum, r.zpub);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
  // y^T K^-1 y = z^T z, alpha = L^-T z in place, R = L^-1 (triangular right-hand side) into the second slab.  A failed
  // problem runs on through here and through the entry's own steps on whatever its factor holds: every launch has fixed
  // trip counts and none waits on another workgroup's data, so it costs nothing but its own (discarded) results.
  if (quad) launch_coldot(s, z, np2, z, np2, n, count, g.quad, -1.0, nullptr);
  backward_solve_vec_batched(s, A, stride_A, n, lda, invd, stride_I, z, np2, count);
  launch_set_identity_batched(s, R, lda, stride_A, n, count);
  forward_solve_mat_batched(s, A, stride_A, n, lda, invd, stride_I, R, stride_A, n, lda, /*rhs_lower=*/true, count);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[3], s));
  if (rtr) {
    launch_rtr_lower_batched(s, R, lda, stride_A, n, A, lda, stride_A, count);  // K_b^-1 over L_b
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[4], s));
  }
  return AGP_OK;
}

// [logsum | quad | flags], the gradients and (when asked for) every vec_d column: three transfers, one synchronisation;
// then the host outputs.  value(n_b, logsum_b, quad_b): the objective of a problem of n_b (real) rows.  A failed problem gets
// NaN for its value and its gradient column and keeps its column of vec; a good one receives the n_b values of its column.
template <class Value>
static int gradient_batch_finish(agp_context_impl *ctx, const GradientBatch &g, int count, const int *n_slots, Value value,
                                 double *values, double *grad, int64_t ldg, const double *vec_d, double *vec, int64_t ldvec,
                                 int *status) {
  hipStream_t s = ctx->stream;
  const long long n = g.n, cp2 = g.cp2;
  AGP_HIP_CHECK(ctx, hipGetLastError());
  std::vector<double> h_head(4 * (size_t)cp2);
  std::vector<double> h_grad(g.max_slots > 0 ? (size_t)count * (size_t)g.ldgd : 0);
  std::vector<double> h_vec(vec ? (size_t)count * (size_t)n : 0);
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_head.data(), g.logsum, sizeof(double) * h_head.size(), hipMemcpyDeviceToHost, s));
  if (g.max_slots > 0) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_grad.data(), g.grad_d, sizeof(double) * h_grad.size(), hipMemcpyDeviceToHost, s));
  if (vec)
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(h_vec.data(), sizeof(double) * (size_t)n, vec_d, sizeof(double) * (size_t)g.np2, sizeof(double) * (size_t)n,
                                        (size_t)count, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  const int *h_flags = reinterpret_cast<const int *>(h_head.data() + 2 * cp2);
  for (int b = 0; b < count; ++b)
    if (h_flags[4 * b + 2]) {  // a hand-over of the fused panel launches timed out (its producer died)
      ctx->last_error = "batched factorisation: hand-over timed out";
      return AGP_ERR_HIP;
    }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int b = 0; b < count; ++b) {
    const int *fl = h_flags + 4 * b;
    status[b] = fl[0] ? AGP_ERR_NAN_INPUT : (fl[1] ? AGP_ERR_NOT_POSITIVE_DEFINITE : AGP_OK);
    const bool ok = status[b] == AGP_OK;
    values[b] = ok ? value(g.nb[(size_t)b], h_head[(size_t)b], h_head[(size_t)cp2 + (size_t)b]) : nan;
    for (int j = 0; j < n_slots[b]; ++j) grad[(size_t)b * (size_t)ldg + (size_t)j] = ok ? h_grad[(size_t)b * (size_t)g.ldgd + (size_t)j] : nan;
    if (vec && ok) std::memcpy(vec + (size_t)b * (size_t)ldvec, h_vec.data() + (size_t)b * (size_t)n, sizeof(double) * (size_t)g.nb[(size_t)b]);
  }
  return AGP_OK;
}

// ---- agp_nll_gradient for `count` problems in lock step ----------------------------------------------------------
// The steps of agp_nll_gradient with blockIdx.y = problem: gradient_batch_begin (z_b^T z_b, alpha_b, R_b, K_b^-1 =
// R_b^T R_b over L_b), the contraction (grid x = tile, y = problem, z = slot group) and the reduction.  Workspace: the A
// and R slabs (2 lda n doubles per problem) plus the tile images (stride_I) and O(n) vectors per problem.
// `ragged`: agp_nll_gradient_batch_ragged (gradient_batch_begin); the grids keep the padded size.
static int nll_gradient_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                              const double *y, int64_t ldy, const double *y_var, int64_t ldv, const int *n_slots,
                              const agp_gradient_slot *const *slots, const double *const *tangents, int64_t ldt, double *nll,
                              double *grad_nll, int64_t ldg, double *information, int64_t ldi, int *status, bool ragged) {
  if (!c || count <= 0 || !kernels || !features || !y || !n_slots || !nll || !status) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  GradientBatch g;
  int st = gradient_batch_begin(ctx, count, kernels, features, y, ldy, y_var, ldv, n_slots, slots, tangents, ldt, grad_nll, ldg,
                                information, ldi, /*quad=*/true, /*rtr=*/true, 0, -1, ragged, -1, g);
  if (st != AGP_OK) return st;
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling;
  if (g.groups > 0) {
    launch_contract_batched<false>(s, g.dim_max, g.desc_d, g.tiles, count, g.groups);
    launch_grad_reduce_batched(s, g.desc_d, g.tiles, count, g.groups, 0.5, g.grad_d, g.ldgd);
  }
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
  st = gradient_batch_finish(ctx, g, count, n_slots,
                             [&](long long nb, double logsum, double quad) {  // likelihood.hpp:46
                               const double n_log_2pi = (double)nb * std::log(2 * M_PI);
                               return 0.5 * (2. * logsum + quad + n_log_2pi);
                             },
                             nll, grad_nll, ldg, g.z, information, ldi, status);
  if (st != AGP_OK) return st;
  if (prof) {
    for (int k : {3, 4, 5, 8, 9}) ctx->stage_ms[k] = 0.;
    ctx->stage_ms[0] = elapsed(ctx->stage_ev[0], ctx->stage_ev[1]);
    ctx->stage_ms[1] = elapsed(ctx->stage_ev[1], ctx->stage_ev[2]);
    ctx->stage_ms[2] = elapsed(ctx->stage_ev[2], ctx->stage_ev[3]);
    ctx->stage_ms[6] = elapsed(ctx->stage_ev[3], ctx->stage_ev[4]);
    ctx->stage_ms[7] = elapsed(ctx->stage_ev[4], ctx->stage_ev[5]);
  }
  return AGP_OK;
}

// ---- agp_loo_nll_gradient for `count` problems in lock step --------------------------------------------------------
// The steps of agp_loo_nll_gradient with blockIdx.y (z for the G tiles) = problem, each ONE launch for the batch:
// gradient_batch_begin (alpha_b, R_b, C_b = R_b^T R_b over L_b), the per-point terms from C_b's diagonal and their sum,
// u_b = C_b a_b (launch_symv_lower_batched), G_b over R_b, S_b = G_b^T G_b over C_b, the contraction of
// S_b - sym(u_b alpha_b^T) and the reduction.  Value only (no slots anywhere, no mean_weights): c from the squared
// column norms of the R slabs, which lie back to back and are one lda x (count n) matrix; no C, G or G^T G.
// Workspace: that of agp_nll_gradient_batch plus five vectors per problem, [term | a | sqrt_b | u | c], each an
// np2 x count array like z.
// `ragged`: agp_loo_nll_gradient_batch_ragged.  The terms kernel and the sum know every problem's real rows (g.rows_d): a
// phantom row has term = a = sqrt_b = 0, so u_b = diag(C_b, I) (a_b, 0) and G_b = diag(sqrt_b) diag(C_b, I) are zero there
// and S_b = G_b^T G_b is diag(S_b, 0); the value-only path sees c = 1 on a phantom row and never reads it.
static int loo_nll_gradient_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                                  const double *y, int64_t ldy, const double *y_var, int64_t ldv, const int *n_slots,
                                  const agp_gradient_slot *const *slots, const double *const *tangents, int64_t ldt,
                                  double *loo_nll, double *grad_loo_nll, int64_t ldg, double *mean_weights, int64_t ldw,
                                  int *status, bool ragged) {
  if (!c || count <= 0 || count > BATCH_MAX_PROBLEMS || !kernels || !features || !y || !n_slots || !loo_nll || !status)
    return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  bool need_c = mean_weights != nullptr;  // u = C a needs C = R^T R; the values alone need only diag(C)
  for (int b = 0; b < count; ++b) need_c = need_c || n_slots[b] != 0;
  enum { TERM, A_VEC, SQRT_B, U_VEC, C_DIAG, N_VECTORS };  // the extra np2 x count arrays
  GradientBatch g;
  int st = gradient_batch_begin(ctx, count, kernels, features, y, ldy, y_var, ldv, n_slots, slots, tangents, ldt, grad_loo_nll, ldg,
                                mean_weights, ldw, /*quad=*/false, /*rtr=*/need_c, N_VECTORS, U_VEC, ragged, -1, g);
  if (st != AGP_OK) return st;
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling;
  const long long n = g.n, np2 = g.np2;
  double *term = g.vector(TERM), *a = g.vector(A_VEC), *sqrt_b = g.vector(SQRT_B), *u = g.vector(U_VEC), *cdiag = g.vector(C_DIAG);
  const dim3 egrid((unsigned)((n + 255) / 256), (unsigned)count);
  if (!need_c) {
    // c_b[i] = ||R_b[:, i]||^2: count n values, contiguous (the terms kernel's cbatch = n)
    launch_coldot(s, g.R, g.lda, g.R, g.lda, n, (long long)count * n, cdiag, -1.0, nullptr);
    hipLaunchKernelGGL(loo_terms_kernel, egrid, dim3(256), 0, s, cdiag, 1LL, n, g.z, g.yvar_d, n, g.np2, term, nullptr, nullptr,
                       g.rows_d);
  } else {
    hipLaunchKernelGGL(loo_terms_kernel, egrid, dim3(256), 0, s, g.A, g.lda + 1, g.stride_A, g.z, g.yvar_d, n, g.np2, term, a, sqrt_b,
                       g.rows_d);
  }
  hipLaunchKernelGGL(loo_sum_kernel, dim3(1, (unsigned)count), dim3(1024), 0, s, term, n, np2, g.quad, g.rows_d);
  if (need_c) {
    launch_symv_lower_batched(s, g.A, g.lda, g.stride_A, n, a, np2, u, count);  // u_b = C_b a_b
    if (g.groups > 0) {
      const unsigned gt = (unsigned)((n + GF_T - 1) / GF_T);
      hipLaunchKernelGGL(loo_form_g_kernel, dim3(gt, gt, (unsigned)count), dim3(256), 0, s, g.A, g.lda, sqrt_b, n, g.R, g.lda, g.stride_A,
                         np2);  // G_b over R_b
    }
  }
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
  if (g.groups > 0) {
    launch_gtg_lower_batched(s, g.R, g.lda, g.stride_A, n, g.A, g.lda, g.stride_A, count);  // S_b = C_b diag(b) C_b over C_b
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[6], s));
    launch_contract_batched<true>(s, g.dim_max, g.desc_d, g.tiles, count, g.groups);
    launch_grad_reduce_batched(s, g.desc_d, g.tiles, count, g.groups, 1.0, g.grad_d, g.ldgd);
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[7], s));
  }
  st = gradient_batch_finish(ctx, g, count, n_slots, [](long long, double, double loo) { return loo; }, loo_nll, grad_loo_nll, ldg, u,
                             mean_weights, ldw, status);
  if (st != AGP_OK) return st;
  if (prof) {
    // whole-batch times, the indices of agp_loo_nll_gradient
    for (int k : {3, 4, 5, 6, 7, 8, 9}) ctx->stage_ms[k] = 0.;
    ctx->stage_ms[0] = elapsed(ctx->stage_ev[0], ctx->stage_ev[1]);
    ctx->stage_ms[1] = elapsed(ctx->stage_ev[1], ctx->stage_ev[2]);
    ctx->stage_ms[2] = elapsed(ctx->stage_ev[2], ctx->stage_ev[3]);
    if (!need_c) {
      ctx->stage_ms[8] = elapsed(ctx->stage_ev[3], ctx->stage_ev[5]);
    } else {
      ctx->stage_ms[6] = elapsed(ctx->stage_ev[3], ctx->stage_ev[4]);
      ctx->stage_ms[8] = elapsed(ctx->stage_ev[4], ctx->stage_ev[5]);
      if (g.groups > 0) {
        ctx->stage_ms[9] = elapsed(ctx->stage_ev[5], ctx->stage_ev[6]);
        ctx->stage_ms[7] = elapsed(ctx->stage_ev[6], ctx->stage_ev[7]);
      }
    }
  }
  return AGP_OK;
}

// ---- agp_logo_nll_gradient for `count` problems in lock step ---------------------------------------------------------
// gradient_batch_begin as for the leave-one-out batch (alpha_b, R_b, C_b = R_b^T R_b over L_b; `ragged`, so problem b is
// diag(K_b, I) at the padded size), C_b mirrored (ONE launch, blockIdx.z = problem), then the group-block chain ONCE for the
// groups of ALL problems: the pooled plan (logo_batch_plan.h) sorts them by (size, problem, group) and cuts them into
// chunks, each chunk is the chain of logo_chunk_run with every group's problem in its table (LogoProblems), so the number
// of chains follows the size classes of the batch.  The blocks ALWAYS come from C_b, value-only calls included (no
// gathered columns of R: at these sizes R^T R is a small share and one route is one chain to get right); a value-only
// call forms no a, H or S.  Phantom rows belong to no group (the plan refuses an index >= n_b), so they appear in no block,
// a_b and the columns of H_b are zero there, and the descriptors mask the phantom pairs of the contraction.
// Then ONE launch sums every problem's terms in a fixed order and folds its groups' status words into its own
// (logo_problem_sum_kernel), u_b = C_b a_b (launch_symv_lower_batched), S_b = H_b C_b^T into a third slab per problem
// (launch_hct_lower_batched), and the contraction of S_b - sym(u_b alpha_b^T) with the descriptors pointing at S_b.
// Every stage is a plain launch on the context's stream; nothing waits on the host between the uploads and the download.
// Workspace (carve_logo_batch, behind the arrays a and u): the third slab per problem (gradient calls), three block slabs
// and the tile images of the chunk in flight (at most count * n padded columns), O(terms) vectors and the tables.
extern "C" int agp_logo_nll_gradient_batch(agp_context *c, int count, const agp_kernel *const *kernels,
                                           const agp_features *const *features, const double *y, int64_t ldy, const double *y_var,
                                           int64_t ldv, const int64_t *n_groups, const int64_t *const *offsets,
                                           const int64_t *const *indices, int predict_type, const int *n_slots,
                                           const agp_gradient_slot *const *slots, const double *const *tangents, int64_t ldt,
                                           double *logo_nll, double *grad_logo_nll, int64_t ldg, double *mean_weights, int64_t ldw,
                                           double *const *group_nll, int *status) {
  if (!c || count <= 0 || count > BATCH_MAX_PROBLEMS || !kernels || !features || !y || !n_groups || !n_slots || !logo_nll || !status)
    return AGP_ERR_INVALID_ARGUMENT;
  if (predict_type != AGP_PREDICT_JOINT && predict_type != AGP_PREDICT_MARGINAL) return AGP_ERR_INVALID_ARGUMENT;
  const bool marginal = predict_type == AGP_PREDICT_MARGINAL;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  bool need_h = false;  // some problem has a slot: H and S
  std::vector<long long> nb((size_t)count);
  long long n_max = 0;
  for (int b = 0; b < count; ++b) {
    if (!features[b] || features[b]->n <= 0) return AGP_ERR_INVALID_ARGUMENT;
    nb[(size_t)b] = features[b]->n;
    n_max = std::max(n_max, nb[(size_t)b]);
    need_h = need_h || n_slots[b] > 0;
  }
  const bool need_grad = need_h || mean_weights;  // the gradient's half of the chain: a, u (and B_g)
  LogoBatchPlan plan;
  const LogoBatchLimits lim{logo_chunk_groups_max(), logo_chunk_img_elems_max(), (long long)count * n_max, factor_ld, logo_img_stride};
  if (!logo_batch_plan(count, nb.data(), n_groups, offsets, indices, lim, plan)) return AGP_ERR_INVALID_ARGUMENT;

  const BatchGeometry geo = batch_geometry(n_max, count);
  const size_t term_elems = (size_t)round_up(plan.terms > 0 ? plan.terms : 1, 2);
  auto carve = [&](WsLayout &w) {
    return carve_logo_batch(w, geo, need_h, plan.block_elems, plan.img_elems, plan.vec_elems, plan.count_elems, term_elems, plan.meta.size());
  };
  WsLayout size_own;
  carve(size_own);
  enum { A_VEC, U_VEC, OWN };  // the extra np2 x count arrays: a, u, then the entry's own region (S first)
  const size_t per_vector = sizeof(double) * geo.vectors();
  const int extra_vectors = OWN + (int)((size_own.bytes() + per_vector - 1) / per_vector);
  GradientBatch g;
  int st = gradient_batch_begin(ctx, count, kernels, features, y, ldy, y_var, ldv, n_slots, slots, tangents, ldt, grad_logo_nll, ldg,
                                mean_weights, ldw, /*quad=*/false, /*rtr=*/true, extra_vectors, U_VEC, /*ragged=*/true,
                                need_h ? OWN : -1, g);
  if (st != AGP_OK) return st;
  hipStream_t s = ctx->stream;
  // The plan's tables go up and the terms come down without a synchronisation of their own: both host vectors outlive the
  // call's one synchronisation (gradient_batch_finish), and on an early return this drains the stream before they go.
  std::vector<double> h_term;
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  const bool prof = ctx->profiling;
  const long long n = g.n, np2 = g.np2;
  WsLayout own(g.vector(OWN));
  const LogoBatchRegions rb = carve(own);
  const LogoRegions &r = rb.chain;
  double *a = g.vector(A_VEC), *u = g.vector(U_VEC);
  int *flags = g.flags;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(r.meta, plan.meta.data(), sizeof(long long) * plan.meta.size(), hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(rb.gflags, 0, sizeof(int) * 4 * term_elems, s));
  const unsigned mt = (unsigned)((n + GF_T - 1) / GF_T);
  hipLaunchKernelGGL(mirror_lower_kernel, dim3(mt, mt, (unsigned)count), dim3(256), 0, s, g.A, g.lda, n, g.stride_A);
  if (need_grad) AGP_HIP_CHECK(ctx, hipMemsetAsync(a, 0, sizeof(double) * geo.vectors(), s));
  if (need_h) AGP_HIP_CHECK(ctx, hipMemsetAsync(g.R, 0, sizeof(double) * geo.slabs(), s));  // H_b over R_b
  const LogoChainArgs chain{n, g.lda, g.A, g.R, a, g.R, g.z, g.yvar_d};
  for (const LogoBatchChunk &bc : plan.chunks) {
    const LogoChunk ch{bc.m, bc.count, bc.idx_off, bc.size_off, bc.term_off};
    const LogoProblems P{r.meta + bc.prob_off, g.stride_A, np2, flags};
    logo_chunk_run(ctx, chain, r, ch, /*from_c=*/true, need_grad, need_h, marginal, P, rb.gflags + 4 * bc.term_off);
  }
  hipLaunchKernelGGL(logo_problem_sum_kernel, dim3((unsigned)count), dim3(256), 0, s, r.term, rb.gflags, r.meta + plan.csr_at,
                     r.meta + plan.csr_terms_at, g.z, np2, g.desc_d, g.quad, flags);
  if (need_grad) launch_symv_lower_batched(s, g.A, g.lda, g.stride_A, n, a, np2, u, count);  // u_b = C_b a_b
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
  if (need_h) {
    launch_hct_lower_batched(s, g.R, g.lda, g.stride_A, g.A, g.lda, g.stride_A, n, r.S, g.lda, g.stride_A, count);  // S_b = C_b B_b C_b
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[6], s));
    launch_contract_batched<true>(s, g.dim_max, g.desc_d, g.tiles, count, g.groups);
    launch_grad_reduce_batched(s, g.desc_d, g.tiles, count, g.groups, 1.0, g.grad_d, g.ldgd);
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[7], s));
  }
  bool want_terms = false;
  if (group_nll)
    for (int b = 0; b < count; ++b) want_terms = want_terms || (group_nll[b] && n_groups[b] > 0);
  if (want_terms) h_term.resize((size_t)plan.terms);
  if (!h_term.empty()) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_term.data(), r.term, sizeof(double) * h_term.size(), hipMemcpyDeviceToHost, s));
  st = gradient_batch_finish(ctx, g, count, n_slots, [](long long, double, double logo) { return logo; }, logo_nll, grad_logo_nll, ldg,
                             u, mean_weights, ldw, status);
  if (st != AGP_OK) return st;
  if (want_terms) {  // the terms hold 2 NLL_g in the plan's order; an empty group has none; a failed problem's are NaN
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int b = 0; b < count; ++b)
      if (group_nll[b]) std::fill(group_nll[b], group_nll[b] + n_groups[b], status[b] == AGP_OK ? 0. : nan);
    for (size_t q = 0; q < h_term.size(); ++q) {
      const long long b = plan.problem[q];
      if (group_nll[b] && status[b] == AGP_OK) group_nll[b][plan.group[q]] = 0.5 * h_term[q];
    }
  }
  if (prof) {
    // whole-batch times, the indices of agp_logo_nll_gradient: 6 R^T R, 8 the mirror, the group blocks, the sums, u and H,
    // 9 the products H C^T, 7 the contraction
    for (int k : {3, 4, 5, 6, 7, 8, 9}) ctx->stage_ms[k] = 0.;
    ctx->stage_ms[0] = elapsed(ctx->stage_ev[0], ctx->stage_ev[1]);
    ctx->stage_ms[1] = elapsed(ctx->stage_ev[1], ctx->stage_ev[2]);
    ctx->stage_ms[2] = elapsed(ctx->stage_ev[2], ctx->stage_ev[3]);
    ctx->stage_ms[6] = elapsed(ctx->stage_ev[3], ctx->stage_ev[4]);
    ctx->stage_ms[8] = elapsed(ctx->stage_ev[4], ctx->stage_ev[5]);
    if (need_h) {
      ctx->stage_ms[9] = elapsed(ctx->stage_ev[5], ctx->stage_ev[6]);
      ctx->stage_ms[7] = elapsed(ctx->stage_ev[6], ctx->stage_ev[7]);
    }
  }
  return AGP_OK;
}

extern "C" {

int agp_nll_gradient_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                           const double *y, int64_t ldy, const double *y_var, int64_t ldv, const int *n_slots,
                           const agp_gradient_slot *const *slots, const double *const *tangents, int64_t ldt, double *nll,
                           double *grad_nll, int64_t ldg, double *information, int64_t ldi, int *status) {
  return nll_gradient_batch(c, count, kernels, features, y, ldy, y_var, ldv, n_slots, slots, tangents, ldt, nll, grad_nll, ldg,
                            information, ldi, status, false);
}

int agp_nll_gradient_batch_ragged(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                                  const double *y, int64_t ldy, const double *y_var, int64_t ldv, const int *n_slots,
                                  const agp_gradient_slot *const *slots, const double *const *tangents, int64_t ldt, double *nll,
                                  double *grad_nll, int64_t ldg, double *information, int64_t ldi, int *status) {
  return nll_gradient_batch(c, count, kernels, features, y, ldy, y_var, ldv, n_slots, slots, tangents, ldt, nll, grad_nll, ldg,
                            information, ldi, status, true);
}

int agp_loo_nll_gradient_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                               const double *y, int64_t ldy, const double *y_var, int64_t ldv, const int *n_slots,
                               const agp_gradient_slot *const *slots, const double *const *tangents, int64_t ldt,
                               double *loo_nll, double *grad_loo_nll, int64_t ldg, double *mean_weights, int64_t ldw,
                               int *status) {
  return loo_nll_gradient_batch(c, count, kernels, features, y, ldy, y_var, ldv, n_slots, slots, tangents, ldt, loo_nll,
                                grad_loo_nll, ldg, mean_weights, ldw, status, false);
}

int agp_loo_nll_gradient_batch_ragged(agp_context *c, int count, const agp_kernel *const *kernels,
                                      const agp_features *const *features, const double *y, int64_t ldy, const double *y_var,
                                      int64_t ldv, const int *n_slots, const agp_gradient_slot *const *slots,
                                      const double *const *tangents, int64_t ldt, double *loo_nll, double *grad_loo_nll,
                                      int64_t ldg, double *mean_weights, int64_t ldw, int *status) {
  return loo_nll_gradient_batch(c, count, kernels, features, y, ldy, y_var, ldv, n_slots, slots, tangents, ldt, loo_nll,
                                grad_loo_nll, ldg, mean_weights, ldw, status, true);
}

}  // extern "C"
