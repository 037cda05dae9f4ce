// contract.h — the contraction every gradient ends in: partial[tile][g] = sum over the tile's pairs of
// w(row, col) dk(row, col) / dslot_g, the weight w against the tangent form of the covariance program (cov_eval.h:
// eval_pair_tangent), which never stores dK / dtheta.  One workgroup per CT x CT tile; lane = row (coalesced reads of
// the weight's column), each wave walks CT / 4 columns whose point is the same for the whole wave.  No float atomics:
// per-tile partial sums and fixed-order reductions, so two calls give bit-identical results.  The kernels
// (gradient.hip, sparse_gradient.hip) differ in how a tile id becomes a ContractTile and in the weight.
#pragma once
#include "cov_eval.h"

namespace agp {

constexpr int GRAD_GROUP = 4;  // slots per walk of the tangent program (the weight is read ceil(P / GRAD_GROUP) times)
constexpr int CT = 64;         // contraction tile edge
constexpr int CT_THREADS = 256;

// row-major enumeration of the lower tiles: id = bi (bi + 1) / 2 + bj, bi >= bj
__device__ __forceinline__ void lower_tile(long long id, int &bi, int &bj) {
  bi = (int)((sqrt(8. * (double)id + 1.) - 1.) * 0.5);
  while ((long long)bi * (bi + 1) / 2 > id) --bi;
  while ((long long)(bi + 1) * (bi + 2) / 2 <= id) ++bi;
  bj = (int)(id - (long long)bi * (bi + 1) / 2);
}

// lower tiles of an n x n weight
inline long long lower_tiles(long long n) {
  const long long t = (n + CT - 1) / CT;
  return t * (t + 1) / 2;
}

// Tile (bi, bj) of a weight with nrl x ncl local rows and columns; local row 0 / column 0 is point rbase / cbase of the
// row / column features.  lower: only the pairs row >= col, the strictly lower ones twice.
struct ContractTile {
  int bi, bj;
  long long rbase, cbase, nrl, ncl;
  bool lower;
};

// The unscaled weight of the pair (local row il, local column jl); row(il) is called once, before the columns.
struct NllWeight {  // K^-1_ij - alpha_i alpha_j
  const double *C;
  long long ldc;
  const double *alpha;
  double ai = 0.;  // alpha of the row
  __device__ void row(long long il) { ai = alpha[il]; }
  __device__ double operator()(long long il, long long jl) const { return C[il + jl * ldc] - ai * alpha[jl]; }
};
struct LooWeight {  // S_ij - 1/2 (u_i alpha_j + alpha_i u_j)
  const double *S;
  long long lds;
  const double *alpha, *u;
  double ai = 0., ui = 0.;
  __device__ void row(long long il) { ai = alpha[il]; ui = u[il]; }
  __device__ double operator()(long long il, long long jl) const { return S[il + jl * lds] - 0.5 * (ui * alpha[jl] + ai * u[jl]); }
};
struct MatrixWeight {  // W_ij
  const double *W;
  long long ldw;
  __device__ void row(long long) {}
  __device__ double operator()(long long il, long long jl) const { return W[il + jl * ldw]; }
};

// partial[id][g] = the workgroup's sum of acc[g] in a fixed order: butterfly inside the wave, then the four waves in order
__device__ __forceinline__ void reduce_tile(const double (&acc)[GRAD_GROUP], long long id, double *partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double red[CT_THREADS / 64][GRAD_GROUP];
#pragma unroll
  for (int g = 0; g < GRAD_GROUP; ++g) {
    double v = acc[g];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][g] = v;
  }
  __syncthreads();
  if (threadIdx.x < GRAD_GROUP) {
    const int g = threadIdx.x;
    double v = red[0][g];
#pragma unroll
    for (int w = 1; w < CT_THREADS / 64; ++w) v += red[w][g];
    partial[id * GRAD_GROUP + g] = v;
  }
}

// The tile body of every contraction kernel.  R / C: the row / column features (with the measurement / equality
// semantics of the Gram call that built the weighted matrix), tr[g] / tc[g]: the tangent column of AGP_OP_SCALING slot g
// at the row / column features, else nullptr.  The whole workgroup must call it (reduce_tile synchronises).
template <int DIMP, class Weight>
__device__ __forceinline__ void contract_tile(const DevProgram *__restrict__ P, const TangentSlots<GRAD_GROUP> &slots,
                                              const FeatView &R, const FeatView &C, const ContractTile &t,
                                              const double *const (&tr)[GRAD_GROUP], const double *const (&tc)[GRAD_GROUP],
                                              Weight wt, long long id, double *partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long il = (long long)t.bi * CT + lane;
  const bool need_norm = (P->metric_mask & ((1 << AGP_METRIC_RADIAL) | (1 << AGP_METRIC_ANGULAR))) != 0;
  const bool have_ids = R.ids != nullptr && C.ids != nullptr, both_meas = R.meas != 0 && C.meas != 0;
  double acc[GRAD_GROUP];
#pragma unroll
  for (int g = 0; g < GRAD_GROUP; ++g) acc[g] = 0.;
  if (il < t.nrl) {
    Point<DIMP> x;
    load_point<DIMP>(R, t.rbase + il, need_norm, x);
    double tx[GRAD_GROUP];
#pragma unroll
    for (int g = 0; g < GRAD_GROUP; ++g) tx[g] = tr[g] ? tr[g][t.rbase + il] : 0.;
    wt.row(il);
    for (int c = wave; c < CT; c += CT_THREADS / 64) {
      const long long jl = (long long)t.bj * CT + c;
      if (jl >= t.ncl || (t.lower && jl > il)) continue;
      Point<DIMP> y;
      load_point<DIMP>(C, t.cbase + jl, need_norm, y);
      double ty[GRAD_GROUP];
#pragma unroll
      for (int g = 0; g < GRAD_GROUP; ++g) ty[g] = tc[g] ? tc[g][t.cbase + jl] : 0.;
      const double w = ((t.lower && il != jl) ? 2. : 1.) * wt(il, jl);
      double dk[GRAD_GROUP];
      eval_pair_tangent<DIMP, GRAD_GROUP>(P, slots, x, y, tx, ty, have_ids, both_meas, dk);
#pragma unroll
      for (int g = 0; g < GRAD_GROUP; ++g) acc[g] += w * dk[g];
    }
  }
  reduce_tile(acc, id, partial);
}

// sum over tiles of partial[tile][g] in a fixed order (256 strided partial sums, then a tree) by a workgroup of 256;
// __syncthreads() before the next call (the shared array is reused)
__device__ __forceinline__ double reduce_partials(const double *__restrict__ partial, long long tiles, int g) {
  double v = 0.;
  for (long long t = threadIdx.x; t < tiles; t += 256) v += partial[t * GRAD_GROUP + g];
  __shared__ double red[256];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

}  // namespace agp
