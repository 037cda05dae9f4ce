// gram_fast.h — the radial fast path of the covariance kernels (gram.hip) as device code other translation units can
// instantiate: the tile body of the Gram kernels and the per-pair arithmetic of the radial<Euclidean> [+ noise] trees.
// predict_batch.hip builds its table-driven launches from the same body, so a cross covariance has the same bits
// whether it is made by launch_gram or by a launch for many problems.  Translation units that include this header
// are compiled without FMA contraction, like gram.hip (csrc/Makefile).
#pragma once
#include "common.h"

namespace agp {

constexpr int TM = 128;  // tile rows
constexpr int TN = 32;   // tile cols
constexpr int GRAM_THREADS = 256;

// ---------------------------------------------------------------------------
// Fast path for the commonest trees:  radial<Euclidean>  and
// radial<Euclidean> + [measurement_only](IndependentNoise | Nugget).
// Same tile shape and the same IEEE operation sequence per pair as the generic
// evaluator (distance -> q -> exp), but the tree is fixed at compile time: no
// program walk, no evaluation stack.  ~2.5x fewer VALU instructions per pair.
// ---------------------------------------------------------------------------
struct FastParams {
  double length_scale, sigma;
  double noise_var;   // sigma_noise^2 (0 when there is no noise term)
  int has_noise;      // tree is radial + noise
  int noise_meas_only;  // the noise term is wrapped in MeasurementOnly
  // host-side precomputation (match_fast): the pair loop multiplies instead of dividing
  double sigma2;      // sigma^2
  double inv_l2;      // SquaredExponential: 1 / l^2      (exp(-(d/l)^2) = exp(-d^2 / l^2): no sqrt, no divide per pair)
  double cq;          // Exponential: 1 / l, Matern-3/2: sqrt(3) / l, Matern-5/2: sqrt(5) / l
};

// k(x, y) from the SQUARED Euclidean distance s2 (radial.hpp:25-33,191-198,289-297,461-470).  Differs from the
// reference's operation sequence (sqrt, divide by l, square) by a few ulp of the exponent argument; the parity bar of
// tests/test_gram_gpu.py (4e-16 max|K| + 2e-14 |value|) holds with a margin of 10x.
template <int OP>
__device__ __forceinline__ double radial_fast(double s2, const FastParams &fp) {
  if (fp.length_scale <= 0.) return 0.;
  if (OP == AGP_OP_SQUARED_EXPONENTIAL) {
    return fp.sigma2 * exp_neg(s2 * fp.inv_l2);
  } else if (OP == AGP_OP_EXPONENTIAL) {
    return fp.sigma2 * exp_neg(sqrt(s2) * fp.cq);
  } else if (OP == AGP_OP_MATERN32) {
    const double q = sqrt(s2) * fp.cq;
    return fp.sigma2 * (1 + q) * exp_neg(q);
  } else {
    const double q = sqrt(s2) * fp.cq;
    return fp.sigma2 * (1 + q + q * q * (1. / 3.)) * exp_neg(q);
  }
}

// NT values at once, without the test of the length scale's sign (radial.hpp: 0 if l <= 0; the caller handles it) and
// with the exponentials in lock step (cov_eval.h: exp_neg_n).  Per value the operations of radial_fast.
template <int OP, int NT>
__device__ __forceinline__ void radial_fast_n(const double (&s2)[NT], const FastParams &fp, double (&v)[NT]) {
  double arg[NT], pre[NT], e[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (OP == AGP_OP_SQUARED_EXPONENTIAL) {
      arg[i] = s2[i] * fp.inv_l2;
      pre[i] = fp.sigma2;
    } else if (OP == AGP_OP_EXPONENTIAL) {
      arg[i] = sqrt(s2[i]) * fp.cq;
      pre[i] = fp.sigma2;
    } else if (OP == AGP_OP_MATERN32) {
      const double q = sqrt(s2[i]) * fp.cq;
      arg[i] = q;
      pre[i] = fp.sigma2 * (1 + q);
    } else {
      const double q = sqrt(s2[i]) * fp.cq;
      arg[i] = q;
      pre[i] = fp.sigma2 * (1 + q + q * q * (1. / 3.));
    }
  }
  exp_neg_n<NT>(arg, e);
#pragma unroll
  for (int i = 0; i < NT; ++i) v[i] = pre[i] * e[i];
}

template <int DIMP, int OP>
__device__ __forceinline__ void gram_fast_body(const FastParams &fp, FeatView X, FeatView Y, int lower_only, double *out, long long ld,
                                               const double *diag_add, int *nan_flag, long long blk_rows, long long blk_stride,
                                               long long tile_r = -1, long long tile_c = -1) {
  __shared__ double xs[DIMP][TM], ys[DIMP][TN];
  __shared__ long long xid[TM], yid[TN];
  if (blk_rows > 0) {  // blockIdx.z = one diagonal block of a block-diagonal Gram matrix (launch_gram_blocks)
    const long long z = blockIdx.z;
    X.coords += z * blk_rows * X.dim; Y.coords += z * blk_rows * Y.dim;
    if (X.ids) X.ids += z * blk_rows;
    if (Y.ids) Y.ids += z * blk_rows;
    X.n = Y.n = blk_rows;
    out += z * blk_stride;
    if (diag_add) diag_add += z * blk_rows;
  }
  const long long row0 = (tile_r >= 0 ? tile_r : (long long)blockIdx.x) * TM;
  const long long col0 = (tile_c >= 0 ? tile_c : (long long)blockIdx.y) * TN;
  if (lower_only && col0 > row0 + TM - 1) return;
  const bool have_ids = X.ids != nullptr && Y.ids != nullptr;
  for (int t = threadIdx.x; t < TM + TN; t += GRAM_THREADS) {
    const bool isx = t < TM;
    const FeatView &F = isx ? X : Y;
    const long long g = isx ? row0 + t : col0 + (t - TM);
    const bool ok = g < F.n;
#pragma unroll
    for (int d = 0; d < DIMP; ++d) {
      const double v = (ok && d < F.dim) ? F.coords[g * F.dim + d] : 0.;
      if (isx) xs[d][t] = v; else ys[d][t - TM] = v;
    }
    const long long id = (ok && F.ids) ? F.ids[g] : -1;
    if (isx) xid[t] = id; else yid[t - TM] = id;
  }
  __syncthreads();
  const int lane_row = 2 * (threadIdx.x & 63);
  const int cgrp = threadIdx.x >> 6;
  double xa[DIMP], xb[DIMP];
#pragma unroll
  for (int d = 0; d < DIMP; ++d) { xa[d] = xs[d][lane_row]; xb[d] = xs[d][lane_row + 1]; }
  const long long ida = xid[lane_row], idb = xid[lane_row + 1];
  const long long ra = row0 + lane_row, rb = ra + 1;
  const bool wide = ((ld & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const bool noise_on = fp.has_noise && (!fp.noise_meas_only || (X.meas && Y.meas));
  bool saw_nan = false;
  const bool dead = fp.length_scale <= 0.;  // radial.hpp: the covariance is 0 for a non-positive length scale (wave-uniform)
  // Two columns (four entries) per trip: their exponentials run in lock step (cov_eval.h: exp_neg_n) - round 5's loop made
  // two separate calls per trip, which the compiler left one behind the other -, and the noise term's equality test
  // (noise.hpp:37-43) runs only in a wave that holds an equal pair: equal coordinates give a squared distance of exactly 0.
  // Same operations per entry as before: bit-identical matrices.
  for (int jj = 0; jj < TN / 4; jj += 2) {
    const int cslot = cgrp * (TN / 4) + jj;
    const long long col = col0 + cslot;
    if (col >= Y.n) break;
    const bool two = col + 1 < Y.n;  // (TN / 4 is even: the second column is this wave group's too)
    double s2[4] = {0., 0., 0., 0.};  // (row a, col 0), (row b, col 0), (row a, col 1), (row b, col 1)
    double yv[2][DIMP];
#pragma unroll
    for (int d = 0; d < DIMP; ++d) {
      yv[0][d] = ys[d][cslot];
      yv[1][d] = ys[d][cslot + 1];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int d = 0; d < DIMP; ++d) {
        const double ta = xa[d] - yv[c][d], tb = xb[d] - yv[c][d];
        s2[2 * c] += ta * ta;
        s2[2 * c + 1] += tb * tb;
      }
    double v[4];
    if (dead) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = 0.;
    } else {
      radial_fast_n<OP, 4>(s2, fp, v);
    }
    if (fp.has_noise) {  // lhs + rhs with rhs = noise (0 when not measurements / not equal)
      bool e[4] = {false, false, false, false};
      bool maybe = false;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const long long yi = yid[cslot + c];
        maybe = maybe || (have_ids ? (ida == yi || idb == yi) : (s2[2 * c] == 0. || s2[2 * c + 1] == 0.));
      }
      if (noise_on && __any(maybe)) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          bool ea = true, eb = true;
#pragma unroll
          for (int d = 0; d < DIMP; ++d) {
            ea = ea && (xa[d] == yv[c][d]);
            eb = eb && (xb[d] == yv[c][d]);
          }
          if (have_ids) {
            ea = ida == yid[cslot + c];
            eb = idb == yid[cslot + c];
          }
          e[2 * c] = ea;
          e[2 * c + 1] = eb;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = v[q] + (e[q] ? fp.noise_var : 0.);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (c == 1 && !two) break;
      const long long cc = col + c;
      double va = v[2 * c], vb = v[2 * c + 1];
      if (diag_add) {
        if (ra == cc) va += diag_add[cc];
        if (rb == cc) vb += diag_add[cc];
      }
      // only entries that are stored count (padding rows of an edge tile are zero
      // vectors: the angular metric makes NaN out of them)
      saw_nan = saw_nan || (ra < X.n && va != va) || (rb < X.n && vb != vb);
      double *dst = out + cc * ld + ra;
      if (rb < X.n) {
        if (wide) *reinterpret_cast<double2 *>(dst) = make_double2(va, vb);  // (non-temporal stores measured in round 6: no difference)
        else { dst[0] = va; dst[1] = vb; }
      } else if (ra < X.n) {
        dst[0] = va;
      }
    }
  }
  if (saw_nan && nan_flag) atomicOr(nan_flag, 1);
}

// Does the program have one of the fast-path shapes (and is the fast path switched on: AGP_GRAM_SOP)?  gram.hip
bool gram_match_fast(const DevProgram &H, FastParams *fp, int *op);

}  // namespace agp
