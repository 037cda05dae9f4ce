// lanczos_quadrature.h — the Gauss quadrature of log from the coefficients of one conjugate-gradient recurrence
// (agp_iterative_nll, iterative.hip).  Plain C++, no HIP: the work is O(k^2) per column with k <= max_iterations, one
// dependent chain of rotations; the entry gives the columns of a chunk a host thread each.
//
// Preconditioned CG on A x = z with preconditioner P is Lanczos on M = P^-1/2 A P^-1/2 started at u = P^-1/2 z.  With a_i,
// b_i the alpha and beta of iteration i (b_0 = 0) the Lanczos tridiagonal of M is
//   T[i, i] = 1 / a_i + b_i / a_{i-1}  (i = 0: the first term alone),    T[i-1, i] = T[i, i-1] = sqrt(b_i) / a_{i-1},
// and u^T log(M) u ~ |u|^2 e_1^T log(T) e_1 = rz0 sum_i V[0, i]^2 log lambda_i with (lambda, V) the eigendecomposition of T
// and rz0 = z^T P^-1 z = |u|^2 (Golub & Meurant, "Matrices, Moments and Quadrature", 1994; Golub & Welsch 1969 for
// carrying the first row of V alone through the implicit QL iteration).  No reorthogonalisation: the quadrature from the
// coefficients of a finite-precision recurrence keeps its accuracy (the ghost eigenvalues share the weight of the one they
// copy).  The entry runs the iteration in long double: the weights of a tridiagonal with clustered eigenvalues then carry
// no error a double could show (lanczos_quadrature_as<double> is there for the host check of examples/ to compare with).
#pragma once
#include <cmath>
#include <limits>
#include <vector>
#include "../../include/albatross_amd.h"

namespace agp {

// *out = rz0 e_1^T log(T) e_1 for the k x k tridiagonal of a[i * stride], b[i * stride], i < k (b[0] is not read).
// k == 0: 0.  AGP_ERR_NOT_POSITIVE_DEFINITE: a coefficient that no positive definite M produces (a_i <= 0, b_i < 0, not
// finite), an eigenvalue of T <= 0, or a QL sweep count no symmetric tridiagonal needs; *out is then not written.
template <typename real>
int lanczos_quadrature_as(double rz0, const double *a, const double *b, long long stride, int k, double *out) {
  if (k < 0 || !out || (k > 0 && (!a || !b))) return AGP_ERR_INVALID_ARGUMENT;
  if (k == 0) { *out = 0.; return AGP_OK; }
  if (!(rz0 > 0.) || !std::isfinite(rz0)) return AGP_ERR_NOT_POSITIVE_DEFINITE;
  std::vector<real> d((size_t)k), e((size_t)k, real(0)), z((size_t)k, real(0));
  for (int i = 0; i < k; ++i) {
    const double ai = a[i * stride], bi = i > 0 ? b[i * stride] : 0.;
    if (!(ai > 0.) || !std::isfinite(ai) || !(bi >= 0.) || !std::isfinite(bi)) return AGP_ERR_NOT_POSITIVE_DEFINITE;
    d[i] = real(1) / (real)ai;
    if (i > 0) {
      const real ap = (real)a[(i - 1) * stride];
      d[i] += (real)bi / ap;
      e[i - 1] = std::sqrt((real)bi) / ap;  // e[i]: the entry between rows i and i + 1
    }
  }
  z[0] = real(1);
  const real eps = std::numeric_limits<real>::epsilon();
  for (int l = 0; l < k; ++l) {
    for (int sweeps = 0;; ++sweeps) {
      int m = l;
      for (; m < k - 1; ++m)
        if (std::fabs(e[m]) <= eps * (std::fabs(d[m]) + std::fabs(d[m + 1]))) break;
      if (m == l) break;
      if (sweeps == 80) return AGP_ERR_NOT_POSITIVE_DEFINITE;
      real g = (d[l + 1] - d[l]) / (real(2) * e[l]);
      real r = std::sqrt(g * g + real(1));
      g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
      real s = real(1), c = real(1), p = real(0);
      int i = m - 1;
      for (; i >= l; --i) {
        real f = s * e[i];
        const real h = c * e[i];
        r = std::sqrt(f * f + g * g);
        e[i + 1] = r;
        if (r == real(0)) {  // (an underflow of the rotation: deflate and start the sweep again)
          d[i + 1] -= p;
          e[m] = real(0);
          break;
        }
        s = f / r;
        c = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * s + real(2) * c * h;
        p = s * r;
        d[i + 1] = g + p;
        g = c * r - h;
        f = z[i + 1];  // the first row of the eigenvectors
        z[i + 1] = s * z[i] + c * f;
        z[i] = c * z[i] - s * f;
      }
      if (r == real(0) && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[m] = real(0);
    }
  }
  real sum = real(0);
  for (int i = 0; i < k; ++i) {
    if (!(d[i] > real(0))) return AGP_ERR_NOT_POSITIVE_DEFINITE;
    sum += z[i] * z[i] * std::log(d[i]);
  }
  *out = (double)((real)rz0 * sum);
  return AGP_OK;
}

inline int lanczos_quadrature(double rz0, const double *a, const double *b, long long stride, int k, double *out) {
  return lanczos_quadrature_as<long double>(rz0, a, b, stride, k, out);
}

}  // namespace agp
