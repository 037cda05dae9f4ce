// chi_squared.h — the chi-squared cumulative distribution (stats/chi_squared.hpp:29-67) as ONE function for the host and
// the device: the C++ binding (albatross.hpp: chi_squared_cdf) and the RANSAC scoring kernel (csrc/ransac.hip) include
// this file, so an inlier metric computed on the device and a candidate or consensus check computed on the host run the
// same series and the same continued fraction.  Plain C++ under a host compiler; under hipcc the functions are
// __host__ __device__.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define AGP_HOST_DEVICE __host__ __device__
#else
#define AGP_HOST_DEVICE
#endif

namespace albatross_amd_stats {

// the regularised lower incomplete gamma P(a, x), a > 0 (the role of stats/incomplete_gamma.hpp:134): the series below
// a + 1, Lentz's continued fraction of Q above
AGP_HOST_DEVICE inline double regularized_lower_gamma(double a, double x) {
  if (x <= 0.) return 0.;
  const double log_front = a * log(x) - x - lgamma(a);
  if (x < a + 1.) {
    double term = 1. / a, total = term, n = a;
    for (int i = 0; i < 10000; ++i) {
      n += 1.;
      term *= x / n;
      total += term;
      if (fabs(term) < fabs(total) * 1e-17) break;
    }
    const double v = total * exp(log_front);
    return v < 1. ? v : 1.;
  }
  const double tiny = 1e-300;
  double b = x + 1. - a, c = 1. / tiny, d = 1. / b, h = d;
  for (int i = 1; i < 10000; ++i) {
    const double an = -static_cast<double>(i) * (static_cast<double>(i) - a);
    b += 2.;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1. / d;
    const double delta = d * c;
    h *= delta;
    if (fabs(delta - 1.) < 1e-16) break;
  }
  const double v = 1. - exp(log_front) * h;
  return v > 0. ? v : 0.;
}

// chi_squared_cdf(x, dof), stats/chi_squared.hpp:29-67
AGP_HOST_DEVICE inline double chi_squared_cdf(double x, double degrees_of_freedom) {
  if (x != x || x < 0.) return nan("");
  if (degrees_of_freedom == 0) return 1.;
  if (2.220446049250313e-16 > x) return 0.;
  if (x > 1.7976931348623157e308) return 1.;
  return regularized_lower_gamma(0.5 * degrees_of_freedom, 0.5 * x);
}

}  // namespace albatross_amd_stats
