// greedy_inducing_check.cpp — the greedy pivoted Cholesky factorisation and the inducing-point strategy built on it,
// through the C++ surface: albatross::pivoted_cholesky and GreedyVarianceInducingPoints as the InducingPointStrategy of
// sparse_gp_from_covariance, for a PITC model (Matern-3/2 + measurement-only noise) on seeded, clustered 2-D data with
// groups by the first coordinate.  Prints "key,value" lines (the data, the pivots, the rank, the residual trace, the
// inducing points of the fit and a marginal prediction) that tests/test_greedy_inducing_gpu.py compares with the Python
// surface, and exits non-zero when the fit's inducing points are not the features at the pivots.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include <albatross_amd/albatross.hpp>

using namespace albatross;
using P2 = std::array<double, 2>;

int main() {
  std::mt19937 gen(29);
  std::uniform_real_distribution<double> centre(0., 10.), spread(-0.4, 0.4);
  const int n = 360, clusters = 12, m = 40;
  std::vector<P2> x(n);
  Vector y(n);
  std::vector<P2> c(clusters);
  for (auto &p : c) p = {centre(gen), centre(gen)};
  for (int i = 0; i < n; ++i) {
    const P2 &q = c[static_cast<std::size_t>(i % clusters)];
    x[i] = {q[0] + spread(gen), q[1] + spread(gen)};
    y[i] = std::sin(x[i][0]) + std::cos(0.7 * x[i][1]);
  }
  auto cov = Matern32<EuclideanDistance>(2.5, 1.2) + measurement_only(IndependentNoise<P2>(0.1));
  for (int i = 0; i < n; ++i) std::printf("x,%d,%.17g,%.17g,%.17g\n", i, x[i][0], x[i][1], y[i]);

  const PivotedCholesky f = pivoted_cholesky(cov, x, m, 1e-12);
  std::printf("rank,%lld\n", static_cast<long long>(f.rank));
  std::printf("trace_residual,%.17g\n", f.trace_residual);
  for (std::size_t j = 0; j < f.pivots.size(); ++j)
    std::printf("pivot,%zu,%lld,%.17g\n", j, static_cast<long long>(f.pivots[j]), f.factor(f.pivots[j], static_cast<std::int64_t>(j)));

  const auto grouper = [](const P2 &p) { return static_cast<long>(std::floor(p[0] / 2.0)); };
  auto model = sparse_gp_from_covariance(cov, grouper, GreedyVarianceInducingPoints(m), "greedy_inducing_check");
  model.set_param_value(details::inducing_nugget_name(), 1e-8);
  const RegressionDataset<P2> data(x, MarginalDistribution(y));
  const auto fit_model = model.fit(data);
  const auto &u = fit_model.get_fit().train_features;
  int failures = 0;
  if (u.size() != f.pivots.size()) ++failures;
  for (std::size_t j = 0; j < u.size() && j < f.pivots.size(); ++j) {
    std::printf("inducing,%zu,%.17g,%.17g\n", j, u[j][0], u[j][1]);
    if (!(u[j] == x[static_cast<std::size_t>(f.pivots[j])])) ++failures;
  }
  std::vector<P2> xs;
  for (int i = 0; i < 7; ++i) xs.push_back({1.3 * i + 0.5, 9.1 - 1.1 * i});
  const MarginalDistribution p = fit_model.predict(xs).marginal();
  for (std::size_t i = 0; i < xs.size(); ++i)
    std::printf("prediction,%zu,%.17g,%.17g,%.17g,%.17g\n", i, xs[i][0], xs[i][1], p.mean[i], p.covariance[i]);
  if (failures) {
    std::fprintf(stderr, "MISMATCH: the fit's inducing points are not the features at the pivots\n");
    return EXIT_FAILURE;
  }
  std::printf("greedy_inducing_check ok\n");
  return EXIT_SUCCESS;
}
