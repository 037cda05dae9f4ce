// iterative_fit_check.cpp — the matrix-free fit through the C++ surface (albatross::gram_matvec, IterativeOptions,
// model.fit_iterative) against the dense fit of the same model and the stored matrix: a squared exponential plus
// measurement-only noise and a linear mean on seeded 2-D data with target variances.  Prints "name,value" rows - the
// largest differences, each relative to its bar of 1e-8, the iteration count and the preconditioner's rank - and exits
// non-zero when a difference exceeds its bar, when joint() does not throw, or when three iterations do not raise
// NotConvergedError.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include <albatross_amd/albatross.hpp>

using namespace albatross;
using P2 = std::array<double, 2>;

struct Tilt {  // a mean function of the first coordinate
  std::string get_name() const { return "tilt"; }
  ParameterStore get_params() const { return {}; }
  bool has_param(const std::string &) const { return false; }
  void set_param(const std::string &n, double) { throw std::out_of_range("unknown parameter " + n); }
  double _call_impl(const P2 &x) const { return 0.3 * x[0] - 1.; }
};

static double max_abs(const Vector &v) {
  double m = 0.;
  for (double a : v) m = std::fmax(m, std::fabs(a));
  return m;
}

int main() {
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> u(0., 10.), var(0.02, 0.2);
  const int n = 700, m = 23, cols = 17;
  std::vector<P2> x(n), xs(m);
  Vector y(n), v(n);
  for (int i = 0; i < n; ++i) {
    x[i] = {u(gen), u(gen)};
    y[i] = std::sin(x[i][0]) + std::cos(0.7 * x[i][1]) + 0.3 * x[i][0] - 1.;
    v[i] = var(gen);
  }
  for (auto &p : xs) p = {u(gen), u(gen)};
  auto cov = SquaredExponential<EuclideanDistance>(1.5, 1.) + measurement_only(IndependentNoise<P2>(0.05));
  int failures = 0;
  auto row = [&failures](const char *name, double value, double bar) {
    std::printf("%s,%.6g\n", name, value);
    if (!(value <= bar)) { std::fprintf(stderr, "MISMATCH: %s = %g exceeds %g\n", name, value, bar); ++failures; }
  };

  // gram_matvec against the stored matrix: columns of the identity give the columns of cov(x) + diag(v), bit for bit
  Matrix K = cov(x);
  for (int i = 0; i < n; ++i) K(i, i) += v[i];
  Matrix E(n, cols);
  for (int c = 0; c < cols; ++c) E(n - cols + c, c) = 1.;
  const Matrix KE = gram_matvec(cov, x, E, v);
  double unequal = 0.;
  for (int c = 0; c < cols; ++c)
    for (int i = 0; i < n; ++i) unequal += KE(i, c) == K(i, n - cols + c) ? 0. : 1.;
  row("matvec_entries_that_differ", unequal, 0.);

  const GaussianProcessRegression<decltype(cov), Tilt> model(cov, Tilt(), "iterative_fit_check");
  const RegressionDataset<P2> data(x, MarginalDistribution(y, v));
  const auto dense = model.fit(data);
  IterativeOptions opt;
  opt.preconditioner_rank = 64;
  const auto fm = model.fit_iterative(data, opt);
  std::printf("iterations,%d\n", fm.get_fit().iterations);
  std::printf("preconditioner_rank,%lld\n", static_cast<long long>(fm.get_fit().preconditioner_rank));
  row("residual_over_tolerance", fm.get_fit().residual / opt.tolerance, 1.);
  const Vector &a = fm.get_fit().information, &b = dense.get_fit().information;
  double d = 0.;
  for (int i = 0; i < n; ++i) d = std::fmax(d, std::fabs(a[i] - b[i]));
  row("information_over_bar", d / (1e-8 * max_abs(b)), 1.);

  const MarginalDistribution pi = fm.predict(xs).marginal(), pd = dense.predict(xs).marginal();
  double dm = 0., dv = 0.;
  for (int j = 0; j < m; ++j) {
    dm = std::fmax(dm, std::fabs(pi.mean[j] - pd.mean[j]));
    dv = std::fmax(dv, std::fabs(pi.covariance[j] - pd.covariance[j]));
  }
  row("mean_over_bar", dm / (1e-8 * max_abs(pd.mean)), 1.);
  row("variance_over_bar", dv / 1e-8, 1.);
  const Vector mean_only = fm.predict(xs).mean();
  double dmm = 0.;
  for (int j = 0; j < m; ++j) dmm = std::fmax(dmm, std::fabs(mean_only[j] - pi.mean[j]));
  row("mean_against_marginal_mean", dmm, 0.);

  // solve: the targets less the mean give the information vector again; a zero column gives zeros
  const Tilt tilt;
  Matrix B(n, 3);
  for (int i = 0; i < n; ++i) { B(i, 0) = y[i] - tilt._call_impl(x[i]); B(i, 2) = std::cos(0.1 * i); }  // (column 1 stays zero)
  const Matrix X = fm.get_fit().solve(B);
  double dz = 0., ds = 0.;
  for (int i = 0; i < n; ++i) {
    dz = std::fmax(dz, std::fabs(X(i, 1)));
    ds = std::fmax(ds, std::fabs(X(i, 0) - b[i]));
  }
  row("zero_column", dz, 0.);
  row("solve_over_bar", ds / (1e-8 * max_abs(b)), 1.);

  bool threw = false;
  try { fm.predict(xs).joint(); } catch (const std::logic_error &) { threw = true; }
  row("joint_did_not_throw", threw ? 0. : 1., 0.);
  threw = false;
  IterativeOptions three;
  three.preconditioner_rank = 0;
  three.max_iterations = 3;
  try { model.fit_iterative(data, three); } catch (const NotConvergedError &e) { threw = e.iterations == 3 && e.residual > three.tolerance; }
  row("three_iterations_did_not_raise", threw ? 0. : 1., 0.);

  if (failures) return EXIT_FAILURE;
  std::printf("iterative_fit_check ok\n");
  return EXIT_SUCCESS;
}
