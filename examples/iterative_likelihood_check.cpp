// iterative_likelihood_check.cpp — the log-likelihood value of the matrix-free fit through the C++ surface
// (IterativeLikelihoodOptions, IterativeFitModel::log_likelihood and ::log_likelihood_and_gradient) against the dense fit of
// the same model: a squared exponential plus noise and a one-parameter mean on seeded 3-D data.
// Prints "name,value" rows - each difference relative to its bar - and exits non-zero when one exceeds its bar.
//   * a rank-0 fit has P = delta I, so the probes Z = sqrt(n delta) I (t = n) exhaust it and the estimator is exact: value
//     and gradient from ONE call within 1e-8 (n + |dense|) and 1e-7 of the gradient's scale of the dense ones (fit tolerance
//     1e-12; delta = mean_i A_ii = 1.01 here);
//   * seeded probes on a rank-64 fit: the standard errors are the stated functions of the returned samples, two seeds differ
//     by half the difference of their sample means, the value lies within four standard errors of the dense one, two calls
//     give equal bits, one probe gives a NaN standard error, a looser quadrature tolerance shortens the recurrences;
//   * a fit that converged in 0 iterations under max_iterations = 1 raises NotConvergedError from the value.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include <albatross_amd/albatross.hpp>

using namespace albatross;
using P3 = std::array<double, 3>;

struct Slope {  // mu(x) = slope * x_0
  double slope = 0.3;
  std::string get_name() const { return "slope_mean"; }
  ParameterStore get_params() const { return {{"slope", slope}}; }
  bool has_param(const std::string &n) const { return n == "slope"; }
  void set_param(const std::string &n, double v) {
    if (n != "slope") throw std::out_of_range("unknown parameter " + n);
    slope = v;
  }
  double _call_impl(const P3 &x) const { return slope * x[0]; }
};

static double mean_of(const Vector &v) {
  double s = 0.;
  for (double x : v) s += x;
  return s / static_cast<double>(v.size());
}

int main() {
  std::mt19937 gen(5);
  std::uniform_real_distribution<double> u(0., 4.);
  std::normal_distribution<double> noise(0., 0.1);
  const int n = 130;
  std::vector<P3> x(n);
  Vector y(n), on_mean(n);
  for (int i = 0; i < n; ++i) {
    x[i] = {u(gen), u(gen), u(gen)};
    on_mean[i] = 0.3 * x[i][0];
    y[i] = std::sin(x[i][0]) + std::sin(x[i][1]) + std::sin(x[i][2]) + on_mean[i] + noise(gen);
  }
  auto cov = SquaredExponential<EuclideanDistance>(1., 1.) + IndependentNoise<P3>(0.1);
  int failures = 0;
  auto row = [&failures](const std::string &name, double value, double bar) {
    std::printf("%s,%.6g\n", name.c_str(), value);
    if (!(value <= bar)) { std::fprintf(stderr, "MISMATCH: %s = %g exceeds %g\n", name.c_str(), value, bar); ++failures; }
  };

  const GaussianProcessRegression<decltype(cov), Slope> model(cov, Slope(), "iterative_likelihood_check");
  const RegressionDataset<P3> data(x, MarginalDistribution(y));
  const auto dense = model.log_likelihood_gradient(data);
  const double dense_value = model.log_likelihood(data);

  // ---- rank 0: P = delta I, delta the mean of diag(A); sqrt(n delta) I exhausts it ----
  IterativeOptions plain;
  plain.preconditioner_rank = 0;
  plain.tolerance = 1e-12;
  const auto fm0 = model.fit_iterative(data, plain);
  const double delta = 1. * 1. + 0.1 * 0.1;  // every A_ii: sigma^2 of the squared exponential plus the noise variance
  IterativeLikelihoodOptions exhaust;
  exhaust.probes = Matrix(n, n);
  for (int i = 0; i < n; ++i) exhaust.probes(i, i) = std::sqrt(static_cast<double>(n) * delta);
  const IterativeLikelihood exact = fm0.log_likelihood_and_gradient(exhaust);
  row("exhausting_value_over_bar", std::fabs(exact.value - dense_value) / (1e-8 * (n + std::fabs(dense_value))), 1.);
  double worst = 0.;
  for (const auto &kv : dense.gradient) {
    double scale = std::fabs(kv.second);
    const auto smp = exact.gradient.samples.find(kv.first);
    if (smp != exact.gradient.samples.end()) {
      double sum = 0., abs_sum = 0.;
      for (double s : smp->second) { sum += s; abs_sum += std::fabs(s); }
      const double alpha_term = 0.5 * sum / n + exact.gradient.gradient.at(kv.first);  // d log p = -tau / 2 + a / 2
      scale = 0.5 * abs_sum / n + std::fabs(alpha_term);
    }
    worst = std::fmax(worst, std::fabs(exact.gradient.gradient.at(kv.first) - kv.second) / (1e-7 * scale));
  }
  row("exhausting_gradient_over_bar", worst, 1.);
  row("mean_parameter_standard_error", exact.gradient.standard_error.at("slope"), 0.);
  std::printf("probe_iterations,%d\n", exact.iterations[0]);

  // ---- seeded probes on a preconditioned fit ----
  IterativeOptions opt;
  opt.preconditioner_rank = 64;
  opt.tolerance = 1e-12;
  const auto fm = model.fit_iterative(data, opt);
  IterativeLikelihoodOptions seeded;
  seeded.num_probes = 32;
  seeded.seed = 3;
  const IterativeLikelihood est = fm.log_likelihood_and_gradient(seeded), again = fm.log_likelihood_and_gradient(seeded);
  const IterativeLikelihood value_only = fm.log_likelihood(seeded);
  double dev2 = 0.;
  const double mu = mean_of(est.samples);
  for (double s : est.samples) dev2 += (s - mu) * (s - mu);
  const double se = std::sqrt(dev2 / (32. * 31.));
  double fn = std::fabs(est.log_determinant_standard_error - se) / (1e-12 * se);
  fn = std::fmax(fn, std::fabs(est.standard_error - 0.5 * se) / (1e-12 * se));
  IterativeLikelihoodOptions other = seeded;
  other.seed = 4;
  const IterativeLikelihood est2 = fm.log_likelihood(other);
  const double mu2 = mean_of(est2.samples);
  fn = std::fmax(fn, std::fabs((est.value - est2.value) + 0.5 * (mu - mu2)) / (1e-10 * (std::fabs(est.value) + std::fabs(mu) + std::fabs(mu2))));
  fn = std::fmax(fn, std::fabs((est.log_determinant - est2.log_determinant) - (mu - mu2)) /
                         (1e-10 * (std::fabs(est.log_determinant) + std::fabs(mu) + std::fabs(mu2))));
  row("seeded_functions_of_the_samples_over_bar", fn, 1.);
  row("seeded_value_standard_errors_from_dense_over_4", std::fabs(est.value - dense_value) / est.standard_error / 4., 1.);
  double bits = est.value == again.value && est.standard_error == again.standard_error && est.value == value_only.value ? 0. : 1.;
  for (const auto &kv : est.gradient.gradient) bits += kv.second == again.gradient.gradient.at(kv.first) ? 0. : 1.;
  row("second_call_differs", bits, 0.);
  IterativeLikelihoodOptions one;
  one.num_probes = 1;
  row("one_probe_standard_error_is_not_nan", std::isnan(fm.log_likelihood(one).standard_error) ? 0. : 1., 0.);
  IterativeLikelihoodOptions loose = seeded;
  loose.quadrature_tolerance = 1e-4;
  const IterativeLikelihood quick = fm.log_likelihood(loose);
  int longest_quick = 0, shortest_full = 1 << 30;
  for (int k : quick.iterations) longest_quick = std::max(longest_quick, k);
  for (int k : est.iterations) shortest_full = std::min(shortest_full, k);
  row("loose_quadrature_is_not_shorter", longest_quick < shortest_full ? 0. : 1., 0.);
  row("loose_quadrature_moved_the_value_by_standard_errors", std::fabs(quick.value - est.value) / est.standard_error, 1e-3);

  // ---- a fit of targets that sit on the mean converges in 0 iterations; one iteration is not enough for a probe ----
  IterativeOptions single_iteration;
  single_iteration.preconditioner_rank = 0;
  single_iteration.max_iterations = 1;
  const auto flat = model.fit_iterative(RegressionDataset<P3>(x, MarginalDistribution(on_mean)), single_iteration);
  row("zero_fit_iterations", flat.get_fit().iterations, 0.);
  bool threw = false;
  try { flat.log_likelihood(seeded); } catch (const NotConvergedError &e) { threw = e.iterations == 1 && e.residual > single_iteration.tolerance; }
  row("one_iteration_did_not_raise", threw ? 0. : 1., 0.);

  if (failures) return EXIT_FAILURE;
  std::printf("iterative_likelihood_check ok\n");
  return EXIT_SUCCESS;
}
