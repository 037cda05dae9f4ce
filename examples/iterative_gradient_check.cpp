// iterative_gradient_check.cpp — the probe gradient of the matrix-free fit through the C++ surface
// (albatross::gram_tangent_forms, IterativeGradientOptions, IterativeFitModel::log_likelihood_gradient) against the exact
// gradient of the dense fit of the same model: a squared exponential plus noise and a one-parameter mean on seeded 3-D data.
// Prints "name,value" rows - each difference relative to its bar - and exits non-zero when one exceeds its bar.
//   * identity probes Z = sqrt(n) I make the estimator exact: every parameter within 1e-7 of the scale of its own terms,
//     1/2 mean_c |s_cp| + 1/2 |alpha^T dA_p alpha|, of the dense gradient (fit tolerance 1e-12);
//   * seeded probes: the gradient and the standard error are the stated functions of the returned samples, one probe gives a
//     NaN standard error, the mean parameter is exact with standard error 0;
//   * gram_tangent_forms against central differences of the stored matrix;
//   * a fit that converged in 0 iterations under max_iterations = 1 raises NotConvergedError from the gradient.
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

  const GaussianProcessRegression<decltype(cov), Slope> model(cov, Slope(), "iterative_gradient_check");
  const RegressionDataset<P3> data(x, MarginalDistribution(y));
  const auto dense = model.log_likelihood_gradient(data);
  IterativeOptions opt;
  opt.preconditioner_rank = 64;
  opt.tolerance = 1e-12;
  const auto fm = model.fit_iterative(data, opt);

  // ---- identity probes: exact ----
  IterativeGradientOptions identity;
  identity.probes = Matrix(n, n);
  for (int i = 0; i < n; ++i) identity.probes(i, i) = std::sqrt(static_cast<double>(n));
  const IterativeGradient exact = fm.log_likelihood_gradient(identity);
  double worst = 0.;
  for (const auto &kv : dense.gradient) {
    double scale = std::fabs(kv.second);
    const auto smp = exact.samples.find(kv.first);
    if (smp != exact.samples.end()) {
      double sum = 0., abs_sum = 0.;
      for (double s : smp->second) { sum += s; abs_sum += std::fabs(s); }
      const double alpha_term = 0.5 * sum / n + exact.gradient.at(kv.first);  // d log p = -tau / 2 + a / 2
      scale = 0.5 * abs_sum / n + std::fabs(alpha_term);
    }
    worst = std::fmax(worst, std::fabs(exact.gradient.at(kv.first) - kv.second) / (1e-7 * scale));
  }
  row("identity_gradient_over_bar", worst, 1.);
  row("mean_parameter_standard_error", exact.standard_error.at("slope"), 0.);
  std::printf("probe_iterations,%d\n", exact.iterations[0]);

  // ---- seeded probes: the stated functions of the samples ----
  IterativeGradientOptions seeded;
  seeded.num_probes = 17;
  seeded.seed = 3;
  const IterativeGradient est = fm.log_likelihood_gradient(seeded), again = fm.log_likelihood_gradient(seeded);
  double fn = 0., bits = 0.;
  for (const auto &kv : est.samples) {
    double sum = 0., dev2 = 0.;
    for (double s : kv.second) sum += s;
    const double tau = sum / 17.;
    for (double s : kv.second) dev2 += (s - tau) * (s - tau);
    const double se = 0.5 * std::sqrt(dev2 / (17. * 16.));
    fn = std::fmax(fn, std::fabs(est.standard_error.at(kv.first) - se) / (1e-12 * se));
    // the alpha term is the exact call's: gradient = -tau / 2 + a / 2
    double esum = 0.;
    for (double s : exact.samples.at(kv.first)) esum += s;
    const double a_half = exact.gradient.at(kv.first) + 0.5 * esum / n;
    fn = std::fmax(fn, std::fabs(est.gradient.at(kv.first) - (a_half - 0.5 * tau)) / (1e-10 * (std::fabs(a_half) + std::fabs(0.5 * tau))));
    bits += est.gradient.at(kv.first) == again.gradient.at(kv.first) ? 0. : 1.;
  }
  row("seeded_functions_of_the_samples_over_bar", fn, 1.);
  row("second_call_differs", bits, 0.);
  IterativeGradientOptions one;
  one.num_probes = 1;
  const IterativeGradient single = fm.log_likelihood_gradient(one);
  row("one_probe_standard_error_is_not_nan", std::isnan(single.standard_error.at("sigma_independent_noise")) ? 0. : 1., 0.);

  // ---- gram_tangent_forms against central differences of the stored matrix ----
  const int cols = 5;
  Matrix U(n, cols), V(n, cols);
  std::normal_distribution<double> g01(0., 1.);
  for (int c = 0; c < cols; ++c)
    for (int i = 0; i < n; ++i) { U(i, c) = g01(gen); V(i, c) = g01(gen); }
  const auto forms = gram_tangent_forms(cov, x, U, V);
  double fd = 0.;
  for (const auto &kv : cov.get_params()) {
    const double h = 1e-6;
    auto up = cov, down = cov;
    up.set_param(kv.first, kv.second + h);
    down.set_param(kv.first, kv.second - h);
    const Matrix Ku = up(x), Kd = down(x);
    for (int c = 0; c < cols; ++c) {
      double want = 0., scale = 0.;
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          const double d = (Ku(i, j) - Kd(i, j)) / (2. * h);
          want += U(i, c) * d * V(j, c);
          scale += std::fabs(U(i, c) * d * V(j, c));
        }
      fd = std::fmax(fd, std::fabs(forms.at(kv.first)[c] - want) / (1e-6 * scale + 1e-9));
    }
  }
  row("forms_against_central_differences_over_bar", fd, 1.);

  // ---- a fit of targets that sit on the mean converges in 0 iterations; one iteration is not enough for a probe ----
  IterativeOptions single_iteration;
  single_iteration.preconditioner_rank = 0;
  single_iteration.max_iterations = 1;
  const auto flat = model.fit_iterative(RegressionDataset<P3>(x, MarginalDistribution(on_mean)), single_iteration);
  row("zero_fit_iterations", flat.get_fit().iterations, 0.);
  bool threw = false;
  try { flat.log_likelihood_gradient(seeded); } catch (const NotConvergedError &e) { threw = e.iterations == 1 && e.residual > single_iteration.tolerance; }
  row("one_iteration_did_not_raise", threw ? 0. : 1., 0.);

  if (failures) return EXIT_FAILURE;
  std::printf("iterative_gradient_check ok\n");
  return EXIT_SUCCESS;
}
