// loo_gradient_batch_check.cpp — GaussianProcessRegression::leave_one_out_likelihood_gradients and
// leave_one_out_likelihoods (agp_loo_nll_gradient_batch) through the C++ surface: the model and data of
// loo_gradient_check.cpp, a target variance per point, under the four parameter sets of gradient_batch_check.cpp.
// Prints "key,value" lines (the data with the variances, then per set b "loo_nll,b,value", "loo_nll_value_only,b,value"
// and one "grad_<name>,b,value" row per parameter) that tests/test_loo_gradient_batch_gpu.py compares with the Python
// surface.
#include <array>
#include <cmath>
#include <cstdio>
#include <random>

#include <albatross_amd/albatross.hpp>

using namespace albatross;
using P3 = std::array<double, 3>;

struct Elevation {  // the ScalingFunction of gradient_check
  double center = 4.0, factor = 0.3;
  std::string get_name() const { return "elevation_scaling"; }
  ParameterStore get_params() const { return {{"elevation_scaling_center", center}, {"elevation_scaling_factor", factor}}; }
  void set_param(const std::string &n, double v) { (n == "elevation_scaling_center" ? center : factor) = v; }
  double _call_impl(const P3 &x) const { return 1. + factor * std::fmax(center - x[2], 0.); }
};

struct FirstCoordinateMean {  // slope * x[0] + offset on 3-D features
  double slope = 0.2, offset = -0.4;
  std::string get_name() const { return "first_coordinate_linear"; }
  ParameterStore get_params() const { return {{"slope", slope}, {"offset", offset}}; }
  bool has_param(const std::string &n) const { return n == "slope" || n == "offset"; }
  void set_param(const std::string &n, double v) { (n == "slope" ? slope : offset) = v; }
  double _call_impl(const P3 &x) const { return slope * x[0] + offset; }
};

int main() {
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> u(0., 10.), w(0.001, 0.02);
  const int n = 500;
  std::vector<P3> x(n);
  Vector y(n), var(n);
  for (int i = 0; i < n; ++i) {
    x[i] = {u(gen), u(gen), u(gen)};
    y[i] = std::sin(x[i][0]) + std::sin(x[i][1]) + std::sin(x[i][2]) + 0.3 * x[i][0];
    var[i] = w(gen);
  }
  auto cov = ScalingTerm<Elevation>() * Constant(0.5) + Matern52<EuclideanDistance>(2.0, 1.0) + IndependentNoise<P3>(0.1);
  GaussianProcessRegression<decltype(cov), FirstCoordinateMean> model(cov, FirstCoordinateMean(), "loo_gradient_batch_check");
  RegressionDataset<P3> data(x, MarginalDistribution(y, var));
  const std::vector<ParameterStore> sets = {
      {},
      {{"elevation_scaling_center", 5.0}},
      {{"sigma_matern_52", 1.3}, {"slope", 0.5}},
      {{"elevation_scaling_factor", 0.5}, {"sigma_independent_noise", 0.2}, {"offset", 0.1}},
  };
  const auto g = model.leave_one_out_likelihood_gradients(data, sets);
  const Vector values = model.leave_one_out_likelihoods(data, sets);
  for (int i = 0; i < n; ++i)
    std::printf("x,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n", i, x[i][0], x[i][1], x[i][2], y[i], var[i]);
  for (std::size_t b = 0; b < g.size(); ++b) {
    std::printf("loo_nll,%zu,%.17g\n", b, g[b].value);
    std::printf("loo_nll_value_only,%zu,%.17g\n", b, values[b]);
    for (const auto &kv : g[b].gradient) std::printf("grad_%s,%zu,%.17g\n", kv.first.c_str(), b, kv.second);
  }
  return 0;
}
