// ragged_gradient_check.cpp — model.log_likelihood_gradient_batch and model.leave_one_out_likelihood_gradient_batch on
// datasets of UNEQUAL sizes through the C++ surface (agp_nll_gradient_batch_ragged, agp_loo_nll_gradient_batch_ragged over
// detail::size_classes): one model - a ScalingTerm with tangent columns, Matern52, noise and a mean function - on seven
// datasets whose sizes fall into four size classes, every second one with a target variance, against the per-dataset loop
// over log_likelihood_gradient / leave_one_out_likelihood_gradient.  Prints "key,value" lines: per metric the largest
// relative difference of the values, and per parameter the largest absolute difference of its gradient over the datasets
// with its scale, the sum over the datasets of the magnitudes of the loop's gradients of that parameter
// (tests/test_ragged_gradient_batch_cpp_gpu.py holds them to 1e-10 and 1e-9 scale).  Exits non-zero when a value is not
// finite or a result is missing.
#include <array>
#include <cmath>
#include <cstdio>
#include <map>
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

struct Worst {
  double value_rel = 0.;
  std::map<std::string, double> diff, scale;
  bool finite = true;
  void add(double got, double want, const ParameterStore &g_got, const ParameterStore &g_want) {
    value_rel = std::fmax(value_rel, std::fabs(got - want) / std::fabs(want));
    finite = finite && std::isfinite(got) && std::isfinite(want) && g_got.size() == g_want.size();
    for (const auto &kv : g_want) {
      const auto it = g_got.find(kv.first);
      if (it == g_got.end() || !std::isfinite(it->second) || !std::isfinite(kv.second)) {
        finite = false;
        continue;
      }
      diff[kv.first] = std::fmax(diff[kv.first], std::fabs(it->second - kv.second));
      scale[kv.first] += std::fabs(kv.second);
    }
  }
  void print(const char *metric) const {
    std::printf("%s_value_rel,%.17g\n", metric, value_rel);
    for (const auto &kv : diff) std::printf("%s_diff_%s,%.17g\n%s_scale_%s,%.17g\n", metric, kv.first.c_str(), kv.second, metric, kv.first.c_str(), scale.at(kv.first));
  }
};

int main() {
  std::mt19937 gen(23);
  std::uniform_real_distribution<double> u(0., 10.), w(0.001, 0.02);
  const std::vector<int> sizes = {300, 60, 129, 700, 256, 128, 250};  // the classes {60, 128} {129, 256, 250} {300} {700}
  auto cov = ScalingTerm<Elevation>() * Constant(0.5) + Matern52<EuclideanDistance>(2.0, 1.0) + IndependentNoise<P3>(0.1);
  GaussianProcessRegression<decltype(cov), FirstCoordinateMean> model(cov, FirstCoordinateMean(), "ragged_gradient_check");
  std::vector<RegressionDataset<P3>> datasets;
  for (std::size_t b = 0; b < sizes.size(); ++b) {
    const int n = sizes[b];
    std::vector<P3> x(n);
    Vector y(n), var(n);
    for (int i = 0; i < n; ++i) {
      x[i] = {u(gen), u(gen), u(gen)};
      y[i] = std::sin(x[i][0]) + std::sin(x[i][1]) + std::sin(x[i][2]) + 0.3 * x[i][0] + 0.05 * (double)b;
      var[i] = w(gen);
    }
    if (b % 2) datasets.push_back(RegressionDataset<P3>(x, MarginalDistribution(y, var)));
    else datasets.push_back(RegressionDataset<P3>(x, y));
  }
  const auto ll = model.log_likelihood_gradient_batch(datasets);
  const auto loo = model.leave_one_out_likelihood_gradient_batch(datasets);
  if (ll.size() != datasets.size() || loo.size() != datasets.size()) {
    std::printf("ragged_gradient_check FAILED: %zu and %zu results for %zu datasets\n", ll.size(), loo.size(), datasets.size());
    return 1;
  }
  Worst w_ll, w_loo;
  for (std::size_t b = 0; b < datasets.size(); ++b) {
    const auto s_ll = model.log_likelihood_gradient(datasets[b]);
    const auto s_loo = model.leave_one_out_likelihood_gradient(datasets[b]);
    w_ll.add(ll[b].log_likelihood, s_ll.log_likelihood, ll[b].gradient, s_ll.gradient);
    w_loo.add(loo[b].value, s_loo.value, loo[b].gradient, s_loo.gradient);
  }
  std::printf("problems,%zu\n", datasets.size());
  w_ll.print("log_likelihood");
  w_loo.print("leave_one_out");
  const bool finite = w_ll.finite && w_loo.finite;
  std::printf(finite ? "ragged_gradient_check ok\n" : "ragged_gradient_check FAILED: a value is not finite or missing\n");
  return finite ? 0 : 1;
}
