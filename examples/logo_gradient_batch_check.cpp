// logo_gradient_batch_check.cpp — model.leave_one_group_out_likelihood_gradient_batch on datasets of UNEQUAL sizes through
// the C++ surface (agp_logo_nll_gradient_batch over detail::size_classes), both predict types: one model - a ScalingTerm
// with tangent columns, Matern52, noise and a mean function - on seven datasets whose sizes fall into four size classes,
// every second one with a target variance, grouped by a callable on the feature (a grid of cells, so the groups are ragged
// and differ per dataset), against the per-dataset loop over leave_one_group_out_likelihood_gradient.  Prints "key,value"
// lines: per predict type the largest relative difference of the values, and per parameter the largest absolute difference
// of its gradient over the datasets with its scale, the sum over the datasets of the magnitudes of the loop's gradients of
// that parameter (tests/test_logo_gradient_batch_cpp_gpu.py holds them to 1e-10 and 1e-9 scale).  Exits non-zero when a
// value is not finite or a result is missing.
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
  GaussianProcessRegression<decltype(cov), FirstCoordinateMean> model(cov, FirstCoordinateMean(), "logo_gradient_batch_check");
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
  const auto cell = [](const P3 &x) { return static_cast<int>(x[0] / 2.5) + 4 * static_cast<int>(x[1] / 2.5); };
  const auto joint = model.leave_one_group_out_likelihood_gradient_batch(datasets, cell);
  const auto marginal = model.leave_one_group_out_likelihood_gradient_batch<MarginalDistribution>(datasets, cell);
  if (joint.size() != datasets.size() || marginal.size() != datasets.size()) {
    std::printf("logo_gradient_batch_check FAILED: %zu and %zu results for %zu datasets\n", joint.size(), marginal.size(), datasets.size());
    return 1;
  }
  Worst w_joint, w_marginal;
  for (std::size_t b = 0; b < datasets.size(); ++b) {
    const auto s_joint = model.leave_one_group_out_likelihood_gradient(datasets[b], cell);
    const auto s_marginal = model.leave_one_group_out_likelihood_gradient<MarginalDistribution>(datasets[b], cell);
    w_joint.add(joint[b].value, s_joint.value, joint[b].gradient, s_joint.gradient);
    w_marginal.add(marginal[b].value, s_marginal.value, marginal[b].gradient, s_marginal.gradient);
  }
  std::printf("problems,%zu\n", datasets.size());
  w_joint.print("joint");
  w_marginal.print("marginal");
  const bool finite = w_joint.finite && w_marginal.finite;
  std::printf(finite ? "logo_gradient_batch_check ok\n" : "logo_gradient_batch_check FAILED: a value is not finite or missing\n");
  return finite ? 0 : 1;
}
