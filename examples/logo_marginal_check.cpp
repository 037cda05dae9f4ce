// logo_marginal_check.cpp — the MARGINAL predict type of the leave-one-group-out metric through the C++ surface:
// GaussianProcessRegression::leave_one_group_out_likelihood_gradient<MarginalDistribution> and
// LeaveOneGroupOutLikelihood<FeatureType, MarginalDistribution> with its per-group scores, on the model, data and
// stations of logo_gradient_check.  LeaveOneOutLikelihood<MarginalDistribution> is instantiated too (the same number as
// the Joint one).  Prints "key,value" lines (the data with the variances, the metric from both surfaces, one grad_<name>
// row per parameter, one group_<key> row per station) that tests/test_logo_marginal_gpu.py compares with the Python
// surface.
#include <array>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>

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

std::string station(const P3 &x) { return std::to_string(static_cast<int>(x[0])); }

int main() {
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> u(0., 10.), w(0.001, 0.02);
  const int n = 300;
  std::vector<P3> x(n);
  Vector y(n), var(n);
  for (int i = 0; i < n; ++i) {
    x[i] = {u(gen), u(gen), u(gen)};
    y[i] = std::sin(x[i][0]) + std::sin(x[i][1]) + std::sin(x[i][2]) + 0.3 * x[i][0];
    var[i] = w(gen);
  }
  auto cov = ScalingTerm<Elevation>() * Constant(0.5) + Matern52<EuclideanDistance>(2.0, 1.0) + IndependentNoise<P3>(0.1);
  GaussianProcessRegression<decltype(cov), FirstCoordinateMean> model(cov, FirstCoordinateMean(), "logo_marginal_check");
  RegressionDataset<P3> data(x, MarginalDistribution(y, var));
  const auto g = model.leave_one_group_out_likelihood_gradient<MarginalDistribution>(data, station);
  const LeaveOneGroupOutLikelihood<P3, MarginalDistribution> metric(station);
  for (int i = 0; i < n; ++i)
    std::printf("x,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n", i, x[i][0], x[i][1], x[i][2], y[i], var[i]);
  std::printf("logo_nll,%.17g\n", g.value);
  std::printf("logo_nll_metric,%.17g\n", metric(data, model));
  std::printf("loo_nll_joint,%.17g\n", LeaveOneOutLikelihood<JointDistribution>()(data, model));
  std::printf("loo_nll_marginal,%.17g\n", LeaveOneOutLikelihood<MarginalDistribution>()(data, model));
  for (const auto &kv : g.gradient) std::printf("grad_%s,%.17g\n", kv.first.c_str(), kv.second);
  for (const auto &kv : metric.group_scores(data, model)) std::printf("group_%s,%.17g\n", kv.first.c_str(), kv.second);
  return 0;
}
