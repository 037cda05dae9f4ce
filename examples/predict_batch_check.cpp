// predict_batch_check.cpp — predict_batch (agp_predict_batch) through the C++ surface: the FitModels of two fit_batch calls
// (two parameter vectors of one model type, a mean function among them) predicted in lock step, against the per-model
// predict() loop.  Prints "key,value" lines: for mean / marginal / joint the maximum absolute difference between the two
// and the maximum magnitude of the loop's values (tests/test_predict_batch_cpp_gpu.py holds the differences against the
// bounds of the Python tests).  Exits non-zero when a value is not finite.
#include <array>
#include <cmath>
#include <cstdio>
#include <random>

#include <albatross_amd/albatross.hpp>

using namespace albatross;
using P3 = std::array<double, 3>;

struct FirstCoordinateMean {  // slope * x[0] + offset on 3-D features (LinearMean is 1-D)
  double slope = 0.2, offset = -0.4;
  std::string get_name() const { return "first_coordinate_linear"; }
  ParameterStore get_params() const { return {{"slope", slope}, {"offset", offset}}; }
  bool has_param(const std::string &n) const { return n == "slope" || n == "offset"; }
  void set_param(const std::string &n, double v) { (n == "slope" ? slope : offset) = v; }
  double _call_impl(const P3 &x) const { return slope * x[0] + offset; }
};

struct Worst {
  double diff = 0., scale = 0.;
  void add(double got, double want) {
    diff = std::fmax(diff, std::fabs(got - want));
    scale = std::fmax(scale, std::fabs(want));
    if (!std::isfinite(got) || !std::isfinite(want)) diff = INFINITY;
  }
};

int main() {
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> u(0., 10.);
  const int n = 300, m = 45, per_call = 3;
  auto cov = Matern52<EuclideanDistance>(2.0, 1.0) + IndependentNoise<P3>(0.1);
  using Model = GaussianProcessRegression<decltype(cov), FirstCoordinateMean>;
  Model model_a(cov, FirstCoordinateMean(), "predict_batch_check");
  Model model_b = model_a;
  model_b.set_param("matern_52_length_scale", 1.4);
  model_b.set_param("slope", -0.3);
  std::vector<FitModel<Model, P3>> fms;
  for (const Model *model : {&model_a, &model_b}) {
    std::vector<RegressionDataset<P3>> datasets;
    for (int b = 0; b < per_call; ++b) {
      std::vector<P3> x(n);
      Vector y(n);
      for (int i = 0; i < n; ++i) {
        x[i] = {u(gen), u(gen), u(gen)};
        y[i] = std::sin(x[i][0]) + std::sin(x[i][1]) + std::sin(x[i][2]) + 0.3 * x[i][0] + 0.05 * b;
      }
      datasets.emplace_back(x, y);
    }
    for (auto &fm : model->fit_batch(datasets)) fms.push_back(std::move(fm));
  }
  std::vector<std::vector<P3>> xs(fms.size(), std::vector<P3>(m));
  for (auto &v : xs)
    for (auto &p : v) p = {u(gen), u(gen), u(gen)};

  const auto batch = predict_batch(fms, xs);
  const auto means = batch.mean();
  const auto marginals = batch.marginal();
  const auto joints = batch.joint();
  Worst mean, marg_mean, marg_var, joint_mean, joint_cov;
  for (std::size_t b = 0; b < fms.size(); ++b) {
    const auto single = fms[b].predict(xs[b]);
    const Vector sm = single.mean();
    const MarginalDistribution sg = single.marginal();
    const JointDistribution sj = single.joint();
    for (int j = 0; j < m; ++j) {
      mean.add(means[b][j], sm[j]);
      marg_mean.add(marginals[b].mean[j], sg.mean[j]);
      marg_var.add(marginals[b].covariance[j], sg.covariance[j]);
      joint_mean.add(joints[b].mean[j], sj.mean[j]);
      for (int i = 0; i < m; ++i) joint_cov.add(joints[b].covariance(i, j), sj.covariance(i, j));
    }
  }
  std::printf("problems,%zu\n", fms.size());
  std::printf("mean_diff,%.17g\nmean_scale,%.17g\n", mean.diff, mean.scale);
  std::printf("marginal_mean_diff,%.17g\nmarginal_mean_scale,%.17g\n", marg_mean.diff, marg_mean.scale);
  std::printf("marginal_variance_diff,%.17g\nmarginal_variance_scale,%.17g\n", marg_var.diff, marg_var.scale);
  std::printf("joint_mean_diff,%.17g\njoint_mean_scale,%.17g\n", joint_mean.diff, joint_mean.scale);
  std::printf("joint_covariance_diff,%.17g\njoint_covariance_scale,%.17g\n", joint_cov.diff, joint_cov.scale);
  const bool finite = std::isfinite(mean.diff) && std::isfinite(marg_mean.diff) && std::isfinite(marg_var.diff) &&
                      std::isfinite(joint_mean.diff) && std::isfinite(joint_cov.diff);
  std::printf(finite ? "predict_batch_check ok\n" : "predict_batch_check FAILED: a value is not finite\n");
  return finite ? 0 : 1;
}
