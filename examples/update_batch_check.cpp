// update_batch_check.cpp — update_batch (agp_fit_update_batch) through the C++ surface: the FitModels of two fit_batch calls
// (two parameter vectors of one model type, a mean function among them) conditioned on further observations in ONE call,
// against the per-model update() loop.  Prints "key,value" lines: for the information vectors and the mean / marginal /
// joint predictions of the grown fits the maximum absolute difference between the two and the maximum magnitude of the
// loop's values (tests/test_update_batch_cpp_gpu.py holds the differences against the bounds of the Python tests).
// Exits non-zero when a value is not finite.
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
  std::mt19937 gen(13);
  std::uniform_real_distribution<double> u(0., 10.);
  const int n = 300, extra = 70, m = 45, per_call = 3;
  auto cov = Matern52<EuclideanDistance>(2.0, 1.0) + IndependentNoise<P3>(0.1);
  using Model = GaussianProcessRegression<decltype(cov), FirstCoordinateMean>;
  Model model_a(cov, FirstCoordinateMean(), "update_batch_check");
  Model model_b = model_a;
  model_b.set_param("matern_52_length_scale", 1.4);
  model_b.set_param("slope", -0.3);
  auto dataset = [&](int count, int b) {
    std::vector<P3> x(count);
    Vector y(count);
    for (int i = 0; i < count; ++i) {
      x[i] = {u(gen), u(gen), u(gen)};
      y[i] = std::sin(x[i][0]) + std::sin(x[i][1]) + std::sin(x[i][2]) + 0.3 * x[i][0] + 0.05 * b;
    }
    return RegressionDataset<P3>(x, y);
  };
  std::vector<FitModel<Model, P3>> fms;
  for (const Model *model : {&model_a, &model_b}) {
    std::vector<RegressionDataset<P3>> datasets;
    for (int b = 0; b < per_call; ++b) datasets.push_back(dataset(n, b));
    for (auto &fm : model->fit_batch(datasets)) fms.push_back(std::move(fm));
  }
  std::vector<RegressionDataset<P3>> further;
  for (std::size_t b = 0; b < fms.size(); ++b) further.push_back(dataset(extra, (int)b));
  std::vector<P3> xs(m);
  for (auto &p : xs) p = {u(gen), u(gen), u(gen)};

  const auto grown = update_batch(fms, further);
  Worst info, mean, marg_var, joint_cov;
  for (std::size_t b = 0; b < fms.size(); ++b) {
    const auto single = fms[b].update(further[b]);
    const Vector &gi = grown[b].get_fit().information, &si = single.get_fit().information;
    if (gi.size() != (std::size_t)(n + extra) || si.size() != gi.size()) {
      std::printf("update_batch_check FAILED: problem %zu has %zu rows\n", b, gi.size());
      return 1;
    }
    for (std::size_t i = 0; i < gi.size(); ++i) info.add(gi[i], si[i]);
    const auto pb = grown[b].predict(xs), ps = single.predict(xs);
    const Vector bm = pb.mean(), sm = ps.mean();
    const MarginalDistribution bg = pb.marginal(), sg = ps.marginal();
    const JointDistribution bj = pb.joint(), sj = ps.joint();
    for (int j = 0; j < m; ++j) {
      mean.add(bm[j], sm[j]);
      marg_var.add(bg.covariance[j], sg.covariance[j]);
      for (int i = 0; i < m; ++i) joint_cov.add(bj.covariance(i, j), sj.covariance(i, j));
    }
  }
  std::printf("problems,%zu\n", grown.size());
  std::printf("information_diff,%.17g\ninformation_scale,%.17g\n", info.diff, info.scale);
  std::printf("mean_diff,%.17g\nmean_scale,%.17g\n", mean.diff, mean.scale);
  std::printf("marginal_variance_diff,%.17g\nmarginal_variance_scale,%.17g\n", marg_var.diff, marg_var.scale);
  std::printf("joint_covariance_diff,%.17g\njoint_covariance_scale,%.17g\n", joint_cov.diff, joint_cov.scale);
  const bool finite = std::isfinite(info.diff) && std::isfinite(mean.diff) && std::isfinite(marg_var.diff) && std::isfinite(joint_cov.diff);
  std::printf(finite ? "update_batch_check ok\n" : "update_batch_check FAILED: a value is not finite\n");
  return finite ? 0 : 1;
}
