// ragged_batch_check.cpp — fit_batch, predict_batch and update_batch on datasets of UNEQUAL sizes through the C++ surface
// (agp_fit_create_batch_ragged, then agp_predict_batch and agp_fit_update_batch on fits with differing phantom rows): two
// models (a mean function among them) fit seven datasets each, whose sizes fall into four size classes, against the
// per-model fit / predict / update loop.  Prints "key,value" lines: for the information vectors of the fits, the mean /
// marginal / joint predictions from them, and the information vectors and predictions of the updated fits, the maximum
// absolute difference between batch and loop and the maximum magnitude of the loop's values
// (tests/test_ragged_batch_cpp_gpu.py holds the differences against the bounds of the Python tests).  Exits non-zero when a
// value is not finite or a result has the wrong number of rows.
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
  void print(const char *name) const { std::printf("%s_diff,%.17g\n%s_scale,%.17g\n", name, diff, name, scale); }
};

int main() {
  std::mt19937 gen(17);
  std::uniform_real_distribution<double> u(0., 10.);
  const std::vector<int> sizes = {60, 128, 129, 250, 256, 300, 700};  // the classes {60, 128} {129, 250, 256} {300} {700}
  const int extra = 45, m = 33;
  auto cov = Matern52<EuclideanDistance>(2.0, 1.0) + IndependentNoise<P3>(0.1);
  using Model = GaussianProcessRegression<decltype(cov), FirstCoordinateMean>;
  Model model_a(cov, FirstCoordinateMean(), "ragged_batch_check");
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
  std::vector<FitModel<Model, P3>> fms, singles;
  std::vector<int> rows;
  for (const Model *model : {&model_a, &model_b}) {
    std::vector<RegressionDataset<P3>> datasets;
    for (std::size_t b = 0; b < sizes.size(); ++b) datasets.push_back(dataset(sizes[b], (int)b));
    for (auto &fm : model->fit_batch(datasets)) fms.push_back(std::move(fm));
    for (std::size_t b = 0; b < sizes.size(); ++b) {
      singles.push_back(model->fit(datasets[b]));
      rows.push_back(sizes[b]);
    }
  }
  const std::size_t count = fms.size();
  std::vector<RegressionDataset<P3>> further;
  std::vector<std::vector<P3>> xs(count, std::vector<P3>(m));
  for (std::size_t b = 0; b < count; ++b) {
    further.push_back(dataset(extra, (int)b));
    for (auto &p : xs[b]) p = {u(gen), u(gen), u(gen)};
  }

  Worst fit_info, mean, marg_var, joint_cov, upd_info, upd_mean, upd_var;
  for (std::size_t b = 0; b < count; ++b) {
    const Vector &gi = fms[b].get_fit().information, &si = singles[b].get_fit().information;
    if (gi.size() != (std::size_t)rows[b] || si.size() != gi.size()) {
      std::printf("ragged_batch_check FAILED: fit %zu has %zu rows\n", b, gi.size());
      return 1;
    }
    for (std::size_t i = 0; i < gi.size(); ++i) fit_info.add(gi[i], si[i]);
  }
  const auto batch = predict_batch(fms, xs);
  const std::vector<Vector> bm = batch.mean();
  const std::vector<MarginalDistribution> bg = batch.marginal();
  const std::vector<JointDistribution> bj = batch.joint();
  for (std::size_t b = 0; b < count; ++b) {
    const auto ps = singles[b].predict(xs[b]);
    const Vector sm = ps.mean();
    const MarginalDistribution sg = ps.marginal();
    const JointDistribution sj = ps.joint();
    for (int j = 0; j < m; ++j) {
      mean.add(bm[b][j], sm[j]);
      mean.add(bg[b].mean[j], sm[j]);
      marg_var.add(bg[b].covariance[j], sg.covariance[j]);
      for (int i = 0; i < m; ++i) joint_cov.add(bj[b].covariance(i, j), sj.covariance(i, j));
    }
  }
  const auto grown = update_batch(fms, further);
  for (std::size_t b = 0; b < count; ++b) {
    const auto single = singles[b].update(further[b]);
    const Vector &gi = grown[b].get_fit().information, &si = single.get_fit().information;
    if (gi.size() != (std::size_t)(rows[b] + extra) || si.size() != gi.size()) {
      std::printf("ragged_batch_check FAILED: updated fit %zu has %zu rows\n", b, gi.size());
      return 1;
    }
    for (std::size_t i = 0; i < gi.size(); ++i) upd_info.add(gi[i], si[i]);
    const MarginalDistribution g = grown[b].predict(xs[b]).marginal(), s = single.predict(xs[b]).marginal();
    for (int j = 0; j < m; ++j) {
      upd_mean.add(g.mean[j], s.mean[j]);
      upd_var.add(g.covariance[j], s.covariance[j]);
    }
  }
  std::printf("problems,%zu\n", count);
  fit_info.print("information");
  mean.print("mean");
  marg_var.print("marginal_variance");
  joint_cov.print("joint_covariance");
  upd_info.print("updated_information");
  upd_mean.print("updated_mean");
  upd_var.print("updated_marginal_variance");
  bool finite = true;
  for (const Worst *w : {&fit_info, &mean, &marg_var, &joint_cov, &upd_info, &upd_mean, &upd_var}) finite = finite && std::isfinite(w->diff);
  std::printf(finite ? "ragged_batch_check ok\n" : "ragged_batch_check FAILED: a value is not finite\n");
  return finite ? 0 : 1;
}
