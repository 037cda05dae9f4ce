// sparse_logo_check.cpp — leave-one-group-out cross validation of the sparse model from one fit, through the C++ surface:
// SparseGaussianProcessRegression::leave_one_group_out_likelihood<PredictType>, group_scores<PredictType> and
// held_out_predictions (agp_sparse_held_out) for a Matern-5/2 + measurement-only noise model on seeded 3-D data with
// target variances, groups by the first coordinate, every 10th observation an inducing point.  Prints "key,value" lines
// (the data, the metric for both predict types, one group_<type>_<key> row per group, the held-out prediction of one
// group) that tests/test_sparse_held_out_gpu.py compares with the Python surface.
#include <array>
#include <cmath>
#include <cstdio>
#include <random>

#include <albatross_amd/albatross.hpp>

using namespace albatross;
using P3 = std::array<double, 3>;

struct EveryTenth {  // an InducingPointStrategy: a fixed subset of the observations
  template <typename Cov>
  std::vector<P3> operator()(const Cov &, const std::vector<P3> &features) const {
    std::vector<P3> u;
    for (std::size_t i = 0; i < features.size(); i += 10) u.push_back(features[i]);
    return u;
  }
};

int main() {
  std::mt19937 gen(23);
  std::uniform_real_distribution<double> uni(0., 10.), w(0.01, 0.04);
  const int n = 300;
  std::vector<P3> x(n);
  Vector y(n), var(n);
  for (int i = 0; i < n; ++i) {
    x[i] = {uni(gen), uni(gen), uni(gen)};
    y[i] = std::sin(x[i][0]) + std::sin(x[i][1]) + std::sin(x[i][2]) + 0.3 * x[i][0];
    var[i] = w(gen);
  }
  auto cov = Matern52<EuclideanDistance>(2.0, 1.0) + measurement_only(IndependentNoise<P3>(0.2));
  const auto grouper = [](const P3 &p) { return static_cast<long>(std::floor(p[0] / 1.3)); };
  auto model = sparse_gp_from_covariance(cov, grouper, EveryTenth(), "sparse_logo_check");
  model.set_param_value(details::inducing_nugget_name(), 1e-6);
  RegressionDataset<P3> data(x, MarginalDistribution(y, var));
  for (int i = 0; i < n; ++i) std::printf("x,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n", i, x[i][0], x[i][1], x[i][2], y[i], var[i]);
  std::printf("logo_joint,%.17g\n", model.leave_one_group_out_likelihood<JointDistribution>(data));
  std::printf("logo_marginal,%.17g\n", model.leave_one_group_out_likelihood<MarginalDistribution>(data));
  for (const auto &kv : model.group_scores<JointDistribution>(data)) std::printf("group_joint_%ld,%.17g\n", kv.first, kv.second);
  for (const auto &kv : model.group_scores<MarginalDistribution>(data)) std::printf("group_marginal_%ld,%.17g\n", kv.first, kv.second);
  const auto held = model.held_out_predictions(data);
  const JointDistribution &p = held.at(3);
  std::printf("held_size,%zu\n", p.mean.size());
  for (std::size_t i = 0; i < p.mean.size(); ++i)
    std::printf("held,%zu,%.17g,%.17g,%.17g\n", i, p.mean[i], p.covariance(static_cast<std::int64_t>(i), static_cast<std::int64_t>(i)),
                p.covariance(static_cast<std::int64_t>(i), 0));
  return 0;
}
