// GP RANSAC through the C++ names (include/albatross_amd/albatross.hpp): test_ransac_direct of the reference's
// tests/test_ransac.cc on make_toy_linear_data() with observations 3 and 5 set to (-1)^i 400.  LeaveOneOutGrouper,
// threshold 1, sample 3, min consensus 3, 20 iterations, DefaultGPRansacStrategy: the consensus must hold 8 groups and
// leave 3 and 5 out.  Also the chi-squared strategy of MakeRansacChiSquaredGaussianProcess on the clean data, the
// edge-case return codes, and prediction through the wrapper.  Prints name,value rows; exits non-zero on a mismatch.
#include <cmath>
#include <cstdio>
#include <string>

#include "albatross_amd/albatross.hpp"

using namespace albatross;

static int failures = 0;
static void expect(bool ok, const char *what) {
  if (!ok) {
    std::printf("FAILED,%s\n", what);
    ++failures;
  }
}

int main() {
  const double toy_y[10] = {5.01841281968535, 5.899404483909093, 6.9658019644108045, 7.995527586269562,
                            9.027844091455382, 9.941910600141895, 10.984848510737773, 11.885256581824562,
                            12.938899996351795, 13.881048261401078};  // make_toy_linear_data(): tests/golden/toy_linear.json
  std::vector<double> x(10);
  Vector clean(10), y(10);
  for (int i = 0; i < 10; ++i) {
    x[i] = i;
    clean[i] = y[i] = toy_y[i];
  }
  for (int i : {3, 5}) y[i] = std::pow(-1., i) * 400.;
  const auto cov = SquaredExponential<EuclideanDistance>(100., 100.) + measurement_only(IndependentNoise<double>(0.1));
  const auto model = gp_from_covariance(cov, "toy");
  const RegressionDataset<double> dataset(x, y);

  const DefaultGPRansacStrategy strategy;
  const auto ransac_model = model.ransac(strategy, 1., 3, 3, 20);
  expect(ransac_model.get_name() == "ransac[toy]", "get_name");
  const auto fit_model = ransac_model.fit(dataset);
  const auto &out = fit_model.get_fit().ransac_output;
  const auto consensus = out.best.consensus();
  std::printf("return_code,%s\n", to_string(out.return_code).c_str());
  std::printf("iterations,%zu\n", out.iterations.size());
  std::printf("consensus_size,%zu\n", consensus.size());
  std::string members;
  for (const auto g : consensus) members += (members.empty() ? "" : " ") + std::to_string(g);
  std::printf("consensus,%s\n", members.c_str());
  std::printf("consensus_metric,%.17g\n", out.best.consensus_metric_value);
  expect(ransac_success(out.return_code), "success");
  expect(consensus.size() == 8, "consensus of 8");
  expect(out.best.outliers.count(3) == 1 && out.best.outliers.count(5) == 1, "3 and 5 are outliers");
  expect(std::isfinite(out.best.consensus_metric_value), "finite consensus metric");
  expect(fit_model.get_fit().has_fit_model(), "has_fit_model");

  // test_ransac_model: the wrapper predicts like the sub-model fit to the consensus set
  RegressionDataset<double> good;
  for (const auto g : consensus) {
    good.features.push_back(x[g]);
    good.targets.mean.push_back(y[g]);
  }
  const std::vector<double> xs = {-1., 0.5, 3., 5., 7.25, 11.};
  const Vector a = fit_model.predict(xs).mean(), b = model.fit(good).predict(xs).mean();
  double worst = 0.;
  for (std::size_t i = 0; i < a.size(); ++i) worst = std::fmax(worst, std::fabs(a[i] - b[i]));
  std::printf("predict_diff,%.3g\n", worst);
  expect(worst == 0., "predict forwards to the consensus fit");

  // the chi-squared strategy on the clean data: every group agrees
  const auto chi = gp_ransac_strategy(ChiSquaredCdf(), ChiSquaredConsensusMetric(), ChiSquaredIsValidCandidateMetric(),
                                      LeaveOneOutGrouper());
  const auto chi_fit = model.ransac(chi, RansacConfig(0.999, 3, 3, 20, 20)).fit(RegressionDataset<double>(x, clean));
  const auto &chi_out = chi_fit.get_fit().ransac_output;
  std::printf("chi_squared_return_code,%s\n", to_string(chi_out.return_code).c_str());
  std::printf("chi_squared_consensus_size,%zu\n", chi_out.best.consensus().size());
  std::printf("chi_squared_consensus_metric,%.17g\n", chi_out.best.consensus_metric_value);
  expect(ransac_success(chi_out.return_code) && chi_out.best.consensus().size() == 10, "chi-squared strategy keeps all ten");
  expect(chi_out.best.consensus_metric_value >= 0. && chi_out.best.consensus_metric_value <= 1., "chi-squared consensus metric in [0, 1]");

  // the differential entropy consensus metric and the marginal inlier metric
  const auto ent = gp_ransac_strategy(NegativeLogLikelihood<MarginalDistribution>(), DifferentialEntropyConsensusMetric(),
                                      LeaveOneOutGrouper());
  const auto ent_out = model.ransac(ent, 1., 3, 3, 20).fit(dataset).get_fit().ransac_output;
  std::printf("entropy_consensus_size,%zu\n", ent_out.best.consensus().size());
  expect(ransac_success(ent_out.return_code) && std::isfinite(ent_out.best.consensus_metric_value), "entropy strategy");
  expect(ent_out.best.inliers.count(3) == 0 && ent_out.best.inliers.count(5) == 0, "entropy strategy leaves 3 and 5 out");

  // test_ransac_edge_cases
  const auto code = [&](const RansacConfig &config) { return model.ransac(strategy, config).fit(dataset).get_fit().ransac_output.return_code; };
  expect(code(RansacConfig(-HUGE_VAL, 1, 2, 20, 0)) == RANSAC_RETURN_CODE_NO_CONSENSUS, "no consensus");
  expect(code(RansacConfig(1., 1, 10, 20, 0)) == RANSAC_RETURN_CODE_INVALID_ARGUMENTS, "min_consensus_size = G");
  expect(code(RansacConfig(1., 10, 2, 20, 0)) == RANSAC_RETURN_CODE_INVALID_ARGUMENTS, "random_sample_size = G");
  expect(code(RansacConfig(1., 1, 2, 0, 0)) == RANSAC_RETURN_CODE_INVALID_ARGUMENTS, "max_iterations = 0");
  const auto never = gp_ransac_strategy(NegativeLogLikelihood<JointDistribution>(), FeatureCountConsensusMetric(),
                                        ChiSquaredIsValidCandidateMetric(-1.), LeaveOneOutGrouper());
  const auto never_out = model.ransac(never, RansacConfig(1., 1, 2, 20, 3)).fit(dataset).get_fit();
  expect(never_out.ransac_output.return_code == RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES, "exceeded max failed candidates");
  expect(never_out.ransac_output.iterations.size() == 3 && !never_out.has_fit_model(), "three failed candidates, no fit model");

  // the draw is the one every binding makes
  const auto d1 = ransac_draw_candidates(7, 10, 3, 4), d2 = ransac_draw_candidates(7, 10, 3, 4);
  expect(d1 == d2 && d1[0].size() == 3 && d1[0][0] < d1[0][1] && d1[0][1] < d1[0][2] && d1[0][2] < 10, "draw_candidates");

  if (failures) return 1;
  std::printf("ransac_check ok\n");
  return 0;
}
