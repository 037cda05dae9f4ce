"""MI355X-native dense Gaussian-process fit/predict engine (albatross hot path).

Host-side mirror of albatross's GaussianProcessRegression / CovarianceFunction
call surface over the C-ABI in include/albatross_amd.h.  All Gram / factor /
solve / predict arithmetic runs in the HIP library; there is no CPU fallback.
"""
from .covariance import (AngularDistance, Constant, CovarianceFunction, EuclideanDistance, Exponential,
                         FeatureSet, IndependentNoise, LinearCombination, Matern32, Matern52, Measurement, MeasurementOnly,
                         Nugget, Polynomial, ProductOfCovarianceFunctions, RadialDistance, ScalingFunction,
                         ScalingTerm, SquaredExponential, SumOfCovarianceFunctions, as_measurements,
                         measurement_only, OnlyForAlternatives, VariantFeatures, only_for_alternatives)

from .gp import (AlbatrossAmdError, DeviceJointDistribution, BlockSymmetric, ExplainedCovariance, PivotedLDLT, Context, DeviceArray, CrossValidation, CrossValidationPrediction, DenseFactor,
                 LeaveOneOutGrouper, LeaveOneOutLikelihood, LeaveOneGroupOutLikelihood, group_indexer, root_mean_square_error, UpdatedGPFit, negative_log_likelihood, FitModel, GaussianProcessRegression, GPFit, JointDistribution,
                 LinearMean, MeanFunction, SumOfMeanFunctions, ProductOfMeanFunctions, MarginalDistribution, NanInputError, NotPositiveDefiniteError, Prediction,
                 RegressionDataset, ZeroMean, default_context, fit_batch, predict_batch, update_batch, log_likelihood_gradient_batch,
                 leave_one_out_likelihood_gradient_batch, pooled_log_likelihood_gradient,
                 pooled_leave_one_out_likelihood_gradient, leave_one_group_out_likelihood_gradient_batch,
                 pooled_leave_one_group_out_likelihood_gradient, gp_from_covariance, gp_from_covariance_and_mean)

from .sparse_gp import (FixedInducingPoints, SparseCrossValidation, SparseCrossValidationPrediction, SparseFitModel, SparseGaussianProcessRegression, SparseGPFit,
                        UniformlySpacedInducingPoints, rebase_inducing_points, sparse_gp_from_covariance,
                        sparse_gp_from_covariance_and_mean)

from .pivoted import GreedyVarianceInducingPoints, PivotedCholesky, pivoted_cholesky

from .iterative import (MATVEC_MAX_RHS, TANGENT_FORMS_MAX_PAIRS, IterativeFitModel, IterativeGPFit, IterativePrediction,
                        NotConvergedError, gram_matvec, gram_tangent_forms)

from .scores import chi_squared_cdf, crps_normal, draw_mvn, energy_score, variogram_score

from .ransac import (RANSAC_RETURN_CODE_EXCEEDED_MAX_FAILED_CANDIDATES, RANSAC_RETURN_CODE_FAILURE, RANSAC_RETURN_CODE_INVALID,
                     RANSAC_RETURN_CODE_INVALID_ARGUMENTS, RANSAC_RETURN_CODE_NO_CONSENSUS, RANSAC_RETURN_CODE_SUCCESS,
                     AlwaysAcceptCandidateMetric, ChiSquaredCdf, ChiSquaredConsensusMetric, ChiSquaredIsValidCandidateMetric,
                     DefaultGPRansacStrategy, DifferentialEntropyConsensusMetric, FeatureCountConsensusMetric,
                     GaussianProcessRansacStrategy, GPRansacScorer, NegativeLogLikelihood, Ransac, RansacConfig, RansacFit,
                     RansacIteration, RansacOutput, draw_candidates, gp_ransac_strategy, ransac, ransac_return_code_to_string,
                     ransac_success)

__all__ = [n for n in dir() if not n.startswith("_")]
