/*
 * albatross_amd.h — C-ABI of the MI355X-native dense Gaussian-process engine.
 *
 * This is the drop-in boundary for the dense GP hot path of swift-nav/albatross
 * (Gram build -> LL^T factor -> solve -> log-marginal-likelihood -> predict).
 * The reference is a header-only C++ template library with no FFI of its own;
 * each entry point below names the reference function (file:line, relative to
 * the albatross checkout) whose work it replaces.  Plain pointers and sizes
 * only; opaque handles; int status returns; no exceptions cross this boundary.
 *
 * Matrix layout: column-major fp64, exactly like Eigen::MatrixXd.
 * Feature layout: row-major n x dim fp64 (array-of-structs, like
 * std::vector<Eigen::Vector3d> / std::vector<double>).
 */
#ifndef ALBATROSS_AMD_H
#define ALBATROSS_AMD_H

#include <stdint.h>

/* Every entry point below is exported with default visibility; the library is built with -fvisibility=hidden, so these
 * declarations ARE its export list (tests/test_capi_host.py compares them with `nm -D`). */
#if defined(__GNUC__) || defined(__clang__)
#define AGP_API __attribute__((visibility("default")))
#else
#define AGP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
typedef enum {
  AGP_OK = 0,
  AGP_ERR_INVALID_ARGUMENT = 1,
  /* the assembled covariance holds a NaN: ALBATROSS_ASSERT(!cov.hasNaN()),
   * include/albatross/src/models/gp.hpp:66 */
  AGP_ERR_NAN_INPUT = 2,
  /* un-pivoted LL^T met a pivot <= 0.  The reference's pivoted LDL^T tolerates semi-definite input: callers
   * that want that behaviour go on to the DEVICE implementation of that algorithm, agp_ldlt_* below (the
   * host mirrors do: gp.py `pivoted_fallback`, albatross.hpp `fit_pivoted`).  There is no CPU path. */
  AGP_ERR_NOT_POSITIVE_DEFINITE = 3,
  AGP_ERR_HIP = 4,
  AGP_ERR_COMM = 5,
  AGP_ERR_UNSUPPORTED = 6,
  AGP_ERR_NO_DEVICE = 7,
  /* agp_iterative_fit_create / agp_iterative_solve: max_iterations reached with a right-hand side still above the
   * tolerance */
  AGP_ERR_NOT_CONVERGED = 8
} agp_status;

/* ---- covariance-function descriptor ------------------------------------- */
/* One node of a postfix (reverse-Polish) program describing a composed
 * CovarianceFunction.  Leaves push one value, SUM / PRODUCT pop two and push
 * one, MEASUREMENT_ONLY pops one and pushes one. */
typedef enum {
  /* sigma^2 exp(-(d/l)^2); params = {length_scale, sigma}
   * src/covariance_functions/radial.hpp:25-33,131-189 */
  AGP_OP_SQUARED_EXPONENTIAL = 1,
  /* sigma^2 exp(-|d/l|);   radial.hpp:191-198,239-287 */
  AGP_OP_EXPONENTIAL = 2,
  /* sigma^2 (1+q) exp(-q), q = sqrt(3) d/l; radial.hpp:289-297,421-459 */
  AGP_OP_MATERN32 = 3,
  /* sigma^2 (1+q+q^2/3) exp(-q), q = sqrt(5) d/l; radial.hpp:461-470,491-529 */
  AGP_OP_MATERN52 = 4,
  /* sigma^2; params = {sigma}; polynomials.hpp:31-61 */
  AGP_OP_CONSTANT = 5,
  /* sigma^2 iff x == y (by value / eq_id); params = {sigma}; noise.hpp:20-44 */
  AGP_OP_INDEPENDENT_NOISE = 6,
  /* sigma^2 iff x == y; params = {sigma}; nugget.hpp:32-49 */
  AGP_OP_NUGGET = 7,
  /* sum_p sigma_p^2 x^p y^p on 1-D features, p = 0..order (order <= 3);
   * params = {sigma_0..sigma_order}; polynomials.hpp:63-90 */
  AGP_OP_POLYNOMIAL = 8,
  /* f(x) f(y) with f precomputed per point in scale column `column`;
   * scaling_function.hpp:58-112 */
  AGP_OP_SCALING = 9,
  /* lhs + rhs; covariance_function.hpp:266-272 */
  AGP_OP_SUM = 10,
  /* lhs * rhs, rhs skipped when lhs == 0; covariance_function.hpp:357-367 */
  AGP_OP_PRODUCT = 11,
  /* sub-covariance iff BOTH arguments are Measurement<>, else 0;
   * measurement.hpp:70-106 */
  AGP_OP_MEASUREMENT_ONLY = 12,
  /* sub-covariance iff the two arguments hold the alternatives (a, b) of a
   * variant<> feature type, in either order, else 0: VariantForwarder
   * (covariance_functions/callers.hpp:419-544) returns 0 for every pair of
   * alternatives a covariance function defines no _call_impl for.  The
   * alternative index of each point travels as a value in scale column
   * `column`; params = {a, b}.  A gated-off term is UNDEFINED for the pair:
   * AGP_OP_SUM / AGP_OP_PRODUCT then keep their other operand alone
   * (covariance_function.hpp:266-294, 357-389); an undefined result is 0. */
  AGP_OP_TYPE_PAIR = 13
} agp_op;

typedef enum {
  AGP_METRIC_EUCLIDEAN = 0, /* distance_metrics.hpp:30-45 */
  AGP_METRIC_RADIAL = 1,    /* distance_metrics.hpp:47-62 */
  AGP_METRIC_ANGULAR = 2    /* distance_metrics.hpp:64-90 */
} agp_metric;

#define AGP_MAX_KERNEL_NODES 32
#define AGP_MAX_STACK 8
#define AGP_MAX_DIM 8
#define AGP_MAX_SCALE_COLUMNS 4

typedef struct {
  int32_t op;     /* agp_op */
  int32_t metric; /* agp_metric, radial leaves only */
  int32_t column; /* AGP_OP_SCALING / AGP_OP_TYPE_PAIR: which scale column */
  int32_t order;  /* AGP_OP_POLYNOMIAL: polynomial order */
  double params[4];
} agp_kernel_node;

typedef enum { AGP_HOST = 0, AGP_DEVICE = 1 } agp_location;

/* A vector of features, flattened to plain-old-data. */
typedef struct {
  int64_t n;
  int32_t dim;             /* 1..AGP_MAX_DIM */
  int32_t n_scale_columns; /* 0..AGP_MAX_SCALE_COLUMNS */
  const double *coords;    /* n x dim row-major */
  /* optional equality ids for IndependentNoise / Nugget (`x == y`,
   * noise.hpp:37-43): equal id <=> equal feature.  NULL: features are equal
   * iff all coords compare equal. */
  const int64_t *eq_id;
  const double *scales;    /* n x n_scale_columns column-major, or NULL */
  int32_t is_measurement;  /* 1: every feature is wrapped in Measurement<> */
  int32_t location;        /* agp_location of coords / eq_id / scales */
} agp_features;

typedef struct agp_context agp_context;
typedef struct agp_kernel agp_kernel;
typedef struct agp_fit agp_fit;
typedef struct agp_comm agp_comm; /* transport of the multi-GPU entry points, see "multi-GPU" below */

/* ---- context ------------------------------------------------------------- */
/* One context per host thread (or externally locked).  Owns the HIP streams
 * and scratch workspaces.  The reference's equivalent state is the model's
 * ThreadPool (src/core/model.hpp:30-36,133-135). */
AGP_API int agp_context_create(int device_id, agp_context **out);
AGP_API void agp_context_destroy(agp_context *ctx);
/* waits for everything queued on ANY of the context's streams (device-wide: hipDeviceSynchronize on its device) */
AGP_API int agp_context_synchronize(agp_context *ctx);
/* last HIP error text for AGP_ERR_HIP, "" otherwise */
AGP_API const char *agp_last_error(const agp_context *ctx);
AGP_API const char *agp_status_string(int status);
/* number of visible HIP devices (0 when no GPU / no driver) */
AGP_API int agp_device_count(void);

/* ---- device memory for AGP_DEVICE arguments ------------------------------ */
/* Every entry point that takes a `location` accepts buffers that already live in HBM (features, targets, outputs).  A host
 * program that links nothing but this library gets such buffers here - plain hipMalloc / hipMemcpy / hipFree on the
 * context's device, so that a caller needs no HIP headers and no second runtime in its process (bench.py allocates its
 * inputs and outputs with exactly these).  The reference keeps everything in host Eigen matrices; its equivalent is the
 * allocation inside Eigen::MatrixXd (models/gp.hpp:61-69 copies features and covariance into the fit).
 * agp_device_malloc: *out = `bytes` of device memory (bytes > 0).  agp_device_free(NULL) is a no-op.
 * agp_memcpy: `kind` = the agp_location of DST; the source is at the other location for AGP_HOST <-> AGP_DEVICE copies
 * (kind AGP_DEVICE: host -> device, kind AGP_HOST: device -> host); synchronous - it returns after the copy, and a
 * device -> host copy waits for the work queued on the context's streams first. */
AGP_API int agp_device_malloc(agp_context *ctx, int64_t bytes, void **out);
AGP_API int agp_device_free(agp_context *ctx, void *ptr);
AGP_API int agp_memcpy(agp_context *ctx, void *dst, const void *src, int64_t bytes, int kind);

/* ---- covariance function ------------------------------------------------- */
/* Flattened get_params() of a composed covariance function
 * (covariance_function.hpp:222-420). Immutable after creation. */
AGP_API int agp_kernel_create(const agp_kernel_node *postfix, int n_nodes,
                      agp_kernel **out);
AGP_API void agp_kernel_destroy(agp_kernel *k);

/* ---- Gram ---------------------------------------------------------------- */
/* compute_covariance_matrix (src/covariance_functions/callers.hpp:38-166).
 * y == NULL: symmetric n x n Gram of x (callers.hpp:107-166), full matrix
 * written. Else the n_x x n_y cross Gram (callers.hpp:38-102).
 * `out` is column-major with leading dimension ld, at out_location. */
AGP_API int agp_gram(agp_context *ctx, const agp_kernel *k, const agp_features *x,
             const agp_features *y, double *out, int64_t ld, int out_location);

/* Gram of LinearCombination<X> features: LinearCombinationCaller (covariance_functions/callers.hpp:321-396),
 *   out(a, b) = sum_{i in a} sum_{j in b} c_i c_j k(x_i, y_j).
 * x (y) holds the EXPANDED points, combination a = expanded points x_offsets[a] .. x_offsets[a + 1) with coefficients
 * x_coefficients[..] (nx + 1 offsets and one coefficient per expanded point, host arrays; offsets[0] = 0,
 * offsets[nx] = x->n).  A side with offsets == NULL is a vector of plain features (nx ignored).  y == NULL: the
 * symmetric Gram of x with itself (evaluated for a >= b and mirrored, callers.hpp:119-127).  The Measurement<> flag
 * of x / y applies to the expanded points (MeasurementForwarder sits outside LinearCombinationCaller).  Gram and
 * contraction both run on the device. */
AGP_API int agp_gram_combined(agp_context *ctx, const agp_kernel *k, const agp_features *x, int64_t nx, const int64_t *x_offsets,
                      const double *x_coefficients, const agp_features *y, int64_t ny, const int64_t *y_offsets,
                      const double *y_coefficients, double *out, int64_t ld, int out_location);

/* ---- fit ----------------------------------------------------------------- */
/* Fit<GPFit<...>>::Fit(features, train_cov, targets) (src/models/gp.hpp:61-69)
 * preceded by the Gram of GaussianProcessBase::_fit_impl (gp.hpp:281-294):
 *   K = k(x, x) + diag(y_var);  K = L L^T;  information = K^-1 y.
 * y, y_var (may be NULL = zeros) live at x->location; the factor stays on the
 * device inside *out.  information (n doubles, host) and log_det (host) may be
 * NULL.  The training features are copied into the fit (gp.hpp:63). */
/* A fit belongs to the context that created it and must be destroyed before
 * that context. */
AGP_API int agp_fit_create(agp_context *ctx, const agp_kernel *k, const agp_features *x,
                   const double *y, const double *y_var, agp_fit **out,
                   double *information, double *log_det);
/* Mixed-precision variant of agp_fit_create (BASELINE.json configs[3], SURVEY
 * section 8d config 4): the same Fit<GPFit> constructor (models/gp.hpp:61-69),
 * but the bulk trailing updates (and the next-block-column update) of the LL^T
 * form their products on the 16-bit matrix pipe: every row is scaled by a power
 * of two taken from the diagonal (|L[i, k]| <= sqrt(A[i, i])), every panel is split
 * ONCE into two fp16 planes (h1 + h2 = the scaled value to 22 bits), a product is
 * the four partial products (four v_mfma_f32_16x16x32_f16 per 16 x 16 x 32 block,
 * each exact in fp32; csrc/gemm_split_planes.hip), accumulated in fp32 inside one launch,
 * un-scaled exactly and subtracted from the fp64 matrix; the panel chain, the matrix
 * and every accumulation between outer steps stay fp64.  (AGP_MIXED_F16=0 selects
 * round 5's path, three bf16 planes and six products per block,
 * csrc/gemm_split_planes.hip; AGP_MIXED_BF16=0 the oldest fallback: fp32-rounded panels on
 * v_mfma_f32_16x16x4_f32.)  The information
 * vector is then refined in fp64: conjugate gradients on the exact fp64 covariance,
 * preconditioned with that factor, until ||y - K a||_2 <= tolerance * ||y||_2,
 * `max_iterations` steps, or the fp64 floor of the system.  *iterations /
 * *residual (may be NULL) report the steps taken and the final relative residual.
 * What the result is good for (tests/test_full_size_configs_gpu.py and
 * tests/test_mixed_precision_gpu.py hold each line; all figures MEASURED,
 * profiles/r06/mixed_log_determinant_by_path.txt):
 *   information vector, predicted means: 1e-8 relative to the fp64 fit (refined) on every path;
 *   predicted variances: 1e-4 relative (they come from the mixed factor);
 *   log_det, default path: BASELINE config 4's covariance at N = 32768 0.017 absolute
 *     = 0.5e-6 N; config 3's kernel (SE(1,1) + noise(0.1)) 0.062 = 1.9e-6 N at N = 32768
 *     and 1.4e-6 N at N = 8192; Matern-5/2(2,1) + noise(0.1) at N = 5300 1.9e-6 N - all
 *     INSIDE the log-likelihood bar of the fp64 path (|nll error| <= 1e-6 N, i.e.
 *     |log_det error| <= 2e-6 N), the last three AT it: the bound is a property of the
 *     covariance function (how much of log|K| sits in the fp32 accumulation), not of N
 *     alone, and is not proven for an arbitrary one;
 *   log_det, bf16 x 3 path: 0.8e-6 N on config 4, 4.3e-6 N / 4.9e-6 N on the other two - outside;
 *   log_det, fp32 fallback path: 1.3e-5 relative (0.6 absolute) on config 4 - outside.
 * Use agp_nll / an fp64 fit where the likelihood must meet the bar for an arbitrary
 * covariance; the host mirrors make reading log_det of a mixed fit an explicit opt-in.
 * The reference has no reduced-precision path; this one exists for problems where one
 * fp64 factorisation is too slow (N >= 32768).  Device memory next to the factor (kept
 * in the context between mixed fits): the exact covariance (8 N^2 B), an fp32 copy of
 * the factor for the preconditioner (4 N^2 B), two panel copies (2 x 3 KB x N: room
 * for the bf16 planes; the fp16 planes take 2 x 2 KB x N of it) and 16 N B of row scales. */
AGP_API int agp_fit_create_mixed(agp_context *ctx, const agp_kernel *k, const agp_features *x,
                         const double *y, const double *y_var, int max_iterations,
                         double tolerance, agp_fit **out, double *information,
                         double *log_det, int *iterations, double *residual);
AGP_API void agp_fit_destroy(agp_fit *fit);
AGP_API int64_t agp_fit_size(const agp_fit *fit);
/* 0-based index of the first non-positive pivot of the last failed factor */
AGP_API int64_t agp_fit_failed_pivot(const agp_fit *fit);
/* sum(log D) of the reference's LDLT == 2 sum(log L_ii)
 * (src/eigen/serializable_ldlt.hpp:128-135) */
AGP_API int agp_fit_log_determinant(const agp_fit *fit, double *out);
/* lower-triangular factor, column-major n x n, strictly-upper part zeroed */
AGP_API int agp_fit_download_factor(agp_context *ctx, const agp_fit *fit, double *L,
                            int64_t ld);
AGP_API int agp_fit_download_information(agp_context *ctx, const agp_fit *fit,
                                 double *information);

/* negative_log_likelihood(deviation, covariance)
 * (src/evaluation/likelihood.hpp:38-66) on K = k(x,x) + diag(y_var):
 *   0.5 (log|K| + y^T K^-1 y + n log 2 pi).
 * Factor is not kept (GaussianProcessBase::log_likelihood, gp.hpp:442-451). */
AGP_API int agp_nll(agp_context *ctx, const agp_kernel *k, const agp_features *x,
            const double *y, const double *y_var, double *out);

/* Exact gradient of agp_nll with respect to covariance parameters: one fit, K^-1 = R^T R with R = L^-1, and
 *   dNLL / dtheta = 1/2 sum_ij (K^-1 - alpha alpha^T)_ij dK_ij / dtheta,   alpha = K^-1 y,
 * with dK / dtheta evaluated pair by pair (never stored).  ~2 N^3 / 3 flop beyond the fit, whatever n_slots is;
 * exact to fp64 rounding (the reference's tuner takes forward differences of the log-likelihood,
 * tune/finite_difference.hpp:37-90).  Two calls give bit-identical results.
 * A slot names one parameter: `node` is the index of a LEAF in the kernel's postfix program and `param`
 *   - for a radial, constant, noise, nugget or polynomial leaf: the index into that node's params[] (derivative with
 *     respect to the raw value, e.g. sigma, not sigma^2);
 *   - for an AGP_OP_SCALING leaf: the column of `tangents` that holds df/dtheta at the n features (column-major,
 *     leading dimension ldt >= n; the highest such column + 1 columns are read).
 * y, y_var and tangents live at x->location, as for agp_nll.  nll (1 value), grad_nll (n_slots values) and
 * information (n values, alpha; may be NULL) are host memory.  Slots that name a non-leaf node or a parameter the
 * leaf does not have, or more than AGP_MAX_GRADIENT_SLOTS slots: AGP_ERR_INVALID_ARGUMENT.  NaN input and a covariance
 * that is not positive definite: AGP_ERR_NAN_INPUT / AGP_ERR_NOT_POSITIVE_DEFINITE, as agp_nll.  With profiling on,
 * agp_last_stage_ms reports 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R, 7 the contraction. */
#define AGP_MAX_GRADIENT_SLOTS 64
typedef struct {
  int32_t node;
  int32_t param;
} agp_gradient_slot;
AGP_API int agp_nll_gradient(agp_context *ctx, const agp_kernel *k, const agp_features *x,
                     const double *y, const double *y_var,
                     int n_slots, const agp_gradient_slot *slots,
                     const double *tangents, int64_t ldt,
                     double *nll, double *grad_nll,
                     double *information);

/* agp_nll_gradient for `count` problems of one size in lock step: problem b computes exactly what agp_nll_gradient computes
 * for kernels[b], features[b] and column b of y / y_var, with its own slot table (same slot semantics: a leaf node and a
 * params[] index, or a tangent column for an AGP_OP_SCALING leaf; gradients with respect to the raw value).  The
 * regime of the tuner and of many independent small models (N of a few hundred to a few thousand), where one gradient
 * is a serial chain of small launches: the batch runs each step once for all problems (blockIdx.y = problem).
 *   kernels[b], features[b]   covariance function and features of problem b: all n equal, all at features[0]->location;
 *                             dim may differ between problems
 *   y, ldy                    targets, n x count column-major at that location (ldy = 0: one vector shared by all)
 *   y_var, ldv                target variances likewise (added to the diagonal), or NULL
 *   n_slots[b], slots[b]      problem b's slot table (0..AGP_MAX_GRADIENT_SLOTS slots; slots[b] may be NULL if it has none)
 *   tangents[b], ldt          problem b's tangent columns at that location (ldt >= n), NULL if it has no AGP_OP_SCALING slot
 *   nll[b]                    the negative log-likelihood (host)
 *   grad_nll, ldg             ldg x count (host): column b holds problem b's n_slots[b] values; ldg >= max n_slots[b]
 *   information, ldi          n x count (host, alpha_b), or NULL
 *   status[b]                 AGP_OK / AGP_ERR_NAN_INPUT / AGP_ERR_NOT_POSITIVE_DEFINITE (host)
 * A failed problem gets nll[b] = NaN and a NaN column of grad_nll (the tuner's NaN objective, tune.hpp:163-165); its
 * column of information is left untouched and the rest of the batch is unaffected.  A malformed argument in any problem
 * (count <= 0, n mismatch, mixed locations, a bad slot, ldg < max n_slots, missing tangents or ldt < n where they are
 * needed) makes the call return AGP_ERR_INVALID_ARGUMENT and write nothing.  No float atomics, fixed-order reductions:
 * two identical calls are bit-identical, and no problem's arithmetic depends on its position or its neighbours.
 * Workspace: about count * (2 lda n + tile images) doubles (the A slab and the R slab of every problem, lda ~ n) -
 * size batches from that.  With profiling on, agp_last_stage_ms reports whole-batch times: 0 gram, 1 factor, 2 alpha
 * and R = L^-1, 6 R^T R, 7 the contraction. */
AGP_API int agp_nll_gradient_batch(agp_context *ctx, int count,
                                   const agp_kernel *const *kernels, const agp_features *const *features,
                                   const double *y, int64_t ldy,
                                   const double *y_var, int64_t ldv,
                                   const int *n_slots,
                                   const agp_gradient_slot *const *slots,
                                   const double *const *tangents, int64_t ldt,
                                   double *nll,
                                   double *grad_nll, int64_t ldg,
                                   double *information, int64_t ldi,
                                   int *status);

/* The leave-one-out likelihood metric, LeaveOneOutLikelihood<>()(dataset, model) (evaluation/model_metrics.hpp:59-72,
 * without the prior term), and its exact gradient with respect to covariance parameters.  Per point i, with
 * K = cov(x, x) + diag(y_var), C = K^-1, alpha = C y, c_i = C_ii and s_i = y_var[i] (0 if y_var is NULL):
 *   v_i = 1/c_i + s_i,   d_i = alpha_i / c_i,   NLL_i = 1/2 (log v_i + d_i^2 / v_i + log 2 pi),   loo_nll = sum_i NLL_i.
 * y_var is used in BOTH places, as the reference does: in the fit (gp.hpp:65) and once more as the truth's variance of
 * the score (prediction_metrics.hpp:113-119).  (agp_nll / log_likelihood add it nowhere.)
 * Gradient (GPML 5.4.2, eqs. 5.10-5.13, with s):
 *   dloo_nll / dtheta = sum_ij W_ij dK_ij / dtheta,   W = C diag(b) C - 1/2 (u alpha^T + alpha u^T),
 *   b_i = (1 - d_i^2/v_i + 2 alpha_i d_i) / (2 v_i c_i^2),   u = C a,   a_i = d_i / (v_i c_i).
 * The steps of agp_nll_gradient (fit, alpha, R = L^-1, C = R^T R), then u = C a, G = diag(b)^1/2 C and
 * C diag(b) C = G^T G on the fp64 MFMA: N^3 flop beyond agp_nll_gradient, whatever n_slots is, then the contraction.
 * For a mean-function parameter, dloo_nll / dtheta = -mean_weights^T dm / dtheta (mean_weights = u; y = targets - m).
 * n_slots == 0 and mean_weights NULL: the value alone, c_i from R's squared column norms (agp_fit_inverse_diagonal);
 * neither C nor G^T G is formed: a fit plus N^3 / 3 flop.
 * Slots, tangents, locations, determinism and status codes as agp_nll_gradient: AGP_ERR_INVALID_ARGUMENT for a slot on
 * a non-leaf node or a parameter the leaf does not have, or more than AGP_MAX_GRADIENT_SLOTS slots; AGP_ERR_NAN_INPUT;
 * AGP_ERR_NOT_POSITIVE_DEFINITE.  loo_nll (1 value), grad_loo_nll (n_slots values) and mean_weights (n values, may be
 * NULL) are host memory.  With profiling on, agp_last_stage_ms reports 0 gram, 1 factor, 2 alpha and R = L^-1,
 * 6 R^T R, 8 the per-point terms, u and G (value only: R's column norms and the terms), 9 G^T G, 7 the contraction;
 * stages a call does not run report 0. */
AGP_API int agp_loo_nll_gradient(agp_context *ctx, const agp_kernel *k, const agp_features *x,
                                 const double *y, const double *y_var,
                                 int n_slots, const agp_gradient_slot *slots,
                                 const double *tangents, int64_t ldt,
                                 double *loo_nll, double *grad_loo_nll,
                                 double *mean_weights);

/* agp_loo_nll_gradient for `count` problems of one size in lock step: problem b computes exactly what
 * agp_loo_nll_gradient computes for kernels[b], features[b] and column b of y / y_var (used in both places, the fit and
 * the truth's variance), with its own slot table.  The leave-one-out counterpart of agp_nll_gradient_batch, for the same
 * regime (a multi-start or finite-difference tuner of the metric, an ensemble over hyper-parameters, one model per
 * station): every step runs once for the whole batch (blockIdx.y = problem), the number of launches does not depend on
 * count.  Arguments as agp_nll_gradient_batch, with
 *   loo_nll[b]                the leave-one-out metric (host)
 *   grad_loo_nll, ldg         ldg x count (host): column b holds problem b's n_slots[b] values; ldg >= max n_slots[b]
 *   mean_weights, ldw         n x count (host, column b is u_b; ldw >= n), or NULL
 *   status[b]                 AGP_OK / AGP_ERR_NAN_INPUT / AGP_ERR_NOT_POSITIVE_DEFINITE (host)
 * A failed problem gets loo_nll[b] = NaN and a NaN column of grad_loo_nll; its column of mean_weights is left untouched
 * and the rest of the batch is unaffected.  A malformed argument in any problem (the list of agp_nll_gradient_batch, or
 * mean_weights with ldw < n) makes the call return AGP_ERR_INVALID_ARGUMENT and write nothing.  Every n_slots[b] == 0 and
 * mean_weights NULL: the values alone, c_i from the squared column norms of the R slabs; neither C, G nor G^T G is formed.
 * No float atomics, fixed-order reductions: two identical calls are bit-identical, and no problem's arithmetic depends on
 * its position or its neighbours.  Workspace: that of agp_nll_gradient_batch (two lda x n slabs per problem: G_b is
 * written over R_b and S_b over C_b) plus five n-vectors per problem.  With profiling on, agp_last_stage_ms reports
 * whole-batch times with the indices of agp_loo_nll_gradient: 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R, 8 the
 * per-point terms, u and G (value only: the column norms and the terms), 9 G^T G, 7 the contraction. */
AGP_API int agp_loo_nll_gradient_batch(agp_context *ctx, int count,
                                       const agp_kernel *const *kernels, const agp_features *const *features,
                                       const double *y, int64_t ldy,
                                       const double *y_var, int64_t ldv,
                                       const int *n_slots,
                                       const agp_gradient_slot *const *slots,
                                       const double *const *tangents, int64_t ldt,
                                       double *loo_nll,
                                       double *grad_loo_nll, int64_t ldg,
                                       double *mean_weights, int64_t ldw,
                                       int *status);

/* The leave-one-GROUP-out likelihood metric, LeaveOneGroupOutLikelihood<FeatureType>(grouper)(dataset, model) with
 * PredictType = JointDistribution (evaluation/model_metrics.hpp:74-93, without the prior term), and its exact gradient
 * with respect to covariance parameters: the objective to tune with when observations come in correlated bunches (one
 * group per station, pass or day), where a point's neighbours in its own group must not stay in the fit.  (PredictType =
 * MarginalDistribution scores the marginals only: agp_logo_nll_gradient_typed below.)
 * Groups as in agp_held_out_predictions: group g holds indices[offsets[g] .. offsets[g + 1]), offsets[0] = 0, host
 * arrays, indices in any order inside a group.  Empty groups contribute nothing; points in no group contribute no term.
 * With K = cov(x, x) + diag(y_var), C = K^-1, alpha = C y, s = y_var (0 if NULL), and per group with index set I (size m):
 *   A = C[I, I]   (SerializableLDLT::inverse_blocks),
 *   Sigma = A^-1,   d = Sigma alpha_I   (held_out_prediction, Joint: cross_validation_utils.hpp:188-197),
 *   V = Sigma + diag(s_I)   (negative_log_likelihood(Joint, Marginal): prediction_metrics.hpp:112-119),
 *   NLL_g = 1/2 (log |V| + d^T V^-1 d + m log 2 pi),   logo_nll = sum_g NLL_g.
 * y_var is used in BOTH places, as for agp_loo_nll_gradient: in the fit, and as the truth's covariance of the score.
 * Gradient, with q = V^-1 d and a_I = Sigma q (a: an n-vector assembled over the groups, 0 where a point is in no group):
 *   B_g = 1/2 Sigma V^-1 Sigma - 1/2 a_I a_I^T + 1/2 (a_I d^T + d a_I^T)   (m x m, symmetric),
 *   B = the block matrix with B_g at [I_g, I_g], zero elsewhere,   u = C a,   W = C B C - 1/2 (u alpha^T + alpha u^T),
 *   dlogo_nll / dtheta = sum_ij W_ij dK_ij / dtheta,   dlogo_nll / dtheta_mean = -mean_weights^T dm / dtheta (mean_weights = u).
 * With singleton groups these are the b_i, a_i, u and W of agp_loo_nll_gradient.  B_g is NOT positive semi-definite in
 * general (B_g = 1/2 Sigma V^-1 Sigma + 1/2 d d^T - 1/2 e e^T, e = diag(s_I) V^-1 d), so the product takes B as a general
 * symmetric block matrix: H = sym(C) B, then C B C = H C^T on the fp64 MFMA.
 * Steps: those of agp_loo_nll_gradient up to C = R^T R; C mirrored to both triangles; the groups sorted by size and cut
 * into chunks of comparable size (at most 2x padding), each chunk ONE chain of batched launches (gather, two LL^T, two
 * triangular solves, two products, the assembly), so the number of chains follows the number of size classes, not of
 * groups; H (2 N sum_g m_g^2 flop); C B C (N^3 flop, as agp_loo_nll_gradient's G^T G); the contraction.
 * n_slots == 0 and mean_weights NULL: the value alone; A_g = R[:, I_g]^T R[:, I_g] from gathered columns of R, and
 * neither C, H nor C B C is formed: a fit plus N^3 / 3 flop plus 2 N sum_g m_g^2 for the blocks.
 * Workspace: ONE lda x n slab more than agp_loo_nll_gradient (C B C cannot overwrite an operand: three slabs, C, H over
 * R, and S), plus three padded block slabs and the tile images of the chunk in flight (at most max(n, m) padded columns
 * and 256 MiB of images per chunk) and O(n) vectors.
 * An index out of range, an index in two groups or twice in one, malformed offsets, or a malformed slot (the list of
 * agp_nll_gradient): AGP_ERR_INVALID_ARGUMENT, nothing written.  A group block (A_g or V_g) that does not factor:
 * AGP_ERR_NOT_POSITIVE_DEFINITE, nothing written.  Slots, tangents, locations and the other status codes as
 * agp_loo_nll_gradient; logo_nll (1 value), grad_logo_nll (n_slots values) and mean_weights (n values, may be NULL) are
 * host memory.  No float atomics, fixed-order reductions: two identical calls are bit-identical.  With profiling on,
 * agp_last_stage_ms reports 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R, 8 the group blocks, u and H (value only:
 * the group blocks from R), 9 the product C B C, 7 the contraction; stages a call does not run report 0. */
AGP_API int agp_logo_nll_gradient(agp_context *ctx, const agp_kernel *k, const agp_features *x,
                                  const double *y, const double *y_var,
                                  int64_t n_groups, const int64_t *offsets, const int64_t *indices,
                                  int n_slots, const agp_gradient_slot *slots,
                                  const double *tangents, int64_t ldt,
                                  double *logo_nll, double *grad_logo_nll,
                                  double *mean_weights);

/* agp_logo_nll_gradient with the score's predict type as an argument, and the metric per group.
 * predict_type = AGP_PREDICT_JOINT, group_nll = NULL is agp_logo_nll_gradient itself, bit for bit.
 * predict_type = AGP_PREDICT_MARGINAL is LeaveOneGroupOutLikelihood<FeatureType, MarginalDistribution>: the second
 * overload of NegativeLogLikelihood (prediction_metrics.hpp:112-128) scores a held-out group against the DIAGONAL of its
 * predictive covariance only, the robust objective for large groups, whose joint score is dominated by the smallest
 * eigenvalues of V.  With the notation of agp_logo_nll_gradient (A = C[I, I], Sigma = A^-1, d = Sigma alpha_I, s = y_var):
 *   v_i = Sigma_ii + s_i   (i in I),
 *   NLL_g = 1/2 sum_i (log v_i + d_i^2 / v_i + log 2 pi),   logo_nll = sum_g NLL_g,
 *   q_i = d_i / v_i,   w_i = 1/2 (1 / v_i - q_i^2),   a_I = Sigma q,
 *   B_g = Sigma diag(w) Sigma + 1/2 (a_I d^T + d a_I^T)   (m x m, symmetric),
 * and B, u = C a, W = C B C - 1/2 (u alpha^T + alpha u^T), dlogo_nll / dtheta = sum_ij W_ij dK_ij / dtheta and the mean
 * term -mean_weights^T dm / dtheta exactly as for the Joint type (which is the same expression with V^-1 in place of
 * diag(1 / v)).  w_i < 0 whenever d_i^2 > v_i: B_g is indefinite in general and goes through the same general symmetric
 * product.  With singleton groups both types are agp_loo_nll_gradient.
 * Steps: the chain of agp_logo_nll_gradient up to Sigma_g; then per column d, v, q and the terms, and for the gradient
 * a_I and the block product (Sigma diag(w)) Sigma^T in place of T^T T: no second LL^T and no second triangular solve;
 * H, C B C and the contraction unchanged.  The value alone stops at the terms.  Same workspace.
 * group_nll (host, n_groups values, or NULL; both predict types, value-only and gradient calls): group_nll[g] = NLL_g
 * of group g in the CALLER's order (the device holds one term per non-empty group in its own order, by size; they are
 * downloaded once and scattered back), 0 for an empty group; their sum is logo_nll up to rounding.
 * An unknown predict_type: AGP_ERR_INVALID_ARGUMENT.  Every other argument, status code, location rule, the profiling
 * stages and the determinism guarantee are those of agp_logo_nll_gradient; on any failure nothing is written, group_nll
 * included.  (Marginal: only A_g is factored, so AGP_ERR_NOT_POSITIVE_DEFINITE refers to A_g.) */
#define AGP_PREDICT_JOINT 0
#define AGP_PREDICT_MARGINAL 1
AGP_API int agp_logo_nll_gradient_typed(agp_context *ctx, const agp_kernel *k, const agp_features *x,
                                        const double *y, const double *y_var,
                                        int64_t n_groups, const int64_t *offsets, const int64_t *indices,
                                        int predict_type,
                                        int n_slots, const agp_gradient_slot *slots,
                                        const double *tangents, int64_t ldt,
                                        double *logo_nll, double *grad_logo_nll,
                                        double *mean_weights, double *group_nll);

/* ---- GP RANSAC: the trials of one run scored in lock step (models/ransac.hpp:172-257 around models/ransac_gp.hpp and
 * models/conditional_gaussian.hpp).  The reference fits and predicts once per trial; here the prior covariance of the
 * measurements is built ONCE and n_trials trials are one batch, each O(s^3 + N s^2) against one N x N Gram.
 * Derived once (gp.hpp:421-425): Sigma = k(as_measurements(x), as_measurements(x)) - y_var is NOT added to it -,
 * d = deviation = y - mean(x), R = diag(y_var) (zeros for NULL).  The grouping is that of agp_logo_nll_gradient (host
 * arrays offsets / indices), here with every group non-empty and no point in two groups; points in no group are never
 * scored.  Trial t has the candidate groups cand_groups[cand_offsets[t] .. cand_offsets[t + 1]) (host, at least one,
 * distinct); with c their points in that order, s = |c|:
 *   A = Sigma_cc + R_c = L L^T,   z = L^-1 d_c,   candidate_quadratic[t] = q_c = z^T z = d_c^T A^-1 d_c,
 *   candidate_log_det[t] = log|A|   (conditional_gaussian.hpp:30-45; chi_squared_cdf(q_c, s) is the candidate check),
 * and for every group g that is not a candidate (conditional_gaussian.hpp:61-91, prediction_metrics.hpp:112-141)
 *   W = L^-1 Sigma_cg,   r = W^T z - d_g,   P = Sigma_gg - W^T W + R_g,
 *   AGP_RANSAC_NLL_JOINT:        1/2 (log|P| + r^T P^-1 r + |g| log 2 pi)
 *   AGP_RANSAC_NLL_MARGINAL:     the same with P -> diag(P)
 *   AGP_RANSAC_CHI_SQUARED_CDF:  chi_squared_cdf(r^T P^-1 r, |g|)   (albatross_amd/chi_squared.h: the host's function)
 * g is an inlier iff metric <= inlier_threshold; a NaN metric (a P that is not positive definite) is an outlier.
 *   metric            n_groups x n_trials, column t = trial t, leading dimension ld_metric >= n_groups, at
 *                     metric_location; NaN at the trial's own candidates; may be NULL
 *   inlier_groups[t], inlier_points[t]   accepted groups and their observations, candidates not counted (host)
 *   status[t]         AGP_OK, or AGP_ERR_NOT_POSITIVE_DEFINITE when A did not factor: that trial's metrics, q_c and
 *                     log|A| are NaN and its counts 0; the other trials are unaffected (host)
 * deviation and y_var live at x->location.
 * Size limits, checked before anything is launched (AGP_ERR_INVALID_ARGUMENT, nothing written): at most
 * AGP_RANSAC_MAX_CANDIDATE_POINTS candidate points per trial and AGP_RANSAC_MAX_GROUP_POINTS points per group - the
 * scoring kernel keeps W for one tile of 64 columns in LDS, 128 KiB of the CU's 160 KiB at s = 256 -, 1 <= n_trials
 * <= 65535; likewise a candidate id out of range or twice in one trial, an empty group, an index out of range or in
 * two groups, malformed offsets, an unknown inlier_metric.
 * Stages: the Gram; a gather of A_t and d_c into slabs padded with a unit diagonal; the batched LL^T of
 * agp_fit_create_batch in its plain schedule; ONE scoring launch over (tile of groups, trial); a per-trial reduction.
 * Trials run in size classes of 16, 32, 64, 128 and 256 candidate points, so a trial's padding depends on the trial
 * alone: a trial scored on its own and the same trial inside any batch give identical bits, as do two identical calls.
 * Workspace: the N x N Gram, n_groups x n_trials metrics, and at most 512 MiB of slabs for the trials in flight.
 * With profiling on, agp_last_stage_ms reports 0 gram, 2 gather, 1 factor, 8 scoring and counts. */
#define AGP_RANSAC_NLL_JOINT 0
#define AGP_RANSAC_NLL_MARGINAL 1
#define AGP_RANSAC_CHI_SQUARED_CDF 2
#define AGP_RANSAC_MAX_CANDIDATE_POINTS 256
#define AGP_RANSAC_MAX_GROUP_POINTS 64
AGP_API int agp_ransac_score_trials(agp_context *ctx, const agp_kernel *k, const agp_features *x,
                                    const double *deviation, const double *y_var,
                                    int64_t n_groups, const int64_t *offsets, const int64_t *indices,
                                    int64_t n_trials, const int64_t *cand_offsets, const int64_t *cand_groups,
                                    int inlier_metric, double inlier_threshold,
                                    double *metric, int64_t ld_metric, int metric_location,
                                    int64_t *inlier_groups, int64_t *inlier_points,
                                    double *candidate_quadratic, double *candidate_log_det, int *status);

/* The candidate sets of n_trials trials: out[t * sample_size .. (t + 1) * sample_size) holds sample_size distinct group
 * ids of 0 .. n_groups - 1 in ascending order (host only; no context).  This is the project's OWN seeded draw, one
 * function for every binding so that Python and C++ draw the same sets: trial t seeds a splitmix64 stream with
 * seed ^ (0xD1B54A32D192ED03 * (t + 1)), Floyd's sampling without replacement takes unbiased (rejection) integers from it,
 * and the set is sorted.  It does NOT reproduce the sequence of libstdc++'s std::default_random_engine that the
 * reference's random_without_replacement walks through, so the trials differ from the reference's for the same seed.
 * sample_size > n_groups or a negative size: AGP_ERR_INVALID_ARGUMENT. */
AGP_API int agp_ransac_draw_candidates(uint64_t seed, int64_t n_groups, int64_t sample_size, int64_t n_trials,
                                       int64_t *out);

/* Tuner objective batching: agp_nll for `count` parameter vectors of one model on one dataset in lock step
 * (batched Gram slabs + batched LL^T; blockIdx.y = parameter vector) — the evaluations that
 * compute_gradient (include/albatross/src/tune/finite_difference.hpp:20-94) and the ModelTuner objective
 * (include/albatross/src/tune/tune.hpp:151-161,276-290) perform one after the other.
 *   kernels[b]   the covariance function with parameter vector b
 *   features[b]  its feature view (normally all the same arrays; they differ only when a ScalingTerm
 *                parameter is tuned); all n equal, all at the same location
 *   y            n x count column-major with leading dimension ldy at that location (mean function removed
 *                per parameter vector); ldy = 0: one target vector shared by all
 *   out[b]       the negative log likelihood (host); NaN where the covariance is not positive definite or
 *                has NaN (the reference turns a NaN metric into +inf, tune.hpp:163-165)
 * count is at most 65535 (the batch is one grid dimension of every launch): a larger one, like any other malformed
 * argument, returns AGP_ERR_INVALID_ARGUMENT and writes nothing. */
AGP_API int agp_nll_batch(agp_context *ctx, int count, const agp_kernel *const *kernels,
                  const agp_features *const *features, const double *y, int64_t ldy, const double *y_var,
                  double *out);

/* `count` INDEPENDENT fits of one shape in lock step: the Fit<GPFit> constructor (src/models/gp.hpp:61-69) for several
 * datasets / parameter vectors of n points each at once - the regime of the reference's own workloads
 * (benchmarks/bench_predict.cc:20-40: N = 512; the tuner, tune/tune.hpp:276-290), where one fit alone is bound by the
 * latency of its serial pivots.  The batch shares that latency and fills the GPU with the updates of all problems.
 *   kernels[b], features[b]   covariance function and features of problem b (all n equal, all at one location)
 *   y, ldy                    targets, n x count column-major at that location (ldy = 0: one vector shared by all)
 *   y_var, ldv                target variances likewise, or NULL
 *   out[b]                    an ordinary agp_fit per problem (agp_predict_*, agp_solve, agp_fit_destroy as usual); the fits of
 *                             a batch share one device allocation, released with the last of them
 *   information, ldi          n x count (host) or NULL; log_det[b] (host) or NULL
 *   status[b]                 AGP_OK / AGP_ERR_NAN_INPUT / AGP_ERR_NOT_POSITIVE_DEFINITE per problem (out[b] then reports
 *                             the pivot like agp_fit_create); the return value is about the call as a whole: when it is not
 *                             AGP_OK no handle has been published (every out[b] is NULL) and nothing is left to destroy
 * y and y_var live where features[0] lives (host or device); `information` and `log_det` are HOST arrays whatever the
 * location, and a failed problem leaves its column of `information` untouched.  No pivoted fall-back is applied to a
 * problem that is not positive definite (agp_fit_create's callers go on to agp_ldlt_*; a batch reports and moves on).
 * count is at most 65535 (the batch is one grid dimension of every launch): a larger one returns
 * AGP_ERR_INVALID_ARGUMENT and writes nothing, out and status included. */
AGP_API int agp_fit_create_batch(agp_context *ctx, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                                 const double *y, int64_t ldy, const double *y_var, int64_t ldv, agp_fit **out, double *information,
                                 int64_t ldi, double *log_det, int *status);

/* agp_fit_create_batch for problems of UNEQUAL sizes: the same arguments, but features[b]->n = n_b may differ (many small
 * models, one per station or satellite, never have the same number of observations).  The padded size n of the call is
 * the largest n_b (not rounded).  Problem b is fitted as diag(K_b, I): its handle is an ordinary fit of n_b observations
 * that carries the trailing phantom rows [n_b, n) - identity rows of the factor, zero information, decoupled from
 * everything, the representation agp_fit_update has always used - and every entry shows the n_b real rows only
 * (agp_fit_size, agp_fit_download_information / _factor, agp_solve, agp_predict_*, agp_fit_update,
 * agp_fit_inverse_diagonal; the entries that decline phantom fits - cross validation, agp_draw_mvn - decline these too).
 *   y, ldy            column b holds n_b values; what follows them in the column is never read.  ldy (0: one shared
 *                     vector of n values), ldv (with y_var) and ldi (with information) are at least n
 *   information, ldi  column b receives n_b values; the rest of the column is not written
 *   log_det[b]        that of K_b; status[b] and agp_fit_failed_pivot count real rows
 * Every size must be positive; otherwise the rules of agp_fit_create_batch hold, per-problem failures included.  A
 * malformed argument returns AGP_ERR_INVALID_ARGUMENT and writes nothing, out and status included.  With all sizes equal
 * the call runs the launches of agp_fit_create_batch and returns the same bits.  One device allocation for the batch, one
 * synchronisation behind host-resident inputs and one at the end; fixed-order reductions, no atomics: two identical calls
 * give the same bits.  The cost of the padding: every problem is factored at size n.  Callers bound it by batching sizes
 * of one class ceil(n_b / 128) per call, as the Python and C++ surfaces do.
 * Not covered: unequal numbers of test points in agp_predict_batch and of new points in agp_fit_update_batch, a ragged
 * agp_nll_batch, cross validation of phantom fits, mixed precision, the sharded path.  (The batched gradients of unequal
 * sizes: agp_nll_gradient_batch_ragged and agp_loo_nll_gradient_batch_ragged below.) */
AGP_API int agp_fit_create_batch_ragged(agp_context *ctx, int count, const agp_kernel *const *kernels,
                                        const agp_features *const *features, const double *y, int64_t ldy, const double *y_var,
                                        int64_t ldv, agp_fit **out, double *information, int64_t ldi, double *log_det, int *status);

/* The rows the factor of `fit` holds, phantom rows included (agp_fit_size counts the real ones).  agp_predict_batch and
 * agp_fit_update_batch take fits of one padded size per call. */
AGP_API int64_t agp_fit_padded_size(const agp_fit *fit);

/* agp_nll_gradient_batch for problems of UNEQUAL sizes: the same arguments, but features[b]->n = n_b > 0 may differ (the
 * models that agp_fit_create_batch_ragged fits are tuned with this).  The padded size n of the call is the largest n_b
 * (not rounded).  Problem b computes what agp_nll_gradient computes for its n_b points - the value with n_b log 2 pi, the
 * gradient, alpha_b - as the problem diag(K_b, I): its Gram launch runs on the n_b real rows (so the target variance goes
 * onto real diagonals and the NaN flag comes from real rows only), one pad launch writes the phantom rows [n_b, n) of
 * its slab as identity rows, the factor, alpha, R = L^-1 and R^T R run at size n, and the contraction takes the pairs of
 * the n_b real points only.
 *   y, ldy            column b holds n_b values; what follows them in the column is never read.  ldy and (with y_var) ldv
 *                     are 0 (one shared vector of n values, of which problem b uses the first n_b) or at least n
 *   tangents[b], ldt  every tangent column holds n_b values; ldt >= n whenever some problem has a tangent column
 *   information, ldi  column b receives n_b values; the rest of the column is not written; ldi >= n
 *   status[b]         per problem, about real rows only
 * A failed problem gets nll[b] = NaN and a NaN gradient column and leaves its column of information untouched; its
 * neighbours are unaffected.  A malformed argument anywhere (the list of agp_nll_gradient_batch without the n mismatch, a
 * size <= 0, a leading dimension below n, mixed locations, count > 65535) returns AGP_ERR_INVALID_ARGUMENT and writes
 * nothing, status included.  With all sizes equal the call runs the launches of agp_nll_gradient_batch and returns the
 * same bits.  No float atomics, fixed-order reductions: two identical calls are bit-identical.  The cost of the padding:
 * every problem is factored at size n; callers bound it by batching sizes of one class ceil(n_b / 128) per call, as the
 * Python and C++ surfaces do.  Stage indices of agp_last_stage_ms as agp_nll_gradient_batch (the pad launch counts to
 * stage 0). */
AGP_API int agp_nll_gradient_batch_ragged(agp_context *ctx, int count,
                                          const agp_kernel *const *kernels, const agp_features *const *features,
                                          const double *y, int64_t ldy,
                                          const double *y_var, int64_t ldv,
                                          const int *n_slots,
                                          const agp_gradient_slot *const *slots,
                                          const double *const *tangents, int64_t ldt,
                                          double *nll,
                                          double *grad_nll, int64_t ldg,
                                          double *information, int64_t ldi,
                                          int *status);

/* agp_loo_nll_gradient_batch for problems of UNEQUAL sizes, with the rules of agp_nll_gradient_batch_ragged: problem b
 * computes what agp_loo_nll_gradient computes for its n_b points (the sum of n_b terms with n_b log 2 pi, the gradient,
 * u_b).  The per-point terms of a phantom row are written as zero and its target variance is never read.
 *   mean_weights, ldw  column b receives the n_b values of u_b; the rest of the column is not written; ldw >= n
 * The value-only path (every n_slots[b] == 0, mean_weights NULL) is that of agp_loo_nll_gradient_batch.  With all sizes
 * equal the call runs the launches of agp_loo_nll_gradient_batch and returns the same bits; stage indices likewise. */
AGP_API int agp_loo_nll_gradient_batch_ragged(agp_context *ctx, int count,
                                              const agp_kernel *const *kernels, const agp_features *const *features,
                                              const double *y, int64_t ldy,
                                              const double *y_var, int64_t ldv,
                                              const int *n_slots,
                                              const agp_gradient_slot *const *slots,
                                              const double *const *tangents, int64_t ldt,
                                              double *loo_nll,
                                              double *grad_loo_nll, int64_t ldg,
                                              double *mean_weights, int64_t ldw,
                                              int *status);

/* agp_logo_nll_gradient_typed for `count` problems of any mix of sizes in lock step, with the rules of
 * agp_loo_nll_gradient_batch_ragged for everything but the groups: problem b computes what agp_logo_nll_gradient_typed
 * computes on its own n_b = features[b]->n points (formulas there), as the problem diag(K_b, I) at the padded size n of the
 * call (the largest n_b).  Phantom rows belong to no group and to no pair of the contraction.
 *   n_groups[b], offsets[b], indices[b]   the groups of problem b, host arrays with the rules of agp_logo_nll_gradient and
 *                     indices < n_b: empty groups and points in no group are allowed; offsets[b] and indices[b] may be NULL
 *                     where n_groups[b] == 0 (the tables themselves may then be NULL).  A problem with no non-empty group
 *                     gets the value 0 and a zero gradient
 *   predict_type      AGP_PREDICT_JOINT or AGP_PREDICT_MARGINAL, one for the call
 *   logo_nll[b]       the value per problem (host)
 *   grad_logo_nll, ldg   column b holds the n_slots[b] derivatives of problem b (host); ldg >= the largest n_slots[b]
 *   mean_weights, ldw    column b receives the n_b values of u_b (host), or NULL; ldw >= n
 *   group_nll         NULL, or a host table of `count` pointers; group_nll[b] is NULL or receives n_groups[b] values in the
 *                     caller's order, 0 for an empty group, their sum logo_nll[b] up to rounding (NaN for a failed problem)
 *   status[b]         AGP_OK / AGP_ERR_NAN_INPUT / AGP_ERR_NOT_POSITIVE_DEFINITE per problem (host)
 * A problem FAILS when its covariance or one of its group blocks (A_g, Joint: or V_g) does not factor, or when its input has
 * NaN: it gets its status, logo_nll[b] = NaN, a NaN gradient column and an untouched column of mean_weights, and the rest of
 * the batch is unaffected.  A malformed argument in ANY problem - the lists of agp_logo_nll_gradient and of
 * agp_loo_nll_gradient_batch_ragged, an index >= n_b even where it is below n, an unknown predict_type, count <= 0 or
 * > 65535 - returns AGP_ERR_INVALID_ARGUMENT and writes nothing, status included: every problem is checked before anything is
 * launched.
 * Steps: the front end of agp_loo_nll_gradient_batch_ragged up to C_b = R_b^T R_b (with all sizes equal: its equal-size
 * launches), C_b mirrored; then the group-block chain of agp_logo_nll_gradient_typed ONCE for the groups of all problems:
 * the non-empty groups of the whole batch are sorted by (size, problem, group) and cut into chunks under the limits of the
 * single call (largest group at most 2x the smallest, 16384 groups, 256 MiB of tile images, count * n padded columns), each
 * chunk ONE chain of batched launches whose kernels take every group's problem from a table, so the number of chains
 * follows the size classes of the batch, not the number of problems or groups.  The plan is made before any status is
 * known: the groups of a failed problem run as identity blocks with zero alpha, so nothing NaN enters the chain and
 * nothing waits on the host.  Then one launch sums every problem's terms in a fixed order and folds the status of its
 * blocks into its own, u_b = C_b a_b, H_b, S_b = H_b C_b^T and the contraction, each one launch for the batch.  The value
 * alone (every n_slots[b] == 0, mean_weights NULL) takes its blocks from C_b too - the route over gathered columns of R of
 * the single call is not used - and forms no a, H or S.
 * A group shares its chunk's padded size with groups of OTHER problems, so a problem's bits may depend on the composition
 * of the batch: agreement with agp_logo_nll_gradient_typed called alone is to rounding (1e-10 relative on the value in the
 * tests), not to bits.  No float atomics, fixed-order reductions: two identical calls are bit-identical.
 * Workspace per problem: that of agp_loo_nll_gradient_batch_ragged (the C and R slabs, 2 lda n doubles, images and O(n)
 * vectors) plus, for gradient calls, ONE more lda x n slab (S_b; H_b lies over R_b); per call three padded block slabs and
 * the tile images of the chunk in flight, and O(total groups) words of terms, status and tables.
 * With profiling on, agp_last_stage_ms reports whole-batch times under the indices of agp_logo_nll_gradient: 0 gram (and
 * the pad launch), 1 factor, 2 alpha and R, 6 R^T R, 8 the mirror, the group blocks, the sums, u and H, 9 the products
 * H C^T, 7 the contraction; stages a call does not run report 0. */
AGP_API int agp_logo_nll_gradient_batch(agp_context *ctx, int count,
                                        const agp_kernel *const *kernels, const agp_features *const *features,
                                        const double *y, int64_t ldy,
                                        const double *y_var, int64_t ldv,
                                        const int64_t *n_groups,
                                        const int64_t *const *offsets, const int64_t *const *indices,
                                        int predict_type,
                                        const int *n_slots,
                                        const agp_gradient_slot *const *slots,
                                        const double *const *tangents, int64_t ldt,
                                        double *logo_nll,
                                        double *grad_logo_nll, int64_t ldg,
                                        double *mean_weights, int64_t ldw,
                                        double *const *group_nll,
                                        int *status);

/* ---- solve (CovarianceRepresentation::solve, gp.hpp:42-45,68,96,111) ----- */
/* out = K^-1 rhs; rhs/out column-major n x nrhs (ld = n), at `location`. */
AGP_API int agp_solve(agp_context *ctx, const agp_fit *fit, const double *rhs,
              int64_t nrhs, double *out, int location);

/* ---- dense-matrix factor (CovarianceRepresentation from a matrix) ----------- */
/* Eigen::SerializableLDLT(const MatrixXd &) (src/eigen/serializable_ldlt.hpp:27)
 * as used by update() (models/gp.hpp:393), BlockSymmetric (linalg/block_symmetric.hpp:
 * 46-60) and the dense negative_log_likelihood: factor a symmetric positive-definite
 * matrix given by ONE triangle (column-major, ld, at `location`): uplo = 0 reads the
 * lower triangle, uplo = 1 the upper one (a row-major array handed over as it is).  The handle
 * supports agp_solve, agp_fit_log_determinant, agp_fit_inverse_diagonal,
 * agp_fit_download_factor, agp_fit_size, agp_fit_failed_pivot; it has no training
 * features (agp_predict_* and agp_loo_marginal reject it). */
AGP_API int agp_factor_create(agp_context *ctx, const double *K, int64_t n, int64_t ld,
                      int uplo, int location, agp_fit **out);
/* negative_log_likelihood(deviation, covariance) (src/evaluation/likelihood.hpp:53-66):
 * 0.5 (log|K| + dev^T K^-1 dev + n log 2 pi); the univariate shortcut (:57-60) included. */
AGP_API int agp_nll_dense(agp_context *ctx, const double *deviation, const double *K,
                  int64_t n, int64_t ld, int uplo, int location, double *out);

/* ---- scoring a joint prediction (src/evaluation/prediction_metrics.hpp) ------------------------------------
 * The reference scores a JointDistribution against held-out truth on the host; these entries do it where
 * agp_predict_joint (out_location = AGP_DEVICE) leaves the m x m covariance.  Every ARRAY argument lives at `location`,
 * every SCALAR result goes to host memory, and nothing is written when the status is not AGP_OK.  All reductions have a
 * fixed order and use no floating-point atomics: two identical calls return identical bits.
 *
 * agp_standard_normal: the generator behind the draws, m x n_columns standard normals, entry (i, j) = column
 *   first_column + j of an unbounded matrix that depends on `seed` alone - not on the shape of the call.  Philox4x32-10
 *   (Salmon et al., SC'11) with key = (low, high) word of seed and counter = (row, column, 0, 0) gives r0 .. r3;
 *   u1 = (((r0 | r1 << 32) >> 11) + 0.5) 2^-53, u2 likewise from (r2, r3), z = sqrt(-2 ln u1) cos(2 pi u2) in fp64.  It
 *   replaces std::normal_distribution over std::default_random_engine in detail::draw_mvn (:208-214), whose stream is
 *   NOT reproduced.  m and first_column + n_columns must fit 32 bits.
 * agp_draw_mvn: detail::draw_mvn (:200-217): out (m x n_draws, ldo) = mean 1^T + L Z, L the lower factor of `fit`
 *   (m = agp_fit_size), on the fp64 MFMA; only the lower triangle of the factor is used.  z == NULL: Z = columns
 *   0 .. n_draws - 1 of agp_standard_normal(seed); otherwise Z is the caller's m x n_draws matrix (ldz) and seed is unused.
 *   `fit` is any agp_fit without phantom rows, normally an agp_factor_create of a joint covariance; a fit grown by
 *   agp_fit_update returns AGP_ERR_UNSUPPORTED.  The reference draws through its pivoted L D L^T, P L D^1/2 z; this
 *   library draws through L L^T: the distribution is the same, the sample belonging to ONE z is not - which, with the
 *   different random stream, is why z can be supplied.
 * agp_energy_score: score::energy_score (:387-435), ES = E||X - y|| - 0.5 E||X - X'|| by Monte Carlo.  cov (m x m, ldc,
 *   LOWER triangle read) + diag(truth_var) (truth_var may be NULL) is factored on a copy with the LL^T of
 *   agp_factor_create (the reference: Eigen::LDLT): AGP_ERR_NOT_POSITIVE_DEFINITE for a pivot <= 0, AGP_ERR_NAN_INPUT
 *   for a NaN in the triangle.  k = num_samples / 2 + 1 (:265); sample set A = mean + L z_j for the normal columns
 *   j = 0 .. k - 1 followed by its antithetic half mean - L z_j (:258-277), set B the same from columns k .. 2 k - 1;
 *   *out = max(0, 0.5 (mean_err_norms(A) + mean_err_norms(B)) - 0.5 pairwise_errors_paired(A, B)) (:221-256, :415-421;
 *   weights - m values, NULL = ones - enter the first term unsquared and the second squared, as there).  A NaN result
 *   is returned as NaN.  z == NULL: the normals are agp_standard_normal(seed); otherwise the caller's m x 2 k matrix
 *   (ldz).  num_samples <= 1, m <= 0, ldc < m or ldz < m: AGP_ERR_INVALID_ARGUMENT.  Scratch besides the factor's copy
 *   is O(m k).
 * agp_variogram_score: score::variogram_score (:465-520),
 *   sum_{i < j} w_ij (|y_i - y_j|^p - E|N(mu_j - mu_i, sigma_ij^2)|^p)^2, sigma_ij = sqrt(c_ii + s_i + c_jj + s_j - 2 c_ij),
 *   order p = 1 (madogram, detail::expected_abs_normal_1, :287-301) or 2 (variogram, mu^2 + sigma^2); any other order is
 *   AGP_ERR_INVALID_ARGUMENT.  One pass over the pairs the reference's loop visits: the diagonal and the strict UPPER
 *   triangle of cov (ldc) and the strict upper triangle of weights (m x m, ldw; NULL = ones) are all that is read of
 *   them.  s = truth_var (NULL = none) joins the diagonal inside the kernel (:513-520).  m = 1 gives 0.
 * agp_crps_normal: score::crps_normal (:349-364) elementwise over n triples, its NaN (non-finite argument) and
 *   sigma <= 0 (absolute error) branches included. */
AGP_API int agp_standard_normal(agp_context *ctx, uint64_t seed, int64_t m, int64_t first_column, int64_t n_columns,
                                double *out, int64_t ldo, int location);
AGP_API int agp_draw_mvn(agp_context *ctx, const agp_fit *fit, const double *mean, int64_t n_draws, uint64_t seed,
                         const double *z, int64_t ldz, double *out, int64_t ldo, int location);
AGP_API int agp_energy_score(agp_context *ctx, const double *mean, const double *cov, int64_t ldc, int64_t m,
                             const double *truth, const double *truth_var, const double *weights, uint64_t seed,
                             int64_t num_samples, const double *z, int64_t ldz, int location, double *out);
AGP_API int agp_variogram_score(agp_context *ctx, const double *mean, const double *cov, int64_t ldc, int64_t m,
                                const double *truth, const double *truth_var, const double *weights, int64_t ldw, int order,
                                int location, double *out);
AGP_API int agp_crps_normal(agp_context *ctx, const double *mu, const double *sigma, const double *y, int64_t n, double *out,
                            int location);

/* ---- update: condition a fit on further observations without refitting ------------------------------------
 * FitModel::update -> GaussianProcessBase::_update_impl (src/models/gp.hpp:384-414) with BlockSymmetric
 * (src/linalg/block_symmetric.hpp:46-115).  The reference keeps the old solver plus Ai_B = A^-1 B and the factor of the
 * Schur complement S = C - B^T A^-1 B; here the same algebra extends the RESIDENT factor by one block row,
 *     [[A, B], [B^T, C]] = [[L, 0], [V^T, L_S]] [[L, 0], [V^T, L_S]]^T,   V = L^-1 B,  L_S L_S^T = S,
 * all on the device (triangular solve and SYRK on MFMA, LL^T of the m x m block, one back substitution).  As in the
 * reference: cross = k(train_features, features) and prior = k(features, features) on PLAIN features (gp.hpp:388-396:
 * no Measurement<> wrapper), targets.covariance on the diagonal of the new block, and
 * information = [old - Ai_B S^-1 delta; S^-1 delta].
 *   old      a fit made by agp_fit_create / agp_fit_update on this context (it stays valid)
 *   x_new    the m further features (same dim / scale columns / id convention as the training features)
 *   y_new    their targets with the mean function removed, y_var_new their variances or NULL, at x_new->location
 *   out      a NEW fit of old + m observations for agp_predict_*, agp_solve, agp_fit_download_*, agp_fit_update;
 *            cross-validation entry points reject it (AGP_ERR_UNSUPPORTED)
 *   information  (optional, host) all agp_fit_size(*out) entries: the old observations first, then the new ones */
AGP_API int agp_fit_update(agp_context *ctx, const agp_kernel *k, const agp_fit *old, const agp_features *x_new, const double *y_new,
                   const double *y_var_new, agp_fit **out, double *information, double *log_det);

/* agp_fit_update for `count` fits of one padded size in lock step: problem b computes what
 * agp_fit_update(ctx, kernels[b], olds[b], x_new[b], ...) computes - the same algebra, the plain-feature semantics of
 * cross and prior, the phantom rows when the old size is not a multiple of 128, log determinant = old + 2 sum log
 * diag(L_S) - but every stage is ONE launch or launch chain for the whole batch, the grown fits are slices of ONE device
 * allocation, and the call synchronises twice at most: once behind the uploads of host-resident inputs and once at its
 * end, where status words and log sums come down together.  What a caller does who keeps many small models and
 * conditions each on every new epoch of observations.
 *   olds[b]          plain fp64 fits of this context with training features and forward-substituted targets, all of one
 *                    padded size (agp_fit_padded_size); their real rows and phantom ranges may differ (the fits of an
 *                    agp_fit_create_batch_ragged call).  They need NOT lie at one stride
 *                    or come from one call (their factors, tile images, z and features are gathered through a descriptor
 *                    table); they stay valid and are not modified
 *   x_new[b]         the m > 0 further features of problem b: one m and one location for all problems, dim / scale columns
 *                    / id convention as olds[b] (dim may differ between problems)
 *   y_new, ldy       their targets with the mean function removed, m x count column-major at that location (ldy = 0: one
 *                    vector shared by all); y_var_new, ldv likewise, or NULL
 *   out[b]           an ordinary agp_fit of old + m observations (agp_predict_*, agp_solve, agp_fit_download_*,
 *                    agp_fit_update, agp_fit_update_batch again).  The grown fits of one call lie at constant strides in one
 *                    allocation that is released with the last of them, and reference no memory of the old fits;
 *                    agp_predict_batch runs them in lock step.  Grown fit b carries the phantom ranges of olds[b] plus the
 *                    pad from the old padded size to the next multiple of 128
 *   information, ldi (optional, host) the real rows of every good problem, old observations first: column b gets
 *                    agp_fit_size(olds[b]) + m values, ldi >= the largest of those; log_det[b] (optional, host)
 *   status[b]        AGP_OK / AGP_ERR_NAN_INPUT / AGP_ERR_NOT_POSITIVE_DEFINITE per problem; a failed problem leaves the
 *                    others and its own column of `information` untouched.  A problem that is not positive definite reports
 *                    the pivot through its handle like agp_fit_update (real rows of the old fit + local pivot); a NaN
 *                    problem gets a handle that only carries its status, as in agp_fit_create_batch
 * The return value is about the call as a whole: when it is not AGP_OK every out[b] is NULL and nothing is left to
 * destroy.  A fit without forward-substituted targets: AGP_ERR_UNSUPPORTED.  A mixed-precision or failed fit, a fit of
 * another context, any mismatch, count outside 1 .. 65535, ldy / ldv / ldi too short: AGP_ERR_INVALID_ARGUMENT.  A
 * rejected call writes nothing, out and status included.  No float atomics, fixed-order reductions: two identical calls
 * are bit-identical, and no problem's bits depend on its neighbours (but for the tile shape of the batched MFMA products,
 * which follows the number of tiles of the whole launch, as agp_predict_batch documents).  With profiling on,
 * agp_last_stage_ms reports 0 grow, cross covariance and V, 1 Schur complement and its factor, 2 back substitution. */
AGP_API int agp_fit_update_batch(agp_context *ctx, int count, const agp_kernel *const *kernels, const agp_fit *const *olds,
                                 const agp_features *const *x_new, const double *y_new, int64_t ldy,
                                 const double *y_var_new, int64_t ldv, agp_fit **out, double *information, int64_t ldi,
                                 double *log_det, int *status);

/* ---- leave-one-out fast path (the tuner's LeaveOneOutLikelihood objective; the metric and its gradient: agp_loo_nll_gradient) --- */
/* diag(K^-1): SerializableLDLT::inverse_diagonal (src/eigen/serializable_ldlt.hpp:
 * 137-199: R = L^-1, then the squared column norms of R).  out: n doubles. */
AGP_API int agp_fit_inverse_diagonal(agp_context *ctx, const agp_fit *fit, double *out,
                             int out_location);
/* Leave-one-out predictive marginals, all n at once: held_out_predictions with
 * singleton groups (src/evaluation/cross_validation_utils.hpp:165-232) ==
 * leave_one_out_conditional (:138-163, GPML eq. 5.12):
 *   variance_i = 1 / (K^-1)_ii ,  mean_i = y_i - information_i / (K^-1)_ii.
 * y = the target means as passed to the fit's dataset (n doubles at `location`);
 * mean / variance: n doubles each at `location`. */
AGP_API int agp_loo_marginal(agp_context *ctx, const agp_fit *fit, const double *y,
                     double *mean, double *variance, int location);

/* Leave-one-GROUP-out.  Groups are index sets into the training data: group g is
 * indices[offsets[g] .. offsets[g + 1]) (offsets has n_groups + 1 entries, offsets[0] = 0; both
 * arrays live on the host).
 *
 * agp_fit_inverse_blocks = SerializableLDLT::inverse_blocks
 * (include/albatross/src/eigen/serializable_ldlt.hpp:137-179): blocks receives, concatenated, the
 * column-major |g| x |g| matrices (K^-1)[I_g, I_g].
 *
 * agp_held_out_predictions = details::held_out_predictions
 * (include/albatross/src/evaluation/cross_validation_utils.hpp:165-232; called by
 * gp_cross_validated_predictions, models/gp.hpp:465-482): for every group the prediction of its
 * own targets from all OTHER groups, without refitting:
 *   mean_g = y_g - B_g^-1 information_g,  marginal variance = diag(B_g^-1),  joint = B_g^-1,
 *   B_g = (K^-1)[I_g, I_g].
 * mean / variance (variance may be NULL) are written in the order of `indices`; joint (may be NULL)
 * receives the concatenated column-major blocks.  y, mean, variance, joint live at `location`. */
AGP_API int agp_fit_inverse_blocks(agp_context *ctx, const agp_fit *fit, int64_t n_groups, const int64_t *offsets,
                           const int64_t *indices, double *blocks, int out_location);
AGP_API int agp_held_out_predictions(agp_context *ctx, const agp_fit *fit, const double *y, int64_t n_groups,
                             const int64_t *offsets, const int64_t *indices, double *mean, double *variance,
                             double *joint, int location);

/* ---- pivoted L D L^T ------------------------------------------------------------------------
 * Eigen::LDLT<MatrixXd, Lower> as albatross uses it through SerializableLDLT
 * (include/albatross/src/eigen/serializable_ldlt.hpp:27; evaluation/likelihood.hpp:63,
 * covariance_functions/representations.hpp:64-96, models/gp.hpp:148,393): P A P^T = L D L^T with
 * diagonal pivoting, for symmetric matrices that are only SEMI-definite or too ill-conditioned for
 * the un-pivoted LL^T of agp_factor_create.  The factorisation follows the reference's unblocked
 * left-looking algorithm operation by operation (L, D and the transpositions are bit-identical to
 * the CPU restatement); it is a correctness path, level-2 bound, meant for moderate n.
 *   agp_ldlt_create   K as in agp_factor_create (one triangle, uplo); *success (optional) = Eigen's
 *                     info() == Success (0: a non-zero pivot followed a zero one, NumericalIssue)
 *   agp_ldlt_solve    LDLT::solve: P^T L^-T D^+ L^-1 P rhs, D^+ zeroing the pivots that are not above
 *                     the smallest normal number; rhs / out are n x nrhs column-major at `location`
 *   agp_ldlt_vector_d / _transpositions / _download   vectorD(), transpositionsP(), matrixLDLT() (host) */
typedef struct agp_ldlt agp_ldlt;
AGP_API int agp_ldlt_create(agp_context *ctx, const double *K, int64_t n, int64_t ld, int uplo, int location,
                    agp_ldlt **out, int *success);
AGP_API void agp_ldlt_destroy(agp_ldlt *ldlt);
AGP_API int64_t agp_ldlt_size(const agp_ldlt *ldlt);
AGP_API int agp_ldlt_solve(agp_context *ctx, const agp_ldlt *ldlt, const double *rhs, int64_t nrhs, double *out,
                   int location);
/* SerializableLDLT::sqrt_solve (serializable_ldlt.hpp:99-109): D^-1/2 L^-1 P rhs, D^-1/2 zero where D_i <= 0 (:58-69);
 * out^T out = rhs^T A^-1 rhs.  rhs / out n x nrhs column-major at `location`. */
AGP_API int agp_ldlt_sqrt_solve(agp_context *ctx, const agp_ldlt *ldlt, const double *rhs, int64_t nrhs, double *out,
                        int location);
AGP_API int agp_ldlt_vector_d(const agp_ldlt *ldlt, double *d);
AGP_API int agp_ldlt_transpositions(const agp_ldlt *ldlt, int64_t *tr);
AGP_API int agp_ldlt_download(agp_context *ctx, const agp_ldlt *ldlt, double *packed, int64_t ld);

/* ---- greedy pivoted Cholesky of a covariance ------------------------------------------------
 * The partial Cholesky factorisation of K = k(x, x) with diagonal pivoting, K evaluated column by column and never
 * stored: greedy conditional-variance selection (every step picks the point whose prior variance is least explained
 * by the points chosen so far), the Nystrom factor K ~ L L^T and its residual trace tr(K - L L^T).  K is the matrix
 * agp_gram gives for x (is_measurement, equality ids, scale columns and metrics included), entry by entry the same bits.
 *   d_i = K_ii;  d0 = max_i d_i;  step j = 0 .. max_rank - 1:
 *     p_j = the unselected index with the largest d (the lowest index on equal values);
 *     stop with rank = j if d_{p_j} <= rel_tol d0 or d_{p_j} <= 0;
 *     L_ij = (k(x_i, x_{p_j}) - sum_{t<j} L_it L_{p_j t}) / sqrt(d_{p_j}), the sum in the order t = 0, 1, ...;
 *     d_i = max(d_i - L_ij^2, 0);  exactly: L_{p_j j} = sqrt(d_{p_j}), d_{p_j} = 0, L_ij = 0 for rows selected before.
 *   The rows of L in pivot order form a lower trapezoid with a positive diagonal.
 *   pivots         (host) max_rank entries; p_0 .. p_{rank-1} are written, the entries from rank on are not touched
 *   rank           (host) the steps carried out
 *   L, ldl         n x max_rank column-major at `location` (ldl >= n), or NULL: columns 0 .. rank - 1 are written, the
 *                  columns from rank on and the rows >= n of a padded ldl are not touched
 *   residual_diag  n values at `location`, or NULL: d after the last step
 *   trace_residual (host) or NULL: sum_i d_i, reduced in a fixed order
 * x may be host or device memory (x->location); `location` is that of L and residual_diag.
 * Status: max_rank < 1, max_rank > n, rel_tol < 0 or NaN, ldl < n with an L, a location that is neither AGP_HOST nor
 * AGP_DEVICE, a NULL pivots or rank: AGP_ERR_INVALID_ARGUMENT, nothing written.  A NaN on the diagonal or in a computed
 * column (a NaN coordinate): AGP_ERR_NAN_INPUT, pivots and rank not written (an L on the device may hold the columns
 * computed up to there).
 * One launch per step: a thread per two rows reads L coalesced (the kernel is bound by the n j doubles of L that step
 * j reads: n max_rank^2 / 2 doubles in all); the argmax of a step is left as one partial per workgroup and reduced by
 * every workgroup of the next launch; the stop decision is taken on the device and the host looks at it once per 64
 * steps with the next 64 queued, otherwise the call waits once, at its end.  No float atomics and a fixed order of
 * every sum: two identical calls return identical bits.  Scratch beyond the caller's L: about 1.2 n + max_rank doubles, plus an
 * n x max_rank slab on the device when L is NULL or on the host.  With profiling on, agp_last_stage_ms reports the
 * chain of step launches under stage 10. */
AGP_API int agp_pivoted_cholesky(agp_context *ctx, const agp_kernel *k, const agp_features *x, int64_t max_rank, double rel_tol,
                                 int64_t *pivots, int64_t *rank, double *L, int64_t ldl, double *residual_diag, int location,
                                 double *trace_residual);

/* ---- the covariance times a block of vectors, without the matrix ---------------------------
 *   out[:, c] = (k(x, x) + diag(y_var)) V[:, c],   c = 0 .. nrhs - 1
 * with K evaluated pair by pair inside the product and never stored (memory O(n nrhs) instead of O(n^2)): the building
 * block of a matrix-free solve.  K is the matrix agp_gram(ctx, k, x, NULL, ...) gives (is_measurement, equality ids, scale
 * columns and all metrics included), entry by entry the same bits; y_var is added to the diagonal entry before the
 * product.  Every covariance tree is served: the radial fast path (dim <= 3), the sum-of-products evaluator, the postfix
 * interpreter, chosen as agp_gram chooses.
 *   y_var     n values at x->location, or NULL (zeros)
 *   V, ldv    n x nrhs column-major at `location`, ldv >= n
 *   out, ldo  n x nrhs column-major at `location`, ldo >= n, not overlapping V: rows >= n of a padded ldo and everything
 *             beyond nrhs columns are not touched
 * x may be host or device memory (x->location).  Any nrhs >= 1: the right-hand sides are served in chunks of at most
 * AGP_MATVEC_MAX_RHS inside the call (16, then 4 or 1 for the rest), each entry K_ij evaluated once per chunk.
 * Status: nrhs < 1, ldv < n, ldo < n, a location that is neither AGP_HOST nor AGP_DEVICE, a NULL V or out:
 * AGP_ERR_INVALID_ARGUMENT, nothing written.  A NaN entry of K (a NaN coordinate): AGP_ERR_NAN_INPUT; a host `out` is not
 * written, a device `out` holds the NaNs.  n == 0: AGP_OK.
 * A thread owns one row and the accumulators of a chunk; the column points and their rows of V pass through LDS in tiles
 * of 64, read as broadcasts.  For n below 262144 the column range is split into S slices over a second grid dimension
 * (S depends on n alone) and a second launch adds the S partial sums of an entry in slice order.  No float atomics and a
 * fixed order of every sum: two identical calls return identical bits.  Scratch: S * 16 * n doubles when S > 1, plus
 * copies of V and out (2 n nrhs doubles) for host arrays. */
#define AGP_MATVEC_MAX_RHS 16
AGP_API int agp_gram_matvec(agp_context *ctx, const agp_kernel *k, const agp_features *x, const double *y_var, const double *V,
                            int64_t ldv, int64_t nrhs, double *out, int64_t ldo, int location);

/* ---- tangent bilinear forms without the matrix ----------------------------------------------
 *   forms[c + p * ldf] = sum_i sum_j U[i, c] (dk(x_i, x_j) / dslot_p) V[j, c]      c < ncols, p < n_slots
 * with the tangent matrix dk(x, x) / dslot_p evaluated pair by pair inside the product, never stored, and no n x n weight
 * either: the contraction of agp_nll_gradient against VECTORS.  x is taken as given (is_measurement decides what a
 * measurement_only term contributes, exactly as for agp_gram_matvec); y_var carries no parameter and is not an argument.
 *   slots, tangents, ldt   as for agp_nll_gradient: n_slots <= AGP_MAX_GRADIENT_SLOTS (node, param) pairs, and for the
 *                          AGP_OP_SCALING slots the n x (columns) tangent matrix at `location`, ldt >= n
 *   U, ldu, V, ldv         n x ncols column-major at `location`, ldu, ldv >= n
 *   forms, ldf             HOST memory, ldf >= ncols; nothing beyond ncols x n_slots is touched
 * ncols == 0 or n_slots == 0: AGP_OK, nothing written.  A malformed argument or slot table: AGP_ERR_INVALID_ARGUMENT,
 * nothing written.  A NaN tangent (a NaN coordinate): AGP_ERR_NAN_INPUT, nothing written.
 * The tangent matrix is symmetric: a pair i > j is evaluated once, as agp_nll_gradient evaluates it, and applied with the
 * weight U_ic V_jc + V_ic U_jc, the diagonal once.  A lane owns a row and the accumulators of a chunk of at most
 * AGP_TANGENT_FORMS_MAX_PAIRS column pairs (8, then 4 or 1 for the rest) times 4 slots; one evaluation of a pair's
 * tangents serves the whole chunk.  A workgroup walks the column tiles of row blocks b and (blocks - 1 - b) - together the
 * same length for every b - or a fixed slice of them, keeps its sums in registers and writes one block of them; a second
 * launch adds the blocks in a fixed order.  No float atomics: two identical calls return identical bits.  Scratch: 32
 * doubles per workgroup (about a thousand workgroups), plus copies of U, V and the tangent columns for host arrays -
 * never a table per tile of the matrix. */
#define AGP_TANGENT_FORMS_MAX_PAIRS 8
AGP_API int agp_gram_tangent_forms(agp_context *ctx, const agp_kernel *k, const agp_features *x, int n_slots,
                                   const agp_gradient_slot *slots, const double *tangents, int64_t ldt, const double *U, int64_t ldu,
                                   const double *V, int64_t ldv, int64_t ncols, double *forms, int64_t ldf, int location);

/* ---- matrix-free fit: preconditioned conjugate gradients around agp_gram_matvec --------------
 * The exact fit that never forms A = k(x, x) + diag(y_var) (x as measurements, exactly the matrix agp_fit_create
 * factors; the predictions see the training features as agp_predict_* do): information = A^-1 y by conjugate gradients whose products
 * are agp_gram_matvec launches, preconditioned by the greedy pivoted Cholesky factor of A.  Memory is O(n (m + t)) for a
 * preconditioner of rank m and t right-hand sides in flight, instead of O(n^2).
 *   (L, m, trace) = agp_pivoted_cholesky of A with max_rank = min(precond_rank, n), rel_tol = precond_rel_tol (m may come
 *   out below precond_rank: duplicated points);  P = L L^T + delta I,  delta = max(trace / (n - m), 1e-8 max_i A_ii), the
 *   floor alone when m = n;  P^-1 r = (r - L (delta I + L^T L)^-1 L^T r) / delta, with L^T L formed once on the fp64 GEMM
 *   and its m x m matrix factored by the dense LL^T.  precond_rank = 0: P = delta I with delta the mean of diag(A), plain CG.
 * The right-hand sides of a call run INDEPENDENT recurrences in chunks of at most AGP_MATVEC_MAX_RHS that share each
 * product launch (not block CG).  A right-hand side stops at the first iteration with ||r||_2 <= tolerance ||b||_2 (r the
 * recurrence's residual) and is frozen from then on; a zero right-hand side returns zeros after 0 iterations.  The scalars
 * of the recurrences live on the device; the host looks at the stop marks once per 8 iterations with the next 8 queued.
 *   options       precond_rank >= 0, precond_rel_tol >= 0, tolerance > 0, max_iterations >= 1
 *   y, y_var      n values at x->location; y_var may be NULL (zeros)
 *   information   n doubles (host), may be NULL;  iterations / residual (host, may be NULL): the iterations carried out and
 *                 the final ||r|| / ||y|| of the recurrence - written whenever the iteration ran, also on
 *                 AGP_ERR_NOT_CONVERGED
 * The handle owns a copy of the features, y_var, the information vector, L, the factor of delta I + L^T L and delta; it
 * belongs to its context and must be destroyed before it.
 * Status: a malformed argument AGP_ERR_INVALID_ARGUMENT, nothing written.  A_ii <= 0 for some i (before any iteration) or
 * p^T A p <= 0 in an active recurrence: AGP_ERR_NOT_POSITIVE_DEFINITE.  A NaN coordinate, target or variance:
 * AGP_ERR_NAN_INPUT.  max_iterations reached with a right-hand side still active: AGP_ERR_NOT_CONVERGED (no handle, no
 * solution).  No float atomics, a fixed order of every sum: two identical calls return identical bits, iteration counts
 * included.  Scratch of a solve: 4 n t doubles for the recurrences, m t for the preconditioner, plus that of
 * agp_gram_matvec.  With profiling on, agp_last_stage_ms reports the preconditioner build under stage 11 and the
 * conjugate-gradient chain under stage 12.
 * agp_iterative_solve: out = A^-1 rhs for nrhs >= 1 right-hand sides (n x nrhs column-major at `location`, ldr, ldo >= n)
 *   at the fit's tolerance and max_iterations; iterations / residual: nrhs host values each, may be NULL.
 * agp_iterative_predict_mean: mean_j = sum_i k(x_i, xs_j) information_i, the launches of agp_predict_mean.
 * agp_iterative_predict_marginal: also variance_j = k(xs_j, xs_j) - k_j^T A^-1 k_j; the cross covariances come from the
 *   Gram kernels in slices of 16 test points, each slice solved by the same conjugate gradients (its status is returned).
 * agp_iterative_nll_gradient: the gradient of the negative log-likelihood with respect to parameter slots, WITHOUT its
 *   value (agp_iterative_nll below returns both from one chain of solves; this entry keeps its Rademacher probes).  With A, alpha = information, the preconditioner, tolerance and max_iterations those of `fit`, dA_p = dA / dslot_p:
 *     dNLL / dslot_p = 1/2 tr(A^-1 dA_p) - 1/2 alpha^T dA_p alpha
 *   The second term is exact (one agp_gram_tangent_forms column pair U = V = alpha).  The trace is estimated from t =
 *   n_probes probe vectors z_c:  w_c = A^-1 z_c by the fit's conjugate gradients in chunks of AGP_MATVEC_MAX_RHS,
 *     s_cp = w_c^T dA_p z_c (agp_gram_tangent_forms on the features as measurements),  tau_p = mean_c s_cp,
 *     grad_nll[p] = 1/2 tau_p - 1/2 alpha^T dA_p alpha,
 *     grad_stderr[p] = 1/2 sqrt(sum_c (s_cp - tau_p)^2 / (t (t - 1)))   (NaN when t = 1).
 *   probes == NULL: Rademacher probes, z_ic = +1 if entry (i, c) of agp_standard_normal(seed) is >= 0, else -1; column c
 *     depends on (seed, c) alone, and the probes are generated chunk by chunk (never n x t).
 *   probes != NULL: the caller's n x t matrix at `location` (ldp >= n), used as is.  The estimator is unbiased when
 *     E z z^T = I, and EXACT for Z = sqrt(n) I with t = n.
 *   slots, tangents, ldt   as for agp_nll_gradient (the covariance function is the fit's); tangents at `location`
 *   grad_nll, grad_stderr  n_slots host values each;  samples (host, t x n_slots column-major at lds >= t, may be NULL): s_cp
 *   iterations, residual   t host values each, may be NULL
 *   Status: invalid slots, n_probes <= 0, ldp < n, lds < n_probes: AGP_ERR_INVALID_ARGUMENT.  A probe solve that runs out of
 *   iterations: AGP_ERR_NOT_CONVERGED with iterations / residual filled as far as the solves went and the gradient outputs
 *   untouched.  NaN and not-positive-definite as agp_iterative_solve reports them.  The handle is not modified.  Two
 *   identical calls return identical bits.  Scratch: 2 n 16 doubles of probes and solutions plus that of a solve.  With
 *   profiling on, the probe solves report under stage 12 and the forms (the alpha term included) under stage 13.
 * agp_iterative_nll: the VALUE of the negative log-likelihood by stochastic Lanczos quadrature, and - from the same
 *   solves - its gradient.  With P = L L^T + delta I the fit's preconditioner (rank m) and M = P^-1/2 A P^-1/2:
 *     log det A = log det P + tr log M,   log det P = (n - m) log delta + log det(delta I + L^T L)   (m = 0: n log delta)
 *   the second term of log det P from the factor the fit holds.  For z ~ N(0, P), u = P^-1/2 z is standard normal and
 *   E[u^T log(M) u] = tr log M.  The fit's conjugate gradients on A w = z are Lanczos on M started at u: with a_k, b_k the
 *   alpha and beta of iteration k (b_0 = 0), which the solve keeps per column instead of overwriting them,
 *     T[k, k] = 1 / a_k + b_k / a_{k-1},   T[k-1, k] = T[k, k-1] = sqrt(b_k) / a_{k-1}     (k < the column's iterations)
 *     s_c = (z_c^T P^-1 z_c) sum_i V[0, i]^2 log lambda_i,   (lambda, V) the eigendecomposition of T   (Gauss quadrature)
 *   taken on the host by the implicit QL iteration carrying the first row of V alone, O(k^2) per column, without
 *   reorthogonalisation.  Then
 *     log_det = log det P + mean_c s_c,   its standard error e = sqrt(sum_c (s_c - mean)^2 / (t (t - 1)))  (NaN when t = 1),
 *     nll = 1/2 alpha^T A alpha + 1/2 log_det + n/2 log 2 pi,   nll_stderr = e / 2,
 *   the data term from one agp_gram_matvec of alpha and one dot in a fixed order (the handle does not keep y).
 *   probes == NULL: z_c = L g1_c + sqrt(delta) g2_c with g2_c column c of agp_standard_normal(seed) on n rows and g1_c
 *     column c of agp_standard_normal(seed ^ 0x9E3779B97F4A7C15) on m rows; column c depends on (seed, c) alone and the
 *     probes are generated chunk by chunk (never n x t).  The better the preconditioner, the nearer M is to I and the
 *     smaller the variance: at rank 0 the estimator is the plain one on A / delta.
 *   probes != NULL: the caller's n x t matrix at `location` (ldp >= n), used as z as is.  The estimate is unbiased when
 *     E z z^T = P, and EXACT for Z = sqrt(t) [L | sqrt(delta) I] with t = n + m.
 *   quadrature_tolerance: the relative residual at which a probe's recurrence stops when n_slots == 0; <= 0: the fit's.  A
 *     looser one shortens T; the quadrature converges about twice as fast as the solve, and what it costs is the
 *     caller's to judge.  With n_slots > 0 the solves run at the fit's tolerance whatever it says.
 *   n_slots > 0: also the gradient.  With w_c = A^-1 z_c (the solve) and v_c = P^-1 z_c (one preconditioner application),
 *     E[w^T dA_p v] = tr(A^-1 dA_p):  g_cp = w_c^T dA_p v_c (agp_gram_tangent_forms),
 *     grad_nll[p] = 1/2 mean_c g_cp - 1/2 alpha^T dA_p alpha,   grad_stderr[p] = 1/2 sqrt(sum_c (g_cp - mean)^2 / (t (t - 1))).
 *     slots, tangents, ldt as for agp_iterative_nll_gradient; n_slots == 0: the value alone, the four are not read.
 *   nll, nll_stderr, log_det   one host double each, any may be NULL;  log_det_samples (host, t values, may be NULL): s_c
 *   grad_nll, grad_stderr      n_slots host values each;  grad_samples (host, t x n_slots at lds >= t, may be NULL): g_cp
 *   iterations, residual       t host values each, may be NULL
 *   Status: as agp_iterative_nll_gradient; a probe solve that runs out of iterations: AGP_ERR_NOT_CONVERGED with
 *   iterations / residual filled as far as the solves went and every other output untouched.  A T with an eigenvalue <= 0:
 *   AGP_ERR_NOT_POSITIVE_DEFINITE.  The handle is not modified; agp_iterative_solve and agp_iterative_nll_gradient return
 *   the bits they returned before.  No float atomics, a fixed order of every sum: two identical calls return identical
 *   bits.  Scratch: 3 n 16 doubles (2 n 16 for the value alone) plus that of a solve, and 16 (1 + 2 max_iterations) doubles
 *   of coefficients.  With profiling on: the probe solves under stage 12, the forms under 13, and the probes' generation, the
 *   quadrature (host time) and log det P under 14.
 * Out of scope, by design: joint predictions, variance-reduced trace estimators, gradients of the leave-one-out metrics,
 * LinearCombination features, the sharded and the mixed-precision path - the dense entry points serve them up to the n
 * their memory allows. */
typedef struct {
  int64_t precond_rank;
  double precond_rel_tol;
  double tolerance;
  int max_iterations;
} agp_iterative_options;
typedef struct agp_iterative_fit agp_iterative_fit;
AGP_API int agp_iterative_fit_create(agp_context *ctx, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                                     const agp_iterative_options *options, agp_iterative_fit **out, double *information,
                                     int *iterations, double *residual);
AGP_API void agp_iterative_fit_destroy(agp_iterative_fit *fit);
AGP_API int64_t agp_iterative_fit_size(const agp_iterative_fit *fit);
AGP_API int64_t agp_iterative_fit_preconditioner_rank(const agp_iterative_fit *fit);
AGP_API int agp_iterative_fit_download_information(agp_context *ctx, const agp_iterative_fit *fit, double *information);
AGP_API int agp_iterative_solve(agp_context *ctx, const agp_iterative_fit *fit, const double *rhs, int64_t ldr, int64_t nrhs, double *out,
                                int64_t ldo, int location, int *iterations, double *residual);
AGP_API int agp_iterative_predict_mean(agp_context *ctx, const agp_kernel *k, const agp_iterative_fit *fit, const agp_features *xs,
                                       double *mean, int location);
AGP_API int agp_iterative_predict_marginal(agp_context *ctx, const agp_kernel *k, const agp_iterative_fit *fit, const agp_features *xs,
                                           double *mean, double *variance, int location);
AGP_API int agp_iterative_nll_gradient(agp_context *ctx, const agp_iterative_fit *fit, int n_slots, const agp_gradient_slot *slots,
                                       const double *tangents, int64_t ldt, int64_t n_probes, uint64_t seed, const double *probes,
                                       int64_t ldp, int location, double *grad_nll, double *grad_stderr, double *samples, int64_t lds,
                                       int *iterations, double *residual);
AGP_API int agp_iterative_nll(agp_context *ctx, const agp_iterative_fit *fit, int64_t n_probes, uint64_t seed, const double *probes,
                              int64_t ldp, int location, double quadrature_tolerance, int n_slots, const agp_gradient_slot *slots,
                              const double *tangents, int64_t ldt, double *nll, double *nll_stderr, double *log_det,
                              double *log_det_samples, double *grad_nll, double *grad_stderr, double *grad_samples, int64_t lds,
                              int *iterations, double *residual);

/* ---- sparse Gaussian process (FITC / PITC) --------------------------------------------------
 * SparseGaussianProcessRegression, include/albatross/src/models/sparse_gp.hpp.
 *
 * agp_sparse_fit_create = _fit_impl (:354-381) on compute_internal_components (:631-706):
 *   x        the n training features ALREADY reordered group by group (reordered_inds, :645-662):
 *            independent group g = rows offsets[g] .. offsets[g + 1) (offsets: n_groups + 1 host
 *            entries, offsets[0] = 0, offsets[n_groups] = n); they are wrapped as measurements
 *            inside (as_measurements, :649-650)
 *   y, y_var target means / variances (or NULL) in the same order, at x->location; y is used as
 *            given (the reference copies y before it removes the mean function, :664-668)
 *   u        the m inducing features (the InducingPointStrategy's result, :358-360)
 *   nuggets  measurement_nugget on every diagonal of A (:692-696), inducing_nugget on K_uu (:676-677)
 * The handle keeps what prediction needs (Fit<SparseGPFit>: inducing features, the K_uu factor,
 * the factor of Sigma^-1 = K_uu + K_uf A^-1 K_fu, the information vector).  information (m doubles,
 * host) and nll (= -log_likelihood, :524-596, without parameter priors) are optional outputs.
 * out may be NULL (only nll / information wanted); agp_sparse_nll is that call.
 * Two algorithms: LL^T of K_uu and CholeskyQR2 of B (MFMA-bound, the fast path) first; where that finds K_uu or
 * B^T B not numerically positive definite - inducing points denser than the length scale, as in the reference's own
 * tests - the reference's algorithm itself runs on the device: pivoted L D L^T of K_uu (agp_ldlt_*) and the
 * column-pivoted Householder QR of B (level-2 bound, moderate m; AGP_SPARSE_PIVOTED=1 forces it; not with a
 * communicator).  Fits of the second kind are in "pivoted form" (R, P as the reference stores them) and stay so
 * under agp_sparse_fit_update.
 * Errors: AGP_ERR_NOT_POSITIVE_DEFINITE if a block of A is not numerically positive definite (the reference's
 * block LDLT would continue), AGP_ERR_NAN_INPUT. */
typedef struct agp_sparse_fit agp_sparse_fit;
AGP_API int agp_sparse_fit_create(agp_context *ctx, const agp_kernel *kernel, const agp_features *x, int64_t n_groups,
                          const int64_t *offsets, const double *y, const double *y_var, const agp_features *u,
                          double measurement_nugget, double inducing_nugget, agp_sparse_fit **out,
                          double *information, double *nll);
/* The same fit with the observations split BY GROUP over the ranks of a communicator (BASELINE
 * configs[4]: "SparseGP (PITC) ... on 8 GPUs").  The groups of a PITC / FITC model are independent given the inducing
 * points (sparse_gp.hpp:129-243), so every rank builds K_uf, P, the blocks of A and W for ITS groups alone (x, offsets, y,
 * y_var: this rank's groups only, at least one) and the m x m sums over observations - W W^T and its CholeskyQR2
 * repair - plus four m-vectors are all-reduced (2 x 8 m^2 B + O(m) per fit: 2 x 32 MiB at m = 2048).  Every rank passes
 * the same inducing points u and receives the same fit (handle, information, nll of ALL observations); predictions then
 * need no further exchange.  Collective. */
AGP_API int agp_sparse_fit_create_sharded(agp_context *ctx, agp_comm *comm, const agp_kernel *kernel, const agp_features *x,
                                  int64_t n_groups, const int64_t *offsets, const double *y, const double *y_var,
                                  const agp_features *u, double measurement_nugget, double inducing_nugget,
                                  agp_sparse_fit **out, double *information, double *nll);
AGP_API void agp_sparse_fit_destroy(agp_sparse_fit *fit);
AGP_API int64_t agp_sparse_fit_size(const agp_sparse_fit *fit); /* number of inducing points */
AGP_API int agp_sparse_fit_information(agp_context *ctx, const agp_sparse_fit *fit, double *information);
/* FitModel::update for a sparse fit: _update_impl (sparse_gp.hpp:322-371).  Further observations (grouped
 * like those of agp_sparse_fit_create; wrapped as measurements inside) are folded into `old` through
 * B = [R_old P_old^T; A^-1/2 K_fu],  y_aug = [R_old P_old^T v_old; A^-1/2 y]; the inducing points and their
 * K_uu factor are shared with `old`, which stays valid.  Returns a NEW handle in *out; information
 * (m doubles, host) is optional.  An `old` made by agp_sparse_fit_from_prediction (or by an update of one) is
 * updated with the reference's own algorithm - the column-pivoted QR of B, v = B_qr.solve(y_aug), R's diagonal
 * inflated by 1e-10 when B is rank deficient (:353-365) - and the result stays in that pivoted form. */
AGP_API int agp_sparse_fit_update(agp_context *ctx, const agp_kernel *kernel, const agp_sparse_fit *old,
                          const agp_features *x, int64_t n_groups, const int64_t *offsets, const double *y,
                          const double *y_var, double measurement_nugget, agp_sparse_fit **out,
                          double *information);
/* SparseGaussianProcessRegression::fit_from_prediction (sparse_gp.hpp:406-461), the body of
 * rebase_inducing_points (:714-725): the fit on the m inducing features z that reproduces a joint prediction made
 * AT z - mean (m) and covariance (m x m column-major, leading dimension ldc, both triangles), at `location`.
 *   train_covariance = LDLT(K_zz) (no nugget), information = train_covariance.solve(mean),
 *   C = covariance + 1e-8 I (DEFAULT_NUGGET, :20), B_z = C_ldlt.sqrt_solve(K_zz), (R, P) = QR(B_z).
 * K_zz is singular to working precision whenever z is denser than the length scale, so this path runs the
 * reference's pivoted factorisations on the device (the pivoted L D L^T of agp_ldlt_*, a column-pivoted Householder
 * QR) instead of the LL^T / CholeskyQR2 of agp_sparse_fit_create; they are level-2 bound, meant for moderate m.
 * inducing_nugget is what a later agp_sparse_fit_update adds to K_zz for P = K_zz^-1/2 K_zf (:674-685).
 * Optional outputs: information (m doubles, host), numerical_rank (B_qr->rank(), :458). */
AGP_API int agp_sparse_fit_from_prediction(agp_context *ctx, const agp_kernel *kernel, const agp_features *z,
                                   const double *mean, const double *covariance, int64_t ldc, int location,
                                   double inducing_nugget, agp_sparse_fit **out, double *information,
                                   int64_t *numerical_rank);
/* Fit<SparseGPFit>::numerical_rank: the rank of the pivoted QR for fits in pivoted form, m otherwise. */
AGP_API int64_t agp_sparse_fit_numerical_rank(const agp_sparse_fit *fit);
AGP_API int agp_sparse_nll(agp_context *ctx, const agp_kernel *kernel, const agp_features *x, int64_t n_groups,
                   const int64_t *offsets, const double *y, const double *y_var, const agp_features *u,
                   double measurement_nugget, double inducing_nugget, double *out);
/* Exact gradient of agp_sparse_nll with respect to covariance parameters and the two nuggets.  Arguments up to
 * inducing_nugget exactly as agp_sparse_nll; slots exactly as agp_nll_gradient (same validation, same
 * AGP_MAX_GRADIENT_SLOTS, derivative with respect to the raw parameter value).  An AGP_OP_SCALING slot reads its tangent
 * column at the observations from tangents_x (n values per column, leading dimension ldtx >= n, at x->location) and at
 * the inducing points from tangents_u (m values per column, ldtu >= m, at u->location).  nll (1 value, the value
 * agp_sparse_nll returns for the same arguments, bit for bit), grad_nll (n_slots values), grad_nuggets (2 values:
 * dNLL / d measurement_nugget, dNLL / d inducing_nugget; may be NULL) and alpha (n values, Kt^-1 y in the caller's grouped
 * order; may be NULL) are host memory.  The inducing points are held fixed.
 *
 * With D = diag(y_var) + measurement_nugget I, K_uu = k(u, u) + inducing_nugget I, E = K_fu K_uu^-1,
 * A = blockdiag_g(k(x_g, x_g) + D_g - (E K_uf)_gg), Kt = A + E K_uf, alpha = Kt^-1 y, G = Kt^-1 - alpha alpha^T,
 * bd(.) the group-block diagonal part and H = G - bd(G):
 *   2 dNLL / dtheta = sum_g <bd(G)_g, dk(x_g, x_g) / dtheta>       (measurement, measurement) pairs, group blocks only
 *                   + <2 H E, dk(x, u) / dtheta>                   (measurement, plain): a MEASUREMENT_ONLY term adds nothing
 *                   + <-E^T H E, dk(u, u) / dtheta>                (plain, plain)
 *   dNLL / d measurement_nugget = 1/2 trace(bd(G)),   dNLL / d inducing_nugget = 1/2 trace(-E^T H E)
 * formed without any n x n matrix from what the fit holds (Sigma = (K_uu + K_uf A^-1 K_fu)^-1 = Lacc^-T Lacc^-1):
 *   alpha = A^-1 (y - K_fu v),  Kt^-1 E = A^-1 K_fu Sigma,  bd(Kt^-1)_g = A_g^-1 - V_g V_g^T with V = A^-1 K_fu Lacc^-T,
 *   E^T = L_u^-T P,  A_g^-1 = R_g^T R_g with R_g = L_g^-1.
 * Work beyond the fit: ~6 n m^2 + 4 n s m + n s^2 flop for groups of s (triangular solves and products on the fp64 MFMA)
 * and three contractions per group of 4 slots, each reading its weight once.  Workspace: the fit's pool plus ONE more
 * ldk x n slab (ldk = m rounded up to even; Q1^T no longer shares P's region), 2 n s doubles of group slabs and
 * O(n + m^2) vectors.  No float atomics, fixed-order reductions: two identical calls give bit-identical results.
 *
 * Runs on the LL^T / CholeskyQR2 path only: where agp_sparse_fit_create would fall back to the pivoted L D L^T / QR
 * (K_uu or B^T B not numerically positive definite) it returns AGP_ERR_NOT_POSITIVE_DEFINITE and writes NaN to nll,
 * grad_nll and grad_nuggets.  A block of A that is not positive definite and NaN input: status as agp_sparse_nll, NaN
 * outputs.  Conditioning: the formulas contain K_uu^-1 explicitly, so the error of the gradient relative to the sum
 * of the absolute contracted terms is of order eps cond(K_uu) (and eps cond(Kt)), not eps: keep the inducing points no
 * denser than the length scale or raise inducing_nugget when gradients matter.
 * AGP_SPARSE_TIMING=1 prints the gradient's stages after the fit's. */
AGP_API int agp_sparse_nll_gradient(agp_context *ctx, const agp_kernel *kernel, const agp_features *x, int64_t n_groups,
                            const int64_t *offsets, const double *y, const double *y_var, const agp_features *u,
                            double measurement_nugget, double inducing_nugget,
                            int n_slots, const agp_gradient_slot *slots,
                            const double *tangents_x, int64_t ldtx, const double *tangents_u, int64_t ldtu,
                            double *nll, double *grad_nll, double *grad_nuggets, double *alpha);
/* Leave-one-group-out cross validation of the sparse model from ONE fit: for every group g of the fit, the prediction of
 * g by the model fitted to all the OTHER groups (cross_validate() / LeaveOneGroupOutLikelihood through refits,
 * evaluation/cross_validation.hpp, model_metrics.hpp:74-93, with _predict_impl :447-521 at the plain features of g), and its
 * negative log-likelihood against the group's targets with their variances added (prediction_metrics.hpp:112-128).
 * Arguments up to inducing_nugget exactly as agp_sparse_nll; the held-out groups are the fit's own, offsets[g] ..
 * offsets[g + 1].  The inducing points u are those of the call and are held fixed.
 *
 * With D, Kt as above (agp_sparse_nll_gradient), B_g = (Kt^-1)[g, g], Sigma_g = B_g^-1, alpha = Kt^-1 y: dropping group g
 * from a PITC model leaves exactly Kt without g's rows and columns, so
 *   d_g    = Sigma_g alpha_g                       (truth minus held-out mean)
 *   mean_g = y_g - d_g
 *   cov_g  = Sigma_g - D_g - M_g,   M_g = k(Measurement x_g, Measurement x_g) - k(x_g, x_g)
 *   V_g    = cov_g + diag(y_var_g) = Sigma_g - measurement_nugget I - M_g
 *   AGP_PREDICT_JOINT:    NLL_g = 1/2 (log|V_g| + d_g^T V_g^-1 d_g + |g| log 2 pi)
 *   AGP_PREDICT_MARGINAL: NLL_g = 1/2 sum_c (log v_c + d_c^2 / v_c + log 2 pi),   v_c = (V_g)_cc
 * M_g is the part of the covariance function that only measurements carry: the fit builds its blocks from measurement
 * features, a prediction is made at plain ones.  No prior term.  (The dense agp_logo_nll_gradient keeps the fit's noise in
 * the held-out covariance as the reference's dense fast path does; the sparse model has no fast path there, the refit is
 * the definition.)
 *
 * Outputs, each may be NULL: logo_nll (host, 1 value: sum_g NLL_g), group_nll (host, n_groups values in the caller's
 * order), and at x->location mean and variance (n values, the caller's grouped order; variance = diag(cov_g)) and joint
 * (the column-major |g| x |g| blocks cov_g one after the other, sum_g |g|^2 values, as agp_held_out_predictions).
 *
 * Stages: the fit; R_g, alpha, Z, N_g and B_g = R_g^T R_g - N_g^T N_g exactly as agp_sparse_nll_gradient forms them (the
 * same function; nothing after them - no E^T, no Lacc^-T solves, no W_uu); then per chunk of groups of similar size, in
 * lock step: B_g = L L^T, Q = L^-1, Sigma_g = Q^T Q, M_g pair by pair, V_g, (Joint) V_g = L_V L_V^T with d riding along,
 * the terms, and one fixed-order sum.
 * Work beyond the fit: ~2 n m^2 + 4 n s m + 3 n s^2 flop for groups of s, and 2 n s evaluations of the covariance
 * function.  Workspace: the fit's pool plus ONE more ldk x n slab, 2 n s doubles of group slabs, four padded block slabs
 * of the largest chunk (at most 4 x 2 n s doubles), O(n) vectors, and sum_g |g|^2 doubles when joint is asked for.
 * No float atomics, fixed-order reductions: two identical calls give bit-identical results.
 *
 * Status: malformed offsets (offsets[0] != 0, offsets[n_groups] != n, an empty group), n_groups <= 0 or an unknown
 * predict_type: AGP_ERR_INVALID_ARGUMENT, nothing is written.  LL^T / CholeskyQR2 path only: where agp_sparse_fit_create
 * would fall back to the pivoted path, AGP_ERR_NOT_POSITIVE_DEFINITE.  NaN input and a block of A that is not positive
 * definite: status as agp_sparse_nll.  A B_g or (Joint) a V_g that is not positive definite:
 * AGP_ERR_NOT_POSITIVE_DEFINITE.  Every failure after the argument checks writes NaN to all outputs.
 * AGP_SPARSE_TIMING=1 prints the stages after the fit's. */
AGP_API int agp_sparse_held_out(agp_context *ctx, const agp_kernel *kernel, const agp_features *x, int64_t n_groups,
                        const int64_t *offsets, const double *y, const double *y_var, const agp_features *u,
                        double measurement_nugget, double inducing_nugget, int predict_type,
                        double *logo_nll, double *group_nll, double *mean, double *variance, double *joint);
/* _predict_impl (:447-521): mean = K_*u v; covariance = K_** - Q_** + K_*u Sigma K_u*.  The mean
 * function is the caller's (mean_function_.add_to). */
AGP_API int agp_sparse_predict_mean(agp_context *ctx, const agp_kernel *kernel, const agp_sparse_fit *fit,
                            const agp_features *xs, double *mean, int out_location);
AGP_API int agp_sparse_predict_marginal(agp_context *ctx, const agp_kernel *kernel, const agp_sparse_fit *fit,
                                const agp_features *xs, double *mean, double *variance, int out_location);
AGP_API int agp_sparse_predict_joint(agp_context *ctx, const agp_kernel *kernel, const agp_sparse_fit *fit,
                             const agp_features *xs, double *mean, double *covariance, int out_location);

/* ---- predict ------------------------------------------------------------- */
/* gp_mean_prediction (gp.hpp:82-85) via _predict_impl (gp.hpp:350-366):
 *   mean = k(train, xs)^T information.  mean: m doubles at out_location. */
AGP_API int agp_predict_mean(agp_context *ctx, const agp_kernel *k, const agp_fit *fit,
                     const agp_features *xs, double *mean, int out_location);
/* gp_marginal_prediction (gp.hpp:87-101) via _predict_impl (gp.hpp:326-348):
 *   var_j = k(xs_j, xs_j) - sum_i (K^-1 K*)_ij K*_ij.
 * Any number of test points: they pass in slices that keep the n x m workspace at 2 GiB (nothing couples the
 * columns of a marginal prediction). */
AGP_API int agp_predict_marginal(agp_context *ctx, const agp_kernel *k,
                         const agp_fit *fit, const agp_features *xs,
                         double *mean, double *variance, int out_location);
/* gp_joint_prediction (gp.hpp:103-113) via _predict_impl (gp.hpp:305-324):
 *   cov = k(xs, xs) - K*^T K^-1 K*.  cov: m x m column-major, ld = m. */
AGP_API int agp_predict_joint(agp_context *ctx, const agp_kernel *k, const agp_fit *fit,
                      const agp_features *xs, double *mean, double *cov,
                      int out_location);

/* agp_predict_mean / _marginal / _joint for `count` fits of one padded size in lock step: problem b computes exactly what the
 * single call computes for kernels[b], fits[b], xs[b] (gp.hpp:305-366, 82-113; each xs[b]'s own is_measurement flag is
 * honoured).  The counterpart of agp_fit_create_batch for what every user does after fitting: at N of a few hundred one
 * prediction is a handful of latency-bound launches, a batch runs each of them once (one grid dimension = problem).
 *   mode                 0 mean, 1 marginal, 2 joint (the numbering of agp_solver_predict)
 *   kernels[b], xs[b]    covariance function and test features of problem b: all xs[b] have one m and one location,
 *                        dim == the training dimension of fits[b]; dim may differ between problems
 *   fits[b]              plain fp64 LL^T fits with training features, of one padded size (agp_fit_padded_size; the real
 *                        rows and phantom ranges may differ), living on ctx (a mixed-precision fit, a factor of
 *                        agp_factor_create: AGP_ERR_INVALID_ARGUMENT)
 *   mean, ldm            m x count, ldm >= m
 *   second, lds          marginal: m x count variances, lds >= m; joint: problem b's full symmetric m x m covariance,
 *                        column-major with ld = m, at second + b * lds, lds >= m * m; ignored for mode 0
 *   status[b]            (host) what the call that created fits[b] reported: AGP_OK, AGP_ERR_NAN_INPUT or
 *                        AGP_ERR_NOT_POSITIVE_DEFINITE; a failed fit gets NaN-filled outputs, the rest of the batch is
 *                        unaffected and the call returns AGP_OK
 * Both outputs live at out_location.  A malformed argument anywhere (count <= 0, a null entry, unequal n or m, mixed
 * locations, a dimension mismatch, a bad mode, ldm or lds too short, a fit without training features) returns
 * AGP_ERR_INVALID_ARGUMENT and writes nothing; m == 0 returns AGP_OK.
 * Lock step: fits[] is cut into maximal runs in which the factors, the tile images and the information vectors lie at
 * one constant non-negative stride with one leading dimension - consecutive handles of one agp_fit_create_batch call, or
 * any evenly spaced subset of them; the fits need not come from one call.  A run of two or more goes through the
 * batched launches, a run of one through agp_predict_mean / _marginal / _joint unchanged.  Fits with phantom rows (of
 * agp_fit_create_batch_ragged, agp_fit_update_batch) join the runs: one table-driven launch zeroes the phantom rows of
 * their cross covariances before the substitution.  Inside a run there is no synchronisation but the closing one; the descriptor tables are uploaded
 * from the context's pinned staging area.  Host-resident test features of all runs are uploaded into one device
 * allocation before the first launch, with one wait for those uploads (device-resident ones are used in place).  Covariance functions of the radial<Euclidean> [+ noise] shapes with one
 * operator and one dimension in a run are evaluated by ONE launch for the run; other runs by a launch per problem that
 * does the same arithmetic per problem.  No float atomics, fixed-order reductions: two identical calls are bit-identical,
 * and no problem's arithmetic depends on its position or its neighbours - with one caveat: the MFMA products of the
 * substitution and of the joint covariance (launch_gemm_nt_sub_batched) choose their tile shape from tiles x problems
 * of a launch (64 x 64 tiles below 512, 128 x 128 from there on), so a problem's last bits may differ between two
 * batches that fall on different sides of that threshold; within the bounds above they agree.
 * Workspace: per problem ld_n * m doubles (V = L^-1 K*, ld_n = n rounded up to even) for modes 1 and 2, plus ld_m * m
 * (ld_m = m rounded up to even) for mode 2; a run is cut into sub-batches of whole problems,
 *   problems per sub-batch = max(1, min(65535, floor(2^28 / (ld_n m + [mode == 2] ld_m m)))),
 * which keeps those buffers at 2 GiB, the bound of agp_predict_marginal (AGP_PREDICT_CHUNK=<points> replaces the formula
 * by max(1, floor(points / m))).  Host outputs add a staging copy of the
 * sub-batch's results (m, 2 m or m + m * m doubles per problem). */
AGP_API int agp_predict_batch(agp_context *ctx, int count,
                              const agp_kernel *const *kernels, const agp_fit *const *fits,
                              const agp_features *const *xs, int mode,
                              double *mean, int64_t ldm,
                              double *second, int64_t lds,
                              int out_location, int *status);

/* ---- CovarianceRepresentation compositions on the device ----------------------------------------------------------
 * The solvers a fit can hold besides its own factor (src/models/gp.hpp:42-45 asks for `solve` and `rows`), and the generic
 * form of _predict_impl over any of them - everything stays in HBM, a solve is device solves + MFMA products:
 *   agp_solver_from_fit / _from_ldlt   the LL^T factor / the pivoted L D L^T as a solver (borrowed: the fit outlives it)
 *   agp_solver_block_symmetric         BlockSymmetric<Solver> (src/linalg/block_symmetric.hpp:46-133): solver of
 *                                      [[A, B], [B^T, C]] from a solver of A, B (rows(A) x rows(S), ldb, at `location`) and the
 *                                      solver S of the Schur complement C - B^T A^-1 B; Ai_B = A.solve(B) is kept on the device
 *   agp_solver_explained               ExplainedCovariance (src/covariance_functions/representations.hpp:64-96):
 *                                      S^-1 = outer^-1 inner outer^-1, inner n x n (ld, at `location`)
 *   agp_solver_solve                   rhs / out n x nrhs column-major (ld = n) at `location`
 *   agp_solver_predict                 gp.hpp:305-366 over a generic representation: mode 0 mean, 1 marginal (variance m),
 *                                      2 joint (covariance m x m, ld = m); train = the fit's training features as the
 *                                      covariance function sees them, information n doubles; all at `location`
 * Sub-solvers are borrowed and must outlive the composition. */
typedef struct agp_solver agp_solver;
AGP_API int agp_solver_from_fit(agp_context *ctx, const agp_fit *fit, agp_solver **out);
AGP_API int agp_solver_from_ldlt(agp_context *ctx, const agp_ldlt *ldlt, agp_solver **out);
AGP_API int agp_solver_block_symmetric(agp_context *ctx, const agp_solver *A, const double *B, int64_t ldb, int location,
                                       const agp_solver *S, agp_solver **out);
AGP_API int agp_solver_explained(agp_context *ctx, const agp_solver *outer, const double *inner, int64_t ld, int location,
                                 agp_solver **out);
AGP_API int64_t agp_solver_rows(const agp_solver *solver);
AGP_API int agp_solver_solve(agp_context *ctx, const agp_solver *solver, const double *rhs, int64_t nrhs, double *out, int location);
AGP_API int agp_solver_predict(agp_context *ctx, const agp_kernel *k, const agp_solver *solver, const agp_features *train,
                               const double *information, const agp_features *xs, double *mean, double *var_or_cov, int mode,
                               int location);
/* FitModel::update on a generic representation (src/models/gp.hpp:403-407): the information vector of the conditioned fit,
 * [information - Ai_B Si_delta ; Si_delta], from the Ai_B a BlockSymmetric solver holds in HBM (block_symmetric.hpp:51).
 * information: rows(A) doubles, si_delta: rows(S) doubles, out: rows(A) + rows(S) doubles, all at `location`. */
AGP_API int agp_solver_update_information(agp_context *ctx, const agp_solver *block_symmetric, const double *information,
                                          const double *si_delta, double *out, int location);
/* agp_solver_predict for LinearCombination<X> features on either side (covariance_functions/callers.hpp:321-396): train / xs
 * hold the EXPANDED points, combination a of a side = its expanded points offsets[a] .. offsets[a + 1) with
 * coefficients[..] (host arrays as in agp_gram_combined; offsets == NULL: plain features on that side).  The solver's
 * size is the number of training combinations.  Covariances, contraction, solve and products all run on the device. */
AGP_API int agp_solver_predict_combined(agp_context *ctx, const agp_kernel *k, const agp_solver *solver, const agp_features *train,
                                        int64_t n_train, const int64_t *train_offsets, const double *train_coefficients,
                                        const double *information, const agp_features *xs, int64_t n_xs, const int64_t *xs_offsets,
                                        const double *xs_coefficients, double *mean, double *var_or_cov, int mode, int location);
AGP_API void agp_solver_destroy(agp_solver *solver);

/* ---- multi-GPU: ONE fit sharded over the GPUs of a node ---------------------------------------
 * The work of the Fit<GPFit> constructor (include/albatross/src/models/gp.hpp:61-69: covariance +
 * diag(targets.covariance), SerializableLDLT, information = ldlt.solve(y)) and of _fit_impl's Gram
 * (gp.hpp:281-294) for one dataset, spread over `nranks` processes with one GPU each.
 *
 * Layout: ROW-block cyclic.  The training points are cut into row blocks of 512; row block b (the rows
 * 512 b .. 512 b + 511 of the lower triangle, columns 0 .. 512 (b + 1)) belongs to rank
 * snake(b) = 0..G-1, G-1..0, ... (equal work per pair of rounds); every rank stacks its row blocks into one
 * local column-major matrix and builds their Gram entries itself (no communication).  Per block column k:
 *   owner(k)   LL^T of the 512 x 512 diagonal block (+ the fused forward substitution), BROADCAST of
 *              L_kk / its tile images / z_k                                  (2.4 MB, RCCL broadcast)
 *   every rank X = A[own rows > k, k] L_kk^-T on its own rows, y_own -= X z_k
 *   all ranks  ALL-GATHER of the panel rows (each rank contributes its rows; every xGMI link of every GPU
 *              carries 1/G of the panel at the same time)                    (RCCL all-gather)
 *   every rank C[own rows, cols > k] -= X_own P^T                            (fp64 MFMA update kernels)
 * with one block column of look-ahead: the owner of block k + 1 updates and factors its diagonal block while the
 * panel of step k is still being gathered and applied.  information = L^-T z follows super-block by super-block (four
 * row blocks: every rank keeps the diagonal super-blocks and solves them redundantly) with ONE small all-reduce per
 * super-block.  Every rank receives the full information vector and log-determinant.
 *
 * agp_comm wraps the transport: RCCL (librccl of the ROCm installation, loaded at first use), or - for tests and
 * for boxes where RCCL cannot be used (it refuses two ranks on one device) - collectives supplied by the caller. */
#define AGP_COMM_ID_BYTES 128
/* ncclGetUniqueId: rank 0 calls it and hands the bytes to every rank by any means (a file, MPI, a TCP store). */
AGP_API int agp_comm_unique_id(void *id);
/* ncclCommInitRank on ctx's device; collective over all ranks.  AGP_ERR_COMM when RCCL is unavailable or fails. */
AGP_API int agp_comm_create(agp_context *ctx, int nranks, int rank, const void *id, agp_comm **out);
/* op for all_reduce: 0 = sum, 1 = max */
typedef struct {
  void *user;
  /* every callback works on HOST doubles and returns 0 on success; all ranks call them in the same order */
  int (*broadcast)(void *user, double *buf, int64_t count, int root);
  int (*all_gather)(void *user, const double *send, double *recv, int64_t count_per_rank);
  int (*all_reduce)(void *user, double *buf, int64_t count, int op);
} agp_comm_callbacks;
AGP_API int agp_comm_create_callbacks(int nranks, int rank, const agp_comm_callbacks *cb, agp_comm **out);
/* A DEVICE-ASYNCHRONOUS transport between processes that share ONE GPU (csrc/shard_ipc.hip): every collective is a few
 * kernels on the caller's stream - stores into the peers' mailboxes (hipIpcOpenMemHandle), stream-ordered flags, bounded
 * spins - and the host returns at once, as with RCCL.  For exercising the asynchronous multi-rank schedule on a one-GPU
 * box (RCCL refuses two ranks per device; the callback transport is host-synchronous); RCCL remains the transport of
 * real multi-GPU runs.  `bootstrap`: host collectives (all_gather, all_reduce) that carry the 64-byte IPC handles at
 * creation and serve agp_comm_all_reduce_host / agp_comm_barrier afterwards; it must outlive the communicator.
 * mailbox_doubles: capacity of one of the two mailbox slots (0: 8 Mi doubles); larger messages travel in pieces.
 * nranks <= 16; needs HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of every rank.  Collective (also the destroy). */
AGP_API int agp_comm_create_ipc(agp_context *ctx, int nranks, int rank, const agp_comm_callbacks *bootstrap, int64_t mailbox_doubles,
                                agp_comm **out);
AGP_API void agp_comm_destroy(agp_comm *comm);
AGP_API int agp_comm_size(const agp_comm *comm);
AGP_API int agp_comm_rank(const agp_comm *comm);
/* control-plane helpers for host code (bench.py's barrier and max-over-ranks timing): in-place on host doubles */
AGP_API int agp_comm_all_reduce_host(agp_comm *comm, double *buf, int64_t count, int op);
AGP_API int agp_comm_barrier(agp_comm *comm);

/* ownership arithmetic of the row-block-cyclic layout (pure host functions) */
AGP_API int64_t agp_shard_local_rows(int64_t n, int64_t block, int nranks, int rank);
/* global row of local row l of `rank` (l < agp_shard_local_rows) */
AGP_API int64_t agp_shard_global_row(int64_t n, int64_t block, int nranks, int rank, int64_t l);
AGP_API int agp_shard_owner(int64_t block_index, int nranks);

typedef struct agp_sharded_fit agp_sharded_fit;
/* One fit over all ranks of `comm`; collective.  Every rank passes the SAME full dataset (x, y, y_var as in
 * agp_fit_create; at x->location) and receives information (n doubles, host, may be NULL) and log_det.
 * A failure (NaN, non-positive pivot, transport error or timeout: AGP_COMM_TIMEOUT_S seconds, default 120) is
 * reported with the same status on every rank that can still be reached.  comm == NULL: one rank, no transport. */
AGP_API int agp_sharded_fit_create(agp_context *ctx, agp_comm *comm, const agp_kernel *k, const agp_features *x,
                           const double *y, const double *y_var, agp_sharded_fit **out, double *information,
                           double *log_det);
AGP_API void agp_sharded_fit_destroy(agp_sharded_fit *fit);
AGP_API int64_t agp_sharded_fit_failed_pivot(const agp_sharded_fit *fit);
/* Replicate the factor: all-gather of the row blocks, after which every rank holds an ordinary agp_fit of the whole
 * problem (the factor of gp.hpp:61-69) and predicts ITS share of the test points with agp_predict_* - predictions
 * are independent per test point (gp.hpp:82-113), so sharding M needs no further exchange.  Collective. */
AGP_API int agp_sharded_fit_replicate(agp_context *ctx, agp_sharded_fit *fit, agp_fit **out);
/* gp_marginal_prediction (src/models/gp.hpp:87-101) straight from the SHARDED factor, without replicating it: the
 * distributed forward substitution V = L^-1 K* by block rows (the owner of a block row solves it and broadcasts its
 * w x M rows of V, every rank updates its own later rows; N x M doubles of broadcasts per call) and one all-reduce of
 * the M column sums.  For factors too large to hold on every GPU; while it fits, agp_sharded_fit_replicate + the
 * ordinary agp_predict_* on each rank's share of the test points needs no exchange at all.  Collective: every rank
 * passes the same test points and receives all M means and variances (at `location`). */
AGP_API int agp_sharded_predict_marginal(agp_context *ctx, const agp_kernel *k, agp_sharded_fit *fit, const agp_features *xs,
                                         double *mean, double *variance, int location);
/* gp_joint_prediction (src/models/gp.hpp:103-113) from the sharded factor, likewise without replicating it: the same
 * distributed forward substitution, then cov = K** - V^T V where every rank multiplies its own rows of V = L^-1 K* and ONE
 * all-reduce of m x m doubles sums the products.  cov: m x m column-major, ld = m, on every rank.  Collective. */
AGP_API int agp_sharded_predict_joint(agp_context *ctx, const agp_kernel *k, agp_sharded_fit *fit, const agp_features *xs,
                                      double *mean, double *covariance, int location);
/* per-stage device time of the last sharded fit on this rank, ms: 0 gram, 1 factor, 2 back substitution,
 * 3 sum of the bulk update launches, 4 their count, 5 their algorithmic flop, 6 host time spent enqueueing the
 * schedule, 7 host time until the device had drained (6 ~ 7: the host is the bottleneck) */
AGP_API int agp_sharded_fit_stage(const agp_sharded_fit *fit, int stage, double *value);

/* ---- instrumentation (bench.py) ----------------------------------------- */
/* Per-stage device time of the LAST fit / nll on this context, measured with
 * HIP events on the stream the kernels were launched on.  Stages:
 * 0 gram, 1 factor (total), 2 solve, 3 trailing-update kernels only (sum),
 * 4 number of trailing-update launches.  Returns ms (or a count for 4).  Stages 6-9:
 * the gradient entries (agp_nll_gradient, agp_loo_nll_gradient).  Stage 10: the step chain of agp_pivoted_cholesky.
 * Stages 11, 12: the preconditioner build and the conjugate-gradient chain of agp_iterative_fit_create.
 * Stages 12, 13: the probe solves and the tangent forms of agp_iterative_nll_gradient and agp_iterative_nll.
 * Stage 14: the probes' generation, the host quadrature and log det P of agp_iterative_nll. */
AGP_API int agp_last_stage_ms(const agp_context *ctx, int stage, double *ms);
/* enable (1) / disable (0) per-stage event timing (default off: events add
 * host overhead to the launch chain). */
AGP_API int agp_set_profiling(agp_context *ctx, int enabled);

/* ---- switches ------------------------------------------------------------
 * The library reads the following environment variables, ONCE per context, in agp_context_create (csrc/api.hip:
 * read_tuning); a later change of the environment does not affect an existing context.  Nothing else is switchable:
 * the schedule's other parameters are constants (csrc/chol.hip).
 *   AGP_PANEL_FUSED=0        POTRF and panel TRSM as two launches instead of the fused panel kernel
 *   AGP_STEP_BELOW=<rows>    remaining rows at or below which every panel is ONE step launch (default 4608; 0: off)
 *   AGP_MERGE_ABOVE=<rows>   trailing rows above which the update of the NEXT block column rides in the bulk launch (its
 *                            tiles first, counted; a one-wave gate kernel on the panel stream) instead of being a launch
 *                            of its own behind an event (default 8704; 0: the round-5 schedule)
 *   AGP_GRAM_SOP=0           covariance trees through the stack interpreter only (parity tests run both evaluators)
 *   AGP_MIXED_F16=0          agp_fit_create_mixed forms its products from three bf16 planes (round 5) instead of two fp16 planes
 *   AGP_F16X2_TERMS=3        ... from two fp16 planes WITHOUT the h2 h2 product (3 % faster, log_det outside the bar: gemm_split_planes.hip)
 *   AGP_F16X2_LDS_PAD=<b>    extra LDS bytes per workgroup of the fp16 x 2 kernel (default 8192: two per CU; 0: three)
 *   AGP_MIXED_BF16=0         agp_fit_create_mixed forms its fp32-accurate products on the fp32 MFMA instead of the 16-bit planes
 *   AGP_BF16X3_LDS_PAD=<b>   extra LDS bytes per workgroup of the bf16 x 3 kernel (default 8192: two per CU; 0: three)
 *   AGP_MIXED_NBO=<w>        outer block width of the mixed factorisation while > 8192 rows remain (default 512)
 *   AGP_SOLVE_NBO=<w>        outer block width of the forward substitution with many right-hand sides (predictions; default 512;
 *                            measured flat from 256 to 1024: profiles/r06/time_predict_marginal_nbo.txt)
 *   AGP_FP64_NBO=<w>         the same for the fp64 factorisation (default 0 = 512; a multiple of 128 above 512, any other
 *                            value is ignored - the rule of AGP_MIXED_NBO)
 *   AGP_GEMM_SMALL_LIMIT=<t> 64 x 64 instead of 128 x 128 tiles for products of fewer than t 128-tiles (default 512)
 *   AGP_BACKSUB_COOP=0       the fit's back substitution as one launch per block (rounds 1-4) instead of ONE launch
 *   AGP_BACKSUB_COOP_MAX=<n> largest fit that uses the one-launch back substitution (default 2047)
 *   AGP_SPARSE_PIVOTED=1     the sparse GP always takes the literal (pivoted LDL^T + column-pivoted QR) path
 *   AGP_PREDICT_CHUNK=<m>    test points per slice of marginal predictions (default: by memory, 2 GiB per slice);
 *                            agp_predict_batch: V columns per sub-batch, i.e. max(1, floor(<m> / m)) problems
 *   AGP_SHARD_BLOCK=<b>      128 / 256 / 512 rows per row block of the sharded fit (default 512; tests)
 *   AGP_SHARD_FORCE_COMM=1   ONE rank runs the multi-rank schedule through its transport (RCCL group of one; tests)
 *   AGP_SHARD_HOST_PACING=1  the sharded schedule is paced by the host instead of device-side flags
 *   AGP_SHARD_MASK_GFLOP=<g> flop of a rank's bulk update per step (default 40e9) below which a sharded fit counts as
 *                            chain-bound: bulk updates on the CU-masked stream + device-side pacing from there on
 * and, process-wide, at first use:
 *   AGP_COMM_TIMEOUT_S=<s>   deadline of every wait that may hold a collective (default 120)
 *   AGP_RCCL_LIB=<path>      librccl to dlopen (default: the ROCm installation's)
 *   AGP_ROCTX=1              roctx ranges around the stages (rocprofv3 --marker-trace)
 * Test-only entry points (kernel probes, the schedule over caller-supplied block arithmetic, a transport that moves
 * nothing) are `agp_debug_*` in libalbatross_amd_debug.so and are not part of this interface. */

#ifdef __cplusplus
}
#endif
#endif /* ALBATROSS_AMD_H */
