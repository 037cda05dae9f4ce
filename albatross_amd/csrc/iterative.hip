// iterative.hip — the exact Gaussian-process fit that never forms K: preconditioned conjugate gradients around the fused
// product of gram_matvec.hip, preconditioned by the greedy pivoted Cholesky factor of pivoted_chol.hip
// (agp_iterative_fit_create, agp_iterative_solve, agp_iterative_predict_*; include/albatross_amd.h), the probe estimate
// of its log-likelihood gradient (agp_iterative_nll_gradient) around the tangent forms of gram_tangent.hip, and the
// log-likelihood VALUE by stochastic Lanczos quadrature (agp_iterative_nll): the alpha and beta of every iteration, which
// the recurrences derive on the device anyway, are the Lanczos tridiagonal of the preconditioned matrix; pcg_record_kernel
// keeps them, lanczos_quadrature.h takes the Gauss quadrature of log on the host, and log det P is known in closed form.
//
//   A = k(x, x) + diag(y_var);  A ~ L L^T + (A - L L^T), L = n x m from the pivoted Cholesky of A (m <= precond_rank);
//   P = L L^T + delta I,  delta = max(tr(A - L L^T) / (n - m), 1e-8 max_i A_ii)  (m = n: the floor alone);
//   P^-1 r = (r - L (delta I + L^T L)^-1 L^T r) / delta  (Woodbury): L^T L once on the fp64 GEMM, its m x m matrix factored
//   by the dense LL^T; per iteration two skinny products (pcg_lt_r_kernel, pcg_precond_kernel) and the two substitutions.
//
// The right-hand sides of a chunk (<= 16) run INDEPENDENT recurrences that share each launch - this is not block CG.  All
// per-column scalars (alpha, beta, r^T z, p^T A p, the norms, the stop marks) live in one control block on the device;
// every reduction is one workgroup per column with a fixed order (no float atomics), and its last thread derives the
// scalars.  A column stops when ||r|| <= tolerance ||b||; from then on every kernel skips it, so its vectors keep their
// bits whatever is queued behind.  The host looks at the control block once per PCG_LOOK iterations with the next
// PCG_LOOK queued behind (the pattern of agp_pivoted_cholesky); once no column is active, or an error is marked, every
// queued kernel returns at its first instruction.
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <thread>
#include <vector>
#include "api_internal.h"
#include "gram_matvec.h"
#include "gram_tangent.h"
#include "iterative_internal.h"
#include "lanczos_quadrature.h"
#include "trace.h"

int pivoted_cholesky_impl(agp_context *c, const agp_kernel *k, const agp_features *x, const double *diag_dev, int64_t max_rank,
                          double rel_tol, int64_t *pivots, int64_t *rank, double *L, int64_t ldl, double *residual_diag, int location,
                          double *trace_residual, double *d0_out);  // pivoted_chol.hip

namespace agp {

// one workgroup per column c: s = sum_i A[i, c] B[i, c] in a fixed order, then the scalars that follow from it
template <int MODE>
__global__ __launch_bounds__(PCG_DOT_THREADS) void pcg_dot_kernel(PcgCtrl *ctrl, const double *A, const double *B, long long ld,
                                                                  long long n, int k, double tol) {
  if (MODE != DOT_BB && ctrl->active <= 0) return;
  const int c = blockIdx.x;
  if (MODE != DOT_BB && ctrl->stopped[c]) return;
  __shared__ double red[PCG_DOT_THREADS / 64];
  const double *a = A + (long long)c * ld, *b = B + (long long)c * ld;
  double acc = 0.;
  for (long long i = threadIdx.x; i < n; i += PCG_DOT_THREADS) acc += a[i] * b[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.;
  for (int w = 0; w < PCG_DOT_THREADS / 64; ++w) s += red[w];
  if (s != s) {
    ctrl->nan = 1;
    atomicSub(&ctrl->active, PCG_ERROR);
    return;
  }
  if (MODE == DOT_BB) {
    ctrl->bb[c] = s;
    ctrl->resid[c] = s > 0. ? 1. : 0.;
    if (s > 0.) atomicAdd(&ctrl->active, 1);
    else ctrl->stopped[c] = 1;  // a zero right-hand side: the solution is zero, no iteration
  } else if (MODE == DOT_RZ) {
    ctrl->rz[k & 1][c] = s;
    ctrl->beta[c] = k == 0 ? 0. : s / ctrl->rz[(k - 1) & 1][c];
  } else if (MODE == DOT_PQ) {
    if (s <= 0.) {
      ctrl->npd = 1;
      atomicSub(&ctrl->active, PCG_ERROR);
      return;
    }
    ctrl->alpha[c] = ctrl->rz[k & 1][c] / s;
  } else {
    const double bb = ctrl->bb[c];
    ctrl->iters[c] = k + 1;
    ctrl->resid[c] = sqrt(s) / sqrt(bb);
    if (sqrt(s) <= tol * sqrt(bb)) {
      ctrl->stopped[c] = 1;
      atomicSub(&ctrl->active, 1);
    }
  }
}

// T1[j, c] = sum_i L[i, j] R[i, c]: workgroup j reads column j of L once for the t right-hand sides
__global__ __launch_bounds__(256) void pcg_lt_r_kernel(const PcgCtrl *ctrl, const double *L, long long ldl, long long n, const double *R,
                                                       long long ldr, int t, double *T1, long long ldt) {
  if (ctrl->active <= 0) return;
  __shared__ double red[4][PCG_COLS];
  const long long j = blockIdx.x;
  const double *col = L + j * ldl;
  double acc[PCG_COLS];
#pragma unroll
  for (int c = 0; c < PCG_COLS; ++c) acc[c] = 0.;
  for (long long i = threadIdx.x; i < n; i += 256) {
    const double l = col[i];
#pragma unroll
    for (int c = 0; c < PCG_COLS; ++c)
      if (c < t) acc[c] += l * R[(long long)c * ldr + i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < PCG_COLS; ++c) {
    double r = acc[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
    if (lane == 0) red[wave][c] = r;
  }
  __syncthreads();
  if ((int)threadIdx.x < t) T1[(long long)threadIdx.x * ldt + j] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// Z = (R - L U) / delta, a thread per row, the sum over j = 0, 1, ... (m = 0: Z = R / delta)
__global__ __launch_bounds__(256) void pcg_precond_kernel(const PcgCtrl *ctrl, const double *L, long long ldl, long long n, long long m,
                                                          const double *U, long long ldu, const double *R, double *Z, long long ld, int t,
                                                          double delta) {
  if (ctrl->active <= 0) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc[PCG_COLS];
#pragma unroll
  for (int c = 0; c < PCG_COLS; ++c) acc[c] = 0.;
  for (long long j = 0; j < m; ++j) {
    const double l = L[j * ldl + i];
#pragma unroll
    for (int c = 0; c < PCG_COLS; ++c)
      if (c < t) acc[c] += l * U[(long long)c * ldu + j];
  }
#pragma unroll
  for (int c = 0; c < PCG_COLS; ++c)
    if (c < t && !ctrl->stopped[c]) Z[(long long)c * ld + i] = (R[(long long)c * ld + i] - acc[c]) / delta;
}

// row k of the coefficient log (iterative_internal.h) = alpha, beta of the columns that iterate; one wave, lane = column
__global__ __launch_bounds__(64) void pcg_record_kernel(const PcgCtrl *ctrl, double *log, int max_iterations, int k, int t) {
  if (ctrl->active <= 0) return;
  const int c = threadIdx.x;
  if (c >= t || c >= PCG_COLS || ctrl->stopped[c]) return;
  if (k == 0) log[c] = ctrl->rz[0][c];
  double *alpha = log + PCG_COLS, *beta = alpha + (size_t)max_iterations * PCG_COLS;
  alpha[(size_t)k * PCG_COLS + c] = ctrl->alpha[c];
  beta[(size_t)k * PCG_COLS + c] = ctrl->beta[c];
}

// Z = L G1 + sqrt_delta G2, a thread per row, the sum over j = 0, 1, ... (m = 0: Z = sqrt_delta G2); Z may be G2
__global__ __launch_bounds__(256) void pcg_probe_kernel(const double *L, long long ldl, long long n, long long m, const double *G1,
                                                        long long ldg1, const double *G2, long long ldg2, double *Z, long long ldz, int t,
                                                        double sqrt_delta) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc[PCG_COLS];
#pragma unroll
  for (int c = 0; c < PCG_COLS; ++c) acc[c] = 0.;
  for (long long j = 0; j < m; ++j) {
    const double l = L[j * ldl + i];
#pragma unroll
    for (int c = 0; c < PCG_COLS; ++c)
      if (c < t) acc[c] += l * G1[(long long)c * ldg1 + j];
  }
#pragma unroll
  for (int c = 0; c < PCG_COLS; ++c)
    if (c < t) Z[(long long)c * ldz + i] = acc[c] + sqrt_delta * G2[(long long)c * ldg2 + i];
}

// P = Z + beta P (the first iteration: P = Z); blockIdx.y = column
__global__ __launch_bounds__(256) void pcg_p_kernel(const PcgCtrl *ctrl, const double *Z, double *P, long long ld, long long n, int first) {
  if (ctrl->active <= 0) return;
  const int c = blockIdx.y;
  if (ctrl->stopped[c]) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long e = (long long)c * ld + i;
  P[e] = first ? Z[e] : Z[e] + ctrl->beta[c] * P[e];
}

// X += alpha P, R -= alpha Q; blockIdx.y = column
__global__ __launch_bounds__(256) void pcg_xr_kernel(const PcgCtrl *ctrl, double *X, long long ldx, double *R, const double *P, const double *Q,
                                                     long long ld, long long n) {
  if (ctrl->active <= 0) return;
  const int c = blockIdx.y;
  if (ctrl->stopped[c]) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double alpha = ctrl->alpha[c];
  const long long e = (long long)c * ld + i;
  X[(long long)c * ldx + i] += alpha * P[e];
  R[e] -= alpha * Q[e];
}

// stats[0] = max, [1] = min, [2] = sum (fixed order), [3] = 1 on a NaN, of d_i + yvar_i
__global__ __launch_bounds__(1024) void pcg_diag_stats_kernel(const double *d, const double *yvar, long long n, double *stats) {
  __shared__ double smax[1024], smin[1024], ssum[1024];
  __shared__ int snan;
  if (threadIdx.x == 0) snan = 0;
  __syncthreads();
  double mx = -INFINITY, mn = INFINITY, sm = 0.;
  bool bad = false;
  for (long long i = threadIdx.x; i < n; i += 1024) {
    const double v = d[i] + (yvar ? yvar[i] : 0.);
    bad = bad || v != v;
    mx = fmax(mx, v);
    mn = fmin(mn, v);
    sm += v;
  }
  if (bad) atomicOr(&snan, 1);
  smax[threadIdx.x] = mx; smin[threadIdx.x] = mn; ssum[threadIdx.x] = sm;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]);
      smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + w]);
      ssum[threadIdx.x] += ssum[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { stats[0] = smax[0]; stats[1] = smin[0]; stats[2] = ssum[0]; stats[3] = snan ? 1. : 0.; }
}

// M = delta I - C (C = -L^T L from the GEMM), m x m
__global__ __launch_bounds__(256) void pcg_shift_kernel(double *C, long long ldc, long long m, double delta) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (i >= m) return;
  C[j * ldc + i] = (i == j ? delta : 0.) - C[j * ldc + i];
}

// var_j = prior_j - sum_i Kc[i, j] S[i, j]; one workgroup per test point of the slice
__global__ __launch_bounds__(256) void pcg_variance_kernel(const double *Kc, const double *S, long long ld, long long n, const double *prior,
                                                           double *var) {
  __shared__ double red[4];
  const long long j = blockIdx.x;
  double acc = 0.;
  for (long long i = threadIdx.x; i < n; i += 256) acc += Kc[j * ld + i] * S[j * ld + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) var[j] = prior[j] - ((red[0] + red[1]) + (red[2] + red[3]));
}

// ---- the launchers (iterative_internal.h): the product below and the probes of debug_api.hip launch through these ----
void launch_pcg_dot(hipStream_t s, int mode, PcgCtrl *ctrl, const double *A, const double *B, long long ld, long long n, int t, int k,
                    double tol) {
  const dim3 grid(t), block(PCG_DOT_THREADS);
  switch (mode) {
  case DOT_BB: hipLaunchKernelGGL(pcg_dot_kernel<DOT_BB>, grid, block, 0, s, ctrl, A, B, ld, n, k, tol); break;
  case DOT_RZ: hipLaunchKernelGGL(pcg_dot_kernel<DOT_RZ>, grid, block, 0, s, ctrl, A, B, ld, n, k, tol); break;
  case DOT_PQ: hipLaunchKernelGGL(pcg_dot_kernel<DOT_PQ>, grid, block, 0, s, ctrl, A, B, ld, n, k, tol); break;
  default: hipLaunchKernelGGL(pcg_dot_kernel<DOT_RR>, grid, block, 0, s, ctrl, A, B, ld, n, k, tol); break;
  }
}

void launch_pcg_lt_r(hipStream_t s, const PcgCtrl *ctrl, const double *L, long long ldl, long long n, long long m, const double *R,
                     long long ldr, int t, double *T1, long long ldt) {
  hipLaunchKernelGGL(pcg_lt_r_kernel, dim3((unsigned)m), dim3(256), 0, s, ctrl, L, ldl, n, R, ldr, t, T1, ldt);
}

void launch_pcg_precond(hipStream_t s, const PcgCtrl *ctrl, const double *L, long long ldl, long long n, long long m, const double *U,
                        long long ldu, const double *R, double *Z, long long ld, int t, double delta) {
  hipLaunchKernelGGL(pcg_precond_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ctrl, L, ldl, n, m, U, ldu, R, Z, ld, t, delta);
}

void launch_pcg_p(hipStream_t s, const PcgCtrl *ctrl, const double *Z, double *P, long long ld, long long n, int t, int first) {
  hipLaunchKernelGGL(pcg_p_kernel, dim3((unsigned)((n + 255) / 256), t), dim3(256), 0, s, ctrl, Z, P, ld, n, first);
}

void launch_pcg_xr(hipStream_t s, const PcgCtrl *ctrl, double *X, long long ldx, double *R, const double *P, const double *Q, long long ld,
                   long long n, int t) {
  hipLaunchKernelGGL(pcg_xr_kernel, dim3((unsigned)((n + 255) / 256), t), dim3(256), 0, s, ctrl, X, ldx, R, P, Q, ld, n);
}

void launch_pcg_diag_stats(hipStream_t s, const double *d, const double *yvar, long long n, double *stats) {
  hipLaunchKernelGGL(pcg_diag_stats_kernel, dim3(1), dim3(1024), 0, s, d, yvar, n, stats);
}

void launch_pcg_shift(hipStream_t s, double *C, long long ldc, long long m, double delta) {
  hipLaunchKernelGGL(pcg_shift_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)m), dim3(256), 0, s, C, ldc, m, delta);
}

void launch_pcg_variance(hipStream_t s, const double *Kc, const double *S, long long ld, long long n, long long t, const double *prior,
                         double *var) {
  hipLaunchKernelGGL(pcg_variance_kernel, dim3((unsigned)t), dim3(256), 0, s, Kc, S, ld, n, prior, var);
}

void launch_pcg_record(hipStream_t s, const PcgCtrl *ctrl, double *log, int max_iterations, int k, int t) {
  hipLaunchKernelGGL(pcg_record_kernel, dim3(1), dim3(64), 0, s, ctrl, log, max_iterations, k, t);
}

void launch_pcg_probe(hipStream_t s, const double *L, long long ldl, long long n, long long m, const double *G1, long long ldg1,
                      const double *G2, long long ldg2, double *Z, long long ldz, int t, double sqrt_delta) {
  hipLaunchKernelGGL(pcg_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, L, ldl, n, m, G1, ldg1, G2, ldg2, Z, ldz, t,
                     sqrt_delta);
}

}  // namespace agp

using namespace agp;

struct agp_iterative_fit {
  agp_context *ctx = nullptr;
  int64_t n = 0, rank = 0;
  agp_kernel_full kernel;              // the covariance function of the fit (host copy)
  DevMem<DevProgram> dprog;            // ... and its device copy
  DeviceFeatures train;                // owned copy of the features, as the predictions see them (not measurements)
  // ... and as the fit sees them: as_measurements(features), gp.hpp:288 - what agp_fit_create builds its covariance of
  FeatView fit_view() const {
    FeatView v = train.v;
    v.meas = 1;
    return v;
  }
  DevMem<double> yvar, alpha, L;       // y_var (or empty), K^-1 y, the n x rank Nystrom factor (ldl)
  long long ldl = 0;
  agp_fit *mfac = nullptr;             // LL^T of delta I + L^T L (rank x rank), or nullptr for rank 0
  double delta = 0.;
  double tolerance = 0.;
  int max_iterations = 0;
  ~agp_iterative_fit() {
    if (mfac) agp_fit_destroy(mfac);
  }
};

namespace agp {

void pcg_apply_preconditioner(hipStream_t s, const agp_iterative_fit *f, const PcgCtrl *ctrl, const double *R, double *Z, long long ld,
                              int t, double *T1, long long ldt) {
  const long long n = f->n, m = f->rank;
  if (m > 0) {
    launch_pcg_lt_r(s, ctrl, f->L.get(), f->ldl, n, m, R, ld, t, T1, ldt);
    forward_solve_mat(s, f->mfac->A, m, f->mfac->lda, f->mfac->invd, T1, t, ldt);
    backward_solve_mat(s, f->mfac->A, m, f->mfac->lda, f->mfac->invd, T1, t, ldt);
  }
  launch_pcg_precond(s, ctrl, f->L.get(), f->ldl, n, m, T1, ldt, R, Z, ld, t, f->delta);
}

PcgPrecondState iterative_precond_state(const agp_iterative_fit *f) {
  PcgPrecondState st;
  st.ctx = f->ctx;
  st.n = f->n;
  st.rank = f->rank;
  st.ldl = f->ldl;
  st.delta = f->delta;
  st.L = f->L.get();
  st.mfac = f->mfac;
  return st;
}

}  // namespace agp

namespace {

struct IterDestroy {
  void operator()(agp_iterative_fit *f) const { delete f; }
};

// the scratch of one chunk of recurrences: control block | r z p q (n x t each) | t1 (m x t) | the matvec's partial sums | the
// coefficient log, where one is kept
struct PcgWork {
  DevMem<double> ws;
  PcgCtrl *ctrl = nullptr;
  double *R = nullptr, *Z = nullptr, *P = nullptr, *Q = nullptr, *T1 = nullptr, *mvws = nullptr, *log = nullptr;
  long long ld = 0, ldt = 0;
  size_t vec = 0;
  hipError_t alloc(const agp_iterative_fit *f, int tmax, bool with_log) {
    const long long n = f->n, m = f->rank;
    ld = round_up(n, 2);
    ldt = round_up(m > 0 ? m : 1, 2);
    vec = (size_t)ld * (size_t)tmax;
    const size_t ctrl_elems = (sizeof(PcgCtrl) + sizeof(double) - 1) / sizeof(double), t1 = (size_t)ldt * (size_t)tmax;
    const size_t mv = gram_matvec_ws_elems(n);
    const hipError_t e = alloc_doubles(ws, ctrl_elems + 4 * vec + t1 + mv + (with_log ? pcg_log_elems(f->max_iterations) : 0));
    if (e != hipSuccess) return e;
    ctrl = reinterpret_cast<PcgCtrl *>(ws.get());
    R = ws.get() + ctrl_elems; Z = R + vec; P = Z + vec; Q = P + vec; T1 = Q + vec; mvws = T1 + t1;
    log = with_log ? mvws + mv : nullptr;
    return hipSuccess;
  }
};

// the start of a chunk: x = 0, r = b, the norms of b and the columns that iterate at all
hipError_t pcg_queue_start(hipStream_t s, const agp_iterative_fit *f, const PcgWork &w, const double *B, long long ldb, double *Xc,
                           long long ldx, int t, double tol) {
  const long long n = f->n;
  hipError_t e = hipMemsetAsync(w.ctrl, 0, sizeof(PcgCtrl), s);
  if (e == hipSuccess) e = hipMemsetAsync(w.Z, 0, sizeof(double) * 3 * w.vec, s);  // (a zero right-hand side never writes its z, p, q)
  if (e == hipSuccess) e = hipMemset2DAsync(Xc, sizeof(double) * (size_t)ldx, 0, sizeof(double) * (size_t)n, (size_t)t, s);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(w.R, sizeof(double) * (size_t)w.ld, B, sizeof(double) * (size_t)ldb, sizeof(double) * (size_t)n, (size_t)t,
                         hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && w.log) e = hipMemsetAsync(w.log, 0xff, sizeof(double) * pcg_log_elems(f->max_iterations), s);  // (NaNs)
  if (e != hipSuccess) return e;
  launch_pcg_dot(s, DOT_BB, w.ctrl, w.R, w.R, w.ld, n, t, 0, tol);
  return hipSuccess;
}

// the launches of iteration k of a chunk; with a coefficient log, one more after p^T A p: its row k
void pcg_queue_iteration(hipStream_t s, const agp_iterative_fit *f, const PcgWork &w, const FeatView &xm, double *Xc, long long ldx, int t,
                         int k, double tol) {
  const long long n = f->n, ld = w.ld;
  pcg_apply_preconditioner(s, f, w.ctrl, w.R, w.Z, ld, t, w.T1, w.ldt);
  launch_pcg_dot(s, DOT_RZ, w.ctrl, w.R, w.Z, ld, n, t, k, tol);
  launch_pcg_p(s, w.ctrl, w.Z, w.P, ld, n, t, k == 0 ? 1 : 0);
  launch_gram_matvec(s, f->dprog.get(), &f->kernel.prog, xm, f->yvar.get(), w.P, ld, t, w.Q, ld, w.mvws, &w.ctrl->nan, &w.ctrl->active);
  launch_pcg_dot(s, DOT_PQ, w.ctrl, w.P, w.Q, ld, n, t, k, tol);
  if (w.log) launch_pcg_record(s, w.ctrl, w.log, f->max_iterations, k, t);
  launch_pcg_xr(s, w.ctrl, Xc, ldx, w.R, w.P, w.Q, ld, n, t);
  launch_pcg_dot(s, DOT_RR, w.ctrl, w.R, w.R, ld, n, t, k, tol);
}

// rows 0 .. rows - 1 of a chunk's device log to the host copy of the same layout (after the chunk's synchronisation)
hipError_t pcg_download_log(hipStream_t s, const double *log, int max_iterations, int rows, double *host) {
  const size_t mi = (size_t)max_iterations * PCG_COLS, nr = (size_t)rows * PCG_COLS;
  hipError_t e = hipMemcpyAsync(host, log, sizeof(double) * (PCG_COLS + nr), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && rows > 0)
    e = hipMemcpyAsync(host + PCG_COLS + mi, log + PCG_COLS + mi, sizeof(double) * nr, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e;
}

// X (n x nrhs, ldx, device) = A^-1 B (n x nrhs, ldb, device) by PCG, chunk by chunk; iterations / residual: nrhs host values.
// host_log (optional): pcg_log_elems(max_iterations) doubles per chunk, the coefficient logs; tolerance <= 0: the fit's
int pcg_solve(agp_context_impl *ctx, const agp_iterative_fit *f, const double *B, long long ldb, long long nrhs, double *X, long long ldx,
              int *iterations, double *residual, double *host_log = nullptr, double tolerance = 0.) {
  hipStream_t s = ctx->stream;
  const double tol = tolerance > 0. ? tolerance : f->tolerance;
  const int tmax = (int)(nrhs < PCG_COLS ? nrhs : PCG_COLS);
  PcgWork w;
  AGP_HIP_CHECK(ctx, w.alloc(f, tmax, host_log != nullptr));
  PcgCtrl *ctrl = w.ctrl;
  PcgCtrl *h_look = static_cast<PcgCtrl *>(host_stage(ctx, 3 * sizeof(PcgCtrl)));
  if (!h_look) { ctx->last_error = "agp_iterative: no pinned staging memory"; return AGP_ERR_HIP; }
  PcgCtrl *h_final = h_look + 2;
  hipEvent_t ev[2] = {ctx->ev_a, ctx->ev_b};
  const FeatView xm = f->fit_view();
  int status = AGP_OK;
  for (long long c0 = 0; c0 < nrhs && status == AGP_OK; c0 += PCG_COLS) {
    const int t = (int)(nrhs - c0 < PCG_COLS ? nrhs - c0 : PCG_COLS);
    double *Xc = X + c0 * ldx;
    AGP_HIP_CHECK(ctx, pcg_queue_start(s, f, w, B + c0 * ldb, ldb, Xc, ldx, t, tol));
    long long blocks = 0;
    bool done = false;
    for (int k0 = 0; k0 < f->max_iterations && !done; k0 += PCG_LOOK, ++blocks) {
      const int k1 = k0 + PCG_LOOK < f->max_iterations ? k0 + PCG_LOOK : f->max_iterations;
      for (int k = k0; k < k1; ++k) pcg_queue_iteration(s, f, w, xm, Xc, ldx, t, k, tol);
      if (k1 == f->max_iterations) break;
      AGP_HIP_CHECK(ctx, hipMemcpyAsync(&h_look[blocks & 1], ctrl, sizeof(PcgCtrl), hipMemcpyDeviceToHost, s));
      AGP_HIP_CHECK(ctx, hipEventRecord(ev[blocks & 1], s));
      if (blocks >= 1) {
        AGP_HIP_CHECK(ctx, hipEventSynchronize(ev[(blocks - 1) & 1]));
        done = h_look[(blocks - 1) & 1].active <= 0;
      }
    }
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_final, ctrl, sizeof(PcgCtrl), hipMemcpyDeviceToHost, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
    AGP_HIP_CHECK(ctx, hipGetLastError());
    int rows = 0;
    for (int c = 0; c < t; ++c) {
      if (iterations) iterations[c0 + c] = h_final->iters[c];
      if (residual) residual[c0 + c] = h_final->resid[c];
      if (h_final->iters[c] > rows) rows = h_final->iters[c];
    }
    if (host_log)
      AGP_HIP_CHECK(ctx, pcg_download_log(s, w.log, f->max_iterations, rows, host_log + (size_t)(c0 / PCG_COLS) * pcg_log_elems(f->max_iterations)));
    if (h_final->nan) status = AGP_ERR_NAN_INPUT;
    else if (h_final->npd) status = AGP_ERR_NOT_POSITIVE_DEFINITE;
    else if (h_final->active > 0) status = AGP_ERR_NOT_CONVERGED;
  }
  return status;
}

// diag(A) statistics, the pivoted Cholesky factor, delta and the factor of delta I + L^T L
int build_preconditioner(agp_context_impl *ctx, agp_iterative_fit *f, const agp_kernel *k, long long want_rank, double rel_tol) {
  hipStream_t s = ctx->stream;
  const long long n = f->n;
  DevMem<double> ws;
  AGP_HIP_CHECK(ctx, alloc_doubles(ws, (size_t)n + 4));
  double *stats_dev = ws.get() + n;
  launch_gram_diagonal(s, f->dprog.get(), f->fit_view(), ws.get());
  launch_pcg_diag_stats(s, ws.get(), f->yvar.get(), n, stats_dev);
  double stats[4];
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(stats, stats_dev, sizeof(stats), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (stats[3] != 0.) return AGP_ERR_NAN_INPUT;
  if (!(stats[1] > 0.)) return AGP_ERR_NOT_POSITIVE_DEFINITE;
  const double d0 = stats[0];
  double trace = stats[2];
  long long rank = 0;
  if (want_rank > 0) {
    f->ldl = round_up(n, 2);
    AGP_HIP_CHECK(ctx, f->L.alloc_cached(sizeof(double) * (size_t)f->ldl * (size_t)want_rank));
    agp_features xs{};
    xs.n = n; xs.dim = f->train.v.dim; xs.n_scale_columns = f->train.v.nsc; xs.coords = f->train.v.coords;
    xs.eq_id = reinterpret_cast<const int64_t *>(f->train.v.ids); xs.scales = f->train.v.scales;
    xs.is_measurement = 1; xs.location = AGP_DEVICE;
    std::vector<int64_t> pivots((size_t)want_rank);
    int64_t r = 0;
    const int st = pivoted_cholesky_impl(ctx, k, &xs, f->yvar.get(), want_rank, rel_tol, pivots.data(), &r, f->L.get(), f->ldl, nullptr,
                                         AGP_DEVICE, &trace, nullptr);
    if (st != AGP_OK) return st;
    rank = r;
  }
  f->rank = rank;
  const double floor_delta = 1e-8 * d0;
  f->delta = rank < n ? std::fmax(trace / (double)(n - rank), floor_delta) : floor_delta;
  if (rank == 0) { f->L.reset(); return AGP_OK; }
  // M = delta I + L^T L: C = 0 - L^T L on the fp64 GEMM (both operands read transposed), then the shift
  const long long ldm = round_up(rank, 2);
  DevMem<double> M;
  AGP_HIP_CHECK(ctx, M.alloc_cached(sizeof(double) * (size_t)ldm * (size_t)rank));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(M.get(), 0, sizeof(double) * (size_t)ldm * (size_t)rank, s));
  launch_gemm_nt_sub(s, M.get(), ldm, f->L.get(), f->ldl, true, f->L.get(), f->ldl, true, rank, rank, n, false);
  launch_pcg_shift(s, M.get(), ldm, rank, f->delta);
  return agp_factor_create(ctx, M.get(), rank, ldm, 0, AGP_DEVICE, &f->mfac);
}

int check_fit(const agp_context *ctx, const agp_iterative_fit *fit) {
  return (ctx && fit && fit->ctx == ctx) ? AGP_OK : AGP_ERR_INVALID_ARGUMENT;
}

}  // namespace

namespace agp {

int iterative_max_iterations(const agp_iterative_fit *f) { return f->max_iterations; }

void iterative_queue_probes(hipStream_t s, const agp_iterative_fit *f, unsigned long long seed, long long c0, int tc, double *Z,
                            long long ldz, double *G1, long long ldg) {
  launch_standard_normal(s, seed, f->n, c0, tc, Z, ldz);
  if (f->rank > 0) launch_standard_normal(s, pcg_probe_factor_seed(seed), f->rank, c0, tc, G1, ldg);
  launch_pcg_probe(s, f->L.get(), f->ldl, f->n, f->rank, G1, ldg, Z, ldz, Z, ldz, tc, std::sqrt(f->delta));
}

int iterative_solve_logged(agp_context *c, const agp_iterative_fit *f, const double *B, long long ldb, long long nrhs, double *X,
                           long long ldx, int *iterations, double *residual, double *host_log, double tolerance) {
  return pcg_solve(static_cast<agp_context_impl *>(c), f, B, ldb, nrhs, X, ldx, iterations, residual, host_log, tolerance);
}

int iterative_solve_stepped(agp_context *c, const agp_iterative_fit *f, const double *B, long long ldb, int t, double *X, long long ldx,
                            PcgCtrl *trace, int *steps, double *host_log) {
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  hipStream_t s = ctx->stream;
  PcgWork w;
  AGP_HIP_CHECK(ctx, w.alloc(f, t, true));
  const FeatView xm = f->fit_view();
  AGP_HIP_CHECK(ctx, pcg_queue_start(s, f, w, B, ldb, X, ldx, t, f->tolerance));
  int k = 0;
  while (k < f->max_iterations) {
    pcg_queue_iteration(s, f, w, xm, X, ldx, t, k, f->tolerance);
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(&trace[k], w.ctrl, sizeof(PcgCtrl), hipMemcpyDeviceToHost, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
    if (trace[k++].active <= 0) break;
  }
  AGP_HIP_CHECK(ctx, hipGetLastError());
  *steps = k;
  AGP_HIP_CHECK(ctx, pcg_download_log(s, w.log, f->max_iterations, k, host_log));
  const PcgCtrl &last = trace[k - 1];
  return last.nan ? AGP_ERR_NAN_INPUT : last.npd ? AGP_ERR_NOT_POSITIVE_DEFINITE : last.active > 0 ? AGP_ERR_NOT_CONVERGED : AGP_OK;
}

}  // namespace agp

extern "C" {

int agp_iterative_fit_create(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                             const agp_iterative_options *opt, agp_iterative_fit **out, double *information, int *iterations,
                             double *residual) {
  if (!c || !k || !x || !y || !opt || !out) return AGP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n < 1 || opt->precond_rank < 0 || !(opt->precond_rel_tol >= 0.) || !(opt->tolerance > 0.) || opt->max_iterations < 1)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (iterations) *iterations = 0;
  if (residual) *residual = 0.;
  std::unique_ptr<agp_iterative_fit, IterDestroy> f(new (std::nothrow) agp_iterative_fit());
  if (!f) return AGP_ERR_INVALID_ARGUMENT;
  f->ctx = ctx;
  f->n = n;
  f->tolerance = opt->tolerance;
  f->max_iterations = opt->max_iterations;
  f->kernel.prog = k->prog;
  f->kernel.uid = 0;
  AGP_HIP_CHECK(ctx, f->dprog.alloc_plain(sizeof(DevProgram)));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(f->dprog.get(), &k->prog, sizeof(DevProgram), hipMemcpyHostToDevice, s));
  if ((st = to_device(ctx, x, true, &f->train)) != AGP_OK) return st;
  f->train.v.meas = 0;
  const long long ld = round_up(n, 2);
  if (y_var) {
    AGP_HIP_CHECK(ctx, f->yvar.alloc_cached(sizeof(double) * (size_t)ld));
    if ((st = vector_to_device(ctx, y_var, n, x->location, f->yvar.get())) != AGP_OK) return st;
  }
  AGP_HIP_CHECK(ctx, f->alpha.alloc_cached(sizeof(double) * (size_t)ld));
  DevMem<double> yd;
  AGP_HIP_CHECK(ctx, alloc_doubles(yd, (size_t)ld));
  if ((st = vector_to_device(ctx, y, n, x->location, yd.get())) != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // (the program's pageable source)
  const bool prof = ctx->profiling;
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[0], s));
  {
    TraceRange tr("agp: iterative fit, preconditioner (pivoted Cholesky, L^T L, its factor)");
    const long long want = opt->precond_rank < n ? opt->precond_rank : n;
    if ((st = build_preconditioner(ctx, f.get(), k, want, opt->precond_rel_tol)) != AGP_OK) return st;
  }
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
  int its = 0;
  double res = 0.;
  {
    TraceRange tr("agp: iterative fit, preconditioned conjugate gradients");
    st = pcg_solve(ctx, f.get(), yd.get(), ld, 1, f->alpha.get(), ld, &its, &res);
  }
  if (prof) {
    AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
    AGP_HIP_CHECK(ctx, hipEventSynchronize(ctx->stage_ev[2]));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->stage_ev[0], ctx->stage_ev[1]) == hipSuccess) ctx->stage_ms[11] = ms;
    if (hipEventElapsedTime(&ms, ctx->stage_ev[1], ctx->stage_ev[2]) == hipSuccess) ctx->stage_ms[12] = ms;
  }
  if (iterations) *iterations = its;
  if (residual) *residual = res;
  if (st != AGP_OK) return st;
  if (information && (st = copy_out(ctx, f->alpha.get(), n, information, AGP_HOST)) != AGP_OK) return st;
  *out = f.release();
  return AGP_OK;
}

void agp_iterative_fit_destroy(agp_iterative_fit *fit) { delete fit; }

int64_t agp_iterative_fit_size(const agp_iterative_fit *fit) { return fit ? fit->n : 0; }

int64_t agp_iterative_fit_preconditioner_rank(const agp_iterative_fit *fit) { return fit ? fit->rank : 0; }

int agp_iterative_fit_download_information(agp_context *ctx, const agp_iterative_fit *fit, double *information) {
  if (check_fit(ctx, fit) != AGP_OK || !information) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return copy_out(ctx, fit->alpha.get(), fit->n, information, AGP_HOST);
}

int agp_iterative_solve(agp_context *c, const agp_iterative_fit *fit, const double *rhs, int64_t ldr, int64_t nrhs, double *out,
                        int64_t ldo, int location, int *iterations, double *residual) {
  if (check_fit(c, fit) != AGP_OK || !rhs || !out || nrhs < 1 || ldr < fit->n || ldo < fit->n ||
      (location != AGP_HOST && location != AGP_DEVICE))
    return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const long long n = fit->n, ld = round_up(n, 2);
  if (location == AGP_DEVICE) return pcg_solve(ctx, fit, rhs, ldr, nrhs, out, ldo, iterations, residual);
  DevMem<double> stage;
  AGP_HIP_CHECK(ctx, alloc_doubles(stage, 2 * (size_t)ld * (size_t)nrhs));
  double *Bd = stage.get(), *Xd = Bd + (size_t)ld * (size_t)nrhs;
  AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(Bd, sizeof(double) * (size_t)ld, rhs, sizeof(double) * (size_t)ldr, sizeof(double) * (size_t)n,
                                      (size_t)nrhs, hipMemcpyHostToDevice, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  const int st = pcg_solve(ctx, fit, Bd, ld, nrhs, Xd, ld, iterations, residual);
  if (st != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(out, sizeof(double) * (size_t)ldo, Xd, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n,
                                      (size_t)nrhs, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return AGP_OK;
}

int agp_iterative_predict_mean(agp_context *c, const agp_kernel *k, const agp_iterative_fit *fit, const agp_features *xs, double *mean,
                               int location) {
  if (check_fit(c, fit) != AGP_OK || !k || !xs || !mean || (location != AGP_HOST && location != AGP_DEVICE))
    return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  int st = validate_features(xs);
  if (st != AGP_OK) return st;
  if (xs->dim != fit->train.v.dim) return AGP_ERR_INVALID_ARGUMENT;
  const long long M = xs->n;
  if (M == 0) return AGP_OK;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dxs;
  if ((st = to_device(ctx, xs, false, &dxs)) != AGP_OK) return st;
  DevMem<double> md;
  double *dst = mean;
  if (location == AGP_HOST) {
    AGP_HIP_CHECK(ctx, alloc_doubles(md, (size_t)M));
    dst = md.get();
  }
  launch_predict_mean(ctx->stream, dprog, fit->train.v, dxs.v, fit->alpha.get(), dst, &k->prog);
  if (location == AGP_HOST) return copy_out(ctx, dst, M, mean, AGP_HOST);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

int agp_iterative_predict_marginal(agp_context *c, const agp_kernel *k, const agp_iterative_fit *fit, const agp_features *xs,
                                   double *mean, double *variance, int location) {
  if (!variance) return AGP_ERR_INVALID_ARGUMENT;
  int st = agp_iterative_predict_mean(c, k, fit, xs, mean, location);
  if (st != AGP_OK) return st;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  const long long M = xs->n, n = fit->n, ld = round_up(n, 2);
  if (M == 0) return AGP_OK;
  hipStream_t s = ctx->stream;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dxs;
  if ((st = to_device(ctx, xs, false, &dxs)) != AGP_OK) return st;
  // prior variances | variances | the cross covariances of a slice | their solutions
  DevMem<double> ws;
  AGP_HIP_CHECK(ctx, alloc_doubles(ws, 2 * (size_t)M + 2 * (size_t)ld * PCG_COLS));
  double *prior = ws.get(), *var = prior + M, *Kc = var + M, *S = Kc + (size_t)ld * PCG_COLS;
  launch_gram_diagonal(s, dprog, dxs.v, prior);
  for (long long j0 = 0; j0 < M; j0 += PCG_COLS) {
    const long long t = M - j0 < PCG_COLS ? M - j0 : PCG_COLS;
    FeatView slice = dxs.v;
    slice.coords += j0 * slice.dim;
    if (slice.ids) slice.ids += j0;
    if (slice.scales) { slice.sstride = scale_stride(dxs.v); slice.scales += j0; }
    slice.n = t;
    launch_gram(s, dprog, fit->train.v, slice, false, false, Kc, ld, nullptr, nullptr, &k->prog);
    if ((st = pcg_solve(ctx, fit, Kc, ld, t, S, ld, nullptr, nullptr)) != AGP_OK) return st;
    launch_pcg_variance(s, Kc, S, ld, n, t, prior + j0, var + j0);
  }
  return copy_out(ctx, var, M, variance, location);
}


// dNLL / dslot_p = 1/2 tr(A^-1 dA_p) - 1/2 alpha^T dA_p alpha with the trace estimated from probes: s_cp = w_c^T dA_p z_c,
// w_c = A^-1 z_c by the fit's own conjugate gradients, chunk by chunk (n x 16 of probes and of solutions at a time).  The
// handle is read, never written.  No value: agp_iterative_nll below returns value and gradient from one chain of solves
// (probes of covariance P there; this entry keeps its Rademacher probes and its bits).
int agp_iterative_nll_gradient(agp_context *c, const agp_iterative_fit *fit, int n_slots, const agp_gradient_slot *slots,
                               const double *tangents, int64_t ldt, int64_t n_probes, uint64_t seed, const double *probes, int64_t ldp,
                               int location, double *grad_nll, double *grad_stderr, double *samples, int64_t lds, int *iterations,
                               double *residual) {
  if (check_fit(c, fit) != AGP_OK) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && (!slots || !grad_nll || !grad_stderr)) || n_probes <= 0 ||
      (location != AGP_HOST && location != AGP_DEVICE))
    return AGP_ERR_INVALID_ARGUMENT;
  const long long n = fit->n, t = n_probes;
  if ((probes && ldp < n) || (samples && lds < t) || t > 0x7fffffffll) return AGP_ERR_INVALID_ARGUMENT;
  int ntc = 0, st = check_slots(&fit->kernel, n_slots, slots, &ntc);
  if (st != AGP_OK) return st;
  if (ntc > 0 && (!tangents || ldt < n)) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots == 0) return AGP_OK;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling, host = location == AGP_HOST;
  const long long ld = round_up(n, 2), ldf = round_up(t + 1, 2);  // column t of the forms: the alpha term
  // scratch: the NaN flag | the forms | the tangent columns of a host caller | the probes and the solutions of a chunk | the
  // workgroups' blocks of the forms kernel
  const size_t forms_elems = (size_t)ldf * (size_t)n_slots, tang_elems = host ? (size_t)ld * (size_t)ntc : 0;
  const size_t vec = (size_t)ld * PCG_COLS;
  DevMem<double> ws;
  AGP_HIP_CHECK(ctx, alloc_doubles(ws, 2 + forms_elems + tang_elems + 2 * vec + gram_tangent_ws_elems(n)));
  int *flag = reinterpret_cast<int *>(ws.get());
  double *forms_d = ws.get() + 2, *tang_stage = forms_d + forms_elems, *Z = tang_stage + tang_elems, *W = Z + vec, *tfws = W + vec;
  const double *Td = tangents;
  long long ldtd = ldt;
  if (host && ntc > 0) {
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(tang_stage, sizeof(double) * (size_t)ld, tangents, sizeof(double) * (size_t)ldt,
                                        sizeof(double) * (size_t)n, (size_t)ntc, hipMemcpyHostToDevice, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable source
    Td = tang_stage;
    ldtd = ld;
  }
  AGP_HIP_CHECK(ctx, hipMemsetAsync(flag, 0, sizeof(int), s));
  const FeatView xm = fit->fit_view();
  double solve_ms = 0., forms_ms = 0.;
  auto lap = [&](int a, int b, double &into) -> hipError_t {  // (profiling only: waits for event b)
    hipError_t e = hipEventSynchronize(ctx->stage_ev[b]);
    float ms = 0.f;
    if (e == hipSuccess && (e = hipEventElapsedTime(&ms, ctx->stage_ev[a], ctx->stage_ev[b])) == hipSuccess) into += ms;
    return e;
  };
  for (long long c0 = 0; c0 < t; c0 += PCG_COLS) {
    const long long tc = t - c0 < PCG_COLS ? t - c0 : PCG_COLS;
    const double *Zc = Z;
    if (!probes) {
      launch_rademacher(s, seed, n, c0, tc, Z, ld);
    } else if (host) {
      AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(Z, sizeof(double) * (size_t)ld, probes + c0 * ldp, sizeof(double) * (size_t)ldp,
                                          sizeof(double) * (size_t)n, (size_t)tc, hipMemcpyHostToDevice, s));
      AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable source
    } else {
      Zc = probes + c0 * ldp;
    }
    const long long ldz = Zc == Z ? ld : ldp;
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[0], s));
    {
      TraceRange tr("agp: iterative gradient, probe solves");
      st = pcg_solve(ctx, fit, Zc, ldz, tc, W, ld, iterations ? iterations + c0 : nullptr, residual ? residual + c0 : nullptr);
    }
    if (st != AGP_OK) return st;
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
    {
      TraceRange tr("agp: iterative gradient, tangent forms");
      launch_gram_tangent_forms(s, fit->dprog.get(), &fit->kernel, xm, n_slots, slots, Td, ldtd, W, ld, Zc, ldz, tc, forms_d + c0, ldf, tfws,
                                flag);
    }
    if (prof) {
      AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
      AGP_HIP_CHECK(ctx, lap(0, 1, solve_ms));
      AGP_HIP_CHECK(ctx, lap(1, 2, forms_ms));
    }
  }
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
  launch_gram_tangent_forms(s, fit->dprog.get(), &fit->kernel, xm, n_slots, slots, Td, ldtd, fit->alpha.get(), ld, fit->alpha.get(), ld, 1,
                            forms_d + t, ldf, tfws, flag);
  if (prof) {
    AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
    AGP_HIP_CHECK(ctx, lap(1, 2, forms_ms));
    ctx->stage_ms[12] = solve_ms;
    ctx->stage_ms[13] = forms_ms;
  }
  std::vector<double> h_forms(forms_elems);
  int h_flag = 0;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_forms.data(), forms_d, sizeof(double) * forms_elems, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (h_flag) return AGP_ERR_NAN_INPUT;
  for (int p = 0; p < n_slots; ++p) {
    const double *sp = h_forms.data() + (size_t)p * (size_t)ldf;
    double sum = 0.;
    for (long long cc = 0; cc < t; ++cc) sum += sp[cc];
    const double tau = sum / (double)t;
    double dev2 = 0.;
    for (long long cc = 0; cc < t; ++cc) dev2 += (sp[cc] - tau) * (sp[cc] - tau);
    grad_nll[p] = 0.5 * tau - 0.5 * sp[t];
    grad_stderr[p] = t > 1 ? 0.5 * std::sqrt(dev2 / ((double)t * (double)(t - 1))) : NAN;
    if (samples)
      for (long long cc = 0; cc < t; ++cc) samples[cc + (long long)p * lds] = sp[cc];
  }
  return AGP_OK;
}

// NLL = 1/2 alpha^T A alpha + 1/2 log det A + n/2 log 2 pi with log det A = log det P + tr log(P^-1/2 A P^-1/2), the trace by
// stochastic Lanczos quadrature: the probes z_c ~ N(0, P) go through the fit's conjugate gradients with the coefficient log
// kept, and each column's alpha_k, beta_k are the Lanczos tridiagonal of the preconditioned matrix (lanczos_quadrature.h).
// The same solves serve the gradient: w_c = A^-1 z_c, v_c = P^-1 z_c, E[w^T dA_p v] = tr(A^-1 dA_p).  The handle is read,
// never written.  The host takes the quadrature of a chunk while the device works on that chunk's forms.
int agp_iterative_nll(agp_context *c, const agp_iterative_fit *fit, int64_t n_probes, uint64_t seed, const double *probes, int64_t ldp,
                      int location, double quadrature_tolerance, int n_slots, const agp_gradient_slot *slots, const double *tangents,
                      int64_t ldt, double *nll, double *nll_stderr, double *log_det, double *log_det_samples, double *grad_nll,
                      double *grad_stderr, double *grad_samples, int64_t lds, int *iterations, double *residual) {
  if (check_fit(c, fit) != AGP_OK) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && (!slots || !grad_nll || !grad_stderr)) || n_probes <= 0 ||
      (location != AGP_HOST && location != AGP_DEVICE) || quadrature_tolerance != quadrature_tolerance)
    return AGP_ERR_INVALID_ARGUMENT;
  const long long n = fit->n, m = fit->rank, t = n_probes;
  if ((probes && ldp < n) || (grad_samples && lds < t) || t > 0x7fffffffll) return AGP_ERR_INVALID_ARGUMENT;
  int ntc = 0, st = check_slots(&fit->kernel, n_slots, slots, &ntc);
  if (st != AGP_OK) return st;
  if (ntc > 0 && (!tangents || ldt < n)) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling, host = location == AGP_HOST, grad = n_slots > 0, draw = probes == nullptr;
  const double tol = grad || !(quadrature_tolerance > 0.) ? fit->tolerance : quadrature_tolerance;
  const long long ld = round_up(n, 2), ldf = round_up(t + 1, 2), ldg = round_up(m > 0 ? m : 1, 2);  // column t of the forms: the alpha term
  // scratch: the NaN flag | alpha^T A alpha | the forms | the tangent columns of a host caller | the probes, the solutions and
  // the preconditioned probes of a chunk | A alpha | the m x 16 normals of a chunk | the preconditioner's m x 16 | its control
  // block | the workgroups' sums of the product and of the forms
  const size_t forms_elems = grad ? (size_t)ldf * (size_t)n_slots : 0, tang_elems = host ? (size_t)ld * (size_t)ntc : 0;
  const size_t vec = (size_t)ld * PCG_COLS, small = (size_t)ldg * PCG_COLS;
  const size_t ctrl_elems = (sizeof(PcgCtrl) + sizeof(double) - 1) / sizeof(double), mv_elems = gram_matvec_ws_elems(n);
  DevMem<double> ws;
  AGP_HIP_CHECK(ctx, alloc_doubles(ws, 4 + forms_elems + tang_elems + (grad ? 3 : 2) * vec + (size_t)ld + 2 * small + ctrl_elems + mv_elems +
                                           (grad ? gram_tangent_ws_elems(n) : 0)));
  int *flag = reinterpret_cast<int *>(ws.get());
  double *quad_d = ws.get() + 2, *forms_d = ws.get() + 4, *tang_stage = forms_d + forms_elems, *Z = tang_stage + tang_elems, *W = Z + vec;
  double *V = W + vec, *Aa = V + (grad ? vec : 0), *G1 = Aa + ld, *T1 = G1 + small;
  PcgCtrl *pctrl = reinterpret_cast<PcgCtrl *>(T1 + small);
  double *mvws = T1 + small + ctrl_elems, *tfws = mvws + mv_elems;
  const double *Td = tangents;
  long long ldtd = ldt;
  if (host && ntc > 0 && grad) {
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(tang_stage, sizeof(double) * (size_t)ld, tangents, sizeof(double) * (size_t)ldt,
                                        sizeof(double) * (size_t)n, (size_t)ntc, hipMemcpyHostToDevice, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable source
    Td = tang_stage;
    ldtd = ld;
  }
  AGP_HIP_CHECK(ctx, hipMemsetAsync(flag, 0, sizeof(int), s));
  if (grad) {  // the preconditioner's kernels read a control block: one column set that is all active
    PcgCtrl hc;
    std::memset(&hc, 0, sizeof(hc));
    hc.active = 1;
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(pctrl, &hc, sizeof(hc), hipMemcpyHostToDevice, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable source
  }
  const FeatView xm = fit->fit_view();
  // the data term: one product with alpha and one dot, both in a fixed order
  launch_gram_matvec(s, fit->dprog.get(), &fit->kernel.prog, xm, fit->yvar.get(), fit->alpha.get(), ld, 1, Aa, ld, mvws, flag);
  launch_dot(s, fit->alpha.get(), Aa, n, quad_d);
  double solve_ms = 0., forms_ms = 0., value_ms = 0.;
  auto lap = [&](int a, int b, double &into) -> hipError_t {  // (profiling only: waits for event b)
    hipError_t e = hipEventSynchronize(ctx->stage_ev[b]);
    float ms = 0.f;
    if (e == hipSuccess && (e = hipEventElapsedTime(&ms, ctx->stage_ev[a], ctx->stage_ev[b])) == hipSuccess) into += ms;
    return e;
  };
  std::vector<double> hlog(pcg_log_elems(fit->max_iterations)), sample((size_t)t);
  std::vector<int> its((size_t)PCG_COLS);
  for (long long c0 = 0; c0 < t; c0 += PCG_COLS) {
    const int tc = (int)(t - c0 < PCG_COLS ? t - c0 : PCG_COLS);
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[3], s));
    if (draw) {
      TraceRange tr("agp: iterative value, probes");
      iterative_queue_probes(s, fit, seed, c0, tc, Z, ld, G1, ldg);
    } else {
      AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(Z, sizeof(double) * (size_t)ld, probes + c0 * ldp, sizeof(double) * (size_t)ldp,
                                          sizeof(double) * (size_t)n, (size_t)tc, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
      if (host) AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable source
    }
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[0], s));
    {
      TraceRange tr("agp: iterative value, probe solves");
      st = pcg_solve(ctx, fit, Z, ld, tc, W, ld, its.data(), residual ? residual + c0 : nullptr, hlog.data(), tol);
    }
    if (iterations)
      for (int cc = 0; cc < tc; ++cc) iterations[c0 + cc] = its[cc];
    if (st != AGP_OK) return st;
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
    if (grad) {
      TraceRange tr("agp: iterative value, tangent forms");
      pcg_apply_preconditioner(s, fit, pctrl, Z, V, ld, tc, T1, ldg);
      launch_gram_tangent_forms(s, fit->dprog.get(), &fit->kernel, xm, n_slots, slots, Td, ldtd, W, ld, V, ld, tc, forms_d + c0, ldf, tfws, flag);
    }
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
    {
      TraceRange tr("agp: iterative value, Lanczos quadrature");
      const auto t0 = std::chrono::steady_clock::now();
      const double *la = hlog.data() + PCG_COLS, *lb = la + (size_t)fit->max_iterations * PCG_COLS;
      int quad[PCG_COLS], longest = 0;
      auto column = [&](int cc) { quad[cc] = lanczos_quadrature(hlog[cc], la + cc, lb + cc, PCG_COLS, its[cc], &sample[c0 + cc]); };
      for (int cc = 0; cc < tc; ++cc) longest = its[cc] > longest ? its[cc] : longest;
      // O(k^2) per column and one dependent chain of rotations: the columns of a chunk go to a host thread each once they
      // are long enough to repay it (each writes its own sample: the bits do not depend on the threads)
      // (a thread that cannot be started - std::system_error, bad_alloc - leaves its column and the later ones to this one:
      // no exception leaves the entry)
      std::vector<std::thread> pool;
      int threaded = 0;
      try {
        if (longest >= 128) {
          pool.reserve((size_t)tc);
          for (int cc = 1; cc < tc; ++cc) { pool.emplace_back(column, cc); threaded = cc; }
        }
      } catch (...) {
      }
      column(0);
      for (int cc = threaded + 1; cc < tc; ++cc) column(cc);
      for (auto &th : pool) th.join();
      for (int cc = 0; cc < tc; ++cc)
        if (quad[cc] != AGP_OK) return quad[cc];
      if (prof) value_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (prof) {
      AGP_HIP_CHECK(ctx, lap(3, 0, value_ms));
      AGP_HIP_CHECK(ctx, lap(0, 1, solve_ms));
      AGP_HIP_CHECK(ctx, lap(1, 2, forms_ms));
    }
  }
  if (grad) {
    if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
    launch_gram_tangent_forms(s, fit->dprog.get(), &fit->kernel, xm, n_slots, slots, Td, ldtd, fit->alpha.get(), ld, fit->alpha.get(), ld, 1,
                              forms_d + t, ldf, tfws, flag);
    if (prof) {
      AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
      AGP_HIP_CHECK(ctx, lap(1, 2, forms_ms));
    }
  }
  std::vector<double> h_forms(forms_elems);
  int h_flag = 0;
  double quad = 0.;
  if (grad) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_forms.data(), forms_d, sizeof(double) * forms_elems, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(&quad, quad_d, sizeof(double), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (h_flag || quad != quad) return AGP_ERR_NAN_INPUT;
  // log det P = (n - m) log delta + log det(delta I + L^T L)
  double ld_p = (double)(n - m) * std::log(fit->delta);
  if (m > 0) {
    double ld_m = 0.;
    if ((st = agp_fit_log_determinant(fit->mfac, &ld_m)) != AGP_OK) return st;
    ld_p += ld_m;
  }
  double sum = 0.;
  for (long long cc = 0; cc < t; ++cc) sum += sample[cc];
  const double mean = sum / (double)t;
  double dev2 = 0.;
  for (long long cc = 0; cc < t; ++cc) dev2 += (sample[cc] - mean) * (sample[cc] - mean);
  const double ld_a = ld_p + mean, ld_se = t > 1 ? std::sqrt(dev2 / ((double)t * (double)(t - 1))) : NAN;
  if (prof) {
    ctx->stage_ms[12] = solve_ms;
    ctx->stage_ms[13] = forms_ms;
    ctx->stage_ms[14] = value_ms;
  }
  if (log_det) *log_det = ld_a;
  if (nll) *nll = 0.5 * quad + 0.5 * ld_a + 0.5 * (double)n * std::log(2. * M_PI);
  if (nll_stderr) *nll_stderr = 0.5 * ld_se;
  if (log_det_samples)
    for (long long cc = 0; cc < t; ++cc) log_det_samples[cc] = sample[cc];
  for (int p = 0; p < n_slots; ++p) {
    const double *sp = h_forms.data() + (size_t)p * (size_t)ldf;
    double fsum = 0.;
    for (long long cc = 0; cc < t; ++cc) fsum += sp[cc];
    const double tau = fsum / (double)t;
    double fdev2 = 0.;
    for (long long cc = 0; cc < t; ++cc) fdev2 += (sp[cc] - tau) * (sp[cc] - tau);
    grad_nll[p] = 0.5 * tau - 0.5 * sp[t];
    grad_stderr[p] = t > 1 ? 0.5 * std::sqrt(fdev2 / ((double)t * (double)(t - 1))) : NAN;
    if (grad_samples)
      for (long long cc = 0; cc < t; ++cc) grad_samples[cc + (long long)p * lds] = sp[cc];
  }
  return AGP_OK;
}

}  // extern "C"
