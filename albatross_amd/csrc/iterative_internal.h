// iterative_internal.h — what iterative.hip shares with the probes of debug_api.hip: the control block of the preconditioned
// conjugate gradients, one host launcher per kernel of the file (each carries the grid and block arithmetic of the product,
// which calls it too), the preconditioner application of one iteration, and the preconditioner state of a fit.  Not part of
// the public interface.
#pragma once
#include "common.h"
#include "gram_matvec.h"

struct agp_iterative_fit;

namespace agp {

constexpr int PCG_LOOK = 8;             // iterations between two looks of the host
constexpr int PCG_COLS = MV_MAX_RHS;    // right-hand sides of a chunk
constexpr int PCG_DOT_THREADS = 1024;
constexpr int PCG_ERROR = 1 << 20;      // subtracted from `active` by the kernel that marks an error: nothing runs after

struct PcgCtrl {
  int active;              // columns still iterating; <= 0: every kernel returns at once (also gram_matvec's `go` word)
  int npd;                 // p^T A p <= 0 in an active column
  int nan;                 // a NaN in a reduction or in an entry of A
  int pad;
  int stopped[PCG_COLS];
  int iters[PCG_COLS];     // iterations carried out by the column
  double bb[PCG_COLS], rz[2][PCG_COLS], alpha[PCG_COLS], beta[PCG_COLS], resid[PCG_COLS];
};

enum { DOT_BB = 0, DOT_RZ = 1, DOT_PQ = 2, DOT_RR = 3 };

// pcg_dot_kernel<mode>: one workgroup per column of the t
void launch_pcg_dot(hipStream_t s, int mode, PcgCtrl *ctrl, const double *A, const double *B, long long ld, long long n, int t, int k,
                    double tol);
// pcg_lt_r_kernel: T1 (m x t, ldt) = L^T R, one workgroup per column of L (m >= 1)
void launch_pcg_lt_r(hipStream_t s, const PcgCtrl *ctrl, const double *L, long long ldl, long long n, long long m, const double *R,
                     long long ldr, int t, double *T1, long long ldt);
// pcg_precond_kernel: Z = (R - L U) / delta, 256 rows per workgroup (m = 0: L and U are not read)
void launch_pcg_precond(hipStream_t s, const PcgCtrl *ctrl, const double *L, long long ldl, long long n, long long m, const double *U,
                        long long ldu, const double *R, double *Z, long long ld, int t, double delta);
// pcg_p_kernel: P = Z + beta P (first: P = Z)
void launch_pcg_p(hipStream_t s, const PcgCtrl *ctrl, const double *Z, double *P, long long ld, long long n, int t, int first);
// pcg_xr_kernel: X += alpha P, R -= alpha Q
void launch_pcg_xr(hipStream_t s, const PcgCtrl *ctrl, double *X, long long ldx, double *R, const double *P, const double *Q, long long ld,
                   long long n, int t);
// pcg_diag_stats_kernel: stats[0..3] = max, min, sum, NaN mark of d + yvar (yvar may be null); one workgroup
void launch_pcg_diag_stats(hipStream_t s, const double *d, const double *yvar, long long n, double *stats);
// pcg_shift_kernel: C (m x m, ldc) = delta I - C
void launch_pcg_shift(hipStream_t s, double *C, long long ldc, long long m, double delta);
// pcg_variance_kernel: var_j = prior_j - sum_i Kc[i, j] S[i, j] for the t test points of a slice
void launch_pcg_variance(hipStream_t s, const double *Kc, const double *S, long long ld, long long n, long long t, const double *prior,
                         double *var);

// Z = P^-1 R for the t columns of a chunk (both n x t at ld), as one iteration of pcg_solve queues it: L^T R, the two
// substitutions against the factor of delta I + L^T L, then (R - L U) / delta.  T1: ldt x t doubles of scratch, ldt >= rank.
void pcg_apply_preconditioner(hipStream_t s, const agp_iterative_fit *f, const PcgCtrl *ctrl, const double *R, double *Z, long long ld,
                              int t, double *T1, long long ldt);

// the preconditioner of a fit: L (n x rank at ldl, device; null at rank 0), delta, the factor of delta I + L^T L (null at rank 0)
struct PcgPrecondState {
  const agp_context *ctx = nullptr;
  long long n = 0, rank = 0, ldl = 0;
  double delta = 0.;
  const double *L = nullptr;
  const agp_fit *mfac = nullptr;
};
PcgPrecondState iterative_precond_state(const agp_iterative_fit *f);

}  // namespace agp
