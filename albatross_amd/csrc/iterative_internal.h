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

// The coefficient log of one chunk of pcg_solve (agp_iterative_nll reads the Lanczos tridiagonals from it):
//   rz0[PCG_COLS] | alpha[max_iterations][PCG_COLS] | beta[max_iterations][PCG_COLS]   doubles
// Column c's valid rows are 0 .. iters[c] - 1; the kernel leaves what no iteration wrote as it was, and pcg_solve fills the
// log with NaNs (all bits set) before the chunk starts.
inline size_t pcg_log_elems(int max_iterations) { return (size_t)PCG_COLS * (1 + 2 * (size_t)max_iterations); }
// pcg_record_kernel: one wave, after DOT_PQ of iteration k: row k of the log = alpha[c], beta[c] of every column c < t that is
// not stopped (k = 0: also rz0[c] = rz[0][c]); nothing when active <= 0.  k < max_iterations.
void launch_pcg_record(hipStream_t s, const PcgCtrl *ctrl, double *log, int max_iterations, int k, int t);
// pcg_probe_kernel: Z (n x t, ldz) = L G1 + sqrt_delta G2, 256 rows per workgroup, the sum over j = 0, 1, ... in order;
// L n x m at ldl, G1 m x t at ldg1, G2 n x t at ldg2 (m = 0: L and G1 are not read).  Z may be G2 itself.
void launch_pcg_probe(hipStream_t s, const double *L, long long ldl, long long n, long long m, const double *G1, long long ldg1,
                      const double *G2, long long ldg2, double *Z, long long ldz, int t, double sqrt_delta);
// the seed of the m x t normals G1 of the probes of agp_iterative_nll: a stream of agp_standard_normal apart from the
// seed's own, which gives G2
inline unsigned long long pcg_probe_factor_seed(unsigned long long seed) { return seed ^ 0x9E3779B97F4A7C15ull; }

// columns c0 .. c0 + tc - 1 (tc <= PCG_COLS) of the probes agp_iterative_nll draws for `seed`, z ~ N(0, P):
// Z (n x tc, ldz) = L G1 + sqrt(delta) G2 with G2 = those columns of agp_standard_normal(seed) on n rows and G1 the same
// columns of agp_standard_normal(pcg_probe_factor_seed(seed)) on rank rows (scratch, rank x tc at ldg; not touched at rank 0)
void iterative_queue_probes(hipStream_t s, const agp_iterative_fit *f, unsigned long long seed, long long c0, int tc, double *Z,
                            long long ldz, double *G1, long long ldg);

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

// agp_iterative_solve on device arrays with the coefficient log kept: host_log holds pcg_log_elems(max_iterations) doubles
// per chunk of PCG_COLS columns, written as far as the chunk's longest recurrence went (rows 0 .. max_c iters[c] - 1).
// tolerance <= 0: the fit's.  iterative_max_iterations: the fit's (the row count of the log's layout).
int iterative_solve_logged(agp_context *ctx, const agp_iterative_fit *f, const double *B, long long ldb, long long nrhs, double *X,
                           long long ldx, int *iterations, double *residual, double *host_log, double tolerance);
int iterative_max_iterations(const agp_iterative_fit *f);
// ONE chunk (t <= PCG_COLS) through the start and the per-iteration launches pcg_solve queues, with a look after every
// iteration instead of every PCG_LOOK: trace[k] = the control block after iteration k (max_iterations entries), *steps the
// iterations queued, host_log the chunk's coefficient log.  For the probes of debug_api.hip.
int iterative_solve_stepped(agp_context *ctx, const agp_iterative_fit *f, const double *B, long long ldb, int t, double *X, long long ldx,
                            PcgCtrl *trace, int *steps, double *host_log);

}  // namespace agp
