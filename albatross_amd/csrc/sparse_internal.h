// sparse_internal.h — what sparse_api.hip (the fit) shares with sparse_gradient.hip (its gradient and the
// held-out predictions of its groups).  Not part of the public interface.
#pragma once
#include <chrono>
#include <cstdio>
#include <memory>
#include <vector>

#include "api_internal.h"

struct agp_sparse_fit {
  agp_context *ctx = nullptr;
  long long m = 0;
  std::shared_ptr<agp::DeviceFeatures> u;   // train_features = inducing points (shared with updated fits)
  std::shared_ptr<agp_fit> kuu;        // train_covariance = factor of K_uu + inducing_nugget I
  agp_fit *sigma = nullptr;            // L1
  agp_fit *sigma2 = nullptr;           // L2
  agp::DevMem<double> Lacc;            // L1 L2, m x ldm, zero above the diagonal
  agp::DevMem<double> v;               // information (m)
  double nll = 0.;
  // "pivoted form" of a fit made by agp_sparse_fit_from_prediction (rebase_inducing_points) or by an update of one:
  // the reference's own representation, for covariances that are singular to working precision.
  std::shared_ptr<agp_ldlt> kz;        // train_covariance as a pivoted L D L^T: K_zz WITHOUT nugget after fit_from_prediction
                                       // (:416-418), K_uu + inducing nugget after a pivoted fit (:676-679); else kuu
  std::shared_ptr<agp_ldlt> kp;        // pivoted L D L^T of K_uu + inducing nugget for P = K_uu^-1/2 K_uf of an update, when
                                       // the LL^T of that matrix (kuu) does not exist
  agp::DevMem<double> R;               // m x round_up(m, 2), upper triangular: Sigma^-1 = P R^T R P^T; else sigma/sigma2
  agp::DevMem<long long> perm;         // P: perm[i] = original index of the column at position i
  long long rank = -1;                 // numerical_rank of the QR (-1: not a pivoted fit)
  double inducing_nugget = 0.;         // the nugget an update adds to K_uu for P = K_uu^-1/2 K_uf (:674-685)
};

namespace agp {

struct SparseScratch {
  double *Kuf = nullptr, *Pbuf = nullptr, *Q1T = nullptr;  // (regions of ctx->pool_sparse, below)
  DevMem<double> M0, T, vecs, partial, Ag, Pimg, Winv;
  std::vector<agp_fit *> blocks;
  DeviceFeatures dx;
  // Kuf, Pbuf / Q1T (one region: P is dead before Q1^T is formed) and the split-K slabs live in ctx->pool_sparse
  double *slabs = nullptr, *pads = nullptr;
  long long slab_count = 0;
  // agp_sparse_nll_gradient (sparse_gradient.hip): Q1^T gets a region of its own, so that P = L_u^-1 K_uf outlives the fit
  bool keep_P = false;
  int layout = 0;  // which path built the blocks of A: 0 lock step (Ag, Pimg), 1 the same on padded slabs, 2 one agp_fit per block
  ~SparseScratch() {
    for (agp_fit *b : blocks) agp_fit_destroy(b);
  }
};

// AGP_SPARSE_TIMING=1: wall time of every stage (with a stream synchronisation at each boundary) on stderr
struct StageTimer {
  hipStream_t s;
  bool on;
  std::chrono::steady_clock::time_point last;
  explicit StageTimer(hipStream_t st, bool enabled) : s(st), on(enabled), last(std::chrono::steady_clock::now()) {}
  void operator()(const char *name) {
    if (!on) return;
    (void)hipStreamSynchronize(s);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "  [sparse fit] %-28s %8.2f ms\n", name, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

// agp_sparse_fit_create's LL^T / CholeskyQR2 path for one process.  keep (optional): the caller's scratch, which then
// still holds W = K_uf A^-T/2 (Kuf), Q1^T, the block factors of A and - with keep->keep_P - P after the call;
// yw_out: A^-1/2 y inside keep->vecs.
int sparse_fit_fast(agp_context *ctx, const agp_kernel *k, const agp_features *x, int64_t n_groups, const int64_t *offsets,
                    const double *y, const double *y_var, const agp_features *u, double measurement_nugget,
                    double inducing_nugget, agp_sparse_fit **out, double *nll_out, SparseScratch *keep, double **yw_out);
// C (m x m, lower tiles) -= A B^T for A, B m x n (ld ldw) with n >> m, through the split-K slabs of the scratch
void gemm_over_observations(hipStream_t s, SparseScratch &w, double *C, long long ldc, const double *A, const double *B,
                            long long ldw, long long m, long long n);

}  // namespace agp
