// host_sanitize_check.cpp — the host-side C++ of the project under AddressSanitizer + UndefinedBehaviorSanitizer, on
// a machine WITHOUT a GPU (examples/Makefile: `make asan`).  Seven parts:
//
//  1. the sharded-fit schedule (albatross_amd/csrc/shard_sched.hip is plain C++: compiled INTO this binary with the
//     sanitizers on) driven through agp_debug_shard_factor_custom (csrc/shard_custom.hip) with naive block operations, one rank and - through
//     in-process "collectives" - the forced multi-rank path; checked against a naive dense solve;
//  2. the header-only host layer (include/albatross_amd/albatross.hpp): covariance-function programs, parameter
//     handling, feature flattening (Measurement<>, scale columns), grouping - everything that runs before the
//     first device call;
//  3. the workspace layouts of the batched fits (albatross_amd/csrc/ws_layout.h, batch_layout.h: plain C++) over a
//     malloc'd base: every region aligned, inside the allocation and disjoint from the others, the sizing pass equal to
//     the real one, the size within the alignment padding of the plain sums, first and last word of every region written;
//  4. the schedule of the dense factorisation (albatross_amd/csrc/factor_plan.h: plain C++): every n up to 20480 planned
//     under four switch sets (two of them resolved from the FactorRequest of a call), every step's panels planned, and a sweep of the step-launch shapes.
//  5. the owners of device memory (albatross_amd/csrc/dev_mem.h: plain C++) over malloc / free: the four allocator
//     functions are defined HERE with a table of live blocks, a log of the calls and a switch that fails the k-th
//     allocation; every move, hand-over, refusal and failure of DevMem, ParkSlot and GrowBuf, no block left at the end.
//
//  6. the pooled plan of the batched leave-one-group-out gradient (albatross_amd/csrc/logo_batch_plan.h: plain C++) on
//     ragged groupings over 1-12 problems, every table walked, with the carve of its workspace (carve_logo_batch, part 3).
//
//  7. the tiling of the MFMA update launches (albatross_amd/csrc/update_plan.h: plain C++): every bulk update up to 160
//     tile rows planned under three slot counts and five heads, the tile decode walked there and back, every order table
//     built and read entry by entry, and sweeps of the product and staircase plans.
//
//  8. the host quadrature of the matrix-free fit's log-likelihood value (albatross_amd/csrc/lanczos_quadrature.h: plain
//     C++): coefficient sets of 1 to 600 rows, strided as the coefficient log strides them, against the closed forms at one
//     and two rows and against the double instantiation, and every refused input.
//
// Prints "host_sanitize_check ok" and exits 0; any sanitizer report aborts with a non-zero status.
#include <cmath>
#include <random>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "albatross_amd/albatross.hpp"
#include "dev_mem.h"         // csrc/: DevMem, ParkSlot, GrowBuf
#include "batch_layout.h"    // csrc/: WsLayout, BatchGeometry, the carve functions
#include "factor_plan.h"     // csrc/: FactorPlanner, plan_panels, step_launch_shape
#include "logo_batch_plan.h" // csrc/: the pooled plan of agp_logo_nll_gradient_batch
#include "update_plan.h"     // csrc/: plan_bulk_update, plan_nt_sub, plan_stair, lower_tile_of, xcd_tile_order
#include "lanczos_quadrature.h"  // csrc/: the Gauss quadrature of log from conjugate-gradient coefficients
#include "shard_internal.h"  // agp_shard_ops_callbacks (csrc/, test-only)

extern "C" {
int64_t agp_debug_shard_work_doubles(int64_t n, int64_t block, int nranks, int rank);
int agp_debug_shard_factor_custom(const agp_shard_ops_callbacks *ops, agp_comm *comm, int64_t n, int64_t block, double *A, int64_t ld,
                                  double *y, double *work, double *information, double *log_det, int64_t *bad_pivot);
}

using namespace albatross;

namespace {
double *at(double *p, std::int64_t ld, std::int64_t r, std::int64_t c) { return p + r + c * ld; }

std::int64_t cb_factor_diag(void *, double *D, std::int64_t ld, std::int64_t w, double *, double *z, double *logsum) {
  std::int64_t bad = 0;
  double ls = 0.;
  for (std::int64_t j = 0; j < w; ++j) {
    double d = *at(D, ld, j, j);
    for (std::int64_t k = 0; k < j; ++k) d -= *at(D, ld, j, k) * *at(D, ld, j, k);
    if (!(d > 0.) && bad == 0) bad = j + 1;
    const double l = std::sqrt(d);
    *at(D, ld, j, j) = l;
    ls += std::log(l);
    for (std::int64_t i = j + 1; i < w; ++i) {
      double v = *at(D, ld, i, j);
      for (std::int64_t k = 0; k < j; ++k) v -= *at(D, ld, i, k) * *at(D, ld, j, k);
      *at(D, ld, i, j) = v / l;
    }
  }
  for (std::int64_t i = 0; i < w; ++i) {
    double v = z[i];
    for (std::int64_t k = 0; k < i; ++k) v -= *at(D, ld, i, k) * z[k];
    z[i] = v / *at(D, ld, i, i);
  }
  *logsum = ls;
  return bad;
}
void cb_trsm_rows(void *, double *X, std::int64_t ld, std::int64_t nrows, std::int64_t w, const double *L, const double *, const double *z,
                  double *y) {
  for (std::int64_t r = 0; r < nrows; ++r) {
    for (std::int64_t c = 0; c < w; ++c) {
      double v = *at(X, ld, r, c);
      for (std::int64_t k = 0; k < c; ++k) v -= *at(X, ld, r, k) * L[c + k * w];
      *at(X, ld, r, c) = v / L[c + c * w];
    }
    for (std::int64_t c = 0; c < w; ++c) y[r] -= *at(X, ld, r, c) * z[c];
  }
}
void cb_gemm(void *, double *C, std::int64_t ldc, const double *P, std::int64_t ldp, const double *Q, std::int64_t ldq, std::int64_t M,
             std::int64_t N, std::int64_t K, int tri) {
  for (std::int64_t j = 0; j < N; ++j)
    for (std::int64_t i = tri ? j : 0; i < M; ++i) {
      double s = 0.;
      for (std::int64_t k = 0; k < K; ++k) s += P[i + k * ldp] * Q[j + k * ldq];
      C[i + j * ldc] -= s;
    }
}
void cb_copy2d(void *, double *dst, std::int64_t ldd, const double *src, std::int64_t lds, std::int64_t rows, std::int64_t cols) {
  for (std::int64_t c = 0; c < cols; ++c)
    for (std::int64_t r = 0; r < rows; ++r) dst[r + c * ldd] = src[r + c * lds];
}
void cb_invert_diag(void *, const double *D, std::int64_t ld, std::int64_t w, const double *, double *W) {
  for (std::int64_t c = 0; c < w; ++c)
    for (std::int64_t r = 0; r < w; ++r) {
      double v = r == c ? 1. : 0.;
      for (std::int64_t k = 0; k < r; ++k) v -= D[r + k * ld] * W[k + c * w];
      W[r + c * w] = v / D[r + r * ld];
    }
}
void cb_colvec_dot(void *, const double *W, std::int64_t ld, std::int64_t m, std::int64_t n, const double *v, double alpha, double beta,
                   const double *base, double *out) {
  for (std::int64_t c = 0; c < n; ++c) {
    double s = 0.;
    for (std::int64_t r = 0; r < m; ++r) s += W[r + c * ld] * v[r];
    out[c] = alpha * s + (base ? beta * base[c] : 0.);
  }
}
void cb_axpby(void *, std::int64_t n, double a, const double *x, double b, const double *y, double *out) {
  for (std::int64_t i = 0; i < n; ++i) out[i] = a * x[i] + b * y[i];
}
void cb_fill_zero(void *, double *p, std::int64_t count) {
  for (std::int64_t i = 0; i < count; ++i) p[i] = 0.;
}
int cb_broadcast(void *, double *, std::int64_t, int root) { return root == 0 ? 0 : 1; }
int cb_all_gather(void *, const double *send, double *recv, std::int64_t count) {
  for (std::int64_t i = 0; i < count; ++i) recv[i] = send[i];
  return 0;
}
int cb_all_reduce(void *, double *, std::int64_t, int) { return 0; }

void require(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "host_sanitize_check: FAILED: %s\n", what);
    std::exit(1);
  }
}

void schedule_under_sanitizers(bool force_comm) {
  const std::int64_t n = 333, block = 128;
  std::vector<double> K(n * n), y(n), ref(n);
  unsigned long long s = 88172645463325252ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) * (1.0 / 9007199254740992.0); };
  std::vector<double> pts(n);
  for (auto &p : pts) p = 10. * rnd();
  for (std::int64_t i = 0; i < n; ++i) {
    y[i] = std::sin(pts[i]);
    for (std::int64_t j = 0; j < n; ++j) K[i + j * n] = std::exp(-(pts[i] - pts[j]) * (pts[i] - pts[j])) + (i == j ? 0.01 : 0.);
  }
  // reference: naive dense LL^T solve
  {
    std::vector<double> L(K), z(y);
    double ls = 0.;
    require(cb_factor_diag(nullptr, L.data(), n, n, nullptr, z.data(), &ls) == 0, "reference factorisation");
    for (std::int64_t i = n - 1; i >= 0; --i) {
      double v = z[i];
      for (std::int64_t k = i + 1; k < n; ++k) v -= L[k + i * n] * ref[k];
      ref[i] = v / L[i + i * n];
    }
  }
  if (force_comm) setenv("AGP_SHARD_FORCE_COMM", "1", 1);
  else unsetenv("AGP_SHARD_FORCE_COMM");
  agp_comm *comm = nullptr;
  agp_comm_callbacks ccb{nullptr, cb_broadcast, cb_all_gather, cb_all_reduce};
  if (force_comm) require(agp_comm_create_callbacks(1, 0, &ccb, &comm) == AGP_OK, "agp_comm_create_callbacks");
  const std::int64_t n_loc = agp_shard_local_rows(n, block, 1, 0);
  require(n_loc == n, "one rank owns every row");
  const std::int64_t ld = n_loc + 1;
  std::vector<double> A((size_t)ld * n, std::nan("")), yl(y), work((size_t)agp_debug_shard_work_doubles(n, block, 1, 0), std::nan("")), info(n);
  for (std::int64_t l = 0; l < n_loc; ++l) {
    const std::int64_t g = agp_shard_global_row(n, block, 1, 0, l);
    const std::int64_t end = std::min<std::int64_t>(n, (g / block + 1) * block);
    for (std::int64_t c = 0; c < end; ++c) A[l + c * ld] = K[g + c * n];
  }
  agp_shard_ops_callbacks ops{nullptr, cb_factor_diag, cb_trsm_rows, cb_gemm, cb_copy2d, cb_invert_diag, cb_colvec_dot, cb_axpby, cb_fill_zero};
  double logdet = 0.;
  std::int64_t bad = -1;
  const int st = agp_debug_shard_factor_custom(&ops, comm, n, block, A.data(), ld, yl.data(), work.data(), info.data(), &logdet, &bad);
  require(st == AGP_OK && bad == -1, "agp_debug_shard_factor_custom");
  double worst = 0., scale = 0.;
  for (std::int64_t i = 0; i < n; ++i) { worst = std::fmax(worst, std::fabs(info[i] - ref[i])); scale = std::fmax(scale, std::fabs(ref[i])); }
  require(worst <= 1e-9 * scale, "sharded schedule == dense solve");
  agp_comm_destroy(comm);
}

void host_layer_under_sanitizers() {
  auto cov = SquaredExponential<EuclideanDistance>(2.0, 1.5) * Matern52<EuclideanDistance>(3.0, 0.7) + measurement_only(IndependentNoise<double>(0.1)) +
             Constant(2.0);
  const auto prog = cov.program();
  require(!prog.empty() && prog.size() <= AGP_MAX_KERNEL_NODES, "program size");
  int depth = 0;
  for (const auto &nd : prog) {  // a well-formed postfix program ends with exactly one value on the stack
    if (nd.op == AGP_OP_SUM || nd.op == AGP_OP_PRODUCT) --depth;
    else if (nd.op != AGP_OP_MEASUREMENT_ONLY && nd.op != AGP_OP_TYPE_PAIR) ++depth;
    require(depth >= 1, "stack underflow");
  }
  require(depth == 1, "one value left");
  agp_kernel *k = nullptr;
  require(agp_kernel_create(prog.data(), (int)prog.size(), &k) == AGP_OK, "agp_kernel_create");
  agp_kernel_destroy(k);
  agp_kernel_node bad_prog[2] = {prog[0], prog[0]};  // two leaves, no operator
  require(agp_kernel_create(bad_prog, 2, &k) == AGP_ERR_INVALID_ARGUMENT, "malformed program rejected");
  auto params = cov.get_params();
  require(!params.empty(), "parameters");
  for (const auto &kv : params) cov.set_param(kv.first, kv.second * 1.5);
  for (const auto &kv : cov.get_params()) require(std::fabs(kv.second - 1.5 * params.at(kv.first)) < 1e-15, "set_param round trip");
  std::vector<double> xs = {0.5, 1.5, 2.5, 1.5};
  auto flat = detail::flatten(cov, xs);
  require(flat.view.n == 4 && flat.view.dim == 1 && flat.view.is_measurement == 0 && flat.coords[2] == 2.5, "flatten");
  auto flat_m = detail::flatten(cov, as_measurements(xs));
  require(flat_m.view.is_measurement == 1 && flat_m.coords.size() == 4, "flatten Measurement<>");
  auto groups = group_indexer(xs, [](const double &x) { return (int)std::floor(x); });
  require(groups.size() == 3 && groups.at(1).size() == 2, "group_indexer");
  auto loo = group_indexer(xs, LeaveOneOutGrouper{});
  require(loo.size() == 4, "leave-one-out grouper");
  RegressionDataset<double> ds(xs, MarginalDistribution(Vector{1., 2., 3., 4.}, Vector{0.1, 0.1, 0.1, 0.1}));
  require(ds.size() == 4, "dataset");
}

// ---- part 3: the workspace layouts ---------------------------------------------------------------------------------
struct Region {
  void *p;
  size_t bytes;
};

// `carve` run over a null base and over a malloc'd one; want_elems: the plain sum of 8-byte elements the layout replaces
void check_layout(const char *what, size_t want_elems, const std::function<std::vector<Region>(agp::WsLayout &)> &carve) {
  agp::WsLayout size;
  for (const Region &r : carve(size)) require(r.p == nullptr, what);
  const size_t bytes = size.bytes();
  char *base = static_cast<char *>(std::malloc(bytes ? bytes : 1));  // (malloc aligns to 16 bytes)
  require(base != nullptr && reinterpret_cast<std::uintptr_t>(base) % 16 == 0, "malloc");
  agp::WsLayout ws(base);
  const std::vector<Region> regions = carve(ws);
  require(ws.bytes() == bytes, what);
  require(bytes >= 8 * want_elems && bytes <= 8 * want_elems + 16 * regions.size(), what);
  for (size_t i = 0; i < regions.size(); ++i) {
    const Region &r = regions[i];
    if (!r.p) continue;  // a region this configuration does not have
    char *p = static_cast<char *>(r.p);
    require(reinterpret_cast<std::uintptr_t>(p) % 16 == 0, what);
    require(p >= base && p + r.bytes <= base + bytes, what);
    for (size_t j = 0; j < i; ++j) {
      const char *q = static_cast<const char *>(regions[j].p);
      require(!q || p + r.bytes <= q || q + regions[j].bytes <= p, what);
    }
    if (r.bytes >= 4) {  // first and last word (the status words are ints)
      *reinterpret_cast<int *>(p) = 1;
      *reinterpret_cast<int *>(p + r.bytes - 4) = 2;
    }
  }
  std::free(base);
}

void layouts_under_sanitizers() {
  const long long NB = 128, IMG = 36 * 16 * 16;  // csrc/common.h: NB; the tile image of one diagonal block, 36 MB x MB tiles
  const long long shapes[][2] = {{1, 1}, {100, 1}, {129, 3}, {520, 8}, {1100, 50}};
  for (const auto &shape : shapes)
    for (int has_var = 0; has_var < 2; ++has_var)
      for (int fused = 0; fused < 2; ++fused) {
        const long long n = shape[0], count = shape[1];
        long long lda = (n + 7) / 8 * 8;  // csrc/api.hip: factor_ld
        if (lda % 256 == 0) lda += 8;
        const agp::BatchGeometry g(n, count, lda, NB, IMG);
        const size_t nblk = (size_t)((n + NB - 1) / NB), np2 = (size_t)((n + 1) / 2 * 2), cp2 = (size_t)((count + 1) / 2 * 2), B = (size_t)count;
        const size_t sA = (size_t)(lda * n), sI = nblk * (size_t)IMG;
        require((size_t)g.nblk == nblk && (size_t)g.np2 == np2 && (size_t)g.cp2 == cp2 && (size_t)g.stride_A == sA && (size_t)g.stride_I == sI,
                "BatchGeometry");
        const size_t D = sizeof(double);
        const size_t gram_bytes = 184 * B + 8, desc_bytes = 1000 * B, copy_bytes = 24 * 3 * B;  // tables: any sizes, 16-byte multiples or not
        const size_t up8 = 7;  // (bytes + up8) / 8: a table's bytes as 8-byte elements
        // agp_nll_batch
        check_layout("carve_nll_batch", B * (sA + sI + np2) + np2 + 2 * cp2 + (fused ? B * np2 : 0) + (gram_bytes + up8) / 8, [&](agp::WsLayout &w) {
          const agp::NllBatchRegions r = agp::carve_nll_batch(w, g, fused, gram_bytes);
          return std::vector<Region>{{r.A, D * B * sA}, {r.invd, D * B * sI}, {r.ys, D * B * np2}, {r.yvar, D * np2}, {r.logsum, D * cp2},
                                     {r.quad, D * cp2}, {r.zpub, D * B * np2}, {r.gram_table, gram_bytes}};
        });
        // agp_fit_create_batch: the slab, then the scratch of the call
        check_layout("carve_fit_batch", B * (sA + sI + 2 * np2) + cp2 + 2 * cp2 + (has_var ? B * np2 : 0), [&](agp::WsLayout &w) {
          const agp::FitBatchRegions r = agp::carve_fit_batch(w, g, has_var);
          return std::vector<Region>{{r.A, D * B * sA}, {r.invd, D * B * sI}, {r.alpha, D * B * np2}, {r.z, D * B * np2}, {r.logsum, D * cp2},
                                     {r.flags, sizeof(int) * 4 * cp2}, {r.yvar, D * B * np2}};
        });
        check_layout("carve_fit_batch_tables", (copy_bytes + 15) / 16 * 2 + (gram_bytes + 15) / 16 * 2 + (fused ? B * np2 : 0), [&](agp::WsLayout &w) {
          const agp::FitBatchTables r = agp::carve_fit_batch_tables(w, g, fused, copy_bytes, gram_bytes);
          return std::vector<Region>{{r.copy_table, copy_bytes}, {r.gram_table, gram_bytes}, {r.zpub, D * B * np2}};
        });
        // agp_fit_update_batch: the slab of the grown fits, then the scratch of the call (mp2 new points per problem)
        check_layout("carve_update_batch", B * (sA + sI + 2 * np2) + cp2 + 2 * cp2, [&](agp::WsLayout &w) {
          const agp::UpdateBatchRegions r = agp::carve_update_batch(w, g);
          return std::vector<Region>{{r.A, D * B * sA}, {r.invd, D * B * sI}, {r.alpha, D * B * np2}, {r.z, D * B * np2}, {r.logsum, D * cp2},
                                     {r.flags, sizeof(int) * 4 * cp2}};
        });
        const size_t mp2 = 2 * (size_t)((n + 3) / 4), stage = fused ? 5 * B * mp2 + 3 : 0;
        check_layout("carve_update_batch_scratch",
                     B * mp2 + (has_var ? B * mp2 : 0) + stage + (desc_bytes + up8) / 8 + (copy_bytes + up8) / 8 + (gram_bytes + up8) / 8,
                     [&](agp::WsLayout &w) {
                       const agp::UpdateBatchScratch r = agp::carve_update_batch_scratch(w, g, mp2, has_var, stage, desc_bytes, copy_bytes, gram_bytes);
                       return std::vector<Region>{{r.ynew, D * B * mp2}, {r.yvar, D * B * mp2}, {r.xstage, D * stage}, {r.grow_table, desc_bytes},
                                                  {r.cross_table, copy_bytes}, {r.gram_table, gram_bytes}};
                     });
        // the batched gradients: ws_A, ws_aux
        check_layout("carve_gradient_batch", (B * sA + 1) / 2 * 2 + B * sI + B * np2 + (has_var ? B * np2 : 0) + 4 * cp2 + (fused ? B * np2 : 0),
                     [&](agp::WsLayout &w) {
                       const agp::GradientBatchRegions r = agp::carve_gradient_batch(w, g, has_var, fused);
                       return std::vector<Region>{{r.A, D * B * sA}, {r.invd, D * B * sI}, {r.z, D * B * np2}, {r.yvar, D * B * np2},
                                                  {r.logsum, D * cp2}, {r.quad, D * cp2}, {r.flags, sizeof(int) * 4 * cp2}, {r.zpub, D * B * np2}};
                     });
        const size_t tang = has_var ? 2 * B * np2 : 0, part_per = 3 * 10 * 4, ldgd = 6, extra = fused ? 5 : 0;
        check_layout("carve_gradient_batch_aux",
                     (B * sA + 1) / 2 * 2 + tang + B * part_per + B * ldgd + ((gram_bytes + 15) / 16 * 16 + (desc_bytes + 15) / 16 * 16) / 8 + extra * B * np2,
                     [&](agp::WsLayout &w) {
                       const agp::GradientBatchAuxRegions r = agp::carve_gradient_batch_aux(w, g, tang, part_per, ldgd, gram_bytes, desc_bytes, extra);
                       return std::vector<Region>{{r.R, D * B * sA}, {r.tang, D * tang}, {r.partial, D * B * part_per}, {r.grad, D * B * ldgd},
                                                  {r.gram_table, gram_bytes}, {r.desc, desc_bytes}, {r.extra, D * extra * B * np2}};
                     });
        {  // agp_logo_nll_gradient_batch's own region behind its a and u arrays (odd element counts; with and without S)
          const size_t blk = 3 * (size_t)lda + 5, img = 2 * (size_t)IMG, vec = 2 * np2, cnt = 6, terms = 2 * B + 4, meta = 5 * np2 + B + 8;
          const bool slab = fused != 0;
          check_layout("carve_logo_batch", (slab ? (B * sA + 1) / 2 * 2 : 0) + 3 * blk + img + 3 * vec + 2 * cnt + terms + meta + 2 * terms,
                       [&](agp::WsLayout &w) {
                         const agp::LogoBatchRegions r = agp::carve_logo_batch(w, g, slab, blk, img, vec, cnt, terms, meta);
                         const agp::LogoRegions &c = r.chain;
                         require(!c.a && !c.u && !c.symv, "carve_logo_batch: regions of the single entry");
                         return std::vector<Region>{{c.S, D * B * sA}, {c.X0, D * blk}, {c.X1, D * blk}, {c.X2, D * blk}, {c.img, D * img},
                                                    {c.d, D * vec}, {c.z, D * vec}, {c.a_pad, D * vec}, {c.logs_A, D * cnt}, {c.logs_V, D * cnt},
                                                    {c.term, D * terms}, {c.meta, sizeof(long long) * meta}, {r.gflags, sizeof(int) * 4 * terms}};
                       });
        }
        if (count == 1) {  // the single-problem entries: agp_nll's ws_A, the gradients' ws_aux
          check_layout("carve_fit", sA + sI + 2 * np2, [&](agp::WsLayout &w) {
            const agp::FitRegions r = agp::carve_fit(w, g);
            return std::vector<Region>{{r.A, D * sA}, {r.invd, D * sI}, {r.z, D * np2}, {r.yvar, D * np2}};
          });
          const size_t bs = 2 * np2 + 3, part = 10 * 4, grad = 16, xtra = fused ? 5 * np2 + 7 : 0;
          check_layout("carve_gradient_aux", sA + bs + part + grad + tang + xtra, [&](agp::WsLayout &w) {
            const agp::GradientAuxRegions r = agp::carve_gradient_aux(w, g, bs, part, grad, tang, xtra);
            return std::vector<Region>{{r.R, D * sA}, {r.bs_ws, D * bs}, {r.partial, D * part}, {r.grad, D * grad}, {r.tang, D * tang},
                                       {r.extra, D * xtra}};
          });
          // agp_logo_nll_gradient's own region (odd element counts: every region still starts on 16 bytes)
          const size_t blk = 3 * (size_t)lda + 5, img = 2 * (size_t)IMG, vec = 2 * np2, cnt = 6, terms = 4, symv = np2 + 3, meta = 2 * np2 + 7;
          const bool slab = fused != 0;  // (with or without the third slab)
          check_layout("carve_logo", (slab ? sA : 0) + 3 * blk + img + 3 * vec + 2 * cnt + terms + 2 * np2 + symv + meta, [&](agp::WsLayout &w) {
            const agp::LogoRegions r = agp::carve_logo(w, g, slab, blk, img, vec, cnt, terms, symv, meta);
            return std::vector<Region>{{r.S, D * sA}, {r.X0, D * blk}, {r.X1, D * blk}, {r.X2, D * blk}, {r.img, D * img}, {r.d, D * vec},
                                       {r.z, D * vec}, {r.a_pad, D * vec}, {r.logs_A, D * cnt}, {r.logs_V, D * cnt}, {r.term, D * terms},
                                       {r.a, D * np2}, {r.u, D * np2}, {r.symv, D * symv}, {r.meta, sizeof(long long) * meta}};
          });
          // agp_sparse_held_out's one allocation: every combination of the optional outputs (has_var: target variances
          // given; fused: mean and variance asked for; slab: joint asked for)
          const bool want_mean = fused != 0, want_var = fused != 0, want_yvar = has_var != 0 && (want_var || slab);
          const size_t jnt = slab ? 3 * np2 + 1 : 0;
          check_layout("carve_sparse_held_out",
                       4 * blk + img + 3 * vec + 2 * cnt + terms + 2 * np2 + ((want_mean ? 2 : 0) + (want_yvar ? 1 : 0) + (want_var ? 1 : 0)) * np2 +
                           jnt + meta + (slab ? terms : 0),
                       [&](agp::WsLayout &w) {
                         const agp::SparseHeldOutRegions r =
                             agp::carve_sparse_held_out(w, np2, blk, img, vec, cnt, terms, meta, want_mean, want_yvar, want_mean, want_var, jnt);
                         const agp::LogoRegions &c = r.chain;
                         require(!c.S && !c.a && !c.u && !c.symv, "carve_sparse_held_out: regions of the dense entry");
                         require((r.y != nullptr) == (want_mean && w.base) && (r.joint != nullptr) == (slab && w.base), "carve_sparse_held_out: options");
                         return std::vector<Region>{{c.X0, D * blk}, {c.X1, D * blk}, {c.X2, D * blk}, {r.M, D * blk}, {c.img, D * img}, {c.d, D * vec},
                                                    {c.z, D * vec}, {c.a_pad, D * vec}, {c.logs_A, D * cnt}, {c.logs_V, D * cnt}, {c.term, D * terms},
                                                    {r.aw, D * np2}, {r.alpha, D * np2}, {r.y, D * np2}, {r.yvar, D * np2}, {r.mean, D * np2},
                                                    {r.variance, D * np2}, {r.joint, D * jnt}, {c.meta, sizeof(long long) * meta},
                                                    {r.joff, sizeof(long long) * terms}};
                       });
        }
      }
}

// ---- part 6: the pooled plan of agp_logo_nll_gradient_batch (csrc/logo_batch_plan.h) ------------------------------------------
// Ragged groupings over 1-12 problems from a fixed linear congruential stream, under the entry's limits and under small
// ones that split every size class: every table of the plan is walked (each read inside meta), every non-empty group is
// found once with its problem and its indices, the per-problem lists partition the terms, and the carve sized from the
// plan holds every chunk's slabs, vectors and tables.  Malformed groupings are refused.
long long ld_of(long long n) {  // csrc/api.hip: factor_ld
  long long ld = (n + 7) / 8 * 8;
  return ld % 256 == 0 ? ld + 8 : ld;
}
long long img_stride_of(long long m) { return (m + 127) / 128 * (36ll * 16 * 16); }  // gradient.hip: logo_img_stride

void logo_batch_plan_under_sanitizers() {
  std::uint64_t state = 12345;
  auto next = [&](std::uint64_t mod) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (state >> 33) % mod;
  };
  for (long long count = 1; count <= 12; ++count)
    for (int small = 0; small < 2; ++small) {
      std::vector<long long> n((size_t)count);
      std::vector<std::int64_t> n_groups((size_t)count);
      std::vector<std::vector<std::int64_t>> offsets((size_t)count), indices((size_t)count);
      long long n_max = 0, want_terms = 0;
      for (long long b = 0; b < count; ++b) {
        n[(size_t)b] = 1 + (long long)next(300);
        n_max = std::max(n_max, n[(size_t)b]);
        std::vector<std::int64_t> perm((size_t)n[(size_t)b]);
        for (size_t i = 0; i < perm.size(); ++i) perm[i] = (std::int64_t)i;
        for (size_t i = perm.size(); i > 1; --i) std::swap(perm[i - 1], perm[(size_t)next(i)]);
        offsets[(size_t)b].push_back(0);
        long long at = 0;
        if (next(6) != 0)  // (else: a problem without groups)
          while (at < n[(size_t)b] && next(20) != 0) {
            const long long sizes[] = {0, 1, 1, 2, 3, 4, 7, 16, 33, 64, 130};
            const long long m = std::min(n[(size_t)b] - at, sizes[next(11)]);
            for (long long i = 0; i < m; ++i) indices[(size_t)b].push_back(perm[(size_t)(at + i)]);
            at += m;
            offsets[(size_t)b].push_back(at);
            want_terms += m > 0;
          }
        n_groups[(size_t)b] = (std::int64_t)offsets[(size_t)b].size() - 1;
      }
      std::vector<const std::int64_t *> optr, iptr;
      for (long long b = 0; b < count; ++b) {
        optr.push_back(offsets[(size_t)b].data());
        iptr.push_back(indices[(size_t)b].empty() ? nullptr : indices[(size_t)b].data());
      }
      const agp::LogoBatchLimits lim{small ? 5 : 16384, small ? 3 * img_stride_of(1) : (32ll << 20), small ? 40 : count * n_max, ld_of,
                                     img_stride_of};
      agp::LogoBatchPlan p;
      require(agp::logo_batch_plan(count, n.data(), n_groups.data(), optr.data(), iptr.data(), lim, p), "logo_batch_plan");
      require(p.terms == want_terms && p.problems == count, "logo_batch_plan: terms");
      std::vector<int> seen((size_t)p.terms, 0);
      long long at = 0;
      for (const agp::LogoBatchChunk &ch : p.chunks) {
        require(ch.term_off == at && ch.count >= 1, "logo_batch_plan: chunk order");
        require(ch.count <= lim.groups_max && ch.count * img_stride_of(ch.m) <= lim.img_elems_max, "logo_batch_plan: limits");
        require(ch.count == 1 || ch.count * ch.m <= lim.cols_max, "logo_batch_plan: columns");
        require((size_t)ch.count * (size_t)(ld_of(ch.m) * ch.m) <= p.block_elems && (size_t)(ch.count * ch.m) <= p.vec_elems &&
                    (size_t)ch.count <= p.count_elems && (size_t)(ch.count * img_stride_of(ch.m)) <= p.img_elems,
                "logo_batch_plan: carve sizes");
        long long smallest = ch.m;
        for (long long q = 0; q < ch.count; ++q) {
          const long long sz = p.meta.at((size_t)(ch.size_off + q)), b = p.meta.at((size_t)(ch.prob_off + q));
          const long long term = ch.term_off + q;
          require(sz >= 1 && sz <= ch.m && b == p.problem.at((size_t)term) && sz == p.size.at((size_t)term), "logo_batch_plan: tables");
          smallest = std::min(smallest, sz);
          const std::int64_t *src = indices[(size_t)b].data() + offsets[(size_t)b][(size_t)p.group.at((size_t)term)];
          require(offsets[(size_t)b][(size_t)p.group[(size_t)term] + 1] - offsets[(size_t)b][(size_t)p.group[(size_t)term]] == sz, "logo_batch_plan: group");
          for (long long a = 0; a < ch.m; ++a) {
            const long long v = p.meta.at((size_t)(ch.idx_off + q * ch.m + a));
            require(a < sz ? (v == src[a] && v < n[(size_t)b]) : v == -1, "logo_batch_plan: indices");
          }
        }
        require(ch.m <= 2 * smallest, "logo_batch_plan: padding");
        at += ch.count;
      }
      require(at == p.terms, "logo_batch_plan: every term in a chunk");
      for (long long b = 0; b < count; ++b) {
        long long last = -1;
        for (long long i = p.meta.at((size_t)(p.csr_at + b)); i < p.meta.at((size_t)(p.csr_at + b + 1)); ++i) {
          const long long q = p.meta.at((size_t)(p.csr_terms_at + i));
          require(q > last && p.problem.at((size_t)q) == b && !seen.at((size_t)q)++, "logo_batch_plan: term lists");
          last = q;
        }
      }
      for (int v : seen) require(v == 1, "logo_batch_plan: the lists partition the terms");
      require((size_t)(p.csr_terms_at + p.terms) == p.meta.size(), "logo_batch_plan: meta");
      // refused: an index of a problem at or past its own size, and one that occurs twice
      for (long long b = 0; b < count; ++b)
        if (!indices[(size_t)b].empty()) {
          const std::int64_t keep = indices[(size_t)b][0];
          agp::LogoBatchPlan q;
          indices[(size_t)b][0] = n[(size_t)b];
          require(!agp::logo_batch_plan(count, n.data(), n_groups.data(), optr.data(), iptr.data(), lim, q), "logo_batch_plan: index >= n_b");
          if (indices[(size_t)b].size() > 1) {
            agp::LogoBatchPlan t;
            indices[(size_t)b][0] = indices[(size_t)b][1];
            require(!agp::logo_batch_plan(count, n.data(), n_groups.data(), optr.data(), iptr.data(), lim, t), "logo_batch_plan: index twice");
          }
          indices[(size_t)b][0] = keep;
          break;
        }
    }
}

// ---- part 4: the factorisation's schedule --------------------------------------------------------------------------
void factor_plan_under_sanitizers() {
  agp::FactorSwitches on;  // an MI355X with everything set up, a fit's inversion of the wide blocks requested
  on.step_slots = 512; on.have_masked_stream = on.headcnt_ready = on.step_buffers_ready = on.fused_buffers_ready = true;
  on.inv_requested = true; on.bs_BW = 512;
  agp::FactorSwitches off;  // the two-launch schedule of a context that was demoted, nothing requested
  off.panel_fused = false; off.step_below = off.merge_above = 0;
  // the same two through the request of a call (factor_plan.h: apply_request): a deferred fp64 fit that asks for the early
  // inversion behind fills its caller planned, and a mixed fit (fp16 x 2, wide outer blocks) that found nothing planned
  double images[1], inverses[1];
  agp::FactorRequest fp64_fit, mixed_fit;
  fp64_fit.inv_W = inverses; fp64_fit.inv_BW = 512;
  fp64_fit.prep.img = images; fp64_fit.prep.upto = 20480; fp64_fit.prep.headcnt = true;
  mixed_fit.products = agp::BulkProducts::F16x2; mixed_fit.nbo_wide = 1024;
  agp::FactorSwitches inv = on, mixed = on;
  inv.inv_requested = inv.headcnt_ready = inv.fused_buffers_ready = false; inv.bs_BW = 0;
  agp::apply_request(inv, fp64_fit, fp64_fit.products, fp64_fit.prep, images, 20480, 0, true);
  require(inv.inv_requested && inv.bs_BW == 512 && inv.bs_done == 0 && inv.headcnt_ready && inv.fused_buffers_ready && inv.products == agp::BulkProducts::Fp64 &&
              inv.nbo_wide == 0, "request of a deferred fp64 fit");
  require(!fp64_fit.prep.covers(images, 20481) && !fp64_fit.prep.covers(inverses, 512) && !agp::FusedPrep().covers(nullptr, 0),
          "fills planned for other images or fewer columns do not count");
  agp::apply_request(mixed, mixed_fit, mixed_fit.products, mixed_fit.prep, images, 20480, 768, true);
  require(!mixed.inv_requested && !mixed.headcnt_ready && !mixed.fused_buffers_ready && mixed.products == agp::BulkProducts::F16x2 && mixed.nbo_wide == 1024,
          "request of a mixed fit");
  mixed.fused_buffers_ready = true;  // (as if factor_lower had prepared the fills itself)
  for (const agp::FactorSwitches &sw : {on, off, inv, mixed})
    for (long long n = 1; n <= 20480; ++n) {
      agp::FactorPlanner plan(n, sw);
      agp::OuterStep s;
      long long end = 0, steps = 0, panels = 0;
      while (plan.next(s)) {
        require(s.kend == end && s.next_end > end && s.next_end <= n && s.k0 <= s.kend, "outer steps follow each other");
        const agp::PanelPlan pp = agp::plan_panels(n, s.kend, s.next_end, s.step_mode, sw);
        require(!(pp.step_mode && pp.inner_left) && (!pp.fused || sw.panel_fused), "panel plan");
        require(s.inv_count == 0 || (s.mark_after >= s.kend && s.mark_after < n), "mark inside the step");
        plan.inversion_under_panels(s, s.inv_count > 0);
        panels += (s.next_end - end + agp::PLAN_NB - 1) / agp::PLAN_NB;
        end = s.next_end;
        ++steps;
      }
      require(end == n && steps <= 2 + n / agp::PLAN_NB && panels == (n + agp::PLAN_NB - 1) / agp::PLAN_NB, "the steps cover the matrix");
      require(plan.bs_done() * sw.bs_BW < n || plan.bs_done() == 0, "the last wide block is never inverted early");
    }
  for (long long slots : {146ll, 512ll, 1024ll})
    for (long long below = 0; below <= 4608; ++below) {
      const agp::StepLaunchShape sh = agp::step_launch_shape(below, 3, slots, 256);
      const long long critical = agp::STEP_FIXED_CRITICAL + (below + 63) / 64;
      require(below == 0 ? sh.grid == critical : sh.grid == critical + sh.trail_workers + sh.hold_count, "grid of a step launch");
      require(sh.trail_workers >= 1 && (below == 0 || sh.trail_workers <= sh.trail_tiles), "trailing workgroups");
    }
}

// ---- part 7: the tiling of the update launches -----------------------------------------------------------------------
void update_plan_under_sanitizers() {
  for (int ntr = 1; ntr <= 160; ++ntr) {
    // the decode there and back: every tile of the lower and of the full grid, and nothing behind the last one
    for (int tri = 0; tri <= 1; ++tri)
      for (int ntc : {1, (ntr + 1) / 2, ntr}) {
        const long long count = agp::lower_tile_count(ntr, ntc, tri);
        long long id = 0;
        for (int bj = 0; bj < ntc; ++bj)
          for (int bi = tri ? bj : 0; bi < ntr; ++bi, ++id) {
            int gi = -1, gj = -1;
            require(agp::lower_tile_of(id, ntr, ntc, tri, gi, gj) && gi == bi && gj == bj, "decode of a tile number");
            require(!tri || agp::lower_tile_index(bi, bj, ntr) == id, "tile number of a tile");
          }
        int gi, gj;
        require(id == count && !agp::lower_tile_of(count, ntr, ntc, tri, gi, gj) && !agp::lower_tile_of(count + 7, ntr, ntc, tri, gi, gj),
                "no tile from the count on");
      }
    for (long long slots : {512ll, 208ll, 64ll})
      for (int head_cols : {0, 1, 2, 4, 8}) {
        const int h = head_cols < ntr ? head_cols : ntr, sub = ntr - h;
        const long long tiles = agp::lower_tile_count(sub, sub, 1), head_count = agp::lower_tile_count(ntr, h, 1);
        const agp::BulkSplit sp = agp::plan_bulk_update(tiles, slots, h > 0);
        require(sp.full >= 0 && sp.rem >= 0 && sp.full + sp.rem == tiles && (sp.full % slots == 0 || sp.full == tiles), "split of a bulk update");
        require((sp.kernel == agp::SplitKernel::QuadrantsOnly) == (sp.full == 0 && h == 0), "kernel of a bulk update");
        if (sp.full == 0) {
          require(agp::bulk_grid(sp, head_count, 0) == head_count + 4 * tiles, "grid without whole tiles");
          continue;
        }
        // the order table of the whole tiles: every entry read, every tile [0, full) exactly once
        const std::vector<int> table = agp::xcd_tile_order(sub, sp.full);
        std::vector<char> seen((std::size_t)sp.full, 0);
        require(table.size() == (std::size_t)((sp.full + agp::XCDS - 1) / agp::XCDS * agp::XCDS), "length of an order table");
        for (std::size_t i = 0; i < table.size(); ++i) {
          if (table[i] < 0) {
            require(i + agp::XCDS >= table.size(), "fillers only in the last row");
            continue;
          }
          const int bi = table[i] >> 16, bj = table[i] & 0xffff;
          const long long id = agp::lower_tile_index(bi, bj, sub);
          require(bj <= bi && bi < sub && id < sp.full && !seen[(std::size_t)id], "an order table names every whole tile once");
          seen[(std::size_t)id] = 1;
        }
        require(agp::bulk_grid(sp, head_count, (long long)table.size()) == head_count + (long long)table.size() + 4 * sp.rem, "grid with a table");
        require(agp::lower_entries(128ll * sub - 5, sub, tiles) == 0.5 * (double)(128ll * sub - 5) * (double)(128ll * sub - 4), "entries of all tiles");
      }
  }
  // products and staircases: ragged sizes on both sides of every rule, every layout
  for (long long M : {1ll, 64ll, 65ll, 960ll, 1024ll, 1408ll, 2900ll, 8192ll})
    for (long long N : {1ll, 63ll, 128ll, 1088ll, 2944ll, 9344ll})
      for (long long K : {1ll, 255ll, 256ll})
        for (int layout = 0; layout < 8; ++layout)
          for (long long count : {1ll, 7ll}) {
            const bool tri = layout & 4;
            const agp::NtSubPlan p = agp::plan_nt_sub(M, N, K, tri, layout & 1, layout & 2, count, 512);
            require((p.edge == 128 || p.edge == 64 || p.edge == 32) && (!p.transposed || (p.edge == 64 && !tri)), "tile edge of a product");
            require(p.ntr == (M + p.edge - 1) / p.edge && p.ntc <= (N + p.edge - 1) / p.edge && p.grid == agp::lower_tile_count(p.ntr, p.ntc, tri && !p.transposed),
                    "grid of a product");
            int bi, bj;
            require(p.grid > 0 && agp::lower_tile_of(p.grid - 1, p.ntr, p.ntc, tri && !p.transposed, bi, bj) && bi < p.ntr && bj < p.ntc, "last tile of a product");
          }
  for (long long slots : {512ll, 208ll, 64ll})
    for (long long blocks = 1; blocks <= 24; ++blocks)
      for (long long cols : {1ll, 16ll, 80ll, 240ll}) {
        const agp::StairPlan p = agp::plan_stair(blocks * 1536, cols * 128, 1536, 384, slots);
        require((p.edge == 128 || p.edge == 64) && p.st_tpb * p.edge == 1536 && p.st_c0t * p.edge == 384 && p.ntr == blocks * p.st_tpb, "staircase plan");
        // the last row tile of the last block owns its own diagonal tile and nothing right of it (rank 0 of 1, first block 0)
        const long long diag = (blocks - 1) * p.st_tpb - p.st_c0t + (p.st_tpb - 1);
        require(agp::stair_tile_owned(p.ntr - 1, (int)diag, 0, p.st_tpb, 1, 0, p.st_c0t) &&
                    !agp::stair_tile_owned(p.ntr - 1, (int)diag + 1, 0, p.st_tpb, 1, 0, p.st_c0t), "staircase edge");
      }
  require(agp::quadrant_skipped(3, 3, 0, 1) && !agp::quadrant_skipped(3, 3, 1, 0) && !agp::quadrant_skipped(4, 3, 0, 1) && !agp::quadrant_skipped(3, 3, 1, 1),
          "only the upper quadrant of a diagonal tile is skipped");
  require(!agp::mixed_bulk_ordered(agp::ORDERED_FROM_TILES - 1) && agp::mixed_bulk_ordered(agp::ORDERED_FROM_TILES), "order rule of the mixed fit");
}

// ---- part 5: the owners of device memory -----------------------------------------------------------------------------
struct FakeDevice {
  std::set<void *> live;
  std::string log;       // one letter per call: c cached allocation, p plain allocation, f dev_free, r dev_release
  int fail_at = 0;       // the allocation that fails, counted from the next one (0: none)
  int alloc(void **p, std::size_t bytes, char tag) {
    log += tag;
    if (fail_at > 0 && --fail_at == 0) return 2;  // (hipErrorOutOfMemory)
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    return 0;
  }
  int free(void *p, char tag) {
    log += tag;
    require(live.erase(p) == 1, "a block is freed once, and only a live one");
    std::free(p);
    return 0;
  }
  std::string take_log() { std::string l; l.swap(log); return l; }
} fake;
}  // namespace

namespace agp {  // the four functions dev_mem.h declares (the library's are in csrc/api.hip)
int dev_malloc_bytes(void **p, std::size_t bytes) { return fake.alloc(p, bytes, 'c'); }
int dev_malloc_plain_bytes(void **p, std::size_t bytes) { return fake.alloc(p, bytes, 'p'); }
int dev_free(void *p) { return p ? fake.free(p, 'f') : 0; }
int dev_release(void *p) { return p ? fake.free(p, 'r') : 0; }
}  // namespace agp

namespace {
void dev_mem_under_sanitizers() {
  using agp::DevMem; using agp::GrowBuf; using agp::ParkSlot;
  {  // DevMem
    DevMem<double> empty;  // (destroyed empty at the end of the block: no call)
    DevMem<double> a, b;
    require(a.alloc_cached(64) == 0 && b.alloc_plain(32) == 0 && a && b && fake.take_log() == "cp", "both allocators");
    double *pa = a, *pb = b;
    DevMem<double> c(std::move(a));
    require(!a && c.get() == pa && fake.take_log().empty(), "move construction hands the block over");
    c = std::move(b);  // onto an occupied owner: its block goes first
    require(!b && c.get() == pb && fake.take_log() == "f" && !fake.live.count(pa), "move assignment frees the occupant");
    double *raw = c.release();
    require(!c && raw == pb && fake.take_log().empty(), "release gives the block up without a call");
    c.adopt(raw);
    require(c.get() == pb, "adopt");
    c.reset();
    c.reset();
    require(!c && fake.take_log() == "f", "reset twice frees once");
    fake.fail_at = 1;
    require(c.alloc_plain(16) != 0 && !c && fake.take_log() == "p", "a failed allocation leaves the owner empty");
    DevMem<void> v;
    require(v.alloc_cached(8) == 0 && v.get() != nullptr && fake.take_log() == "c", "an untyped block");
  }
  require(fake.take_log() == "f" && fake.live.empty(), "scope exit frees what is still owned");
  {  // ParkSlot
    ParkSlot slot;
    require(slot.take(100) == nullptr && !slot, "take from an empty slot");
    void *p100 = nullptr, *q100 = nullptr, *p200 = nullptr, *p300 = nullptr;
    agp::dev_malloc_plain_bytes(&p100, 100); agp::dev_malloc_plain_bytes(&q100, 100);
    agp::dev_malloc_plain_bytes(&p200, 200); agp::dev_malloc_plain_bytes(&p300, 300);
    (void)fake.take_log();
    require(slot.park(p100, 100) && slot.bytes() == 100, "an empty slot keeps the block");
    require(slot.take(100) == p100 && !slot && fake.take_log().empty(), "the same size comes back, without a call");
    require(slot.park(p100, 100) && slot.take(200) == nullptr && slot.bytes() == 100, "another size: null, the occupant stays");
    require(!slot.park(q100, 100) && fake.live.count(q100) && fake.take_log().empty(), "the same size onto an occupied slot is refused");
    require(slot.park(p200, 200) && fake.take_log() == "r" && !fake.live.count(p100) && slot.bytes() == 200,
            "another size over an occupant: the occupant is released, once");
    require(!slot.park(p300, 300, /*evict=*/false) && slot.bytes() == 200 && fake.take_log().empty(),
            "without eviction an occupant of another size stays and the block is refused");
    require(slot.take(200) == p200 && slot.park(p300, 300, false) && fake.take_log().empty(), "without eviction an empty slot keeps the block");
    agp::dev_free(q100); agp::dev_free(p200);
    (void)fake.take_log();
  }  // (the slot goes with p300 in it)
  require(fake.take_log() == "r" && fake.live.empty(), "a slot releases its occupant when it goes");
  {  // GrowBuf
    GrowBuf<float> buf;
    require(buf.reserve(0) == 0 && !buf && fake.take_log().empty(), "nothing asked, nothing done");
    require(buf.reserve(64) == 0 && buf && buf.bytes() == 64 && fake.take_log() == "p", "first growth: one allocation");
    float *p = buf;
    require(buf.reserve(64) == 0 && buf.reserve(8) == 0 && buf.get() == p && fake.take_log().empty(), "smaller or equal: no call");
    require(buf.reserve(128) == 0 && buf.bytes() == 128 && fake.take_log() == "fp", "growth: one free, then one allocation");
    fake.fail_at = 1;
    require(buf.reserve(256) != 0 && !buf && buf.bytes() == 0 && fake.take_log() == "fp", "a failing allocation: empty, size 0");
    require(buf.reserve(256) == 0 && buf.bytes() == 256 && fake.take_log() == "p", "a later reserve succeeds");
  }
  require(fake.take_log() == "f" && fake.live.empty(), "no block is left");
}
}  // namespace

// ---- part 8: the Gauss quadrature of agp_iterative_nll (csrc/lanczos_quadrature.h) ----------------------------------------------
void lanczos_quadrature_under_sanitizers() {
  std::mt19937 gen(8);
  std::uniform_real_distribution<double> ua(0.02, 2.), ub(0.05, 0.95);
  const long long stride = 16;  // PCG_COLS: the log's rows
  for (int k : {0, 1, 2, 3, 17, 128, 343, 600}) {
    std::vector<double> a((size_t)std::max(k, 1) * stride, NAN), b((size_t)std::max(k, 1) * stride, NAN);
    for (int i = 0; i < k; ++i) { a[(size_t)(i * stride + 5)] = ua(gen); b[(size_t)(i * stride + 5)] = ub(gen); }
    double wide = NAN, plain = NAN;
    require(agp::lanczos_quadrature(3.5, a.data() + 5, b.data() + 5, stride, k, &wide) == AGP_OK, "lanczos_quadrature: status");
    require(agp::lanczos_quadrature_as<double>(3.5, a.data() + 5, b.data() + 5, stride, k, &plain) == AGP_OK, "lanczos_quadrature: double");
    require(std::fabs(wide - plain) <= 1e-11 * (1. + std::fabs(wide)), "lanczos_quadrature: the two precisions agree");
    if (k == 0) require(wide == 0., "lanczos_quadrature: no row");
    if (k == 1) require(std::fabs(wide - 3.5 * std::log(1. / a[5])) <= 1e-14 * (1. + std::fabs(wide)), "lanczos_quadrature: one row");
    if (k == 2) {  // e_1^T log(T) e_1 of a 2 x 2 matrix from its eigenvalues and the first components of its eigenvectors
      const double t00 = 1. / a[5], t11 = 1. / a[stride + 5] + b[stride + 5] / a[5], t01 = std::sqrt(b[stride + 5]) / a[5];
      const double mid = 0.5 * (t00 + t11), rad = std::sqrt(0.25 * (t00 - t11) * (t00 - t11) + t01 * t01);
      const double l0 = mid - rad, l1 = mid + rad, w1 = (t00 - l0) / (l1 - l0);
      require(std::fabs(wide - 3.5 * ((1. - w1) * std::log(l0) + w1 * std::log(l1))) <= 1e-12 * (1. + std::fabs(wide)), "lanczos_quadrature: two rows");
    }
  }
  double out = -7.;
  const double a_neg[2] = {1., -1. / 3.}, b_neg[2] = {0., 4.}, a_nan[2] = {1., NAN}, b_bad[2] = {0., -1.}, a_one[2] = {1., 1.};
  require(agp::lanczos_quadrature(1., a_neg, b_neg, 1, 2, &out) == AGP_ERR_NOT_POSITIVE_DEFINITE, "lanczos_quadrature: a < 0");
  require(agp::lanczos_quadrature(1., a_nan, b_neg, 1, 2, &out) == AGP_ERR_NOT_POSITIVE_DEFINITE, "lanczos_quadrature: NaN");
  require(agp::lanczos_quadrature(1., a_one, b_bad, 1, 2, &out) == AGP_ERR_NOT_POSITIVE_DEFINITE, "lanczos_quadrature: b < 0");
  require(agp::lanczos_quadrature(0., a_one, b_neg, 1, 2, &out) == AGP_ERR_NOT_POSITIVE_DEFINITE, "lanczos_quadrature: rz0");
  require(agp::lanczos_quadrature(1., nullptr, nullptr, 1, 2, &out) == AGP_ERR_INVALID_ARGUMENT, "lanczos_quadrature: null");
  require(out == -7., "lanczos_quadrature: a refusal writes nothing");
}

int main() {
  schedule_under_sanitizers(false);
  schedule_under_sanitizers(true);
  host_layer_under_sanitizers();
  layouts_under_sanitizers();
  factor_plan_under_sanitizers();
  dev_mem_under_sanitizers();
  logo_batch_plan_under_sanitizers();
  update_plan_under_sanitizers();
  lanczos_quadrature_under_sanitizers();
  std::printf("host_sanitize_check ok\n");
  return 0;
}
