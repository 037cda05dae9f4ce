// common.h — internal types shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/albatross_amd.h"
#include "cov_eval.h"
#include "dev_mem.h"      // DevMem, ParkSlot, GrowBuf: the owners of device memory
#include "factor_plan.h"  // FactorRequest, FactorOutcome, FusedPrep: the arguments of factor_lower
#include "update_plan.h"  // BulkKernel and the tile decode of the update launches

// Wave priority of the panel-chain kernels (s_setprio); the bulk update stays at 0 (the four combinations were measured:
// DESIGN.md section 8, profiles/r03/sweep_prio.txt)
#define AGP_CHAIN_PRIO 3

namespace agp {

// Blocking factors of the LL^T factorisation:
//   NB    diagonal-block / panel width handled by one potrf + one trsm launch
//   NBO   outer block: trailing updates accumulate NBO columns of panel (K=NBO)
//   MB    micro-block inside a diagonal block (one f64 MFMA tile)
constexpr int NB = 128;
constexpr int NBO = 512;
constexpr int MB = 16;
constexpr int NMB = NB / MB;  // 8 micro blocks per diagonal block

// f(std::integral_constant<int, DIMP>{}) with the padded dimension DIMP (1, 2, 3, 4 or 8) of a dim-dimensional feature
// set: the launch of a kernel template on Point<DIMP>
template <class F>
inline void dispatch_dim(int dim, F &&f) {
  if (dim == 1) f(std::integral_constant<int, 1>{});
  else if (dim == 2) f(std::integral_constant<int, 2>{});
  else if (dim == 3) f(std::integral_constant<int, 3>{});
  else if (dim == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// Which split-plane kernels of the mixed-precision factorisation run and how (gemm_split_planes.hip): part of a
// context's tuning, handed to their launchers by value
struct F16x2Tuning {
  int lds_pad = 8192;  // AGP_F16X2_LDS_PAD: extra dynamic LDS per workgroup (bytes)
  int terms = 4;       // AGP_F16X2_TERMS: 3, or 4: with the h2 h2 product
  int chunk = 32;      // AGP_F16X2_CHUNK: k per LDS stage and per plane chunk, 32 or 64 (fixes the layout of the planes)
};
struct Bf16x3Tuning {
  int lds_pad = 8192;  // AGP_BF16X3_LDS_PAD: extra dynamic LDS per workgroup (bytes)
};

struct DeviceFeatures {
  FeatView v{};
  DevMem<void> owned[3];  // error paths return early: the owned device copies go with the object
  void release() {
    for (auto &p : owned) p.reset();
    v = FeatView{};
  }
};

}  // namespace agp

struct agp_kernel {
  agp::DevProgram prog;
};

struct agp_context {
  int device = 0;
  hipStream_t stream = nullptr;   // main chain
  hipStream_t stream2 = nullptr;  // look-ahead / side chain
  hipStream_t stream3 = nullptr;  // host-side control-plane collectives of the RCCL transport (shard_hip.hip)
  // bulk stream restricted to a CU mask (hipExtStreamCreateWithCUMask): in the chain-bound end phase of the
  // factorisation the bulk updates run here and leave a few CUs per XCD to the panel chain (chol.hip: factor_lower)
  hipStream_t stream_masked = nullptr;
  hipEvent_t ev_c = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  std::vector<hipEvent_t> ev_pool;
  std::string last_error;
  agp::DevMem<int> d_flags;  // [0] nan flag, [1] first bad pivot + 1
  int *h_flags = nullptr;  // pinned mirror
  double *d_scalars = nullptr;  // [0] sum log L_ii, [1] z^T z
  double *h_scalars = nullptr;  // pinned mirror
  void *h_status_dev = nullptr;  // h_flags (the whole status block) as the device addresses it, or nullptr
  bool profiling = false;
  double stage_ms[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // [10]: the step chain of agp_pivoted_cholesky; [11], [12]: agp_iterative_fit_create; [12], [13]: agp_iterative_nll_gradient; [12] .. [14]: agp_iterative_nll
  // reusable factor workspace (agp_nll re-uses it between tuner steps)
  agp::GrowBuf<double> ws_A;
  agp::GrowBuf<double> ws_aux;
  agp::GrowBuf<double> ws_refine;  // scratch of the mixed fit's refinement (api.hip: refine_information), kept between fits
  // one cached factor allocation (agp_fit_destroy parks its N x N buffer here;
  // the next agp_fit_create of the same size takes it instead of hipMalloc)
  agp::ParkSlot pool_A;
  // ... and one cached exact-covariance buffer of the mixed-precision fit (its CG refinement multiplies with K itself)
  agp::ParkSlot pool_K;
  // mixed-precision fits: two alternating low-precision copies of the current panel, in whichever format the fit's
  // products take (fp32, or split 16-bit planes); reserved and handed out by PanelStager (chol.hip) alone
  agp::GrowBuf<unsigned char> panel_copies;
  agp::GrowBuf<double> f16_scales;  // fp16 x 2 products (gemm_split_planes.hip): row scales r and 1 / r, f16_scales_n doubles each
  long long f16_scales_n = 0;
  // ... and the fp32 copy of the factor that preconditions their refinement
  agp::ParkSlot pool_L32;
  // ... and one cached block of a fit's small buffers (agp_fit::aux_base)
  agp::ParkSlot pool_aux;
  // scratch of the sharded fit (agp_sharded_fit_destroy parks it here, like pool_A)
  agp::ParkSlot pool_shard;
  // the n-sized buffers of a sparse GP fit (K_uf / W, P / Q1^T, split-K slabs): grow-only, kept between fits - a tuner
  // re-fits the same shapes, and hipMalloc / hipFree of several GB per call costs more than some of the stages
  agp::GrowBuf<double> pool_sparse;
  // ... and one cached slab of agp_fit_create_batch (released by the last fit of a batch)
  agp::ParkSlot pool_batch;
  // fused panel kernel (chol.hip: panel_fused_kernel): the slots through which a diagonal block's z_b reaches the
  // workgroups solving the rows below in the same launch (one per matrix row, sentinel-filled per factorisation: what has
  // been filled for which tile images is the FusedPrep that panel_fused_plan returns, not kept here)
  agp::GrowBuf<double> d_zpub;
  long long zpub_cap = 0;
  // ... and the slots through which an UPDATED diagonal block reaches the workgroup that factors it (one tile image
  // per diagonal block, like invd; only allocated when the update-ahead panel kernel is in use)
  agp::GrowBuf<double> d_dpub;
  long long dpub_cap = 0;  // diagonal blocks
  int cus = 256;  // CUs of the device (hipDeviceAttributeMultiprocessorCount)
  long long step_slots = 0;  // workgroups of the panel step kernel the device holds at once (chol.hip: step_slots)
  // The switches a caller can set through the environment, read ONCE at agp_context_create (api.hip: read_tuning; the
  // table is in include/albatross_amd.h).  Everything else about the schedule is a constant of the library.
  struct Tuning {
    bool panel_fused = true;       // AGP_PANEL_FUSED=0: POTRF and panel TRSM as two launches
    long long step_below = 4608;   // AGP_STEP_BELOW: remaining rows at or below which every panel is ONE step launch (0: off)
    bool gram_sop = true;          // AGP_GRAM_SOP=0: covariance trees through the stack interpreter only
    long long fp64_nbo = 0;        // AGP_FP64_NBO: outer block width of the fp64 factorisation while > 8192 rows remain (0: 512)
    long long mixed_nbo = 512;     // AGP_MIXED_NBO: outer block width of the bf16 x 3 factorisation while > 8192 rows remain
    bool mixed_f16 = true;         // AGP_MIXED_F16=0: the mixed-precision fit's products from three bf16 planes (round 5) instead of two fp16 planes
    bool mixed_bf16 = true;        // AGP_MIXED_BF16=0: the mixed-precision fit's products on the fp32 MFMA (rounds 1-4) instead of bf16 x 3
    long long backsub_coop_max = 2047;  // AGP_BACKSUB_COOP_MAX: largest n whose fit uses it (measurement switch)
    bool backsub_coop = true;      // AGP_BACKSUB_COOP=0: the fit's back substitution as a launch per block (rounds 1-4) instead of ONE launch
    bool sparse_pivoted = false;   // AGP_SPARSE_PIVOTED=1: the sparse GP's literal (pivoted LDL^T + QR) path always
    long long predict_chunk = 0;   // AGP_PREDICT_CHUNK: test points per slice of the marginal / joint predictions (0: by memory)
    long long shard_block = 0;     // AGP_SHARD_BLOCK: 128 / 256 / 512 rows per row block of the sharded fit (0: 512)
    bool shard_force_comm = false; // AGP_SHARD_FORCE_COMM=1: ONE rank runs the multi-rank schedule through its transport
    bool shard_host_pacing = false;  // AGP_SHARD_HOST_PACING=1: the sharded schedule is paced by the host (round-3 scheme)
    double shard_mask_gflop = 40.;   // AGP_SHARD_MASK_GFLOP: bulk update per step below which a sharded fit is chain-bound
    long long merge_above = 8704;  // AGP_MERGE_ABOVE: trailing rows above which the next-block-column update rides in the bulk launch (0: never)
    agp::F16x2Tuning f16x2;        // AGP_F16X2_*: the fp16 x 2 kernels of the mixed-precision fit
    agp::Bf16x3Tuning bf16x3;      // AGP_BF16X3_*: the bf16 x 3 kernels
  } tune;
  unsigned long long *d_rowcnt = nullptr;  // one counter per 64 rows (tail of the d_dpub allocation): hand-over of the step launches' row updates
  // merged bulk updates (chol.hip: factor_lower): one counter per outer step - the tiles of the next block column count
  // themselves, the chain stream's gate kernel waits for all of them; zeroed by panel_fused_plan (FusedPrep::headcnt)
  // pinned host memory for the small tables a batched entry point uploads (descriptors of its problems): a copy from
  // pinned memory is really asynchronous, so the call needs no synchronisation between building a table and the launch
  // that reads it (api.hip: host_stage; valid until the call's final synchronisation)
  void *h_stage = nullptr;
  size_t h_stage_bytes = 0;
  static constexpr long long HEADCNT_WORDS = 256;
  agp::DevMem<unsigned long long> d_headcnt;
  // What the last factorisation / fit of this context ran: host-side only, filled by factor_lower from each planned step
  // it has carried out (factor_plan.h: OuterStep), at the panel launches of panel_phase (chol.hip) and by fit_create_impl
  // (api.hip), read by the tests through agp_debug_schedule (debug_api.hip,
  // which documents the layout).  Nothing in the library reads it back.
  struct ScheduleRecord {
    // outer steps: bits of each step
    static constexpr unsigned MERGED = 1, STEP = 2, THROTTLED = 4, MASKED = 8, SINGLE = 16;
    // back substitution of the last fit
    enum Backsub { BS_NONE = 0, BS_COOP_DIRECT = 1, BS_COOP_FLAGS = 2, BS_WIDE = 3, BS_CHAIN = 4 };
    // inversions of the wide diagonal blocks under the factorisation (bits)
    static constexpr unsigned INV_EARLY = 1, INV_LAST_STEP = 2, INV_TAIL = 4;
    long long n = 0;
    long long steps = 0, steps_dropped = 0;  // outer steps recorded / not recorded (beyond HEADCNT_WORDS)
    long long kend[HEADCNT_WORDS] = {};      // last column + 1 of each outer step
    unsigned bits[HEADCNT_WORDS] = {};
    long long panels_step = 0, panels_fused = 0, panels_split = 0;  // panel_fused_kernel<true> / <false> / POTRF + TRSM
    int backsub = BS_NONE;
    long long bs_done = 0;  // wide inverses computed under the factorisation
    unsigned inv_bits = 0;
    int handover_timeout = 0;  // flags[2] after the factorisation (fit: after the whole fit)
    long long demotions = 0;   // fit_create_retrying fell back to the two-launch schedule (over the life of the context)
    void reset_factor(long long n_) {
      n = n_;
      steps = steps_dropped = 0;
      panels_step = panels_fused = panels_split = 0;
      inv_bits = 0;
      handover_timeout = 0;
    }
    void add_step(long long end, unsigned b) {
      if (steps < HEADCNT_WORDS) { kend[steps] = end; bits[steps] = b; ++steps; }
      else ++steps_dropped;
    }
  } sched;
  // recorded behind the early inversion of the wide diagonal blocks a fit asks factor_lower for (FactorRequest::inv_W)
  hipEvent_t ev_inv = nullptr;
  // sharded fit, device-side pacing (shard_hip.hip: HipShardOps): one flag per schedule event + probe flags in device
  // memory, their sequence numbers (monotonic over the life of the context), and the pacing mode (-1: not decided yet)
  hipStream_t stream_comm = nullptr;  // queue of the collectives (created by the first sharded call)
  agp::DevMem<unsigned long long> shard_flags;
  unsigned long long shard_seq[16] = {};
  unsigned long long shard_probe_seq = 0;
  int shard_host_pacing = -1;
  bool shard_probe_ok = false;
};

// agp_fit_create_batch: the fits of one batch are slices of ONE device allocation (the batched kernels need constant
// strides between the problems); it goes when the last of them is destroyed
struct agp_fit_slab {
  agp::DevMem<double> base;
  size_t bytes = 0;
  int refs = 0;
};

struct agp_fit {
  agp_context *ctx = nullptr;  // owner; a fit must not outlive its context
  agp_fit_slab *slab = nullptr;  // non-null: A / invd / alpha / z are slices of slab->base (winv: not kept)
  size_t A_bytes = 0;
  int device = 0;
  int64_t n = 0;
  int64_t lda = 0;
  double *A = nullptr;      // n x n lower factor, column-major, ld = lda
  double *invd = nullptr;   // tile image of every NB x NB diagonal block (72 KiB each):
                            // negated off-diagonal micro tiles + inverted diagonal micro tiles
  double *winv = nullptr;   // (n/NB) inverted NB x NB diagonal blocks
  double *alpha = nullptr;  // information vector K^-1 y
  double *z = nullptr;      // L^-1 y
  // A, invd, winv, alpha and z above are what the kernels read.  What the fit OWNS of them, every maker says here, and
  // agp_fit_destroy never asks which regime it is in: it offers own_A and aux_base to the context's slots and deletes.
  //   own_A: the factor's block (empty for a fit of a batch, whose blocks are slices of slab->base)
  //   aux_base: agp_fit_create makes invd / winv / alpha / z (and the training features) slices of ONE allocation, which
  //             parks in the context like the factor's buffer: four hipMalloc + four hipFree per fit less
  //   own_part: invd / winv / alpha / z where they are allocations of their own (every other maker of a single fit)
  agp::DevMem<double> own_A;
  agp::DevMem<double> aux_base;
  size_t aux_bytes = 0;
  agp::DevMem<double> own_part[4];
  agp::DeviceFeatures train;
  double log_det = 0.;
  int64_t failed_pivot = -1;
  // What the creating call reported for this fit: AGP_OK, AGP_ERR_NAN_INPUT or AGP_ERR_NOT_POSITIVE_DEFINITE (failed_pivot
  // alone cannot tell a NaN input from a good fit).  agp_predict_batch hands it on in status[b].
  int fail_status = 0;
  bool mixed = false;  // made by agp_fit_create_mixed: the factor carries the rounding of the low-precision bulk products
  // Fits grown by agp_fit_update: the appended block starts at a multiple of 128, so when the size before the update
  // was not one, the rows in between are PHANTOM rows (identity rows of the factor, zero information, decoupled from
  // everything).  `n` counts them - every kernel works on the padded factor -, `n_real` does not (0: no phantoms) and
  // the C-ABI only ever shows real rows.  phantom: sorted half-open ranges [first, last) of padded row indices.
  int64_t n_real = 0;
  std::vector<std::pair<long long, long long>> phantom;
};

#define AGP_HIP_CHECK(ctx, expr)                                              \
  do {                                                                        \
    const hipError_t _e = static_cast<hipError_t>(expr);                      \
    if (_e != hipSuccess) {                                                   \
      if (ctx) {                                                              \
        (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e); \
      }                                                                       \
      return AGP_ERR_HIP;                                                     \
    }                                                                         \
  } while (0)

namespace agp {

// ---- launchers implemented in the .hip files ----
bool launch_gram_blocks(hipStream_t s, const DevProgram *host_program, const FeatView &X, long long rows, long long count,
                        double *out, long long ld, long long stride, const double *diag_add, int *nan_flag);
void launch_gram(hipStream_t s, const DevProgram *P, const FeatView &X, const FeatView &Y,
                 bool symmetric, bool lower_only, double *out, long long ld,
                 const double *diag_add, int *nan_flag, const DevProgram *host_program = nullptr);
// `count` symmetric lower-only Gram matrices in ONE launch when every problem takes the same fast path (gram.hip); false:
// not applicable, nothing launched.  table_dev: gram_batch_table_bytes(count) bytes of device scratch.
size_t gram_batch_table_bytes(long long count);
// host_stage (optional): gram_batch_table_bytes(count) bytes of PINNED host memory that stay untouched until the launch has
// run - the table is built there and uploaded without a synchronisation; nullptr: pageable staging + one stream synchronisation
bool launch_gram_batch(hipStream_t s, long long count, const DevProgram *const *host_programs, const FeatView *Xs, double *const *outs,
                       long long ld, const double *const *diag_adds, int *const *nan_flags, void *table_dev, void *host_stage = nullptr);
void launch_gram_diagonal(hipStream_t s, const DevProgram *P, const FeatView &X, double *out);
// Which kernel launch_gram / launch_predict_mean runs for a program and two feature views (gram.hip).  The launchers switch
// on the value these functions return and decide nothing themselves, so the path a caller is told is the path that ran.
// plan (optional): the parameters of the chosen kernel, for the launcher.
enum class GramPath : int { FAST_TRI = 0, FAST_RECT = 1, PAIR2 = 2, SOP = 3, INTERP = 4 };
enum class PredictMeanPath : int { TILED8 = 0, TILED4 = 1, FAST_WAVE = 2, SOP = 3, INTERP = 4 };
struct GramPlan;
struct PredictMeanPlan;
GramPath gram_select_path(const DevProgram *host_program, const FeatView &X, const FeatView &Y, bool lower_only,
                          GramPlan *plan = nullptr);
PredictMeanPath predict_mean_select_path(const DevProgram *host_program, const FeatView &X, const FeatView &XS,
                                         PredictMeanPlan *plan = nullptr);
// mean_j = sum_i k(x_i, xs_j) alpha_i without materialising the cross Gram
void launch_predict_mean(hipStream_t s, const DevProgram *P, const FeatView &X, const FeatView &XS,
                         const double *alpha, double *mean, const DevProgram *host_program = nullptr);

// LL^T of the n x n lower triangle of A (ld = lda), in place.  y (n) is
// overwritten with z = L^-1 y when non-null.  invd receives the inverted
// diagonal micro blocks.  flags[1] = first non-positive pivot + 1.
// scalars[0] += sum log L_ii.
struct FactorTimers {
  hipEvent_t *ev = nullptr;  // optional pool: one (start, stop) pair per trailing-update launch
  double *flops = nullptr;   // per pair: flop of that launch
  int n_ev = 0;
  int used = 0;
};
// req: everything that is particular to this call (factor_plan.h: FactorRequest; the default is the plain fp64 factorisation)
FactorOutcome factor_lower(agp_context *ctx, double *A, long long n, long long lda, double *invd, double *y,
                           const FactorRequest &req = {});
struct PrepArgs;  // pub.h
// the fills planned (FactorRequest::prep for the factor_lower they are meant for); empty: not planned
FusedPrep panel_fused_plan(agp_context *ctx, double *invd, long long k_begin, long long k_end, bool want_step, PrepArgs *prep);

// Winv[b] = inv(L_bb) for every NB x NB diagonal block (batched, one launch)
void invert_diag_blocks(hipStream_t s, const double *A, long long n, long long lda, const double *invd,
                        double *Winv);
// x = L^-T z (one right-hand side), z overwritten.
void invert_diag_blocks_forward(hipStream_t s, long long n, const double *invd, double *Wfwd);
void forward_solve_vec(hipStream_t s, const double *A, long long n, long long lda, const double *Wfwd, double *z,
                       double *xstage);
void backward_solve_vec(hipStream_t s, const double *A, long long n, long long lda, const double *Winv,
                        double *z, double *xstage);
// B (n x m, ldb) <- L^-1 B
void forward_solve_mat(hipStream_t s, const double *A, long long n, long long lda, const double *invd,
                       double *B, long long m, long long ldb, bool rhs_lower = false);
// B (n x m, ldb) <- L^-T B
void factor_lower_batched(hipStream_t s, double *A, long long stride_A, long long n, long long lda, double *invd,
                          long long stride_invd, double *y, long long stride_y, long long count, int *flags,
                          double *logsum, long long stride_flags = 0, double *zpub = nullptr, long long stride_zpub = 0);
// may a batch of `count` n x n problems use the fused panel launches of factor_lower_batched (zpub != nullptr)?
bool batched_fused_fits(agp_context *ctx, long long n, long long count);
void factor_lower_batched_lookahead(agp_context *ctx, double *A, long long stride_A, long long n, long long lda, double *invd,
                                    long long stride_invd, double *y, long long stride_y, long long count, int *flags,
                                    double *logsum, long long stride_flags = 0);
// z_b <- L_b^-T z_b for `count` problems, one vector each (solve.hip)
void backward_solve_vec_batched(hipStream_t s, const double *A, long long stride_A, long long n, long long lda,
                                const double *invd, long long stride_invd, double *z, long long stride_z, long long count);
// x = L^-T z in ONE launch (solve.hip: backsub_coop_kernel); done: backsub_done_words(n, count) ZEROED words (PrepArgs::fill),
// or nullptr with x SENTINEL-filled (PrepArgs::sentinel) for at most BACKSUB_DIRECT_BLOCKS 128-row blocks
constexpr long long BACKSUB_DIRECT_BLOCKS = 16;
long long backsub_done_words(long long n, long long count);
void backward_solve_coop(hipStream_t s, const double *A, long long n, long long lda, const double *invd, const double *z,
                         double *x, int *flags, unsigned long long *done, long long count = 1, long long stride_A = 0,
                         long long stride_invd = 0, long long stride_z = 0, long long stride_x = 0, long long stride_flags = 0,
                         const void *status_src = nullptr, void *status_dst = nullptr, int status_words = 0);
void launch_fill_sentinel(hipStream_t s, double *p, long long count);
void forward_solve_mat_batched(hipStream_t s, const double *A, long long stride_A, long long n, long long lda,
                               const double *invd, long long stride_invd, double *B, long long stride_B, long long m,
                               long long ldb, bool rhs_lower, long long count);
void right_solve_lt_batched(hipStream_t s, const double *A, long long stride_A, long long n, long long lda,
                            const double *invd, long long stride_invd, double *X, long long stride_X, long long nrows,
                            long long ldx, long long count);
void launch_gemm_nt_sub_batched(hipStream_t s, double *C, long long ldc, long long batch_C, const double *A,
                                long long lda, bool a_kmajor, long long batch_A, const double *B, long long ldb,
                                bool b_kmajor, long long batch_B, long long M, long long N, long long K, bool tri,
                                long long count);
void right_solve_lt(hipStream_t s, const double *A, long long n, long long lda, const double *invd, double *X,
                    long long nrows, long long ldx);
void forward_solve_mat_lookahead(agp_context *ctx, const double *A, long long n, long long lda, const double *invd,
                                 double *B, long long m, long long ldb, bool rhs_lower = false);
void backward_solve_mat(hipStream_t s, const double *A, long long n, long long lda, const double *invd,
                        double *B, long long m, long long ldb);
// X = L^-1 B OUT OF PLACE for a right-hand side much wider than L (the sparse GP's m x n matrices): see solve.hip
constexpr long long WIDE_BW = 512;
bool forward_solve_wide_ok(long long n, long long ncols);
void invert_wide_blocks(hipStream_t s, const double *A, long long n, long long lda, const double *invd, long long BW, double *W);
void forward_solve_wide(hipStream_t s, const double *A, long long n, long long lda, const double *Winv, const double *B,
                        long long ldb, double *X, long long ldx, long long ncols);

// out[j] = sum_i A[i,j] * B[i,j]   (column-wise dot of two n x m matrices)
void launch_coldot(hipStream_t s, const double *A, long long lda, const double *B, long long ldb,
                   long long n, long long m, double *out, double scale, const double *base);
// C (m x m, ldc) = base - V^T W  with V, W n x m
void launch_gemm_tn_sub(hipStream_t s, const double *V, long long ldv, const double *W, long long ldw,
                        long long n, long long m, double *C, long long ldc);
// y = A^T x for A n x m
void launch_gemv_t(hipStream_t s, const double *A, long long lda, long long n, long long m,
                   const double *x, double *y);
void launch_dot(hipStream_t s, const double *a, const double *b, long long n, double *out);
// launch_tall_matvec / launch_tall_matvec_f32 (reduce.hip; declared in api_internal.h) stage x in LDS and launch NOTHING for more columns than this: every
// caller checks its width against it where the width is chosen - api.hip: backsolve_width (static_assert) and
// mixed_precondition_setup; solver_api.hip: agp_solver_update_information (launch_matvec beyond it)
constexpr long long TALL_MATVEC_MAX_COLS = 2048;

}  // namespace agp

namespace agp {
// C(M x N) -= A(M x K) * B(N x K)^T  (fp64 MFMA).  a_kmajor / b_kmajor select
// transposed operand storage; tri keeps only tiles on/below C's diagonal.
void launch_gemm_nt_sub(hipStream_t s, double *C, long long ldc, const double *A, long long lda,
                        bool a_kmajor, const double *B, long long ldb, bool b_kmajor, long long M,
                        long long N, long long K, bool tri);
void launch_gemm_nt_ext(hipStream_t s, double *C, long long ldc, const double *Cin, long long ldcin, const double *A, long long lda,
                        const double *B, long long ldb, long long M, long long N, long long K);
void launch_gemm_nt_sub_stair(hipStream_t s, double *C, long long ldc, const double *A, long long lda, const double *B,
                              long long ldb, long long M, long long N, long long K, int world, int rank, long long lb0,
                              long long block, long long c0);
// bulk trailing update of the factorisation: C(M x M, lower tiles) -= P Q^T
// `timing` (optional): an event pair recorded around the trailing_update_kernel launch of this update
// (not around the 64-tile tail launch) and the algorithmic flop of exactly the tiles that launch covers;
// flops == 0 on return means no such launch was made and the events were not recorded.
struct BulkTiming {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double flops = 0.;
};
void launch_trailing_update_as(BulkKernel kernel, hipStream_t s, double *C, long long ldc, const double *P,
                               const double *Q, long long ldp, long long M, long long K,
                               BulkTiming *timing = nullptr, const float *P32 = nullptr, const float *Q32 = nullptr,
                               long long ld32 = 0);
void launch_trailing_update(hipStream_t s, double *C, long long ldc, const double *P, const double *Q,
                            long long ldp, long long M, long long K, BulkTiming *timing = nullptr);
void read_bulk_probe(unsigned long long *out);   // gemm.hip: cycles and 100 MHz ticks of one tile of a -DAGP_BULK_STAMPS build (zeros otherwise)
void read_bf16_probe(unsigned long long *out);   // gemm_split_planes.hip: 8 words of a -DAGP_BF16_STAMPS build (zeros otherwise)
void read_potrf_probe(unsigned long long *out);  // chol.hip: 4 x 32 cycle stamps of a -DAGP_POTRF_TIMING build (zeros otherwise)
void launch_head_gate(hipStream_t s, const unsigned long long *done, unsigned long long expect, int *flags);  // chol.hip
// the whole trailing matrix of an outer step in ONE launch, the next block column's tiles first and counted (gemm.hip)
void launch_trailing_update_merged(hipStream_t s, double *C, long long ldc, const double *P, long long ldp, long long M, long long K,
                                   int head_cols, unsigned long long *head_done, long long *head_tiles, BulkTiming *timing = nullptr);
void launch_update_f32(hipStream_t s, double *C, long long ldc, const double *P, const double *Q, long long ldp, long long M,
                       long long N, long long K, const float *P32 = nullptr, const float *Q32 = nullptr, long long ld32 = 0);
// The split-plane paths of the mixed-precision factorisation (gemm_split_planes.hip).  bf16 x 3: the panel of one outer
// step as three bf16 planes (hi + mid + lo = the value to fp32 accuracy), and C -= P[row_a ..] P[row_b ..]^T from them on
// the BF16 pipe
size_t split_planes_bytes(int planes, long long rows, long long K);  // `planes` planes of a rows x K panel, padding included
void launch_convert_panel_bf16x3(hipStream_t s, const double *P, long long ldp, long long rows, long long K, unsigned short *planes);
void launch_update_bf16x3(hipStream_t s, Bf16x3Tuning tune, double *C, long long ldc, const unsigned short *planes, long long panel_rows, long long row_a,
                          long long row_b, long long M, long long N, long long K, const int *order = nullptr, long long order_len = 0);
// fp16 x 2: power-of-two row scales from the diagonal (rs, irs = 1 / rs: n doubles each), the
// panel of one outer step as two fp16 planes of the scaled rows, and C -= P[row_a ..] P[row_b ..]^T from them (three
// v_mfma_f32_16x16x32_f16 per block; irs belongs to the panel's row 0)
void launch_f16x2_row_scales(hipStream_t s, const double *A, long long lda, long long n, double *rs, double *irs);
void launch_convert_panel_f16x2(hipStream_t s, F16x2Tuning tune, const double *P, long long ldp, long long rows, long long K,
                                const double *rs, unsigned short *planes);
bool f16x2_depth_ok(F16x2Tuning tune, long long K);  // K a whole number of the kernel's K chunks
void launch_update_f16x2(hipStream_t s, F16x2Tuning tune, double *C, long long ldc, const unsigned short *planes, long long panel_rows, long long row_a,
                         long long row_b, const double *irs, long long M, long long N, long long K, const int *order = nullptr,
                         long long order_len = 0);
// the XCD-aware order of the `tiles` first lower 128 x 128 tiles of a grid with ntr tile rows (gemm.hip; cached): nullptr = none
const int *bulk_tile_order(int ntr, long long tiles, long long *len);
// P32 (rows x K, ld32) = (float) P: the fp32 copy of one outer step's panel for the fp32-product kernels
void launch_convert_panel_f32(hipStream_t s, const double *P, long long ldp, long long rows, long long K, float *P32, long long ld32);

// Mixed precision (chol.hip): ONE low-precision copy of a step's panel for all the tiles of U1 and of the bulk update, in
// the format of the fit's BulkProducts (factor_plan.h) - fp32, three bf16 planes or two fp16 planes of scaled rows.
// PanelStager owns the format: the buffers, the fall-backs, the layout; StagedPanel is one step's copy and launches the
// kernel that reads it.  Without a copy (nothing reserved, or the panel does not fit) the fp32-product kernels round the
// fp64 operands themselves while they stage them - twice their operand traffic, which is what they wait for.
class StagedPanel {
 public:
  bool staged() const { return P32_ || P16_; }
  // C (M x N, lower tiles; C(0, 0) at panel row row_offset, on the matrix diagonal) -= P[row_offset ..] P[row_offset ..]^T
  // with low-precision products.  M == N is the bulk shape: the tiles in the XCD-aware order once there are 1024 of them,
  // and `timers` as for every bulk launch (chol.hip: timed_gemm); the split-plane kernels are not timed.
  void apply(hipStream_t s, double *C, long long ldc, long long row_offset, long long M, long long N, long long K,
             FactorTimers *timers = nullptr) const;

 private:
  friend class PanelStager;
  BulkProducts products_ = BulkProducts::Fp32;  // of the copy; without a copy: Fp32, rounded by the kernel itself
  const double *P_ = nullptr;                   // the fp64 panel
  long long ldp_ = 0, rows_ = 0;
  const float *P32_ = nullptr;
  long long ld32_ = 0;
  const unsigned short *P16_ = nullptr;
  const double *irs_ = nullptr;                 // F16x2: 1 / r of the panel's rows
  F16x2Tuning f16x2_;
  Bf16x3Tuning bf16x3_;
};
class PanelStager {
 public:
  // The context's two alternating buffers for fits of n rows and outer blocks up to max(512, nbo_wide) columns, sized for
  // the largest format `requested` may fall back to, and the row scales of F16x2.  A reservation that fails clears the HIP
  // error: no scales - begin() resolves to Bf16x3; no buffers - nothing is staged.
  static void reserve(agp_context *ctx, BulkProducts requested, long long n, long long nbo_wide);
  // Before the first panel of a factorisation of A (n x n): the fp16 row scales from its diagonal, which the panels
  // overwrite.  Returns the products in force.
  BulkProducts begin(agp_context *ctx, hipStream_t s, BulkProducts requested, const double *A, long long lda, long long n);
  // P: the panel, rows x K (rows kend.. of the matrix).  The two buffers alternate: the bulk update of step j still reads
  // its copy while step j + 1 makes the next one; the copy of step j + 2 is written after U2(j) has been waited for.
  // Nothing is staged where the copy does not fit its buffer or K is no whole number of the format's K chunks.
  StagedPanel stage(hipStream_t s, const double *P, long long ldp, long long rows, long long K, long long kend);
  StagedPanel unstaged(const double *P, long long ldp) const;  // the panel of a step too short for a copy to pay

 private:
  agp_context *ctx_ = nullptr;
  BulkProducts products_ = BulkProducts::Fp64;
  const double *rs_ = nullptr, *irs_ = nullptr;  // F16x2: the row scales r and 1 / r of the whole matrix
  bool flip_ = false;                            // which of the two buffers is next
};
}  // namespace agp
