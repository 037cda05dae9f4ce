// api_internal.h — host-side helpers shared by the translation units that implement the C-ABI
// (api.hip: context / Gram / dense fit / predict; cv_api.hip: leave-one-group-out;
// sparse_api.hip: sparse GP).  Not part of the public interface.  What the batched fits share beyond these helpers -
// argument checks, uploads, Gram tables, factor schedule - is batch_front.h, which builds on this header.
#pragma once
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "contract.h"

namespace agp {
void dev_cache_trim();
void dev_forget(void *p);  // the table of dev_malloc's live blocks drops p: it moved into a context slot (api.hip)
// `elems` doubles (at least one) of a call's scratch from the cached allocator
inline hipError_t alloc_doubles(DevMem<double> &m, size_t elems) {
  return static_cast<hipError_t>(m.alloc_cached(sizeof(double) * (elems ? elems : 1)));
}
void launch_symmetrize(hipStream_t s, double *A, long long ld, long long n);
void launch_transpose_blocks(hipStream_t s, const double *src, double *dst, long long m, long long count);  // reduce.hip
void launch_copy_lower(hipStream_t s, const double *src, long long ld, long long n, double *dst, int *nan_flag);  // reduce.hip
void launch_zero_upper(hipStream_t s, double *A, long long ld, long long n);
void launch_set_identity(hipStream_t s, double *B, long long ld, long long n);
void launch_nan_scan_lower(hipStream_t s, const double *A, long long ld, long long n, int *flag);
void launch_upper_to_lower(hipStream_t s, const double *src, long long ld_src, double *dst, long long ld_dst,
                           long long n);
void launch_gather_cols(hipStream_t s, const double *R, long long ldr, const long long *idx, long long m,
                        long long row0, long long n, double *G, long long ldg);
void launch_gather_vec(hipStream_t s, const double *src, const long long *idx, long long m, const double *sub,
                       double *out);
void launch_negate(hipStream_t s, double *A, long long ld, long long m, double *diag_out);
void launch_matvec(hipStream_t s, const double *W, long long ld, long long m, long long n, const double *x,
                   double *partial, double alpha, double beta, const double *base, double *out);
void launch_contract_combinations(hipStream_t s, const double *K, long long ldk, const long long *xoff, const double *xc, long long na,
                                  const long long *yoff, const double *yc, long long nb, bool symmetric, double *out, long long ldo);
// (no launch for more than TALL_MATVEC_MAX_COLS columns: common.h)
void launch_tall_matvec(hipStream_t s, const double *W, long long ld, long long rows, long long ncols, const double *x, double alpha,
                        double beta, const double *base, double *out);
void launch_tall_matvec_f32(hipStream_t s, const float *W, long long ld, long long rows, long long ncols, const double *x, double alpha,
                            double beta, const double *base, double *out);
void launch_colvec_dot_f32(hipStream_t s, const float *W, long long ld, long long m, long long n, const double *v,
                           double alpha, double beta, const double *base, double *out);
void launch_convert_lower_f32(hipStream_t s, const double *L, long long ld, long long n, float *L32);
void launch_colvec_dot(hipStream_t s, const double *W, long long ld, long long m, long long n, const double *v,
                       double alpha, double beta, const double *base, double *out);
void launch_colvec_dot_strided(hipStream_t s, const double *W, long long ld, long long stride_W, long long m, long long n,
                               const double *v, long long stride_v, double alpha, double beta, const double *base, double *out,
                               long long count);
// out = alpha K p + beta base for a symmetric K given by its LOWER triangle only (reduce.hip); ws: symv_ws_elems(n) doubles
size_t symv_ws_elems(long long n);
void launch_symv_lower(hipStream_t s, const double *K, long long ld, long long n, const double *p, double alpha, double beta,
                       const double *base, double *out, double *ws);
// out_b = K_b p_b for `count` such matrices in one launch, without scratch: K_b = K + b * stride_K, p_b and out_b at
// stride_v (blockIdx.y = problem)
void launch_symv_lower_batched(hipStream_t s, const double *K, long long ld, long long stride_K, long long n, const double *p,
                               long long stride_v, double *out, long long count);
void launch_axpby(hipStream_t s, long long n, double a, const double *x, double b, const double *y, double *out);
void launch_loo(hipStream_t s, const double *kinv_diag, const double *y, const double *information, long long n,
                double *mean, double *variance);
void launch_colvec_dot_batched(hipStream_t s, const double *Q, long long ld, long long stride_Q, long long m,
                               const double *z, long long stride_z, long long count, double *out);
void launch_set_identity_batched(hipStream_t s, double *B, long long ld, long long stride, long long m, long long count);
void launch_pad_columns(hipStream_t s, const double *src, long long ld_src, const long long *off, long long smax,
                        long long n_groups, long long rows, double *dst, long long ld_dst, int dir);
void launch_pad_identity(hipStream_t s, double *A, long long ld, long long stride, const long long *off, long long smax,
                         long long n_groups);
void launch_compact_blocks(hipStream_t s, const double *slabs, long long ld, long long stride, const long long *off,
                           const long long *boff, long long smax, long long n_groups, double *out);
long long round_up(long long x, long long m);
long long factor_ld(long long n);
// fits grown by agp_fit_update carry phantom rows (common.h: agp_fit::phantom); update_api.hip
long long fit_real_rows(const agp_fit *f);
int fit_compact_vector(agp_context *ctx, const agp_fit *f, const double *padded_dev, double *real_out, int location);
int fit_expand_matrix(agp_context *ctx, const agp_fit *f, const double *real_in, long long ldr, long long nrhs, double *padded_dev,
                      long long ldp, int location);
int fit_compact_matrix(agp_context *ctx, const agp_fit *f, const double *padded_dev, long long ldp, long long nrhs, double *real_out,
                       long long ldr, int location);
void fit_zero_phantom_rows(hipStream_t s, const agp_fit *f, double *V, long long ldv, long long cols);
// pivoted L D L^T (ldlt.hip)
void ldlt_factor(hipStream_t s, double *A, long long lda, long long n, const long long *tr_host, double *temp, int *info,
                 double *scal);
void ldlt_factor_blocked(hipStream_t s, double *Ap, long long lda, long long n, double *T, double *dotacc, int *info);
void ldlt_permute_sym(hipStream_t s, const double *S, long long lds, const long long *q_dev, long long n, double *Ap,
                      long long lda);
void ldlt_solve(hipStream_t s, const double *A, long long lda, long long n, const long long *q_dev, double *W,
                double *R, long long ldw, long long nrhs);
void ldlt_sqrt_solve(hipStream_t s, const double *A, long long lda, long long n, const long long *q_dev, double *W,
                     const double *R, long long ldw, long long nrhs);
// column-pivoted Householder QR and the substitutions against R (qr.hip)
void colpiv_qr(hipStream_t s, double *A, long long lda, long long rows, long long cols, long long extra, double *tau,
               long long *perm, double *norms, double *state);
void qr_extract_r(hipStream_t s, const double *A, long long lda, long long m, double *R, long long ldr, double inflate);
void qr_root(hipStream_t s, const double *R, long long ldr, const long long *perm, long long m, double *T, long long ldt);
void qr_sqrt_solve(hipStream_t s, const double *R, long long ldr, const long long *perm, long long m, const double *X,
                   long long ldx, double *W, long long ldw, long long nrhs);
void qr_back_solve(hipStream_t s, const double *R, long long ldr, const long long *perm, long long m, long long np, double *c,
                   double *out);
}  // namespace agp

// holds a fit while its maker builds it: an early return destroys it (its blocks go to the context's slots)
struct FitDestroy {
  void operator()(agp_fit *f) const { agp_fit_destroy(f); }
};
using FitGuard = std::unique_ptr<agp_fit, FitDestroy>;

struct agp_ldlt {
  agp_context *ctx = nullptr;
  long long n = 0, lda = 0;
  agp::DevMem<double> A;        // matrixLDLT: L strictly below the diagonal (unit diagonal implied), D on it
  agp::DevMem<long long> q_dev; // the permutation the transpositions compose to: (P b)[i] = b[q[i]]
  std::vector<long long> tr;
  std::vector<double> d;        // vectorD (host copy)
  int success = 1;              // Eigen's info() == Success
};

struct ProgSlot {
  unsigned long long uid = 0;
  agp::DevMem<agp::DevProgram> dev;
};

struct agp_context_ext {
  ProgSlot slots[8];
  int next = 0;
};

extern std::atomic<unsigned long long> g_kernel_uid;

struct agp_kernel_full : agp_kernel {
  unsigned long long uid;
};


struct agp_context_impl : agp_context {
  agp_context_ext ext;
  std::vector<hipEvent_t> gemm_events;
  std::vector<double> gemm_flops;
  hipEvent_t stage_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double gemm_ms_sum = 0., gemm_flop_sum = 0.;
  int gemm_launches = 0;
  // helper contexts (own streams / workspaces) for host threads that work through independent
  // small problems concurrently (the blocks of a sparse GP); created on first use
  std::vector<agp_context *> helpers;
};

// device copy of a kernel program (small LRU ring per context)
int device_program(agp_context *ctx, const agp_kernel *k, const agp::DevProgram **out);
int validate_features(const agp_features *f);
// device view of a feature vector (uploads host data; `copy` forces an owned device copy)
int to_device(agp_context *ctx, const agp_features *f, bool copy, agp::DeviceFeatures *out);
// grow a scratch buffer of the context that launches on ctx->stream may still read: waits for the stream before the old
// block goes, and reports a failure in last_error
int reserve_ws(agp_context *ctx, agp::GrowBuf<double> &ws, size_t need);
int vector_to_device(agp_context *ctx, const double *src, long long n, int location, double *dst);
int copy_out(agp_context *ctx, const double *dev, long long count, double *dst, int location);
int copy_out_2d(agp_context *ctx, const double *dev, long long ld_dev, long long rows, long long cols, double *dst,
                long long ld_dst, int location);
int status_from_flags(const agp_context *ctx);
// slot table of a gradient entry (gradient.hip): every slot a leaf node and a parameter the leaf has; n_tangent_columns:
// the highest AGP_OP_SCALING tangent column + 1
int check_slots(const agp_kernel *k, int n_slots, const agp_gradient_slot *slots, int *n_tangent_columns);
// slots [g0, g0 + GRAD_GROUP) of the table as one group of the contraction (gradient.hip; slots past n_slots: node -1);
// scaling[j]: slot j is an AGP_OP_SCALING leaf, whose tangent column is group.param[j].  Returns the number of used slots.
int fill_slot_group(const agp_kernel *k, int n_slots, const agp_gradient_slot *slots, int g0,
                    agp::TangentSlots<agp::GRAD_GROUP> &group, bool (&scaling)[agp::GRAD_GROUP]);
// ntc tangent columns of n values (leading dimension ld) where the kernels read them (gradient.hip): host columns are
// copied to *cursor with leading dimension round_up(n, 2) and the cursor moves past them, device ones are read in place
int stage_tangents(agp_context *ctx, hipStream_t s, const double *tangents, long long ld, int location, long long n, int ntc,
                   double **cursor, const double **dev, long long *ld_dev);
// ---- leave-one-group-out: the chunks of groups that advance in lock step (gradient.hip) --------------------------------
// The non-empty groups sorted by size and cut into chunks: a chunk is padded to its largest group, which is at most twice
// its smallest, holds at most max(n, m) padded columns (value only: the gathered columns of R fit the slab L leaves) and a
// bounded volume of tile images.  Every chunk is ONE chain of batched launches (blockIdx.y = group), so the number of
// chains follows the number of size classes (<= log2 n, plus the splits of a class too large for one chunk), not the
// number of groups.  meta: per chunk idx[count * m] (-1 = padding) then sizes[count]; term_off: the chunk's first NLL term.
struct LogoChunk {
  long long m, count, idx_off, size_off, term_off;
};
struct LogoPlan {
  std::vector<long long> meta;
  std::vector<LogoChunk> chunks;
  std::vector<long long> group;  // term q belongs to the caller's group group[q]
  long long terms = 0;
  size_t block_elems = 0, img_elems = 0, vec_elems = 0, count_elems = 0;
};
namespace agp {
struct LogoRegions;  // batch_layout.h
}
long long logo_img_stride(long long m);
// AGP_ERR_INVALID_ARGUMENT for malformed offsets, an index out of range, or an index that occurs twice (in one group or
// in two); empty groups are dropped, points in no group are allowed
int logo_plan(long long n, int64_t n_groups, const int64_t *offsets, const int64_t *indices, LogoPlan &p);
// the halves of a chunk's value chain on either side of the sigma kernel, and the fixed-order sum of the terms.
// group_flags: 4 status words per group of the chunk (agp_logo_nll_gradient_batch, whose groups belong to different
// problems); nullptr: the context's one status for all of them
void logo_chunk_sigma(agp_context_impl *ctx, const agp::LogoRegions &r, const LogoChunk &ch, int *group_flags = nullptr);
void logo_chunk_terms(agp_context_impl *ctx, const agp::LogoRegions &r, const LogoChunk &ch, bool marginal, int *group_flags = nullptr);
// the limits of one chunk, shared with the pooled plan of agp_logo_nll_gradient_batch (logo_batch_plan.h)
long long logo_chunk_groups_max();
long long logo_chunk_img_elems_max();
void launch_logo_sum(hipStream_t s, const double *term, long long count, double *out);
namespace agp {
// Gram + LL^T + forward substitution of y exactly as agp_nll makes them (api.hip: build_and_factor); on return the stream
// is synchronised and ctx->h_flags / h_scalars hold the status and the log determinant
int build_and_factor_nll(agp_context *c, const DevProgram *dprog, const DevProgram *hprog, const FeatView &xm, double *A,
                         long long lda, double *invd, double *y, const double *yvar);
// C (lower tiles, ldc) = R^T R for a lower-triangular n x n R (gradient.hip)
void launch_rtr_lower(hipStream_t s, const double *R, long long ldr, long long n, double *C, long long ldc);
// the same for `count` problems in one launch: R_b = R + b * stride_R, C_b = C + b * stride_C (blockIdx.y = problem)
void launch_rtr_lower_batched(hipStream_t s, const double *R, long long ldr, long long stride_R, long long n, double *C,
                              long long ldc, long long stride_C, long long count);
// S (lower tiles, lds) = G^T G for a full n x n G (gradient.hip: agp_loo_nll_gradient's C diag(b) C)
void launch_gtg_lower(hipStream_t s, const double *G, long long ldg, long long n, double *S, long long lds);
// the same for `count` problems in one launch: G_b = G + b * stride_G, S_b = S + b * stride_S (blockIdx.y = problem)
void launch_gtg_lower_batched(hipStream_t s, const double *G, long long ldg, long long stride_G, long long n, double *S,
                              long long lds, long long stride_S, long long count);
}  // namespace agp
// LL^T of a dense matrix at `location` into a fresh factor buffer of `fit` (api.hip: agp_factor_create, agp_nll_dense;
// scores.hip: agp_energy_score).  y (device, optional) receives the fused forward substitution, diag_add (device,
// optional) is added to the diagonal of the copy first.  Returns the status of the factorisation.  (Declared in the
// extern "C" block below.)
namespace agp {
bool gram_sop_enabled();     // api.hip: the AGP_GRAM_SOP switch the Gram launchers of THIS library image follow
void gram_sop_set(bool on);  // (debug_api.hip only: GramSopScope)
void launch_add_diagonal(hipStream_t s, double *A, long long lda, long long n, const double *d);  // scores.hip
// out[i + j * ldo] = entry (i, first_column + j) of agp_standard_normal(seed) (scores.hip)
void launch_standard_normal(hipStream_t s, unsigned long long seed, long long m, long long first_column, long long n_columns,
                            double *out, long long ldo);
// out[i + j * ldo] = +1 where entry (i, first_column + j) of agp_standard_normal(seed) is >= 0, else -1 (scores.hip)
void launch_rademacher(hipStream_t s, unsigned long long seed, long long m, long long first_column, long long n_columns, double *out,
                       long long ldo);
}
// x = L^-T z for ONE vector (api.hip): z is overwritten with x; ws: backsolve_ws_elems(n) doubles of scratch
extern "C" {  // (defined inside api.hip's extern "C" block)
int factor_dense(agp_context *ctx, const double *K, long long n, long long ld, int uplo, int location, agp_fit *fit, double *y,
                 const double *diag_add = nullptr);
// `bytes` of the context's pinned staging area, or nullptr; valid until the call's final synchronisation
void *host_stage(agp_context *ctx, size_t bytes);
long long backsolve_width(long long n);  // the wide path's block width (512), or 0: the 128-row chain
size_t backsolve_ws_elems(long long n);
void backward_solve_vec_any(hipStream_t s, const double *A, long long n, long long lda, const double *invd, double *z,
                            double *ws, long long first_done = 0, hipEvent_t ev_done = nullptr);
// One right-hand side through explicitly inverted BW x BW diagonal blocks W (invert_wide_blocks; n a multiple of BW,
// BW <= TALL_MATVEC_MAX_COLS): z <- L^-1 z and z <- L^-T z in place; partial / xs: n doubles of scratch; A32 (optional):
// the fp32 copy of the factor (launch_convert_lower_f32) for the products with the blocks off the diagonal.
void forward_solve_vec_wide(hipStream_t s, const double *A, long long n, long long lda, const double *W, long long BW,
                            double *z, double *partial, const float *A32 = nullptr);
void backward_solve_vec_wide(hipStream_t s, const double *A, long long n, long long lda, const double *W, long long BW,
                             double *z, double *xs, const float *A32 = nullptr);
// The preconditioner of the mixed fit's refinement (api.hip: refine_information): out = Lt^-T Lt^-1 in, where Lt has the
// factor's BW-wide diagonal blocks in fp64 - applied through their explicit inverses W and the transposed copies WT -
// and the fp32 copy L32 of everything below them.  The caller owns every buffer: W, WT n / BW blocks of BW x BW; L32
// lda x n floats, or nullptr (then the sweeps read the fp64 factor, through forward / backward_solve_vec_wide and
// `scratch`); t1, t2, scratch n doubles each.
struct MixedPreconditioner {
  const double *A = nullptr;
  long long n = 0, lda = 0, BW = 0;
  double *W = nullptr, *WT = nullptr;
  float *L32 = nullptr;
  double *t1 = nullptr, *t2 = nullptr, *scratch = nullptr;
};
// inverts the diagonal blocks into W, transposes them into WT and converts the factor into L32 (when there is one);
// AGP_ERR_INVALID_ARGUMENT, with nothing launched, for a BW the sweeps' kernels do not take
int mixed_precondition_setup(hipStream_t s, const MixedPreconditioner &pc, const double *invd);
// out = M^-1 in; `in` is left as it is
void mixed_precondition_apply(hipStream_t s, const MixedPreconditioner &pc, const double *in, double *out);
// its two sweeps with an L32 (apply is one after the other): t2 = Lt^-1 in, consuming t1; out = Lt^-T t2, consuming t2.
// Declared here ONLY for agp_debug_wide_sweep (debug_api.hip), which copies t2 between them to check each sweep on its
// own: product code calls mixed_precondition_apply - backward alone reads whatever the last forward sweep left in t2.
void mixed_precondition_forward(hipStream_t s, const MixedPreconditioner &pc, const double *in);
void mixed_precondition_backward(hipStream_t s, const MixedPreconditioner &pc, double *out);
}
