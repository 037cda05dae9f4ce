// contract_internal.h — what gradient.hip and sparse_gradient.hip share with the probes of debug_api.hip: the argument
// records of the contraction kernels (contract.h: contract_tile) and one host launcher per kernel, each with the grid and
// block arithmetic of the product, which calls it too.  Not part of the public interface.
#pragma once
#include "common.h"
#include "contract.h"

namespace agp {

// ---- contraction of a weight's lower triangle: tile blockIdx.x of the row-major lower enumeration (gradient.hip) ----
struct ContractArgs {
  TangentSlots<GRAD_GROUP> slots;
  const double *tang[GRAD_GROUP];  // AGP_OP_SCALING slot g: its tangent column (n values), else nullptr
  const double *C;                 // K^-1 (LOO: S = C diag(b) C), lower triangle
  long long ldc;
  const double *alpha;
  const double *u;                 // LOO only: u = C a
  double *partial;                 // [tile][GRAD_GROUP]
};

// ---- the batched contraction (agp_nll_gradient_batch, agp_loo_nll_gradient_batch) -----------------------------------
// One descriptor per problem, built on the host for the call and uploaded with it: the program by value (not the
// context's device program cache, whose slots later problems would overwrite), the features, K^-1 and alpha of the
// problem's slabs, its slot table in groups of GRAD_GROUP and the tangent column of every AGP_OP_SCALING slot.
constexpr int GRAD_GROUPS_MAX = (AGP_MAX_GRADIENT_SLOTS + GRAD_GROUP - 1) / GRAD_GROUP;
struct ContractDesc {
  DevProgram prog;
  FeatView X;
  const double *C;         // K_b^-1 (LOO: S_b = C_b diag(b) C_b), lower triangle
  long long ldc;
  const double *alpha;
  const double *u;         // LOO only: u_b = C_b a_b
  double *partial;         // [group][tile][GRAD_GROUP]
  int n_slots;
  int pad;
  TangentSlots<GRAD_GROUP> slots[GRAD_GROUPS_MAX];
  const double *tang[GRAD_GROUPS_MAX * GRAD_GROUP];
};

// ---- the sparse GP's contractions (sparse_gradient.hip): one kernel, three shapes (mode) ------------------------------
//   0  rectangular: rows = feature set R (the inducing points), columns = feature set C (the observations), weight W
//      (rows x cols, ldw), every pair once.  Tiles column-block-major: id = bc * tiles_r + br.
//   1  symmetric over one feature set (R == C): lower tiles only, pairs row >= col, off-diagonal pairs twice
//   2  group blocks: tile ids run over the lower tiles of every group's s_g x s_g slab (tstart[g] = first tile of group
//      g); rows and columns are the points off[g] .. off[g + 1] of ONE feature set, the weight slab of group g is
//      W + woff[g] with leading dimension wld[g]
struct SparseContractArgs {
  TangentSlots<GRAD_GROUP> slots;
  const double *tr[GRAD_GROUP];  // AGP_OP_SCALING slot g: its tangent column at the row features, else nullptr
  const double *tc[GRAD_GROUP];  // ... at the column features
  const double *W;
  long long ldw;
  long long tiles_r;           // mode 0: row tiles
  const long long *off, *woff, *wld, *tstart;  // mode 2
  long long G;
  double *partial;             // [tile][GRAD_GROUP]
  int mode;
};

// nll_grad_contract_kernel<DIMP, LOO>: one workgroup per lower tile of the X.n x X.n weight (tiles = lower_tiles(X.n))
template <bool LOO>
void launch_contract(hipStream_t s, const DevProgram *P, const FeatView &X, const ContractArgs &a, long long tiles);
// nll_grad_reduce_kernel: out[g] = scale * sum over tiles of partial[tile][g] for the first `count` slots of the group
void launch_grad_reduce(hipStream_t s, const double *partial, long long tiles, int count, double scale, double *out);
// nll_grad_contract_batched_kernel<DIMP, LOO>: grid (tile, problem, slot group); tiles = lower_tiles(the padded n), DIMP
// covers dim_max
template <bool LOO>
void launch_contract_batched(hipStream_t s, int dim_max, const ContractDesc *D, long long tiles, long long count, int groups);
// nll_grad_reduce_batched_kernel: out[b * ldo + slot] = scale * problem b's sum of that slot, groups * GRAD_GROUP slots
void launch_grad_reduce_batched(hipStream_t s, const ContractDesc *D, long long tiles, long long count, int groups, double scale,
                                double *out, long long ldo);
// sparse_contract_kernel<DIMP>: one workgroup per tile of the mode's enumeration (no launch for tiles <= 0)
void launch_sparse_contract(hipStream_t s, const DevProgram *P, const FeatView &R, const FeatView &C, const SparseContractArgs &a,
                            long long tiles);
// sparse_grad_reduce_kernel: out[g] = -1/2 S0[g] - S1[g] - 1/2 S2[g] for the first `count` slots of the group, S_q the sum
// of the t_q tiles of p_q
void launch_sparse_grad_reduce(hipStream_t s, const double *p0, long long t0, const double *p1, long long t1, const double *p2,
                               long long t2, int count, double *out);

}  // namespace agp

// The descriptor of one problem of the batched contraction (gradient.hip): the program by value, the view X (whose n masks
// the phantom pairs of a padded batch), the weight operands, the problem's partials, and its slot table in groups with
// the tangent column tcol + param * tld of every AGP_OP_SCALING slot.  The slot table has passed check_slots.
void fill_contract_desc(agp::ContractDesc &d, const agp_kernel *k, const agp::FeatView &X, const double *C, long long ldc,
                        const double *alpha, const double *u, double *partial, int n_slots, const agp_gradient_slot *slots,
                        const double *tcol, long long tld);
