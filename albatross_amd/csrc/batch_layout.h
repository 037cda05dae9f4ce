// batch_layout.h — the slab geometry of a batch of fits of one size and the workspace layouts of the entries built on
// it (batch_front.h), each written once: a struct whose members are the regions in order, and a carve function that takes
// them from a WsLayout in that order (a braced list is evaluated left to right).  Plain C++, like ws_layout.h.
// cp2, np2, lda and the tile images are even: every region of doubles is a multiple of 16 bytes, so neighbouring regions
// are contiguous (an entry zero-fills or downloads [logsum | quad | flags] as one range).
#pragma once
#include "ws_layout.h"

namespace agp {

// `count` problems of n points: factor slabs of lda x n at stride_A, the tile images of the nblk diagonal blocks at
// stride_I, per-problem vectors at np2, per-batch scalars in arrays of cp2
struct BatchGeometry {
  long long n, count, lda, nblk, np2, cp2, stride_A, stride_I;
  // block: rows of a diagonal block; image_elems: doubles of one block's tile image (batch_front.h: batch_geometry)
  BatchGeometry(long long n_, long long count_, long long lda_, long long block, long long image_elems)
      : n(n_), count(count_), lda(lda_), nblk((n_ + block - 1) / block), np2((n_ + 1) / 2 * 2), cp2((count_ + 1) / 2 * 2),
        stride_A(lda_ * n_), stride_I(nblk * image_elems) {}
  size_t slabs() const { return (size_t)count * (size_t)stride_A; }
  size_t images() const { return (size_t)count * (size_t)stride_I; }
  size_t vectors() const { return (size_t)count * (size_t)np2; }
};

// agp_nll and the single-problem gradients, ws_A (count = 1)
struct FitRegions {
  double *A, *invd, *z, *yvar;
};
inline FitRegions carve_fit(WsLayout &ws, const BatchGeometry &g) {
  return {ws.take<double>(g.slabs()), ws.take<double>(g.images()), ws.take<double>(g.vectors()), ws.take<double>(g.vectors())};
}

// the single-problem gradients, ws_aux: R = L^-1, back-substitution scratch, partials [tile][GRAD_GROUP], the gradient,
// host tangent columns (leading dimension np2), the entry's own vectors
struct GradientAuxRegions {
  double *R, *bs_ws, *partial, *grad, *tang, *extra;
};
inline GradientAuxRegions carve_gradient_aux(WsLayout &ws, const BatchGeometry &g, size_t bs_elems, size_t part_elems,
                                             size_t grad_elems, size_t tang_elems, size_t extra_elems) {
  return {ws.take<double>(g.slabs()),   ws.take<double>(bs_elems),   ws.take<double>(part_elems),
          ws.take<double>(grad_elems), ws.take<double>(tang_elems), ws.take<double>(extra_elems)};
}

// agp_logo_nll_gradient, the entry's own region at the end of ws_aux (GradientAuxRegions::extra).  S: the third
// lda x n slab (C B C; gradient calls only).  X0 / X1 / X2: the padded block slabs of the chunk of groups in flight
// (A_g then V_g | L_A^-1 then T_g | Sigma_g then B_g), img their tile images, d / z / a_pad its padded vectors, logs_A /
// logs_V its log sums; term: one NLL term per non-empty group; a, u: n-vectors; meta: the padded index tables and
// the group sizes of every chunk.
struct LogoRegions {
  double *S, *X0, *X1, *X2, *img, *d, *z, *a_pad, *logs_A, *logs_V, *term, *a, *u, *symv;
  long long *meta;
};
inline LogoRegions carve_logo(WsLayout &ws, const BatchGeometry &g, bool gradient, size_t block_elems, size_t img_elems,
                              size_t vec_elems, size_t count_elems, size_t term_elems, size_t symv_elems, size_t meta_elems) {
  return {gradient ? ws.take<double>(g.slabs()) : nullptr,
          ws.take<double>(block_elems), ws.take<double>(block_elems), ws.take<double>(block_elems),
          ws.take<double>(img_elems),   ws.take<double>(vec_elems),   ws.take<double>(vec_elems),
          ws.take<double>(vec_elems),   ws.take<double>(count_elems), ws.take<double>(count_elems),
          ws.take<double>(term_elems),  ws.take<double>((size_t)g.np2), ws.take<double>((size_t)g.np2),
          ws.take<double>(symv_elems),  ws.take<long long>(meta_elems)};
}

// agp_logo_nll_gradient_batch, the entry's own region behind its a and u arrays in the extra arrays of
// carve_gradient_batch_aux.  chain.S: the third slab of EVERY problem (count lda x n slabs, C_b B_b C_b; gradient calls only;
// first, so that the descriptors find it at a fixed place); chain.X0 .. term as carve_logo, for the chunk of the POOLED plan
// in flight; chain.a, u, symv: not carved (a and u are np2 x count arrays of the caller, the batched symv needs no scratch);
// chain.meta: the chunk tables and the per-problem term lists (logo_batch_plan.h); gflags: 4 status words per term, which
// the block factorisations write and the per-problem sum folds into the problem's own.
struct LogoBatchRegions {
  LogoRegions chain;
  int *gflags;
};
inline LogoBatchRegions carve_logo_batch(WsLayout &ws, const BatchGeometry &g, bool gradient, size_t block_elems, size_t img_elems,
                                         size_t vec_elems, size_t count_elems, size_t term_elems, size_t meta_elems) {
  LogoBatchRegions r;
  LogoRegions &c = r.chain;
  c.a = c.u = c.symv = nullptr;
  c.S = gradient ? ws.take<double>(g.slabs()) : nullptr;
  c.X0 = ws.take<double>(block_elems);
  c.X1 = ws.take<double>(block_elems);
  c.X2 = ws.take<double>(block_elems);
  c.img = ws.take<double>(img_elems);
  c.d = ws.take<double>(vec_elems);
  c.z = ws.take<double>(vec_elems);
  c.a_pad = ws.take<double>(vec_elems);
  c.logs_A = ws.take<double>(count_elems);
  c.logs_V = ws.take<double>(count_elems);
  c.term = ws.take<double>(term_elems);
  c.meta = ws.take<long long>(meta_elems);
  r.gflags = ws.take<int>(4 * term_elems);
  return r;
}

// agp_sparse_held_out, the entry's one allocation beyond what the fit and the inverse blocks hold.  chain: the regions
// the value chain of a chunk works in (S, a, u, symv: not used, nullptr); M: the chunk's slabs of M_g + nugget I; aw,
// alpha: n-vectors in the grouped order; y, yvar, mean, variance: the same, each only where an output needs it; joint:
// the concatenated blocks cov_g; joff: where each term's block starts in joint.
struct SparseHeldOutRegions {
  LogoRegions chain;
  double *M, *aw, *alpha, *y, *yvar, *mean, *variance, *joint;
  long long *joff;
};
inline SparseHeldOutRegions carve_sparse_held_out(WsLayout &ws, size_t np2, size_t block_elems, size_t img_elems, size_t vec_elems,
                                                  size_t count_elems, size_t term_elems, size_t meta_elems, bool want_y,
                                                  bool want_yvar, bool want_mean, bool want_variance, size_t joint_elems) {
  SparseHeldOutRegions r;
  LogoRegions &c = r.chain;
  c.S = c.a = c.u = c.symv = nullptr;
  c.X0 = ws.take<double>(block_elems);
  c.X1 = ws.take<double>(block_elems);
  c.X2 = ws.take<double>(block_elems);
  r.M = ws.take<double>(block_elems);
  c.img = ws.take<double>(img_elems);
  c.d = ws.take<double>(vec_elems);
  c.z = ws.take<double>(vec_elems);
  c.a_pad = ws.take<double>(vec_elems);
  c.logs_A = ws.take<double>(count_elems);
  c.logs_V = ws.take<double>(count_elems);
  c.term = ws.take<double>(term_elems);
  r.aw = ws.take<double>(np2);
  r.alpha = ws.take<double>(np2);
  r.y = want_y ? ws.take<double>(np2) : nullptr;
  r.yvar = want_yvar ? ws.take<double>(np2) : nullptr;
  r.mean = want_mean ? ws.take<double>(np2) : nullptr;
  r.variance = want_variance ? ws.take<double>(np2) : nullptr;
  r.joint = joint_elems ? ws.take<double>(joint_elems) : nullptr;
  c.meta = ws.take<long long>(meta_elems);
  r.joff = joint_elems ? ws.take<long long>(term_elems) : nullptr;
  return r;
}

// agp_nll_batch, ws_A.  yvar: one vector shared by all problems; zpub: the z slots of the fused panel launches
struct NllBatchRegions {
  double *A, *invd, *ys, *yvar, *logsum, *quad, *zpub;
  void *gram_table;
};
inline NllBatchRegions carve_nll_batch(WsLayout &ws, const BatchGeometry &g, bool fused_panels, size_t gram_table_bytes) {
  return {ws.take<double>(g.slabs()),      ws.take<double>(g.images()),     ws.take<double>(g.vectors()),
          ws.take<double>((size_t)g.np2), ws.take<double>((size_t)g.cp2), ws.take<double>((size_t)g.cp2),
          fused_panels ? ws.take<double>(g.vectors()) : nullptr, ws.take<char>(gram_table_bytes)};
}

// agp_fit_create_batch, the slab the fits share (alpha: information; flags: 4 ints per problem; yvar: scratch of the
// call); the copies of the training features follow on the same WsLayout
struct FitBatchRegions {
  double *A, *invd, *alpha, *z, *logsum;
  int *flags;
  double *yvar;
};
inline FitBatchRegions carve_fit_batch(WsLayout &ws, const BatchGeometry &g, bool has_yvar) {
  return {ws.take<double>(g.slabs()),      ws.take<double>(g.images()),       ws.take<double>(g.vectors()), ws.take<double>(g.vectors()),
          ws.take<double>((size_t)g.cp2), ws.take<int>(4 * (size_t)g.cp2), has_yvar ? ws.take<double>(g.vectors()) : nullptr};
}

// agp_fit_create_batch, the scratch that goes with the call
struct FitBatchTables {
  void *copy_table, *gram_table;
  double *zpub;
};
inline FitBatchTables carve_fit_batch_tables(WsLayout &ws, const BatchGeometry &g, bool fused_panels, size_t copy_table_bytes,
                                             size_t gram_table_bytes) {
  return {ws.take<char>(copy_table_bytes), ws.take<char>(gram_table_bytes), fused_panels ? ws.take<double>(g.vectors()) : nullptr};
}

// agp_fit_update_batch, the slab the grown fits share (g: the geometry of the GROWN size; alpha: information; logsum and
// flags - 4 ints per problem - are one contiguous range, downloaded as one); the grown training features of every
// problem follow on the same WsLayout
struct UpdateBatchRegions {
  double *A, *invd, *alpha, *z, *logsum;
  int *flags;
};
inline UpdateBatchRegions carve_update_batch(WsLayout &ws, const BatchGeometry &g) {
  return {ws.take<double>(g.slabs()),   ws.take<double>(g.images()),     ws.take<double>(g.vectors()),
          ws.take<double>(g.vectors()), ws.take<double>((size_t)g.cp2), ws.take<int>(4 * (size_t)g.cp2)};
}

// agp_fit_update_batch, the scratch that goes with the call: new targets and variances (leading dimension mp2), the
// staged host features, then the descriptor tables of the grow, cross-covariance and prior launches - the tail of the
// region, laid out alike in the pinned staging area
struct UpdateBatchScratch {
  double *ynew, *yvar, *xstage;
  void *grow_table, *cross_table, *gram_table;
};
inline UpdateBatchScratch carve_update_batch_scratch(WsLayout &ws, const BatchGeometry &g, size_t mp2, bool has_yvar, size_t stage_words,
                                                     size_t grow_table_bytes, size_t cross_table_bytes, size_t gram_table_bytes) {
  return {ws.take<double>((size_t)g.count * mp2), has_yvar ? ws.take<double>((size_t)g.count * mp2) : nullptr,
          ws.take<double>(stage_words),           ws.take<char>(grow_table_bytes),
          ws.take<char>(cross_table_bytes),       ws.take<char>(gram_table_bytes)};
}

// the batched gradients, ws_A (z: then alpha, in place; flags: 4 ints per problem)
struct GradientBatchRegions {
  double *A, *invd, *z, *yvar, *logsum, *quad;
  int *flags;
  double *zpub;
};
inline GradientBatchRegions carve_gradient_batch(WsLayout &ws, const BatchGeometry &g, bool has_yvar, bool fused_panels) {
  return {ws.take<double>(g.slabs()),      ws.take<double>(g.images()),     ws.take<double>(g.vectors()),
          has_yvar ? ws.take<double>(g.vectors()) : nullptr,
          ws.take<double>((size_t)g.cp2), ws.take<double>((size_t)g.cp2), ws.take<int>(4 * (size_t)g.cp2),
          fused_panels ? ws.take<double>(g.vectors()) : nullptr};
}

// the batched gradients, ws_aux: R slabs, host tangent columns (leading dimension np2), partials
// [problem][group][tile][GRAD_GROUP], gradients [problem][ldgd], the Gram table, the contraction descriptors, the entry's
// own np2 x count arrays
struct GradientBatchAuxRegions {
  double *R, *tang, *partial, *grad;
  void *gram_table, *desc;
  double *extra;
};
inline GradientBatchAuxRegions carve_gradient_batch_aux(WsLayout &ws, const BatchGeometry &g, size_t tang_elems, size_t part_per,
                                                        size_t ldgd, size_t gram_table_bytes, size_t desc_bytes,
                                                        size_t extra_vectors) {
  return {ws.take<double>(g.slabs()),   ws.take<double>(tang_elems), ws.take<double>((size_t)g.count * part_per),
          ws.take<double>((size_t)g.count * ldgd), ws.take<char>(gram_table_bytes), ws.take<char>(desc_bytes),
          ws.take<double>(extra_vectors * g.vectors())};
}

}  // namespace agp
