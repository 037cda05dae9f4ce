// batch_front.hip — the shared front end of the batched fits (batch_front.h).  Host code only.
#include "batch_front.h"

namespace agp {

BatchGeometry batch_geometry(long long n, long long count) { return BatchGeometry(n, count, factor_ld(n), NB, 36 * MB * MB); }

int check_batch_problems(int count, const agp_kernel *const *kernels, const agp_features *const *features, int64_t ldy,
                         const double *y_var, int64_t ldv, long long *n_out) {
  if (count <= 0 || count > BATCH_MAX_PROBLEMS || !kernels || !features) return AGP_ERR_INVALID_ARGUMENT;
  const long long n = features[0] ? features[0]->n : 0;
  if (n <= 0 || (ldy != 0 && ldy < n) || (y_var && ldv != 0 && ldv < n)) return AGP_ERR_INVALID_ARGUMENT;
  for (int b = 0; b < count; ++b) {
    if (!kernels[b] || !features[b] || features[b]->n != n || features[b]->location != features[0]->location)
      return AGP_ERR_INVALID_ARGUMENT;
    const int st = validate_features(features[b]);
    if (st != AGP_OK) return st;
  }
  *n_out = n;
  return AGP_OK;
}

int check_batch_problems_ragged(int count, const agp_kernel *const *kernels, const agp_features *const *features, int64_t ldy,
                                const double *y_var, int64_t ldv, long long *n_out, bool *equal) {
  if (count <= 0 || count > BATCH_MAX_PROBLEMS || !kernels || !features) return AGP_ERR_INVALID_ARGUMENT;
  long long n = 0;
  bool same = true;
  for (int b = 0; b < count; ++b) {
    if (!kernels[b] || !features[b] || features[b]->n <= 0 || features[b]->location != features[0]->location)
      return AGP_ERR_INVALID_ARGUMENT;
    if (features[b]->n != features[0]->n) same = false;
    if (features[b]->n > n) n = features[b]->n;
  }
  if ((ldy != 0 && ldy < n) || (y_var && ldv != 0 && ldv < n)) return AGP_ERR_INVALID_ARGUMENT;
  for (int b = 0; b < count; ++b) {
    const int st = validate_features(features[b]);
    if (st != AGP_OK) return st;
  }
  *n_out = n;
  *equal = same;
  return AGP_OK;
}

int upload_problem_columns(agp_context *ctx, const double *src, int64_t ld, long long n, long long columns, int location,
                           double *dst, long long ld_dst) {
  const hipMemcpyKind kind = location == AGP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  hipStream_t s = ctx->stream;
  AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, sizeof(double) * (size_t)ld_dst, src, sizeof(double) * (size_t)(ld ? ld : n),
                                      sizeof(double) * (size_t)n, (size_t)(ld ? columns : 1), kind, s));
  if (!ld)
    for (long long b = 1; b < columns; ++b)
      AGP_HIP_CHECK(ctx, hipMemcpyAsync(dst + (size_t)b * (size_t)ld_dst, src, sizeof(double) * (size_t)n, kind, s));
  return AGP_OK;
}

BatchGramTables::BatchGramTables(const BatchGeometry &g, const agp_kernel *const *kernels, double *A, const double *yvar,
                                 long long stride_yvar, int *flags, long long stride_flags)
    : views((size_t)g.count), hprogs((size_t)g.count), outs((size_t)g.count), diag((size_t)g.count, nullptr),
      nanf((size_t)g.count, nullptr) {
  for (long long b = 0; b < g.count; ++b) {
    hprogs[(size_t)b] = &kernels[b]->prog;
    outs[(size_t)b] = A + (size_t)b * (size_t)g.stride_A;
    if (yvar) diag[(size_t)b] = yvar + (size_t)b * (size_t)stride_yvar;
    if (flags) nanf[(size_t)b] = flags + (size_t)b * (size_t)stride_flags;
  }
}

int BatchGramTables::upload_features(agp_context *ctx, const agp_features *const *features) {
  const int count = (int)views.size();
  uploads = std::vector<DeviceFeatures>((size_t)count);
  const agp_features *last = nullptr;
  int last_b = -1;
  for (int b = 0; b < count; ++b) {
    const agp_features *f = features[b];
    const bool same = last && f->coords == last->coords && f->scales == last->scales && f->eq_id == last->eq_id &&
                      f->dim == last->dim && f->n_scale_columns == last->n_scale_columns && f->n == last->n;
    if (!same) {
      const int st = to_device(ctx, f, false, &uploads[(size_t)b]);
      if (st != AGP_OK) return st;
      last = f;
      last_b = b;
    }
    set_view(b, uploads[(size_t)(same ? last_b : b)].v);
  }
  return AGP_OK;
}

int launch_batch_grams(agp_context *ctx, const BatchGeometry &g, const BatchGramTables &t, const agp_kernel *const *kernels,
                       void *table_dev, void *table_pinned) {
  hipStream_t s = ctx->stream;
  if (g.count > 1 && table_dev &&
      launch_gram_batch(s, g.count, t.hprogs.data(), t.views.data(), t.outs.data(), g.lda, t.diag.data(), t.nanf.data(), table_dev,
                        table_pinned))
    return AGP_OK;
  for (long long b = 0; b < g.count; ++b) {
    const DevProgram *dprog = nullptr;
    const int st = device_program(ctx, kernels[b], &dprog);
    if (st != AGP_OK) return st;
    const FeatView &v = t.views[(size_t)b];
    launch_gram(s, dprog, v, v, true, true, t.outs[(size_t)b], g.lda, t.diag[(size_t)b], t.nanf[(size_t)b], t.hprogs[(size_t)b]);
  }
  return AGP_OK;
}

bool batched_lookahead(long long count, long long n) { return (double)count * (double)n * (double)n >= 6e7 && n > 2 * NBO; }

bool batched_fused_panels(agp_context *ctx, const BatchGeometry &g, bool allow_lookahead) {
  return !(allow_lookahead && batched_lookahead(g.count, g.n)) && batched_fused_fits(ctx, g.n, g.count);
}

void launch_batch_prep(hipStream_t s, PrepArgs &prep, const BatchGeometry &g, double *invd, double *zpub) {
  if (zpub) {  // every tile image and every z slot of the batch
    prep.sentinel(invd, g.count * g.stride_I);
    prep.sentinel(zpub, g.count * g.np2);
  }
  launch_prep(s, prep);
}

void factor_batch(agp_context *ctx, const BatchGeometry &g, bool allow_lookahead, double *A, double *invd, double *z, int *flags,
                  long long stride_flags, double *logsum, double *zpub) {
  if (allow_lookahead && batched_lookahead(g.count, g.n))
    factor_lower_batched_lookahead(ctx, A, g.stride_A, g.n, g.lda, invd, g.stride_I, z, g.np2, g.count, flags, logsum, stride_flags);
  else
    factor_lower_batched(ctx->stream, A, g.stride_A, g.n, g.lda, invd, g.stride_I, z, g.np2, g.count, flags, logsum, stride_flags,
                         zpub, g.np2);
}

}  // namespace agp
