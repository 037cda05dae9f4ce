// debug_api.hip — kernel-level entry points used only by tests/ and scripts/ to check and time the
// building blocks (MFMA lane map, update kernel, factorisation) in isolation.
// Not part of include/albatross_amd.h and NOT linked into libalbatross_amd.so: they live in
// libalbatross_amd_debug.so (the product objects + this file; csrc/Makefile), loaded by
// albatross_amd._capi.load_debug().
#include <algorithm>
#include <climits>
#include <cstdio>
#include "common.h"
#include "api_internal.h"
#include "mfma_f64.h"
#include "gram_matvec.h"
#include "gram_tangent.h"
#include "iterative_internal.h"
#include "lanczos_quadrature.h"
#include "contract_internal.h"
#include "shard_internal.h"
#include "pub.h"
#include "trsm_kernel.h"
#include "factor_plan.h"
#include "update_plan.h"
#include "logo_batch_plan.h"
#include <vector>
#include <cstdlib>
#include <cstring>
#include <new>

#define AGP_DEBUG_API __attribute__((visibility("default")))

namespace agp {

__global__ void mfma_tile_kernel(const double *A, const double *B, double *D) {
  const int l = threadIdx.x;
  // A is 16x4 row-major, B is 4x16 row-major, D 16x16 row-major
  v4d acc = v4zero();
  acc = mfma16(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], acc);
  for (int r = 0; r < 4; ++r) D[((l >> 4) + 4 * r) * 16 + (l & 15)] = acc[r];
}

// cycles (s_memtime) and 100 MHz ticks (s_memrealtime) around a loop of
// `iters` x NACC independent v_mfma_f64_16x16x4_f64 per wave
template <int NACC>
__global__ __launch_bounds__(256) void mfma_clock_kernel(unsigned long long *out, int iters, double a0, double b0) {
  v4d acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = v4zero();
  const double a = a0 * (1.0 + (threadIdx.x % 7) * 0.125), b = b0 * (1.0 - (threadIdx.x % 5) * 0.0625);
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = mfma16(a, b, acc[i]);
  }
  double s = 0.;
#pragma unroll
  for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][3];
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = c1 - c0;
    out[2 * blockIdx.x + 1] = r1 - r0;
  }
  if (s == 1.2345e300) out[0] = 0;
}

// NM MFMA + NV independent v_fma_f64 per loop iteration, per wave
template <int NM, int NV>
__global__ __launch_bounds__(256) void mix_clock_kernel(unsigned long long *out, int iters, double a0, double b0) {
  v4d acc[NM > 0 ? NM : 1];
  double v[NV > 0 ? NV : 1];
#pragma unroll
  for (int i = 0; i < (NM > 0 ? NM : 1); ++i) acc[i] = v4zero();
#pragma unroll
  for (int i = 0; i < (NV > 0 ? NV : 1); ++i) v[i] = 0.001 * (i + 1) + threadIdx.x * 1e-6;
  const double a = a0 * (1.0 + (threadIdx.x % 7) * 0.125), b = b0 * (1.0 - (threadIdx.x % 5) * 0.0625);
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < NM; ++i) acc[i] = mfma16(a, b, acc[i]);
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = __builtin_fma(v[i], 0.999999, b);
  }
  double s = 0.;
#pragma unroll
  for (int i = 0; i < (NM > 0 ? NM : 1); ++i) s += acc[i][0] + acc[i][3];
#pragma unroll
  for (int i = 0; i < (NV > 0 ? NV : 1); ++i) s += v[i];
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = c1 - c0;
    out[2 * blockIdx.x + 1] = r1 - r0;
  }
  if (s == 1.2345e300) out[0] = 0;
}

// 64 independent v_fmac_f64 per loop iteration: MODE 0 plain VGPR operands, 1 SGPR src0,
// 2 DPP row_newbcast src0.  out[0..63] (MODE 2 semantics probe): acc after ONE fmac with b = lane id, a = 1.
template <int MODE>
__global__ __launch_bounds__(256) void fmac_rate_kernel(unsigned long long *out, double *probe, int iters, double b0) {
  double acc[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) acc[i] = 0.;
  double a[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = 1.0 + 0.001 * r + threadIdx.x * 1e-6;
  double b = b0 * (1.0 + (threadIdx.x & 63) * 0.01);
  const double bs = __builtin_amdgcn_readfirstlane((int)(b0 * 1000.0)) * 0.001;
  if (probe && MODE == 2) {
    double pa = 1.0, pb = (double)(threadIdx.x & 63), pacc = 0.;
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "+v"(pacc) : "v"(pb), "v"(pa));
    if (blockIdx.x == 0 && threadIdx.x < 64) probe[threadIdx.x] = pacc;
  }
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      if (MODE == 0) asm volatile("v_fmac_f64_e32 %0, %1, %2" : "+v"(acc[i]) : "v"(b), "v"(a[i & 3]));
      else if (MODE == 1) asm volatile("v_fmac_f64_e32 %0, %1, %2" : "+v"(acc[i]) : "s"(bs), "v"(a[i & 3]));
      else asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:7 row_mask:0xf bank_mask:0xf" : "+v"(acc[i]) : "v"(b), "v"(a[i & 3]));
    }
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  double s = 0.;
#pragma unroll
  for (int i = 0; i < 64; ++i) s += acc[i];
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = c1 - c0;
    out[2 * blockIdx.x + 1] = r1 - r0;
  }
  if (s == 1.2345e300) out[0] = 0;
}

}  // namespace agp

using namespace agp;

// Bare issue loops of the two fp64 MFMA shapes: mode 0 = v_mfma_f64_16x16x4_f64 with NACC independent
// accumulators, mode 1 = v_mfma_f64_4x4x4_4b_f64 (four 4 x 4 x 4 blocks, 512 flop) with NACC accumulators.
template <int MODE, int NACC>
__global__ __launch_bounds__(256) void mfma_shape_kernel(double *sink, int iters, double a0, double b0) {
  double a = a0 + threadIdx.x * 1e-9, b = b0 - threadIdx.x * 1e-9;
  double s = 0.;
  if (MODE == 0) {
    agp::v4d acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = agp::v4zero();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  } else if (MODE == 1) {
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, acc[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NACC; ++i) s += acc[i];
  } else {
    // mode 2: as mode 1 but with 16 different A and 4 different B operand registers (the GEMM pattern)
    double acc[NACC], av[16], bv[4];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.;
    // a0 < 0 selects operands with random mantissas in [1, 2) x (+-1): data-dependent power
    unsigned h = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 12345u;
    auto rnd = [&]() {
      h ^= h << 13; h ^= h >> 17; h ^= h << 5;
      const unsigned lo = h;
      h ^= h << 13; h ^= h >> 17; h ^= h << 5;
      const unsigned hi = (h & 0x800fffffu) | 0x3ff00000u;
      return __hiloint2double((int)hi, (int)lo);
    };
#pragma unroll
    for (int i = 0; i < 16; ++i) av[i] = a0 < 0. ? rnd() * 0.01 : a + i * 1e-3;
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = a0 < 0. ? rnd() * 0.01 : b - i * 1e-3;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[i & 15], bv[(i >> 4) & 3], acc[i], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(av[i]));
    }
#pragma unroll
    for (int i = 0; i < NACC; ++i) s += acc[i];
  }
  if (s == 123.456) sink[0] = s;
}


// Lane-map probe of v_mfma_f64_4x4x4_4b_f64: for every pair (la, lb) the operand A is one-hot in lane la and
// B one-hot in lane lb; out[(la * 64 + lb)] = mask of result lanes that are non-zero.
template <int CBSZ, int ABID>
__global__ __launch_bounds__(64) void mfma44_probe_kernel(unsigned long long *out) {
  const int lane = threadIdx.x;
  for (int la = 0; la < 64; ++la)
    for (int lb = 0; lb < 64; ++lb) {
      const double a = lane == la ? 1. : 0., b = lane == lb ? 1. : 0.;
      const double d = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0., CBSZ, ABID, 0);
      const unsigned long long m = __ballot(d != 0.);
      if (lane == 0) out[la * 64 + lb] = m;
    }
}

// exp_neg (cov_eval.h) on an array: accuracy test against the correctly rounded exp
__global__ void exp_neg_kernel(const double *t, double *out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = agp::exp_neg(t[i]);
}
extern "C" AGP_DEBUG_API int agp_debug_exp_neg(agp_context *ctx, const double *t, int64_t n, double *out) {
  if (!ctx || !t || !out || n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double *d = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&d, sizeof(double) * 2 * (size_t)n));
  AGP_HIP_CHECK(ctx, hipMemcpy(d, t, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(exp_neg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d, d + n, (long long)n);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipMemcpy(out, d + n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return AGP_OK;
}

// {sum of shader-clock cycles, sum of 100 MHz ticks, workgroups} of the trailing_update_kernel launches since the last
// reset (a library built with -DAGP_CLOCK_PROBE; zeros otherwise)
extern "C" AGP_DEBUG_API int agp_debug_symv_lower(agp_context *ctx, const double *K, int64_t n, int64_t ld, const double *p,
                                                  double alpha, double beta, const double *base, double *out) {
  if (!ctx || !K || !p || !out || n <= 0 || ld < n) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double *dK = nullptr, *dv = nullptr, *ws = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dK, sizeof(double) * (size_t)ld * (size_t)n));
  AGP_HIP_CHECK(ctx, hipMalloc(&dv, sizeof(double) * 3 * (size_t)n));
  AGP_HIP_CHECK(ctx, hipMalloc(&ws, sizeof(double) * symv_ws_elems(n)));
  AGP_HIP_CHECK(ctx, hipMemcpy(dK, K, sizeof(double) * (size_t)ld * (size_t)n, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dv, p, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  if (base) AGP_HIP_CHECK(ctx, hipMemcpy(dv + n, base, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  launch_symv_lower(ctx->stream, dK, ld, n, dv, alpha, beta, base ? dv + n : nullptr, dv + 2 * n, ws);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipMemcpy(out, dv + 2 * n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  (void)hipFree(dK); (void)hipFree(dv); (void)hipFree(ws);
  return AGP_OK;
}

// C = R^T R (lower tiles; the whole diagonal tiles) for a lower-triangular n x n R, column-major with leading dimension ld:
// the kernel of agp_nll_gradient's K^-1 (gradient.hip: rtr_lower_kernel).  ms (optional): its device time.
extern "C" AGP_DEBUG_API int agp_debug_rtr_lower(agp_context *ctx, const double *R, int64_t n, int64_t ld, double *C,
                                                 double *ms) {
  if (!ctx || !R || !C || n <= 0 || ld < n) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(double) * (size_t)ld * (size_t)n;
  double *dR = nullptr, *dC = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dR, bytes));
  AGP_HIP_CHECK(ctx, hipMalloc(&dC, bytes));
  AGP_HIP_CHECK(ctx, hipMemcpy(dR, R, bytes, hipMemcpyHostToDevice));
  // on the kernel's stream: a hipMemset on the null stream does not order with the context's non-blocking stream and
  // could still be zeroing tiles the kernel has written
  AGP_HIP_CHECK(ctx, hipMemsetAsync(dC, 0, bytes, ctx->stream));
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
  launch_rtr_lower(ctx->stream, dR, ld, n, dC, ld);
  AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  if (ms) *ms = t;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  AGP_HIP_CHECK(ctx, hipMemcpy(C, dC, bytes, hipMemcpyDeviceToHost));
  (void)hipFree(dR); (void)hipFree(dC);
  return AGP_OK;
}

// agp_debug_rtr_lower for `count` problems in one launch (gradient.hip: launch_rtr_lower_batched, agp_nll_gradient_batch's
// K_b^-1): R and C hold `count` slabs of ld * n doubles each.  ms (optional): the kernel's device time.
extern "C" AGP_DEBUG_API int agp_debug_rtr_lower_batched(agp_context *ctx, const double *R, int64_t n, int64_t ld, int64_t count,
                                                         double *C, double *ms) {
  if (!ctx || !R || !C || n <= 0 || ld < n || count <= 0 || count > 65535) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(double) * (size_t)ld * (size_t)n * (size_t)count;
  double *dR = nullptr, *dC = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dR, bytes));
  AGP_HIP_CHECK(ctx, hipMalloc(&dC, bytes));
  AGP_HIP_CHECK(ctx, hipMemcpy(dR, R, bytes, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(dC, 0, bytes, ctx->stream));  // on the kernel's stream, as agp_debug_rtr_lower
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
  launch_rtr_lower_batched(ctx->stream, dR, ld, ld * n, n, dC, ld, ld * n, count);
  AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  if (ms) *ms = t;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  AGP_HIP_CHECK(ctx, hipMemcpy(C, dC, bytes, hipMemcpyDeviceToHost));
  (void)hipFree(dR); (void)hipFree(dC);
  return AGP_OK;
}

// S = G^T G (lower tiles; the whole diagonal tiles) for a full n x n G, column-major with leading dimension ld: the
// kernel of agp_loo_nll_gradient's C diag(b) C (gradient.hip: gtg_lower_kernel).  ms (optional): its device time.
extern "C" AGP_DEBUG_API int agp_debug_gtg_lower(agp_context *ctx, const double *G, int64_t n, int64_t ld, double *S,
                                                 double *ms) {
  if (!ctx || !G || !S || n <= 0 || ld < n) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(double) * (size_t)ld * (size_t)n;
  double *dG = nullptr, *dS = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dG, bytes));
  AGP_HIP_CHECK(ctx, hipMalloc(&dS, bytes));
  AGP_HIP_CHECK(ctx, hipMemcpy(dG, G, bytes, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(dS, 0, bytes, ctx->stream));  // on the kernel's stream, as agp_debug_rtr_lower
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
  launch_gtg_lower(ctx->stream, dG, ld, n, dS, ld);
  AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  if (ms) *ms = t;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  AGP_HIP_CHECK(ctx, hipMemcpy(S, dS, bytes, hipMemcpyDeviceToHost));
  (void)hipFree(dG); (void)hipFree(dS);
  return AGP_OK;
}

// agp_debug_gtg_lower for `count` problems in one launch (gradient.hip: launch_gtg_lower_batched,
// agp_loo_nll_gradient_batch's C_b diag(b) C_b): G and S hold `count` slabs of ld * n doubles each.  ms (optional): the
// kernel's device time.
extern "C" AGP_DEBUG_API int agp_debug_gtg_lower_batched(agp_context *ctx, const double *G, int64_t n, int64_t ld, int64_t count,
                                                         double *S, double *ms) {
  if (!ctx || !G || !S || n <= 0 || ld < n || count <= 0 || count > 65535) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(double) * (size_t)ld * (size_t)n * (size_t)count;
  double *dG = nullptr, *dS = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dG, bytes));
  AGP_HIP_CHECK(ctx, hipMalloc(&dS, bytes));
  AGP_HIP_CHECK(ctx, hipMemcpy(dG, G, bytes, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(dS, 0, bytes, ctx->stream));  // on the kernel's stream, as agp_debug_rtr_lower
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
  launch_gtg_lower_batched(ctx->stream, dG, ld, ld * n, n, dS, ld, ld * n, count);
  AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  if (ms) *ms = t;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  AGP_HIP_CHECK(ctx, hipMemcpy(S, dS, bytes, hipMemcpyDeviceToHost));
  (void)hipFree(dG); (void)hipFree(dS);
  return AGP_OK;
}

// acos_fast (cov_eval.h) on an array: accuracy test against the correctly rounded acos
__global__ void acos_fast_kernel(const double *t, double *out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = agp::acos_fast(t[i]);
}
extern "C" AGP_DEBUG_API int agp_debug_acos_fast(agp_context *ctx, const double *t, int64_t n, double *out) {
  if (!ctx || !t || !out || n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double *d = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&d, sizeof(double) * 2 * (size_t)n));
  AGP_HIP_CHECK(ctx, hipMemcpy(d, t, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(acos_fast_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d, d + n, (long long)n);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipMemcpy(out, d + n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return AGP_OK;
}

// ---- launch-chain latency probe ------------------------------------------------------------------------------
// Synthetic kernels with a chosen static LDS footprint: every workgroup writes a little, then spins `spin` shader
// clocks.  Used to find out what a dependent launch costs on this part when consecutive kernels of one stream
// differ (code, LDS size, grid): the panel chain of the factorisation is such a sequence of tiny launches.
template <int LDS_DOUBLES>
__global__ __launch_bounds__(256) void chain_probe_kernel(double *buf, long long stride, int spin, int touch) {
  __shared__ double lds[LDS_DOUBLES > 0 ? LDS_DOUBLES : 1];
  if (LDS_DOUBLES > 0) lds[threadIdx.x % LDS_DOUBLES] = threadIdx.x;
  __syncthreads();
  double v = (LDS_DOUBLES > 0) ? lds[(threadIdx.x + 1) % (LDS_DOUBLES > 0 ? LDS_DOUBLES : 1)] : 1.0;
  double *p = buf + (long long)blockIdx.x * stride;
  for (int t = 0; t < touch; ++t) p[threadIdx.x + 256 * t] = p[threadIdx.x + 256 * t] * 0.5 + v;
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  while ((long long)(__builtin_amdgcn_s_memtime() - c0) < spin) {}
}

static void launch_probe(hipStream_t s, int kind, int wgs, double *buf, long long stride, int spin, int touch) {
  switch (kind) {
  case 0: hipLaunchKernelGGL(chain_probe_kernel<0>, dim3(wgs), dim3(256), 0, s, buf, stride, spin, touch); break;
  case 1: hipLaunchKernelGGL(chain_probe_kernel<5120>, dim3(wgs), dim3(256), 0, s, buf, stride, spin, touch); break;   // 40 KB
  case 2: hipLaunchKernelGGL(chain_probe_kernel<9344>, dim3(wgs), dim3(256), 0, s, buf, stride, spin, touch); break;   // 73 KB
  default: hipLaunchKernelGGL(chain_probe_kernel<9856>, dim3(wgs), dim3(256), 0, s, buf, stride, spin, touch); break;  // 77 KB
  }
}

extern "C" AGP_DEBUG_API int agp_debug_chain_probe(agp_context *ctx, const int *kinds, const int *wgs, int period, int reps, int spin,
                                     int touch, int priority_stream, double *us_per_launch) {
  if (!ctx || !kinds || !wgs || period <= 0 || reps <= 0 || !us_per_launch) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = priority_stream ? ctx->stream : ctx->stream2;
  const long long stride = 256LL * (touch > 0 ? touch : 1);
  double *buf = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&buf, sizeof(double) * (size_t)stride * 4096));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(buf, 0, sizeof(double) * (size_t)stride * 4096, s));
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  for (int i = 0; i < period * 3; ++i) launch_probe(s, kinds[i % period], wgs[i % period], buf, stride, spin, touch);
  AGP_HIP_CHECK(ctx, hipEventRecord(e0, s));
  for (int i = 0; i < period * reps; ++i) launch_probe(s, kinds[i % period], wgs[i % period], buf, stride, spin, touch);
  AGP_HIP_CHECK(ctx, hipEventRecord(e1, s));
  AGP_HIP_CHECK(ctx, hipEventSynchronize(e1));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  *us_per_launch = 1e3 * ms / (double)(period * reps);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(buf);
  return AGP_OK;
}

// the REAL chain: the panel phase (POTRF, TRSM, inner update per 128 columns) of an n x n block, `reps` times
namespace agp {
void panel_phase_public(agp_context *ctx, hipStream_t s, double *A, long long n, long long lda, double *img, double *y,
                        long long K0, long long kend);
// solve.hip: z[c] -= sum_r L[k0 + r][c] x[r] for c < ncols, r < nbk (back_update_kernel)
void launch_back_update(hipStream_t s, const double *A, long long lda, long long k0, int nbk, long long ncols, const double *x,
                        double *z);
}
// blocked: while the chain runs, `blocked` other streams sit at a hipStreamWaitEvent on an event that is recorded
// behind a long one-workgroup spinner on yet another stream (a queue whose head is an unsatisfied barrier packet)
extern "C" AGP_DEBUG_API int agp_debug_panel_chain(agp_context *ctx, int64_t n, int64_t width, int reps, int blocked, double *us_per_phase) {
  if (!ctx || n <= 0 || width <= 0 || width > n || reps <= 0 || !us_per_phase) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  hipStream_t extra[3] = {nullptr, nullptr, nullptr};
  hipEvent_t gate = nullptr;
  double *spinbuf = nullptr;
  // blocked = -1: only the spinner (a long one-workgroup kernel on another stream), nobody waits on it
  // blocked = -2: a stream blocked in hipStreamWaitValue32 on host memory, NO kernel running elsewhere
  unsigned int *flag = nullptr;
  if (blocked == -2) {
    AGP_HIP_CHECK(ctx, hipStreamCreateWithFlags(&extra[1], hipStreamNonBlocking));
    AGP_HIP_CHECK(ctx, hipExtMallocWithFlags((void **)&flag, 64, hipMallocSignalMemory));
    *flag = 0;
    AGP_HIP_CHECK(ctx, hipMalloc(&spinbuf, sizeof(double) * 4096));
    AGP_HIP_CHECK(ctx, hipStreamWaitValue32(extra[1], flag, 1, hipStreamWaitValueEq, 0xffffffffu));
    hipLaunchKernelGGL(chain_probe_kernel<0>, dim3(1), dim3(256), 0, extra[1], spinbuf, 256, 100, 1);
  }
  if (blocked == -1) {
    AGP_HIP_CHECK(ctx, hipStreamCreateWithFlags(&extra[0], hipStreamNonBlocking));
    AGP_HIP_CHECK(ctx, hipMalloc(&spinbuf, sizeof(double) * 4096));
    hipLaunchKernelGGL(chain_probe_kernel<0>, dim3(1), dim3(256), 0, extra[0], spinbuf, 256, 144000000, 1);
  }
  if (blocked > 0) {
    if (blocked > 2) blocked = 2;
    for (int i = 0; i <= blocked; ++i) AGP_HIP_CHECK(ctx, hipStreamCreateWithFlags(&extra[i], hipStreamNonBlocking));
    AGP_HIP_CHECK(ctx, hipEventCreateWithFlags(&gate, hipEventDisableTiming));
    AGP_HIP_CHECK(ctx, hipMalloc(&spinbuf, sizeof(double) * 4096));
    // ~60 ms spinner (2.4 GHz shader clock) on extra[0]; the gate event completes when it ends
    hipLaunchKernelGGL(chain_probe_kernel<0>, dim3(1), dim3(256), 0, extra[0], spinbuf, 256, 144000000, 1);
    AGP_HIP_CHECK(ctx, hipEventRecord(gate, extra[0]));
    for (int i = 1; i <= blocked; ++i) {
      AGP_HIP_CHECK(ctx, hipStreamWaitEvent(extra[i], gate, 0));
      hipLaunchKernelGGL(chain_probe_kernel<0>, dim3(1), dim3(256), 0, extra[i], spinbuf + 1024 * i, 256, 100, 1);
    }
  }
  const long long lda = n + 8;
  double *A = nullptr, *img = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&A, sizeof(double) * (size_t)lda * (size_t)width));
  AGP_HIP_CHECK(ctx, hipMalloc(&img, sizeof(double) * (size_t)((width + NB - 1) / NB) * 36 * 256));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(A, 0, sizeof(double) * (size_t)lda * (size_t)width, s));  // zeros: NaN results, same timing
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  agp::panel_phase_public(ctx, s, A, n, lda, img, nullptr, 0, width);
  AGP_HIP_CHECK(ctx, hipEventRecord(e0, s));
  for (int r = 0; r < reps; ++r) agp::panel_phase_public(ctx, s, A, n, lda, img, nullptr, 0, width);
  AGP_HIP_CHECK(ctx, hipEventRecord(e1, s));
  AGP_HIP_CHECK(ctx, hipEventSynchronize(e1));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  *us_per_phase = 1e3 * ms / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(A);
  (void)hipFree(img);
  if (flag) *flag = 1;  // release the stream blocked on host memory
  if (blocked != 0) {
    (void)hipDeviceSynchronize();
    for (auto st : extra) if (st) (void)hipStreamDestroy(st);
    if (gate) (void)hipEventDestroy(gate);
    (void)hipFree(spinbuf);
    if (flag) (void)hipFree(flag);
  }
  return AGP_OK;
}

extern "C" {

AGP_DEBUG_API int agp_debug_mfma_tile(agp_context *ctx, const double *A, const double *B, double *D) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double *d = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&d, sizeof(double) * (64 + 64 + 256)));
  AGP_HIP_CHECK(ctx, hipMemcpy(d, A, sizeof(double) * 64, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(d + 64, B, sizeof(double) * 64, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_tile_kernel, dim3(1), dim3(64), 0, ctx->stream, d, d + 64, d + 128);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipMemcpy(D, d + 128, sizeof(double) * 256, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipFree(d));
  return AGP_OK;
}

// out[0] = median cycles per MFMA per wave, out[1] = effective clock (GHz),
// out[2] = chip TFLOP/s.  waves_per_simd in {1, 2}; nacc in {1, 4, 8}.
AGP_DEBUG_API int agp_debug_mfma_clock(agp_context *ctx, int blocks, int waves_per_simd, int nacc, int iters, double a0,
                         double b0, double *out) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int nblk = blocks * waves_per_simd;
  unsigned long long *d = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&d, sizeof(unsigned long long) * 2 * nblk));
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  for (int rep = 0; rep < 2; ++rep) {
    AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
    if (nacc == 1) hipLaunchKernelGGL(mfma_clock_kernel<1>, dim3(nblk), dim3(256), 0, ctx->stream, d, iters, a0, b0);
    else if (nacc == 4) hipLaunchKernelGGL(mfma_clock_kernel<4>, dim3(nblk), dim3(256), 0, ctx->stream, d, iters, a0, b0);
    else hipLaunchKernelGGL(mfma_clock_kernel<8>, dim3(nblk), dim3(256), 0, ctx->stream, d, iters, a0, b0);
    AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
    AGP_HIP_CHECK(ctx, hipEventSynchronize(e1));
  }
  float ms = 0.f;
  AGP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> h(2 * nblk);
  AGP_HIP_CHECK(ctx, hipMemcpy(h.data(), d, sizeof(unsigned long long) * 2 * nblk, hipMemcpyDeviceToHost));
  std::vector<double> cyc(nblk), clk(nblk);
  const int na = nacc == 1 ? 1 : (nacc == 4 ? 4 : 8);
  for (int i = 0; i < nblk; ++i) {
    cyc[i] = (double)h[2 * i] / ((double)iters * na);
    clk[i] = (double)h[2 * i] / ((double)h[2 * i + 1] * 10.0) ;  // cycles per 10 ns tick -> GHz
  }
  std::sort(cyc.begin(), cyc.end());
  std::sort(clk.begin(), clk.end());
  out[0] = cyc[nblk / 2];
  out[1] = clk[nblk / 2];
  out[2] = (double)nblk * 4.0 * iters * na * 2048.0 / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(d);
  return AGP_OK;
}

// out[0] = cycles per loop iteration per wave, out[1] = clock GHz, out[2] = chip TFLOP/s (MFMA + VALU flops)
AGP_DEBUG_API int agp_debug_mix_clock(agp_context *ctx, int waves_per_simd, int variant, int iters, double *out) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int nblk = 256 * waves_per_simd;
  unsigned long long *d = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&d, sizeof(unsigned long long) * 2 * nblk));
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  int nm = 0, nv = 0;
  for (int rep = 0; rep < 2; ++rep) {
    AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
#define MIX(NM_, NV_) { nm = NM_; nv = NV_; hipLaunchKernelGGL((mix_clock_kernel<NM_, NV_>), dim3(nblk), dim3(256), 0, ctx->stream, d, iters, 1.1, 0.9); }
    switch (variant) {
    case 0: MIX(0, 16) break;
    case 1: MIX(0, 32) break;
    case 2: MIX(4, 0) break;
    case 3: MIX(4, 16) break;
    case 4: MIX(4, 32) break;
    case 5: MIX(4, 64) break;
    case 6: MIX(4, 96) break;
    case 7: MIX(2, 48) break;
    default: MIX(4, 48) break;
    }
#undef MIX
    AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
    AGP_HIP_CHECK(ctx, hipEventSynchronize(e1));
  }
  float ms = 0.f;
  AGP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> h(2 * nblk);
  AGP_HIP_CHECK(ctx, hipMemcpy(h.data(), d, sizeof(unsigned long long) * 2 * nblk, hipMemcpyDeviceToHost));
  std::vector<double> cyc(nblk), clk(nblk);
  for (int i = 0; i < nblk; ++i) {
    cyc[i] = (double)h[2 * i] / (double)iters;
    clk[i] = (double)h[2 * i] / ((double)h[2 * i + 1] * 10.0);
  }
  std::sort(cyc.begin(), cyc.end());
  std::sort(clk.begin(), clk.end());
  out[0] = cyc[nblk / 2];
  out[1] = clk[nblk / 2];
  out[2] = (double)nblk * 4.0 * iters * (nm * 2048.0 + nv * 128.0) / (ms * 1e-3) / 1e12;
  out[3] = nm; out[4] = nv;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(d);
  return AGP_OK;
}

// C (M x N, ldc) -= A * B^T on host arrays.
//   a_kmajor == 0: A is M x K column-major (lda >= M); else K x M column-major (lda >= K)
//   b_kmajor likewise with N.
AGP_DEBUG_API int agp_debug_gemm(agp_context *ctx, double *C, int64_t ldc, const double *A, int64_t lda, int a_kmajor,
                   const double *B, int64_t ldb, int b_kmajor, int64_t M, int64_t N, int64_t K, int tri) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t cb = sizeof(double) * (size_t)ldc * (size_t)N;
  const size_t ab = sizeof(double) * (size_t)lda * (size_t)(a_kmajor ? M : K);
  const size_t bb = sizeof(double) * (size_t)ldb * (size_t)(b_kmajor ? N : K);
  double *dC = nullptr, *dA = nullptr, *dB = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dC, cb));
  AGP_HIP_CHECK(ctx, hipMalloc(&dA, ab));
  AGP_HIP_CHECK(ctx, hipMalloc(&dB, bb));
  AGP_HIP_CHECK(ctx, hipMemcpy(dC, C, cb, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dA, A, ab, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dB, B, bb, hipMemcpyHostToDevice));
  launch_gemm_nt_sub(ctx->stream, dC, ldc, dA, lda, a_kmajor != 0, dB, ldb, b_kmajor != 0, M, N, K, tri != 0);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(C, dC, cb, hipMemcpyDeviceToHost));
  (void)hipFree(dC); (void)hipFree(dA); (void)hipFree(dB);
  return AGP_OK;
}

// v_fmac_f64 issue rate with VGPR (mode 0), SGPR (1) or DPP row_newbcast (2) src0.
// out[0] = cycles per 64-FMA iteration per wave, out[1] = clock GHz, out[2] = chip TFLOP/s;
// probe[64] (mode 2): result of one fmac with b = lane id, a = 1, row_newbcast:5.
AGP_DEBUG_API int agp_debug_fmac_rate(agp_context *ctx, int waves_per_simd, int mode, int iters, double *out, double *probe) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int nblk = 256 * waves_per_simd;
  unsigned long long *d = nullptr;
  double *dp = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&d, sizeof(unsigned long long) * 2 * nblk));
  AGP_HIP_CHECK(ctx, hipMalloc(&dp, sizeof(double) * 64));
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  for (int rep = 0; rep < 2; ++rep) {
    AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
    if (mode == 0) hipLaunchKernelGGL(fmac_rate_kernel<0>, dim3(nblk), dim3(256), 0, ctx->stream, d, dp, iters, 1.1);
    else if (mode == 1) hipLaunchKernelGGL(fmac_rate_kernel<1>, dim3(nblk), dim3(256), 0, ctx->stream, d, dp, iters, 1.1);
    else hipLaunchKernelGGL(fmac_rate_kernel<2>, dim3(nblk), dim3(256), 0, ctx->stream, d, dp, iters, 1.1);
    AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
    AGP_HIP_CHECK(ctx, hipEventSynchronize(e1));
  }
  float ms = 0.f;
  AGP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> h(2 * nblk);
  AGP_HIP_CHECK(ctx, hipMemcpy(h.data(), d, sizeof(unsigned long long) * 2 * nblk, hipMemcpyDeviceToHost));
  if (probe) AGP_HIP_CHECK(ctx, hipMemcpy(probe, dp, sizeof(double) * 64, hipMemcpyDeviceToHost));
  std::vector<double> cyc(nblk), clk(nblk);
  for (int i = 0; i < nblk; ++i) {
    cyc[i] = (double)h[2 * i] / (double)iters;
    clk[i] = (double)h[2 * i] / ((double)h[2 * i + 1] * 10.0);
  }
  std::sort(cyc.begin(), cyc.end());
  std::sort(clk.begin(), clk.end());
  out[0] = cyc[nblk / 2];
  out[1] = clk[nblk / 2];
  out[2] = (double)nblk * 4.0 * iters * 64.0 * 128.0 / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(d); (void)hipFree(dp);
  return AGP_OK;
}

// mode 0: cbsz = 0; mode 1..4: cbsz = 2, abid = mode - 1.  out: 4096 masks.
AGP_DEBUG_API int agp_debug_mfma44_probe(agp_context *ctx, int mode, unsigned long long *out) {
  if (!ctx || !out) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  unsigned long long *d = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&d, sizeof(unsigned long long) * 4096));
  hipStream_t s = ctx->stream;
  switch (mode) {
    case 0: hipLaunchKernelGGL((mfma44_probe_kernel<0, 0>), dim3(1), dim3(64), 0, s, d); break;
    case 1: hipLaunchKernelGGL((mfma44_probe_kernel<2, 0>), dim3(1), dim3(64), 0, s, d); break;
    case 2: hipLaunchKernelGGL((mfma44_probe_kernel<2, 1>), dim3(1), dim3(64), 0, s, d); break;
    case 3: hipLaunchKernelGGL((mfma44_probe_kernel<2, 2>), dim3(1), dim3(64), 0, s, d); break;
    default: hipLaunchKernelGGL((mfma44_probe_kernel<2, 3>), dim3(1), dim3(64), 0, s, d); break;
  }
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(out, d, sizeof(unsigned long long) * 4096, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  (void)hipFree(d);
  return AGP_OK;
}


// out[0] = chip TFLOP/s, out[1] = ms
AGP_DEBUG_API int agp_debug_mfma_shape(agp_context *ctx, int mode, int nacc, int waves_per_simd, int iters, double *out) {
  const double a0 = iters < 0 ? -1.0 : 1.0;  // negative iteration count: random operands
  if (iters < 0) iters = -iters;
  if (!ctx || !out) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double *sink = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&sink, 8));
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  const int blocks = 256 * waves_per_simd;
  hipStream_t s = ctx->stream;
  for (int rep = 0; rep < 2; ++rep) {
    AGP_HIP_CHECK(ctx, hipEventRecord(e0, s));
#define SHAPE_LAUNCH(M_, N_) hipLaunchKernelGGL((mfma_shape_kernel<M_, N_>), dim3(blocks), dim3(256), 0, s, sink, iters, a0, 2.0)
    if (mode == 0 && nacc == 8) SHAPE_LAUNCH(0, 8);
    else if (mode == 0 && nacc == 16) SHAPE_LAUNCH(0, 16);
    else if (mode == 1 && nacc == 8) SHAPE_LAUNCH(1, 8);
    else if (mode == 1 && nacc == 16) SHAPE_LAUNCH(1, 16);
    else if (mode == 1 && nacc == 32) SHAPE_LAUNCH(1, 32);
    else if (mode == 1 && nacc == 64) SHAPE_LAUNCH(1, 64);
    else if (mode == 2 && nacc == 64) SHAPE_LAUNCH(2, 64);
    else if (mode == 2 && nacc == 32) SHAPE_LAUNCH(2, 32);
    else return AGP_ERR_INVALID_ARGUMENT;
#undef SHAPE_LAUNCH
    AGP_HIP_CHECK(ctx, hipEventRecord(e1, s));
    AGP_HIP_CHECK(ctx, hipEventSynchronize(e1));
  }
  float ms = 0.f;
  AGP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, e0, e1));
  const double flop_per_mfma = mode == 0 ? 2.0 * 16 * 16 * 4 : 2.0 * 4 * 4 * 4 * 4;
  out[0] = (double)blocks * 4.0 * (double)iters * nacc * flop_per_mfma / (ms * 1e-3) / 1e12;
  out[1] = ms;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(sink);
  return AGP_OK;
}

// The panel of a probe (host copy hP, device copy dP: rows x K) staged as the mixed fit stages a step's panel - through the
// fit's own PanelStager and the context's buffers.  The fp16 row scales come from a diagonal of the panel's squared row
// norms - the bound a Cholesky factor's rows obey.  A probe runs the products it names: a fall-back is an error.
static int stage_probe_panel(agp_context *ctx, agp::BulkProducts products, const double *hP, const double *dP, long long ldp,
                             long long rows, long long K, agp::StagedPanel *out) {
  std::vector<double> diag((size_t)rows, 0.);
  for (long long k = 0; k < K; ++k)
    for (long long i = 0; i < rows; ++i) diag[(size_t)i] += hP[i + k * ldp] * hP[i + k * ldp];
  agp::DevMem<double> d_diag;
  AGP_HIP_CHECK(ctx, d_diag.alloc_plain(sizeof(double) * (size_t)rows));
  AGP_HIP_CHECK(ctx, hipMemcpy(d_diag, diag.data(), sizeof(double) * (size_t)rows, hipMemcpyHostToDevice));
  agp::PanelStager::reserve(ctx, products, rows, K);
  agp::PanelStager stager;
  const bool in_force = stager.begin(ctx, ctx->stream, products, d_diag, 0, rows) == products;
  if (in_force) *out = stager.stage(ctx->stream, dP, ldp, rows, K, 0);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (!in_force || !out->staged()) {
    ctx->last_error = "the panel copy of a probe was not staged";
    return AGP_ERR_HIP;
  }
  return AGP_OK;
}

// The kernel selector of the bulk-update probes below: the ONE place their integers become a BulkKernel (update_plan.h).
// 0: the fp64 product launch, 3: the fp32-product kernel, 30 / 31: every tile a whole 128 x 128 workgroup on the ring loop /
// on the register-staged loop.  Every other integer runs the fp64 product launch too: 2, 4 and 5 once named kernels that
// are gone (a VALU kernel, all-quadrants, a tile tail), and tests and scripts still pass them.
static agp::BulkKernel bulk_kernel_of(int variant) {
  return variant == 3 ? agp::BulkKernel::Fp32Products : variant == 30 ? agp::BulkKernel::Fp64WholeRing
       : variant == 31 ? agp::BulkKernel::Fp64WholeRegisterStaged : agp::BulkKernel::Fp64;
}

// Bulk trailing update C (M x M, lower tiles) -= P P^T on host data.  variant: bulk_kernel_of (with 30 / 31 shapes of a few
// tile rows reach the large tile bodies), and 13 / 14 / 15: the fp32-product kernel on an fp32 copy of the panel / the
// bf16 x 3 kernel on its three bf16 planes / the fp16 x 2 kernel on the two fp16 planes of its scaled rows, staged and applied
// as the mixed fit does; 20 + h: the merged update with a head of h tile columns.
AGP_DEBUG_API int agp_debug_trailing_update(agp_context *ctx, double *C, int64_t ldc, const double *P, int64_t ldp, int64_t M,
                              int64_t K, int variant) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  const agp::BulkProducts products = variant == 13 ? agp::BulkProducts::Fp32 : variant == 14 ? agp::BulkProducts::Bf16x3
                                   : variant == 15 ? agp::BulkProducts::F16x2 : agp::BulkProducts::Fp64;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t cb = sizeof(double) * (size_t)ldc * (size_t)M;
  const size_t pb = sizeof(double) * (size_t)ldp * (size_t)K;
  double *dC = nullptr, *dP = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dC, cb));
  AGP_HIP_CHECK(ctx, hipMalloc(&dP, pb));
  AGP_HIP_CHECK(ctx, hipMemcpy(dC, C, cb, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dP, P, pb, hipMemcpyHostToDevice));
  int st = AGP_OK;
  if (agp::is_mixed(products)) {
    agp::StagedPanel staged;
    st = stage_probe_panel(ctx, products, P, dP, ldp, M, K, &staged);
    if (st == AGP_OK) staged.apply(ctx->stream, dC, ldc, 0, M, M, K);
  } else if (variant >= 20 && variant < 30) {
    // the MERGED update of factor_lower with head_cols = variant - 20: the launch on the bulk stream, the gate kernel on
    // the chain stream (it must end - the head counted itself completely - although the launch it waits for is on another
    // stream), and the count it left must be exactly the number of head tiles
    unsigned long long *cnt = ctx->d_headcnt + 7, seen = ~0ull;
    AGP_HIP_CHECK(ctx, hipMemset(cnt, 0, sizeof(unsigned long long)));
    AGP_HIP_CHECK(ctx, hipMemset(ctx->d_flags, 0, 4 * sizeof(int)));
    long long head_tiles = 0;
    launch_trailing_update_merged(ctx->stream2, dC, ldc, dP, ldp, M, K, variant - 20, cnt, &head_tiles);
    launch_head_gate(ctx->stream, cnt, (unsigned long long)head_tiles, ctx->d_flags);
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream2));
    int flags[4] = {0, 0, 0, 0};
    AGP_HIP_CHECK(ctx, hipMemcpy(&seen, cnt, sizeof(seen), hipMemcpyDeviceToHost));
    AGP_HIP_CHECK(ctx, hipMemcpy(flags, ctx->d_flags, sizeof(flags), hipMemcpyDeviceToHost));
    if (seen != (unsigned long long)head_tiles || flags[2] != 0 || head_tiles <= 0) st = AGP_ERR_HIP;
  } else {
    launch_trailing_update_as(bulk_kernel_of(variant), ctx->stream, dC, ldc, dP, dP, ldp, M, K);
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(C, dC, cb, hipMemcpyDeviceToHost));
  (void)hipFree(dC); (void)hipFree(dP);
  return st;
}

// C (M x N lower tiles; C(0, 0) at row row_offset of the panel) -= P[row_offset ..] P[row_offset ..]^T with the products
// named (3 / 4 / 5: factor_plan.h, BulkProducts) from a copy of the WHOLE panel P (rows x K) - staged and applied as
// factor_lower does for the next block column (N < M, offset 0) and for the bulk update (M == N at an offset).  The host
// C has ldc rows and N + 128 columns: the 128 guard columns behind the updated ones travel to the device and back, so that
// the caller sees a kernel that writes beyond column N.
AGP_DEBUG_API int agp_debug_staged_update(agp_context *ctx, double *C, int64_t ldc, const double *P, int64_t ldp, int64_t rows, int64_t K,
                                          int products, int64_t row_offset, int64_t M, int64_t N) {
  const agp::BulkProducts bp = (agp::BulkProducts)products;
  if (!ctx || !C || !P || !agp::is_mixed(bp) || K <= 0 || N <= 0 || N > M || row_offset < 0 || row_offset + M > rows || ldc < M || ldp < rows)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t cb = sizeof(double) * (size_t)ldc * (size_t)(N + 128);
  const size_t pb = sizeof(double) * (size_t)ldp * (size_t)K;
  agp::DevMem<double> dC, dP;
  AGP_HIP_CHECK(ctx, dC.alloc_plain(cb));
  AGP_HIP_CHECK(ctx, dP.alloc_plain(pb));
  AGP_HIP_CHECK(ctx, hipMemcpy(dC, C, cb, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dP, P, pb, hipMemcpyHostToDevice));
  agp::StagedPanel staged;
  const int st = stage_probe_panel(ctx, bp, P, dP, ldp, rows, K, &staged);
  if (st != AGP_OK) return st;
  staged.apply(ctx->stream, dC, ldc, row_offset, M, N, K);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(C, dC, cb, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// One outer step's panel of the mixed fit, staged and applied exactly as factor_lower does - PanelStager::begin on the
// caller's diagonal, PanelStager::stage at kend = first_row, StagedPanel::apply - with everything the step leaves behind
// handed back (tests/test_split_plane_kernels_gpu.py).
//   products   3 / 4 / 5 (factor_plan.h, BulkProducts); P: the panel, rows x K (ldp)
//   diag       first_row + rows diagonal entries of the matrix the panel belongs to: panel row 0 is matrix row first_row,
//              so its fp16 scales are those of diag[first_row]
//   C, ldc, row_offset, M, N   as agp_debug_staged_update, the 128 guard columns included; C == NULL: the copy is made and
//              nothing is applied
//   copy_out   (optional, copy_bytes long) the staged copy as it lies in the context's buffer: the planes, padding
//              included (split_planes_bytes), or the fp32 copy (*ld32_out floats per column).  The buffer is filled with
//              0xff bytes before the panel is staged, so whatever the conversion did not write comes back as 0xff.
//   rs_out, irs_out   (optional, first_row + rows each) the row scales r and 1 / r (products 5 only)
// Returns AGP_OK when the copy was staged in the format asked for, AGP_DEBUG_NOT_STAGED when PanelStager declined to make a
// copy (K no whole number of chunks, no buffer) and AGP_DEBUG_OTHER_PRODUCTS when begin() resolved to another format; in
// both of these nothing is applied and C comes back unchanged.
enum { AGP_DEBUG_NOT_STAGED = 100, AGP_DEBUG_OTHER_PRODUCTS = 101 };
AGP_DEBUG_API int agp_debug_split_plane_step(agp_context *ctx, int products, const double *P, int64_t ldp, int64_t rows, int64_t K,
                                             const double *diag, int64_t first_row, double *C, int64_t ldc, int64_t row_offset,
                                             int64_t M, int64_t N, void *copy_out, int64_t copy_bytes, int64_t *ld32_out,
                                             double *rs_out, double *irs_out) {
  const agp::BulkProducts bp = (agp::BulkProducts)products;
  if (!ctx || !P || !diag || !agp::is_mixed(bp) || rows <= 0 || K <= 0 || ldp < rows || first_row < 0 || copy_bytes < 0) return AGP_ERR_INVALID_ARGUMENT;
  if (C && (N <= 0 || N > M || row_offset < 0 || row_offset + M > rows || ldc < M)) return AGP_ERR_INVALID_ARGUMENT;
  if ((rs_out || irs_out) && bp != agp::BulkProducts::F16x2) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const long long n = first_row + rows;
  const size_t cb = C ? sizeof(double) * (size_t)ldc * (size_t)(N + 128) : 0;
  const size_t pb = sizeof(double) * (size_t)ldp * (size_t)K;
  agp::DevMem<double> dC, dP, d_diag;
  if (C) {
    AGP_HIP_CHECK(ctx, dC.alloc_plain(cb));
    AGP_HIP_CHECK(ctx, hipMemcpy(dC, C, cb, hipMemcpyHostToDevice));
  }
  AGP_HIP_CHECK(ctx, dP.alloc_plain(pb));
  AGP_HIP_CHECK(ctx, hipMemcpy(dP, P, pb, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, d_diag.alloc_plain(sizeof(double) * (size_t)n));
  AGP_HIP_CHECK(ctx, hipMemcpy(d_diag, diag, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  agp::PanelStager::reserve(ctx, bp, n, K);
  // a new PanelStager hands out the first of the context's two buffers first
  const size_t half = ctx->panel_copies.bytes() / 2;
  if ((size_t)copy_bytes > half) return AGP_ERR_INVALID_ARGUMENT;
  if (ctx->panel_copies && copy_bytes > 0) AGP_HIP_CHECK(ctx, hipMemsetAsync(ctx->panel_copies.get(), 0xFF, (size_t)copy_bytes, ctx->stream));
  agp::PanelStager stager;
  if (stager.begin(ctx, ctx->stream, bp, d_diag, 0, n) != bp) {
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return AGP_DEBUG_OTHER_PRODUCTS;
  }
  const agp::StagedPanel staged = stager.stage(ctx->stream, dP, ldp, rows, K, first_row);
  if (!staged.staged()) {
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return AGP_DEBUG_NOT_STAGED;
  }
  if (C) staged.apply(ctx->stream, dC, ldc, row_offset, M, N, K);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (C) AGP_HIP_CHECK(ctx, hipMemcpy(C, dC, cb, hipMemcpyDeviceToHost));
  if (copy_out && copy_bytes > 0) AGP_HIP_CHECK(ctx, hipMemcpy(copy_out, ctx->panel_copies.get(), (size_t)copy_bytes, hipMemcpyDeviceToHost));
  if (ld32_out) {  // (PanelStager::stage: whole groups of 8 rows, and no multiple of 512)
    *ld32_out = (rows + 7) / 8 * 8;
    if (*ld32_out % 512 == 0) *ld32_out += 8;
  }
  if (rs_out) AGP_HIP_CHECK(ctx, hipMemcpy(rs_out, ctx->f16_scales.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  if (irs_out)
    AGP_HIP_CHECK(ctx, hipMemcpy(irs_out, ctx->f16_scales.get() + ctx->f16_scales_n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// The bulk trailing update on a stream restricted to a CU mask (hipExtStreamCreateWithCUMask): mask_words 32-bit words, bit i = CU i.
// At the same time (optional, chain_reps > 0) the panel chain of an n = M block runs on the context's main stream:
// *chain_us = its time per 512-wide panel phase while the masked bulk updates are in flight.
AGP_DEBUG_API int agp_debug_time_masked_update(agp_context *ctx, int64_t M, int64_t K, int variant, int reps, const uint32_t *mask,
                                 int mask_words, int chain_reps, double *ms_out, double *chain_us) {
  if (!ctx || M <= 0 || K <= 0 || reps <= 0 || !ms_out) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t sm = nullptr;
  if (mask && mask_words > 0) AGP_HIP_CHECK(ctx, hipExtStreamCreateWithCUMask(&sm, (uint32_t)mask_words, mask));
  else AGP_HIP_CHECK(ctx, hipStreamCreateWithFlags(&sm, hipStreamNonBlocking));
  const long long ld = M + 8;
  double *dC = nullptr, *dP = nullptr, *pA = nullptr, *pimg = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dC, sizeof(double) * (size_t)ld * (size_t)M));
  AGP_HIP_CHECK(ctx, hipMalloc(&dP, sizeof(double) * (size_t)ld * (size_t)K));
  AGP_HIP_CHECK(ctx, hipMemset(dC, 0, sizeof(double) * (size_t)ld * (size_t)M));
  AGP_HIP_CHECK(ctx, hipMemset(dP, 0, sizeof(double) * (size_t)ld * (size_t)K));
  const long long pw = 512, plda = M + 8;
  AGP_HIP_CHECK(ctx, hipMalloc(&pA, sizeof(double) * (size_t)plda * (size_t)pw));
  AGP_HIP_CHECK(ctx, hipMalloc(&pimg, sizeof(double) * 4 * 36 * 256));
  AGP_HIP_CHECK(ctx, hipMemset(pA, 0, sizeof(double) * (size_t)plda * (size_t)pw));
  hipEvent_t e0, e1, c0, c1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  AGP_HIP_CHECK(ctx, hipEventCreate(&c0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&c1));
  for (int r = -2; r < reps; ++r) {
    if (r == 0) AGP_HIP_CHECK(ctx, hipEventRecord(e0, sm));
    launch_trailing_update_as(bulk_kernel_of(variant), sm, dC, ld, dP, dP, ld, M, K);
    if (r == 0 && chain_reps > 0) {
      AGP_HIP_CHECK(ctx, hipEventRecord(c0, ctx->stream));
      for (int c = 0; c < chain_reps; ++c) agp::panel_phase_public(ctx, ctx->stream, pA, M, plda, pimg, nullptr, 0, pw);
      AGP_HIP_CHECK(ctx, hipEventRecord(c1, ctx->stream));
    }
  }
  AGP_HIP_CHECK(ctx, hipEventRecord(e1, sm));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  float ms = 0.f;
  AGP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, e0, e1));
  *ms_out = (double)ms / reps;
  if (chain_us) {
    *chain_us = 0.;
    if (chain_reps > 0) {
      AGP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, c0, c1));
      *chain_us = 1e3 * (double)ms / chain_reps;
    }
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(c0); (void)hipEventDestroy(c1);
  (void)hipFree(dC); (void)hipFree(dP); (void)hipFree(pA); (void)hipFree(pimg);
  (void)hipStreamDestroy(sm);
  return AGP_OK;
}

// Average milliseconds of `reps` bulk trailing updates of an M x M matrix (device-side random-ish data).
// (variants 30 / 31 in alternation: the ring loop against the register-staged loop in one build, scripts/time_update_k.py)
AGP_DEBUG_API int agp_debug_time_trailing_update(agp_context *ctx, int64_t M, int64_t K, int variant, int reps, double *ms_out) {
  if (!ctx || M <= 0 || K <= 0 || reps <= 0) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const long long ld = M + 8;
  double *dC = nullptr, *dP = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dC, sizeof(double) * (size_t)ld * (size_t)M));
  AGP_HIP_CHECK(ctx, hipMalloc(&dP, sizeof(double) * (size_t)ld * (size_t)K));
  std::vector<double> h((size_t)ld * (size_t)K);
  unsigned long long x = 88172645463325252ull;
  for (auto &v : h) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5; }
  // (AGP_DEBUG_ZERO_OPERANDS=1: how much of the kernel's time depends on the DATA - at K = 512 the update is 11 % faster on
  // zeros, at K = 2048 not at all: power, with the memory traffic as the swing term; profiles/r04/bulk_update_vs_k.txt)
  // (=1: panel and C zero, =2: the panel only, =3: C only)
  int zero_mode = getenv("AGP_DEBUG_ZERO_OPERANDS") ? atoi(getenv("AGP_DEBUG_ZERO_OPERANDS")) : 0;
  std::vector<double> hz;
  if (zero_mode) hz.assign(h.size(), 0.);
  if (zero_mode == 4) { zero_mode = 2; hz.assign(h.size(), 0.3); }                                         // constant panel
  if (zero_mode == 5) { zero_mode = 2; for (size_t i = 0; i < h.size(); ++i) hz[i] = h[i] < 0. ? -0.3 : 0.3; }  // random signs only
  if (zero_mode == 6) { zero_mode = 2; for (size_t i = 0; i < h.size(); ++i) hz[i] = (i % 7 == 0) ? h[i] : 0.; }  // 1 in 7 entries non-zero
  AGP_HIP_CHECK(ctx, hipMemcpy(dP, (zero_mode == 1 || zero_mode == 2) ? hz.data() : h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  for (long long c = 0; c < M; c += K) {
    const long long w = (M - c < K) ? M - c : K;
    AGP_HIP_CHECK(ctx, hipMemcpy(dC + c * ld, (zero_mode == 1 || zero_mode == 3) ? hz.data() : h.data(), sizeof(double) * (size_t)ld * (size_t)w,
                            hipMemcpyHostToDevice));
  }
  hipEvent_t e0, e1;
  AGP_HIP_CHECK(ctx, hipEventCreate(&e0));
  AGP_HIP_CHECK(ctx, hipEventCreate(&e1));
  int st = AGP_OK;
  // variants 4 / 5 / 6: the low-precision products of the mixed fit - fp32 panel copy / bf16 x 3 / fp16 x 2 of scaled rows -
  // on a copy of the panel staged once
  const agp::BulkProducts products = variant == 4 ? agp::BulkProducts::Fp32 : variant == 5 ? agp::BulkProducts::Bf16x3
                                   : variant == 6 ? agp::BulkProducts::F16x2 : agp::BulkProducts::Fp64;
  agp::StagedPanel staged;
  if (agp::is_mixed(products))
    st = stage_probe_panel(ctx, products, (zero_mode == 1 || zero_mode == 2) ? hz.data() : h.data(), dP, ld, M, K, &staged);
  for (int r = -2; r < reps && st == AGP_OK; ++r) {
    if (r == 0) AGP_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
    if (agp::is_mixed(products)) staged.apply(ctx->stream, dC, ld, 0, M, M, K);
    else launch_trailing_update_as(bulk_kernel_of(variant), ctx->stream, dC, ld, dP, dP, ld, M, K);
  }
  if (st == AGP_OK) {
    AGP_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
    AGP_HIP_CHECK(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    AGP_HIP_CHECK(ctx, hipEventElapsedTime(&ms, e0, e1));
    *ms_out = (double)ms / reps;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(dC); (void)hipFree(dP);
  return st;
}

// X = L^-1 B for L = the LL^T factor of the host matrix K (n x n, lower triangle, ld n) through
// forward_solve_wide (solve.hip): out of place, explicitly inverted 512 x 512 diagonal blocks.  n a multiple of 512.
// The device buffers have the leading dimension n + 2 and X enters filled with NaN.  ldx = n: X (n x ncols) receives the n
// rows of the result; ldx = n + 2: the whole padded buffer, so that the caller sees its two padding rows.  L_out
// (optional, n x n, ld n): the factor the solve ran against.
AGP_DEBUG_API int agp_debug_forward_solve_wide(agp_context *ctx, const double *K, int64_t n, const double *B, int64_t ncols, double *X,
                                               int64_t ldx, double *L_out) {
  if (!ctx || !K || !B || !X || n < 1024 || n % 512 != 0 || ncols <= 0 || (ldx != n && ldx != n + 2)) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  agp_fit *f = nullptr;
  int st = agp_factor_create(ctx, K, n, n, 0, AGP_HOST, &f);
  if (st != AGP_OK) return st;
  const long long ldb = n + 2;  // (a right-hand side whose leading dimension is not the matrix's)
  double *dB = nullptr, *dX = nullptr, *dW = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dB, sizeof(double) * (size_t)ldb * (size_t)ncols));
  AGP_HIP_CHECK(ctx, hipMalloc(&dX, sizeof(double) * (size_t)ldb * (size_t)ncols));
  AGP_HIP_CHECK(ctx, hipMalloc(&dW, sizeof(double) * (size_t)n * 512));
  AGP_HIP_CHECK(ctx, hipMemcpy2D(dB, sizeof(double) * (size_t)ldb, B, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)ncols,
                                 hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(dX, 0xFF, sizeof(double) * (size_t)ldb * (size_t)ncols, ctx->stream));  // (all ones: a NaN)
  invert_wide_blocks(ctx->stream, f->A, n, f->lda, f->invd, WIDE_BW, dW);
  forward_solve_wide(ctx->stream, f->A, n, f->lda, dW, dB, ldb, dX, ldb, ncols);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy2D(X, sizeof(double) * (size_t)ldx, dX, sizeof(double) * (size_t)ldb, sizeof(double) * (size_t)ldx, (size_t)ncols,
                                 hipMemcpyDeviceToHost));
  if (L_out)
    AGP_HIP_CHECK(ctx, hipMemcpy2D(L_out, sizeof(double) * (size_t)n, f->A, sizeof(double) * (size_t)f->lda, sizeof(double) * (size_t)n,
                                   (size_t)n, hipMemcpyDeviceToHost));
  (void)hipFree(dB); (void)hipFree(dX); (void)hipFree(dW);
  agp_fit_destroy(f);
  return AGP_OK;
}

// ONE substitution of solve.hip on host data, with the buffers prepared as the product prepares them (tests/test_substitutions_gpu.py).
//   K      `count` SPD matrices (n x n, ld n, one after the other), each factored by agp_factor_create
//   lda    0: the substitution runs on the factor's own A / lda / invd (count = 1); >= n: the factors and their tile images are
//          copied into slabs with this leading dimension, `count` of them at strides LARGER than a slab, gaps and padding
//          rows NaN (the batched kinds; the vector kinds at an odd leading dimension)
//   B      the caller's whole right-hand side buffer, b_doubles long, padding and gaps included: copied in, run in place,
//          copied back.  Problem p starts at B + p * stride_B; its leading dimension is ldb.
//   rows, cols   the shape of one right-hand side: n x m for the left solves, nrows x n for the right solves, n x 1 for a vector
//   opt    rhs_lower of the forward kinds; k0 of SUB_BACK_UPDATE
//   flags_out (2 * count ints): [2 p] the hand-over time-out flag of problem p (flags[2] of the one-launch kinds),
//          [2 p + 1] 1 if forward_solve_mat_lookahead's conditions for its two-stream path held
//   L_out  (optional, count x n x n, ld n) the factors;  W_out (optional, ceil(n / 128) x 128 x 128) the inverted diagonal
//          blocks of the vector kinds, as the kernels read them
// A batched kind with count = 1 and stride_B = 0 passes zero strides throughout.
enum {
  SUB_FWD_MAT = 0, SUB_FWD_MAT_LOOKAHEAD, SUB_FWD_MAT_BATCHED, SUB_BWD_MAT, SUB_RIGHT_LT, SUB_RIGHT_LT_BATCHED, SUB_FWD_VEC,
  SUB_BWD_VEC, SUB_BWD_VEC_BATCHED, SUB_COOP_DIRECT, SUB_COOP_FLAGS, SUB_COOP_BATCHED, SUB_BACK_UPDATE, SUB_KINDS
};
AGP_DEBUG_API int agp_debug_substitute(agp_context *ctx, int kind, const double *K, int64_t n, int64_t count, int64_t lda, double *B,
                                       int64_t b_doubles, int64_t rows, int64_t cols, int64_t ldb, int64_t stride_B, int64_t opt,
                                       int *flags_out, double *L_out, double *W_out) {
  if (!ctx || !K || !B || !flags_out || kind < 0 || kind >= SUB_KINDS || n <= 0 || count <= 0 || count > 4096 || rows <= 0 ||
      cols <= 0 || ldb < rows || stride_B < 0 || (lda != 0 && lda < n))
    return AGP_ERR_INVALID_ARGUMENT;
  const bool batched = kind == SUB_FWD_MAT_BATCHED || kind == SUB_RIGHT_LT_BATCHED || kind == SUB_BWD_VEC_BATCHED || kind == SUB_COOP_BATCHED;
  const bool right = kind == SUB_RIGHT_LT || kind == SUB_RIGHT_LT_BATCHED;
  const bool vector = kind == SUB_FWD_VEC || kind == SUB_BWD_VEC || kind == SUB_BWD_VEC_BATCHED || kind == SUB_COOP_DIRECT ||
                      kind == SUB_COOP_FLAGS || kind == SUB_COOP_BATCHED;
  const bool coop = kind == SUB_COOP_DIRECT || kind == SUB_COOP_FLAGS || kind == SUB_COOP_BATCHED;
  const long long nblk = (n + NB - 1) / NB;
  const bool zero_strides = batched && count == 1 && stride_B == 0;
  if (!batched && count != 1) return AGP_ERR_INVALID_ARGUMENT;
  if (batched && !zero_strides && lda == 0) return AGP_ERR_INVALID_ARGUMENT;
  if ((right ? cols : rows) != n && kind != SUB_BACK_UPDATE) return AGP_ERR_INVALID_ARGUMENT;
  if (vector && cols != 1) return AGP_ERR_INVALID_ARGUMENT;
  const long long one_rhs = ldb * (cols - 1) + rows;  // doubles one right-hand side spans
  if (!zero_strides && batched && stride_B < one_rhs) return AGP_ERR_INVALID_ARGUMENT;
  if (b_doubles < (count - 1) * stride_B + one_rhs) return AGP_ERR_INVALID_ARGUMENT;
  long long k0 = 0, nbk0 = 0;
  if (kind == SUB_BACK_UPDATE) {  // B: column 0 = z (k0 doubles), column 1 = x (nbk doubles)
    k0 = opt;
    if (k0 <= 0 || k0 >= n || k0 % NB != 0 || cols != 2 || rows < k0) return AGP_ERR_INVALID_ARGUMENT;
    nbk0 = n - k0 < NB ? n - k0 : NB;
    if (rows < nbk0) return AGP_ERR_INVALID_ARGUMENT;
  }
  if (coop) {
    // only what the product dispatches (api.hip: fit_create_impl, agp_fit_create_batch): the kernel's liveness argument
    // and its hand-over modes are stated for these shapes
    if (!ctx->tune.backsub_coop || n > ctx->tune.backsub_coop_max) return AGP_ERR_INVALID_ARGUMENT;
    if (kind != SUB_COOP_FLAGS && nblk > BACKSUB_DIRECT_BLOCKS) return AGP_ERR_INVALID_ARGUMENT;
    if (kind == SUB_COOP_FLAGS && nblk <= BACKSUB_DIRECT_BLOCKS) return AGP_ERR_INVALID_ARGUMENT;
  }
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  for (int64_t p = 0; p < count; ++p) { flags_out[2 * p] = 0; flags_out[2 * p + 1] = 0; }

  // ---- the factors: the fit's own buffers, or NaN-padded slabs
  agp_fit *own = nullptr;
  double *slabA = nullptr, *slabI = nullptr;
  const double *A = nullptr, *invd = nullptr;
  long long ldA = 0, stride_A = 0, stride_I = 0;
  int st = AGP_OK;
  auto cleanup = [&]() {
    if (own) agp_fit_destroy(own);
    if (slabA) (void)hipFree(slabA);
    if (slabI) (void)hipFree(slabI);
  };
  if (lda == 0) {
    st = agp_factor_create(ctx, K, n, n, 0, AGP_HOST, &own);
    if (st != AGP_OK) { cleanup(); return st; }
    A = own->A; invd = own->invd; ldA = own->lda;
    if (L_out)
      AGP_HIP_CHECK(ctx, hipMemcpy2D(L_out, sizeof(double) * (size_t)n, own->A, sizeof(double) * (size_t)own->lda,
                                     sizeof(double) * (size_t)n, (size_t)n, hipMemcpyDeviceToHost));
  } else {
    ldA = lda;
    stride_A = round_up(lda * n, 2) + 10;              // (even: the slabs keep the 16-byte alignment of the first)
    stride_I = nblk * (long long)IMG_DOUBLES + 6;
    AGP_HIP_CHECK(ctx, hipMalloc(&slabA, sizeof(double) * (size_t)stride_A * (size_t)count));
    AGP_HIP_CHECK(ctx, hipMalloc(&slabI, sizeof(double) * (size_t)stride_I * (size_t)count));
    AGP_HIP_CHECK(ctx, hipMemset(slabA, 0xFF, sizeof(double) * (size_t)stride_A * (size_t)count));  // (all ones: a NaN)
    AGP_HIP_CHECK(ctx, hipMemset(slabI, 0xFF, sizeof(double) * (size_t)stride_I * (size_t)count));
    for (int64_t p = 0; p < count; ++p) {
      agp_fit *f = nullptr;
      st = agp_factor_create(ctx, K + (size_t)p * (size_t)n * (size_t)n, n, n, 0, AGP_HOST, &f);
      if (st != AGP_OK) { if (f) agp_fit_destroy(f); cleanup(); return st; }
      hipError_t e = hipMemcpy2D(slabA + p * stride_A, sizeof(double) * (size_t)lda, f->A, sizeof(double) * (size_t)f->lda,
                                 sizeof(double) * (size_t)n, (size_t)n, hipMemcpyDeviceToDevice);
      if (e == hipSuccess)
        e = hipMemcpy(slabI + p * stride_I, f->invd, sizeof(double) * (size_t)nblk * IMG_DOUBLES, hipMemcpyDeviceToDevice);
      if (e == hipSuccess && L_out)
        e = hipMemcpy2D(L_out + (size_t)p * (size_t)n * (size_t)n, sizeof(double) * (size_t)n, f->A, sizeof(double) * (size_t)f->lda,
                        sizeof(double) * (size_t)n, (size_t)n, hipMemcpyDeviceToHost);
      agp_fit_destroy(f);
      if (e != hipSuccess) { cleanup(); ctx->last_error = hipGetErrorString(e); return AGP_ERR_HIP; }
    }
    A = slabA; invd = slabI;
  }
  if (zero_strides) stride_A = stride_I = 0;

  // ---- the right-hand side and the scratch of the kind
  const size_t bbytes = sizeof(double) * (size_t)b_doubles;
  double *dB = nullptr, *dX = nullptr, *dW = nullptr, *xstage = nullptr;
  int *dflags = nullptr;
  unsigned long long *done = nullptr;
  auto cleanup_rhs = [&]() {
    for (void *q : {(void *)dB, (void *)dX, (void *)dW, (void *)xstage, (void *)dflags, (void *)done})
      if (q) (void)hipFree(q);
    cleanup();
  };
#define SUB_CHECK(expr)                                                                              \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) { ctx->last_error = hipGetErrorString(_e); cleanup_rhs(); return AGP_ERR_HIP; } \
  } while (0)
  SUB_CHECK(hipMalloc(&dB, bbytes));
  SUB_CHECK(hipMemcpy(dB, B, bbytes, hipMemcpyHostToDevice));
  if (kind == SUB_FWD_VEC || kind == SUB_BWD_VEC) {
    SUB_CHECK(hipMalloc(&dW, sizeof(double) * (size_t)nblk * NB * NB));
    SUB_CHECK(hipMalloc(&xstage, sizeof(double) * (size_t)n));
  }
  if (coop) {
    // x: the caller's buffer once more (its padding and gaps are what comes back around the solution), the sentinel in the
    // n words of every problem (the product fills count * stride words, its stride being n rounded up to 2)
    SUB_CHECK(hipMalloc(&dX, bbytes));
    SUB_CHECK(hipMemcpyAsync(dX, dB, bbytes, hipMemcpyDeviceToDevice, s));
    SUB_CHECK(hipMalloc(&dflags, sizeof(int) * 4 * (size_t)count));
    SUB_CHECK(hipMemsetAsync(dflags, 0, sizeof(int) * 4 * (size_t)count, s));
    if (kind == SUB_COOP_FLAGS) {
      SUB_CHECK(hipMalloc(&done, sizeof(unsigned long long) * (size_t)backsub_done_words(n, 1)));
      PrepArgs pre;
      pre.fill(done, 0ull, backsub_done_words(n, 1));
      launch_prep(s, pre);
    } else {
      for (int64_t p = 0; p < count; ++p) launch_fill_sentinel(s, dX + p * stride_B, n);
    }
  }
  const bool lower = opt != 0;
  switch (kind) {
  case SUB_FWD_MAT: forward_solve_mat(s, A, n, ldA, invd, dB, cols, ldb, lower); break;
  case SUB_FWD_MAT_LOOKAHEAD:
    flags_out[1] = (n > 2 * NBO && ctx->stream2 && cols >= 64) ? 1 : 0;
    forward_solve_mat_lookahead(ctx, A, n, ldA, invd, dB, cols, ldb, lower);
    break;
  case SUB_FWD_MAT_BATCHED:
    forward_solve_mat_batched(s, A, stride_A, n, ldA, invd, stride_I, dB, stride_B, cols, ldb, lower, count);
    break;
  case SUB_BWD_MAT: backward_solve_mat(s, A, n, ldA, invd, dB, cols, ldb); break;
  case SUB_RIGHT_LT: right_solve_lt(s, A, n, ldA, invd, dB, rows, ldb); break;
  case SUB_RIGHT_LT_BATCHED: right_solve_lt_batched(s, A, stride_A, n, ldA, invd, stride_I, dB, stride_B, rows, ldb, count); break;
  case SUB_FWD_VEC:
    invert_diag_blocks_forward(s, n, invd, dW);
    forward_solve_vec(s, A, n, ldA, dW, dB, xstage);
    break;
  case SUB_BWD_VEC:
    invert_diag_blocks(s, A, n, ldA, invd, dW);
    backward_solve_vec(s, A, n, ldA, dW, dB, xstage);
    break;
  case SUB_BWD_VEC_BATCHED: backward_solve_vec_batched(s, A, stride_A, n, ldA, invd, stride_I, dB, stride_B, count); break;
  case SUB_COOP_DIRECT: backward_solve_coop(s, A, n, ldA, invd, dB, dX, dflags, nullptr, 1, 0, 0, 0, 0, 0); break;
  case SUB_COOP_FLAGS: backward_solve_coop(s, A, n, ldA, invd, dB, dX, dflags, done, 1, 0, 0, 0, 0, 0); break;
  case SUB_COOP_BATCHED:
    backward_solve_coop(s, A, n, ldA, invd, dB, dX, dflags, nullptr, count, stride_A, stride_I, stride_B, stride_B, 4);
    break;
  default:  // SUB_BACK_UPDATE: z[c] -= sum_r L[k0 + r][c] x[r], c < k0
    launch_back_update(s, A, ldA, k0, (int)nbk0, k0, dB + ldb, dB);
    break;
  }
  SUB_CHECK(hipStreamSynchronize(s));
  SUB_CHECK(hipGetLastError());
  SUB_CHECK(hipMemcpy(B, coop ? dX : dB, bbytes, hipMemcpyDeviceToHost));
  if (W_out && dW) SUB_CHECK(hipMemcpy(W_out, dW, sizeof(double) * (size_t)nblk * NB * NB, hipMemcpyDeviceToHost));
  if (coop) {
    std::vector<int> hf(4 * (size_t)count);
    SUB_CHECK(hipMemcpy(hf.data(), dflags, sizeof(int) * 4 * (size_t)count, hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < count; ++p) flags_out[2 * p] = hf[4 * (size_t)p + 2];
  }
#undef SUB_CHECK
  cleanup_rhs();
  return AGP_OK;
}

// In-place LL^T of the lower triangle of a host matrix; y (optional) -> L^-1 y.
AGP_DEBUG_API int agp_debug_factor(agp_context *ctx, double *A, int64_t n, int64_t lda, double *y, double *log_det,
                     int64_t *bad_pivot) {
  if (!ctx || !A || n <= 0 || lda < n) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t ab = sizeof(double) * (size_t)lda * (size_t)n;
  const long long nblk = (n + NB - 1) / NB;
  double *dA = nullptr, *dI = nullptr, *dy = nullptr;
  AGP_HIP_CHECK(ctx, hipMalloc(&dA, ab));
  AGP_HIP_CHECK(ctx, hipMalloc(&dI, sizeof(double) * (size_t)nblk * (36 * MB * MB)));
  AGP_HIP_CHECK(ctx, hipMemcpy(dA, A, ab, hipMemcpyHostToDevice));
  if (y) {
    AGP_HIP_CHECK(ctx, hipMalloc(&dy, sizeof(double) * (size_t)n));
    AGP_HIP_CHECK(ctx, hipMemcpy(dy, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  }
  AGP_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), ctx->stream));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_scalars, 0, 4 * sizeof(double), ctx->stream));
  factor_lower(ctx, dA, n, lda, dI, dy);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(A, dA, ab, hipMemcpyDeviceToHost));
  if (y) AGP_HIP_CHECK(ctx, hipMemcpy(y, dy, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  int flags[4];
  double scal[4];
  AGP_HIP_CHECK(ctx, hipMemcpy(flags, ctx->d_flags, sizeof(flags), hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(scal, ctx->d_scalars, sizeof(scal), hipMemcpyDeviceToHost));
  if (log_det) *log_det = 2. * scal[0];
  if (bad_pivot) *bad_pivot = flags[1] ? flags[1] - 1 : -1;
  (void)hipFree(dA); (void)hipFree(dI);
  if (dy) (void)hipFree(dy);
  ctx->sched.backsub = agp_context::ScheduleRecord::BS_NONE;
  ctx->sched.bs_done = 0;
  ctx->sched.handover_timeout = flags[2];
  return AGP_OK;
}

// The schedule record of the context (common.h: agp_context::ScheduleRecord): what its last factorisation - through
// agp_debug_factor or a fit of the product library on the same context - and its last fit ran.  Layout of `out` (int64):
//   [0]  n of the last factorisation          [1]  outer steps recorded      [2]  outer steps beyond the record
//   [3]  panel step launches (panel_fused_kernel<true>)   [4]  fused panel launches (<false>)   [5]  POTRF + TRSM panels
//   [6]  back substitution of the last fit: 0 none (agp_debug_factor), 1 one launch with the output as hand-over,
//        2 one launch with per-block flags, 3 512-wide inverted blocks, 4 the 128-row chain
//   [7]  wide inverses computed under the factorisation (bs_done)
//   [8]  when: 1 early (all-step factorisation), 2 at the last outer step, 4 under the step tail
//   [9]  hand-over time-out flag (flags[2]) after the factorisation or fit   [10] demotions of this context
//   [11] workgroup slots of the step kernel (0: not asked yet)   [12] CUs   [13] 1 if the CU-masked bulk stream exists
//   [14..18] switches in force: AGP_STEP_BELOW, AGP_PANEL_FUSED, AGP_MERGE_ABOVE, AGP_BACKSUB_COOP, AGP_FP64_NBO
//   [19] reserved (0)
//   [20 + 2 i], [21 + 2 i]: last column + 1 and bits of outer step i (1 merged bulk launch, 2 step launches, 4 host-throttled
//        bulk update, 8 bulk update on the CU-masked stream, 16 single-stream end)
// At most `cap` words are written; the full record is 20 + 2 * HEADCNT_WORDS.
constexpr int64_t SCHED_HEADER = 20;
AGP_DEBUG_API int agp_debug_schedule(agp_context *ctx, int64_t *out, int64_t cap) {
  if (!ctx || !out || cap < 0) return AGP_ERR_INVALID_ARGUMENT;
  const agp_context::ScheduleRecord &r = ctx->sched;
  int64_t w[SCHED_HEADER + 2 * agp_context::HEADCNT_WORDS] = {};
  w[0] = r.n; w[1] = r.steps; w[2] = r.steps_dropped;
  w[3] = r.panels_step; w[4] = r.panels_fused; w[5] = r.panels_split;
  w[6] = r.backsub; w[7] = r.bs_done; w[8] = r.inv_bits; w[9] = r.handover_timeout; w[10] = r.demotions;
  w[11] = ctx->step_slots; w[12] = ctx->cus; w[13] = ctx->stream_masked ? 1 : 0;
  w[14] = ctx->tune.step_below; w[15] = ctx->tune.panel_fused ? 1 : 0; w[16] = ctx->tune.merge_above;
  w[17] = ctx->tune.backsub_coop ? 1 : 0; w[18] = ctx->tune.fp64_nbo;
  for (long long i = 0; i < r.steps; ++i) {
    w[SCHED_HEADER + 2 * i] = r.kend[i];
    w[SCHED_HEADER + 2 * i + 1] = r.bits[i];
  }
  const int64_t total = SCHED_HEADER + 2 * agp_context::HEADCNT_WORDS;
  for (int64_t i = 0; i < cap && i < total; ++i) out[i] = w[i];
  return AGP_OK;
}

// The schedule factor_lower WOULD run for n rows under the given switches (factor_plan.h) - no context, no device.
// switches (int64, the fields of FactorSwitches in order): panel_fused, step_below, merge_above, nbo_override, nbo_wide,
// products, step_slots, cus, have_masked_stream, headcnt_ready, step_buffers_ready, fused_buffers_ready, inv_requested,
// bs_BW, bs_done.  `out` has the layout of agp_debug_schedule - [0] n, [1] steps, [2] steps beyond the record, [3..5] the
// panel launches, [7] bs_done and [8] the inversion bits if every host-side wait succeeds, [20 + 2 i] end and bits of
// step i - followed, from word 20 + 2 * 256 on, by five words per step: the inversion intents of OuterStep
// (inv_last_step, inv_first, inv_count, mark_after, inv_bit).  At most `cap` words are written.
constexpr int64_t PLAN_WORDS = SCHED_HEADER + 7 * agp_context::HEADCNT_WORDS;
AGP_DEBUG_API int agp_debug_factor_plan(const int64_t *switches, int64_t n, int64_t *out, int64_t cap) {
  if (!switches || !out || n < 1 || cap < 0) return AGP_ERR_INVALID_ARGUMENT;
  agp::FactorSwitches sw;
  sw.panel_fused = switches[0] != 0; sw.step_below = switches[1]; sw.merge_above = switches[2];
  sw.nbo_override = switches[3]; sw.nbo_wide = switches[4]; sw.products = (agp::BulkProducts)switches[5];
  sw.step_slots = switches[6]; sw.cus = switches[7];
  sw.have_masked_stream = switches[8] != 0; sw.headcnt_ready = switches[9] != 0;
  sw.step_buffers_ready = switches[10] != 0; sw.fused_buffers_ready = switches[11] != 0;
  sw.inv_requested = switches[12] != 0; sw.bs_BW = switches[13]; sw.bs_done = switches[14];
  int64_t w[PLAN_WORDS] = {};
  int64_t *steps = w + SCHED_HEADER, *intents = steps + 2 * agp_context::HEADCNT_WORDS;
  agp::FactorPlanner plan(n, sw);
  agp::OuterStep s;
  w[0] = n;
  while (plan.next(s)) {
    const int64_t blocks = (s.next_end - s.kend + agp::NB - 1) / agp::NB;
    const agp::PanelPlan pp = agp::plan_panels(n, s.kend, s.next_end, s.step_mode, sw);
    // (panel_phase: a step block's first panel is a plain fused launch)
    if (!pp.fused) w[5] += blocks;
    else if (!pp.step_mode) w[4] += blocks;
    else { w[4] += 1; w[3] += blocks - 1; }
    w[8] |= (s.inv_last_step > 0 ? agp::INV_BIT_LAST_STEP : 0u) | (s.inv_count > 0 ? s.inv_bit : 0u);
    plan.inversion_under_panels(s, s.inv_count > 0);
    if (w[1] >= agp_context::HEADCNT_WORDS) { ++w[2]; continue; }
    const int64_t i = w[1]++;
    steps[2 * i] = s.next_end; steps[2 * i + 1] = s.bits;
    const int64_t intent[5] = {s.inv_last_step, s.inv_first, s.inv_count, s.mark_after, s.inv_bit};
    std::copy(intent, intent + 5, intents + 5 * i);
  }
  w[7] = plan.bs_done();
  std::copy(w, w + std::min(cap, PLAN_WORDS), out);
  return AGP_OK;
}

// The pooled plan agp_logo_nll_gradient_batch WOULD run for `count` problems of n[b] rows with the given groups
// (logo_batch_plan.h) - no context, no device.  cols_max <= 0: the entry's own bound, count * max n.  Returns
// AGP_ERR_INVALID_ARGUMENT where the entry would.  *words receives the length of the record, of which at most `cap` words
// are written to `out`:
//   [0] terms T, [1] chunks K, [2] cols_max in force, [3] the group limit, [4] the image limit (doubles), [5] reserved
//   K x 4: m, count, term_off, image doubles of one group       T x 3: problem, group (the caller's number), size
//   per chunk count * m padded indices (-1 = padding)            count + 1 words csr_off, T words csr_terms
AGP_DEBUG_API int agp_debug_logo_batch_plan(int64_t count, const int64_t *n, const int64_t *n_groups, const int64_t *const *offsets,
                                            const int64_t *const *indices, int64_t cols_max, int64_t *out, int64_t cap, int64_t *words) {
  if (count <= 0 || !n || !n_groups || !words || cap < 0 || (cap > 0 && !out)) return AGP_ERR_INVALID_ARGUMENT;
  std::vector<long long> nb((size_t)count);
  long long n_max = 0;
  for (int64_t b = 0; b < count; ++b) {
    nb[(size_t)b] = n[b];
    n_max = std::max(n_max, nb[(size_t)b]);
  }
  if (cols_max <= 0) cols_max = count * n_max;
  const agp::LogoBatchLimits lim{logo_chunk_groups_max(), logo_chunk_img_elems_max(), cols_max, factor_ld, logo_img_stride};
  agp::LogoBatchPlan p;
  if (!agp::logo_batch_plan(count, nb.data(), n_groups, offsets, indices, lim, p)) return AGP_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> w{p.terms, (int64_t)p.chunks.size(), cols_max, lim.groups_max, lim.img_elems_max, 0};
  for (const agp::LogoBatchChunk &ch : p.chunks) w.insert(w.end(), {ch.m, ch.count, ch.term_off, logo_img_stride(ch.m)});
  for (long long q = 0; q < p.terms; ++q) w.insert(w.end(), {p.problem[(size_t)q], p.group[(size_t)q], p.size[(size_t)q]});
  for (const agp::LogoBatchChunk &ch : p.chunks) w.insert(w.end(), p.meta.begin() + ch.idx_off, p.meta.begin() + ch.idx_off + ch.count * ch.m);
  w.insert(w.end(), p.meta.begin() + p.csr_at, p.meta.end());
  *words = (int64_t)w.size();
  std::copy(w.begin(), w.begin() + std::min<int64_t>(cap, (int64_t)w.size()), out);
  return AGP_OK;
}

// step_launch_shape (factor_plan.h) for `below` rows under the panels_done-th panel of its block: out[0..6] = grid,
// trail_first, trail_tiles, trail_workers, hold_index, hold_count, rowcnt_expect.
AGP_DEBUG_API int agp_debug_step_launch_shape(int64_t below, int64_t panels_done, int64_t step_slots, int64_t cus, int64_t *out) {
  if (!out || below < 0) return AGP_ERR_INVALID_ARGUMENT;
  const agp::StepLaunchShape sh = agp::step_launch_shape(below, panels_done, step_slots, cus);
  const int64_t w[7] = {sh.grid, sh.trail_first, sh.trail_tiles, sh.trail_workers, sh.hold_index, sh.hold_count, (int64_t)sh.rowcnt_expect};
  std::copy(w, w + 7, out);
  return AGP_OK;
}

// The tiling an update launch WOULD get (update_plan.h) - no context, no device.  in[0] says what is asked:
//   0  bulk update: in = {0, nth, head_cols, slots} (nth: tile rows of the whole trailing matrix) ->
//      {ntr, tiles, full, rem, kernel (0 trailing_update_kernel, 1 trailing_update_tail_kernel), head_count, order_len, grid}
//      as launch_trailing_update_merged (head_cols > 0) / launch_trailing_update_as (Fp64) fill them; order_len: length of
//      the order table of the whole tiles, 0 without one
//   1  plan_nt_sub: in = {1, M, N, K, tri, a_kmajor, b_kmajor, count, small_limit} -> {edge, transposed, ntr, ntc, grid}
//   2  plan_stair: in = {2, M, N, block, c0, slots} -> {edge, ntr, ntc, st_tpb, st_c0t}
//   3  lower_tile_of: in = {3, first id, ids, ntr, ntc, tri} -> per id {found, bi, bj}
//   4  xcd_tile_order: in = {4, ntr, full} -> the table
// *words receives the length of the answer, of which at most `cap` words are written to `out`.
AGP_DEBUG_API int agp_debug_update_plan(const int64_t *in, int64_t n_in, int64_t *out, int64_t cap, int64_t *words) {
  static const int64_t need[5] = {4, 9, 6, 6, 3};
  if (!in || !words || n_in < 1 || cap < 0 || (cap > 0 && !out) || in[0] < 0 || in[0] > 4 || n_in < need[in[0]]) return AGP_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> w;
  if (in[0] == 0) {
    const int nth = (int)in[1], head_cols = (int)std::min(in[2], in[1]), ntr = nth - head_cols;
    if (nth < 1 || head_cols < 0 || in[3] < 1) return AGP_ERR_INVALID_ARGUMENT;
    const long long tiles = agp::lower_tile_count(ntr, ntr, 1), head_count = agp::lower_tile_count(nth, head_cols, 1);
    const agp::BulkSplit sp = agp::plan_bulk_update(tiles, in[3], head_cols > 0);
    const bool tail = sp.kernel == agp::SplitKernel::QuadrantsOnly;
    const long long order_len = !tail && sp.full > 0 ? (long long)agp::xcd_tile_order(ntr, sp.full).size() : 0;
    w = {ntr, tiles, sp.full, sp.rem, tail ? 1 : 0, head_count, order_len, agp::bulk_grid(sp, head_count, order_len)};
  } else if (in[0] == 1) {
    if (in[1] < 1 || in[2] < 1 || in[3] < 1 || in[7] < 1) return AGP_ERR_INVALID_ARGUMENT;
    const agp::NtSubPlan p = agp::plan_nt_sub(in[1], in[2], in[3], in[4] != 0, in[5] != 0, in[6] != 0, in[7], in[8]);
    w = {p.edge, p.transposed ? 1 : 0, p.ntr, p.ntc, p.grid};
  } else if (in[0] == 2) {
    if (in[1] < 1 || in[2] < 1 || in[3] < 1 || in[4] < 0 || in[5] < 1) return AGP_ERR_INVALID_ARGUMENT;
    const agp::StairPlan p = agp::plan_stair(in[1], in[2], in[3], in[4], in[5]);
    w = {p.edge, p.ntr, p.ntc, p.st_tpb, p.st_c0t};
  } else if (in[0] == 3) {
    if (in[1] < 0 || in[2] < 0 || in[3] < 1 || in[4] < 1) return AGP_ERR_INVALID_ARGUMENT;
    for (int64_t id = in[1]; id < in[1] + in[2]; ++id) {
      int bi = -1, bj = -1;
      const bool found = agp::lower_tile_of(id, (int)in[3], (int)in[4], in[5] != 0, bi, bj);
      w.insert(w.end(), {found ? 1 : 0, found ? bi : -1, found ? bj : -1});
    }
  } else {
    if (in[1] < 1 || in[2] < 0) return AGP_ERR_INVALID_ARGUMENT;
    const std::vector<int> table = agp::xcd_tile_order((int)in[1], in[2]);
    w.assign(table.begin(), table.end());
  }
  *words = (int64_t)w.size();
  std::copy(w.begin(), w.begin() + std::min<int64_t>(cap, (int64_t)w.size()), out);
  return AGP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Test / measurement instrumentation that used to sit in the product library's ABI
// ---------------------------------------------------------------------------------------------------------------
namespace agp {
// ---- bare MFMA issue loop: measured fp64 matrix peak of this device ----------
__global__ __launch_bounds__(256) void mfma_peak_kernel(double *sink, int iters, double a0, double b0) {
  v4d acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = v4zero();
  double a = a0 + threadIdx.x * 1e-9, b = b0 - threadIdx.x * 1e-9;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = mfma16(a, b, acc[i]);
  }
  double s = 0.;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  if (s == 123.456) sink[0] = s;  // keep the loop live
}

static int mfma_f64_peak(hipStream_t s, int iters, double *tflops) {
  double *sink = nullptr;
  if (hipMalloc(&sink, 8) != hipSuccess) return AGP_ERR_HIP;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  const int blocks = 256 * 2;  // 2 workgroups of 4 waves per CU: 2 waves per SIMD
  hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, s, sink, 16, 1.0, 2.0);
  (void)hipEventRecord(e0, s);
  hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, s, sink, iters, 1.0, 2.0);
  (void)hipEventRecord(e1, s);
  hipError_t e = hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double flop = (double)blocks * 4.0 * (double)iters * 8.0 * 2.0 * 16 * 16 * 4;
  *tflops = flop / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(sink);
  return e == hipSuccess ? AGP_OK : AGP_ERR_HIP;
}

// A transport that moves nothing: times ONE rank's share of a G-rank sharded fit on a box with one GPU - same kernels,
// same shapes, same launch chain; the peers' data is whatever the buffers hold, so the numerical result is
// meaningless (scripts/time_sharded_rank.py).
struct NullComm : HostReducingComm {
  int broadcast(ShardOps &, int, double *, long long, int) override { return AGP_OK; }
  int all_gather(ShardOps &, int, const double *, double *, long long) override { return AGP_OK; }
  int all_reduce(ShardOps &, int, double *, long long, int) override { return AGP_OK; }
  int all_reduce_host(double *, long long, int) override { return AGP_OK; }
};
}  // namespace agp

namespace {
// a device buffer of the Gram entry points below (agp_debug_gram, ...): freed on every return, the early ones of AGP_HIP_CHECK included
template <class T>
struct DevBuf {
  T *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc(&p, sizeof(T) * count); }
};
// This library image has its own copy of the AGP_GRAM_SOP switch the Gram launchers follow (api.hip: g_gram_sop), which a
// context made by the product library never sets: for the length of one entry point the switch is the one of the context
// handed in, then what it was.  EVERY debug entry point that launches a covariance kernel holds one of these.
struct GramSopScope {
  bool before;
  explicit GramSopScope(const agp_context *ctx) : before(gram_sop_enabled()) { gram_sop_set(ctx->tune.gram_sop); }
  GramSopScope(const GramSopScope &) = delete;
  GramSopScope &operator=(const GramSopScope &) = delete;
  ~GramSopScope() { gram_sop_set(before); }
};
}  // namespace

extern "C" {

// the cycle stamps the factoring workgroup of the LAST potrf / panel launch left (a -DAGP_POTRF_TIMING build; zeros otherwise)
AGP_DEBUG_API int agp_debug_potrf_probe(agp_context *ctx, unsigned long long *out) {
  if (!ctx || !out) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  read_potrf_probe(out);
  return AGP_OK;
}

// cycles and 100 MHz ticks of one tile of the LAST fp64 bulk launch (a -DAGP_BULK_STAMPS build; zeros otherwise)
AGP_DEBUG_API int agp_debug_bulk_probe(agp_context *ctx, unsigned long long *out) {
  if (!ctx || !out) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  read_bulk_probe(out);
  return AGP_OK;
}

// the phase cycle sums one workgroup of the LAST bf16 x 3 bulk launch left (a -DAGP_BF16_STAMPS build; zeros otherwise)
AGP_DEBUG_API int agp_debug_bf16_probe(agp_context *ctx, unsigned long long *out) {
  if (!ctx || !out) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  read_bf16_probe(out);
  return AGP_OK;
}

AGP_DEBUG_API int agp_debug_mfma_f64_peak(agp_context *ctx, int iters, double *tflops) {
  if (!ctx || !tflops || iters <= 0) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return mfma_f64_peak(ctx->stream, iters, tflops);
}

// ---- the covariance kernels of gram.hip / gram_fast.h one launch at a time (tests/test_gram_paths_gpu.py) ----------------------
// launch_gram on host data.  out_host: the caller's WHOLE buffer of out_offset_elems + ld * cols doubles (cols = y ? y->n :
// x->n), padding rows and the elements before the matrix included: uploaded, the launch writes at d_out + out_offset_elems
// with leading dimension ld, downloaded - what the kernel did not store comes back bit for bit.  (An odd offset leaves the
// output 8-byte aligned only: the kernels' scalar store pair.)  y = nullptr: Y is the very view of X, as the fits pass it.
// diag_add (optional): cols values.  nan_flag: the flag the kernel raised; path: the GramPath that gram_select_path chose
// for exactly these views (the launcher switches on the same call).
AGP_DEBUG_API int agp_debug_gram(agp_context *ctx, const agp_kernel *k, const agp_features *x, const agp_features *y, int symmetric,
                                 int lower_only, int64_t ld, int64_t out_offset_elems, const double *diag_add, double *out_host,
                                 int *nan_flag, int *path) {
  if (!ctx || !k || !x || !out_host || !nan_flag || !path || out_offset_elems < 0) return AGP_ERR_INVALID_ARGUMENT;
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  if (y && (st = validate_features(y)) != AGP_OK) return st;
  if (y && (y->dim != x->dim || symmetric)) return AGP_ERR_INVALID_ARGUMENT;
  const long long rows = x->n, cols = y ? y->n : x->n;
  if (rows <= 0 || cols <= 0 || ld < rows) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx, dy;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  if (y && (st = to_device(ctx, y, false, &dy)) != AGP_OK) return st;
  const FeatView &vy = y ? dy.v : dx.v;
  const size_t total = (size_t)out_offset_elems + (size_t)ld * (size_t)cols;
  DevBuf<double> d_out, d_diag;
  DevBuf<int> d_flag;
  AGP_HIP_CHECK(ctx, d_out.alloc(total));
  AGP_HIP_CHECK(ctx, d_flag.alloc(1));
  AGP_HIP_CHECK(ctx, hipMemcpy(d_out.p, out_host, sizeof(double) * total, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemset(d_flag.p, 0, sizeof(int)));
  if (diag_add) {
    AGP_HIP_CHECK(ctx, d_diag.alloc((size_t)cols));
    AGP_HIP_CHECK(ctx, hipMemcpy(d_diag.p, diag_add, sizeof(double) * (size_t)cols, hipMemcpyHostToDevice));
  }
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());  // (the null-stream copies above do not order with the context's stream)
  GramSopScope sop_switch(ctx);
  *path = (int)gram_select_path(&k->prog, dx.v, vy, lower_only != 0);
  launch_gram(ctx->stream, dprog, dx.v, vy, symmetric != 0, lower_only != 0, d_out.p + out_offset_elems, ld, d_diag.p, d_flag.p,
              &k->prog);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(out_host, d_out.p, sizeof(double) * total, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(nan_flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost));
  return AGP_OK;
}

// launch_gram_blocks on host data: `count` diagonal blocks of `rows` consecutive features of x each, block g at
// out + g * stride with leading dimension ld.  out_host: the caller's whole buffer of (count - 1) * stride + ld * rows doubles,
// uploaded and downloaded as above.  diag_add (optional): rows * count values.  launched: 0 when the tree has none of the
// fast shapes (nothing ran, the buffer comes back as it went in).
AGP_DEBUG_API int agp_debug_gram_blocks(agp_context *ctx, const agp_kernel *k, const agp_features *x, int64_t rows, int64_t count,
                                        int64_t ld, int64_t stride, const double *diag_add, double *out_host, int *launched) {
  if (!ctx || !k || !x || !out_host || !launched || rows <= 0 || count <= 0 || ld < rows || stride < 0) return AGP_ERR_INVALID_ARGUMENT;
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  if (x->n < rows * count) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  const size_t total = (size_t)(count - 1) * (size_t)stride + (size_t)ld * (size_t)rows;
  DevBuf<double> d_out, d_diag;
  AGP_HIP_CHECK(ctx, d_out.alloc(total));
  AGP_HIP_CHECK(ctx, hipMemcpy(d_out.p, out_host, sizeof(double) * total, hipMemcpyHostToDevice));
  if (diag_add) {
    AGP_HIP_CHECK(ctx, d_diag.alloc((size_t)(rows * count)));
    AGP_HIP_CHECK(ctx, hipMemcpy(d_diag.p, diag_add, sizeof(double) * (size_t)(rows * count), hipMemcpyHostToDevice));
  }
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  GramSopScope sop_switch(ctx);
  *launched = launch_gram_blocks(ctx->stream, &k->prog, dx.v, rows, count, d_out.p, ld, stride, d_diag.p, nullptr) ? 1 : 0;
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(out_host, d_out.p, sizeof(double) * total, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// launch_predict_mean with the caller's alpha (x->n values): no fit and no factorisation between the kernel and the check.
// mean_host: xs->n + 2 doubles, uploaded first and downloaded whole, so that the two trailing ones show a store past the
// last test point.  path: the PredictMeanPath that predict_mean_select_path chose for exactly these views.
AGP_DEBUG_API int agp_debug_predict_mean(agp_context *ctx, const agp_kernel *k, const agp_features *x, const agp_features *xs,
                                         const double *alpha_host, double *mean_host, int *path) {
  if (!ctx || !k || !x || !xs || !alpha_host || !mean_host || !path) return AGP_ERR_INVALID_ARGUMENT;
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  if ((st = validate_features(xs)) != AGP_OK) return st;
  if (x->dim != xs->dim || x->n <= 0 || xs->n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx, dxs;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  if ((st = to_device(ctx, xs, false, &dxs)) != AGP_OK) return st;
  const size_t n = (size_t)x->n, m = (size_t)xs->n;
  DevBuf<double> d;  // alpha (n), then mean (m + 2)
  AGP_HIP_CHECK(ctx, d.alloc(n + m + 2));
  AGP_HIP_CHECK(ctx, hipMemcpy(d.p, alpha_host, sizeof(double) * n, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(d.p + n, mean_host, sizeof(double) * (m + 2), hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  GramSopScope sop_switch(ctx);
  *path = (int)predict_mean_select_path(&k->prog, dx.v, dxs.v);
  launch_predict_mean(ctx->stream, dprog, dx.v, dxs.v, d.p, d.p + n, &k->prog);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(mean_host, d.p + n, sizeof(double) * (m + 2), hipMemcpyDeviceToHost));
  return AGP_OK;
}

// What agp_gram_matvec runs for these features (gram_matvec.hip: the launcher switches on the same gram_matvec_plan call):
// plan[0] the evaluator (0 radial fast path, 1 sum of products, 2 interpreter), plan[1] the column slices S, plan[2] the
// columns of a slice, plan[3] the rows of a workgroup, plan[4] the columns of an LDS tile, plan[5] the right-hand sides of
// the first chunk's kernel for `nrhs` of them (1, 4 or 16).  Launches nothing (tests/test_gram_matvec_gpu.py).
AGP_DEBUG_API int agp_debug_gram_matvec_plan(agp_context *ctx, const agp_kernel *k, const agp_features *x, int64_t nrhs, int64_t *plan) {
  if (!ctx || !k || !x || !plan || nrhs < 1) return AGP_ERR_INVALID_ARGUMENT;
  const int st = validate_features(x);
  if (st != AGP_OK) return st;
  GramSopScope sop_switch(ctx);
  FeatView v{};
  v.n = x->n; v.dim = x->dim; v.nsc = x->n_scale_columns; v.meas = x->is_measurement;
  const MvPlan p = gram_matvec_plan(&k->prog, v);
  plan[0] = p.path; plan[1] = p.slices; plan[2] = p.cols_per_slice;
  plan[3] = MV_ROWS; plan[4] = MV_COLS; plan[5] = gram_matvec_chunk_width(nrhs);
  return AGP_OK;
}

// the tiling launch_gram_tangent_forms runs for n rows (gram_tangent.h; no device): plan = [row blocks, units (pairs of row
// blocks), slices, tiles per slice, the longest tile list of a unit, TF_ROWS, TF_COLS, TF_MAX_PAIRS, GRAD_GROUP, the width
// of the first chunk of ncols column pairs]
AGP_DEBUG_API int agp_debug_gram_tangent_plan(int64_t n, int64_t ncols, int64_t *plan) {
  if (!plan || n < 1 || ncols < 1) return AGP_ERR_INVALID_ARGUMENT;
  const TfPlan p = gram_tangent_plan(n);
  plan[0] = p.row_blocks; plan[1] = p.units; plan[2] = p.slices; plan[3] = p.tiles_per_slice; plan[4] = p.max_tiles;
  plan[5] = TF_ROWS; plan[6] = TF_COLS; plan[7] = TF_MAX_PAIRS; plan[8] = GRAD_GROUP; plan[9] = gram_tangent_chunk_width(ncols);
  return AGP_OK;
}

// ---- the column-pivoted QR of qr.hip and the substitutions against its R, one building block at a time (tests/test_qr_gpu.py) ----
// Every entry point takes the caller's WHOLE padded host buffers, uploads them, runs on ctx->stream and downloads them whole:
// what the kernels did not store comes back bit for bit.  A permutation that is not one of 0 .. m - 1 is refused before
// anything is launched (the kernels index with it).
static bool qr_perm_valid(const int64_t *perm, int64_t m) {
  std::vector<char> seen((size_t)m, 0);
  for (int64_t i = 0; i < m; ++i) {
    if (perm[i] < 0 || perm[i] >= m || seen[(size_t)perm[i]]) return false;
    seen[(size_t)perm[i]] = 1;
  }
  return true;
}

// colpiv_qr: A (lda x alloc_cols; the rows x (cols + extra) part is factored in place), tau (cols), perm (cols), state (4:
// threshold helper, max |pivot|, nonzero_pivots, rank).  rows < cols is refused: the product never factors a wide matrix
// (sparse_api.hip: sparse_pivoted_from_rows has rows >= m) and qr_extract_r reads m rows of it.
AGP_DEBUG_API int agp_debug_colpiv_qr(agp_context *ctx, double *A, int64_t lda, int64_t rows, int64_t cols, int64_t extra,
                                      int64_t alloc_cols, double *tau, int64_t *perm, double *state) {
  if (!ctx || !A || !tau || !perm || !state || rows <= 0 || cols <= 0 || extra < 0 || rows < cols || lda < rows ||
      alloc_cols < cols + extra)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t na = (size_t)lda * (size_t)alloc_cols, nc = (size_t)cols;
  DevBuf<double> dA, aux;  // aux: tau | norms | state
  DevBuf<long long> dperm;
  AGP_HIP_CHECK(ctx, dA.alloc(na));
  AGP_HIP_CHECK(ctx, aux.alloc(2 * nc + 4));
  AGP_HIP_CHECK(ctx, dperm.alloc(nc));
  AGP_HIP_CHECK(ctx, hipMemcpy(dA.p, A, sizeof(double) * na, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemset(aux.p, 0xFF, sizeof(double) * (2 * nc + 4)));  // (all ones: a NaN)
  AGP_HIP_CHECK(ctx, hipMemset(dperm.p, 0xFF, sizeof(long long) * nc));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());  // (the null-stream copies above do not order with the context's stream)
  colpiv_qr(ctx->stream, dA.p, lda, rows, cols, extra, aux.p, dperm.p, aux.p + nc, aux.p + 2 * nc);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  static_assert(sizeof(long long) == sizeof(int64_t), "perm is copied as it is");
  AGP_HIP_CHECK(ctx, hipMemcpy(A, dA.p, sizeof(double) * na, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(tau, aux.p, sizeof(double) * nc, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(state, aux.p + 2 * nc, sizeof(double) * 4, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(perm, dperm.p, sizeof(int64_t) * nc, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// qr_extract_r: A (lda x m, read), R (ldr x m, the caller's filling; its first m rows are written)
AGP_DEBUG_API int agp_debug_qr_extract_r(agp_context *ctx, const double *A, int64_t lda, int64_t m, double *R, int64_t ldr,
                                         double inflate) {
  if (!ctx || !A || !R || m <= 0 || lda < m || ldr < m) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t na = (size_t)lda * (size_t)m, nr = (size_t)ldr * (size_t)m;
  DevBuf<double> dA, dR;
  AGP_HIP_CHECK(ctx, dA.alloc(na));
  AGP_HIP_CHECK(ctx, dR.alloc(nr));
  AGP_HIP_CHECK(ctx, hipMemcpy(dA.p, A, sizeof(double) * na, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dR.p, R, sizeof(double) * nr, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  qr_extract_r(ctx->stream, dA.p, lda, m, dR.p, ldr, inflate);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(R, dR.p, sizeof(double) * nr, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// qr_root: R (ldr x m, read), T (ldt x m, the caller's filling; qr_root clears all of it and writes P R^T)
AGP_DEBUG_API int agp_debug_qr_root(agp_context *ctx, const double *R, int64_t ldr, const int64_t *perm, int64_t m, double *T,
                                    int64_t ldt) {
  if (!ctx || !R || !perm || !T || m <= 0 || ldr < m || ldt < m || !qr_perm_valid(perm, m)) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t nr = (size_t)ldr * (size_t)m, nt = (size_t)ldt * (size_t)m;
  DevBuf<double> dR, dT;
  DevBuf<long long> dperm;
  AGP_HIP_CHECK(ctx, dR.alloc(nr));
  AGP_HIP_CHECK(ctx, dT.alloc(nt));
  AGP_HIP_CHECK(ctx, dperm.alloc((size_t)m));
  AGP_HIP_CHECK(ctx, hipMemcpy(dR.p, R, sizeof(double) * nr, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dT.p, T, sizeof(double) * nt, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dperm.p, perm, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  qr_root(ctx->stream, dR.p, ldr, dperm.p, m, dT.p, ldt);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(T, dT.p, sizeof(double) * nt, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// qr_sqrt_solve: W = R^-T P^T X.  X (ldx x alloc_cols, read) and W (ldw x alloc_cols) are the caller's whole buffers; both
// come back, so that the test sees X unchanged and W written in its m x nrhs part only.
AGP_DEBUG_API int agp_debug_qr_sqrt_solve(agp_context *ctx, const double *R, int64_t ldr, const int64_t *perm, int64_t m, double *X,
                                          int64_t ldx, double *W, int64_t ldw, int64_t nrhs, int64_t alloc_cols) {
  if (!ctx || !R || !perm || !X || !W || m <= 0 || nrhs <= 0 || ldr < m || ldx < m || ldw < m || alloc_cols < nrhs ||
      !qr_perm_valid(perm, m))
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t nr = (size_t)ldr * (size_t)m, nx = (size_t)ldx * (size_t)alloc_cols, nw = (size_t)ldw * (size_t)alloc_cols;
  DevBuf<double> dR, dX, dW;
  DevBuf<long long> dperm;
  AGP_HIP_CHECK(ctx, dR.alloc(nr));
  AGP_HIP_CHECK(ctx, dX.alloc(nx));
  AGP_HIP_CHECK(ctx, dW.alloc(nw));
  AGP_HIP_CHECK(ctx, dperm.alloc((size_t)m));
  AGP_HIP_CHECK(ctx, hipMemcpy(dR.p, R, sizeof(double) * nr, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dX.p, X, sizeof(double) * nx, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dW.p, W, sizeof(double) * nw, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dperm.p, perm, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  qr_sqrt_solve(ctx->stream, dR.p, ldr, dperm.p, m, dX.p, ldx, dW.p, ldw, nrhs);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(X, dX.p, sizeof(double) * nx, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(W, dW.p, sizeof(double) * nw, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// qr_back_solve: out = P [R11^-1 c[0 : np]; 0].  c and out are m + 2 doubles each, uploaded and downloaded whole: c comes
// back with its first np entries solved in place, and the two trailing doubles of either show a store past the end.
AGP_DEBUG_API int agp_debug_qr_back_solve(agp_context *ctx, const double *R, int64_t ldr, const int64_t *perm, int64_t m, int64_t np,
                                          double *c, double *out) {
  if (!ctx || !R || !perm || !c || !out || m <= 0 || np < 0 || np > m || ldr < m || !qr_perm_valid(perm, m))
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t nr = (size_t)ldr * (size_t)m, nv = (size_t)m + 2;
  DevBuf<double> dR, dv;  // dv: c (m + 2), then out (m + 2)
  DevBuf<long long> dperm;
  AGP_HIP_CHECK(ctx, dR.alloc(nr));
  AGP_HIP_CHECK(ctx, dv.alloc(2 * nv));
  AGP_HIP_CHECK(ctx, dperm.alloc((size_t)m));
  AGP_HIP_CHECK(ctx, hipMemcpy(dR.p, R, sizeof(double) * nr, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dv.p, c, sizeof(double) * nv, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dv.p + nv, out, sizeof(double) * nv, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(dperm.p, perm, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  qr_back_solve(ctx->stream, dR.p, ldr, dperm.p, m, np, dv.p, dv.p + nv);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(c, dv.p, sizeof(double) * nv, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(out, dv.p + nv, sizeof(double) * nv, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// ONE wide vector sweep of api.hip on host data (tests/test_reduce_kernels_gpu.py): the single-right-hand-side substitutions
// through explicitly inverted BW x BW diagonal blocks, and one application of the mixed fit's preconditioner.
//   kind   WS_FWD_VEC_WIDE / WS_BWD_VEC_WIDE: forward_solve_vec_wide / backward_solve_vec_wide, with the fp32 copy of the
//          factor for the blocks off the diagonal when use_a32;  WS_BWD_VEC_ANY_WIDE: backward_solve_vec_any's wide branch
//          (first_done = 0, no event; BW must be backsolve_width(n));  WS_MIXED_PRECONDITION: mixed_precondition_setup
//          and ONE application, sweep by sweep (always with the fp32 copy)
//   K      the SPD matrix (n x n, ld n), factored by agp_factor_create; n a multiple of BW, BW 512 or 1024
//   z      the caller's whole vector buffer, z_doubles >= n long, padding included: copied in, solved in place (the
//          preconditioner: read from a copy, its output written over the buffer's first n words), copied back
//   t2_out (WS_MIXED_PRECONDITION, z_doubles long) the forward sweep's result (t2 before the backward sweep consumes it),
//          the words behind it all-ones NaN
//   L_out  (optional, n x n, ld n) the factor;  L32_out (optional, n x n FLOATS, ld n) the top n rows of the fp32 copy,
//          all-ones NaN before the conversion.  Only z and t2 come back with their padding: the padding rows of the factor
//          and of its fp32 copy (lda > n) are not returned - RED_CONVERT_LOWER_F32 below checks the whole buffer of the copy
enum { WS_FWD_VEC_WIDE = 0, WS_BWD_VEC_WIDE, WS_BWD_VEC_ANY_WIDE, WS_MIXED_PRECONDITION, WS_KINDS };
AGP_DEBUG_API int agp_debug_wide_sweep(agp_context *ctx, int kind, const double *K, int64_t n, int64_t BW, int use_a32, double *z,
                                       int64_t z_doubles, double *t2_out, double *L_out, float *L32_out) {
  if (!ctx || !K || !z || kind < 0 || kind >= WS_KINDS || (BW != 512 && BW != 1024) || n <= 0 || n > 16384 || n % BW != 0 ||
      z_doubles < n || z_doubles > n + 4096)
    return AGP_ERR_INVALID_ARGUMENT;
  if (kind == WS_BWD_VEC_ANY_WIDE && (use_a32 || BW != backsolve_width(n))) return AGP_ERR_INVALID_ARGUMENT;
  if (kind == WS_MIXED_PRECONDITION && !t2_out) return AGP_ERR_INVALID_ARGUMENT;
  const bool a32 = use_a32 || kind == WS_MIXED_PRECONDITION;
  if (L32_out && !a32) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  struct FitHolder {
    agp_fit *f = nullptr;
    ~FitHolder() { if (f) agp_fit_destroy(f); }
  } fh;
  const int st = agp_factor_create(ctx, K, n, n, 0, AGP_HOST, &fh.f);
  if (st != AGP_OK) return st;
  const agp_fit *f = fh.f;
  const long long lda = f->lda;
  const size_t zbytes = sizeof(double) * (size_t)z_doubles, wide = (size_t)n * (size_t)BW;
  DevBuf<double> dz, din, dt1, dt2, dW, dWT, dws;
  DevBuf<float> dL32;
  AGP_HIP_CHECK(ctx, dz.alloc((size_t)z_doubles));
  AGP_HIP_CHECK(ctx, hipMemcpy(dz.p, z, zbytes, hipMemcpyHostToDevice));
  if (a32) {
    AGP_HIP_CHECK(ctx, dL32.alloc((size_t)lda * (size_t)n));
    AGP_HIP_CHECK(ctx, hipMemsetAsync(dL32.p, 0xFF, sizeof(float) * (size_t)lda * (size_t)n, s));  // (all ones: a NaN)
  }
  if (kind == WS_BWD_VEC_ANY_WIDE) {
    AGP_HIP_CHECK(ctx, dws.alloc(backsolve_ws_elems(n)));
    backward_solve_vec_any(s, f->A, n, lda, f->invd, dz.p, dws.p, 0, nullptr);
  } else if (kind == WS_MIXED_PRECONDITION) {
    AGP_HIP_CHECK(ctx, din.alloc((size_t)n));
    AGP_HIP_CHECK(ctx, dt1.alloc((size_t)z_doubles));
    AGP_HIP_CHECK(ctx, dt2.alloc((size_t)z_doubles));
    AGP_HIP_CHECK(ctx, dW.alloc(wide));
    AGP_HIP_CHECK(ctx, dWT.alloc(wide));
    AGP_HIP_CHECK(ctx, dws.alloc((size_t)n));
    AGP_HIP_CHECK(ctx, hipMemcpy(din.p, z, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    AGP_HIP_CHECK(ctx, hipMemsetAsync(dt1.p, 0xFF, zbytes, s));
    AGP_HIP_CHECK(ctx, hipMemsetAsync(dt2.p, 0xFF, zbytes, s));
    MixedPreconditioner pc;
    pc.A = f->A; pc.n = n; pc.lda = lda; pc.BW = BW;
    pc.W = dW.p; pc.WT = dWT.p; pc.L32 = dL32.p;
    pc.t1 = dt1.p; pc.t2 = dt2.p; pc.scratch = dws.p;
    const int stp = mixed_precondition_setup(s, pc, f->invd);
    if (stp != AGP_OK) return stp;
    // (mixed_precondition_apply, with the forward sweep's result kept before the backward sweep consumes it)
    mixed_precondition_forward(s, pc, din.p);
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(dt1.p, dt2.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    mixed_precondition_backward(s, pc, dz.p);
  } else {
    AGP_HIP_CHECK(ctx, dW.alloc(wide));
    AGP_HIP_CHECK(ctx, dws.alloc((size_t)n));
    invert_wide_blocks(s, f->A, n, lda, f->invd, BW, dW.p);
    if (a32) launch_convert_lower_f32(s, f->A, lda, n, dL32.p);
    if (kind == WS_FWD_VEC_WIDE) forward_solve_vec_wide(s, f->A, n, lda, dW.p, BW, dz.p, dws.p, dL32.p);
    else backward_solve_vec_wide(s, f->A, n, lda, dW.p, BW, dz.p, dws.p, dL32.p);
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(z, dz.p, zbytes, hipMemcpyDeviceToHost));
  if (kind == WS_MIXED_PRECONDITION) AGP_HIP_CHECK(ctx, hipMemcpy(t2_out, dt1.p, zbytes, hipMemcpyDeviceToHost));
  if (L_out)
    AGP_HIP_CHECK(ctx, hipMemcpy2D(L_out, sizeof(double) * (size_t)n, f->A, sizeof(double) * (size_t)lda, sizeof(double) * (size_t)n,
                                   (size_t)n, hipMemcpyDeviceToHost));
  if (L32_out)
    AGP_HIP_CHECK(ctx, hipMemcpy2D(L32_out, sizeof(float) * (size_t)n, dL32.p, sizeof(float) * (size_t)lda, sizeof(float) * (size_t)n,
                                   (size_t)n, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// ONE launch_* of reduce.hip on host data (tests/test_reduce_kernels_gpu.py).  bufs[k] (bytes[k] long, or null for an optional
// pointer) are copied to the device whole, the launcher runs once on the context's stream, and every buffer is copied back
// whole - padding, gaps and sentinels included.  Two entries with the SAME host pointer share one device buffer (base
// aliasing out, the variance of loo aliasing diag(K^-1)).  ip / dp: the integer and floating-point arguments, per op in the
// order of the table below; buffers in the order given there.  Every extent the kernels address - the index lists' contents
// included - is checked against bytes[] on the host first: AGP_ERR_INVALID_ARGUMENT, with nothing launched.  So is a
// tall_matvec of more than TALL_MATVEC_MAX_COLS columns, for which the launcher would silently do nothing.
//   RED_COLDOT               ip lda ldb n m;  dp scale;  A B out [base]
//   RED_DOT                  ip n;  a b out
//   RED_MATVEC               ip ld m n;  dp alpha beta;  W x partial [base] out        (n = 0: W and x may be null)
//   RED_TALL_MATVEC(_F32)    ip ld rows ncols;  dp alpha beta;  W x [base] out
//   RED_COLVEC_DOT(_F32)     ip ld m n;  dp alpha beta;  W v [base] out
//   RED_COLVEC_DOT_STRIDED   ip ld stride_W m n stride_v count;  dp alpha beta;  W v [base] out
//   RED_COLVEC_DOT_BATCHED   ip ld stride_Q m stride_z count;  Q z out
//   RED_SYMV_LOWER_BATCHED   ip ld stride_K n stride_v count;  K p out
//   RED_CONTRACT             ip ldk na nb symmetric ldo;  K [xoff] [xc] [yoff] [yc] out
//   RED_SYMMETRIZE, RED_ZERO_UPPER, RED_SET_IDENTITY   ip ld n;  A
//   RED_UPPER_TO_LOWER       ip ld_src ld_dst n;  src dst
//   RED_TRANSPOSE_BLOCKS     ip m count;  src dst
//   RED_SET_IDENTITY_BATCHED ip ld stride m count;  B
//   RED_NEGATE               ip ld m;  A [diag_out]
//   RED_NAN_SCAN_LOWER       ip ld n;  A flag(int)
//   RED_COPY_LOWER           ip ld n;  src dst [flag(int)]          (ld even)
//   RED_CONVERT_LOWER_F32    ip ld n;  L L32(float)                 (ld even)
//   RED_LOO                  ip n;  kinv_diag y information mean variance
//   RED_GATHER_COLS          ip ldr m row0 n ldg cols_of_R;  R idx(int64) G
//   RED_GATHER_VEC           ip m len_of_src;  src idx(int64) [sub] out
//   RED_PAD_COLUMNS          ip ld_src smax n_groups rows ld_dst dir;  src off(int64) dst
//   RED_PAD_IDENTITY         ip ld stride smax n_groups;  A off(int64)
//   RED_COMPACT_BLOCKS       ip ld stride smax n_groups;  slabs off(int64) boff(int64) out
//   RED_AXPBY                ip n;  dp a b;  [x] [y] out
enum {
  RED_COLDOT = 0, RED_DOT, RED_MATVEC, RED_TALL_MATVEC, RED_TALL_MATVEC_F32, RED_COLVEC_DOT, RED_COLVEC_DOT_STRIDED,
  RED_COLVEC_DOT_BATCHED, RED_COLVEC_DOT_F32, RED_SYMV_LOWER_BATCHED, RED_CONTRACT, RED_SYMMETRIZE, RED_UPPER_TO_LOWER,
  RED_TRANSPOSE_BLOCKS, RED_ZERO_UPPER, RED_SET_IDENTITY, RED_SET_IDENTITY_BATCHED, RED_NEGATE, RED_NAN_SCAN_LOWER,
  RED_COPY_LOWER, RED_CONVERT_LOWER_F32, RED_LOO, RED_GATHER_COLS, RED_GATHER_VEC, RED_PAD_COLUMNS, RED_PAD_IDENTITY,
  RED_COMPACT_BLOCKS, RED_AXPBY, RED_OPS
};
AGP_DEBUG_API int agp_debug_reduce(agp_context *ctx, int op, const int64_t *ip, int n_ip, const double *dp, int n_dp, void *const *bufs,
                                   const int64_t *bytes, int n_bufs) {
  constexpr int MAXB = 6;
  constexpr long long LIM = 1ll << 26;  // no dimension, stride or count of a test comes near it: the products below cannot overflow
  if (!ctx || op < 0 || op >= RED_OPS || !ip || !bufs || !bytes || n_ip < 1 || n_ip > 8 || n_dp < 0 || n_dp > 2 || (n_dp && !dp) ||
      n_bufs < 1 || n_bufs > MAXB)
    return AGP_ERR_INVALID_ARGUMENT;
  long long I[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n_ip; ++k) {
    if (ip[k] < 0 || ip[k] > LIM) return AGP_ERR_INVALID_ARGUMENT;
    I[k] = ip[k];
  }
  const double d0 = n_dp > 0 ? dp[0] : 0., d1 = n_dp > 1 ? dp[1] : 0.;
  for (int k = 0; k < n_bufs; ++k)
    if (bytes[k] < 0 || (bufs[k] && bytes[k] == 0)) return AGP_ERR_INVALID_ARGUMENT;
  auto has = [&](int k) { return k < n_bufs && bufs[k] != nullptr; };
  // buffer k is there and holds `elems` elements of `esize` bytes
  auto fits = [&](int k, long long elems, long long esize = 8) { return has(k) && elems >= 0 && elems <= LIM * 64 && bytes[k] >= elems * esize; };
  auto opt_fits = [&](int k, long long elems) { return !has(k) || fits(k, elems); };
  // elements a column-major rows x cols matrix of leading dimension ld spans; -1 (fits nothing) for ld < rows
  auto mat = [](long long ld, long long rows, long long cols) -> long long {
    if (ld < rows || rows < 1 || cols < 1) return -1;
    return ld * (cols - 1) + rows;
  };
  auto slabs = [&](long long count, long long stride, long long one) -> long long {
    return (count < 1 || one < 0) ? -1 : (count - 1) * stride + one;
  };
  // a list of `entries` int64 in buffer k
  auto list = [&](int k, long long entries) -> const long long * {
    return fits(k, entries) ? static_cast<const long long *>(bufs[k]) : nullptr;
  };
  // group offsets off[0 .. groups]: ascending from >= 0, no group larger than smax; the total, or -1
  auto groups_total = [&](const long long *off, long long groups, long long smax) -> long long {
    if (!off || off[0] < 0) return -1;
    for (long long g = 0; g < groups; ++g)
      if (off[g + 1] < off[g] || off[g + 1] - off[g] > smax || off[g + 1] > LIM) return -1;
    return off[groups];
  };
  bool ok = false;
  switch (op) {
  case RED_COLDOT:
    ok = n_ip == 4 && fits(0, mat(I[0], I[2], I[3])) && fits(1, mat(I[1], I[2], I[3])) && fits(2, I[3]) && I[3] >= 1 && opt_fits(3, I[3]);
    break;
  case RED_DOT: ok = n_ip == 1 && I[0] >= 1 && fits(0, I[0]) && fits(1, I[0]) && fits(2, 1); break;
  case RED_MATVEC:
    ok = n_ip == 3 && I[1] >= 1 && I[0] >= I[1] && (I[2] == 0 || (fits(0, mat(I[0], I[1], I[2])) && fits(1, I[2]))) &&
         fits(2, (I[2] + 1023) / 1024 * I[1]) && opt_fits(3, I[1]) && fits(4, I[1]);
    break;
  case RED_TALL_MATVEC:
  case RED_TALL_MATVEC_F32:
    ok = n_ip == 3 && I[2] <= TALL_MATVEC_MAX_COLS && fits(0, mat(I[0], I[1], I[2]), op == RED_TALL_MATVEC ? 8 : 4) && fits(1, I[2]) &&
         opt_fits(2, I[1]) && fits(3, I[1]);
    break;
  case RED_COLVEC_DOT:
  case RED_COLVEC_DOT_F32:
    ok = n_ip == 3 && fits(0, mat(I[0], I[1], I[2]), op == RED_COLVEC_DOT ? 8 : 4) && fits(1, I[1]) && opt_fits(2, I[2]) && fits(3, I[2]);
    break;
  case RED_COLVEC_DOT_STRIDED:
    ok = n_ip == 6 && fits(0, slabs(I[5], I[1], mat(I[0], I[2], I[3]))) && fits(1, slabs(I[5], I[4], I[2])) &&
         opt_fits(2, slabs(I[5], I[4], I[3])) && fits(3, slabs(I[5], I[4], I[3]));
    break;
  case RED_COLVEC_DOT_BATCHED:
    ok = n_ip == 5 && fits(0, slabs(I[4], I[1], mat(I[0], I[2], I[2]))) && fits(1, slabs(I[4], I[3], I[2])) && I[4] >= 1 &&
         fits(2, I[4] * I[2]);
    break;
  case RED_SYMV_LOWER_BATCHED:
    ok = n_ip == 5 && fits(0, slabs(I[4], I[1], mat(I[0], I[2], I[2]))) && fits(1, slabs(I[4], I[3], I[2])) &&
         fits(2, slabs(I[4], I[3], I[2]));
    break;
  case RED_CONTRACT: {
    const long long na = I[1], nb = I[2];
    if (n_ip != 5 || na < 1 || nb < 1 || (I[3] && na != nb)) break;
    const long long nx = has(1) ? groups_total(list(1, na + 1), na, LIM) : na, ny = has(3) ? groups_total(list(3, nb + 1), nb, LIM) : nb;
    // (an empty K - every member list empty - is never addressed)
    ok = nx >= 0 && ny >= 0 && (nx == 0 || ny == 0 || fits(0, mat(I[0], nx, ny))) && has(0) && opt_fits(2, nx) && opt_fits(4, ny) &&
         fits(5, mat(I[4], na, nb));
    break;
  }
  case RED_SYMMETRIZE:
  case RED_ZERO_UPPER:
  case RED_SET_IDENTITY: ok = n_ip == 2 && fits(0, mat(I[0], I[1], I[1])); break;
  case RED_UPPER_TO_LOWER: ok = n_ip == 3 && fits(0, mat(I[0], I[2], I[2])) && fits(1, mat(I[1], I[2], I[2])) && bufs[0] != bufs[1]; break;
  case RED_TRANSPOSE_BLOCKS:
    ok = n_ip == 2 && I[0] >= 1 && I[1] >= 1 && fits(0, I[1] * I[0] * I[0]) && fits(1, I[1] * I[0] * I[0]) && bufs[0] != bufs[1];
    break;
  case RED_SET_IDENTITY_BATCHED: ok = n_ip == 4 && fits(0, slabs(I[3], I[1], mat(I[0], I[2], I[2]))); break;
  case RED_NEGATE: ok = n_ip == 2 && fits(0, mat(I[0], I[1], I[1])) && opt_fits(1, I[1]); break;
  case RED_NAN_SCAN_LOWER: ok = n_ip == 2 && fits(0, mat(I[0], I[1], I[1])) && fits(1, 1, 4); break;
  case RED_COPY_LOWER:
    ok = n_ip == 2 && I[0] % 2 == 0 && fits(0, mat(I[0], I[1], I[1])) && fits(1, mat(I[0], I[1], I[1])) && bufs[0] != bufs[1] &&
         (!has(2) || fits(2, 1, 4));
    break;
  case RED_CONVERT_LOWER_F32: ok = n_ip == 2 && I[0] % 2 == 0 && fits(0, mat(I[0], I[1], I[1])) && fits(1, mat(I[0], I[1], I[1]), 4); break;
  case RED_LOO: ok = n_ip == 1 && I[0] >= 1 && fits(0, I[0]) && fits(1, I[0]) && fits(2, I[0]) && fits(3, I[0]) && fits(4, I[0]); break;
  case RED_GATHER_COLS: {
    const long long *idx = n_ip == 6 ? list(1, I[1]) : nullptr;
    ok = idx && I[1] >= 1 && I[2] < I[3] && fits(0, mat(I[0], I[3], I[5])) && fits(2, mat(I[4], I[3], I[1]));
    for (long long a = 0; ok && a < I[1]; ++a) ok = idx[a] < I[5];
    break;
  }
  case RED_GATHER_VEC: {
    const long long *idx = n_ip == 2 ? list(1, I[0]) : nullptr;
    ok = idx && I[0] >= 1 && I[1] >= 1 && fits(0, I[1]) && opt_fits(2, I[0]) && fits(3, I[0]);
    for (long long a = 0; ok && a < I[0]; ++a) ok = idx[a] < I[1];
    break;
  }
  case RED_PAD_COLUMNS: {
    if (n_ip != 6 || I[1] < 1 || I[2] < 1 || I[5] > 1) break;
    const long long total = groups_total(list(1, I[2] + 1), I[2], I[1]);
    const long long compact = total > 0 ? mat(I[5] == 0 ? I[0] : I[4], I[3], total) : 0;
    const long long padded = mat(I[5] == 0 ? I[4] : I[0], I[3], I[1] * I[2]);
    ok = total >= 0 && compact >= 0 && has(I[5] == 0 ? 0 : 2) && fits(I[5] == 0 ? 0 : 2, compact) && fits(I[5] == 0 ? 2 : 0, padded);
    break;
  }
  case RED_PAD_IDENTITY:
    ok = n_ip == 4 && I[2] >= 1 && I[3] >= 1 && groups_total(list(1, I[3] + 1), I[3], I[2]) >= 0 &&
         fits(0, slabs(I[3], I[1], mat(I[0], I[2], I[2])));
    break;
  case RED_COMPACT_BLOCKS: {
    if (n_ip != 4 || I[2] < 1 || I[3] < 1) break;
    const long long *off = list(1, I[3] + 1), *boff = list(2, I[3]);
    ok = boff && groups_total(off, I[3], I[2]) >= 0 && fits(0, slabs(I[3], I[1], mat(I[0], I[2], I[2]))) && has(3);
    for (long long g = 0; ok && g < I[3]; ++g) {
      const long long sg = off[g + 1] - off[g];
      ok = boff[g] >= 0 && boff[g] <= LIM && fits(3, boff[g] + sg * sg);
    }
    break;
  }
  default:  // RED_AXPBY
    ok = n_ip == 1 && I[0] >= 1 && opt_fits(0, I[0]) && opt_fits(1, I[0]) && fits(2, I[0]);
    break;
  }
  if (!ok) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<char> dev[MAXB];
  void *d[MAXB] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int owner[MAXB];
  for (int k = 0; k < n_bufs; ++k) {
    owner[k] = k;
    if (!bufs[k]) continue;
    for (int j = 0; j < k; ++j)
      if (bufs[j] == bufs[k]) { owner[k] = j; break; }
    if (owner[k] != k) {
      if (bytes[k] > bytes[owner[k]]) return AGP_ERR_INVALID_ARGUMENT;
      d[k] = d[owner[k]];
      continue;
    }
    AGP_HIP_CHECK(ctx, dev[k].alloc((size_t)bytes[k]));
    AGP_HIP_CHECK(ctx, hipMemcpy(dev[k].p, bufs[k], (size_t)bytes[k], hipMemcpyHostToDevice));
    d[k] = dev[k].p;
  }
  auto D = [&](int k) { return static_cast<double *>(d[k]); };
  auto F = [&](int k) { return static_cast<float *>(d[k]); };
  auto L = [&](int k) { return static_cast<long long *>(d[k]); };
  auto N = [&](int k) { return static_cast<int *>(d[k]); };
  switch (op) {
  case RED_COLDOT: launch_coldot(s, D(0), I[0], D(1), I[1], I[2], I[3], D(2), d0, D(3)); break;
  case RED_DOT: launch_dot(s, D(0), D(1), I[0], D(2)); break;
  case RED_MATVEC: launch_matvec(s, D(0), I[0], I[1], I[2], D(1), D(2), d0, d1, D(3), D(4)); break;
  case RED_TALL_MATVEC: launch_tall_matvec(s, D(0), I[0], I[1], I[2], D(1), d0, d1, D(2), D(3)); break;
  case RED_TALL_MATVEC_F32: launch_tall_matvec_f32(s, F(0), I[0], I[1], I[2], D(1), d0, d1, D(2), D(3)); break;
  case RED_COLVEC_DOT: launch_colvec_dot(s, D(0), I[0], I[1], I[2], D(1), d0, d1, D(2), D(3)); break;
  case RED_COLVEC_DOT_F32: launch_colvec_dot_f32(s, F(0), I[0], I[1], I[2], D(1), d0, d1, D(2), D(3)); break;
  case RED_COLVEC_DOT_STRIDED: launch_colvec_dot_strided(s, D(0), I[0], I[1], I[2], I[3], D(1), I[4], d0, d1, D(2), D(3), I[5]); break;
  case RED_COLVEC_DOT_BATCHED: launch_colvec_dot_batched(s, D(0), I[0], I[1], I[2], D(1), I[3], I[4], D(2)); break;
  case RED_SYMV_LOWER_BATCHED: launch_symv_lower_batched(s, D(0), I[0], I[1], I[2], D(1), I[3], D(2), I[4]); break;
  case RED_CONTRACT: launch_contract_combinations(s, D(0), I[0], L(1), D(2), I[1], L(3), D(4), I[2], I[3] != 0, D(5), I[4]); break;
  case RED_SYMMETRIZE: launch_symmetrize(s, D(0), I[0], I[1]); break;
  case RED_ZERO_UPPER: launch_zero_upper(s, D(0), I[0], I[1]); break;
  case RED_SET_IDENTITY: launch_set_identity(s, D(0), I[0], I[1]); break;
  case RED_UPPER_TO_LOWER: launch_upper_to_lower(s, D(0), I[0], D(1), I[1], I[2]); break;
  case RED_TRANSPOSE_BLOCKS: launch_transpose_blocks(s, D(0), D(1), I[0], I[1]); break;
  case RED_SET_IDENTITY_BATCHED: launch_set_identity_batched(s, D(0), I[0], I[1], I[2], I[3]); break;
  case RED_NEGATE: launch_negate(s, D(0), I[0], I[1], D(1)); break;
  case RED_NAN_SCAN_LOWER: launch_nan_scan_lower(s, D(0), I[0], I[1], N(1)); break;
  case RED_COPY_LOWER: launch_copy_lower(s, D(0), I[0], I[1], D(1), N(2)); break;
  case RED_CONVERT_LOWER_F32: launch_convert_lower_f32(s, D(0), I[0], I[1], F(1)); break;
  case RED_LOO: launch_loo(s, D(0), D(1), D(2), I[0], D(3), D(4)); break;
  case RED_GATHER_COLS: launch_gather_cols(s, D(0), I[0], L(1), I[1], I[2], I[3], D(2), I[4]); break;
  case RED_GATHER_VEC: launch_gather_vec(s, D(0), L(1), I[0], D(2), D(3)); break;
  case RED_PAD_COLUMNS: launch_pad_columns(s, D(0), I[0], L(1), I[1], I[2], I[3], D(2), I[4], (int)I[5]); break;
  case RED_PAD_IDENTITY: launch_pad_identity(s, D(0), I[0], I[1], L(1), I[2], I[3]); break;
  case RED_COMPACT_BLOCKS: launch_compact_blocks(s, D(0), I[0], I[1], L(1), L(2), I[2], I[3], D(3)); break;
  default: launch_axpby(s, I[0], d0, D(0), d1, D(1), D(2)); break;
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  for (int k = 0; k < n_bufs; ++k)
    if (bufs[k] && owner[k] == k) AGP_HIP_CHECK(ctx, hipMemcpy(bufs[k], dev[k].p, (size_t)bytes[k], hipMemcpyDeviceToHost));
  return AGP_OK;
}

// sizeof(PcgCtrl) and the byte offset of every field (iterative_internal.h), then PCG_COLS, PCG_LOOK, PCG_DOT_THREADS and
// PCG_ERROR: out[0 .. 15].  tests/test_pcg_kernels_gpu.py asserts its mirror of the struct against this.
AGP_DEBUG_API int agp_debug_pcg_ctrl_layout(int64_t *out, int cap) {
  if (!out || cap < 16) return AGP_ERR_INVALID_ARGUMENT;
  const int64_t v[16] = {(int64_t)sizeof(PcgCtrl), (int64_t)offsetof(PcgCtrl, active), (int64_t)offsetof(PcgCtrl, npd),
                         (int64_t)offsetof(PcgCtrl, nan), (int64_t)offsetof(PcgCtrl, pad), (int64_t)offsetof(PcgCtrl, stopped),
                         (int64_t)offsetof(PcgCtrl, iters), (int64_t)offsetof(PcgCtrl, bb), (int64_t)offsetof(PcgCtrl, rz),
                         (int64_t)offsetof(PcgCtrl, alpha), (int64_t)offsetof(PcgCtrl, beta), (int64_t)offsetof(PcgCtrl, resid),
                         PCG_COLS, PCG_LOOK, PCG_DOT_THREADS, PCG_ERROR};
  for (int k = 0; k < 16; ++k) out[k] = v[k];
  return AGP_OK;
}

// ONE kernel of iterative.hip on host data, through its launcher of iterative_internal.h - the grid and block arithmetic
// the product runs (tests/test_pcg_kernels_gpu.py).  The calling convention of agp_debug_reduce: bufs[k] (bytes[k] long, or
// null for an optional pointer) are copied to the device whole, the launcher runs once on the context's stream, and every
// buffer is copied back whole - padding and sentinels included.  Two entries with the SAME host pointer share one device
// buffer (the r . r of DOT_BB and DOT_RR).  The control block is a buffer like the others: the test sets active, stopped[]
// and rz[][] before the launch and reads every field after it.  Every extent a kernel addresses is checked against bytes[]
// on the host first: AGP_ERR_INVALID_ARGUMENT, with nothing launched.
//   PCG_OP_DOT_BB / _RZ / _PQ / _RR   ip ld n t k;  dp tol;  ctrl A B
//   PCG_OP_LT_R                       ip ldl n m ldr t ldt;  ctrl L R T1                     (m >= 1)
//   PCG_OP_PRECOND                    ip ldl n m ldu ld t;  dp delta;  ctrl [L] [U] R Z      (m = 0: L and U may be null)
//   PCG_OP_P                          ip ld n t first;  ctrl Z P
//   PCG_OP_XR                         ip ldx ld n t;  ctrl X R P Q
//   PCG_OP_DIAG_STATS                 ip n;  d [yvar] stats(4)
//   PCG_OP_SHIFT                      ip ldc m;  dp delta;  C
//   PCG_OP_VARIANCE                   ip ld n t;  Kc S prior var
enum {
  PCG_OP_DOT_BB = 0, PCG_OP_DOT_RZ, PCG_OP_DOT_PQ, PCG_OP_DOT_RR, PCG_OP_LT_R, PCG_OP_PRECOND, PCG_OP_P, PCG_OP_XR,
  PCG_OP_DIAG_STATS, PCG_OP_SHIFT, PCG_OP_VARIANCE, PCG_OPS
};
AGP_DEBUG_API int agp_debug_pcg(agp_context *ctx, int op, const int64_t *ip, int n_ip, const double *dp, int n_dp, void *const *bufs,
                                const int64_t *bytes, int n_bufs) {
  constexpr int MAXB = 5;
  constexpr long long LIM = 1ll << 26;  // no dimension of a test comes near it: the products below cannot overflow
  if (!ctx || op < 0 || op >= PCG_OPS || !ip || !bufs || !bytes || n_ip < 1 || n_ip > 6 || n_dp < 0 || n_dp > 1 || (n_dp && !dp) ||
      n_bufs < 1 || n_bufs > MAXB)
    return AGP_ERR_INVALID_ARGUMENT;
  long long I[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n_ip; ++k) {
    if (ip[k] < 0 || ip[k] > LIM) return AGP_ERR_INVALID_ARGUMENT;
    I[k] = ip[k];
  }
  const double d0 = n_dp > 0 ? dp[0] : 0.;
  for (int k = 0; k < n_bufs; ++k)
    if (bytes[k] < 0 || (bufs[k] && bytes[k] == 0)) return AGP_ERR_INVALID_ARGUMENT;
  auto has = [&](int k) { return k < n_bufs && bufs[k] != nullptr; };
  auto fits = [&](int k, long long elems) { return has(k) && elems >= 0 && elems <= LIM * 64 && bytes[k] >= elems * 8; };
  auto opt_fits = [&](int k, long long elems) { return !has(k) || fits(k, elems); };
  auto ctrl_fits = [&](int k) { return has(k) && bytes[k] >= (long long)sizeof(PcgCtrl); };
  // elements a column-major rows x cols matrix of leading dimension ld spans; -1 (fits nothing) for ld < rows
  auto mat = [](long long ld, long long rows, long long cols) -> long long {
    if (ld < rows || rows < 1 || cols < 1) return -1;
    return ld * (cols - 1) + rows;
  };
  auto cols_ok = [](long long t) { return t >= 1 && t <= PCG_COLS; };
  // an output that is also read by the launch under another name would race
  auto distinct = [&](int a, int b) { return !has(a) || !has(b) || bufs[a] != bufs[b]; };
  bool ok = false;
  switch (op) {
  case PCG_OP_DOT_BB:
  case PCG_OP_DOT_RZ:
  case PCG_OP_DOT_PQ:
  case PCG_OP_DOT_RR:
    ok = n_ip == 4 && cols_ok(I[2]) && ctrl_fits(0) && fits(1, mat(I[0], I[1], I[2])) && fits(2, mat(I[0], I[1], I[2])) && distinct(0, 1) &&
         distinct(0, 2);
    break;
  case PCG_OP_LT_R:
    ok = n_ip == 6 && cols_ok(I[4]) && ctrl_fits(0) && fits(1, mat(I[0], I[1], I[2])) && fits(2, mat(I[3], I[1], I[4])) &&
         fits(3, mat(I[5], I[2], I[4])) && distinct(3, 0) && distinct(3, 1) && distinct(3, 2);
    break;
  case PCG_OP_PRECOND:
    ok = n_ip == 6 && cols_ok(I[5]) && ctrl_fits(0) && (I[2] == 0 || (fits(1, mat(I[0], I[1], I[2])) && fits(2, mat(I[3], I[2], I[5])))) &&
         fits(3, mat(I[4], I[1], I[5])) && fits(4, mat(I[4], I[1], I[5])) && distinct(4, 0) && distinct(4, 1) && distinct(4, 2) &&
         distinct(4, 3);
    break;
  case PCG_OP_P:
    ok = n_ip == 4 && cols_ok(I[2]) && ctrl_fits(0) && fits(1, mat(I[0], I[1], I[2])) && fits(2, mat(I[0], I[1], I[2])) && distinct(2, 0) &&
         distinct(2, 1);
    break;
  case PCG_OP_XR:
    ok = n_ip == 4 && cols_ok(I[3]) && ctrl_fits(0) && fits(1, mat(I[0], I[2], I[3])) && fits(2, mat(I[1], I[2], I[3])) &&
         fits(3, mat(I[1], I[2], I[3])) && fits(4, mat(I[1], I[2], I[3])) && distinct(1, 0) && distinct(2, 0) && distinct(1, 2) &&
         distinct(1, 3) && distinct(1, 4) && distinct(2, 3) && distinct(2, 4);
    break;
  case PCG_OP_DIAG_STATS: ok = n_ip == 1 && I[0] >= 1 && fits(0, I[0]) && opt_fits(1, I[0]) && fits(2, 4) && distinct(2, 0) && distinct(2, 1); break;
  case PCG_OP_SHIFT: ok = n_ip == 2 && fits(0, mat(I[0], I[1], I[1])); break;
  default:  // PCG_OP_VARIANCE
    ok = n_ip == 3 && I[2] >= 1 && fits(0, mat(I[0], I[1], I[2])) && fits(1, mat(I[0], I[1], I[2])) && fits(2, I[2]) && fits(3, I[2]) &&
         distinct(3, 0) && distinct(3, 1) && distinct(3, 2);
    break;
  }
  if (!ok) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<char> dev[MAXB];
  void *d[MAXB] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int owner[MAXB];
  for (int k = 0; k < n_bufs; ++k) {
    owner[k] = k;
    if (!bufs[k]) continue;
    for (int j = 0; j < k; ++j)
      if (bufs[j] == bufs[k]) { owner[k] = j; break; }
    if (owner[k] != k) {
      if (bytes[k] > bytes[owner[k]]) return AGP_ERR_INVALID_ARGUMENT;
      d[k] = d[owner[k]];
      continue;
    }
    AGP_HIP_CHECK(ctx, dev[k].alloc((size_t)bytes[k]));
    AGP_HIP_CHECK(ctx, hipMemcpy(dev[k].p, bufs[k], (size_t)bytes[k], hipMemcpyHostToDevice));
    d[k] = dev[k].p;
  }
  auto D = [&](int k) { return static_cast<double *>(d[k]); };
  PcgCtrl *ctrl = static_cast<PcgCtrl *>(d[0]);  // (of the ops that have one)
  switch (op) {
  case PCG_OP_DOT_BB: launch_pcg_dot(s, DOT_BB, ctrl, D(1), D(2), I[0], I[1], (int)I[2], (int)I[3], d0); break;
  case PCG_OP_DOT_RZ: launch_pcg_dot(s, DOT_RZ, ctrl, D(1), D(2), I[0], I[1], (int)I[2], (int)I[3], d0); break;
  case PCG_OP_DOT_PQ: launch_pcg_dot(s, DOT_PQ, ctrl, D(1), D(2), I[0], I[1], (int)I[2], (int)I[3], d0); break;
  case PCG_OP_DOT_RR: launch_pcg_dot(s, DOT_RR, ctrl, D(1), D(2), I[0], I[1], (int)I[2], (int)I[3], d0); break;
  case PCG_OP_LT_R: launch_pcg_lt_r(s, ctrl, D(1), I[0], I[1], I[2], D(2), I[3], (int)I[4], D(3), I[5]); break;
  case PCG_OP_PRECOND: launch_pcg_precond(s, ctrl, D(1), I[0], I[1], I[2], D(2), I[3], D(3), D(4), I[4], (int)I[5], d0); break;
  case PCG_OP_P: launch_pcg_p(s, ctrl, D(1), D(2), I[0], I[1], (int)I[2], (int)I[3]); break;
  case PCG_OP_XR: launch_pcg_xr(s, ctrl, D(1), I[0], D(2), D(3), D(4), I[1], I[2], (int)I[3]); break;
  case PCG_OP_DIAG_STATS: launch_pcg_diag_stats(s, D(0), D(1), I[0], D(2)); break;
  case PCG_OP_SHIFT: launch_pcg_shift(s, D(0), I[0], I[1], d0); break;
  default: launch_pcg_variance(s, D(0), D(1), I[0], I[1], I[2], D(2), D(3)); break;
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  for (int k = 0; k < n_bufs; ++k)
    if (bufs[k] && owner[k] == k) AGP_HIP_CHECK(ctx, hipMemcpy(bufs[k], dev[k].p, (size_t)bytes[k], hipMemcpyDeviceToHost));
  return AGP_OK;
}

// The preconditioner a live matrix-free fit holds: dims[0 .. 2] = n, rank, ldl of the device; *delta; and, where the
// pointers are given, L (n x rank at ldl_out) and the factor of delta I + L^T L (rank x rank at ldc_out: the lower
// triangle as the device holds it, zeros above).  A first call with both null asks for the sizes.
AGP_DEBUG_API int agp_debug_iterative_state(agp_context *ctx, const agp_iterative_fit *fit, int64_t *dims, double *delta, double *L,
                                            int64_t ldl_out, double *C, int64_t ldc_out) {
  if (!ctx || !fit || !dims || !delta) return AGP_ERR_INVALID_ARGUMENT;
  const PcgPrecondState st = iterative_precond_state(fit);
  if (st.ctx != ctx) return AGP_ERR_INVALID_ARGUMENT;
  dims[0] = st.n; dims[1] = st.rank; dims[2] = st.ldl;
  *delta = st.delta;
  if (st.rank == 0 || (!L && !C)) return AGP_OK;
  if ((L && ldl_out < st.n) || (C && ldc_out < st.rank) || !st.L || !st.mfac) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (L)
    AGP_HIP_CHECK(ctx, hipMemcpy2D(L, sizeof(double) * (size_t)ldl_out, st.L, sizeof(double) * (size_t)st.ldl, sizeof(double) * (size_t)st.n,
                                   (size_t)st.rank, hipMemcpyDeviceToHost));
  if (C) {
    AGP_HIP_CHECK(ctx, hipMemcpy2D(C, sizeof(double) * (size_t)ldc_out, st.mfac->A, sizeof(double) * (size_t)st.mfac->lda,
                                   sizeof(double) * (size_t)st.rank, (size_t)st.rank, hipMemcpyDeviceToHost));
    for (long long j = 1; j < st.rank; ++j)
      for (long long i = 0; i < j; ++i) C[j * ldc_out + i] = 0.;
  }
  return AGP_OK;
}

// ONE application Z = P^-1 R of a live fit's preconditioner through pcg_apply_preconditioner - the function every
// iteration of pcg_solve calls - at the leading dimension and with the scratch pcg_solve gives it; the control block has
// active = 1 and stopped[] as given (t ints).  R: n x t at ldr, read; Z: n x t at ldz, uploaded first, so that the column of
// a stopped right-hand side comes back with the bits it had.  The device's padding row (odd n) is NaN on the way in.
AGP_DEBUG_API int agp_debug_iterative_precondition(agp_context *ctx, const agp_iterative_fit *fit, const double *R, int64_t ldr, int t,
                                                   const int *stopped, double *Z, int64_t ldz) {
  if (!ctx || !fit || !R || !Z || !stopped || t < 1 || t > PCG_COLS) return AGP_ERR_INVALID_ARGUMENT;
  const PcgPrecondState st = iterative_precond_state(fit);
  if (st.ctx != ctx || ldr < st.n || ldz < st.n) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const long long n = st.n, m = st.rank, ld = round_up(n, 2), ldt = round_up(m > 0 ? m : 1, 2);
  const size_t vec = (size_t)ld * (size_t)t, t1 = (size_t)ldt * (size_t)t;
  DevBuf<double> Rd, Zd, T1;
  DevBuf<PcgCtrl> cd;
  AGP_HIP_CHECK(ctx, Rd.alloc(vec));
  AGP_HIP_CHECK(ctx, Zd.alloc(vec));
  AGP_HIP_CHECK(ctx, T1.alloc(t1));
  AGP_HIP_CHECK(ctx, cd.alloc(1));
  PcgCtrl h;
  std::memset(&h, 0, sizeof(h));
  h.active = 1;
  for (int c = 0; c < t; ++c) h.stopped[c] = stopped[c];
  AGP_HIP_CHECK(ctx, hipMemset(Rd.p, 0xff, sizeof(double) * vec));  // (all bits set: a NaN)
  AGP_HIP_CHECK(ctx, hipMemset(Zd.p, 0xff, sizeof(double) * vec));
  AGP_HIP_CHECK(ctx, hipMemset(T1.p, 0xff, sizeof(double) * t1));
  AGP_HIP_CHECK(ctx, hipMemcpy(cd.p, &h, sizeof(h), hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy2D(Rd.p, sizeof(double) * (size_t)ld, R, sizeof(double) * (size_t)ldr, sizeof(double) * (size_t)n, (size_t)t,
                                 hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy2D(Zd.p, sizeof(double) * (size_t)ld, Z, sizeof(double) * (size_t)ldz, sizeof(double) * (size_t)n, (size_t)t,
                                 hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  pcg_apply_preconditioner(s, fit, cd.p, Rd.p, Zd.p, ld, t, T1.p, ldt);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy2D(Z, sizeof(double) * (size_t)ldz, Zd.p, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n, (size_t)t,
                                 hipMemcpyDeviceToHost));
  return AGP_OK;
}

// ---- the log-likelihood value of the matrix-free fit (agp_iterative_nll) -----------------------------------------------------
// lanczos_quadrature.h on host arrays: *out = rz0 e_1^T log(T) e_1 for the tridiagonal of the k coefficient pairs.  Host
// only: no context, no device.
AGP_DEBUG_API int agp_debug_lanczos_quadrature(double rz0, const double *a, const double *b, int k, double *out) {
  return lanczos_quadrature(rz0, a, b, 1, k, out);
}

// ONE launch of pcg_record_kernel through launch_pcg_record.  ctrl: a host PcgCtrl; buf: log_len doubles, uploaded and
// downloaded whole, the log (pcg_log_elems(max_iterations) doubles) starting at buf[offset] - what lies around it are the
// caller's canaries.  Extents are checked first: AGP_ERR_INVALID_ARGUMENT, nothing launched.
AGP_DEBUG_API int agp_debug_pcg_record(agp_context *ctx, const void *ctrl, double *buf, int64_t log_len, int64_t offset, int max_iterations,
                                       int k, int t) {
  if (!ctx || !ctrl || !buf || max_iterations < 1 || max_iterations > (1 << 20) || k < 0 || k >= max_iterations || t < 1 || t > PCG_COLS ||
      offset < 0 || log_len < 1 || offset > log_len || (int64_t)pcg_log_elems(max_iterations) > log_len - offset)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DevBuf<double> d;
  DevBuf<PcgCtrl> cd;
  AGP_HIP_CHECK(ctx, d.alloc((size_t)log_len));
  AGP_HIP_CHECK(ctx, cd.alloc(1));
  AGP_HIP_CHECK(ctx, hipMemcpy(d.p, buf, sizeof(double) * (size_t)log_len, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipMemcpy(cd.p, ctrl, sizeof(PcgCtrl), hipMemcpyHostToDevice));
  launch_pcg_record(ctx->stream, cd.p, d.p + offset, max_iterations, k, t);
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(buf, d.p, sizeof(double) * (size_t)log_len, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// The probes agp_iterative_nll draws for `seed` on a live fit, columns 0 .. t - 1 chunk by chunk through
// iterative_queue_probes, at the leading dimensions the entry uses.  Z: host, n x t at ldz.
AGP_DEBUG_API int agp_debug_iterative_probes(agp_context *ctx, const agp_iterative_fit *fit, uint64_t seed, int64_t t, double *Z, int64_t ldz) {
  if (!ctx || !fit || !Z || t < 1 || t > (1 << 20)) return AGP_ERR_INVALID_ARGUMENT;
  const PcgPrecondState st = iterative_precond_state(fit);
  if (st.ctx != ctx || ldz < st.n) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const long long n = st.n, m = st.rank, ld = round_up(n, 2), ldg = round_up(m > 0 ? m : 1, 2);
  DevBuf<double> Zd, G1;
  AGP_HIP_CHECK(ctx, Zd.alloc((size_t)ld * PCG_COLS));
  AGP_HIP_CHECK(ctx, G1.alloc((size_t)ldg * PCG_COLS));
  for (long long c0 = 0; c0 < t; c0 += PCG_COLS) {
    const int tc = (int)(t - c0 < PCG_COLS ? t - c0 : PCG_COLS);
    iterative_queue_probes(s, fit, seed, c0, tc, Zd.p, ld, G1.p, ldg);
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
    AGP_HIP_CHECK(ctx, hipGetLastError());
    AGP_HIP_CHECK(ctx, hipMemcpy2D(Z + c0 * ldz, sizeof(double) * (size_t)ldz, Zd.p, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n,
                                   (size_t)tc, hipMemcpyDeviceToHost));
  }
  return AGP_OK;
}

// agp_iterative_solve on host right-hand sides with the coefficient log kept (iterative_solve_logged: pcg_solve itself).
// log: ceil(nrhs / PCG_COLS) * pcg_log_elems(max_iterations) host doubles, one log per chunk; only rows 0 .. (the chunk's
// longest recurrence) - 1 are written, the rest keeps the caller's bits.  *max_iterations: the fit's.  A first call with B
// null asks for that alone.
AGP_DEBUG_API int agp_debug_iterative_solve_logged(agp_context *ctx, const agp_iterative_fit *fit, const double *B, int64_t ldb, int64_t nrhs,
                                                   double *X, int64_t ldx, int *iterations, double *residual, double *log, int64_t log_len,
                                                   double tolerance, int *max_iterations) {
  if (!ctx || !fit || !max_iterations) return AGP_ERR_INVALID_ARGUMENT;
  const PcgPrecondState st = iterative_precond_state(fit);
  if (st.ctx != ctx) return AGP_ERR_INVALID_ARGUMENT;
  *max_iterations = iterative_max_iterations(fit);
  if (!B) return AGP_OK;
  const long long n = st.n, ld = round_up(n, 2), chunks = (nrhs + PCG_COLS - 1) / PCG_COLS;
  if (!X || !log || nrhs < 1 || nrhs > 4096 || ldb < n || ldx < n || log_len < chunks * (int64_t)pcg_log_elems(*max_iterations))
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DevBuf<double> Bd, Xd;
  AGP_HIP_CHECK(ctx, Bd.alloc((size_t)ld * (size_t)nrhs));
  AGP_HIP_CHECK(ctx, Xd.alloc((size_t)ld * (size_t)nrhs));
  AGP_HIP_CHECK(ctx, hipMemcpy2D(Bd.p, sizeof(double) * (size_t)ld, B, sizeof(double) * (size_t)ldb, sizeof(double) * (size_t)n, (size_t)nrhs,
                                 hipMemcpyHostToDevice));
  const int status = iterative_solve_logged(ctx, fit, Bd.p, ld, nrhs, Xd.p, ld, iterations, residual, log, tolerance);
  if (status != AGP_OK) return status;
  AGP_HIP_CHECK(ctx, hipMemcpy2D(X, sizeof(double) * (size_t)ldx, Xd.p, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n, (size_t)nrhs,
                                 hipMemcpyDeviceToHost));
  return AGP_OK;
}

// ONE chunk of a live solve iteration by iteration (iterative_solve_stepped): trace receives the control block after every
// iteration (trace_len >= max_iterations * sizeof(PcgCtrl) bytes), *steps the iterations queued, log the chunk's
// coefficient log (pcg_log_elems(max_iterations) doubles, rows 0 .. *steps - 1 written).
AGP_DEBUG_API int agp_debug_iterative_solve_stepped(agp_context *ctx, const agp_iterative_fit *fit, const double *B, int64_t ldb, int t, double *X,
                                                    int64_t ldx, void *trace, int64_t trace_len, int *steps, double *log, int64_t log_len) {
  if (!ctx || !fit || !B || !X || !trace || !steps || !log || t < 1 || t > PCG_COLS) return AGP_ERR_INVALID_ARGUMENT;
  const PcgPrecondState st = iterative_precond_state(fit);
  const int max_it = iterative_max_iterations(fit);
  const long long n = st.n, ld = round_up(n, 2);
  if (st.ctx != ctx || ldb < n || ldx < n || trace_len < (int64_t)max_it * (int64_t)sizeof(PcgCtrl) || log_len < (int64_t)pcg_log_elems(max_it))
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DevBuf<double> Bd, Xd;
  AGP_HIP_CHECK(ctx, Bd.alloc((size_t)ld * (size_t)t));
  AGP_HIP_CHECK(ctx, Xd.alloc((size_t)ld * (size_t)t));
  AGP_HIP_CHECK(ctx, hipMemcpy2D(Bd.p, sizeof(double) * (size_t)ld, B, sizeof(double) * (size_t)ldb, sizeof(double) * (size_t)n, (size_t)t,
                                 hipMemcpyHostToDevice));
  const int status = iterative_solve_stepped(ctx, fit, Bd.p, ld, t, Xd.p, ld, static_cast<PcgCtrl *>(trace), steps, log);
  if (status != AGP_OK) return status;
  AGP_HIP_CHECK(ctx, hipMemcpy2D(X, sizeof(double) * (size_t)ldx, Xd.p, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n, (size_t)t,
                                 hipMemcpyDeviceToHost));
  return AGP_OK;
}

// ---- the gradient contraction kernels (contract.h: contract_tile) on the caller's weights ---------------------------------
// The launchers of contract_internal.h, which the gradient entries call too: no fit, Gram or factorisation between the input
// and the kernel.  Every host array comes with its length in doubles and is uploaded whole, padding and canaries included;
// `out`, `partial` (and `combo`) are uploaded from the caller and downloaded whole, so what no kernel wrote comes back bit for
// bit.  The features keep the is_measurement flag the caller set.
}  // extern "C"

namespace {
int upload_doubles(agp_context *ctx, DevBuf<double> &d, const double *src, int64_t elems) {
  AGP_HIP_CHECK(ctx, d.alloc((size_t)(elems > 0 ? elems : 1)));
  if (elems > 0) AGP_HIP_CHECK(ctx, hipMemcpy(d.p, src, sizeof(double) * (size_t)elems, hipMemcpyHostToDevice));
  return AGP_OK;
}
// a column-major rows x cols matrix at leading dimension ld fits `elems` doubles
bool matrix_fits(int64_t rows, int64_t cols, int64_t ld, int64_t elems) {
  return rows > 0 && cols > 0 && ld >= rows && elems >= ld * (cols - 1) + rows;
}
// the slot table of a probe, and the tangent columns its AGP_OP_SCALING slots read: n values per column at ldt
int check_probe_slots(const agp_kernel *k, int n_slots, const agp_gradient_slot *slots, int64_t n, const double *tangents, int64_t ldt,
                      int64_t tang_elems, int *ntc) {
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && !slots)) return AGP_ERR_INVALID_ARGUMENT;
  const int st = check_slots(k, n_slots, slots, ntc);
  if (st != AGP_OK) return st;
  if (*ntc > 0 && (!tangents || !matrix_fits(n, *ntc, ldt, tang_elems))) return AGP_ERR_INVALID_ARGUMENT;
  return AGP_OK;
}
}  // namespace

extern "C" {

// nll_grad_contract_kernel<DIMP, LOO> + nll_grad_reduce_kernel, GRAD_GROUP slots per pass as contract_slots runs them:
// out[slot] = scale * sum over the lower triangle of (C_ij - alpha_i alpha_j) dk_ij / dslot (off-diagonal pairs twice), or with
// loo of (C_ij - (u_i alpha_j + alpha_i u_j) / 2) ...  C: n x n at ldc (only its lower triangle may be read), alpha and u: n
// values (u is uploaded and handed to the kernel whatever loo says).  partial: at least lower_tiles(n) * GRAD_GROUP doubles,
// comes back holding the partial[tile][GRAD_GROUP] of the LAST slot group.
AGP_DEBUG_API int agp_debug_contract_dense(agp_context *ctx, const agp_kernel *k, const agp_features *x, int n_slots,
                                           const agp_gradient_slot *slots, const double *tangents, int64_t ldt, int64_t tang_elems,
                                           int loo, const double *C, int64_t ldc, int64_t c_elems, const double *alpha, const double *u,
                                           double scale, double *out, int64_t out_elems, double *partial, int64_t partial_elems) {
  if (!ctx || !k || !x || !C || !alpha || !u || !out || !partial) return AGP_ERR_INVALID_ARGUMENT;
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n <= 0 || !matrix_fits(n, n, ldc, c_elems)) return AGP_ERR_INVALID_ARGUMENT;
  int ntc = 0;
  if ((st = check_probe_slots(k, n_slots, slots, n, tangents, ldt, tang_elems, &ntc)) != AGP_OK) return st;
  const long long tiles = lower_tiles(n);
  if (tiles * CT_THREADS > (long long)UINT_MAX || out_elems < n_slots || out_elems < 1 || partial_elems < tiles * GRAD_GROUP)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  FeatView X = dx.v;
  X.meas = x->is_measurement;
  DevBuf<double> d_C, d_alpha, d_u, d_tang, d_out, d_partial;
  if ((st = upload_doubles(ctx, d_C, C, c_elems)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_alpha, alpha, n)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_u, u, n)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_tang, tangents, ntc > 0 ? tang_elems : 0)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_out, out, out_elems)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_partial, partial, partial_elems)) != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());  // (the null-stream copies above do not order with the context's stream)
  hipStream_t s = ctx->stream;
  for (int g0 = 0; g0 < n_slots; g0 += GRAD_GROUP) {
    ContractArgs ca;
    ca.C = d_C.p; ca.ldc = ldc; ca.alpha = d_alpha.p; ca.u = d_u.p; ca.partial = d_partial.p;
    bool scaling[GRAD_GROUP];
    const int cnt = fill_slot_group(k, n_slots, slots, g0, ca.slots, scaling);
    for (int j = 0; j < GRAD_GROUP; ++j) ca.tang[j] = scaling[j] ? d_tang.p + (size_t)ca.slots.param[j] * (size_t)ldt : nullptr;
    if (loo) launch_contract<true>(s, dprog, X, ca, tiles);
    else launch_contract<false>(s, dprog, X, ca, tiles);
    launch_grad_reduce(s, d_partial.p, tiles, cnt, scale, d_out.p + g0);
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(out, d_out.p, sizeof(double) * (size_t)out_elems, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(partial, d_partial.p, sizeof(double) * (size_t)partial_elems, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// nll_grad_contract_batched_kernel<DIMP, LOO> + nll_grad_reduce_batched_kernel on descriptors that fill_contract_desc
// builds: `count` problems, each with its own program, features (of any n_b <= n_pad and any dimension), slot table, tangent
// columns and weight operands (arrays of `count` pointers and lengths as in agp_debug_contract_dense); the grid is that of a
// batch padded to n_pad rows.  out[b * ldo + slot]; partial: [problem][slot group][tile][GRAD_GROUP] with
// ceil(max n_slots / GRAD_GROUP) slot groups and lower_tiles(n_pad) tiles.
AGP_DEBUG_API int agp_debug_contract_batched(agp_context *ctx, int count, const agp_kernel *const *kernels,
                                             const agp_features *const *features, const int *n_slots,
                                             const agp_gradient_slot *const *slots, const double *const *tangents, const int64_t *ldt,
                                             const int64_t *tang_elems, int loo, const double *const *C, const int64_t *ldc,
                                             const int64_t *c_elems, const double *const *alpha, const double *const *u, int64_t n_pad,
                                             double scale, double *out, int64_t ldo, int64_t out_elems, double *partial,
                                             int64_t partial_elems) {
  if (!ctx || count <= 0 || count > 65535 || !kernels || !features || !n_slots || !slots || !tangents || !ldt || !tang_elems || !C ||
      !ldc || !c_elems || !alpha || !u || !out || !partial || n_pad <= 0)
    return AGP_ERR_INVALID_ARGUMENT;
  int st, max_slots = 0, dim_max = 1;
  std::vector<int> ntc((size_t)count, 0);
  for (int b = 0; b < count; ++b) {
    if (!kernels[b] || !features[b] || !C[b] || !alpha[b] || !u[b]) return AGP_ERR_INVALID_ARGUMENT;
    if ((st = validate_features(features[b])) != AGP_OK) return st;
    const long long nb = features[b]->n;
    if (nb <= 0 || nb > n_pad || !matrix_fits(nb, nb, ldc[b], c_elems[b])) return AGP_ERR_INVALID_ARGUMENT;
    if ((st = check_probe_slots(kernels[b], n_slots[b], slots[b], nb, tangents[b], ldt[b], tang_elems[b], &ntc[(size_t)b])) != AGP_OK)
      return st;
    if (n_slots[b] > max_slots) max_slots = n_slots[b];
    if (features[b]->dim > dim_max) dim_max = features[b]->dim;
  }
  const long long tiles = lower_tiles(n_pad);
  const int groups = (max_slots + GRAD_GROUP - 1) / GRAD_GROUP;
  const long long part_per = (long long)groups * tiles * GRAD_GROUP;
  if (tiles * CT_THREADS > (long long)UINT_MAX || tiles * count > (long long)UINT_MAX || ldo < max_slots || ldo < 1 ||
      out_elems < ldo * (count - 1) + (max_slots > 0 ? max_slots : 1) || partial_elems < part_per * count || partial_elems < 1)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<DeviceFeatures> dx((size_t)count);
  std::vector<DevBuf<double>> d_C((size_t)count), d_alpha((size_t)count), d_u((size_t)count), d_tang((size_t)count);
  DevBuf<double> d_out, d_partial;
  DevBuf<ContractDesc> d_desc;
  if ((st = upload_doubles(ctx, d_out, out, out_elems)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_partial, partial, partial_elems)) != AGP_OK) return st;
  std::vector<ContractDesc> desc((size_t)count);
  for (int b = 0; b < count; ++b) {
    const size_t i = (size_t)b;
    const long long nb = features[b]->n;
    if ((st = to_device(ctx, features[b], false, &dx[i])) != AGP_OK) return st;
    if ((st = upload_doubles(ctx, d_C[i], C[b], c_elems[b])) != AGP_OK) return st;
    if ((st = upload_doubles(ctx, d_alpha[i], alpha[b], nb)) != AGP_OK) return st;
    if ((st = upload_doubles(ctx, d_u[i], u[b], nb)) != AGP_OK) return st;
    if ((st = upload_doubles(ctx, d_tang[i], tangents[b], ntc[i] > 0 ? tang_elems[b] : 0)) != AGP_OK) return st;
    FeatView X = dx[i].v;
    X.meas = features[b]->is_measurement;
    fill_contract_desc(desc[i], kernels[b], X, d_C[i].p, ldc[b], d_alpha[i].p, d_u[i].p, d_partial.p + (size_t)b * (size_t)part_per,
                       n_slots[b], n_slots[b] > 0 ? slots[b] : nullptr, d_tang[i].p, ldt[b]);
  }
  AGP_HIP_CHECK(ctx, d_desc.alloc((size_t)count));
  AGP_HIP_CHECK(ctx, hipMemcpy(d_desc.p, desc.data(), sizeof(ContractDesc) * (size_t)count, hipMemcpyHostToDevice));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  hipStream_t s = ctx->stream;
  if (groups > 0) {
    if (loo) launch_contract_batched<true>(s, dim_max, d_desc.p, tiles, count, groups);
    else launch_contract_batched<false>(s, dim_max, d_desc.p, tiles, count, groups);
    launch_grad_reduce_batched(s, d_desc.p, tiles, count, groups, scale, d_out.p, ldo);
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(out, d_out.p, sizeof(double) * (size_t)out_elems, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(partial, d_partial.p, sizeof(double) * (size_t)partial_elems, hipMemcpyDeviceToHost));
  return AGP_OK;
}

// sparse_contract_kernel<DIMP> in one of its three modes, GRAD_GROUP slots per pass as agp_sparse_nll_gradient runs them.
//   mode 0: rows = r, columns = c (same dimension), W: r->n x c->n at ldw, tang_r / tang_c the tangent columns at either set
//   mode 1: c = nullptr (the columns are the very view of the rows), W: n x n at ldw, lower triangle
//   mode 2: c = nullptr, G groups of the points off[g] .. off[g + 1] (off[0] >= 0, off[G] <= n, no empty group), slab g at
//           W + woff[g] with leading dimension wld[g] >= its size, inside the w_elems doubles of W; ldw is not read
// In modes 1 and 2 tang_c = nullptr hands the kernel tang_r for both sides.
// out[slot]: the sum of that contraction's partials (nll_grad_reduce_kernel at scale 1).  combo[slot]: what
// sparse_grad_reduce_kernel forms from three partial sets, this contraction's at position `which` (0, 1, 2) and the caller's
// other_a (tiles_a x GRAD_GROUP) and other_b (tiles_b x GRAD_GROUP) at the two remaining positions in that order; they are
// the same for every slot group.  partial: at least tiles * GRAD_GROUP doubles, comes back holding the last slot group's.
AGP_DEBUG_API int agp_debug_contract_sparse(agp_context *ctx, const agp_kernel *k, const agp_features *r, const agp_features *c, int mode,
                                            int n_slots, const agp_gradient_slot *slots, const double *tang_r, int64_t ldtr,
                                            int64_t tr_elems, const double *tang_c, int64_t ldtc, int64_t tc_elems, const double *W,
                                            int64_t ldw, int64_t w_elems, int64_t G, const int64_t *off, const int64_t *woff,
                                            const int64_t *wld, int which, const double *other_a, int64_t tiles_a, const double *other_b,
                                            int64_t tiles_b, double *out, int64_t out_elems, double *combo, int64_t combo_elems,
                                            double *partial, int64_t partial_elems) {
  if (!ctx || !k || !r || !W || !out || !combo || !partial || mode < 0 || mode > 2 || which < 0 || which > 2 || tiles_a < 0 ||
      tiles_b < 0 || (tiles_a > 0 && !other_a) || (tiles_b > 0 && !other_b) || w_elems <= 0)
    return AGP_ERR_INVALID_ARGUMENT;
  if ((mode == 0) != (c != nullptr)) return AGP_ERR_INVALID_ARGUMENT;
  int st = validate_features(r);
  if (st != AGP_OK) return st;
  if (c && (st = validate_features(c)) != AGP_OK) return st;
  if (c && c->dim != r->dim) return AGP_ERR_INVALID_ARGUMENT;
  const long long rows = r->n, cols = c ? c->n : r->n;
  if (rows <= 0 || cols <= 0) return AGP_ERR_INVALID_ARGUMENT;
  int ntc = 0, ntc_c = 0;
  if ((st = check_probe_slots(k, n_slots, slots, rows, tang_r, ldtr, tr_elems, &ntc)) != AGP_OK) return st;
  const bool own_tc = c != nullptr || tang_c != nullptr;
  if (own_tc && (st = check_probe_slots(k, n_slots, slots, cols, tang_c, ldtc, tc_elems, &ntc_c)) != AGP_OK) return st;
  long long tiles = 0, tiles_r = 0;
  std::vector<long long> tab;  // off | woff | wld | tstart, G + 1 entries each
  if (mode == 0) {
    if (!matrix_fits(rows, cols, ldw, w_elems)) return AGP_ERR_INVALID_ARGUMENT;
    tiles_r = (rows + CT - 1) / CT;
    tiles = tiles_r * ((cols + CT - 1) / CT);
  } else if (mode == 1) {
    if (!matrix_fits(rows, rows, ldw, w_elems)) return AGP_ERR_INVALID_ARGUMENT;
    tiles = lower_tiles(rows);
  } else {
    if (G <= 0 || !off || !woff || !wld || off[0] < 0 || off[G] > rows) return AGP_ERR_INVALID_ARGUMENT;
    tab.assign(4 * (size_t)(G + 1), 0);
    for (long long g = 0; g <= G; ++g) tab[(size_t)g] = off[g];
    for (long long g = 0; g < G; ++g) {
      const long long sg = off[g + 1] - off[g];
      if (sg <= 0 || woff[g] < 0 || !matrix_fits(sg, sg, wld[g], w_elems - woff[g])) return AGP_ERR_INVALID_ARGUMENT;
      tab[(size_t)(G + 1 + g)] = woff[g];
      tab[(size_t)(2 * (G + 1) + g)] = wld[g];
      tab[(size_t)(3 * (G + 1) + g)] = tiles;
      tiles += lower_tiles(sg);
    }
    tab[(size_t)(3 * (G + 1) + G)] = tiles;
  }
  if (tiles * CT_THREADS > (long long)UINT_MAX || out_elems < n_slots || out_elems < 1 || combo_elems < n_slots || combo_elems < 1 ||
      partial_elems < tiles * GRAD_GROUP)
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dr, dc;
  if ((st = to_device(ctx, r, false, &dr)) != AGP_OK) return st;
  if (c && (st = to_device(ctx, c, false, &dc)) != AGP_OK) return st;
  FeatView R = dr.v;
  R.meas = r->is_measurement;
  FeatView Cv = c ? dc.v : R;
  if (c) Cv.meas = c->is_measurement;
  DevBuf<double> d_W, d_tr, d_tc, d_a, d_b, d_out, d_combo, d_partial;
  DevBuf<long long> d_tab;
  if ((st = upload_doubles(ctx, d_W, W, w_elems)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_tr, tang_r, ntc > 0 ? tr_elems : 0)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_tc, tang_c, own_tc && ntc_c > 0 ? tc_elems : 0)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_a, other_a, tiles_a * GRAD_GROUP)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_b, other_b, tiles_b * GRAD_GROUP)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_out, out, out_elems)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_combo, combo, combo_elems)) != AGP_OK) return st;
  if ((st = upload_doubles(ctx, d_partial, partial, partial_elems)) != AGP_OK) return st;
  if (mode == 2) {
    AGP_HIP_CHECK(ctx, d_tab.alloc(tab.size()));
    AGP_HIP_CHECK(ctx, hipMemcpy(d_tab.p, tab.data(), sizeof(long long) * tab.size(), hipMemcpyHostToDevice));
  }
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  hipStream_t s = ctx->stream;
  const double *sets[3];
  long long set_tiles[3];
  for (int q = 0, o = 0; q < 3; ++q) {
    if (q == which) { sets[q] = d_partial.p; set_tiles[q] = tiles; }
    else { sets[q] = o == 0 ? d_a.p : d_b.p; set_tiles[q] = o == 0 ? tiles_a : tiles_b; ++o; }
  }
  for (int g0 = 0; g0 < n_slots; g0 += GRAD_GROUP) {
    SparseContractArgs ca;
    std::memset(static_cast<void *>(&ca), 0, sizeof(ca));
    bool scaling[GRAD_GROUP];
    const int cnt = fill_slot_group(k, n_slots, slots, g0, ca.slots, scaling);
    for (int j = 0; j < GRAD_GROUP; ++j) {
      ca.tr[j] = scaling[j] ? d_tr.p + (size_t)ca.slots.param[j] * (size_t)ldtr : nullptr;
      ca.tc[j] = !own_tc ? ca.tr[j] : (scaling[j] ? d_tc.p + (size_t)ca.slots.param[j] * (size_t)ldtc : nullptr);
    }
    ca.W = d_W.p; ca.ldw = mode == 2 ? 0 : ldw; ca.tiles_r = tiles_r; ca.partial = d_partial.p; ca.mode = mode;
    if (mode == 2) {
      ca.off = d_tab.p; ca.woff = d_tab.p + (G + 1); ca.wld = d_tab.p + 2 * (G + 1); ca.tstart = d_tab.p + 3 * (G + 1);
      ca.G = G;
    }
    launch_sparse_contract(s, dprog, R, Cv, ca, tiles);
    launch_grad_reduce(s, d_partial.p, tiles, cnt, 1.0, d_out.p + g0);
    launch_sparse_grad_reduce(s, sets[0], set_tiles[0], sets[1], set_tiles[1], sets[2], set_tiles[2], cnt, d_combo.p + g0);
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpy(out, d_out.p, sizeof(double) * (size_t)out_elems, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(combo, d_combo.p, sizeof(double) * (size_t)combo_elems, hipMemcpyDeviceToHost));
  AGP_HIP_CHECK(ctx, hipMemcpy(partial, d_partial.p, sizeof(double) * (size_t)partial_elems, hipMemcpyDeviceToHost));
  return AGP_OK;
}

AGP_DEBUG_API int agp_debug_comm_create_null(int nranks, int rank, agp_comm **out) {
  if (!out || nranks < 1 || rank < 0 || rank >= nranks) return AGP_ERR_INVALID_ARGUMENT;
  NullComm *c = new (std::nothrow) NullComm();
  agp_comm *h = new (std::nothrow) agp_comm();
  if (!c || !h) { delete c; delete h; return AGP_ERR_INVALID_ARGUMENT; }
  c->world = nranks;
  c->rank = rank;
  h->impl = c;
  *out = h;
  return AGP_OK;
}

}  // extern "C"
