// chol.hip — K3: blocked right-looking LL^T on fp64 MFMA, with the forward
// substitution z = L^-1 y fused into the panel kernels.
//
// Replaces Eigen::SerializableLDLT(cov) + .solve(y)
// (include/albatross/src/eigen/serializable_ldlt.hpp:27, models/gp.hpp:67-68).
// The reference factor is a pivoted L D L^T; this one is un-pivoted L L^T —
// parity is defined on K^-1 y, log|K| and predictions.
//
// Structure (NB = 128, NBO = 512, micro block MB = 16):
//   for every outer block of NBO columns:
//     for every NB-wide diagonal block inside it:
//       potrf_diag_kernel   one workgroup: 128x128 block in LDS, 8 micro steps
//                           {register POTRF16 + INV16 | MFMA TRSM | MFMA SYRK}
//       trsm_panel_kernel   rows below: X <- X L11^-T by substitution over the
//                           micro blocks, all on MFMA; accumulators of finished
//                           micro columns are reused directly as MFMA operands
//       gemm_nt_sub (K=128) update of the rest of the outer block column
//     gemm_nt_sub (K=512)   trailing update  (the MFMA-bound bulk, gemm.hip)
// The SCHEDULE - outer block widths, merged / throttled / masked / step / single-stream steps, panel and step-launch
// shapes, every switch point - is decided in factor_plan.h (plain C++, tested without a device by
// tests/test_fit_schedule_host.py); factor_lower and panel_phase below carry it out.
#include <cstdlib>
#include "common.h"
#include "mfma_f64.h"
#include "gemm_tiles.h"
#include "trsm_kernel.h"
#include "pub.h"
#include "factor_plan.h"  // the schedule: switch points, outer steps, panel and step-launch shapes

namespace agp {
void launch_set_identity_batched(hipStream_t s, double *B, long long ld, long long stride, long long m, long long count);  // reduce.hip

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// 1/sqrt(x) to full fp64 accuracy: hardware estimate + two Newton steps
// (a short dependent chain: this sits on the serial pivot path)
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
  y = y * (1.5 - h * y * y);
  y = y * (1.5 - h * y * y);
  return y;
}

struct PotrfArgs {
  double *A;        // matrix base
  long long lda;
  long long k0;     // first row/col of the diagonal block
  int nbk;          // valid size of the block (<= NB)
  double *img;      // tile image of this diagonal block (IMG_DOUBLES doubles, see below)
  double *y;        // y + k0 or nullptr
  int *flags;
  double *scalars;
  // batched launches (blockIdx.y = batch entry): element offsets per entry; all 0 = not batched
  long long batch_A = 0, batch_img = 0, batch_y = 0, batch_scalars = 0, batch_flags = 0, batch_zpub = 0;
  // fused panel kernel only: z of this block is also PUBLISHED here (device-scope stores) for the workgroups that solve
  // the rows below in the same launch; `below` = number of those rows
  double *zpub = nullptr;
  long long below = 0;
  // fused panel kernel with the PREVIOUS panel's update folded in (panel_fused_kernel<true>): columns k0 - 128 .. k0 - 1
  // hold the factored previous panel, whose rank-128 update of THIS panel's 128 columns has not been applied yet.
  // dpub: 36 tiles (the LDS tile layout of the diagonal block) through which the workgroups that update the diagonal
  // block hand it to the one that factors it (sentinel-filled, see store_pub)
  double *dpub = nullptr;
  // panel STEP kernel (panel_fused_kernel<true> in the chain-bound tail, see panel_phase): workgroups trail_first ..
  // apply the previous panel's rank-128 update to everything RIGHT of this panel (the `below` x `below` lower triangle,
  // 64 x 64 tiles) while this panel is factored - one launch per panel, no update launch, no second stream.
  unsigned trail_first = 0xffffffffu;
  // workgroup hold_index does nothing but keep its slot until workgroup 0 is done (see panel_phase)
  unsigned hold_index = 0xffffffffu, hold_count = 0;
  // step launches: the previous panel's update of THIS panel's rows below the diagonal block is done by the first
  // 2 x ceil(below / 64) trailing workgroups (64 x 64 tiles, device-scope stores), which count themselves in
  // rowcnt[64-row block] when complete; the workgroup that solves those 64 rows waits for rowcnt_expect there and reads
  // its rows with device-scope loads.  (The counters only grow: every step launch adds two per row block.)
  unsigned long long *rowcnt = nullptr;
  unsigned long long rowcnt_expect = 0;
  long long trail_tiles = 0, trail_workers = 1;  // tiles of the launch (row tiles first) / trailing workgroups that share them
};


// DPP row broadcast on fp64 (gfx90a+ "DPP64": row_newbcast only): every lane reads lane J of its
// own 16-lane row.  One VALU instruction, no SGPR round trip (v_readlane x2 + use).  The leading
// s_nop covers the "VALU write -> DPP read" hazard (2 wait states), which the compiler cannot see
// inside inline asm.
template <int J>
__device__ __forceinline__ double bcast_row(double v) {
  double r;
  asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(J));
  return r;
}

// acc -= (lane J's value of src) * a
template <int J>
__device__ __forceinline__ void fnmac_bcast_row(double &acc, double src, double a) {
  asm("s_nop 1\n\tv_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
      : "+v"(acc) : "v"(src), "v"(a), "n"(J));
}

// ---- hand-scheduled 16 x 16 POTRF + inverse ---------------------------------------------------
// One wave issues in order, so the serial pivot chain (broadcast -> rsq -> Newton -> scale ->
// first rank-1 term) decides the run time unless the ~30 independent rank-1 terms of every column
// are slotted into its latency shadows.  The compiler does not do that for inline asm, so the
// arithmetic on the chain is volatile asm too and the issue order below is the source order:
// the terms of column C that are not needed at once ("deferred": a[j] for j > C + 1, the inverse
// sweep w[r] for r > C) are emitted between the chain steps of column C + 1.
__device__ __forceinline__ double vmul(double a, double b) {
  double r;
  asm volatile("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double vfma(double a, double b, double c) {
  double r;
  asm volatile("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ double vfnma(double a, double b, double c) {  // c - a b
  double r;
  asm volatile("v_fma_f64 %0, -%1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ double vrsq(double a) {
  double r;
  asm volatile("v_rsq_f64 %0, %1" : "=v"(r) : "v"(a));
  return r;
}
template <int J>
__device__ __forceinline__ double vbcast(double v) {
  double r;
  asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(J));
  return r;
}
// acc -= src[lane J of the row] * a.  HAZARD: src may have been written by the previous one or two
// VALU instructions (2 wait states before a DPP read); a whole issue slot, so only where needed.
template <int J, bool HAZARD>
__device__ __forceinline__ void vfnmac_bcast(double &acc, double src, double a) {
  if constexpr (HAZARD)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(src), "v"(a), "n"(J));
  else
    asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(src), "v"(a), "n"(J));
}

// deferred term I of column K (K < 0: nothing).  Order: w[K] *= inv_K, then alternately the
// a-terms j = K + 2 + i and the w-terms r = K + 1 + i.
template <int K, int I>
__device__ __forceinline__ void potrf16_deferred(double (&a)[MB], double (&w)[MB], const double (&dinv)[MB]) {
  if constexpr (K >= 0) {
    constexpr int NA = MB - 2 - K;      // a-terms: j = K + 2 .. 15
    constexpr int NW = MB - 1 - K;      // w-terms: r = K + 1 .. 15
    if constexpr (I == 0) {
      w[K] = vmul(w[K], dinv[K]);
    } else {
      constexpr int q = (I - 1) / 2;
      if constexpr (((I - 1) & 1) == 0) {
        if constexpr (q < NA) vfnmac_bcast<K + 2 + q, false>(a[K + 2 + q], a[K], a[K]);
      } else {
        if constexpr (q < NW) vfnmac_bcast<K + 1 + q, false>(w[K + 1 + q], a[K], w[K]);
      }
    }
  }
}

template <int K, int I0, int I1>
__device__ __forceinline__ void potrf16_deferred_range(double (&a)[MB], double (&w)[MB], const double (&dinv)[MB]) {
  if constexpr (I0 < I1) {
    potrf16_deferred<K, I0>(a, w, dinv);
    potrf16_deferred_range<K, I0 + 1, I1>(a, w, dinv);
  }
}

constexpr int POTRF16_DEFERRED_MAX = 1 + 2 * MB;  // indices beyond a column's last term are no-ops

template <int C>
__device__ __forceinline__ void potrf16_column(double (&a)[MB], double (&w)[MB], double (&dinv)[MB], double &diag,
                                               int ln, int pivot_base, int &bad_pivot) {
  if constexpr (C < MB) {
    const double piv = vbcast<C>(a[C]);
    potrf16_deferred_range<C - 1, 0, 3>(a, w, dinv);
    const double y0 = vrsq(piv);
    potrf16_deferred_range<C - 1, 3, 8>(a, w, dinv);
    // third-order correction of the hardware estimate: e = 1 - piv y0^2, inv = y0 (1 + e/2 + 3 e^2/8)
    const double t = vmul(y0, y0);
    potrf16_deferred_range<C - 1, 8, 10>(a, w, dinv);
    const double e = vfnma(piv, t, 1.0);
    potrf16_deferred_range<C - 1, 10, 12>(a, w, dinv);
    const double pp = vfma(0.375, e, 0.5);
    const double ye = vmul(y0, e);
    potrf16_deferred_range<C - 1, 12, 13>(a, w, dinv);
    const double inv = vfma(ye, pp, y0);
    potrf16_deferred_range<C - 1, 13, 15>(a, w, dinv);
    a[C] = vmul(a[C], inv);  // lane C now holds piv * inv ~ sqrt(piv); the exact diagonal goes to `diag`
    dinv[C] = inv;
    potrf16_deferred_range<C - 1, 15, 17>(a, w, dinv);
    if constexpr (C + 1 < MB) vfnmac_bcast<C + 1, true>(a[C + 1], a[C], a[C]);  // the term the next pivot waits for
    potrf16_deferred_range<C - 1, 17, POTRF16_DEFERRED_MAX>(a, w, dinv);
    // off the chain: pivot check and the Heron-corrected diagonal entry
    if (!(piv > 0.) && bad_pivot == 0) bad_pivot = pivot_base + C + 1;
    double sq = piv * inv;
    sq = sq + 0.5 * inv * (piv - sq * sq);
    diag = (ln == C) ? sq : diag;
    potrf16_column<C + 1>(a, w, dinv, diag, ln, pivot_base, bad_pivot);
  }
}

// POTRF16 + INV16 of one diagonal micro tile by one wave, in registers.
// Lane ln (= lane & 15) owns row ln of the tile / column ln of the inverse; the four 16-lane
// rows of the wave compute the same thing.
// `a` holds row ln of the (updated) diagonal tile.  Results: the tile of L into D (LDS), its inverse into Wout (LDS) and
// img_diag (the tile image; PUB: published, see above).
template <bool PUB = false>
__device__ __forceinline__ void micro_potrf_inv_regs(double (&a)[MB], double *D, double *Wout, double *img_diag, int lane,
                                                     int ln, int pivot_base, int &bad_pivot) {
  double w[MB], dinv[MB], diag = 0.;
#pragma unroll
  for (int r = 0; r < MB; ++r) w[r] = (ln == r) ? 1. : 0.;
  potrf16_column<0>(a, w, dinv, diag, ln, pivot_base, bad_pivot);
  potrf16_deferred_range<MB - 1, 0, POTRF16_DEFERRED_MAX>(a, w, dinv);  // last column: only w[15] *= inv
  if (lane < MB) {
#pragma unroll
    for (int c = 0; c < MB; ++c) D[c * MB + ln] = (c < ln) ? a[c] : ((c == ln) ? diag : 0.);
#pragma unroll
    for (int r = 0; r < MB; ++r) {
      Wout[ln * MB + r] = w[r];
      if constexpr (PUB) store_pub(img_diag + ln * MB + r, w[r]);
      else img_diag[ln * MB + r] = w[r];
    }
  }
}

// POTRF16 + INV16 of one diagonal micro tile by one wave, in registers.
// Lane ln (= lane & 15) owns row ln of the tile / column ln of the inverse; the four 16-lane
// rows of the wave compute the same thing.
template <bool PUB = false>
__device__ __forceinline__ void micro_potrf_inv(double *D, double *Wout, double *img_diag, int lane, int ln, int pivot_base,
                                                int &bad_pivot) {
  double a[MB];
#pragma unroll
  for (int c = 0; c < MB; ++c) a[c] = D[c * MB + ln];
  micro_potrf_inv_regs<PUB>(a, D, Wout, img_diag, lane, ln, pivot_base, bad_pivot);
}

__device__ __forceinline__ void micro_syrk_tile(double *T, int ib, int kb, int jb, int ln, int lg) {
  double *Cc = T + tile_off(ib, kb);
  const double *Xk = T + tile_off(kb, jb), *Xi = T + tile_off(ib, jb);
  v4d acc0, acc1 = v4zero();
#pragma unroll
  for (int r = 0; r < 4; ++r) acc0[r] = Cc[(lg + 4 * r) * MB + ln];
  acc0 = mfma16(-Xk[(0 + lg) * MB + ln], Xi[(0 + lg) * MB + ln], acc0);
  acc1 = mfma16(-Xk[(4 + lg) * MB + ln], Xi[(4 + lg) * MB + ln], acc1);
  acc0 = mfma16(-Xk[(8 + lg) * MB + ln], Xi[(8 + lg) * MB + ln], acc0);
  acc1 = mfma16(-Xk[(12 + lg) * MB + ln], Xi[(12 + lg) * MB + ln], acc1);
#pragma unroll
  for (int r = 0; r < 4; ++r) Cc[(lg + 4 * r) * MB + ln] = acc0[r] + acc1[r];
}

// two SYRK tiles at once (independent accumulators: the MFMA latencies overlap)
__device__ __forceinline__ void micro_syrk_tile2(double *T, int ib0, int kb0, int ib1, int kb1, int jb, int ln, int lg) {
  double *C0 = T + tile_off(ib0, kb0), *C1 = T + tile_off(ib1, kb1);
  const double *Xk0 = T + tile_off(kb0, jb), *Xi0 = T + tile_off(ib0, jb);
  const double *Xk1 = T + tile_off(kb1, jb), *Xi1 = T + tile_off(ib1, jb);
  v4d a0, a1 = v4zero(), b0, b1 = v4zero();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a0[r] = C0[(lg + 4 * r) * MB + ln];
    b0[r] = C1[(lg + 4 * r) * MB + ln];
  }
  a0 = mfma16(-Xk0[(0 + lg) * MB + ln], Xi0[(0 + lg) * MB + ln], a0);
  b0 = mfma16(-Xk1[(0 + lg) * MB + ln], Xi1[(0 + lg) * MB + ln], b0);
  a1 = mfma16(-Xk0[(4 + lg) * MB + ln], Xi0[(4 + lg) * MB + ln], a1);
  b1 = mfma16(-Xk1[(4 + lg) * MB + ln], Xi1[(4 + lg) * MB + ln], b1);
  a0 = mfma16(-Xk0[(8 + lg) * MB + ln], Xi0[(8 + lg) * MB + ln], a0);
  b0 = mfma16(-Xk1[(8 + lg) * MB + ln], Xi1[(8 + lg) * MB + ln], b0);
  a1 = mfma16(-Xk0[(12 + lg) * MB + ln], Xi0[(12 + lg) * MB + ln], a1);
  b1 = mfma16(-Xk1[(12 + lg) * MB + ln], Xi1[(12 + lg) * MB + ln], b1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    C0[(lg + 4 * r) * MB + ln] = a0[r] + a1[r];
    C1[(lg + 4 * r) * MB + ln] = b0[r] + b1[r];
  }
}

constexpr int POTRF_LDS_DOUBLES = IMG_DOUBLES + 2 * MB * MB + NB;  // tiles | two inverse buffers | y

// Cycle probe of the factoring workgroup (a -DAGP_POTRF_TIMING build only: scripts/build_variant.sh probe -DAGP_POTRF_TIMING makes one,
// scripts/probe_potrf.py reads it through agp_debug_potrf_probe).  Slots [wave][stamp]: 0 = entry, 1 = block loaded and the
// first micro tile factored, then per micro step jb = 0 .. 6 two stamps: 2 + 2 jb = this wave's own work of stage B done,
// 3 + 2 jb = behind the barrier that ends the step; the last launch on the device wins.
// Round 6 used it to time a TWO-wave version (POTRF16 chain on wave 0, INV16 + the exact diagonal on wave 3, columns
// handed over through LDS - the split round 5 proposed because ~28 instructions per column at one fp64 issue per 8 cycles
// looked issue-bound): the chain ALONE takes 280-312 cycles per column against 275 with everything on one wave - it is
// bound by the latency of its nine dependent fp64 operations, the other terms already sit in their shadows -, the inverse
// lands ~1.1 k cycles behind it and the SYRK loses a wave: N = 512 0.191 instead of 0.165 ms, N = 4096 1.58 instead of
// 1.41 (profiles/r06/ab_potrf_two_waves.txt, potrf_probe_two_waves.txt).  Not kept; the code is in the git history.
// The same probe on the one-wave body: micro steps 0 and 1 of a block wait for the SYRK waves (27 / 20 tiles over three
// waves, ~1.1 k ticks per tile), the other five for wave 0 (5.5 k ticks each); four SYRK tiles per trip instead of two
// (eight MFMA chains, 48 reads in flight) changed neither (10.4 k ticks for step 0 both ways) and cost 32 registers.
// One dependent operation less per column by folding the pivot's broadcast into `v_rsq_f64_dpp ... row_newbcast` is not
// available: the instruction assembles for gfx950 and returns garbage (scripts/microbench/rsq_dpp_probe.hip) - DPP on
// 64-bit operands works for v_mov_b64 and v_fmac_f64 here, not for the transcendental.
#ifdef AGP_POTRF_TIMING
__device__ unsigned long long g_potrf_probe[4 * 32];
#define AGP_PROBE(slot)                                                                             \
  do {                                                                                              \
    if ((threadIdx.x & 63) == 0) g_potrf_probe[(threadIdx.x >> 6) * 32 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
void read_potrf_probe(unsigned long long *out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_potrf_probe), sizeof(unsigned long long) * 4 * 32); }
#else
#define AGP_PROBE(slot) do { } while (0)
void read_potrf_probe(unsigned long long *out) { for (int i = 0; i < 4 * 32; ++i) out[i] = 0; }
#endif

// PUB: the fused panel kernel - every tile of the image goes out (store_pub) the moment it is final, z_b too
template <bool PUB, bool UPD = false>
__device__ __forceinline__ void potrf_diag_body(PotrfArgs &p, double *T) {
  double *Wc = T + IMG_DOUBLES;
  double *ys = Wc + 2 * MB * MB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, lg = lane >> 4;
  const int nbk = p.nbk;
  AGP_PROBE(0);

  double *Adiag = p.A + p.k0 * p.lda + p.k0;  // element (r, c) of the block at Adiag[c * lda + r]
  if constexpr (UPD) {
    // the block arrives UPDATED (D - X X^T, X = the previous panel's rows of this block) from the update workgroups
    // of the same launch, tile by tile in this very layout: poll until every value has appeared
    double v[NTILE];
    unsigned long long t0 = 0;
    for (int spin = 0;; ++spin) {
      bool ok = true;
#pragma unroll
      for (int t = 0; t < NTILE; ++t) v[t] = load_pub(p.dpub + t * (MB * MB) + tid);
#pragma unroll
      for (int t = 0; t < NTILE; ++t) ok = ok && !is_unpublished(v[t]);
      if (__all(ok)) break;
      if (spin == 0) t0 = __builtin_amdgcn_s_memrealtime();
      else if ((spin & 63) == 0 && poll_expired(t0, p.flags)) break;
      __builtin_amdgcn_s_sleep(2);
    }
#pragma unroll
    for (int t = 0; t < NTILE; ++t) T[t * (MB * MB) + tid] = v[t];
  } else {  // thread (r, c) of every tile; all 36 loads in flight
    const int r = tid & 15, c = tid >> 4;
    double v[NTILE];
#pragma unroll
    for (int ib = 0; ib < NMB; ++ib)
#pragma unroll
      for (int kb = 0; kb <= ib; ++kb) {
        const int gr = ib * MB + r, gc = kb * MB + c;
        double x;
        if (gr < nbk && gc < nbk) x = (gr >= gc) ? Adiag[gc * p.lda + gr] : 0.;
        else x = (gr == gc) ? 1. : 0.;  // identity padding of a partial last block
        v[ib * (ib + 1) / 2 + kb] = x;
      }
#pragma unroll
    for (int t = 0; t < NTILE; ++t) T[t * (MB * MB) + c * MB + r] = v[t];
  }
  if (tid < NB) ys[tid] = (p.y && tid < nbk) ? p.y[tid] : 0.;
  __syncthreads();

  int bad_pivot = 0;
  if (wave == 0) micro_potrf_inv<PUB>(T + tile_off(0, 0), Wc, p.img + tile_off(0, 0), lane, ln, 0, bad_pivot);
  __syncthreads();
  AGP_PROBE(1);

#pragma unroll 1
  for (int jb = 0; jb < NMB; ++jb) {
    const int o = jb * MB;
    const double *W = Wc + (jb & 1) * (MB * MB);
    // ---- stage A: micro TRSM of the tiles below, X <- X W^T, one tile per wave ----
    for (int ib = jb + 1 + wave; ib < NMB; ib += 4) {
      double *X = T + tile_off(ib, jb);
      v4d acc0 = v4zero(), acc1 = v4zero();
      acc0 = mfma16(W[(0 + lg) * MB + ln], X[(0 + lg) * MB + ln], acc0);
      acc1 = mfma16(W[(4 + lg) * MB + ln], X[(4 + lg) * MB + ln], acc1);
      acc0 = mfma16(W[(8 + lg) * MB + ln], X[(8 + lg) * MB + ln], acc0);
      acc1 = mfma16(W[(12 + lg) * MB + ln], X[(12 + lg) * MB + ln], acc1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double x = acc0[r] + acc1[r];  // final: element (ln, lg + 4 r) of tile (ib, jb) of L (the image holds -L)
        X[(lg + 4 * r) * MB + ln] = x;
        if constexpr (PUB) store_pub(p.img + tile_off(ib, jb) + (lg + 4 * r) * MB + ln, -x);
        else p.img[tile_off(ib, jb) + (lg + 4 * r) * MB + ln] = -x;
      }
    }
    // z_jb = W y_jb  (wave 3; reads precede the write in program order)
    if (wave == 3) {
      double zz = 0.;
#pragma unroll
      for (int c = 0; c < MB; ++c) zz += W[c * MB + ln] * ys[o + c];
      if (lane < MB) ys[o + ln] = zz;
    }
    __syncthreads();
    if (jb == NMB - 1) break;

    // ---- stage B: wave 0 updates the NEXT diagonal tile and factors it right
    // away (look-ahead) while waves 1-3 run the remaining SYRK tiles + y update
    if (wave == 0) {
      micro_syrk_tile(T, jb + 1, jb + 1, jb, ln, lg);
      micro_potrf_inv<PUB>(T + tile_off(jb + 1, jb + 1), Wc + ((jb + 1) & 1) * (MB * MB), p.img + tile_off(jb + 1, jb + 1),
                           lane, ln, o + MB, bad_pivot);
    } else {
      const int rem = NMB - 1 - jb;
      const int ntile = rem * (rem + 1) / 2;
      auto tile_of = [&](int tix, int &ib, int &kb) {
        int left = tix;
        kb = 0;
        while (left >= rem - kb) { left -= rem - kb; ++kb; }
        ib = jb + 1 + kb + left;
        kb = jb + 1 + kb;
      };
      // tix 0 is the diagonal tile done by wave 0; two tiles per trip: four independent MFMA chains
      int tix = wave;
      for (; tix + 3 < ntile; tix += 6) {
        int i0, k0, i1, k1;
        tile_of(tix, i0, k0);
        tile_of(tix + 3, i1, k1);
        micro_syrk_tile2(T, i0, k0, i1, k1, jb, ln, lg);
      }
      if (tix < ntile) {
        int i0, k0;
        tile_of(tix, i0, k0);
        micro_syrk_tile(T, i0, k0, jb, ln, lg);
      }
      const int row = o + MB + (tid - 64);
      if (row < NB) {
        const double *Xr = T + tile_off(row >> 4, jb) + (row & 15);
        double s = ys[row];
#pragma unroll
        for (int k = 0; k < MB; ++k) s -= Xr[k * MB] * ys[o + k];
        ys[row] = s;
      }
    }
    AGP_PROBE(2 + 2 * jb);
    __syncthreads();
    AGP_PROBE(3 + 2 * jb);
  }
  if constexpr (PUB) {  // z_b first: the workgroups below wait for it, nobody in this launch waits for the write-back of L11
    if (p.zpub && tid < nbk) store_pub(p.zpub + tid, ys[tid]);
  }

  {  // L11 back into the matrix: thread (r, c) of every tile
    const int r = tid & 15, c = tid >> 4;
#pragma unroll
    for (int ib = 0; ib < NMB; ++ib)
#pragma unroll
      for (int kb = 0; kb <= ib; ++kb) {
        const int gr = ib * MB + r, gc = kb * MB + c;
        if (gr < nbk && gc < nbk && gr >= gc) Adiag[gc * p.lda + gr] = T[(ib * (ib + 1) / 2 + kb) * (MB * MB) + c * MB + r];
      }
  }
  if (p.y && tid < nbk) p.y[tid] = ys[tid];
  // sum log L_ii of this block (log_determinant, serializable_ldlt.hpp:128-135):
  // 128 logs in parallel, fixed-order reduction
  double logsum = (tid < nbk) ? log(T[tile_off(tid >> 4, tid >> 4) + (tid & 15) * (MB + 1)]) : 0.;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) logsum += __shfl_down(logsum, off, 64);
  __syncthreads();
  if (lane == 0) ys[wave] = logsum;
  __syncthreads();
  if (tid == 0) {
    p.scalars[0] += (ys[0] + ys[1]) + (ys[2] + ys[3]);
    if (bad_pivot && p.flags[1] == 0) p.flags[1] = (int)(p.k0 + bad_pivot);
  }
}

__global__ __launch_bounds__(256) void potrf_diag_kernel(PotrfArgs p) {
  // serial panel chain: issue ahead of the bulk-update waves that share this CU
  __builtin_amdgcn_s_setprio(AGP_CHAIN_PRIO);
  {
    const long long b = blockIdx.y;
    p.A += b * p.batch_A;
    p.img += b * p.batch_img;
    if (p.y) p.y += b * p.batch_y;
    if (p.scalars) p.scalars += b * p.batch_scalars;
    if (p.flags) p.flags += b * p.batch_flags;
  }
  __shared__ double T[POTRF_LDS_DOUBLES];
  potrf_diag_body<false>(p, T);
}

// ---------------------------------------------------------------------------------------------------------------
// Fused panel kernel: ONE launch per 128-column panel instead of POTRF -> TRSM.
//   workgroup 0        factors the diagonal block (potrf_diag_body<true>) and publishes its tile image as it goes
//   workgroup 1 + i    solves rows [64 i, 64 i + 64) below the block, X <- X L11^-T (+ the fused y -= X z_b), micro
//                      column by micro column, each as soon as the row of image tiles it needs has appeared
// Row jb of the image (tiles (jb, 0 .. jb - 1)) is final after micro step jb - 1's TRSM stage of the producer, the
// inverted diagonal tile (jb, jb) after its look-ahead POTRF16: the consumers run one micro step behind the producer
// and finish ~1 us after it, instead of starting a 12-40 us kernel after a launch gap.  Consumers keep nothing in
// LDS and never synchronise: every wave reads its MFMA A-operand fragments straight from L2.
// Workgroup 0 is dispatched first (workgroups are dispatched in order), so the consumers only ever wait for a
// workgroup that is already running or will be as soon as a slot of its XCD frees up.
// ---------------------------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void poll_tiles(const double *img_row, int lane, double (&f)[NMB][4], int *flags) {
  // tiles 0 .. NT - 1 of one image row, as A-operand fragments (f[t][s] = element s * 64 + lane of tile t)
  unsigned long long t0 = 0;
  for (int spin = 0;; ++spin) {
    bool ok = true;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) f[t][s] = load_pub(img_row + t * (MB * MB) + s * 64 + lane);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) ok = ok && !is_unpublished(f[t][s]);
    if (__all(ok)) break;
    if (spin == 0) t0 = __builtin_amdgcn_s_memrealtime();
    else if ((spin & 63) == 0 && poll_expired(t0, flags)) break;
    __builtin_amdgcn_s_sleep(4);
  }
}

template <int JB>
__device__ __forceinline__ void trsm_fused_step(const PotrfArgs &p, int lane, v4d (&Y)[NMB], double *base, bool nok,
                                                int lg) {
  if constexpr (JB < NMB) {
    const double *row = p.img + (JB * (JB + 1) / 2) * (MB * MB);
    v4d pa[4] = {Y[JB], v4zero(), v4zero(), v4zero()};
    double f[NMB][4];
    if constexpr (JB > 0) {
      poll_tiles<JB>(row, lane, f, p.flags);
#pragma unroll
      for (int ib = 0; ib < JB; ++ib)
#pragma unroll
        for (int s = 0; s < 4; ++s) pa[s] = mfma16(f[ib][s], Y[ib][s], pa[s]);
    }
    const v4d acc = (pa[0] + pa[1]) + (pa[2] + pa[3]);
    poll_tiles<1>(row + JB * (MB * MB), lane, f, p.flags);  // the inverted diagonal tile: the last thing the producer emits for this row
    v4d po[4] = {v4zero(), v4zero(), v4zero(), v4zero()};
#pragma unroll
    for (int s = 0; s < 4; ++s) po[s] = mfma16(f[0][s], acc[s], po[s]);
    const v4d out = (po[0] + po[1]) + (po[2] + po[3]);
    Y[JB] = out;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = JB * MB + lg + 4 * r;
      if (nok && m < p.nbk) store_pub(base + m * p.lda, out[r]);  // (write-through: read by the next launch, see trail_tile64)
    }
    trsm_fused_step<JB + 1>(p, lane, Y, base, nok, lg);
  }
}

// UPD: one of the 36 micro tiles of the diagonal block per wave: D'(ib, kb) = D(ib, kb) - X_ib X_kb^T with
// X = the previous panel's rows of this block (128 deep: 32 MFMAs in four chains), published to p.dpub in the LDS tile
// layout of potrf_diag_body.  Nine workgroups of four waves cover the block; each finishes in ~2 us.
__device__ __forceinline__ void diag_update_body(const PotrfArgs &p, int tile) {
  const int lane = threadIdx.x & 63, ln = lane & 15, lg = lane >> 4;
  int ib = 0;
  while ((ib + 1) * (ib + 2) / 2 <= tile) ++ib;
  const int kb = tile - ib * (ib + 1) / 2;
  const double *Xd = p.A + (p.k0 - NB) * p.lda + p.k0;  // element (row r of the block, depth k) at Xd[k * lda + r]
  const double *Dd = p.A + p.k0 * p.lda + p.k0;         // element (r, c) of the block at Dd[c * lda + r]
  const int ra = kb * MB + ln, rb = ib * MB + ln;
  const bool oka = ra < p.nbk, okb = rb < p.nbk;
  v4d acc[4] = {v4zero(), v4zero(), v4zero(), v4zero()};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gr = ib * MB + ln, gc = kb * MB + lg + 4 * r;  // D/C layout: register r of lane (ln, lg) = element (row ln, column lg + 4 r)
    double x;
    if (gr < p.nbk && gc < p.nbk) x = (gr >= gc) ? Dd[gc * p.lda + gr] : 0.;
    else x = (gr == gc) ? 1. : 0.;  // identity padding of a partial last block
    acc[0][r] = x;
  }
  {
    // the whole depth (32 k-steps x 2 operands) in flight at once: one load round trip on the launch's critical path
    double av[32], bv[32];
#pragma unroll
    for (int s2 = 0; s2 < 32; ++s2) {
      const long long k = 4 * s2 + lg;
      av[s2] = oka ? Xd[k * p.lda + ra] : 0.;
      bv[s2] = okb ? Xd[k * p.lda + rb] : 0.;
    }
#pragma unroll
    for (int s2 = 0; s2 < 32; ++s2) acc[s2 & 3] = mfma16(-av[s2], bv[s2], acc[s2 & 3]);
  }
  const v4d out = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    // the strictly upper part of a diagonal tile stays zero, as the prologue of potrf_diag_body loads it
    const int gr = ib * MB + ln, gc = kb * MB + lg + 4 * r;
    store_pub(p.dpub + tile * (MB * MB) + (lg + 4 * r) * MB + ln, (gr >= gc) ? out[r] : 0.);
  }
}

template <bool UPD>
__device__ __forceinline__ void trsm_fused_body(const PotrfArgs &p, int first_block) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, lg = lane >> 4;
  const long long n0 = ((long long)(blockIdx.x - first_block) * 4 + wave) * 16;
  const bool active = n0 < p.below;
  const bool nok = active && n0 + ln < p.below;
  double *base = p.A + p.k0 * p.lda + (p.k0 + p.nbk) + (n0 + ln);  // X[n][m] at base[m * lda]
  const bool handed = UPD && p.rowcnt != nullptr;  // the rows arrive updated from the first trailing workgroups of this launch
  if (handed) {
    if (tid == 0) {
      const unsigned long long *c = p.rowcnt + (blockIdx.x - first_block);
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (int spin = 1; __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p.rowcnt_expect; ++spin) {
        if ((spin & 63) == 0 && poll_expired(t0, p.flags)) break;
        __builtin_amdgcn_s_sleep(8);
      }
      // pairs with the RELEASE of trail_tile64<true>'s count: the rows read below are ordered behind the count in the
      // memory model too (on this hardware they already are - every hand-over load is device-scope, sc1, and cannot
      // hit a stale line of the XCD-private L2 -, so the poll itself stays RELAXED and the fence costs one s_waitcnt)
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    __syncthreads();
  }
  if (!active) return;  // from here on the waves are independent: no barrier below
  v4d Y[NMB];
#pragma unroll
  for (int jb = 0; jb < NMB; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = jb * MB + lg + 4 * r;
      Y[jb][r] = (nok && m < p.nbk) ? (handed ? load_pub(base + m * p.lda) : base[m * p.lda]) : 0.;
    }
  trsm_fused_step<0>(p, lane, Y, base, nok, lg);
  if (p.y) {
    // y[n] -= sum_m X[n][m] z[m]: z_b is published when the producer has finished the whole block.  All 32 values of this
    // lane in flight at once and re-read together until none is the sentinel (one element at a time, each poll a
    // dependent L2 round trip, took 6 us - measured with scripts/diag_step.py - and was the last thing the launch waited for)
    double z[NMB][4];
    unsigned long long t0 = 0;
    for (int spin = 0;; ++spin) {
      bool ok = true;
#pragma unroll
      for (int jb = 0; jb < NMB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = jb * MB + lg + 4 * r;
          z[jb][r] = (m < p.nbk) ? load_pub(p.zpub + m) : 0.;
        }
#pragma unroll
      for (int jb = 0; jb < NMB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) ok = ok && !is_unpublished(z[jb][r]);
      if (__all(ok)) break;
      if (spin == 0) t0 = __builtin_amdgcn_s_memrealtime();
      else if ((spin & 63) == 0 && poll_expired(t0, p.flags)) break;
      __builtin_amdgcn_s_sleep(2);
    }
    double part = 0.;
#pragma unroll
    for (int jb = 0; jb < NMB; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) part += Y[jb][r] * z[jb][r];
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    if (lg == 0 && nok) p.y[p.nbk + n0 + ln] -= part;
  }
}

constexpr int UPD_BLOCKS = NTILE / 4;  // 9 workgroups x 4 waves = the 36 micro tiles of the diagonal block

// One 64 x 64 tile (lower triangle, column-major tile order) of  C[k0 + NB .., k0 + NB ..] -= X X^T,  X = rows k0 + NB ..
// of the PREVIOUS panel (columns k0 - NB .. k0 - 1, final since the previous launch).  Nothing in this launch reads or
// writes those tiles, so these workgroups never wait: they fill the chip behind the ~35 us of the panel's POTRF.
// 64 x 64 tile, depth exactly NB = 128, in TWO passes of 64: each pass brings both operand blocks (64 rows x 64 deep)
// into LDS with one round of loads per thread - the second pass's loads are in flight while the first one multiplies -
// instead of the generic body's eight 16-deep chunks (eight load / barrier round trips, which is what a workgroup
// with only two resident workgroups per CU waits for).  lds: 2 * 64 * TRP doubles.
// LDS image of one 64-deep pass: [64 k rows][64] doubles, NO padding; element (k row, col) at col ^ ((k row & 1) << 4).
// A ds_read_b64 is served in two groups of 32 lanes = two k rows x 16 consecutive columns: with a 512-byte pitch both
// rows would sit on the same half of the 256-byte bank row - the swap of the two 16-column halves in odd k rows puts
// them on opposite halves.  (The first version padded the pitch to 72 on the belief that any pitch is conflict-free for
// 16 consecutive lanes: 25 % of the step launches' LDS cycles were bank conflicts, profiles/r05/pmc_lds_n4096.txt.)
// Staging: thread t moves the row pairs 2 (t & 15) and 2 (t & 15) + 32 of k row t >> 4 (+ 16 c): sixteen lanes = 256
// contiguous bytes in memory, eight lanes of a ds_write_b128 = 128 contiguous bytes in LDS.
constexpr int TRP = ST;
__device__ __forceinline__ int trail_col(int krow, int col) { return col ^ ((krow & 1) << 4); }

__device__ __forceinline__ void trail_load_pass(const double *__restrict__ P, long long ld, long long row0, long long nrows,
                                                int k0, bool vec_ok, double (&r)[16]) {
  const int t = threadIdx.x, kk = t >> 4, seg = (t & 15) * 2;
  const long long row = row0 + seg;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double *q = P + row + (long long)(k0 + 16 * c + kk) * ld;
    if (vec_ok && row0 + ST <= nrows) {
      const double2 a = *reinterpret_cast<const double2 *>(q);
      const double2 b = *reinterpret_cast<const double2 *>(q + 32);
      r[4 * c] = a.x; r[4 * c + 1] = a.y; r[4 * c + 2] = b.x; r[4 * c + 3] = b.y;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int off = 32 * (e >> 1) + (e & 1);
        r[4 * c + e] = (row + off < nrows) ? q[off] : 0.;
      }
    }
  }
}

template <bool NEGATE>
__device__ __forceinline__ void trail_store_pass(double *__restrict__ Ls, const double (&r)[16]) {
  const int t = threadIdx.x, kk = t >> 4, seg = (t & 15) * 2;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int krow = 16 * c + kk;
    double *row = Ls + krow * TRP;
    double2 *d0 = reinterpret_cast<double2 *>(row + trail_col(krow, seg)), *d1 = reinterpret_cast<double2 *>(row + trail_col(krow, seg + 32));
    *d0 = NEGATE ? make_double2(-r[4 * c], -r[4 * c + 1]) : make_double2(r[4 * c], r[4 * c + 1]);
    *d1 = NEGATE ? make_double2(-r[4 * c + 2], -r[4 * c + 3]) : make_double2(r[4 * c + 2], r[4 * c + 3]);
  }
}

// Barrier for LDS hand-overs only: waits for this wave's LDS operations, not for its global loads and stores in flight
// (__syncthreads() drains those too: at every tile boundary the trailing workgroups waited for their C stores to be
// acknowledged before the next tile's loads could even be issued).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// K: depth of the product (a multiple of 64; the panel P is K columns wide) - passes of 64 through LDS, the next pass's
// loads in flight while this one multiplies.  WT: write-through stores (see below); false: plain stores.

template <bool PUBLISH = false, bool WT = true>
__device__ __forceinline__ void trail_tile64(double *__restrict__ Cc, const double *__restrict__ P, long long ld, long long M,
                                             long long i0, long long j0, double *lds, unsigned long long *done = nullptr,
                                             int K = NB) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, ln = lane & 15, lg = lane >> 4;
  const bool vec_ok = ((reinterpret_cast<uintptr_t>(P) & 15) == 0) && ((ld & 1) == 0);
  double *As = lds, *Bs = lds + 64 * TRP;
  double ra[16], rb[16];
  trail_load_pass(P, ld, i0, M, 0, vec_ok, ra);
  trail_load_pass(P, ld, j0, M, 0, vec_ok, rb);
  v4d acc[2][2];
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const long long row = i0 + 32 * wr + 16 * ti + ln;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long col = j0 + 32 * wc + 16 * tj + lg + 4 * r;
        acc[tj][ti][r] = (row < M && col < M) ? Cc[row + col * ld] : 0.;
      }
    }
  const int npass = K / 64;
  for (int pass = 0; pass < npass; ++pass) {
    if (pass) lds_barrier();  // the previous pass's readers are done with the buffers
    trail_store_pass<false>(As, ra);
    trail_store_pass<true>(Bs, rb);
    lds_barrier();
    if (pass + 1 < npass) {
      trail_load_pass(P, ld, i0, M, 64 * (pass + 1), vec_ok, ra);
      trail_load_pass(P, ld, j0, M, 64 * (pass + 1), vec_ok, rb);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int krow = (4 * s + lg) * TRP, swz = (lg & 1) << 4;  // (k row 4 s + lg: odd with lg)
      double fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fa[t] = Bs[krow + ((32 * wc + 16 * t + ln) ^ swz)];
        fb[t] = As[krow + ((32 * wr + 16 * t + ln) ^ swz)];
      }
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) acc[tj][ti] = mfma16(fa[tj], fb[ti], acc[tj][ti]);
    }
  }
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const long long row = i0 + 32 * wr + 16 * ti + ln;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long col = j0 + 32 * wc + 16 * tj + lg + 4 * r;
        // device-scope (write-through) stores for every tile: what a step launch writes is read by the NEXT launch, on other
        // XCDs - left dirty in this XCD's L2 it is written back at the kernel boundary, R^2 / 2 doubles at once, and the
        // next launch's first loads (the diagonal block's update, on its critical path) queue behind that
        if (row < M && col < M) {
          if (WT) store_pub(Cc + row + col * ld, acc[tj][ti][r]);
          else Cc[row + col * ld] = acc[tj][ti][r];
        }
      }
    }
  if constexpr (PUBLISH) {
    // every store of this tile acknowledged, then one count: a reader that sees the count reads final values
    // (the tile's stores are write-through already; the RELEASE on the count is what orders them before it in the
    // language's memory model too, not only on this hardware)
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(done, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ void trail_one_tile(const PotrfArgs &p, long long id, double *lds) {
  if (p.rowcnt) {
    // the first 2 x nrb tiles: this panel's own columns, rows below the diagonal block (tile column 0, then 1)
    const long long nrb = (p.below + ST - 1) / ST;
    if (id < 2 * nrb) {
      const long long bj = id / nrb, bi = id % nrb;
      // origin at (k0, k0): rows of the diagonal block = rows 0 .. 127 of the previous panel's rows from k0 on
      trail_tile64<true>(p.A + p.k0 * p.lda + p.k0, p.A + (p.k0 - NB) * p.lda + p.k0, p.lda, p.below + NB, (2 + bi) * ST, bj * ST,
                         lds, p.rowcnt + bi);
      return;
    }
    id -= 2 * nrb;
  }
  const long long t0 = p.k0 + NB;
  double *Cc = p.A + t0 * p.lda + t0;
  const double *P = p.A + (p.k0 - NB) * p.lda + t0;
  const int ntr = (int)((p.below + ST - 1) / ST);
  // (update_plan.h: lower_tile_at is this walk; calling it here renumbers the registers of the whole step kernel, so
  // the chain's kernel keeps its own copy)
  int bj = 0;
  while (id >= ntr - bj) {
    id -= ntr - bj;
    ++bj;
  }
  trail_tile64(Cc, P, p.lda, p.below, (long long)(bj + (int)id) * ST, (long long)bj * ST, lds);
}

// A trailing workgroup takes the tiles worker, worker + trail_workers, ... : no more workgroups than fit on the chip next
// to the critical ones.  (One workgroup per tile: at 4000 remaining rows the dispatcher starts and retires 2600 of them
// during the launch - 20 ns each even when they do nothing - and every start on a CU disturbs what runs there: with
// empty trailing workgroups the diagonal block reached workgroup 0 after 44 us instead of 6, scripts/diag_step.py.)
__device__ __forceinline__ void trail_update_body(const PotrfArgs &p, long long worker, double *lds) {
  for (long long id = worker; id < p.trail_tiles; id += p.trail_workers) {
    if (id != worker) lds_barrier();  // the previous tile's readers are done with lds
    trail_one_tile(p, id, lds);
  }
}

template <bool UPD>
__global__ __launch_bounds__(256, 2) void panel_fused_kernel(PotrfArgs p) {
  __shared__ double T[POTRF_LDS_DOUBLES];
  static_assert(POTRF_LDS_DOUBLES >= 2 * 64 * TRP, "the trailing-update workgroups stage their operands in T");
  if (!UPD && blockIdx.y > 0) {  // batched fused panels (factor_lower_batched): blockIdx.y = problem
    const long long b = blockIdx.y;
    p.A += b * p.batch_A;
    p.img += b * p.batch_img;
    if (p.y) p.y += b * p.batch_y;
    if (p.zpub) p.zpub += b * p.batch_zpub;
    if (p.scalars) p.scalars += b * p.batch_scalars;
    if (p.flags) p.flags += b * p.batch_flags;
  }
  if (UPD && blockIdx.x >= p.trail_first) {
    if (blockIdx.x >= p.hold_index && blockIdx.x < p.hold_index + p.hold_count) {
      // placeholder: idle in the slot next to workgroup 0 until the last tile of the image is out
      const double *last = p.img + tile_off(NMB - 1, NMB - 1) + MB * MB - 1;
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (int spin = 1; is_unpublished(load_pub(last)); ++spin) {
        if ((spin & 63) == 0 && poll_expired(t0, p.flags)) break;
        __builtin_amdgcn_s_sleep(64);
      }
      return;
    }
    trail_update_body(p, (long long)(blockIdx.x - p.trail_first) - (blockIdx.x > p.hold_index ? (long long)p.hold_count : 0), T);
    return;
  }
  __builtin_amdgcn_s_setprio(AGP_CHAIN_PRIO);
  if (blockIdx.x == 0) {
    potrf_diag_body<true, UPD>(p, T);
  } else if (UPD && blockIdx.x <= UPD_BLOCKS) {
    diag_update_body(p, (int)(blockIdx.x - 1) * 4 + (int)(threadIdx.x >> 6));
  } else {
    trsm_fused_body<UPD>(p, UPD ? 1 + UPD_BLOCKS : 1);
  }
}

// In the TRANS staging above the image is indexed t = jb(jb+1)/2 + ib with
// ib <= jb; for the transposed solve the "row block" of the stored pair is jb
// and the "column block" ib, i.e. tile (jb, ib) of L, used when solving micro
// block ib with the already-solved block jb > ib.

static void launch_potrf(hipStream_t s, double *A, long long lda, long long k0, int nbk, double *img,
                         double *y, int *flags, double *scalars) {
  PotrfArgs p;
  p.A = A; p.lda = lda; p.k0 = k0; p.nbk = nbk;
  p.img = img + (k0 / NB) * (long long)IMG_DOUBLES;
  p.y = y ? y + k0 : nullptr;
  p.flags = flags; p.scalars = scalars;
  hipLaunchKernelGGL(potrf_diag_kernel, dim3(1), dim3(256), 0, s, p);
}

// trailing update C -= P P^T (lower tiles) bracketed by a HIP-event pair when
// the caller collects per-launch timings (bench.py's roofline block)
// (kernel: of the bulk update; ldp: of P and Q, 0: lda)
static void timed_gemm(hipStream_t s, FactorTimers *timers, double *C, long long lda, const double *P,
                       const double *Q, long long M, long long N, long long K, bool bulk, BulkKernel kernel = BulkKernel::Fp64,
                       const float *P32 = nullptr, long long ld32 = 0, long long ldp = 0) {
  if (ldp == 0) ldp = lda;
  // only the bulk trailing updates' trailing_update_kernel launches (their own kernel symbol) are
  // event-timed: they run on the second stream, where an event gap is off the critical path
  if (!bulk) {
    launch_gemm_nt_sub(s, C, lda, P, ldp, false, Q, ldp, false, M, N, K, true);
    return;
  }
  BulkTiming bt;
  const bool timed = timers && timers->ev && timers->used + 2 <= timers->n_ev;
  if (timed) { bt.e0 = timers->ev[timers->used]; bt.e1 = timers->ev[timers->used + 1]; }
  launch_trailing_update_as(kernel, s, C, lda, P, Q, ldp, M, K, timed ? &bt : nullptr, P32, P32, ld32);
  if (timed && bt.flops > 0.) {
    timers->flops[timers->used / 2] = bt.flops;  // algorithmic flop: 2 K per covered C entry on or below the diagonal
    timers->used += 2;
  }
}

static_assert(PLAN_NB == NB && STEP_FIXED_CRITICAL == 1 + UPD_BLOCKS && MERGED_STEPS_MAX == agp_context::HEADCNT_WORDS, "factor_plan.h");
using ScheduleRecord = agp_context::ScheduleRecord;
static_assert(STEP_BIT_MERGED == ScheduleRecord::MERGED && STEP_BIT_STEP == ScheduleRecord::STEP && STEP_BIT_THROTTLED == ScheduleRecord::THROTTLED &&
              STEP_BIT_MASKED == ScheduleRecord::MASKED && STEP_BIT_SINGLE == ScheduleRecord::SINGLE && INV_BIT_EARLY == ScheduleRecord::INV_EARLY &&
              INV_BIT_LAST_STEP == ScheduleRecord::INV_LAST_STEP && INV_BIT_TAIL == ScheduleRecord::INV_TAIL, "factor_plan.h");

// Workgroup slots of panel_fused_kernel<true> on this device: occupancy x CUs, asked of the runtime once per context.
static long long step_slots(agp_context *ctx) {
  if (ctx->step_slots <= 0) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, panel_fused_kernel<true>, 256, 0) != hipSuccess || per_cu <= 0) {
      (void)hipGetLastError();
      per_cu = 1;
    }
    ctx->step_slots = (long long)per_cu * ctx->cus;
  }
  return ctx->step_slots;
}

__global__ __launch_bounds__(256) void prep_kernel(PrepArgs a) {
  int e = 0;
  while (e + 1 < a.n && (long long)blockIdx.x >= a.first_block[e + 1]) ++e;
  const long long i0 = ((long long)blockIdx.x - a.first_block[e]) * 1024 + threadIdx.x;
  unsigned long long *d = a.dst[e];
  const unsigned long long *sr = a.src[e];
  const unsigned long long pat = a.pattern[e];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = i0 + 256 * u;
    if (i < a.count[e]) d[i] = sr ? sr[i] : pat;
  }
}

__global__ __launch_bounds__(256) void copy_table_kernel(const CopyItem *__restrict__ table) {
  const CopyItem it = table[blockIdx.y];
  const long long i0 = (long long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = i0 + 256 * u;
    if (i < it.words) it.dst[i] = it.src[i];
  }
}

void launch_copy_table(hipStream_t s, const CopyItem *table_dev, long long count, long long max_words) {
  if (count <= 0 || max_words <= 0) return;
  hipLaunchKernelGGL(copy_table_kernel, dim3((unsigned)((max_words + 1023) / 1024), (unsigned)count), dim3(256), 0, s, table_dev);
}

void launch_prep(hipStream_t s, const PrepArgs &a) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(prep_kernel, dim3((unsigned)a.first_block[a.n]), dim3(256), 0, s, a);
}

// Before the fused panel kernels of one factorisation run: the tile images of the diagonal blocks [k_begin, k_end) and
// the z slots of those rows are sentinel-filled (and, for step launches, the second image and the row counters).
// panel_fused_plan makes sure the buffers exist and APPENDS the fills to `prep`, which the caller launches (stream-ordered
// before the first panel launch) together with whatever else it has to fill or copy; panel_fused_prepare is plan + launch.
// Not planned (and the two-launch path is used) if the fused kernel is off or a buffer cannot be allocated.  What was
// planned is the value returned (factor_plan.h: FusedPrep) - for the one factorisation that runs behind these fills.
FusedPrep panel_fused_plan(agp_context *ctx, double *invd, long long k_begin, long long k_end, bool want_step, PrepArgs *prep) {
  FusedPrep planned;  // (headcnt: set below, only together with the fill that zeroes the counters)
  if (!ctx->tune.panel_fused || k_end <= k_begin) return planned;
  if (ctx->zpub_cap < k_end) {
    // grow; the old buffer may still be read by kernels in flight on this context's streams: drain them first
    (void)hipStreamSynchronize(ctx->stream);
    const long long cap = (k_end + 4095) / 4096 * 4096;
    ctx->zpub_cap = ctx->d_zpub.reserve(sizeof(double) * (size_t)cap) == 0 ? cap : 0;
    if (!ctx->zpub_cap) { (void)hipGetLastError(); return planned; }
  }
  const long long b0 = k_begin / NB, b1 = (k_end + NB - 1) / NB;
  if (want_step && ctx->tune.step_below > 0 && ctx->dpub_cap < b1) {
    (void)hipStreamSynchronize(ctx->stream);
    const long long cap = (b1 + 31) / 32 * 32;
    // (+ two 64-row counters per diagonal block behind the images: the hand-over of the step launches' row updates)
    ctx->dpub_cap = ctx->d_dpub.reserve(sizeof(double) * (size_t)cap * (IMG_DOUBLES + 2)) == 0 ? cap : 0;
    ctx->d_rowcnt = ctx->dpub_cap ? reinterpret_cast<unsigned long long *>(ctx->d_dpub + cap * (long long)IMG_DOUBLES) : nullptr;
    if (!ctx->dpub_cap) (void)hipGetLastError();
  }
  const long long cnt_img = (b1 - b0) * (long long)IMG_DOUBLES, cnt_z = k_end - k_begin;
  if (ctx->d_dpub && ctx->dpub_cap >= b1) {
    prep->fill(ctx->d_rowcnt + 2 * b0, 0ull, 2 * (b1 - b0));
    prep->sentinel(ctx->d_dpub + b0 * (long long)IMG_DOUBLES, cnt_img);
  }
  prep->sentinel(invd + b0 * (long long)IMG_DOUBLES, cnt_img);
  prep->sentinel(ctx->d_zpub + k_begin, cnt_z);
  // (the counters of the merged bulk updates: factor_lower of a whole matrix large enough to have any)
  if (want_step && k_begin == 0 && ctx->d_headcnt && ctx->tune.merge_above > 0 && k_end > ctx->tune.merge_above && !prep->full()) {
    prep->fill(ctx->d_headcnt, 0ull, agp_context::HEADCNT_WORDS);
    planned.headcnt = true;
  }
  planned.img = invd;
  planned.upto = k_end;
  return planned;
}

// plan + launch: the token of what has been launched
FusedPrep panel_fused_prepare(agp_context *ctx, hipStream_t s, double *invd, long long k_begin, long long k_end, bool want_step) {
  PrepArgs prep;
  const FusedPrep planned = panel_fused_plan(ctx, invd, k_begin, k_end, want_step, &prep);
  if (planned.img) launch_prep(s, prep);
  return planned;
}

// What the schedule reads (factor_plan.h: FactorSwitches) - once per factorisation: the tuning and the buffers of the
// context, and what is particular to this call - the request, the products it resolved to, and the fills `prep` made for the
// columns [.., upto) of the tile images `invd`.
static FactorSwitches factor_switches(agp_context *ctx, const FactorRequest &req, BulkProducts products, const FusedPrep &prep,
                                      const double *invd, long long upto) {
  FactorSwitches sw;
  sw.panel_fused = ctx->tune.panel_fused; sw.step_below = ctx->tune.step_below; sw.merge_above = ctx->tune.merge_above;
  sw.step_slots = sw.step_below > 0 ? step_slots(ctx) : 0;
  sw.cus = ctx->cus;
  sw.have_masked_stream = ctx->stream_masked != nullptr;
  apply_request(sw, req, products, prep, invd, upto, ctx->tune.fp64_nbo, ctx->ev_inv && ctx->stream2);
  sw.fused_buffers_ready = sw.fused_buffers_ready && ctx->d_zpub;
  sw.step_buffers_ready = sw.panel_fused && sw.fused_buffers_ready && ctx->d_dpub && ctx->dpub_cap * NB >= upto && ctx->d_rowcnt;
  return sw;
}

// Panel phase of one outer block [K0, kend): for every NB-wide diagonal block
// POTRF, panel TRSM (with the fused forward substitution on y) and the update
// of the remaining columns of the outer block.  Everything on stream s.
static void panel_phase(agp_context *ctx, hipStream_t s, double *A, long long n, long long lda, double *invd,
                        double *y, long long K0, long long kend, FactorTimers *timers, const FactorSwitches &sw,
                        bool want_step = false, long long mark_after = -1, hipEvent_t mark_event = nullptr) {
  // step_mode (the chain-bound tail, factor_lower): ONE launch per panel.  The first panel is a plain fused launch;
  // every later one is panel_fused_kernel<true> - the previous panel's update of this panel's 128 columns on the
  // critical workgroups - plus trailing workgroups that apply the previous panel to everything further right while
  // this panel's POTRF runs.  No update launches, nothing leaves stream s.  (inner_left, fused: factor_plan.h)
  const PanelPlan pp = plan_panels(n, K0, kend, want_step, sw);
  const bool step_mode = pp.step_mode, inner_left = pp.inner_left, fused = pp.fused;
  for (long long k = K0; k < kend; k += NB) {
    const int nbk = (int)((n - k < NB) ? n - k : NB);
    if (mark_event && k == mark_after + NB) (void)hipEventRecord(mark_event, s);  // everything up to panel mark_after is enqueued
    if (inner_left && k > K0) {
      const double *P = A + K0 * lda + k;  // rows k.., columns K0..k
      timed_gemm(s, timers, A + k * lda + k, lda, P, P, n - k, nbk, k - K0, false);
    }
    const long long below = n - (k + nbk);
    if (fused) {
      PotrfArgs pa;
      pa.A = A; pa.lda = lda; pa.k0 = k; pa.nbk = nbk;
      pa.img = invd + (k / NB) * (long long)IMG_DOUBLES;
      pa.y = y ? y + k : nullptr;
      pa.flags = ctx->d_flags; pa.scalars = ctx->d_scalars;
      pa.zpub = y ? ctx->d_zpub + k : nullptr;
      pa.below = below > 0 ? below : 0;
      if (step_mode && k > K0) {
        // the panel before this one (columns k - 128 .. k - 1) has not been applied to these columns - nor to anything
        // right of them - yet
        pa.dpub = ctx->d_dpub + (k / NB) * (long long)IMG_DOUBLES;
        const StepLaunchShape sh = step_launch_shape(pa.below, (k - K0) / NB, sw.step_slots, sw.cus);  // (factor_plan.h: who goes where)
        pa.trail_first = sh.trail_first; pa.trail_tiles = sh.trail_tiles; pa.trail_workers = sh.trail_workers;
        pa.hold_index = sh.hold_index; pa.hold_count = sh.hold_count;
        pa.rowcnt_expect = sh.rowcnt_expect;
        if (pa.below > 0) pa.rowcnt = ctx->d_rowcnt + (k + NB) / 64;
        hipLaunchKernelGGL(panel_fused_kernel<true>, dim3(sh.grid), dim3(256), 0, s, pa);
        ++ctx->sched.panels_step;
      } else {
        hipLaunchKernelGGL(panel_fused_kernel<false>, dim3((unsigned)(1 + (pa.below + 63) / 64)), dim3(256), 0, s, pa);
        ++ctx->sched.panels_fused;
      }
      if (below <= 0) continue;
    } else {
      launch_potrf(s, A, lda, k, nbk, invd, y, ctx->d_flags, ctx->d_scalars);
      ++ctx->sched.panels_split;
      if (below <= 0) continue;
      TrsmArgs t;
      t.img = invd + (k / NB) * (long long)IMG_DOUBLES;
      t.nbk = nbk;
      t.Y = A + k * lda + (k + nbk);
      t.stride_m = lda; t.stride_n = 1;
      t.ncols = below;
      t.z = y ? y + k : nullptr;
      t.yrest = y ? y + k + nbk : nullptr;
      t.batch_img = t.batch_Y = 0; t.n_total = 0;
      const unsigned grid = (unsigned)((below + 63) / 64);
      if (y) hipLaunchKernelGGL((trsm_micro_kernel<false, true>), dim3(grid), dim3(256), 0, s, t);
      else hipLaunchKernelGGL((trsm_micro_kernel<false, false>), dim3(grid), dim3(256), 0, s, t);
    }
    const long long width = kend - (k + nbk);
    if (width > 0 && !inner_left && !(step_mode && fused)) {
      const double *P = A + k * lda + (k + nbk);
      timed_gemm(s, timers, A + (k + nbk) * lda + (k + nbk), lda, P, P, below, width, nbk, false);
    }
  }
}

// The gate of a merged bulk update (factor_lower): ONE wave on the chain stream waits until the tiles of the next block
// column - the first workgroups of the bulk launch that runs on the other stream - have all counted themselves.  The
// kernels behind it on the stream (the next panel phase) then start while the rest of the bulk launch is still running;
// their start is the ACQUIRE that pairs with the tiles' RELEASE.  The wave holds no LDS and four registers; it gives up
// after 2 s like every hand-over of this library (flags[2] -> AGP_ERR_HIP, and the fit is repeated without merged launches).
__global__ __launch_bounds__(64) void head_gate_kernel(const unsigned long long *done, unsigned long long expect, int *flags) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int spin = 1; __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < expect; ++spin) {
      if ((spin & 63) == 0 && poll_expired(t0, flags)) break;
      __builtin_amdgcn_s_sleep(16);
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
  }
}

void launch_head_gate(hipStream_t s, const unsigned long long *done, unsigned long long expect, int *flags) {
  hipLaunchKernelGGL(head_gate_kernel, dim3(1), dim3(64), 0, s, done, expect, flags);
}

// Host-side wait for an event WITHOUT parking a stream at a hipStreamWaitEvent (section 8: a stream that sits at an
// unsatisfied wait slows the launches of the others).  Polls with a pause instruction between queries (the core is
// shared with the launch threads of the other ranks of a box); true only if the event completed - any error ends the
// wait and the caller skips what depended on it.
static bool host_wait_event(hipEvent_t ev) {
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return true;
    if (e != hipErrorNotReady) { (void)hipGetLastError(); return false; }
    for (int i = 0; i < 32; ++i) __builtin_ia32_pause();
  }
}

void panel_phase_public(agp_context *ctx, hipStream_t s, double *A, long long n, long long lda, double *img,
                        double *y, long long K0, long long kend) {
  // (one block column of a sharded fit, or a probe: the block's own panels as step launches - one launch per panel, no
  // update launches - while the second image and the counters, which are indexed by the GLOBAL block number, stay small)
  const long long step_below = ctx->tune.step_below;
  const bool step = kend == n && kend <= 65536 && step_fits(step_below, step_below > 0 ? step_slots(ctx) : 0, kend - K0);
  const FusedPrep prep = panel_fused_prepare(ctx, s, img, K0, kend, step);
  const FactorSwitches sw = factor_switches(ctx, FactorRequest(), BulkProducts::Fp64, prep, img, kend);  // (fp64, nothing else asked for)
  panel_phase(ctx, s, A, n, lda, img, y, K0, kend, nullptr, sw, step && sw.step_buffers_ready);
}

// X (nrows x w, ld) <- X L^-T against an ALREADY FACTORED w x w diagonal block (w <= 512) given by its lower
// triangle Lkk (leading dimension ldl) and the tile images of its 128 x 128 diagonal sub-blocks; yrows (optional)
// receives the fused forward substitution y -= X z.  The panel TRSM of the row-block-sharded fit (shard.h): every
// rank runs it on its own rows against the diagonal block the owner broadcast.  Right-looking over the sub-blocks:
// the same trsm_micro_kernel / MFMA update launches as panel_phase, minus the POTRFs.
void trsm_rows_wide(hipStream_t s, double *X, long long ld, long long nrows, long long w, const double *Lkk,
                    long long ldl, const double *img, const double *z, double *yrows) {
  if (nrows <= 0 || w <= 0) return;
  for (long long c = 0; c < w; c += NB) {
    const int nbk = (int)((w - c < NB) ? w - c : NB);
    TrsmArgs t;
    t.img = img + (c / NB) * (long long)IMG_DOUBLES;
    t.nbk = nbk;
    t.Y = X + c * ld;
    t.stride_m = ld; t.stride_n = 1;
    t.ncols = nrows;
    t.z = (z && yrows) ? z + c : nullptr;
    t.yrest = (z && yrows) ? yrows : nullptr;
    t.batch_img = t.batch_Y = 0; t.n_total = 0;
    const unsigned grid = (unsigned)((nrows + 63) / 64);
    if (t.z) hipLaunchKernelGGL((trsm_micro_kernel<false, true>), dim3(grid), dim3(256), 0, s, t);
    else hipLaunchKernelGGL((trsm_micro_kernel<false, false>), dim3(grid), dim3(256), 0, s, t);
    const long long rest = w - (c + nbk);
    if (rest > 0)  // X[:, c + nbk :] -= X[:, c : c + nbk] L[c + nbk :, c : c + nbk]^T
      launch_gemm_nt_sub(s, X + (c + nbk) * ld, ld, X + c * ld, ld, false, Lkk + (c + nbk) + c * ldl, ldl, false, nrows, rest,
                         nbk, false);
  }
}

// The wide diagonal blocks [first, first + count) of the factor (width bw), inverted into W_all (FactorRequest::inv_W)
// on the second stream for the back substitution of the fit; records ev_inv (same stream every time, so the latest
// record covers the earlier inversions too).  The caller has ordered the stream behind whatever makes those blocks
// final, and keeps count of the blocks done.
static void invert_wide_blocks(agp_context *ctx, double *W_all, long long bw, double *A, long long lda, double *invd, long long first,
                               long long count) {
  const long long img = (bw / NB) * (long long)IMG_DOUBLES;
  hipStream_t si = ctx->stream2;
  double *W = W_all + first * bw * bw;
  launch_set_identity_batched(si, W, bw, bw * bw, bw, count);
  forward_solve_mat_batched(si, A + first * bw * (lda + 1), bw * (lda + 1), bw, lda, invd + first * img, img, W, bw * bw, bw, bw,
                            /*rhs_lower=*/true, count);
  (void)hipEventRecord(ctx->ev_inv, si);
}

// Mixed precision: the low-precision copy of a step's panel, its formats and its kernels (common.h: PanelStager, StagedPanel;
// the split-plane kernels: gemm_split_planes.hip).  Everything that depends on the format is between here and record_step.
void PanelStager::reserve(agp_context *ctx, BulkProducts requested, long long n, long long nbo_wide) {
  if (requested == BulkProducts::F16x2 && ctx->f16_scales_n < n) {
    const long long cap = (n + 1) / 2 * 2;
    ctx->f16_scales_n = ctx->f16_scales.reserve(sizeof(double) * 2 * (size_t)cap) == 0 ? cap : 0;
    if (!ctx->f16_scales_n) (void)hipGetLastError();
  }
  // two panel copies of (n rows + padding) x width: fp32, or three bf16 planes (two fp16 planes fit in the same space: the
  // fall-back from fp16 to bf16 planes needs no second allocation); kept in the context
  const long long width = nbo_wide > 512 ? nbo_wide : 512;
  const size_t want = uses_planes(requested) ? 2 * split_planes_bytes(3, n, width) : sizeof(float) * 2 * ((size_t)n + 16) * (size_t)width;
  if (ctx->panel_copies.reserve(want) != 0) (void)hipGetLastError();
}

BulkProducts PanelStager::begin(agp_context *ctx, hipStream_t s, BulkProducts requested, const double *A, long long lda, long long n) {
  ctx_ = ctx;
  products_ = requested;
  rs_ = irs_ = nullptr;
  if (requested == BulkProducts::F16x2) {
    if (ctx->f16_scales && ctx->f16_scales_n >= n) {
      rs_ = ctx->f16_scales;
      irs_ = ctx->f16_scales + ctx->f16_scales_n;
      launch_f16x2_row_scales(s, A, lda, n, ctx->f16_scales, ctx->f16_scales + ctx->f16_scales_n);
    } else {
      products_ = BulkProducts::Bf16x3;
    }
  }
  return products_;
}

StagedPanel PanelStager::unstaged(const double *P, long long ldp) const {
  StagedPanel out;
  out.P_ = P; out.ldp_ = ldp;
  return out;
}

StagedPanel PanelStager::stage(hipStream_t s, const double *P, long long ldp, long long rows, long long K, long long kend) {
  StagedPanel out = unstaged(P, ldp);
  const size_t bytes = ctx_->panel_copies.bytes();
  if (!ctx_->panel_copies) return out;
  auto take = [&](auto *base) {  // (half the buffer, counted in elements of the copy's type)
    auto *dst = base + (size_t)(flip_ ? 1 : 0) * (bytes / sizeof(*base) / 2);
    flip_ = !flip_;
    return dst;
  };
  float *f32 = reinterpret_cast<float *>(ctx_->panel_copies.get());
  unsigned short *planes = reinterpret_cast<unsigned short *>(ctx_->panel_copies.get());
  const F16x2Tuning f16x2 = ctx_->tune.f16x2;
  if (products_ == BulkProducts::Fp32) {
    out.ld32_ = (rows + 7) / 8 * 8;
    if (out.ld32_ % 512 == 0) out.ld32_ += 8;
    if (sizeof(float) * (size_t)out.ld32_ * (size_t)K * 2 > bytes) return out;
    float *dst = take(f32);
    launch_convert_panel_f32(s, P, ldp, rows, K, dst, out.ld32_);
    out.P32_ = dst;
  } else if (products_ == BulkProducts::Bf16x3 && K % 32 == 0 && 2 * split_planes_bytes(3, rows, K) <= bytes) {
    unsigned short *dst = take(planes);
    launch_convert_panel_bf16x3(s, P, ldp, rows, K, dst);
    out.P16_ = dst;
  } else if (products_ == BulkProducts::F16x2 && f16x2_depth_ok(f16x2, K) && 2 * split_planes_bytes(2, rows, K) <= bytes) {
    unsigned short *dst = take(planes);
    launch_convert_panel_f16x2(s, f16x2, P, ldp, rows, K, rs_ + kend, dst);
    out.P16_ = dst;
    out.irs_ = irs_ + kend;
  }
  if (out.P16_) {
    out.products_ = products_;
    out.rows_ = rows;
    out.f16x2_ = f16x2;
    out.bf16x3_ = ctx_->tune.bf16x3;
  }
  return out;
}

void StagedPanel::apply(hipStream_t s, double *C, long long ldc, long long row_offset, long long M, long long N, long long K,
                        FactorTimers *timers) const {
  const bool bulk = M == N;
  if (P16_) {
    long long olen = 0;
    const int *order = nullptr;
    if (bulk) {
      const int ntr = tile_rows(M);
      const long long tiles = lower_tile_count(ntr, ntr, 1);
      if (mixed_bulk_ordered(tiles)) order = bulk_tile_order(ntr, tiles, &olen);
    }
    if (products_ == BulkProducts::F16x2)
      launch_update_f16x2(s, f16x2_, C, ldc, P16_, rows_, row_offset, row_offset, irs_, M, N, K, order, olen);
    else
      launch_update_bf16x3(s, bf16x3_, C, ldc, P16_, rows_, row_offset, row_offset, M, N, K, order, olen);
    return;
  }
  // products of fp32-rounded panels on the fp32 MFMA path, fp64 subtraction: from the fp32 copy, or rounded by the kernel
  const double *Q = P_ + row_offset;
  const float *Q32 = P32_ ? P32_ + row_offset : nullptr;
  if (bulk) timed_gemm(s, timers, C, ldc, Q, Q, M, N, K, true, BulkKernel::Fp32Products, Q32, ld32_, ldp_);
  else launch_update_f32(s, C, ldc, Q, Q, ldp_, M, N, K, Q32, Q32, ld32_);
}

// The one place the record is filled from the plan: a step factor_lower has carried out, and the inversions that ran.
static void record_step(ScheduleRecord &rec, const OuterStep &s, unsigned inverted) {
  rec.add_step(s.next_end, s.bits);
  rec.inv_bits |= inverted;
}

// Right-looking LL^T with one outer block of look-ahead on two streams:
//   stream  (high priority): panel phase P(j), then U1(j) = update of the
//            NEXT outer block column, then P(j + 1) ...
//   stream2: U2(j) = update of everything right of the next block column
//            (the MFMA-bound bulk), overlapping P(j + 1).
// Dependencies: U1(j), U2(j) after P(j) and after U2(j - 1).
// WHICH outer steps there are and what each does is decided by FactorPlanner (factor_plan.h); this function carries the
// steps out - streams, events, launches - and writes down what it did (ScheduleRecord).  What is particular to the call
// comes in `req` and goes out in the value returned; nothing of it is kept in the context.
FactorOutcome factor_lower(agp_context *ctx, double *A, long long n, long long lda, double *invd, double *y,
                           const FactorRequest &req) {
  hipStream_t sa = ctx->stream, sb = ctx->stream2, sb_prev = sb;
  bool have_u2 = false;
  FactorTimers *timers = req.timers;
  ctx->sched.reset_factor(n);
  // mixed precision: what the low-precision copies need of the matrix BEFORE the first panel overwrites it, and the
  // products in force
  PanelStager stager;
  const BulkProducts products = stager.begin(ctx, sa, req.products, A, lda, n);
  const bool mixed = is_mixed(products);
  // (agp_fit_create has already planned and launched the fills together with its own: req.prep.  A caller that planned
  // and got nothing leaves the planning to this call, which gets the same answer.)
  const FusedPrep prep = req.prep.covers(invd, n) ? req.prep : panel_fused_prepare(ctx, sa, invd, 0, n, true);
  const FactorSwitches sw = factor_switches(ctx, req, products, prep, invd, n);
  FactorPlanner plan(n, sw);  // (sw.bs_done == 0: no wide block is inverted yet; plan.bs_done() counts them from here)
  // The bulk stream of a step - in the end phase the CU-masked one (OuterStep::masked): a bulk update that fills every CU (the
  // 64 x 64-tile kernel takes all 160 KB of LDS) keeps the panel kernels - 75-79 KB of LDS per workgroup - out until its
  // grid has drained: POTRF took 400-500 us instead of 30 (profiles/r02), panel chain and bulk update ran one after
  // the other.  With a few CUs per XCD left free the two overlap.
  auto pick_bulk_stream = [&](const OuterStep &s) {
    sb = s.masked ? ctx->stream_masked : ctx->stream2;
    if (sb != sb_prev && have_u2) (void)hipStreamWaitEvent(sb, ctx->ev_b, 0);  // U2(j - 1) ran on the other bulk stream
    sb_prev = sb;
  };
  OuterStep s;
  while (plan.next(s)) {
    const long long kend = s.kend, next_end = s.next_end, K = kend - s.k0, rows = n - kend;
    const bool throttle = s.bits & STEP_BIT_THROTTLED, last = next_end == n;
    unsigned inverted = 0;
    if (s.inv_last_step > 0) {
      (void)hipEventRecord(ctx->ev_c, sa);  // columns < kend final
      (void)hipStreamWaitEvent(ctx->stream2, ctx->ev_c, 0);
      if (have_u2) (void)hipStreamWaitEvent(ctx->stream2, ctx->ev_b, 0);
      invert_wide_blocks(ctx, req.inv_W, req.inv_BW, A, lda, invd, 0, s.inv_last_step);
      inverted |= INV_BIT_LAST_STEP;
    }
    const double *P = A + s.k0 * lda + kend;  // panel rows kend.., columns K0..kend
    if (kend > 0) {  // (the first step has no panel to apply)
      // (mixed precision: U1 and the bulk update read ONE low-precision copy of this step's panel while it is tall)
      const StagedPanel st = s.mixed_tall ? stager.stage(sa, P, lda, rows, K, kend) : stager.unstaged(P, lda);
      (void)hipEventRecord(ctx->ev_a, sa);                       // P(j) done
      if (s.bits & STEP_BIT_MERGED) {
        // Bulk-bound phase, fp64: U1(j) and U2(j) are ONE launch on the bulk stream - the whole trailing matrix, the tiles of
        // the next block column FIRST (at the bulk kernel's efficiency: as a launch of its own on the chain stream U1 ran
        // 64 x 64 tiles at MfmaUtil 0.38 next to the bulk update, waited for U2(j - 1) through an event, and sat on the
        // critical path of P(j + 1)) and counted; the chain stream carries a one-wave gate kernel in U1's place, which lets
        // P(j + 1) start when the count is complete, ~one tile time into the launch.  The chain stream never waits for ev_b here:
        // the launch is stream-ordered behind U2(j - 1), and its head is what P(j + 1) needs.
        pick_bulk_stream(s);
        (void)hipStreamWaitEvent(sb, ctx->ev_a, 0);
        BulkTiming bt;
        const bool timed = timers && timers->ev && timers->used + 2 <= timers->n_ev;
        if (timed) { bt.e0 = timers->ev[timers->used]; bt.e1 = timers->ev[timers->used + 1]; }
        long long head_tiles = 0;
        unsigned long long *cnt = ctx->d_headcnt + s.index;
        launch_trailing_update_merged(sb, A + kend * lda + kend, lda, P, lda, rows, K, (int)((next_end - kend) / NB), cnt, &head_tiles,
                                      timed ? &bt : nullptr);
        if (timed && bt.flops > 0.) {
          timers->flops[timers->used / 2] = bt.flops;
          timers->used += 2;
        }
        (void)hipEventRecord(ctx->ev_b, sb);
        have_u2 = true;
        launch_head_gate(sa, cnt, (unsigned long long)head_tiles, ctx->d_flags);
      } else {
        // U2(j - 1) must be done before anything of step j touches the next block column
        if (have_u2) (void)hipStreamWaitEvent(sa, ctx->ev_b, 0);
        // U1: block column [kend, next_end), all rows below its diagonal
        if (s.mixed_tall) {
          // mixed precision: U1 with low-precision products like the bulk update while the block column is tall enough
          // for 128 x 128 tiles to fill the chip
          st.apply(sa, A + kend * lda + kend, lda, 0, rows, next_end - kend, K, timers);
        } else if (s.handover_whole_trailing) {
          // hand-over to the step tail: the whole trailing matrix, on the chain stream, alone on the chip - the bulk kernel
          if (mixed) st.apply(sa, A + kend * lda + kend, lda, 0, rows, rows, K, timers);
          else timed_gemm(sa, timers, A + kend * lda + kend, lda, P, P, rows, rows, K, true);
        } else {
          timed_gemm(sa, timers, A + kend * lda + kend, lda, P, P, rows, next_end - kend, K, false);
        }
        // Chain-bound phase (few rows left): a stream that sits at an UNSATISFIED hipStreamWaitEvent slows every dependent
        // launch of the other streams (measured, scripts/probe_chain.py: the panel chain takes 121 instead of 44 us per 128
        // columns while another stream waits on an event) - and here the bulk stream would wait for the panel chain all the
        // time.  So the host enqueues the next panel phase first and hands U2(j) to the bulk stream only once P(j) HAS
        // finished (hipEventQuery): the bulk stream is idle instead of blocked.  In the bulk-bound phase the host must run
        // far ahead, and the waits of the bulk stream are satisfied by the time it reaches them.
        pick_bulk_stream(s);
        if (throttle) panel_phase(ctx, sa, A, n, lda, invd, y, kend, next_end, timers, sw, s.step_mode);
        if (!last) {
          if (!throttle || !host_wait_event(ctx->ev_a)) (void)hipStreamWaitEvent(sb, ctx->ev_a, 0);
          const double *Q = A + s.k0 * lda + next_end;
          const long long M2 = n - next_end;
          if (mixed) st.apply(sb, A + next_end * lda + next_end, lda, next_end - kend, M2, M2, K, timers);
          else timed_gemm(sb, timers, A + next_end * lda + next_end, lda, Q, Q, M2, M2, K, true);
          (void)hipEventRecord(ctx->ev_b, sb);
        }
        have_u2 = !last;
      }
    }
    // P(j + 1).  With an inversion under the panels (factor_plan.h: OuterStep) the host marks the panel after which its
    // blocks are final and - the second stream must not sit at a hipStreamWaitEvent next to the chain (section 8) - hands
    // the inversion over itself once that mark has passed; the last four panels run meanwhile.
    const bool mark = s.inv_count > 0;
    if (!throttle) panel_phase(ctx, sa, A, n, lda, invd, y, kend, next_end, timers, sw, s.step_mode, s.mark_after, mark ? ctx->ev_c : nullptr);
    if (mark) {
      const bool ran = host_wait_event(ctx->ev_c);  // (otherwise bs_done stays: the substitution inverts behind the factorisation)
      if (ran) invert_wide_blocks(ctx, req.inv_W, req.inv_BW, A, lda, invd, s.inv_first, s.inv_count);
      if (ran) inverted |= s.inv_bit;
      plan.inversion_under_panels(s, ran);
    }
    record_step(ctx->sched, s, inverted);
  }
  // the panel stream ran last (its final panel depends on every update)
  return FactorOutcome{plan.bs_done()};
}

// `count` independent n x n factorisations in lock step (blockIdx.y = problem): the blocks of a sparse GP's A, the
// parameter vectors of agp_nll_batch, the fits of agp_fit_create_batch.  Problem b lives at A + b * stride_A (leading
// dimension lda), its tile images at invd + b * stride_invd, its right-hand side (optional, fused forward
// substitution) at y + b * stride_y; logsum[b] receives sum log L_ii; its flags at flags + b * stride_flags (0: shared).
// The blocking of factor_lower without its streams: outer blocks of 512 columns whose panels are left-looking (one
// product of depth <= 384 brings a panel up to date), then ONE trailing update of depth 512 for all problems - with a
// handful of problems that launch fills the chip, and the 27-30 us of a POTRF are shared by all of them.
// zpub (optional, with y): count x stride_zpub doubles; together with the tile images it must enter SENTINEL-filled - then
// every panel is ONE fused launch (panel_fused_kernel<false>, blockIdx.y = problem: the rows below are solved as the image
// appears) instead of POTRF -> TRSM.  For batches whose workgroups fit on the chip at once (batched_fused_fits): the row
// workgroups hold their slots for the whole POTRF.
bool batched_fused_fits(agp_context *ctx, long long n, long long count) {
  if (!ctx->tune.panel_fused || n <= NB) return false;
  const long long per_problem = 1 + (n - NB + 63) / 64;
  return count * per_problem <= step_slots(ctx);
}

void factor_lower_batched(hipStream_t s, double *A, long long stride_A, long long n, long long lda, double *invd,
                          long long stride_invd, double *y, long long stride_y, long long count, int *flags,
                          double *logsum, long long stride_flags, double *zpub, long long stride_zpub) {
  if (count <= 0 || n <= 0) return;
  const bool fused = zpub != nullptr && y != nullptr;
  for (long long K0 = 0; K0 < n; K0 += NBO) {
    const long long kend = (K0 + NBO < n) ? K0 + NBO : n;
    for (long long k = K0; k < kend; k += NB) {
      const int nbk = (int)((n - k < NB) ? n - k : NB);
      if (k > K0) {  // columns [k, k + nbk), rows k.. -= (rows k.. of the panels [K0, k)) (rows k..k+nbk of them)^T
        const double *P = A + K0 * lda + k;
        launch_gemm_nt_sub_batched(s, A + k * lda + k, lda, stride_A, P, lda, false, stride_A, P, lda, false, stride_A, n - k, nbk,
                                   k - K0, true, count);
      }
      PotrfArgs p;
      p.A = A; p.lda = lda; p.k0 = k; p.nbk = nbk;
      p.img = invd + (k / NB) * (long long)IMG_DOUBLES;
      p.y = y ? y + k : nullptr;
      p.flags = flags; p.scalars = logsum;
      p.batch_A = stride_A; p.batch_img = stride_invd; p.batch_y = stride_y; p.batch_scalars = 1; p.batch_flags = stride_flags;
      const long long below = n - (k + nbk);
      if (fused) {
        p.zpub = zpub + k;
        p.batch_zpub = stride_zpub;
        p.below = below > 0 ? below : 0;
        hipLaunchKernelGGL(panel_fused_kernel<false>, dim3((unsigned)(1 + (p.below + 63) / 64), (unsigned)count), dim3(256), 0, s, p);
        continue;
      }
      hipLaunchKernelGGL(potrf_diag_kernel, dim3(1, (unsigned)count), dim3(256), 0, s, p);
      if (below <= 0) continue;
      TrsmArgs t;
      t.img = p.img;
      t.nbk = nbk;
      t.Y = A + k * lda + (k + nbk);
      t.stride_m = lda; t.stride_n = 1;
      t.ncols = below;
      t.z = y ? y + k : nullptr;
      t.yrest = y ? y + k + nbk : nullptr;
      t.batch_img = stride_invd; t.batch_Y = stride_A; t.n_total = 0; t.batch_z = stride_y;
      const dim3 grid((unsigned)((below + 63) / 64), (unsigned)count);
      if (y) hipLaunchKernelGGL((trsm_micro_kernel<false, true>), grid, dim3(256), 0, s, t);
      else hipLaunchKernelGGL((trsm_micro_kernel<false, false>), grid, dim3(256), 0, s, t);
    }
    const long long rest = n - kend;
    if (rest > 0) {  // everything right of the outer block -= (its rows below) (its rows below)^T, depth kend - K0
      const double *P = A + K0 * lda + kend;
      launch_gemm_nt_sub_batched(s, A + kend * lda + kend, lda, stride_A, P, lda, false, stride_A, P, lda, false, stride_A, rest, rest,
                                 kend - K0, true, count);
    }
  }
}
// The same with the two-stream look-ahead of factor_lower (without its end-game): the panels of outer block j + 1 run on
// the context's chain stream while the trailing update of everything right of it (depth 512, all problems: the launch
// that fills the chip) runs on the bulk stream.  For batches whose updates are long enough to hide the chain behind.
void factor_lower_batched_lookahead(agp_context *ctx, double *A, long long stride_A, long long n, long long lda, double *invd,
                                    long long stride_invd, double *y, long long stride_y, long long count, int *flags,
                                    double *logsum, long long stride_flags) {
  if (count <= 0 || n <= 0) return;
  hipStream_t sa = ctx->stream, sb = ctx->stream2;
  bool have_u2 = false;
  auto panels = [&](long long K0, long long kend) {
    for (long long k = K0; k < kend; k += NB) {
      const int nbk = (int)((n - k < NB) ? n - k : NB);
      if (k > K0) {
        const double *P = A + K0 * lda + k;
        launch_gemm_nt_sub_batched(sa, A + k * lda + k, lda, stride_A, P, lda, false, stride_A, P, lda, false, stride_A, n - k, nbk,
                                   k - K0, true, count);
      }
      PotrfArgs p;
      p.A = A; p.lda = lda; p.k0 = k; p.nbk = nbk;
      p.img = invd + (k / NB) * (long long)IMG_DOUBLES;
      p.y = y ? y + k : nullptr;
      p.flags = flags; p.scalars = logsum;
      p.batch_A = stride_A; p.batch_img = stride_invd; p.batch_y = stride_y; p.batch_scalars = 1; p.batch_flags = stride_flags;
      hipLaunchKernelGGL(potrf_diag_kernel, dim3(1, (unsigned)count), dim3(256), 0, sa, p);
      const long long below = n - (k + nbk);
      if (below <= 0) continue;
      TrsmArgs t;
      t.img = p.img;
      t.nbk = nbk;
      t.Y = A + k * lda + (k + nbk);
      t.stride_m = lda; t.stride_n = 1;
      t.ncols = below;
      t.z = y ? y + k : nullptr;
      t.yrest = y ? y + k + nbk : nullptr;
      t.batch_img = stride_invd; t.batch_Y = stride_A; t.n_total = 0; t.batch_z = stride_y;
      const dim3 grid((unsigned)((below + 63) / 64), (unsigned)count);
      if (y) hipLaunchKernelGGL((trsm_micro_kernel<false, true>), grid, dim3(256), 0, sa, t);
      else hipLaunchKernelGGL((trsm_micro_kernel<false, false>), grid, dim3(256), 0, sa, t);
    }
  };
  long long K0 = 0, kend = NBO < n ? NBO : n;
  panels(K0, kend);
  while (kend < n) {
    const long long next_end = (kend + NBO < n) ? kend + NBO : n, K = kend - K0;
    (void)hipEventRecord(ctx->ev_a, sa);                        // P(j) done
    if (have_u2) (void)hipStreamWaitEvent(sa, ctx->ev_b, 0);    // U2(j - 1) wrote the next block column too
    const double *P = A + K0 * lda + kend;                      // panel rows kend.., columns K0 .. kend
    launch_gemm_nt_sub_batched(sa, A + kend * lda + kend, lda, stride_A, P, lda, false, stride_A, P, lda, false, stride_A, n - kend,
                               next_end - kend, K, true, count);  // U1: the next block column
    if (next_end < n) {
      (void)hipStreamWaitEvent(sb, ctx->ev_a, 0);
      const double *Q = A + K0 * lda + next_end;
      launch_gemm_nt_sub_batched(sb, A + next_end * lda + next_end, lda, stride_A, Q, lda, false, stride_A, Q, lda, false, stride_A,
                                 n - next_end, n - next_end, K, true, count);  // U2: everything right of it
      (void)hipEventRecord(ctx->ev_b, sb);
      have_u2 = true;
    } else {
      have_u2 = false;
    }
    panels(kend, next_end);
    K0 = kend;
    kend = next_end;
  }
}
}  // namespace agp
