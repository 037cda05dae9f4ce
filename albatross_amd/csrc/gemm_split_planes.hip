// gemm_split_planes.hip - the bulk trailing update of the MIXED-precision factorisation on the 16-bit matrix pipe, from
// SPLIT PLANES of each outer step's panel: three bf16 planes (round 5) or two fp16 planes of scaled rows (round 6, default).
//
// BASELINE config 4 ("fp32 ... MFMA f32 Gram + mixed-precision Cholesky",
// examples/temperature_example/temperature_example.cc:34-85 at N = 32768): agp_fit_create_mixed keeps the matrix, the
// panel chain and every accumulation between outer steps in fp64 and forms the K <= 512 products of one outer step at
// fp32 accuracy, with fp32 ACCUMULATION.  Rounds 1-4 did that with v_mfma_f32_16x16x4_f32 (157
// TFLOP/s peak, 103 reached).  gfx950 has no faster fp32 matrix instruction, but its 16-bit pipe is 16x that rate.
//
// bf16 x 3.  An fp32 number IS three bf16 numbers: x = hi + mid + lo with 8 significant bits each (24 = the fp32
// significand).  A product of two such numbers to fp32 accuracy needs the six partial products whose weight is above 2^-24,
//     a b ~ hi hi + (hi mid + mid hi) + (hi lo + lo hi + mid mid),
// all accumulated in the fp32 accumulators of v_mfma_f32_16x16x32_bf16: six instructions of 16 cycles for a
// 16 x 16 x 32 block = 171 flop per clock and SIMD, 419 TFLOP/s of fp32-equivalent peak against 157.
//
// fp16 x 2.  fp16 has 11 significant bits against bf16's 8, so TWO planes carry 22 bits, and the whole product of two such
// numbers,
//     a b ~ (h1 + h2)(h1 + h2) = h2 h2 + (h2 h1 + h1 h2) + h1 h1,
// is FOUR instructions of the same rate (v_mfma_f32_16x16x32_f16) against six, on two thirds of the plane traffic; every
// partial product is exact in fp32 (22 bits), so all the error is in the split (<= 2^-22 |x|) and in the fp32 accumulation.
// Three products (AGP_F16X2_TERMS=3, without h2 h2) are 3 % faster in the fit and leave the diagonal of the Schur complement
// systematically too large (sum_k h2[i, k]^2 is never subtracted): log|K| of config 4 at N = 32768 off by +0.055 against -0.017
// with four (bf16 x 3: +0.027), config 3's kernel 0.15 against 0.06 (bf16 x 3: 0.14) - four is the default.
// What fp16 lacks is RANGE (2^-24 .. 65504), so every row is scaled by a power of two first:
//     |L[i, k]| <= sqrt(A[i, i])  (sum_k L[i, k]^2 = A[i, i]),    r_i = 2^(14 - e_i),  sqrt(A[i, i]) < 2^e_i,
// the planes hold h1 = rn16(r_i x), h2 = rn16(r_i x - h1) (|r_i x| < 2^14; the residual is a normal fp16 number down to
// |r_i x| ~ 2^-2 and has an ABSOLUTE error <= 2^-25 below that, i.e. 2^-39 of the row's scale), and the epilogue undoes the
// scales exactly: C[i, j] -= (double)acc / (r_i r_j).  The diagonal is read once, before the first panel
// (launch_f16x2_row_scales); rows whose diagonal is not a positive finite number get r = 1 (the factorisation reports them).
//
//   convert_panel_bf16x3   the fp64 panel of one outer step -> three bf16 planes, ONCE for all the tiles that read it
//                          (hi = rn(x), mid = rn(x - hi), lo = rn(x - hi - mid); |x - hi - mid - lo| <= 2^-25 |x|),
//                          laid out [plane][k / 32][row][k % 32]: the 128 rows x 32 k of a tile's chunk are 8 KB
//                          contiguous per plane
//   convert_panel_f16x2    ... -> two fp16 planes [plane][k / CH][row][k % CH] of the scaled rows (CH = 32 or 64)
//   trailing_update_bf16x3_pair_kernel   128 x 128 tile of C per workgroup, 64 x 64 per wave (16 accumulators), K in
//                          chunks of 32 through ONE LDS stage (unpadded 64-B rows, the four 16-B pieces of a row
//                          permuted so that every ds_read_b128 lane group covers the 256-B bank row once), 48 KB of LDS,
//                          two workgroups per CU; C (fp64) read and written in the epilogue:
//                          C -= (double)(fp32 sum of the step's products) - the same contract as
//                          trailing_update_f32_kernel (gemm.hip), whose place it takes.
//   trailing_update_f16x2_kernel   the same tile and LDS image, 32 KB of LDS (CH = 32);
//                          the fp64 C of the tile comes in one accumulator column (16 doubles per lane) at a time, the first
//                          requested in front of the last chunk's matrix instructions, each next one before the previous is
//                          stored (+1 % on the kernel, -1 % on the fit against two columns loaded and stored in turn)
//
// Measured, bf16 x 3 (profiles/r05/time_bf16x3.txt, pmc_bulk_kernels_sq_counters.txt; N = 32768 trailing shapes,
// fp32-equivalent TFLOP/s at M = 8192 / 15872 / 30720; fp32 kernel: 87-89 / - / 105-107):
//   first version    (no longer here) one workgroup per CU, two LDS stages at an 80-B pitch, C prefetched into 128
//                    registers: 97-99 / 98 / 115-118.  PMC: the MFMA pipe busy 30 % of the time, the (single) wave per SIMD
//                    at an s_waitcnt 52 % of its cycles - 9 % of them for LDS, the rest for the global loads of the next
//                    chunk -, and HALF of the LDS cycles bank conflicts (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE).
//   pair kernel      one stage, no prefetched C, 163 registers: two workgroups per CU, one's MFMAs in the other's
//                    waits: 124-128 / 118 / 141.
//   + swizzled LDS   conflict-free reads AND writes (below), 48 KB per workgroup: 144-146 / 125-127 / 150.
// In the fit the bulk stream runs it back to back at 142 TFLOP/s (80 of the factorisation's 87 ms at N = 32768): what
// is left is the memory system - 768 KB of planes per tile, 37 % of them past the L2, plus 256 KB of fp64 C read and
// written: ~4.9 TB/s beyond the L2 at 150 TFLOP/s.  (A second register stage - the loads of chunk k + 2 in flight while
// chunk k is multiplied, 212 registers - measured 141 against 144.5 TFLOP/s on one box: it is throughput, not latency.)
// Measured, fp16 x 2 (profiles/r06/time_bf16x3.txt, time_mixed.txt; M = 15872 / 30720, K = 512): 175 / 189 TFLOP/s of
// fp32-equivalent products against 125 / 147 of the bf16 x 3 kernel; config 4 (N = 32768) 111.9 -> 94.1 ms.
#include "common.h"
#include "gemm_tiles.h"

namespace agp {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v4f32 __attribute__((ext_vector_type(4)));

namespace {
constexpr int MK = 32;                // k of one v_mfma_f32_16x16x32_f16 / _bf16
constexpr int BK = MK;                // bf16 x 3: k per chunk = one matrix instruction
constexpr int SCALE_EXP = 14;         // fp16 x 2: |r_i x| < 2^14 (fp16 overflows at 65504 ~ 2^16)
// LDS image of one plane tile: 128 rows of CH 16-bit numbers (64 or 128 B, no padding), the 16-B pieces of a row permuted so
// that every lane group of a ds_read_b128 (MI355X_MICROARCH.md, LDS: {0-3, 12-15, 20-27}, ...) covers the 256-B bank row once
// and the eight lanes of a ds_write_b128 group cover 128 contiguous bytes.  CH = 32: piece kg of row r at slot
// kg ^ ((-(r >> 2)) & 3); CH = 64: at slot kg ^ ((r >> 1) & 7) (found by enumeration).  No row PITCH does that: in a lane
// group rows 4-11 read k group lg + 1 while rows 0-3 / 12-15 read lg, and at an 80-B pitch three pairs of them share a 16-B
// slot (PMC: SQ_LDS_BANK_CONFLICT = half of SQ_LDS_IDX_ACTIVE).
template <int CH>
__device__ __forceinline__ int sw_piece(int kg, int row) {
  return CH == 32 ? (kg ^ ((4 - ((row >> 2) & 3)) & 3)) : (kg ^ ((row >> 1) & 7));
}
__device__ __forceinline__ int sw_piece(int kg, int row) { return sw_piece<BK>(kg, row); }
constexpr int SPITCH = 32;             // bf16 x 3: row pitch in bf16 (64 B, no padding)
constexpr int SPLANE = GT * SPITCH;
}  // namespace

__device__ __forceinline__ unsigned short bf16_rn(float f) {
  unsigned int u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even (finite inputs: the panel of a factorisation)
  return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf16_val(unsigned short h) { return __uint_as_float((unsigned int)h << 16); }

// planes: 3 x [K / 32][rows_pad][32] bf16; thread = (row, chunk)
__global__ __launch_bounds__(256) void convert_panel_bf16x3_kernel(const double *__restrict__ P, long long ldp, long long rows, long long rows_pad,
                                                                   unsigned short *__restrict__ planes, long long plane_stride) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long c = blockIdx.y;
  if (row >= rows_pad) return;
  unsigned short *dst = planes + c * rows_pad * BK + row * BK;
#pragma unroll
  for (int q = 0; q < BK / 8; ++q) {
    unsigned short h[8], m[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double x = row < rows ? P[row + (c * BK + 8 * q + j) * ldp] : 0.;
      h[j] = bf16_rn((float)x);
      const double r1 = x - (double)bf16_val(h[j]);
      m[j] = bf16_rn((float)r1);
      const double r2 = r1 - (double)bf16_val(m[j]);
      l[j] = bf16_rn((float)r2);
    }
    auto pack = [](const unsigned short (&v)[8]) {
      uint4 o;
      o.x = v[0] | ((unsigned int)v[1] << 16); o.y = v[2] | ((unsigned int)v[3] << 16);
      o.z = v[4] | ((unsigned int)v[5] << 16); o.w = v[6] | ((unsigned int)v[7] << 16);
      return o;
    };
    *reinterpret_cast<uint4 *>(dst + 8 * q) = pack(h);
    *reinterpret_cast<uint4 *>(dst + plane_stride + 8 * q) = pack(m);
    *reinterpret_cast<uint4 *>(dst + 2 * plane_stride + 8 * q) = pack(l);
  }
}

__global__ __launch_bounds__(256) void f16x2_row_scales_kernel(const double *__restrict__ A, long long lda, long long n, double *__restrict__ rs,
                                                               double *__restrict__ irs) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double d = A[i * (lda + 1)];
  double r = 1., ir = 1.;
  if (d > 0. && d < 1e300) {
    int e = 0;
    (void)frexp(sqrt(d), &e);  // sqrt(d) = m 2^e, 0.5 <= m < 1
    e = e < -200 ? -200 : (e > 200 ? 200 : e);
    r = ldexp(1., SCALE_EXP - e);
    ir = ldexp(1., e - SCALE_EXP);
  }
  rs[i] = r;
  irs[i] = ir;
}

void launch_f16x2_row_scales(hipStream_t s, const double *A, long long lda, long long n, double *rs, double *irs) {
  if (n <= 0) return;
  hipLaunchKernelGGL(f16x2_row_scales_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, lda, n, rs, irs);
}

// planes: 2 x [K / CH][rows_pad][CH] fp16; thread = (row, chunk)
template <int CH>
__global__ __launch_bounds__(256) void convert_panel_f16x2_kernel(const double *__restrict__ P, long long ldp, long long rows, long long rows_pad,
                                                                  const double *__restrict__ rs, unsigned short *__restrict__ planes,
                                                                  long long plane_stride) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long c = blockIdx.y;
  if (row >= rows_pad) return;
  const double r = row < rows ? rs[row] : 0.;
  unsigned short *dst = planes + c * rows_pad * CH + row * CH;
#pragma unroll
  for (int q = 0; q < CH / 8; ++q) {
    v8h h1, h2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double x = row < rows ? r * P[row + (c * CH + 8 * q + j) * ldp] : 0.;
      const _Float16 a = (_Float16)x;
      const _Float16 b = (_Float16)(x - (double)a);
      h1[j] = a;
      h2[j] = b;
    }
    *reinterpret_cast<v8h *>(dst + 8 * q) = h1;
    *reinterpret_cast<v8h *>(dst + plane_stride + 8 * q) = h2;
  }
}

static long long planes_rows_pad(long long rows) { return (rows + GT - 1) / GT * GT + GT; }  // (+ one tile of zero rows: a tile may start anywhere below `rows`)
size_t split_planes_bytes(int planes, long long rows, long long K) {
  return sizeof(unsigned short) * (size_t)planes * (size_t)planes_rows_pad(rows) * (size_t)((K + 63) / 64 * 64);
}
bool f16x2_depth_ok(F16x2Tuning tune, long long K) { return K > 0 && K % tune.chunk == 0; }

void launch_convert_panel_bf16x3(hipStream_t s, const double *P, long long ldp, long long rows, long long K, unsigned short *planes) {
  if (rows <= 0 || K <= 0 || K % BK) return;
  const long long rows_pad = planes_rows_pad(rows);
  hipLaunchKernelGGL(convert_panel_bf16x3_kernel, dim3((unsigned)((rows_pad + 255) / 256), (unsigned)(K / BK)), dim3(256), 0, s, P, ldp, rows,
                     rows_pad, planes, rows_pad * K);
}

// rs: the scales of the panel's rows (rs[0] = the scale of panel row 0).  tune.chunk fixes the layout of the planes: the
// update that reads them gets the same settings (those of the context).
void launch_convert_panel_f16x2(hipStream_t s, F16x2Tuning tune, const double *P, long long ldp, long long rows, long long K,
                                const double *rs, unsigned short *planes) {
  if (rows <= 0 || !f16x2_depth_ok(tune, K)) return;
  const long long rows_pad = planes_rows_pad(rows);
  const dim3 grid((unsigned)((rows_pad + 255) / 256), (unsigned)(K / tune.chunk));
  if (tune.chunk == 64) hipLaunchKernelGGL(convert_panel_f16x2_kernel<64>, grid, dim3(256), 0, s, P, ldp, rows, rows_pad, rs, planes, rows_pad * K);
  else hipLaunchKernelGGL(convert_panel_f16x2_kernel<32>, grid, dim3(256), 0, s, P, ldp, rows, rows_pad, rs, planes, rows_pad * K);
}

// ---- what the tile kernels of both formats share -----------------------------------------------------------------
struct PlaneArgs {
  double *C;
  long long ldc;
  const unsigned short *planes;  // of the panel both operands come from
  long long rows_pad, plane_stride;
  long long row_a, row_b;        // panel row of C's row 0 / of C's column 0
  const double *irs_a, *irs_b;   // fp16 x 2: 1 / r of C's rows / of C's columns (bf16 x 3: nullptr)
  long long M, N, K;
  int ntr, ntc;
  const int *order;              // XCD-aware tile order (gemm.hip: xcd_order) or nullptr
};

// the tile (bi, bj) of this workgroup: from the order table, or of the lower-triangular grid in column-major order; false:
// none.  The walk is update_plan.h's lower_tile_of, kept in its own words here: through the shared helper the compiler
// lays the blocks of these kernels out differently and reorders the loads, LDS reads and MFMAs of their K loops
// (profiles/r08/update_plan_resources.txt).
__device__ __forceinline__ bool plane_tile_of_block(const PlaneArgs &g, int &bi, int &bj) {
  if (g.order) {
    const int packed = g.order[blockIdx.x];
    if (packed < 0) return false;
    bi = packed >> 16;
    bj = packed & 0xffff;
    return true;
  }
  long long id = blockIdx.x;
  bj = 0;
  while (bj < g.ntc && id >= g.ntr - bj) { id -= g.ntr - bj; ++bj; }
  if (bj >= g.ntc) return false;
  bi = bj + (int)id;
  return true;
}

__device__ __forceinline__ void clear_acc(v4f32 (&acc)[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = v4f32{0.f, 0.f, 0.f, 0.f};
}

// C -= acc on a tile that reaches past M or N: entry by entry.  Register r of accumulator (tj, ti) is row rbase + 16 ti,
// column cbase_col + 16 tj + r of C (the C/D map of every non-f64 MFMA).  SCALED: ... / (r_row r_col), ir_row[ti] = 1 / r_row.
template <bool SCALED>
__device__ __forceinline__ void ragged_epilogue(const PlaneArgs &g, const v4f32 (&acc)[4][4], long long rbase, long long cbase_col,
                                                const double *ir_row) {
#pragma unroll
  for (int tj = 0; tj < 4; ++tj)
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      const long long row = rbase + 16 * ti;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long col = cbase_col + 16 * tj + r;
        if (row < g.M && col < g.N) {
          double *c = g.C + row + col * g.ldc;
          if constexpr (SCALED) *c = *c - (double)acc[tj][ti][r] * (ir_row[ti] * g.irs_b[col]);
          else *c = *c - (double)acc[tj][ti][r];
        }
      }
    }
}

// ---- bf16 x 3 ------------------------------------------------------------------------------------------------------
// staging of one K chunk: piece q (16 B) of a plane tile = row q >> 2, k group q & 3; a thread moves pieces tid and tid + 256
// of the three planes of both operands - twelve NAMED registers and macros: an array or a struct of them passed to helper
// functions stayed in scratch once the loads were pinned in front of the MFMAs
#define AGP_BF_LOAD(OFF)                                                                                   \
  do {                                                                                                     \
    const long long o0_ = (OFF) + (long long)tid * 8, o1_ = o0_ + 256 * 8;                                 \
    sa00 = *reinterpret_cast<const uint4 *>(srcA + o0_);                    sa01 = *reinterpret_cast<const uint4 *>(srcA + o1_);                    \
    sb00 = *reinterpret_cast<const uint4 *>(srcB + o0_);                    sb01 = *reinterpret_cast<const uint4 *>(srcB + o1_);                    \
    sa10 = *reinterpret_cast<const uint4 *>(srcA + g.plane_stride + o0_);     sa11 = *reinterpret_cast<const uint4 *>(srcA + g.plane_stride + o1_);     \
    sb10 = *reinterpret_cast<const uint4 *>(srcB + g.plane_stride + o0_);     sb11 = *reinterpret_cast<const uint4 *>(srcB + g.plane_stride + o1_);     \
    sa20 = *reinterpret_cast<const uint4 *>(srcA + 2 * g.plane_stride + o0_); sa21 = *reinterpret_cast<const uint4 *>(srcA + 2 * g.plane_stride + o1_); \
    sb20 = *reinterpret_cast<const uint4 *>(srcB + 2 * g.plane_stride + o0_); sb21 = *reinterpret_cast<const uint4 *>(srcB + 2 * g.plane_stride + o1_); \
  } while (0)
#define AGP_BF_STORE_P(BASE, PL)                                                                            \
  do {                                                                                                     \
    unsigned short *b_ = (BASE);                                                                           \
    *reinterpret_cast<uint4 *>(b_ + 0 * (PL) + d0) = sa00; *reinterpret_cast<uint4 *>(b_ + 0 * (PL) + d1) = sa01; \
    *reinterpret_cast<uint4 *>(b_ + 1 * (PL) + d0) = sa10; *reinterpret_cast<uint4 *>(b_ + 1 * (PL) + d1) = sa11; \
    *reinterpret_cast<uint4 *>(b_ + 2 * (PL) + d0) = sa20; *reinterpret_cast<uint4 *>(b_ + 2 * (PL) + d1) = sa21; \
    *reinterpret_cast<uint4 *>(b_ + 3 * (PL) + d0) = sb00; *reinterpret_cast<uint4 *>(b_ + 3 * (PL) + d1) = sb01; \
    *reinterpret_cast<uint4 *>(b_ + 4 * (PL) + d0) = sb10; *reinterpret_cast<uint4 *>(b_ + 4 * (PL) + d1) = sb11; \
    *reinterpret_cast<uint4 *>(b_ + 5 * (PL) + d0) = sb20; *reinterpret_cast<uint4 *>(b_ + 5 * (PL) + d1) = sb21; \
  } while (0)

// Cycle probe of the pair kernel (a -DAGP_BF16_STAMPS build only: scripts/build_variant.sh bf16_stamps -DAGP_BF16_STAMPS;
// read through agp_debug_bf16_probe by scripts/probe_bf16x3.py).  Wave 0 of the workgroup in the middle of the grid sums,
// over its K chunks, the shader cycles (s_memtime) of the four phases of a chunk - [0] barrier "stage free", [1] wait for
// the global loads + the twelve LDS stores, [2] barrier "stage full", [3] fragment reads + 96 MFMAs (+ the issue of the next
// chunk's loads) - and leaves [4] = cycles and [5] = 100 MHz ticks (s_memrealtime) of the whole loop, [6] = chunks, [7] = cycles of the epilogue (C read, subtract, write): the clock
// the chip held is 100 MHz x [4] / [5].  Every stamp sits where the kernel waits for lgkmcnt(0) anyway.
#ifdef AGP_BF16_STAMPS
__device__ unsigned long long g_bf16_probe[8];
#define AGP_BF_STAMP(var)                              \
  do {                                                 \
    __builtin_amdgcn_sched_barrier(0);                 \
    var = __builtin_amdgcn_s_memtime();                \
    __builtin_amdgcn_sched_barrier(0);                 \
  } while (0)
void read_bf16_probe(unsigned long long *out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bf16_probe), sizeof(unsigned long long) * 8); }
#else
#define AGP_BF_STAMP(var) do { } while (0)
void read_bf16_probe(unsigned long long *out) { for (int i = 0; i < 8; ++i) out[i] = 0; }
#endif

// TWO workgroups per CU: a workgroup has ONE stage (48 KB) and no prefetched C (<= 256 registers), so two of them share
// a CU and one's MFMAs run in the other's holes - the fragment reads in front of the MFMAs, the staging stores behind the
// global loads, the barrier (with ONE wave per SIMD the MFMA pipe was busy 28 % of the time, PMC); C is read and written
// in the epilogue, behind the other workgroup's loop.
__global__ __launch_bounds__(256, 2) void trailing_update_bf16x3_pair_kernel(PlaneArgs g) {
  __shared__ unsigned short lds[6 * SPLANE];  // [operand A: hi mid lo | operand B: hi mid lo][128 rows][32], 16-B pieces swizzled
  int bi, bj;
  if (!plane_tile_of_block(g, bi, bj)) return;
  const long long i0 = (long long)bi * GT, j0 = (long long)bj * GT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int ln = lane & 15, lg = lane >> 4;

  const unsigned short *srcA = g.planes + (g.row_a + i0) * BK, *srcB = g.planes + (g.row_b + j0) * BK;
  const long long chunk_stride = g.rows_pad * BK;
  uint4 sa00, sa01, sa10, sa11, sa20, sa21, sb00, sb01, sb10, sb11, sb20, sb21;
  const int d0 = (tid >> 2) * SPITCH + sw_piece(tid & 3, tid >> 2) * 8, d1 = d0 + 64 * SPITCH;  // (row + 64: the same swizzle)

  v4f32 acc[4][4];  // [tj][ti]
  clear_acc(acc);

  const long long nk = g.K / BK;
  AGP_BF_LOAD(0);
#ifdef AGP_BF16_STAMPS
  unsigned long long ph0 = 0, ph1 = 0, ph2 = 0, ph3 = 0, ta = 0, tb = 0, tc = 0, td = 0, te = 0;
  const unsigned long long loop_c0 = __builtin_amdgcn_s_memtime(), loop_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  for (long long kc = 0; kc < nk; ++kc) {
    AGP_BF_STAMP(ta);
    if (kc > 0) __syncthreads();  // every wave has read chunk kc - 1 out of the stage
    AGP_BF_STAMP(tb);
    AGP_BF_STORE_P(lds, SPLANE);
#ifdef AGP_BF16_STAMPS
    __builtin_amdgcn_s_waitcnt(0);  // (the barrier below waits for the stores anyway)
#endif
    AGP_BF_STAMP(tc);
    __syncthreads();
    AGP_BF_STAMP(td);
#ifdef AGP_DIAG_BF16_NOMEM  // diagnostic build: every chunk re-reads chunk 0 (L2 hits) - the ceiling without the memory side
    AGP_BF_LOAD((kc + 1 < nk ? 1 : 0) * chunk_stride);
#else
    AGP_BF_LOAD((kc + 1 < nk ? kc + 1 : kc) * chunk_stride);  // (unconditional: a guarded load kept the staging registers in scratch)
#endif
#ifdef AGP_BF16_EARLY_LOADS  // (measured, round 6: 198 registers, the waiting phase 1790 -> 1000 cycles, the matrix phase longer by as much)
    __builtin_amdgcn_sched_barrier(0);  // the loads of the next chunk stay in front of this chunk's MFMAs
#endif
    v8bf fa[3][4], fb[3][4];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        fa[p][t] = *reinterpret_cast<const v8bf *>(lds + (3 + p) * SPLANE + (64 * wc + 16 * t + ln) * SPITCH + 8 * sw_piece(lg, ln));
        fb[p][t] = *reinterpret_cast<const v8bf *>(lds + p * SPLANE + (64 * wr + 16 * t + ln) * SPITCH + 8 * sw_piece(lg, ln));
      }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        v4f32 a = acc[tj][ti];
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[2][tj], fb[0][ti], a, 0, 0, 0);  // lo hi (smallest terms first)
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][tj], fb[2][ti], a, 0, 0, 0);  // hi lo
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1][tj], fb[1][ti], a, 0, 0, 0);  // mid mid
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1][tj], fb[0][ti], a, 0, 0, 0);  // mid hi
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][tj], fb[1][ti], a, 0, 0, 0);  // hi mid
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][tj], fb[0][ti], a, 0, 0, 0);  // hi hi
        acc[tj][ti] = a;
      }
#ifdef AGP_BF16_STAMPS
    AGP_BF_STAMP(te);
    ph0 += tb - ta; ph1 += tc - tb; ph2 += td - tc; ph3 += te - td;
#endif
  }
#ifdef AGP_BF16_STAMPS
  if (blockIdx.x == gridDim.x / 2 && tid == 0) {
    g_bf16_probe[0] = ph0; g_bf16_probe[1] = ph1; g_bf16_probe[2] = ph2; g_bf16_probe[3] = ph3;
    g_bf16_probe[4] = __builtin_amdgcn_s_memtime() - loop_c0;
    g_bf16_probe[5] = __builtin_amdgcn_s_memrealtime() - loop_r0;
    g_bf16_probe[6] = (unsigned long long)nk;
  }
  const unsigned long long epi_c0 = __builtin_amdgcn_s_memtime();
#endif
  // C -= acc (register r of accumulator (tj, ti): row 16 ti + ln of the quadrant, column 16 tj + 4 lg + r)
  if (i0 + GT <= g.M && j0 + GT <= g.N) {
    double *const cbase = g.C + (i0 + 64 * wr + ln) + (j0 + 64 * wc + 4 * lg) * g.ldc;
#ifndef AGP_BF16_EPI
#define AGP_BF16_EPI 2  // (1: 163 registers, the epilogue 22 % longer and the kernel 1 % slower; 4: spills)
#endif
    constexpr int EPI = AGP_BF16_EPI;  // accumulator columns (of four) whose C is in flight at a time
#pragma unroll
    for (int t0 = 0; t0 < 4; t0 += EPI) {
      double cv[EPI][4][4];
#pragma unroll
      for (int e = 0; e < EPI; ++e)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
          for (int r = 0; r < 4; ++r) cv[e][ti][r] = __builtin_nontemporal_load(&cbase[16 * ti + (long long)(16 * (t0 + e) + r) * g.ldc]);
#pragma unroll
      for (int e = 0; e < EPI; ++e)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            __builtin_nontemporal_store(cv[e][ti][r] - (double)acc[t0 + e][ti][r], &cbase[16 * ti + (long long)(16 * (t0 + e) + r) * g.ldc]);
    }
#ifdef AGP_BF16_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    if (blockIdx.x == gridDim.x / 2 && tid == 0) g_bf16_probe[7] = __builtin_amdgcn_s_memtime() - epi_c0;  // [7] = epilogue cycles
#endif
    return;
  }
  ragged_epilogue<false>(g, acc, i0 + 64 * wr + ln, j0 + 64 * wc + 4 * lg, nullptr);
}

#undef AGP_BF_LOAD
#undef AGP_BF_STORE_P

// ---- fp16 x 2 ------------------------------------------------------------------------------------------------------
// Staging of one K chunk: piece q (16 B) of a plane tile = row q / (CH / 8), k group q % (CH / 8); a thread moves the pieces
// tid + 256 u of the two planes of both operands.
template <int TERMS, int CH>  // TERMS 3: h2 h1 + h1 h2 + h1 h1; 4: + h2 h2 (the term of weight 2^-22).  CH: k per LDS stage
__global__ __launch_bounds__(256, 2) void trailing_update_f16x2_kernel(PlaneArgs g) {
  constexpr int PIECES = CH / 8;              // 16-B pieces per row
  constexpr int NP = GT * PIECES / 256;       // pieces per thread, plane and operand
  constexpr int PLANE = GT * CH;              // one plane of one operand, in halves
  __shared__ unsigned short lds[4 * PLANE];   // [operand A: h1 h2 | operand B: h1 h2][128 rows][CH], 16-B pieces swizzled
  int bi, bj;
  if (!plane_tile_of_block(g, bi, bj)) return;
  const long long i0 = (long long)bi * GT, j0 = (long long)bj * GT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int ln = lane & 15, lg = lane >> 4;

  // A operand = the C-COLUMN panel (rows j0 ..), B operand = the C-ROW panel (rows i0 ..), as in gemm_tiles.h
  const unsigned short *srcA = g.planes + (g.row_b + j0) * CH + (long long)tid * 8, *srcB = g.planes + (g.row_a + i0) * CH + (long long)tid * 8;
  const long long chunk_stride = g.rows_pad * CH;
  // (named registers and macros: an array of them, or a lambda over them, lives in scratch memory)
  uint4 sa00, sa01, sa02, sa03, sa10, sa11, sa12, sa13, sb00, sb01, sb02, sb03, sb10, sb11, sb12, sb13;  // s<operand><plane><piece>
  const int d0 = (tid / PIECES) * CH + sw_piece<CH>(tid % PIECES, tid / PIECES) * 8;  // (row + 256 / PIECES: the same swizzle)
#define AGP_H_LOAD1(U, OFF)                                                                           \
  do {                                                                                                \
    sa0##U = *reinterpret_cast<const uint4 *>(srcA + (OFF) + (U) * 256 * 8);                          \
    sb0##U = *reinterpret_cast<const uint4 *>(srcB + (OFF) + (U) * 256 * 8);                          \
    sa1##U = *reinterpret_cast<const uint4 *>(srcA + g.plane_stride + (OFF) + (U) * 256 * 8);         \
    sb1##U = *reinterpret_cast<const uint4 *>(srcB + g.plane_stride + (OFF) + (U) * 256 * 8);         \
  } while (0)
#define AGP_H_STORE1(U)                                                                               \
  do {                                                                                                \
    *reinterpret_cast<uint4 *>(lds + 0 * PLANE + d0 + (U) * (256 / PIECES) * CH) = sa0##U;            \
    *reinterpret_cast<uint4 *>(lds + 1 * PLANE + d0 + (U) * (256 / PIECES) * CH) = sa1##U;            \
    *reinterpret_cast<uint4 *>(lds + 2 * PLANE + d0 + (U) * (256 / PIECES) * CH) = sb0##U;            \
    *reinterpret_cast<uint4 *>(lds + 3 * PLANE + d0 + (U) * (256 / PIECES) * CH) = sb1##U;            \
  } while (0)
#define AGP_H_LOAD(OFF)                                                   \
  do {                                                                    \
    const long long off_ = (OFF);                                         \
    AGP_H_LOAD1(0, off_); AGP_H_LOAD1(1, off_);                           \
    if constexpr (NP == 4) { AGP_H_LOAD1(2, off_); AGP_H_LOAD1(3, off_); } \
  } while (0)
#define AGP_H_STORE()                                                     \
  do {                                                                    \
    AGP_H_STORE1(0); AGP_H_STORE1(1);                                     \
    if constexpr (NP == 4) { AGP_H_STORE1(2); AGP_H_STORE1(3); }          \
  } while (0)

  v4f32 acc[4][4];  // [tj][ti]
  clear_acc(acc);

  const long long nk = g.K / CH;
#define AGP_H_COMPUTE()                                                                                                                  \
  do {                                                                                                                                   \
    _Pragma("unroll") for (int t = 0; t < CH / MK; ++t) { /* the matrix instruction's k steps inside the stage */                         \
      v8h fa[2][4], fb[2][4];                                                                                                            \
      _Pragma("unroll") for (int p = 0; p < 2; ++p)                                                                                      \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                                                  \
          fa[p][q] = *reinterpret_cast<const v8h *>(lds + p * PLANE + (64 * wc + 16 * q + ln) * CH + 8 * sw_piece<CH>(4 * t + lg, ln));  \
          fb[p][q] = *reinterpret_cast<const v8h *>(lds + (2 + p) * PLANE + (64 * wr + 16 * q + ln) * CH + 8 * sw_piece<CH>(4 * t + lg, ln)); \
        }                                                                                                                                \
      _Pragma("unroll") for (int tj = 0; tj < 4; ++tj)                                                                                   \
        _Pragma("unroll") for (int ti = 0; ti < 4; ++ti) {                                                                               \
          v4f32 a = acc[tj][ti];                                                                                                         \
          if (TERMS == 4) a = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[1][tj], fb[1][ti], a, 0, 0, 0); /* h2 h2 */                       \
          a = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[1][tj], fb[0][ti], a, 0, 0, 0); /* h2 h1 (smallest terms first) */               \
          a = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[0][tj], fb[1][ti], a, 0, 0, 0); /* h1 h2 */                                      \
          a = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[0][tj], fb[0][ti], a, 0, 0, 0); /* h1 h1 */                                      \
          acc[tj][ti] = a;                                                                                                               \
        }                                                                                                                                \
    }                                                                                                                                    \
  } while (0)
  // C of this wave's quadrant (register r of accumulator (tj, ti): row 16 ti + ln of the quadrant, column 16 tj + 4 lg + r)
  const long long rbase = i0 + 64 * wr + ln, cbase_col = j0 + 64 * wc + 4 * lg;
  const bool interior = i0 + GT <= g.M && j0 + GT <= g.N;
  double *const cbase = g.C + rbase + cbase_col * g.ldc;
  AGP_H_LOAD(0);
  for (long long kc = 0; kc + 1 < nk; ++kc) {
    if (kc > 0) __syncthreads();  // every wave has read chunk kc - 1 out of the stage
#if defined(AGP_DIAG_F16_NOSTORE)  // diagnostic builds (wrong results): which part of the loop the time is in
    if (kc == 0) AGP_H_STORE();
#else
    AGP_H_STORE();
#endif
    __syncthreads();
#if defined(AGP_DIAG_F16_NOLOAD) || defined(AGP_DIAG_F16_NOSTORE)
    asm volatile("" ::: "memory");
#else
    AGP_H_LOAD((kc + 1) * chunk_stride);
#endif
    AGP_H_COMPUTE();
  }
  // the last chunk: nothing left to load for the loop - the first batch of C (one accumulator column: 16 doubles) is requested in
  // front of its matrix instructions instead, and the epilogue below keeps one batch in flight behind the one it stores
  if (nk > 1) __syncthreads();
#if defined(AGP_DIAG_F16_NOSTORE)
  if (nk == 1) AGP_H_STORE();
#else
  AGP_H_STORE();
#endif
  __syncthreads();
  double cv0[4][4], cv1[4][4];
  if (interior) {
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int r = 0; r < 4; ++r) cv0[ti][r] = __builtin_nontemporal_load(&cbase[16 * ti + (long long)r * g.ldc]);
  }
  AGP_H_COMPUTE();
#undef AGP_H_COMPUTE
#undef AGP_H_LOAD
#undef AGP_H_STORE
#undef AGP_H_LOAD1
#undef AGP_H_STORE1
  // C -= acc / (r_row r_col)
  double ir_row[4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti) ir_row[ti] = (rbase + 16 * ti < g.M) ? g.irs_a[rbase + 16 * ti] : 0.;
  if (interior) {
    // software pipeline over the four accumulator columns: column tj + 1 is requested before column tj is stored
#define AGP_H_EPI_LOAD(DST, TJ)                                                                                          \
  _Pragma("unroll") for (int ti = 0; ti < 4; ++ti)                                                                       \
    _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                        \
      DST[ti][r] = __builtin_nontemporal_load(&cbase[16 * ti + (long long)(16 * (TJ) + r) * g.ldc])
#define AGP_H_EPI_STORE(SRC, TJ)                                                                                         \
  do {                                                                                                                   \
    double ic_[4];                                                                                                       \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) ic_[r] = g.irs_b[cbase_col + 16 * (TJ) + r];                           \
    _Pragma("unroll") for (int ti = 0; ti < 4; ++ti)                                                                     \
      _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                      \
        __builtin_nontemporal_store(SRC[ti][r] - (double)acc[TJ][ti][r] * (ir_row[ti] * ic_[r]),                         \
                                    &cbase[16 * ti + (long long)(16 * (TJ) + r) * g.ldc]);                               \
  } while (0)
    AGP_H_EPI_LOAD(cv1, 1);
    AGP_H_EPI_STORE(cv0, 0);
    AGP_H_EPI_LOAD(cv0, 2);
    AGP_H_EPI_STORE(cv1, 1);
    AGP_H_EPI_LOAD(cv1, 3);
    AGP_H_EPI_STORE(cv0, 2);
    AGP_H_EPI_STORE(cv1, 3);
#undef AGP_H_EPI_LOAD
#undef AGP_H_EPI_STORE
    return;
  }
  ragged_epilogue<true>(g, acc, rbase, cbase_col, ir_row);
}

// ---- the launchers ---------------------------------------------------------------------------------------------------
// C (M x N, lower tiles, C(0, 0) on the matrix diagonal) -= P[row_a ..] P[row_b ..]^T from the planes of ONE panel of
// panel_rows rows.  irs: 1 / r of the PANEL's rows (irs[0] belongs to panel row 0; nullptr: bf16 planes).  order / order_len:
// the XCD-aware tile order of gemm.hip (nullptr: column-major tiles).  Returns the workgroups to launch.
static long long plane_args(PlaneArgs &g, double *C, long long ldc, const unsigned short *planes, long long panel_rows, long long row_a,
                            long long row_b, const double *irs, long long M, long long N, long long K, const int *order, long long order_len) {
  g.C = C; g.ldc = ldc; g.planes = planes;
  g.rows_pad = planes_rows_pad(panel_rows);
  g.plane_stride = g.rows_pad * K;
  g.row_a = row_a; g.row_b = row_b;
  g.irs_a = irs ? irs + row_a : nullptr; g.irs_b = irs ? irs + row_b : nullptr;
  g.M = M; g.N = N; g.K = K;
  g.ntr = (int)((M + GT - 1) / GT);
  g.ntc = (int)((N + GT - 1) / GT);
  if (g.ntc > g.ntr) g.ntc = g.ntr;
  g.order = order;
  return order ? order_len : lower_tile_count(g.ntr, g.ntc, 1);
}

// tune.lds_pad (extra dynamic LDS) sets how many workgroups share a CU next to the panel kernels of the chain stream.
// bf16 x 3: 0 = three workgroups per CU (3 x 48 KB), >= 6 KB = two.  Three are the faster KERNEL (+2 %) and the slower FIT
// (126.8 against 123.0 ms at N = 32768, same box): the panel kernels of the chain stream need LDS next to the bulk update.
void launch_update_bf16x3(hipStream_t s, Bf16x3Tuning tune, double *C, long long ldc, const unsigned short *planes, long long panel_rows, long long row_a,
                          long long row_b, long long M, long long N, long long K, const int *order, long long order_len) {
  if (M <= 0 || N <= 0 || K <= 0 || K % BK) return;
  PlaneArgs g;
  const long long wgs = plane_args(g, C, ldc, planes, panel_rows, row_a, row_b, nullptr, M, N, K, order, order_len);
  if (wgs <= 0) return;
  hipLaunchKernelGGL(trailing_update_bf16x3_pair_kernel, dim3((unsigned)wgs), dim3(256), (size_t)tune.lds_pad, s, g);
}

// fp16 x 2: 32 KB static (CH = 32); registers allow two workgroups per CU.
void launch_update_f16x2(hipStream_t s, F16x2Tuning tune, double *C, long long ldc, const unsigned short *planes, long long panel_rows, long long row_a,
                         long long row_b, const double *irs, long long M, long long N, long long K, const int *order, long long order_len) {
  if (M <= 0 || N <= 0 || !f16x2_depth_ok(tune, K)) return;
  PlaneArgs g;
  const long long wgs = plane_args(g, C, ldc, planes, panel_rows, row_a, row_b, irs, M, N, K, order, order_len);
  if (wgs <= 0) return;
  const dim3 grid((unsigned)wgs), block(256);
  const size_t pad = (size_t)tune.lds_pad;
  if (tune.chunk == 64) {
    if (tune.terms == 4) hipLaunchKernelGGL((trailing_update_f16x2_kernel<4, 64>), grid, block, pad, s, g);
    else hipLaunchKernelGGL((trailing_update_f16x2_kernel<3, 64>), grid, block, pad, s, g);
  } else {
    if (tune.terms == 4) hipLaunchKernelGGL((trailing_update_f16x2_kernel<4, 32>), grid, block, pad, s, g);
    else hipLaunchKernelGGL((trailing_update_f16x2_kernel<3, 32>), grid, block, pad, s, g);
  }
}

}  // namespace agp
