// gram_tangent.hip — forms[c, p] = U[:, c]^T (dk(x, x) / dslot_p) V[:, c] for a block of column pairs with the tangent matrix
// evaluated pair by pair (cov_eval.h: eval_pair_tangent) and never stored, and no n x n weight either:
// agp_gram_tangent_forms (include/albatross_amd.h), and launch_gram_tangent_forms for the probe gradient of the matrix-free
// fit (iterative.hip).
//
// The tangent matrix is symmetric: a pair (i > j) is evaluated once, as (row i, column j) like contract_tile's lower
// contraction, and applied both ways with the weight U_ic V_jc + V_ic U_jc; the diagonal pair takes half of that weight,
// which is U_ic V_ic once.  A lane owns a row: its point, its U_ic and V_ic (T <= TF_MAX_PAIRS column pairs of a chunk) and
// its T x GRAD_GROUP accumulators stay in registers.  The column points, their tangent values and their rows of U and V go
// through LDS in tiles of TF_COLS columns; every lane of a wave reads the same column, so the reads are broadcasts, and
// dk[g] is evaluated ONCE per walk of GRAD_GROUP slots for the T weights of the chunk.  The tile after the current one is
// requested from global memory before the current one is evaluated (one barrier per tile), as in gram_matvec_kernel.
//
// Work: the lower triangle in row blocks of TF_ROWS.  Row block b has the column tiles 0 .. its diagonal, so a workgroup
// takes the pair of row blocks (q, nb - 1 - q), whose lists together have the same length for every q, and one slice of
// that list (gram_tangent_plan: depends on n alone).  It keeps its sums in registers over its whole walk and writes ONE
// block of T x GRAD_GROUP sums: scratch is units x slices x TF_MAX_PAIRS x GRAD_GROUP doubles, never one entry per tile.
// A second launch adds the blocks in a fixed order.  No float atomics: identical bits on repeated calls.
#include <cstring>
#include "api_internal.h"
#include "gram_tangent.h"
#include "trace.h"

namespace agp {

template <int DIMP, int T>
struct TfTile {
  static constexpr int TP = T == 1 ? 1 : T + 2;  // padded rows of U and V: the staging writes of a wave spread over the banks
  double c[DIMP][TF_COLS];
  double norm[TF_COLS];
  double s[AGP_MAX_SCALE_COLUMNS][TF_COLS];
  long long id[TF_COLS];
  double ty[GRAD_GROUP][TF_COLS];  // the tangent column of an AGP_OP_SCALING slot at the column point
  double u[TF_COLS][TP];
  double v[TF_COLS][TP];
};

struct TfArgs {
  const DevProgram *P;
  TangentSlots<GRAD_GROUP> slots;
  const double *tang[GRAD_GROUP];  // AGP_OP_SCALING slot g: its tangent column (n values), else nullptr
  FeatView X;
  const double *U, *V;
  long long ldu, ldv;
  int npairs;                      // column pairs of this chunk (<= T)
  long long row_blocks;
  int tiles_per_slice;
  double *partial;                 // [unit][slice][TF_MAX_PAIRS][GRAD_GROUP]
  int *nan_flag;
  const int *go;                   // optional: a value <= 0 there makes the launch return at once
};

// column tiles of row block b: the columns 0 .. its last row
__host__ __device__ inline long long tf_col_tiles(long long b, long long n) {
  const long long end = (b + 1) * TF_ROWS < n ? (b + 1) * TF_ROWS : n;
  return (end + TF_COLS - 1) / TF_COLS;
}

template <int DIMP, int T>
__global__ __launch_bounds__(TF_ROWS) void gram_tangent_kernel(TfArgs a) {
  if (a.go && *a.go <= 0) return;
  constexpr int G = GRAD_GROUP;
  using Tile = TfTile<DIMP, T>;
  __shared__ Tile tiles[2];
  __shared__ double red[TF_ROWS / 64][T * G];
  constexpr int VPT = (TF_COLS * T + TF_ROWS - 1) / TF_ROWS;  // elements of U (and of V) a thread stages per tile
  const long long n = a.X.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long bA = blockIdx.x, bB = a.row_blocks - 1 - bA;
  const int tilesA = (int)tf_col_tiles(bA, n), tilesB = bB > bA ? (int)tf_col_tiles(bB, n) : 0;
  const int t0 = (int)blockIdx.y * a.tiles_per_slice;
  const int t1 = t0 + a.tiles_per_slice < tilesA + tilesB ? t0 + a.tiles_per_slice : tilesA + tilesB;
  const bool need_norm = (a.P->metric_mask & ((1 << AGP_METRIC_RADIAL) | (1 << AGP_METRIC_ANGULAR))) != 0;
  const bool have_ids = a.X.ids != nullptr, meas = a.X.meas != 0;

  double acc[T][G];
#pragma unroll
  for (int c = 0; c < T; ++c)
#pragma unroll
    for (int g = 0; g < G; ++g) acc[c][g] = 0.;
  bool saw_nan = false;

  // ---- the row a lane owns in the current row block ----
  Point<DIMP> x;
  double tx[G], ui[T], vi[T];
  long long row = -1;  // (-1 past the end: no column is at or below it)
  auto load_row = [&](long long block) {
    const long long r = block * TF_ROWS + tid;
    const long long rc = r < n ? r : n - 1;
    load_point<DIMP>(a.X, rc, need_norm, x);
#pragma unroll
    for (int g = 0; g < G; ++g) tx[g] = a.tang[g] ? a.tang[g][rc] : 0.;
#pragma unroll
    for (int c = 0; c < T; ++c) {
      const bool on = r < n && c < a.npairs;
      ui[c] = on ? a.U[(long long)c * a.ldu + r] : 0.;
      vi[c] = on ? a.V[(long long)c * a.ldv + r] : 0.;
    }
    row = r < n ? r : -1;
  };

  // ---- staging: thread t < TF_COLS holds column point t of the next tile, every thread VPT elements of U and of V ----
  Point<DIMP> pn;
  double tyn[G], un[VPT], vn[VPT];
  auto request = [&](int t) {
    const long long c0 = (long long)(t < tilesA ? t : t - tilesA) * TF_COLS;
    if (tid < TF_COLS) {  // (wave 0: wave-uniform)
      const long long j = c0 + tid < n ? c0 + tid : n - 1;  // (past the end: a valid point that no row is at or below)
      load_point<DIMP>(a.X, j, need_norm, pn);
#pragma unroll
      for (int g = 0; g < G; ++g) tyn[g] = a.tang[g] ? a.tang[g][j] : 0.;
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int e = tid + u * TF_ROWS;
      const int c = e / TF_COLS, j = e % TF_COLS;
      const bool on = e < TF_COLS * T && c < a.npairs && c0 + j < n;
      un[u] = on ? a.U[(long long)c * a.ldu + c0 + j] : 0.;
      vn[u] = on ? a.V[(long long)c * a.ldv + c0 + j] : 0.;
    }
  };
  auto deposit = [&](Tile &L) {
    if (tid < TF_COLS) {
#pragma unroll
      for (int d = 0; d < DIMP; ++d) L.c[d][tid] = pn.c[d];
      L.norm[tid] = pn.norm;
#pragma unroll
      for (int k = 0; k < AGP_MAX_SCALE_COLUMNS; ++k) L.s[k][tid] = pn.s[k];
      L.id[tid] = pn.id;
#pragma unroll
      for (int g = 0; g < G; ++g) L.ty[g][tid] = tyn[g];
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int e = tid + u * TF_ROWS;
      if (e < TF_COLS * T) {
        L.u[e % TF_COLS][e / TF_COLS] = un[u];
        L.v[e % TF_COLS][e / TF_COLS] = vn[u];
      }
    }
  };

  if (t0 < t1) {
    long long cur = -1;
    request(t0);
    deposit(tiles[0]);
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
      if (t + 1 < t1) request(t + 1);
      const Tile &L = tiles[(t - t0) & 1];
      const long long blk = t < tilesA ? bA : bB;
      if (blk != cur) {  // (the whole workgroup: once, or twice when the slice spans both row blocks)
        load_row(blk);
        cur = blk;
      }
      const long long c0 = (long long)(t < tilesA ? t : t - tilesA) * TF_COLS;
      const long long wave_last = blk * TF_ROWS + wave * 64 + 63;  // the last row of this wave: columns beyond it have no pair
      const long long left = (wave_last < n - 1 ? wave_last : n - 1) - c0 + 1;
      const int cnt = (int)(left < TF_COLS ? left : TF_COLS);      // (wave-uniform; <= 0: the tile lies above the wave's rows)
#pragma unroll 1
      for (int j = 0; j < cnt; ++j) {
        Point<DIMP> y;
#pragma unroll
        for (int d = 0; d < DIMP; ++d) y.c[d] = L.c[d][j];
        y.norm = L.norm[j];
#pragma unroll
        for (int k = 0; k < AGP_MAX_SCALE_COLUMNS; ++k) y.s[k] = L.s[k][j];
        y.id = L.id[j];
        double ty[G], dk[G];
#pragma unroll
        for (int g = 0; g < G; ++g) ty[g] = L.ty[g][j];
        eval_pair_tangent<DIMP, G>(a.P, a.slots, x, y, tx, ty, have_ids, meas, dk);
        // the pair counts once below the diagonal (applied both ways by the weight), half on it, not above it
        const long long col = c0 + j;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          dk[g] = col < row ? dk[g] : (col == row ? 0.5 * dk[g] : 0.);
          saw_nan = saw_nan || dk[g] != dk[g];
        }
#pragma unroll
        for (int c = 0; c < T; ++c) {
          const double w = ui[c] * L.v[j][c] + vi[c] * L.u[j][c];
#pragma unroll
          for (int g = 0; g < G; ++g) acc[c][g] = __builtin_fma(w, dk[g], acc[c][g]);
        }
      }
      if (t + 1 < t1) deposit(tiles[(t + 1 - t0) & 1]);
      __syncthreads();
    }
  }

  // ---- the workgroup's T x G sums in a fixed order: butterfly inside the wave, then the four waves in order ----
#pragma unroll
  for (int c = 0; c < T; ++c)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double v = acc[c][g];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) red[wave][c * G + g] = v;
    }
  __syncthreads();
  if (tid < T * G) {
    double v = red[0][tid];
#pragma unroll
    for (int w = 1; w < TF_ROWS / 64; ++w) v += red[w][tid];
    a.partial[((long long)blockIdx.x * gridDim.y + blockIdx.y) * (TF_MAX_PAIRS * G) + tid] = v;
  }
  if (saw_nan) atomicOr(a.nan_flag, 1);
}

// forms[c + g * ldf] = the sum over the workgroups' blocks: four strided serial sums, then the four in order
__global__ __launch_bounds__(4 * TF_MAX_PAIRS * GRAD_GROUP) void gram_tangent_sum_kernel(const double *partial, long long blocks, int npairs,
                                                                                         int nslots, double *forms, long long ldf,
                                                                                         const int *go) {
  if (go && *go <= 0) return;
  constexpr int E = TF_MAX_PAIRS * GRAD_GROUP;
  __shared__ double red[4][E];
  const int e = threadIdx.x % E, r = threadIdx.x / E;
  double s = 0.;
  if (e < npairs * GRAD_GROUP)  // (a kernel of T < TF_MAX_PAIRS column pairs writes the first T * GRAD_GROUP entries of a block alone)
    for (long long b = r; b < blocks; b += 4) s += partial[b * E + e];
  red[r][e] = s;
  __syncthreads();
  const int c = e / GRAD_GROUP, g = e % GRAD_GROUP;
  if (r == 0 && c < npairs && g < nslots) forms[c + (long long)g * ldf] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

TfPlan gram_tangent_plan(long long n) {
  TfPlan p{};
  p.row_blocks = (n + TF_ROWS - 1) / TF_ROWS;
  p.units = (p.row_blocks + 1) / 2;
  p.max_tiles = 0;
  for (long long q = 0; q < p.units; ++q) {
    const long long other = p.row_blocks - 1 - q;
    const long long len = tf_col_tiles(q, n) + (other > q ? tf_col_tiles(other, n) : 0);
    if (len > p.max_tiles) p.max_tiles = len;
  }
  if (p.units < 1) { p.units = 0; p.slices = 0; p.tiles_per_slice = TF_MIN_SLICE_TILES; return p; }
  const long long want = (TF_TARGET_WGS + p.units - 1) / p.units;
  long long tps = (p.max_tiles + want - 1) / want;
  if (tps < TF_MIN_SLICE_TILES) tps = TF_MIN_SLICE_TILES;
  p.tiles_per_slice = tps;
  p.slices = (p.max_tiles + tps - 1) / tps;
  return p;
}

int gram_tangent_chunk_width(long long remaining) { return remaining >= 5 ? TF_MAX_PAIRS : (remaining >= 2 ? 4 : 1); }

size_t gram_tangent_ws_elems(long long n) {
  const TfPlan p = gram_tangent_plan(n);
  return (size_t)p.units * (size_t)p.slices * (size_t)(TF_MAX_PAIRS * GRAD_GROUP);
}

template <int DIMP>
static void tf_launch_t(hipStream_t s, dim3 grid, int T, const TfArgs &a) {
  if (T == 1) hipLaunchKernelGGL((gram_tangent_kernel<DIMP, 1>), grid, dim3(TF_ROWS), 0, s, a);
  else if (T == 4) hipLaunchKernelGGL((gram_tangent_kernel<DIMP, 4>), grid, dim3(TF_ROWS), 0, s, a);
  else hipLaunchKernelGGL((gram_tangent_kernel<DIMP, TF_MAX_PAIRS>), grid, dim3(TF_ROWS), 0, s, a);
}

void launch_gram_tangent_forms(hipStream_t s, const DevProgram *P, const agp_kernel *k, const FeatView &X, int n_slots,
                               const agp_gradient_slot *slots, const double *tang, long long ldt, const double *U, long long ldu,
                               const double *V, long long ldv, long long ncols, double *forms, long long ldf, double *ws,
                               int *nan_flag, const int *go) {
  const long long n = X.n;
  if (n <= 0 || ncols <= 0 || n_slots <= 0) return;
  const TfPlan plan = gram_tangent_plan(n);
  TfArgs a{};
  a.P = P;
  a.X = X;
  a.ldu = ldu;
  a.ldv = ldv;
  a.row_blocks = plan.row_blocks;
  a.tiles_per_slice = (int)plan.tiles_per_slice;
  a.partial = ws;
  a.nan_flag = nan_flag;
  a.go = go;
  const dim3 grid((unsigned)plan.units, (unsigned)plan.slices);
  for (int g0 = 0; g0 < n_slots; g0 += GRAD_GROUP) {
    bool scaling[GRAD_GROUP];
    const int cnt = fill_slot_group(k, n_slots, slots, g0, a.slots, scaling);
    for (int j = 0; j < GRAD_GROUP; ++j) a.tang[j] = scaling[j] ? tang + (size_t)a.slots.param[j] * (size_t)ldt : nullptr;
    for (long long c0 = 0; c0 < ncols;) {
      const int T = gram_tangent_chunk_width(ncols - c0);
      const int cn = (int)(ncols - c0 < T ? ncols - c0 : T);
      a.U = U + c0 * ldu;
      a.V = V + c0 * ldv;
      a.npairs = cn;
      dispatch_dim(X.dim, [&](auto D) { tf_launch_t<decltype(D)::value>(s, grid, T, a); });
      hipLaunchKernelGGL(gram_tangent_sum_kernel, dim3(1), dim3(4 * TF_MAX_PAIRS * GRAD_GROUP), 0, s, ws, plan.units * plan.slices, cn, cnt,
                         forms + c0 + (long long)g0 * ldf, ldf, go);
      c0 += cn;
    }
  }
}

}  // namespace agp

using namespace agp;

extern "C" {

int agp_gram_tangent_forms(agp_context *c, const agp_kernel *k, const agp_features *x, int n_slots, const agp_gradient_slot *slots,
                           const double *tangents, int64_t ldt, const double *U, int64_t ldu, const double *V, int64_t ldv,
                           int64_t ncols, double *forms, int64_t ldf, int location) {
  if (!c || !k || !x) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && !slots) || ncols < 0 ||
      (location != AGP_HOST && location != AGP_DEVICE))
    return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n < 1) return AGP_ERR_INVALID_ARGUMENT;
  int ntc = 0;
  if ((st = check_slots(k, n_slots, slots, &ntc)) != AGP_OK) return st;
  if (ntc > 0 && (!tangents || ldt < n)) return AGP_ERR_INVALID_ARGUMENT;
  if (ncols == 0 || n_slots == 0) return AGP_OK;
  if (!U || !V || !forms || ldu < n || ldv < n || ldf < ncols) return AGP_ERR_INVALID_ARGUMENT;
  if ((n + TF_COLS - 1) / TF_COLS > 0x7fffffffll) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;

  // scratch: the NaN flag | the forms | the tangent columns, U and V of a host caller | the workgroups' blocks
  const bool host = location == AGP_HOST;
  const long long ldd = round_up(n, 2), ldfd = round_up(ncols, 2);
  const size_t forms_elems = (size_t)ldfd * (size_t)n_slots;
  const size_t stage_elems = host ? (size_t)ldd * ((size_t)ntc + 2 * (size_t)ncols) : 0;
  DevMem<double> ws;
  AGP_HIP_CHECK(ctx, alloc_doubles(ws, 2 + forms_elems + stage_elems + gram_tangent_ws_elems(n)));
  int *flag = reinterpret_cast<int *>(ws.get());
  double *forms_d = ws.get() + 2, *cur = forms_d + forms_elems;
  const double *Td = tangents, *Ud = U, *Vd = V;
  long long ldtd = ldt, ldud = ldu, ldvd = ldv;
  if (host) {
    auto upload = [&](const double *src, long long ld, long long cols, const double **dev) -> hipError_t {
      *dev = cur;
      const hipError_t e = hipMemcpy2DAsync(cur, sizeof(double) * (size_t)ldd, src, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n,
                                            (size_t)cols, hipMemcpyHostToDevice, s);
      cur += (size_t)ldd * (size_t)cols;
      return e;
    };
    if (ntc > 0) AGP_HIP_CHECK(ctx, upload(tangents, ldt, ntc, &Td));
    AGP_HIP_CHECK(ctx, upload(U, ldu, ncols, &Ud));
    AGP_HIP_CHECK(ctx, upload(V, ldv, ncols, &Vd));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable sources
    ldtd = ldud = ldvd = ldd;
  }
  const size_t out_bytes = sizeof(double) * forms_elems;
  char *h_stage = static_cast<char *>(host_stage(ctx, 64 + out_bytes));
  if (!h_stage) { ctx->last_error = "agp_gram_tangent_forms: no pinned staging memory"; return AGP_ERR_HIP; }
  int *h_flag = reinterpret_cast<int *>(h_stage);
  const double *h_forms = reinterpret_cast<const double *>(h_stage + 64);
  AGP_HIP_CHECK(ctx, hipMemsetAsync(flag, 0, sizeof(int), s));
  {
    TraceRange tr("agp: tangent bilinear forms without the matrix");
    launch_gram_tangent_forms(s, dprog, k, dx.v, n_slots, slots, Td, ldtd, Ud, ldud, Vd, ldvd, ncols, forms_d, ldfd, cur, flag);
  }
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_stage + 64, forms_d, out_bytes, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (*h_flag) return AGP_ERR_NAN_INPUT;
  for (int p = 0; p < n_slots; ++p)  // entry by entry: the padding of the caller's block is not touched
    for (long long cc = 0; cc < ncols; ++cc) forms[cc + (long long)p * ldf] = h_forms[cc + (long long)p * ldfd];
  return AGP_OK;
}

}  // extern "C"
