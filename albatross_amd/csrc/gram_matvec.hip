// gram_matvec.hip — out[:, c] = (k(x, x) + diag(y_var)) V[:, c] for a block of right-hand sides with K evaluated pair by
// pair and never stored: agp_gram_matvec (include/albatross_amd.h), and launch_gram_matvec for the conjugate-gradient
// solve of iterative.hip.
//
// A workgroup of MV_ROWS threads owns MV_ROWS consecutive rows, one per lane, and one slice of the columns; a lane keeps
// the T accumulators of its row (T = 1, 4 or 16 right-hand sides of a chunk) in registers.  The column points and their
// rows of V go through LDS in tiles of MV_COLS columns: every lane of a wave reads the same column j, so the reads are
// broadcasts (no bank conflicts), and the entry K_ij is evaluated ONCE for the T products of the chunk.  The tile after
// the current one is requested from global memory before the current one is evaluated and written to the other LDS
// buffer behind it (one barrier per tile).  The pairs of a group (MV_GROUP_FAST columns on the radial fast path) are
// evaluated in one basic block, their exponential chains in lock step (gram_fast.h: radial_fast_n), as
// predict_mean_tiled_kernel does and explains (gram.hip).
//
// Small n: the column range is split over blockIdx.y into S slices (gram_matvec_slices: S depends on n alone), each of
// which writes its partial sums; a second launch adds the S partials of an entry in slice order.  No float atomics, a
// fixed order of every sum: identical bits on repeated calls.
//
// Entry (i, j) has the bits agp_gram gives it for the symmetric matrix of x: the same evaluator (radial fast path, sum of
// products - which the pair-2 kernel restates -, or the postfix interpreter, chosen as gram.hip chooses), the same
// argument order (evaluated as (i, j) for i >= j and mirrored), y_var added to the diagonal entry before the product;
// this file is compiled without FMA contraction, the accumulation acc = fma(K_ij, V_jc, acc) is spelled out.
#include <cstring>
#include "api_internal.h"
#include "gram_fast.h"
#include "gram_matvec.h"
#include "trace.h"

namespace agp {

constexpr int MV_GROUP_FAST = 4;  // pairs per basic block: radial fast path
constexpr int MV_GROUP_SOP = 2;   // sum of products (the scalar walk of the program is shared by the pairs)

template <int DIMP, int T>
struct MvTile {
  static constexpr int TP = T == 1 ? 1 : T + 2;  // padded row of V: the staging writes of a wave spread over the banks
  double c[DIMP][MV_COLS];
  double norm[MV_COLS];
  double s[AGP_MAX_SCALE_COLUMNS][MV_COLS];
  long long id[MV_COLS];
  double v[MV_COLS][TP];
};

struct MvArgs {
  const DevProgram *P;
  FastParams fp;
  int need_norm;
  FeatView X;
  const double *yvar;  // n values or nullptr
  const double *V;
  long long ldv;
  int nrhs;            // columns of this chunk (<= T)
  double *out;         // one slice: the caller's block; else the partial sums, slice s at out + s * slice_stride
  long long ldo;
  long long slice_stride;
  long long cps;       // columns per slice (a multiple of MV_COLS)
  int *nan_flag;
  const int *go;        // optional: a value <= 0 there makes the launch return at once (the solve's queued iterations after its end)
};

template <int DIMP>
__device__ __forceinline__ Point<DIMP> mv_read_point(const double (&c)[DIMP][MV_COLS], const double (&norm)[MV_COLS],
                                                     const double (&s)[AGP_MAX_SCALE_COLUMNS][MV_COLS],
                                                     const long long (&id)[MV_COLS], int slot) {
  Point<DIMP> p;
#pragma unroll
  for (int d = 0; d < DIMP; ++d) p.c[d] = c[d][slot];
  p.norm = norm[slot];
#pragma unroll
  for (int k = 0; k < AGP_MAX_SCALE_COLUMNS; ++k) p.s[k] = s[k][slot];
  p.id = id[slot];
  return p;
}

template <int DIMP, int EVAL, int OP, int T>
__global__ __launch_bounds__(MV_ROWS) void gram_matvec_kernel(MvArgs a, SopProgram sop) {
  if (a.go && *a.go <= 0) return;
  using Tile = MvTile<DIMP, T>;
  __shared__ Tile tiles[2];
  constexpr int VPT = (MV_COLS * T + MV_ROWS - 1) / MV_ROWS;  // elements of V a thread stages per tile
  const long long n = a.X.n;
  const int tid = threadIdx.x;
  const long long row = (long long)blockIdx.x * MV_ROWS + tid;
  const long long rowc = row < n ? row : n - 1;  // (rows past the end evaluate the last point and store nothing)
  const long long cbeg = (long long)blockIdx.y * a.cps;
  const long long cend = cbeg + a.cps < n ? cbeg + a.cps : n;
  const int ntiles = (int)((cend - cbeg + MV_COLS - 1) / MV_COLS);
  const bool have_ids = a.X.ids != nullptr, meas = a.X.meas != 0;
  const bool need_norm = a.need_norm != 0;
  const long long wave_row0 = (long long)blockIdx.x * MV_ROWS + (tid & ~63);

  Point<DIMP> x;
  load_point<DIMP>(a.X, rowc, need_norm, x);
  const double yv = a.yvar ? a.yvar[rowc] : 0.;
  double acc[T];
#pragma unroll
  for (int c = 0; c < T; ++c) acc[c] = 0.;
  bool saw_nan = false;

  // ---- staging: thread t < MV_COLS holds column point t of the next tile, every thread VPT elements of V ----
  Point<DIMP> pn;
  double vn[VPT];
  auto request = [&](int t) {
    const long long c0 = cbeg + (long long)t * MV_COLS;
    if (tid < MV_COLS) {  // (wave 0: wave-uniform)
      const long long g = c0 + tid < cend ? c0 + tid : cend - 1;  // (past the slice: a valid point, its row of V is zero)
      load_point<DIMP>(a.X, g, need_norm, pn);
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int e = tid + u * MV_ROWS;
      const int c = e / MV_COLS, j = e % MV_COLS;
      vn[u] = (e < MV_COLS * T && c < a.nrhs && c0 + j < cend) ? a.V[(long long)c * a.ldv + c0 + j] : 0.;
    }
  };
  auto deposit = [&](Tile &L) {
    if (tid < MV_COLS) {
#pragma unroll
      for (int d = 0; d < DIMP; ++d) L.c[d][tid] = pn.c[d];
      L.norm[tid] = pn.norm;
#pragma unroll
      for (int k = 0; k < AGP_MAX_SCALE_COLUMNS; ++k) L.s[k][tid] = pn.s[k];
      L.id[tid] = pn.id;
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
      const int e = tid + u * MV_ROWS;
      if (e < MV_COLS * T) L.v[e % MV_COLS][e / MV_COLS] = vn[u];
    }
  };
  // acc += K_ij V_j. for the T columns of the chunk; the row of V is a broadcast read
  auto accumulate = [&](const Tile &L, int j, double kij) {
#pragma unroll
    for (int c = 0; c < T; ++c) acc[c] = __builtin_fma(kij, L.v[j][c], acc[c]);
  };

  request(0);
  deposit(tiles[0]);
  __syncthreads();
  const bool dead = EVAL == MV_PATH_FAST && a.fp.length_scale <= 0.;  // radial.hpp: 0 for a non-positive length scale
  const bool noise_on = a.fp.has_noise && (!a.fp.noise_meas_only || meas);
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) request(t + 1);
    const Tile &L = tiles[t & 1];
    const long long c0 = cbeg + (long long)t * MV_COLS;
    const int cnt = (int)(cend - c0 < MV_COLS ? cend - c0 : MV_COLS);
    // does this tile hold a diagonal entry of one of this wave's rows?  (wave-uniform)
    const bool diag_tile = a.yvar != nullptr && c0 < wave_row0 + 64 && c0 + cnt > wave_row0;
    const int di = (int)(row - c0 >= 0 && row - c0 < MV_COLS ? row - c0 : -1);  // the slot of K_ii in this tile, or -1
    if (EVAL == MV_PATH_FAST) {
      constexpr int G = MV_GROUP_FAST;
#pragma unroll 1
      for (int j0 = 0; j0 < cnt; j0 += G) {  // (cnt rounds up to a whole group: the slots past it hold valid points and zeros of V)
        double s2[G], y[G][DIMP], v[G];
#pragma unroll
        for (int p = 0; p < G; ++p) {
          s2[p] = 0.;
#pragma unroll
          for (int d = 0; d < DIMP; ++d) {
            y[p][d] = L.c[d][j0 + p];
            const double dd = x.c[d] - y[p][d];
            s2[p] += dd * dd;
          }
        }
        if (dead) {
#pragma unroll
          for (int p = 0; p < G; ++p) v[p] = 0.;
        } else {
          if (OP == AGP_OP_SQUARED_EXPONENTIAL) radial_fast_n<AGP_OP_SQUARED_EXPONENTIAL, G>(s2, a.fp, v);
          else if (OP == AGP_OP_EXPONENTIAL) radial_fast_n<AGP_OP_EXPONENTIAL, G>(s2, a.fp, v);
          else if (OP == AGP_OP_MATERN32) radial_fast_n<AGP_OP_MATERN32, G>(s2, a.fp, v);
          else radial_fast_n<AGP_OP_MATERN52, G>(s2, a.fp, v);
        }
        if (a.fp.has_noise) {  // lhs + rhs with rhs = the noise (0 when not measurements / not equal): gram_fast_body
          bool e[G], maybe = false;
#pragma unroll
          for (int p = 0; p < G; ++p) {
            e[p] = false;
            maybe = maybe || (have_ids ? x.id == L.id[j0 + p] : s2[p] == 0.);
          }
          if (noise_on && __any(maybe)) {
#pragma unroll
            for (int p = 0; p < G; ++p) {
              bool eq = true;
#pragma unroll
              for (int d = 0; d < DIMP; ++d) eq = eq && (x.c[d] == y[p][d]);
              if (have_ids) eq = x.id == L.id[j0 + p];
              e[p] = eq;
            }
          }
#pragma unroll
          for (int p = 0; p < G; ++p) v[p] = v[p] + (e[p] ? a.fp.noise_var : 0.);
        }
        if (diag_tile) {
#pragma unroll
          for (int p = 0; p < G; ++p) v[p] = (j0 + p == di) ? v[p] + yv : v[p];
        }
#pragma unroll
        for (int p = 0; p < G; ++p) {
          saw_nan = saw_nan || v[p] != v[p];
          accumulate(L, j0 + p, v[p]);
        }
      }
    } else if (EVAL == MV_PATH_SOP) {
      constexpr int G = MV_GROUP_SOP;
#pragma unroll 1
      for (int j0 = 0; j0 < cnt; j0 += G) {
        const Point<DIMP> y0 = mv_read_point<DIMP>(L.c, L.norm, L.s, L.id, j0);
        const Point<DIMP> y1 = mv_read_point<DIMP>(L.c, L.norm, L.s, L.id, j0 + 1);
        const Point<DIMP> *const xs2[G] = {&x, &x};
        const Point<DIMP> *const ys2[G] = {&y0, &y1};
        // the symmetric Gram matrix is evaluated for i >= j and mirrored (callers.hpp:119-127): the same argument order
        const bool sw2[G] = {row < c0 + j0, row < c0 + j0 + 1};
        double v[G];
        eval_sop_n<DIMP, G>(sop, xs2, ys2, sw2, have_ids, meas, v);
#pragma unroll
        for (int p = 0; p < G; ++p) {
          if (diag_tile) v[p] = (j0 + p == di) ? v[p] + yv : v[p];
          saw_nan = saw_nan || v[p] != v[p];
          accumulate(L, j0 + p, v[p]);
        }
      }
    } else {
#pragma unroll 1
      for (int j = 0; j < cnt; ++j) {
        const Point<DIMP> y = mv_read_point<DIMP>(L.c, L.norm, L.s, L.id, j);
        double v = eval_pair<DIMP>(a.P, x, y, row < c0 + j, have_ids, meas);
        if (diag_tile) v = (j == di) ? v + yv : v;
        saw_nan = saw_nan || v != v;
        accumulate(L, j, v);
      }
    }
    if (t + 1 < ntiles) deposit(tiles[(t + 1) & 1]);
    __syncthreads();
  }
  if (row < n) {
    double *dst = a.out + (long long)blockIdx.y * a.slice_stride + row;
#pragma unroll
    for (int c = 0; c < T; ++c)
      if (c < a.nrhs) dst[(long long)c * a.ldo] = acc[c];
    if (saw_nan) atomicOr(a.nan_flag, 1);
  }
}

// out[i, c] = partial[0][i, c] + partial[1][i, c] + ... in slice order
__global__ __launch_bounds__(256) void gram_matvec_sum_kernel(const double *partial, long long ldp, long long slice_stride,
                                                              long long slices, long long n, double *out, long long ldo, const int *go) {
  if (go && *go <= 0) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *src = partial + (long long)blockIdx.y * ldp + i;
  double s = src[0];
  for (long long k = 1; k < slices; ++k) s += src[k * slice_stride];
  out[(long long)blockIdx.y * ldo + i] = s;
}

bool gram_build_sop(const DevProgram &H, SopProgram *out);  // gram.hip

struct MvPlanFull {
  MvPlan pub;
  FastParams fp;
  int op;
  int need_norm;
  SopProgram sop;
};

// S and the columns of a slice: MV_TARGET_WGS workgroups where n allows it, a slice of MV_MIN_SLICE columns at least and a
// whole number of tiles.  Depends on n alone.
void gram_matvec_slices(long long n, long long *slices, long long *cols_per_slice) {
  const long long row_tiles = (n + MV_ROWS - 1) / MV_ROWS;
  long long want = (MV_TARGET_WGS + row_tiles - 1) / row_tiles;
  const long long most = (n + MV_MIN_SLICE - 1) / MV_MIN_SLICE;
  if (want > most) want = most;
  if (want < 1) want = 1;
  const long long cps = round_up((n + want - 1) / want, MV_COLS);
  *cols_per_slice = cps;
  *slices = (n + cps - 1) / cps;
}

// THE choice of the evaluator (launch_gram_matvec switches on it and decides nothing itself): the one gram_select_path
// makes for the symmetric matrix of X, with the pair-2 trees on the sum-of-products evaluator whose arithmetic that
// kernel restates
static void mv_select(const DevProgram *host_program, const FeatView &X, MvPlanFull *plan) {
  std::memset(&plan->sop, 0, sizeof(plan->sop));
  std::memset(&plan->fp, 0, sizeof(plan->fp));
  plan->op = 0;
  plan->need_norm = 0;
  gram_matvec_slices(X.n, &plan->pub.slices, &plan->pub.cols_per_slice);
  if (host_program && X.dim <= 3 && gram_match_fast(*host_program, &plan->fp, &plan->op) &&
      plan->op >= AGP_OP_SQUARED_EXPONENTIAL && plan->op <= AGP_OP_MATERN52) {
    plan->pub.path = MV_PATH_FAST;
    return;
  }
  std::memset(&plan->fp, 0, sizeof(plan->fp));
  plan->op = 0;
  if (host_program) {
    plan->need_norm = (host_program->metric_mask & ((1 << AGP_METRIC_RADIAL) | (1 << AGP_METRIC_ANGULAR))) != 0;
    if (gram_build_sop(*host_program, &plan->sop)) {
      plan->pub.path = MV_PATH_SOP;
      return;
    }
  } else {
    plan->need_norm = 1;
  }
  std::memset(&plan->sop, 0, sizeof(plan->sop));
  plan->pub.path = MV_PATH_INTERP;
}

MvPlan gram_matvec_plan(const DevProgram *host_program, const FeatView &X) {
  static thread_local MvPlanFull plan;
  mv_select(host_program, X, &plan);
  return plan.pub;
}

size_t gram_matvec_ws_elems(long long n) {
  long long S = 1, cps = 0;
  gram_matvec_slices(n, &S, &cps);
  return S > 1 ? (size_t)S * (size_t)MV_MAX_RHS * (size_t)round_up(n, 2) : 0;
}

template <int DIMP, int EVAL, int OP>
static void mv_launch_t(hipStream_t s, dim3 grid, int T, const MvArgs &a, const SopProgram &sop) {
  if (T == 1) hipLaunchKernelGGL((gram_matvec_kernel<DIMP, EVAL, OP, 1>), grid, dim3(MV_ROWS), 0, s, a, sop);
  else if (T == 4) hipLaunchKernelGGL((gram_matvec_kernel<DIMP, EVAL, OP, 4>), grid, dim3(MV_ROWS), 0, s, a, sop);
  else hipLaunchKernelGGL((gram_matvec_kernel<DIMP, EVAL, OP, MV_MAX_RHS>), grid, dim3(MV_ROWS), 0, s, a, sop);
}

template <int DIMP>
static void mv_launch_fast(hipStream_t s, dim3 grid, int T, int op, const MvArgs &a, const SopProgram &sop) {
#define AGP_MV(O) mv_launch_t<DIMP, MV_PATH_FAST, O>(s, grid, T, a, sop)
  switch (op) {
  case AGP_OP_SQUARED_EXPONENTIAL: AGP_MV(AGP_OP_SQUARED_EXPONENTIAL); break;
  case AGP_OP_EXPONENTIAL: AGP_MV(AGP_OP_EXPONENTIAL); break;
  case AGP_OP_MATERN32: AGP_MV(AGP_OP_MATERN32); break;
  default: AGP_MV(AGP_OP_MATERN52); break;
  }
#undef AGP_MV
}

int gram_matvec_chunk_width(long long remaining) { return remaining >= 5 ? MV_MAX_RHS : (remaining >= 2 ? 4 : 1); }

void launch_gram_matvec(hipStream_t s, const DevProgram *P, const DevProgram *host_program, const FeatView &X, const double *yvar,
                        const double *V, long long ldv, long long nrhs, double *out, long long ldo, double *ws, int *nan_flag, const int *go) {
  const long long n = X.n;
  if (n <= 0 || nrhs <= 0) return;
  static thread_local MvPlanFull plan;
  mv_select(host_program, X, &plan);
  const long long S = plan.pub.slices, ldp = round_up(n, 2);
  MvArgs a{};
  a.P = P;
  a.fp = plan.fp;
  a.need_norm = plan.need_norm;
  a.X = X;
  a.yvar = yvar;
  a.ldv = ldv;
  a.cps = plan.pub.cols_per_slice;
  a.nan_flag = nan_flag;
  a.go = go;
  dim3 grid((unsigned)((n + MV_ROWS - 1) / MV_ROWS), (unsigned)S);
  for (long long c0 = 0; c0 < nrhs;) {
    const int T = gram_matvec_chunk_width(nrhs - c0);
    const int cn = (int)(nrhs - c0 < T ? nrhs - c0 : T);
    a.V = V + c0 * ldv;
    a.nrhs = cn;
    if (S > 1) {
      a.out = ws;
      a.ldo = ldp;
      a.slice_stride = ldp * MV_MAX_RHS;
    } else {
      a.out = out + c0 * ldo;
      a.ldo = ldo;
      a.slice_stride = 0;
    }
    switch (plan.pub.path) {
    case MV_PATH_FAST:
      if (X.dim == 1) mv_launch_fast<1>(s, grid, T, plan.op, a, plan.sop);
      else if (X.dim == 2) mv_launch_fast<2>(s, grid, T, plan.op, a, plan.sop);
      else mv_launch_fast<3>(s, grid, T, plan.op, a, plan.sop);
      break;
    case MV_PATH_SOP:
      dispatch_dim(X.dim, [&](auto D) { mv_launch_t<decltype(D)::value, MV_PATH_SOP, 0>(s, grid, T, a, plan.sop); });
      break;
    default:
      dispatch_dim(X.dim, [&](auto D) { mv_launch_t<decltype(D)::value, MV_PATH_INTERP, 0>(s, grid, T, a, plan.sop); });
      break;
    }
    if (S > 1)
      hipLaunchKernelGGL(gram_matvec_sum_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)cn), dim3(256), 0, s, ws, ldp,
                         ldp * MV_MAX_RHS, S, n, out + c0 * ldo, ldo, go);
    c0 += cn;
  }
}

}  // namespace agp

using namespace agp;

extern "C" {

int agp_gram_matvec(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y_var, const double *V, int64_t ldv,
                    int64_t nrhs, double *out, int64_t ldo, int location) {
  if (!c || !k || !x || !V || !out) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (nrhs < 1 || ldv < n || ldo < n || (location != AGP_HOST && location != AGP_DEVICE)) return AGP_ERR_INVALID_ARGUMENT;
  if (n == 0) return AGP_OK;
  if ((n + MV_ROWS - 1) / MV_ROWS > 0x7fffffffll) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;

  // scratch: the NaN flag | y_var of a host caller | V and out of a host caller | the partial sums of the slices
  const bool host = location == AGP_HOST;
  const bool yvar_host = y_var && x->location == AGP_HOST;
  const long long ldd = round_up(n, 2);
  const size_t stage_elems = host ? 2 * (size_t)ldd * (size_t)nrhs : 0;
  const size_t part_elems = gram_matvec_ws_elems(n);
  DevMem<double> ws;
  AGP_HIP_CHECK(ctx, alloc_doubles(ws, 2 + (yvar_host ? (size_t)ldd : 0) + stage_elems + part_elems));
  int *flag = reinterpret_cast<int *>(ws.get());
  double *cur = ws.get() + 2;
  const double *yv_dev = y_var;
  if (yvar_host) {
    if ((st = vector_to_device(ctx, y_var, n, AGP_HOST, cur)) != AGP_OK) return st;
    yv_dev = cur;
    cur += ldd;
  }
  const double *Vd = V;
  double *od = out;
  long long ldvd = ldv, ldod = ldo;
  if (host) {
    double *Vs = cur;
    od = cur + (size_t)ldd * (size_t)nrhs;
    cur += stage_elems;
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(Vs, sizeof(double) * (size_t)ldd, V, sizeof(double) * (size_t)ldv, sizeof(double) * (size_t)n,
                                        (size_t)nrhs, hipMemcpyHostToDevice, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable source
    Vd = Vs;
    ldvd = ldod = ldd;
  }
  int *h_flag = static_cast<int *>(host_stage(ctx, 64));
  if (!h_flag) { ctx->last_error = "agp_gram_matvec: no pinned staging memory"; return AGP_ERR_HIP; }
  AGP_HIP_CHECK(ctx, hipMemsetAsync(flag, 0, sizeof(int), s));
  {
    TraceRange tr("agp: (k(x, x) + diag(y_var)) V without the matrix");
    launch_gram_matvec(s, dprog, &k->prog, dx.v, yv_dev, Vd, ldvd, nrhs, od, ldod, cur, flag);
  }
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (*h_flag) return AGP_ERR_NAN_INPUT;
  if (host) {  // column by column: the padding rows of the caller's block are not touched
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(out, sizeof(double) * (size_t)ldo, od, sizeof(double) * (size_t)ldd, sizeof(double) * (size_t)n,
                                        (size_t)nrhs, hipMemcpyDeviceToHost, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  }
  return AGP_OK;
}

}  // extern "C"
