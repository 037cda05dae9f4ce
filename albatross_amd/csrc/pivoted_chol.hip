// pivoted_chol.hip — greedy pivoted (partial) Cholesky factorisation of K = k(x, x) with K evaluated column by column
// and never stored: agp_pivoted_cholesky (include/albatross_amd.h).
//
//   d_i = K_ii;  step j: p = argmax of d over the unselected rows (lowest index on equal values), stop when
//   d_p <= rel_tol max_i K_ii or d_p <= 0, else  L_ij = (k(x_i, x_p) - sum_{t<j} L_it L_pt) / sqrt(d_p),
//   d_i = max(d_i - L_ij^2, 0),  L_pj = sqrt(d_p) and d_p = 0 exactly,  L_ij = 0 exactly for rows selected before.
//
// ONE launch per step.  A workgroup is one wave that owns PC_TILE consecutive rows, two per lane: L is column-major, so a
// lane reads its two rows of a column with one 16-byte load and a wave reads 1 KiB of the column per instruction; the t
// loop keeps PC_UNROLL such loads in flight per lane.  The pivot's row of L is gathered into LDS once per workgroup, in
// chunks of PC_CHUNK columns; the pivot's point is read by every lane from one address.  The kernel is bound by the
// HBM reads of L (n j doubles in step j), the pair evaluation is one k(x_i, x_p) per row and step.
//
// The argmax travels with the step: every workgroup leaves the (value, index) maximum of its tile's new d in one of two
// tables that are used in turn, and every workgroup of the NEXT launch reduces the whole table before anything else (the
// order "larger value, then lower index" is total, so every workgroup finds the same pivot whatever the order of the
// reduction).  The kernel boundary is the only synchronisation: no grid barrier, no spinning, no float atomics.  The stop
// decision is each workgroup's own (they all see the same maximum); workgroup 0 records it - the flag and the rank,
// plain vector stores - for the launches behind, which return at once, and for the host, which looks at the flag
// once per PC_HOST_LOOK steps while the next PC_HOST_LOOK are already queued.
//
// Entry (i, p) of a column has the bits agp_gram gives it: the same evaluator (radial fast path, sum of products or the
// postfix interpreter, chosen as gram.hip chooses) and the same argument order, compiled without FMA contraction.
#include <cmath>
#include <cstring>
#include "api_internal.h"
#include "gram_fast.h"
#include "trace.h"

namespace agp {

constexpr int PC_THREADS = 64;                       // one wave per workgroup
constexpr int PC_ROWS_PER_LANE = 2;                  // one 16-byte load per lane and column
constexpr int PC_TILE = PC_THREADS * PC_ROWS_PER_LANE;  // rows of a workgroup
constexpr int PC_UNROLL = 8;                         // independent column loads in flight per lane
constexpr int PC_CHUNK = 512;                        // columns of the pivot's row staged in LDS at a time
constexpr int PC_HOST_LOOK = 64;                     // steps between two looks of the host at the stop flag
constexpr int PC_TRACE_THREADS = 1024;

enum { PC_EVAL_FAST = 0, PC_EVAL_SOP = 1, PC_EVAL_INTERP = 2 };

struct PcPartial {
  double v;
  long long i;
};

struct PcCtrl {
  int stopped;     // a step met the stop rule: the launches behind it return at once
  int nan;         // a NaN on the diagonal or in a column
  long long rank;  // steps carried out (max_rank unless a step stopped)
  double d0;       // max_i K_ii
};

struct PcArgs {
  const DevProgram *P;
  FastParams fp;
  int op;
  int need_norm;
  FeatView X;
  double *L;
  long long ldl;
  double *d;
  unsigned char *sel;
  PcPartial *tab;  // two tables of nblk entries
  long long nblk;
  PcCtrl *ctrl;
  long long *pivots;
  double rel_tol;
  long long max_rank;
  const double *diag;  // n values added to the diagonal of K (the matrix-free fit's y_var), or nullptr
};

// "larger value, then lower index": a total order, NaN never wins
__device__ __forceinline__ bool pc_better(double va, long long ia, double vb, long long ib) {
  return va > vb || (va == vb && ia < ib);
}

__device__ __forceinline__ void pc_wave_argmax(double &v, long long &i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const long long oi = __shfl_xor(i, off, 64);
    if (pc_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

constexpr long long PC_NO_INDEX = 0x7fffffffffffffffll;

template <int DIMP, int EVAL>
__device__ __forceinline__ double pc_eval(const PcArgs &a, const SopProgram &sop, const Point<DIMP> &x, const Point<DIMP> &y,
                                          bool swapped, bool have_ids, bool meas) {
  if (EVAL == PC_EVAL_FAST) {  // gram_fast.h: gram_fast_body, one entry
    double s2 = 0.;
#pragma unroll
    for (int d = 0; d < DIMP; ++d) {
      const double t = x.c[d] - y.c[d];
      s2 += t * t;
    }
    double v;
    if (a.op == AGP_OP_SQUARED_EXPONENTIAL) v = radial_fast<AGP_OP_SQUARED_EXPONENTIAL>(s2, a.fp);
    else if (a.op == AGP_OP_EXPONENTIAL) v = radial_fast<AGP_OP_EXPONENTIAL>(s2, a.fp);
    else if (a.op == AGP_OP_MATERN32) v = radial_fast<AGP_OP_MATERN32>(s2, a.fp);
    else v = radial_fast<AGP_OP_MATERN52>(s2, a.fp);
    if (a.fp.has_noise) {
      bool e = true;
#pragma unroll
      for (int d = 0; d < DIMP; ++d) e = e && (x.c[d] == y.c[d]);
      if (have_ids) e = x.id == y.id;
      const bool noise_on = !a.fp.noise_meas_only || meas;
      v = v + ((noise_on && e) ? a.fp.noise_var : 0.);
    }
    return v;
  } else if (EVAL == PC_EVAL_SOP) {
    return eval_sop<DIMP>(sop, x, y, swapped, have_ids, meas);
  } else {
    return eval_pair<DIMP>(a.P, x, y, swapped, have_ids, meas);
  }
}

// d_i = K_ii, nothing selected, the first table of partial maxima
template <int DIMP, int EVAL>
__global__ __launch_bounds__(PC_THREADS) void pc_init_kernel(PcArgs a, SopProgram sop) {
  const long long n = a.X.n;
  const bool have_ids = a.X.ids != nullptr, meas = a.X.meas != 0;
  double bv = -1.;
  long long bi = PC_NO_INDEX;
  bool saw_nan = false;
#pragma unroll
  for (int h = 0; h < PC_ROWS_PER_LANE; ++h) {
    const long long r = (long long)blockIdx.x * PC_TILE + PC_ROWS_PER_LANE * threadIdx.x + h;
    if (r < n) {
      Point<DIMP> x;
      load_point<DIMP>(a.X, r, a.need_norm != 0, x);
      double v = pc_eval<DIMP, EVAL>(a, sop, x, x, false, have_ids, meas);
      if (a.diag) v += a.diag[r];  // (off the diagonal the columns are those of K: a step never reads entry (p, p) of its column)
      saw_nan = saw_nan || v != v;
      a.d[r] = v;
      a.sel[r] = 0;
      if (pc_better(v, r, bv, bi)) { bv = v; bi = r; }
    }
  }
  pc_wave_argmax(bv, bi);
  if (threadIdx.x == 0) {
    a.tab[blockIdx.x].v = bv;
    a.tab[blockIdx.x].i = bi;
    if (blockIdx.x == 0) a.ctrl->rank = a.max_rank;
  }
  if (saw_nan) atomicOr(&a.ctrl->nan, 1);
}

template <int DIMP, int EVAL>
__global__ __launch_bounds__(PC_THREADS) void pc_step_kernel(PcArgs a, SopProgram sop, long long j) {
  __shared__ double lp[PC_CHUNK];
  PcCtrl *const ctrl = a.ctrl;
  if (ctrl->stopped | ctrl->nan) return;  // decided by an earlier launch
  // ---- the pivot: the maximum of the table the previous launch left ----
  const PcPartial *const tab = a.tab + (size_t)(j & 1) * (size_t)a.nblk;
  double pv = -1.;
  long long p = PC_NO_INDEX;
  for (long long t = threadIdx.x; t < a.nblk; t += PC_THREADS) {
    const double v = tab[t].v;
    const long long i = tab[t].i;
    if (pc_better(v, i, pv, p)) { pv = v; p = i; }
  }
  pc_wave_argmax(pv, p);
  const double d0 = j == 0 ? pv : ctrl->d0;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (!(pv > a.rel_tol * d0) || !(pv > 0.)) {
    if (lead) {
      ctrl->rank = j;
      ctrl->stopped = 1;
    }
    return;
  }
  if (lead) {
    a.pivots[j] = p;
    if (j == 0) ctrl->d0 = pv;
  }
  const double root = sqrt(pv);
  const long long n = a.X.n, ldl = a.ldl;
  const long long r0 = (long long)blockIdx.x * PC_TILE + PC_ROWS_PER_LANE * threadIdx.x, r1 = r0 + 1;
  const bool in0 = r0 < n, in1 = r1 < n;
  const bool have_ids = a.X.ids != nullptr, meas = a.X.meas != 0;
  // ---- the column of K: k(x_i, x_p) as the symmetric Gram matrix holds it (evaluated for i >= p, mirrored) ----
  double c0 = 0., c1 = 0.;
  {
    Point<DIMP> y, x;
    load_point<DIMP>(a.X, p, a.need_norm != 0, y);
    load_point<DIMP>(a.X, in0 ? r0 : n - 1, a.need_norm != 0, x);
    c0 = pc_eval<DIMP, EVAL>(a, sop, x, y, r0 < p, have_ids, meas);
    load_point<DIMP>(a.X, in1 ? r1 : n - 1, a.need_norm != 0, x);
    c1 = pc_eval<DIMP, EVAL>(a, sop, x, y, r1 < p, have_ids, meas);
  }
  // ---- sum_{t<j} L_it L_pt, t = 0, 1, ... ----
  double s0 = 0., s1 = 0.;
  const bool wide = ((ldl & 1) == 0) && ((reinterpret_cast<uintptr_t>(a.L) & 15) == 0);
  for (long long t0 = 0; t0 < j; t0 += PC_CHUNK) {
    const int cnt = (int)(j - t0 < PC_CHUNK ? j - t0 : PC_CHUNK);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += PC_THREADS) lp[t] = a.L[(t0 + t) * ldl + p];
    __syncthreads();
    const double *col = a.L + t0 * ldl + r0;
    int t = 0;
    if (wide && in1) {
      for (; t + PC_UNROLL <= cnt; t += PC_UNROLL) {
        double2 v[PC_UNROLL];
#pragma unroll
        for (int u = 0; u < PC_UNROLL; ++u) v[u] = *reinterpret_cast<const double2 *>(col + (long long)(t + u) * ldl);
#pragma unroll
        for (int u = 0; u < PC_UNROLL; ++u) {
          s0 += v[u].x * lp[t + u];
          s1 += v[u].y * lp[t + u];
        }
      }
      for (; t < cnt; ++t) {
        const double2 v = *reinterpret_cast<const double2 *>(col + (long long)t * ldl);
        s0 += v.x * lp[t];
        s1 += v.y * lp[t];
      }
    } else if (in0) {
      for (; t + PC_UNROLL <= cnt; t += PC_UNROLL) {
        double va[PC_UNROLL], vb[PC_UNROLL];
#pragma unroll
        for (int u = 0; u < PC_UNROLL; ++u) {
          va[u] = col[(long long)(t + u) * ldl];
          vb[u] = in1 ? col[(long long)(t + u) * ldl + 1] : 0.;
        }
#pragma unroll
        for (int u = 0; u < PC_UNROLL; ++u) {
          s0 += va[u] * lp[t + u];
          s1 += vb[u] * lp[t + u];
        }
      }
      for (; t < cnt; ++t) {
        s0 += col[(long long)t * ldl] * lp[t];
        if (in1) s1 += col[(long long)t * ldl + 1] * lp[t];
      }
    }
  }
  // ---- the new column, the new d, the tile's maximum ----
  double l0 = 0., l1 = 0., bv = -1.;
  long long bi = PC_NO_INDEX;
  bool saw_nan = false;
  if (in0) {
    const bool was = a.sel[r0] != 0;
    double dn = 0.;
    if (r0 == p) {
      l0 = root;
      a.sel[r0] = 1;
    } else if (!was) {
      l0 = (c0 - s0) / root;
      saw_nan = saw_nan || l0 != l0;
      dn = fmax(a.d[r0] - l0 * l0, 0.);
      if (pc_better(dn, r0, bv, bi)) { bv = dn; bi = r0; }
    }
    a.d[r0] = dn;
  }
  if (in1) {
    const bool was = a.sel[r1] != 0;
    double dn = 0.;
    if (r1 == p) {
      l1 = root;
      a.sel[r1] = 1;
    } else if (!was) {
      l1 = (c1 - s1) / root;
      saw_nan = saw_nan || l1 != l1;
      dn = fmax(a.d[r1] - l1 * l1, 0.);
      if (pc_better(dn, r1, bv, bi)) { bv = dn; bi = r1; }
    }
    a.d[r1] = dn;
  }
  double *dst = a.L + j * ldl + r0;
  if (in1) {
    if (wide) *reinterpret_cast<double2 *>(dst) = make_double2(l0, l1);
    else { dst[0] = l0; dst[1] = l1; }
  } else if (in0) {
    dst[0] = l0;
  }
  pc_wave_argmax(bv, bi);
  if (threadIdx.x == 0) {
    PcPartial *const out = a.tab + (size_t)((j + 1) & 1) * (size_t)a.nblk;
    out[blockIdx.x].v = bv;
    out[blockIdx.x].i = bi;
  }
  if (saw_nan) atomicOr(&ctrl->nan, 1);
}

// sum_i d_i in a fixed order: thread t adds d_t, d_{t + T}, ... and the T sums meet in a tree
__global__ __launch_bounds__(PC_TRACE_THREADS) void pc_trace_kernel(const double *d, long long n, double *out) {
  __shared__ double red[PC_TRACE_THREADS];
  double s = 0.;
  for (long long i = threadIdx.x; i < n; i += PC_TRACE_THREADS) s += d[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = PC_TRACE_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

bool gram_build_sop(const DevProgram &H, SopProgram *out);  // gram.hip

struct PcLaunch {
  void (*init)(hipStream_t, const PcArgs &, const SopProgram &, unsigned);
  void (*step)(hipStream_t, const PcArgs &, const SopProgram &, unsigned, long long);
};

template <int DIMP, int EVAL>
static PcLaunch pc_launchers() {
  PcLaunch l;
  l.init = [](hipStream_t s, const PcArgs &a, const SopProgram &sop, unsigned grid) {
    hipLaunchKernelGGL((pc_init_kernel<DIMP, EVAL>), dim3(grid), dim3(PC_THREADS), 0, s, a, sop);
  };
  l.step = [](hipStream_t s, const PcArgs &a, const SopProgram &sop, unsigned grid, long long j) {
    hipLaunchKernelGGL((pc_step_kernel<DIMP, EVAL>), dim3(grid), dim3(PC_THREADS), 0, s, a, sop, j);
  };
  return l;
}

// The evaluator agp_gram uses for the full symmetric matrix of these features (gram.hip: gram_select_path - the radial
// fast path, the pair-2 kernel with the arithmetic of the sum of products, the sum of products, the interpreter)
static PcLaunch pc_select(const DevProgram &host_program, int dim, PcArgs *a, SopProgram *sop) {
  std::memset(sop, 0, sizeof(*sop));
  a->op = 0;
  if (dim <= 3 && gram_match_fast(host_program, &a->fp, &a->op) && a->op >= AGP_OP_SQUARED_EXPONENTIAL && a->op <= AGP_OP_MATERN52) {
    a->need_norm = 0;
    if (dim == 1) return pc_launchers<1, PC_EVAL_FAST>();
    if (dim == 2) return pc_launchers<2, PC_EVAL_FAST>();
    return pc_launchers<3, PC_EVAL_FAST>();
  }
  std::memset(&a->fp, 0, sizeof(a->fp));
  a->op = 0;
  a->need_norm = (host_program.metric_mask & ((1 << AGP_METRIC_RADIAL) | (1 << AGP_METRIC_ANGULAR))) != 0;
  PcLaunch l{};
  if (gram_build_sop(host_program, sop)) {
    dispatch_dim(dim, [&](auto D) { l = pc_launchers<decltype(D)::value, PC_EVAL_SOP>(); });
  } else {
    std::memset(sop, 0, sizeof(*sop));
    dispatch_dim(dim, [&](auto D) { l = pc_launchers<decltype(D)::value, PC_EVAL_INTERP>(); });
  }
  return l;
}

}  // namespace agp

using namespace agp;

// agp_pivoted_cholesky of K + diag(diag_dev) (n device values, or nullptr: K itself - the public entry, whose bits this
// leaves as they were); d0 (optional): the largest diagonal entry.  iterative.hip builds its preconditioner with it.
int pivoted_cholesky_impl(agp_context *c, const agp_kernel *k, const agp_features *x, const double *diag_dev, int64_t max_rank,
                          double rel_tol, int64_t *pivots, int64_t *rank, double *L, int64_t ldl, double *residual_diag, int location,
                          double *trace_residual, double *d0_out) {
  if (!c || !k || !x || !pivots || !rank) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (max_rank < 1 || max_rank > n || !(rel_tol >= 0.) || (L && ldl < n) || (location != AGP_HOST && location != AGP_DEVICE))
    return AGP_ERR_INVALID_ARGUMENT;
  const long long nblk = (n + PC_TILE - 1) / PC_TILE;
  if (nblk > 0x7fffffffll) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;

  // O(n) scratch: d | the two tables | the pivots | control block and the trace | the selected marks
  const size_t tab_elems = 2 * (size_t)nblk * (sizeof(PcPartial) / sizeof(double));
  const size_t ctrl_elems = (sizeof(PcCtrl) + sizeof(double) - 1) / sizeof(double) + 1;
  const size_t sel_elems = ((size_t)n + sizeof(double) - 1) / sizeof(double);
  DevMem<double> ws;
  AGP_HIP_CHECK(ctx, alloc_doubles(ws, (size_t)n + tab_elems + (size_t)max_rank + ctrl_elems + sel_elems));
  double *d = ws.get();
  PcPartial *tab = reinterpret_cast<PcPartial *>(d + n);
  long long *piv_dev = reinterpret_cast<long long *>(d + n + tab_elems);
  PcCtrl *ctrl = reinterpret_cast<PcCtrl *>(piv_dev + max_rank);
  double *trace_dev = reinterpret_cast<double *>(ctrl) + (ctrl_elems - 1);
  unsigned char *sel = reinterpret_cast<unsigned char *>(reinterpret_cast<double *>(ctrl) + ctrl_elems);
  // the factor: the caller's block when it is on the device, else a slab of the call
  DevMem<double> slab;
  double *Ldev = L;
  long long ldd = ldl;
  if (!L || location == AGP_HOST) {
    ldd = round_up(n, 2);
    AGP_HIP_CHECK(ctx, alloc_doubles(slab, (size_t)ldd * (size_t)max_rank));
    Ldev = slab.get();
  }
  // pinned: two looks at the stop flag in flight, the control block, the trace, the pivots
  const size_t stage_bytes = 2 * sizeof(int) + sizeof(PcCtrl) + sizeof(double) + sizeof(long long) * (size_t)max_rank + 64;
  char *stage = static_cast<char *>(host_stage(ctx, stage_bytes));
  if (!stage) { ctx->last_error = "agp_pivoted_cholesky: no pinned staging memory"; return AGP_ERR_HIP; }
  int *h_look = reinterpret_cast<int *>(stage);
  PcCtrl *h_ctrl = reinterpret_cast<PcCtrl *>(stage + 16);
  double *h_trace = reinterpret_cast<double *>(stage + 16 + sizeof(PcCtrl));
  long long *h_piv = reinterpret_cast<long long *>(h_trace + 1);

  PcArgs a{};
  a.P = dprog;
  a.X = dx.v;
  a.L = Ldev;
  a.ldl = ldd;
  a.d = d;
  a.sel = sel;
  a.tab = tab;
  a.nblk = nblk;
  a.ctrl = ctrl;
  a.pivots = piv_dev;
  a.rel_tol = rel_tol;
  a.max_rank = max_rank;
  a.diag = diag_dev;
  static thread_local SopProgram sop;
  const PcLaunch launch = pc_select(k->prog, x->dim, &a, &sop);

  const bool prof = ctx->profiling;
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[0], s));
  {
    TraceRange tr("agp: pivoted Cholesky of k(x, x), one launch per step");
    AGP_HIP_CHECK(ctx, hipMemsetAsync(ctrl, 0, sizeof(PcCtrl), s));
    launch.init(s, a, sop, (unsigned)nblk);
    // PC_HOST_LOOK steps, a copy of the flag and an event; the host waits for the event of block b - 1 with block b
    // queued behind it, so the device does not run dry while the host looks
    hipEvent_t ev[2] = {ctx->ev_a, ctx->ev_b};
    long long blocks = 0;
    bool stopped = false;
    for (long long j0 = 0; j0 < max_rank && !stopped; j0 += PC_HOST_LOOK, ++blocks) {
      const long long j1 = j0 + PC_HOST_LOOK < max_rank ? j0 + PC_HOST_LOOK : max_rank;
      for (long long j = j0; j < j1; ++j) launch.step(s, a, sop, (unsigned)nblk, j);
      if (j1 == max_rank) break;
      AGP_HIP_CHECK(ctx, hipMemcpyAsync(&h_look[blocks & 1], &ctrl->stopped, sizeof(int), hipMemcpyDeviceToHost, s));
      AGP_HIP_CHECK(ctx, hipEventRecord(ev[blocks & 1], s));
      if (blocks >= 1) {
        AGP_HIP_CHECK(ctx, hipEventSynchronize(ev[(blocks - 1) & 1]));
        stopped = h_look[(blocks - 1) & 1] != 0;
      }
    }
    if (trace_residual) hipLaunchKernelGGL(pc_trace_kernel, dim3(1), dim3(PC_TRACE_THREADS), 0, s, d, n, trace_dev);
  }
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_ctrl, ctrl, sizeof(PcCtrl), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_piv, piv_dev, sizeof(long long) * (size_t)max_rank, hipMemcpyDeviceToHost, s));
  if (trace_residual) AGP_HIP_CHECK(ctx, hipMemcpyAsync(h_trace, trace_dev, sizeof(double), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->stage_ev[0], ctx->stage_ev[1]) == hipSuccess) ctx->stage_ms[10] = ms;
  }
  if (h_ctrl->nan) return AGP_ERR_NAN_INPUT;
  const long long r = h_ctrl->rank;
  if (L && location == AGP_HOST && r > 0) {
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(L, sizeof(double) * (size_t)ldl, Ldev, sizeof(double) * (size_t)ldd, sizeof(double) * (size_t)n,
                                        (size_t)r, hipMemcpyDeviceToHost, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  }
  if (residual_diag && (st = copy_out(ctx, d, n, residual_diag, location)) != AGP_OK) return st;
  for (long long j = 0; j < r; ++j) pivots[j] = h_piv[j];
  *rank = r;
  if (trace_residual) *trace_residual = *h_trace;
  if (d0_out) *d0_out = h_ctrl->d0;
  return AGP_OK;
}

extern "C" {

int agp_pivoted_cholesky(agp_context *c, const agp_kernel *k, const agp_features *x, int64_t max_rank, double rel_tol,
                         int64_t *pivots, int64_t *rank, double *L, int64_t ldl, double *residual_diag, int location,
                         double *trace_residual) {
  return pivoted_cholesky_impl(c, k, x, nullptr, max_rank, rel_tol, pivots, rank, L, ldl, residual_diag, location, trace_residual,
                               nullptr);
}

}  // extern "C"
