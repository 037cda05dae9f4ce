// gradient.hip — exact gradient of the negative log-likelihood with respect to the covariance parameters
// (agp_nll_gradient).
//
//   dNLL / dtheta = 1/2 sum_ij W_ij dK_ij / dtheta,   W = K^-1 - alpha alpha^T,   alpha = K^-1 y
//
// The reference's tuner gets the gradient by forward differences of the log-likelihood (compute_gradient,
// tune/finite_difference.hpp:37-90): P + 1 evaluations for P parameters, accurate to the likelihood's error over eps.
// Here: one fit (build_and_factor, api.hip), R = L^-1 (forward_solve_mat_lookahead on a triangular right-hand side,
// as inverse_diagonal_device does), K^-1 = R^T R into the factor's buffer (rtr_lower_kernel below), and one contraction
// of W's lower triangle against the tangent form of the covariance program (cov_eval.h: eval_pair_tangent) that never
// stores dK / dtheta.  Cost: a fit plus ~2 N^3 / 3 flop, whatever P is; no float atomics anywhere, so two calls give
// bit-identical gradients.
#include <cstring>
#include <vector>

#include "api_internal.h"
#include "cov_eval.h"
#include "gemm_tiles.h"
#include "pub.h"

namespace agp {

// ---- C = R^T R, lower tiles, R lower triangular -----------------------------------------------------------------
// Tile (bi, bj), bi >= bj, of C sums R(k, i) R(k, j) over k >= i0 = bi * 128 only: R(k, i) = 0 for k < i.  Both
// operands are read k-major (element (row, k) at R[k + row * ldr], the TN product) through gemm_nt_sub_tile's 128 x 128
// body, with the operand pointers moved to row i0 of R and K = n - i0.  The workgroups of the first tile rows (the
// deepest products) are launched first.  Flop: N^3 / 3.  The whole diagonal tile is written; nothing reads its upper
// half.
__global__ __launch_bounds__(GEMM_THREADS, 2) void rtr_lower_kernel(GemmArgs g) {
  __shared__ double lds[2 * 2 * GK * GLD];
  // row-major enumeration of the lower tiles: id = bi (bi + 1) / 2 + bj
  const long long id = blockIdx.x;
  int bi = (int)((sqrt(8. * (double)id + 1.) - 1.) * 0.5);
  while ((long long)bi * (bi + 1) / 2 > id) --bi;
  while ((long long)(bi + 1) * (bi + 2) / 2 <= id) ++bi;
  const int bj = (int)(id - (long long)bi * (bi + 1) / 2);
  const long long k0 = (long long)bi * GT;
  GemmArgs t = g;
  t.A = g.A + k0;
  t.B = g.B + k0;
  t.K = g.K - k0;
  gemm_nt_sub_tile<true, true, true>(t, bi, bj, lds);
}

void launch_rtr_lower(hipStream_t s, const double *R, long long ldr, long long n, double *C, long long ldc) {
  if (n <= 0) return;
  GemmArgs g;
  g.C = C; g.ldc = ldc; g.A = R; g.lda = ldr; g.B = R; g.ldb = ldr;
  g.M = n; g.N = n; g.K = n; g.tri = 1;
  g.ntr = g.ntc = (int)((n + GT - 1) / GT);
  g.assign = 1;  // C = + A B^T, C not read
  const long long tiles = (long long)g.ntr * (g.ntr + 1) / 2;
  hipLaunchKernelGGL(rtr_lower_kernel, dim3((unsigned)tiles), dim3(GEMM_THREADS), 0, s, g);
}

// ---- contraction: partial[tile][g] = sum over the tile's pairs i >= j of w_ij dk_ij / dslot_g ------------------------
constexpr int GRAD_GROUP = 4;   // slots per walk of the tangent program (K^-1 is read ceil(P / GRAD_GROUP) times)
constexpr int CT = 64;          // contraction tile edge
constexpr int CT_THREADS = 256;

struct ContractArgs {
  TangentSlots<GRAD_GROUP> slots;
  const double *tang[GRAD_GROUP];  // AGP_OP_SCALING slot g: its tangent column (n values), else nullptr
  const double *C;                 // K^-1, lower triangle
  long long ldc;
  const double *alpha;
  double *partial;                 // [tile][GRAD_GROUP]
};

template <int DIMP>
__device__ __forceinline__ void load_point(const FeatView &X, long long i, bool need_norm, Point<DIMP> &p) {
  double nn = 0.;
#pragma unroll
  for (int d = 0; d < DIMP; ++d) {
    p.c[d] = d < X.dim ? X.coords[i * X.dim + d] : 0.;
    nn += p.c[d] * p.c[d];
  }
  p.norm = need_norm ? sqrt(nn) : 0.;
#pragma unroll
  for (int k = 0; k < AGP_MAX_SCALE_COLUMNS; ++k) p.s[k] = k < X.nsc ? X.scales[(long long)k * scale_stride(X) + i] : 0.;
  p.id = X.ids ? X.ids[i] : -1;
}

// One workgroup per 64 x 64 lower tile of K^-1; lane = row i (coalesced reads of K^-1), each wave walks 16 columns j,
// whose point is the same for the whole wave.
template <int DIMP>
__global__ __launch_bounds__(CT_THREADS) void nll_grad_contract_kernel(const DevProgram *__restrict__ P, FeatView X,
                                                                       ContractArgs a) {
  const long long id = blockIdx.x;
  int bi = (int)((sqrt(8. * (double)id + 1.) - 1.) * 0.5);
  while ((long long)bi * (bi + 1) / 2 > id) --bi;
  while ((long long)(bi + 1) * (bi + 2) / 2 <= id) ++bi;
  const int bj = (int)(id - (long long)bi * (bi + 1) / 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n = X.n;
  const long long i = (long long)bi * CT + lane;
  const bool need_norm = (P->metric_mask & ((1 << AGP_METRIC_RADIAL) | (1 << AGP_METRIC_ANGULAR))) != 0;
  double acc[GRAD_GROUP];
#pragma unroll
  for (int g = 0; g < GRAD_GROUP; ++g) acc[g] = 0.;
  if (i < n) {
    Point<DIMP> x;
    load_point<DIMP>(X, i, need_norm, x);
    double tx[GRAD_GROUP];
#pragma unroll
    for (int g = 0; g < GRAD_GROUP; ++g) tx[g] = a.tang[g] ? a.tang[g][i] : 0.;
    const double ai = a.alpha[i];
    for (int c = wave; c < CT; c += CT_THREADS / 64) {
      const long long j = (long long)bj * CT + c;
      if (j >= n || j > i) continue;
      Point<DIMP> y;
      load_point<DIMP>(X, j, need_norm, y);
      double ty[GRAD_GROUP];
#pragma unroll
      for (int g = 0; g < GRAD_GROUP; ++g) ty[g] = a.tang[g] ? a.tang[g][j] : 0.;
      const double w = (i == j ? 1. : 2.) * (a.C[i + j * a.ldc] - ai * a.alpha[j]);
      double dk[GRAD_GROUP];
      eval_pair_tangent<DIMP, GRAD_GROUP>(P, a.slots, x, y, tx, ty, X.ids != nullptr, X.meas != 0, dk);
#pragma unroll
      for (int g = 0; g < GRAD_GROUP; ++g) acc[g] += w * dk[g];
    }
  }
  // fixed-order reduction: butterfly inside the wave, then the four waves in order
  __shared__ double red[CT_THREADS / 64][GRAD_GROUP];
#pragma unroll
  for (int g = 0; g < GRAD_GROUP; ++g) {
    double v = acc[g];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][g] = v;
  }
  __syncthreads();
  if (threadIdx.x < GRAD_GROUP) {
    const int g = threadIdx.x;
    double v = red[0][g];
#pragma unroll
    for (int w = 1; w < CT_THREADS / 64; ++w) v += red[w][g];
    a.partial[id * GRAD_GROUP + g] = v;
  }
}

// out[base + g] = scale * sum over tiles of partial[tile][g], in a fixed order; one workgroup per slot of the group
__global__ __launch_bounds__(256) void nll_grad_reduce_kernel(const double *__restrict__ partial, long long tiles, int count,
                                                              double scale, double *__restrict__ out) {
  const int g = blockIdx.x;
  if (g >= count) return;
  double v = 0.;
  for (long long t = threadIdx.x; t < tiles; t += 256) v += partial[t * GRAD_GROUP + g];
  __shared__ double red[256];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[g] = scale * red[0];
}

static long long contract_tiles(long long n) {
  const long long t = (n + CT - 1) / CT;
  return t * (t + 1) / 2;
}

static void launch_contract(hipStream_t s, const DevProgram *P, const FeatView &X, const ContractArgs &a, long long tiles) {
  const dim3 grid((unsigned)tiles), block(CT_THREADS);
  const int dim = X.dim;
  if (dim == 1) hipLaunchKernelGGL(nll_grad_contract_kernel<1>, grid, block, 0, s, P, X, a);
  else if (dim == 2) hipLaunchKernelGGL(nll_grad_contract_kernel<2>, grid, block, 0, s, P, X, a);
  else if (dim == 3) hipLaunchKernelGGL(nll_grad_contract_kernel<3>, grid, block, 0, s, P, X, a);
  else if (dim == 4) hipLaunchKernelGGL(nll_grad_contract_kernel<4>, grid, block, 0, s, P, X, a);
  else hipLaunchKernelGGL(nll_grad_contract_kernel<8>, grid, block, 0, s, P, X, a);
}

}  // namespace agp

using namespace agp;

// ---- slot validation: a leaf node and a parameter index the leaf has ----------------------------------------------
static int check_slots(const agp_kernel *k, int n_slots, const agp_gradient_slot *slots, int *n_tangent_columns) {
  int ntc = 0;
  for (int s = 0; s < n_slots; ++s) {
    const int node = slots[s].node, param = slots[s].param;
    if (node < 0 || node >= k->prog.n_nodes || param < 0) return AGP_ERR_INVALID_ARGUMENT;
    const agp_kernel_node &nd = k->prog.nodes[node];
    int n_params;
    if (nd.op >= AGP_OP_SQUARED_EXPONENTIAL && nd.op <= AGP_OP_MATERN52) n_params = 2;
    else if (nd.op == AGP_OP_CONSTANT || nd.op == AGP_OP_INDEPENDENT_NOISE || nd.op == AGP_OP_NUGGET) n_params = 1;
    else if (nd.op == AGP_OP_POLYNOMIAL) n_params = nd.order + 1;
    else if (nd.op == AGP_OP_SCALING) n_params = -1;  // any tangent column
    else return AGP_ERR_INVALID_ARGUMENT;             // not a leaf
    if (n_params >= 0 && param >= n_params) return AGP_ERR_INVALID_ARGUMENT;
    if (n_params < 0 && param + 1 > ntc) ntc = param + 1;
  }
  *n_tangent_columns = ntc;
  return AGP_OK;
}

extern "C" {

int agp_nll_gradient(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                     int n_slots, const agp_gradient_slot *slots, const double *tangents, int64_t ldt, double *nll,
                     double *grad_nll, double *information) {
  if (!c || !k || !x || !y || !nll) return AGP_ERR_INVALID_ARGUMENT;
  if (n_slots < 0 || n_slots > AGP_MAX_GRADIENT_SLOTS || (n_slots > 0 && (!slots || !grad_nll))) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  int ntc = 0;
  if ((st = check_slots(k, n_slots, slots, &ntc)) != AGP_OK) return st;
  if (ntc > 0 && (!tangents || ldt < n)) return AGP_ERR_INVALID_ARGUMENT;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  hipStream_t s = ctx->stream;

  // ws_A: [A | invd | z | yvar], as agp_nll
  const long long lda = factor_ld(n);
  const long long nblk = (n + NB - 1) / NB;
  const size_t a_bytes = sizeof(double) * (size_t)lda * (size_t)n;
  const size_t aux = sizeof(double) * ((size_t)nblk * (36 * MB * MB) + 2 * (size_t)round_up(n, 2));
  if ((st = ensure_ws(ctx, &ctx->ws_A, &ctx->ws_A_bytes, a_bytes + aux)) != AGP_OK) return st;
  double *A = ctx->ws_A;
  double *invd = A + (size_t)lda * (size_t)n;
  double *z = invd + (size_t)nblk * (36 * MB * MB);
  double *yvar_d = y_var ? z + round_up(n, 2) : nullptr;
  // ws_aux: [R | back-substitution scratch | partials | gradient | tangent columns]
  const long long tiles = contract_tiles(n);
  const size_t r_elems = (size_t)lda * (size_t)n, bs_elems = backsolve_ws_elems(n);
  const size_t part_elems = (size_t)tiles * GRAD_GROUP, grad_elems = (size_t)round_up(AGP_MAX_GRADIENT_SLOTS, 2);
  const bool tang_copy = ntc > 0 && x->location == AGP_HOST;
  const size_t tang_elems = tang_copy ? (size_t)round_up(n, 2) * (size_t)ntc : 0;
  if ((st = ensure_ws(ctx, &ctx->ws_aux, &ctx->ws_aux_bytes,
                      sizeof(double) * (r_elems + bs_elems + part_elems + grad_elems + tang_elems))) != AGP_OK)
    return st;
  double *R = ctx->ws_aux, *bs_ws = R + r_elems, *partial = bs_ws + bs_elems, *grad_d = partial + part_elems;
  const double *tang_d = tangents;
  long long ldt_d = ldt;
  if (tang_copy) {
    double *t = grad_d + grad_elems;
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(t, sizeof(double) * (size_t)round_up(n, 2), tangents, sizeof(double) * (size_t)ldt,
                                        sizeof(double) * (size_t)n, (size_t)ntc, hipMemcpyHostToDevice, s));
    tang_d = t;
    ldt_d = round_up(n, 2);
  }

  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  if ((st = vector_to_device(ctx, y, n, x->location, z)) != AGP_OK) return st;
  if (y_var && (st = vector_to_device(ctx, y_var, n, x->location, yvar_d)) != AGP_OK) return st;
  FeatView xm = dx.v;
  xm.meas = 1;
  // the fit: A = L, z = L^-1 y, flags and log det (api.hip: build_and_factor via agp_nll's path)
  st = build_and_factor_nll(ctx, dprog, &k->prog, xm, A, lda, invd, z, yvar_d);
  if (st == AGP_OK) st = status_from_flags(ctx);
  if (st != AGP_OK) return st;
  const bool prof = ctx->profiling;
  // y^T K^-1 y = z^T z, then alpha = L^-T z in place
  launch_dot(s, z, z, n, ctx->d_scalars + 1);
  backward_solve_vec_any(s, A, n, lda, invd, z, bs_ws);
  const double *alpha = z;
  // R = L^-1 (triangular right-hand side), K^-1 = R^T R over L
  launch_set_identity(s, R, lda, n);
  forward_solve_mat_lookahead(ctx, A, n, lda, invd, R, n, lda, /*rhs_lower=*/true);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[3], s));
  launch_rtr_lower(s, R, lda, n, A, lda);
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[4], s));
  // the contraction, GRAD_GROUP slots per pass
  for (int g0 = 0; g0 < n_slots; g0 += GRAD_GROUP) {
    ContractArgs ca;
    ca.C = A; ca.ldc = lda; ca.alpha = alpha; ca.partial = partial;
    const int cnt = n_slots - g0 < GRAD_GROUP ? n_slots - g0 : GRAD_GROUP;
    for (int g = 0; g < GRAD_GROUP; ++g) {
      const bool used = g < cnt;
      const int node = used ? slots[g0 + g].node : -1, param = used ? slots[g0 + g].param : 0;
      ca.slots.node[g] = node;
      ca.slots.param[g] = param;
      ca.tang[g] = (used && k->prog.nodes[node].op == AGP_OP_SCALING) ? tang_d + (size_t)param * (size_t)ldt_d : nullptr;
    }
    launch_contract(s, dprog, xm, ca, tiles);
    hipLaunchKernelGGL(nll_grad_reduce_kernel, dim3(GRAD_GROUP), dim3(256), 0, s, partial, tiles, cnt, 0.5, grad_d + g0);
  }
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[5], s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_slots > 0) AGP_HIP_CHECK(ctx, hipMemcpyAsync(grad_nll, grad_d, sizeof(double) * (size_t)n_slots, hipMemcpyDeviceToHost, s));
  if (information) AGP_HIP_CHECK(ctx, hipMemcpyAsync(information, alpha, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  *nll = 0.5 * (2. * ctx->h_scalars[0] + ctx->h_scalars[1] + (double)n * std::log(2 * M_PI));  // likelihood.hpp:46
  if (prof) {
    // stage 2: alpha and R = L^-1 (from the end of the factorisation), 6: R^T R, 7: contraction
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->stage_ev[2], ctx->stage_ev[3]);
    ctx->stage_ms[2] = ms;
    (void)hipEventElapsedTime(&ms, ctx->stage_ev[3], ctx->stage_ev[4]);
    ctx->stage_ms[6] = ms;
    (void)hipEventElapsedTime(&ms, ctx->stage_ev[4], ctx->stage_ev[5]);
    ctx->stage_ms[7] = ms;
  }
  return AGP_OK;
}

}  // extern "C"
