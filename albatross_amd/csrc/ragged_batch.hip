// ragged_batch.hip — the device side of batches of small fits of UNEQUAL sizes (agp_fit_create_batch_ragged, the phantom
// fits that agp_predict_batch and agp_fit_update_batch take in lock step, and the batched gradients
// agp_nll_gradient_batch_ragged / agp_loo_nll_gradient_batch_ragged, whose pad items carry the slab and z only).
//
// A fit of n_b points in a batch of padded size n is the ordinary fit of diag(K_b, I): its factor is diag(L_b, I), z and
// the information vector are zero on the trailing phantom rows [n_b, n), the log determinant is that of K_b.  The
// batched factorisation and substitutions work on the padded size and know nothing of it.  What they need is here:
//
//   pad          rows [n_b, n) of the lower triangle of slab b <- e_i^T, z_b <- 0 there, phantom feature rows
//                (behind the Gram launches, which run on views of n_b rows: no Gram value is ever computed for, or the NaN
//                flag raised by, a phantom row, and the target variance is not added to a phantom diagonal)
//   zero rows    the phantom rows of a cross covariance V_b (n x m) before the forward substitution    (agp_predict_batch)
//   zero columns the phantom columns of a transposed cross covariance X_b (m x n_pad)                   (agp_fit_update_batch)
//
// All three are ONE table-driven launch (one grid dimension = problem) with plain vector stores; a problem without phantom
// rows returns at once.  Nothing is reduced here.
#include <cstring>

#include "batch_front.h"

namespace agp {

// blockIdx.y = problem.  The columns of slab b are dealt to the workgroups round-robin.  A real column c < n_b gets zeros in
// the rows n_b .. n; a phantom column gets e_c from the first row of the 128-row block of its diagonal element on (the
// part of that block above the diagonal included, as update_grow_kernel writes it: the tiles the factorisation touches
// hold no stale value).  Rows move as 16-byte pairs: lda is even and the slab 16-byte aligned, so the element (r, c) is
// 16-byte aligned exactly when r is even; an odd first row and an odd last row are single stores.
__global__ __launch_bounds__(64) void ragged_pad_kernel(const RaggedPadItem *__restrict__ items, long long n, long long lda) {
  const RaggedPadItem it = items[blockIdx.y];
  const long long nb = it.nb;
  if (nb >= n) return;
  for (long long c = blockIdx.x; c < n; c += gridDim.x) {
    const bool phantom = c >= nb;
    const long long r0 = phantom ? c / NB * NB : nb;
    double *col = it.A + c * lda;
    const long long re = (r0 + 1) / 2 * 2;  // first even row
    if (threadIdx.x == 0 && re > r0) col[r0] = (phantom && r0 == c) ? 1. : 0.;
    for (long long r = re + 2 * (long long)threadIdx.x; r < n; r += 2 * 64) {
      const double va = (phantom && r == c) ? 1. : 0.;
      if (r + 1 < n) *reinterpret_cast<double2 *>(col + r) = make_double2(va, (phantom && r + 1 == c) ? 1. : 0.);
      else col[r] = va;
    }
  }
  const long long np = n - nb, t0 = (long long)blockIdx.x * 64 + threadIdx.x, step = (long long)gridDim.x * 64;
  for (long long i = t0; i < np; i += step) it.z[nb + i] = 0.;
  const int dim = it.dim;
  for (long long i = t0; i < np * dim; i += step) it.coords[nb * dim + i] = it.coords[i % dim];
  if (it.ids)
    for (long long i = t0; i < np; i += step) it.ids[nb + i] = -2 - i;
  for (int k = 0; k < it.nsc; ++k)
    for (long long i = t0; i < np; i += step) it.scales[(long long)k * n + nb + i] = it.scales[(long long)k * n];
}

void launch_ragged_pad(hipStream_t s, const RaggedPadItem *table_dev, long long count, long long n, long long lda) {
  if (count <= 0 || n <= 0) return;
  hipLaunchKernelGGL(ragged_pad_kernel, dim3((unsigned)(n < 256 ? n : 256), (unsigned)count), dim3(64), 0, s, table_dev, n, lda);
}

void RangeTable::write(void *dst) const {
  std::memcpy(dst, items.data(), item_bytes());
  if (!pairs.empty()) std::memcpy(static_cast<char *>(dst) + item_bytes(), pairs.data(), sizeof(long long) * pairs.size());
}

// blockIdx = (column j, problem): the rows of every range of the problem, a wave across them
__global__ __launch_bounds__(64) void zero_row_ranges_kernel(const RangeItem *__restrict__ items, const long long *__restrict__ pairs,
                                                            double *V, long long stride_V, long long ldv) {
  const RangeItem it = items[blockIdx.y];
  double *col = V + (long long)blockIdx.y * stride_V + (long long)blockIdx.x * ldv;
  for (long long k = 0; k < it.count; ++k) {
    const long long r0 = pairs[2 * (it.first + k)], r1 = pairs[2 * (it.first + k) + 1];
    for (long long r = r0 + threadIdx.x; r < r1; r += 64) col[r] = 0.;
  }
}

void launch_zero_row_ranges(hipStream_t s, const void *table_dev, long long total, long long first, long long count, double *V,
                            long long stride_V, long long ldv, long long m) {
  if (count <= 0 || m <= 0) return;
  const RangeItem *items = static_cast<const RangeItem *>(table_dev);
  const long long *pairs = reinterpret_cast<const long long *>(items + total);
  hipLaunchKernelGGL(zero_row_ranges_kernel, dim3((unsigned)m, (unsigned)count), dim3(64), 0, s, items + first, pairs, V, stride_V, ldv);
}

// blockIdx = (256 rows, column group, problem): the columns of every range of the problem are dealt to the column groups
__global__ __launch_bounds__(256) void zero_column_ranges_kernel(const RangeItem *__restrict__ items, const long long *__restrict__ pairs,
                                                                double *X, long long stride_X, long long ld, long long m) {
  const RangeItem it = items[blockIdx.z];
  double *Xb = X + (long long)blockIdx.z * stride_X;
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  for (long long k = 0; k < it.count; ++k) {
    const long long c0 = pairs[2 * (it.first + k)], c1 = pairs[2 * (it.first + k) + 1];
    for (long long c = c0 + blockIdx.y; c < c1; c += gridDim.y) Xb[r + c * ld] = 0.;
  }
}

void launch_zero_column_ranges(hipStream_t s, const void *table_dev, long long total, long long first, long long count, double *X,
                               long long stride_X, long long ld, long long m) {
  if (count <= 0 || m <= 0) return;
  const RangeItem *items = static_cast<const RangeItem *>(table_dev);
  const long long *pairs = reinterpret_cast<const long long *>(items + total);
  hipLaunchKernelGGL(zero_column_ranges_kernel, dim3((unsigned)((m + 255) / 256), 128u, (unsigned)count), dim3(256), 0, s, items + first,
                     pairs, X, stride_X, ld, m);
}

}  // namespace agp
