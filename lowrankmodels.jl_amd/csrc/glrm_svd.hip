// glrm_svd.hip -- glrm_hip_init_svd: init_svd!(glrm) (src/initialize.jl:35-132) on the resident observation lists.
//
// The reference expands A to an m x d real matrix (categorical columns -> +-1 indicators per level, multi-dimensional ordinal
// columns -> +-1 threshold indicators, :47-80), subtracts the per-column mean of the observed entries (:83-98), leaves unobserved
// entries at 0, scales by m*n/|Omega| (:113) and takes the top-k singular triplets with Arpack (:121):  X = sqrt(S) U',
// Y = sqrt(S) V' diag(std) (:129-130).  Here the standardized matrix B is never materialised: both products of a randomized
// subspace iteration, U <- B V (row view) and V <- B' U (column view), expand the observations on the fly.  The iteration itself
// (subspace_iterate: the tall-skinny blocks orthonormalized through their l x l Gram matrix, eigen-decomposition on the host,
// l = k + oversampling <= 128, the Ritz values of B'U as singular values) and the body of the column product live in
// glrm_subspace.hpp, shared with glrm_nmf.hip; this unit has the expansion (areal, SvdArgs), the column statistics, the row
// product and the factors.  Everything is fp64 and every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "glrm_engine.hpp"
#include "glrm_subspace.hpp"

namespace {

// entry (a, j) of the real-valued expansion of one observed value (src/initialize.jl:52-77)
__device__ __forceinline__ double areal(int kind, int d, double a, int j) {
  if (d <= 1) return a;
  if (kind == GLRM_LOSS_MULTINOMIAL || kind == GLRM_LOSS_OVA) return a == (double)(j + 1) ? 1.0 : -1.0; // CategoricalDomain
  const int nlev = kind == GLRM_LOSS_ORDISTIC ? d : d + 1;                                                // OrdinalDomain: 1..max
  return j < nlev - 1 ? (a > (double)(j + 1) ? 1.0 : -1.0) : 0.0;
}

// the functor of the column product (glrm_subspace.hpp): d expanded vectors per column, centred entries, the finished sum times cscale
struct SvdArgs : ProductArgs {
  const glrm_loss* losses;
  int loss_single;
  const int64_t* ystart;
  const double* means;  // [d]
  double cscale;        // m*n/|Omega_rows|
  struct Col { int kind, d; int64_t ys; };
  __device__ Col col(int64_t f) const {
    const glrm_loss lo = losses[loss_single ? 0 : f];
    return {lo.kind, lo.dim > 1 ? lo.dim : 1, ystart[f]};
  }
  __device__ double value(const Col& c, int j, int64_t t) const { return areal(c.kind, c.d, vals[t], j) - means[c.ys + j]; }
  __device__ double finish(const Col&, int64_t, int, double s) const { return cscale * s; }
};

// per expanded column: mean and corrected standard deviation of the observed entries (:83-95); one workgroup per column
__global__ void __launch_bounds__(256) svd_stats_kernel(const int64_t* colptr, const double* colvals, const glrm_loss* losses, int loss_single,
                                                        const int64_t* ystart, int64_t nl, double tol, double* means, double* stds) {
  const int64_t f = blockIdx.x;
  const glrm_loss lo = losses[loss_single ? 0 : f];
  const int d = lo.dim > 1 ? lo.dim : 1;
  const int64_t b = colptr[f], e = colptr[f + 1], ys = ystart[f];
  __shared__ double sh[256];
  for (int j = 0; j < d; ++j) {
    double s = 0.0;
    for (int64_t t = b + threadIdx.x; t < e; t += 256) s += areal(lo.kind, d, colvals[t], j);
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
    double mean = sh[0] / (double)(e - b); // 0/0 = NaN for an empty column
    __syncthreads();
    double q = 0.0;
    for (int64_t t = b + threadIdx.x; t < e; t += 256) { const double x = areal(lo.kind, d, colvals[t], j) - mean; q = fma(x, x, q); }
    sh[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) {
      double sd = sqrt(sh[0] / (double)(e - b - 1));
      if (mean != mean) mean = 1.0;             // isnan(means[j]) -> 1 (:88-90)
      if (sd < tol || sd != sd) sd = 1.0;       // :92-94
      means[ys + j] = mean;
      stds[ys + j] = sd;
    }
    __syncthreads();
  }
}

// U[e, :] = cscale * sum_{(f,a) in Omega_e} sum_j (areal(a,j) - mean_j) V[ys_f + j, :]      one wave per row
__global__ void __launch_bounds__(256) svd_rows_kernel(const SvdArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= a.nseg) return;
  const int l = a.l;
  double acc0 = 0.0, acc1 = 0.0;
  for (int64_t t = a.ptr[e]; t < a.ptr[e + 1]; ++t) {
    const int32_t f = a.idx[t];
    const double av = a.vals[t];
    const glrm_loss lo = a.losses[a.loss_single ? 0 : f];
    const int d = lo.dim > 1 ? lo.dim : 1;
    const int64_t ys = a.ystart[f];
    for (int j = 0; j < d; ++j) {
      const double v = areal(lo.kind, d, av, j) - a.means[ys + j];
      const double* vr = a.in + (ys + j) * l;
      if (lane < l) acc0 = fma(v, vr[lane], acc0);
      if (lane + 64 < l) acc1 = fma(v, vr[lane + 64], acc1);
    }
  }
  if (lane < l) a.out[e * l + lane] = a.cscale * acc0;
  if (lane + 64 < l) a.out[e * l + lane + 64] = a.cscale * acc1;
}

// V[ys_f + j, :] = cscale * sum_{(e,a) in Omega^f} (areal(a,j) - mean_j) U[e, :]: the shared column product under this unit's names
__global__ void __launch_bounds__(256) svd_cols_kernel(const SvdArgs a) { cols_product_kernel(a); }
__global__ void svd_cols_reduce_kernel(const SvdArgs a) { cols_reduce_kernel(a); }

// X[c, e] = sqrt(s_c) U[e, c];  Y[c, j] = sqrt(s_c) V[j, c] std_j   (k x count, column-major like glrm.X / glrm.Y)
__global__ void factors_kernel(const double* Z, int64_t count, int l, int k, const double* sqrt_s, const double* stds, double* F) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count * k; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / k;
    const int c = (int)(i - r * k);
    F[i] = sqrt_s[c] * Z[r * l + c] * (stds ? stds[r] : 1.0);
  }
}

} // namespace

extern "C" int glrm_hip_init_svd(glrm_handle* h, double* X, double* Y, int32_t max_iter, double tol, uint64_t seed, double* singular_values,
                                 int32_t* iters_done) {
  if (!h || !X || !Y) return fail(GLRM_ERR_INVALID, "NULL argument");
  GLRM_REFUSE_F32(h, "glrm_hip_init_svd");
  if (!glrm_single_shard(h)) return fail(GLRM_ERR_INVALID, "glrm_hip_init_svd needs a single-shard handle");
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_svd works on the observation lists (create the handle without dense_A)");
  GLRM_NEED_FINALIZED(h);
  const int k = h->k;
  const int64_t m = h->m, d = h->d;
  if (k > m || k > d) return fail(GLRM_ERR_INVALID, "k = %d exceeds min(m, d): no k singular triplets", k);
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  const int l = block_width(k, m, d);
  if (l < k) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_svd supports k <= %d", LMAX);
  hipStream_t st = h->stream;
  Work w;
  DevArena scratch;
  double *means = nullptr, *stds = nullptr, *sq = nullptr, *dX = nullptr, *dY = nullptr;
  int rc;
  if ((rc = alloc_work(w, scratch, st, l, m, d, (size_t)l * l)) || (rc = scratch.alloc(&means, (size_t)d)) || (rc = scratch.alloc(&stds, (size_t)d)) ||
      (rc = scratch.alloc(&sq, (size_t)l)))
    return rc;
  // column statistics
  hipLaunchKernelGGL(svd_stats_kernel, dim3((unsigned)h->n), dim3(256), 0, st, h->side[GLRM_COLS].ptr, h->side[GLRM_COLS].vals, h->losses, h->n_losses == 1 ? 1 : 0,
                     h->ystart, h->n, 1e-10, means, stds);
  HIPCK(hipGetLastError());
  SvdArgs ra{}, ca{};
  ra.nseg = m; ra.ptr = h->side[GLRM_ROWS].ptr; ra.idx = h->side[GLRM_ROWS].idx; ra.vals = h->side[GLRM_ROWS].vals;
  ra.losses = h->losses; ra.loss_single = h->n_losses == 1 ? 1 : 0; ra.ystart = h->ystart; ra.means = means;
  ra.cscale = h->side[GLRM_ROWS].nnz > 0 ? (double)m * (double)h->n / (double)h->side[GLRM_ROWS].nnz : 0.0; // Astd *= m*n/sum(map(length, observed_features)) (:113)
  ra.in = w.V; ra.out = w.U; ra.l = l; ra.nsplit = 1; ra.dmax = h->dmax;
  ca = ra;
  ca.nseg = h->n; ca.ptr = h->side[GLRM_COLS].ptr; ca.idx = h->side[GLRM_COLS].idx; ca.vals = h->side[GLRM_COLS].vals; ca.in = w.U; ca.out = w.V;
  if ((rc = chunk_product(h, scratch, ca))) return rc;
  auto BV = [&]() { // U = B V
    hipLaunchKernelGGL(svd_rows_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, ra);
  };
  auto BtU = [&]() { // V = B' U
    hipLaunchKernelGGL(svd_cols_kernel, dim3((unsigned)h->n, (unsigned)ca.nsplit), dim3(256), 0, st, ca);
    if (ca.nsplit > 1) hipLaunchKernelGGL(svd_cols_reduce_kernel, dim3((unsigned)h->n), dim3(256), 0, st, ca);
  };
  std::vector<double> ritz;
  int it = 0;
  if ((rc = subspace_iterate(w, m, d, k, max_iter, tol, seed, BV, BtU, ritz, it))) return rc;
  std::vector<double> sqh((size_t)l);
  for (int c = 0; c < l; ++c) sqh[c] = std::sqrt(std::sqrt(std::max(ritz[c], 0.0))); // sqrt of the singular value
  HIPCK(hipMemcpyAsync(sq, sqh.data(), (size_t)l * 8, hipMemcpyHostToDevice, st));
  if ((rc = scratch.alloc(&dX, (size_t)m * k)) || (rc = scratch.alloc(&dY, (size_t)d * k))) return rc;
  hipLaunchKernelGGL(factors_kernel, dim3(1024), dim3(256), 0, st, w.U, m, l, k, sq, (const double*)nullptr, dX);
  hipLaunchKernelGGL(factors_kernel, dim3(1024), dim3(256), 0, st, w.V, d, l, k, sq, stds, dY);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(X, dX, (size_t)m * k * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(Y, dY, (size_t)d * k * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  if (singular_values) for (int c = 0; c < k; ++c) singular_values[c] = std::sqrt(std::max(ritz[c], 0.0));
  if (iters_done) *iters_done = it;
  return GLRM_OK;
}
