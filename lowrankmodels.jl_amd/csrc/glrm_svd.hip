// glrm_svd.hip -- glrm_hip_init_svd: init_svd!(glrm) (src/initialize.jl:35-132) on the resident observation lists.
//
// The reference expands A to an m x d real matrix (categorical columns -> +-1 indicators per level, multi-dimensional ordinal
// columns -> +-1 threshold indicators, :47-80), subtracts the per-column mean of the observed entries (:83-98), leaves unobserved
// entries at 0, scales by m*n/|Omega| (:113) and takes the top-k singular triplets with Arpack (:121):  X = sqrt(S) U',
// Y = sqrt(S) V' diag(std) (:129-130).  Here the standardized matrix B is never materialised: both products of a randomized
// subspace iteration, U <- B V (row view) and V <- B' U (column view), expand the observations on the fly; the tall-skinny
// blocks are orthonormalized through their l x l Gram matrix (eigen-decomposition on the host, l = k + oversampling <= 128),
// and the Ritz values of B'U give the singular values.  Everything is fp64 and every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "glrm_engine.hpp"
#include "glrm_subspace.hpp"

namespace {

struct SvdArgs {
  int64_t nseg;
  const int64_t* ptr;
  const int32_t* idx;
  const double* vals;
  const glrm_loss* losses;
  int loss_single;
  const int64_t* ystart;
  const double* means;  // [d]
  double cscale;        // m*n/|Omega_rows|
  const double* in;     // rows: V [d][l];  cols: U [m][l]
  double* out;          // rows: U [m][l];  cols: V [d][l] (or partials)
  int l;
  int nsplit;
  int64_t chunk;
  double* partial;      // cols with nsplit > 1: [nseg][nsplit][dmax][l]
  int dmax;
};

// entry (a, j) of the real-valued expansion of one observed value (src/initialize.jl:52-77)
__device__ __forceinline__ double areal(int kind, int d, double a, int j) {
  if (d <= 1) return a;
  if (kind == GLRM_LOSS_MULTINOMIAL || kind == GLRM_LOSS_OVA) return a == (double)(j + 1) ? 1.0 : -1.0; // CategoricalDomain
  const int nlev = kind == GLRM_LOSS_ORDISTIC ? d : d + 1;                                                // OrdinalDomain: 1..max
  return j < nlev - 1 ? (a > (double)(j + 1) ? 1.0 : -1.0) : 0.0;
}

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

// V[ys_f + j, :] = cscale * sum_{(e,a) in Omega^f} (areal(a,j) - mean_j) U[e, :]     workgroup (4 waves) per (column, chunk)
__global__ void __launch_bounds__(256) svd_cols_kernel(const SvdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t f = blockIdx.x;
  const int y = blockIdx.y;
  const int l = a.l;
  const glrm_loss lo = a.losses[a.loss_single ? 0 : f];
  const int d = lo.dim > 1 ? lo.dim : 1;
  const int64_t ys = a.ystart[f];
  int64_t b = a.ptr[f] + (int64_t)y * a.chunk, e = b + a.chunk;
  const int64_t e0 = a.ptr[f + 1];
  b = b < e0 ? b : e0;
  e = e < e0 ? e : e0;
  __shared__ double sh[4][LMAX];
  for (int j = 0; j < d; ++j) {
    const double mean = a.means[ys + j];
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t t = b + wave; t < e; t += 4) {
      const double v = areal(lo.kind, d, a.vals[t], j) - mean;
      const double* ur = a.in + (int64_t)a.idx[t] * l;
      if (lane < l) acc0 = fma(v, ur[lane], acc0);
      if (lane + 64 < l) acc1 = fma(v, ur[lane + 64], acc1);
    }
    if (lane < l) sh[wave][lane] = acc0;
    if (lane + 64 < l) sh[wave][lane + 64] = acc1;
    __syncthreads();
    for (int c = threadIdx.x; c < l; c += 256) {
      const double s = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
      if (a.nsplit > 1) a.partial[(((size_t)f * a.nsplit + y) * a.dmax + j) * l + c] = s;
      else a.out[(ys + j) * l + c] = a.cscale * s;
    }
    __syncthreads();
  }
}

__global__ void svd_cols_reduce_kernel(const SvdArgs a) { // chunk partials in chunk order
  const int64_t f = blockIdx.x;
  const int l = a.l;
  const glrm_loss lo = a.losses[a.loss_single ? 0 : f];
  const int d = lo.dim > 1 ? lo.dim : 1;
  const int64_t ys = a.ystart[f];
  for (int i = threadIdx.x; i < d * l; i += blockDim.x) {
    const int j = i / l, c = i - j * l;
    double s = 0.0;
    for (int y = 0; y < a.nsplit; ++y) s += a.partial[(((size_t)f * a.nsplit + y) * a.dmax + j) * l + c];
    a.out[(ys + j) * l + c] = a.cscale * s;
  }
}

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
  if (max_iter <= 0) max_iter = 60;
  if (!(tol > 0)) tol = 1e-12;
  int l = k + 8;
  if (l > LMAX) l = LMAX;
  if (l > m) l = (int)m;
  if (l > d) l = (int)d;
  if (l < k) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_svd supports k <= %d", LMAX);
  Work w;
  w.h = h; w.st = h->stream; w.l = l;
  hipStream_t st = w.st;
  DevArena scratch;
  int rc;
  if ((rc = scratch.alloc(&w.V, (size_t)d * l)) || (rc = scratch.alloc(&w.U, (size_t)m * l)) || (rc = scratch.alloc(&w.means, (size_t)d)) ||
      (rc = scratch.alloc(&w.stds, (size_t)d)) || (rc = scratch.alloc(&w.gpart, (size_t)w.nblk_max * l * l)) || (rc = scratch.alloc(&w.G, (size_t)l * l)) ||
      (rc = scratch.alloc(&w.M, (size_t)l * l)) || (rc = scratch.alloc(&w.sq, (size_t)l)))
    return rc;
  // column statistics
  hipLaunchKernelGGL(svd_stats_kernel, dim3((unsigned)h->n), dim3(256), 0, st, h->side[GLRM_COLS].ptr, h->side[GLRM_COLS].vals, h->losses, h->n_losses == 1 ? 1 : 0,
                     h->ystart, h->n, 1e-10, w.means, w.stds);
  HIPCK(hipGetLastError());
  SvdArgs ra{}, ca{};
  ra.nseg = m; ra.ptr = h->side[GLRM_ROWS].ptr; ra.idx = h->side[GLRM_ROWS].idx; ra.vals = h->side[GLRM_ROWS].vals;
  ra.losses = h->losses; ra.loss_single = h->n_losses == 1 ? 1 : 0; ra.ystart = h->ystart; ra.means = w.means;
  ra.cscale = h->side[GLRM_ROWS].nnz > 0 ? (double)m * (double)h->n / (double)h->side[GLRM_ROWS].nnz : 0.0; // Astd *= m*n/sum(map(length, observed_features)) (:113)
  ra.in = w.V; ra.out = w.U; ra.l = l; ra.nsplit = 1; ra.dmax = h->dmax;
  ca = ra;
  ca.nseg = h->n; ca.ptr = h->side[GLRM_COLS].ptr; ca.idx = h->side[GLRM_COLS].idx; ca.vals = h->side[GLRM_COLS].vals; ca.in = w.U; ca.out = w.V;
  { // long columns: several workgroups per column, partials added in chunk order
    std::vector<int64_t> cp((size_t)h->n + 1);
    HIPCK(hipMemcpyAsync(cp.data(), h->side[GLRM_COLS].ptr, ((size_t)h->n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    int64_t longest = 0;
    for (int64_t f = 0; f < h->n; ++f) longest = std::max(longest, cp[f + 1] - cp[f]);
    ca.chunk = 16384;
    while ((longest + ca.chunk - 1) / ca.chunk > 65535) ca.chunk *= 2; // gridDim.y
    ca.nsplit = (int)std::max<int64_t>(1, (longest + ca.chunk - 1) / ca.chunk);
    if (ca.nsplit > 1) {
      if ((rc = scratch.alloc(&w.cpart, (size_t)h->n * ca.nsplit * h->dmax * l))) return rc;
      ca.partial = w.cpart;
    } else ca.chunk = longest > 0 ? longest : 1;
  }
  auto BV = [&]() { // U = B V
    hipLaunchKernelGGL(svd_rows_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, ra);
  };
  auto BtU = [&]() { // V = B' U
    hipLaunchKernelGGL(svd_cols_kernel, dim3((unsigned)h->n, (unsigned)ca.nsplit), dim3(256), 0, st, ca);
    if (ca.nsplit > 1) hipLaunchKernelGGL(svd_cols_reduce_kernel, dim3((unsigned)h->n), dim3(256), 0, st, ca);
  };
  hipLaunchKernelGGL(randn_kernel, dim3(1024), dim3(256), 0, st, w.V, d * l, seed);
  if ((rc = orthonormalize(w, w.V, d))) return rc;
  std::vector<double> ritz, prev, E;
  int it = 0;
  for (it = 1; it <= max_iter; ++it) {
    BV();
    if ((rc = orthonormalize(w, w.U, m))) return rc;
    BtU();
    HIPCK(hipGetLastError());
    if ((rc = orthonormalize(w, w.V, d, &ritz, &E))) return rc; // eigenvalues of (B'U)'(B'U) = squared singular values
    bool done = !prev.empty();
    for (int c = 0; c < k && done; ++c) {
      const double s = std::sqrt(std::max(ritz[c], 0.0)), sp = std::sqrt(std::max(prev[c], 0.0)), s0 = std::sqrt(std::max(ritz[0], 0.0));
      if (std::fabs(s - sp) > tol * (s0 > 0 ? s0 : 1.0)) done = false;
    }
    prev = ritz;
    if (done) break;
  }
  if (it > max_iter) it = max_iter;
  // After the last pass: V = orth(B'U) = right singular vectors (columns by descending value); left ones = U E.
  if ((rc = rightmul(w, w.U, m, E))) return rc;
  std::vector<double> sq((size_t)l);
  for (int c = 0; c < l; ++c) sq[c] = std::sqrt(std::sqrt(std::max(ritz[c], 0.0))); // sqrt of the singular value
  HIPCK(hipMemcpyAsync(w.sq, sq.data(), (size_t)l * 8, hipMemcpyHostToDevice, st));
  if ((rc = scratch.alloc(&w.dX, (size_t)m * k)) || (rc = scratch.alloc(&w.dY, (size_t)d * k))) return rc;
  hipLaunchKernelGGL(factors_kernel, dim3(1024), dim3(256), 0, st, w.U, m, l, k, w.sq, (const double*)nullptr, w.dX);
  hipLaunchKernelGGL(factors_kernel, dim3(1024), dim3(256), 0, st, w.V, d, l, k, w.sq, w.stds, w.dY);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(X, w.dX, (size_t)m * k * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(Y, w.dY, (size_t)d * k * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  if (singular_values) for (int c = 0; c < k; ++c) singular_values[c] = std::sqrt(std::max(ritz[c], 0.0));
  if (iters_done) *iters_done = it;
  return GLRM_OK;
}
