// glrm_nmf.hip -- glrm_hip_init_nndsvd: init_nndsvd!(glrm) (src/initialize_nmf.jl) on the resident observation lists.
//
// The reference fills a dense m x n matrix with the observed entries, hands it to NMF.jl's nndsvd and, with max_iters > 0, rewrites
// every missing entry with <x_i, y_j> and decomposes the dense matrix again.  Here nothing m x n exists.  The matrix of a round is
//     B_t = P_Omega(s A - X'Y) + X'Y                 (round 0: B_0 = P_Omega(s A))
// a sparse matrix on the resident lists plus a rank-k term, and the subspace iteration (subspace_iterate in glrm_subspace.hpp, the one
// glrm_svd.hip runs, once per round here) needs only
//     U <- B_t V  = R V  + X'(Y V)                    row view:    nmf_rows_kernel, T = Y V by nmf_tsmm_kernel
//     V <- B_t' U = R' U + Y'(X U)                    column view: nmf_cols_kernel (the shared column product of glrm_subspace.hpp over
//                                                                  NmfArgs), T = X U by nmf_tsmm_kernel
// with R the residuals r = s_f a - <x_e, y_f>, written once per round and view by nmf_residual_kernel (the hot kernel: one k-vector
// gathered per observation, like a gradient pass).  The split (positive / negative squared norms of every singular vector in a fixed
// tree, the mean of B_t for variant `a`, one kernel that writes X and Y) follows include/glrm_hip_nmf.h.  Everything is fp64, no
// floating-point atomics, every reduction has a fixed order.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/glrm_hip_nmf.h"
#include "glrm_engine.hpp"
#include "glrm_subspace.hpp"

namespace {

constexpr int NMF_RG = 8;      // lanes that share one observation's dot product (8 x 16 B = one 128-byte line per load)
constexpr int NMF_RB = 4;      // observations of a lane group whose gathers are in flight together
constexpr int NMF_WAVE_OBS = (64 / NMF_RG) * NMF_RB; // observations a wave covers per trip
constexpr int NMF_PB = 4;      // entries of a row whose gathers are in flight together in the sparse product
constexpr int NMF_TROWS = 16;  // rows per LDS tile of nmf_tsmm_kernel (two tiles of NMF_TROWS x (LMAX + 1) doubles)

struct ResidArgs {
  int64_t nseg;
  const int64_t* ptr;
  const int32_t* idx;
  const double* vals;
  const glrm_loss* losses;
  int loss_single, use_scale;
  int cols;            // 1: a segment is a column (the scale is the segment's, a workgroup per (column, chunk)); 0: a wave per row
  int64_t chunk;
  const double* Fseg;  // k x nseg, the factor of the segments' side
  const double* Fopp;  // k x (opposing count)
  int k;
  double* resid;       // [nnz] in the view's own order
};

// r_t = s_f a_t - <x_e, y_f>.  NMF_RG lanes share an observation: lane p owns the components 2p, 2p+1, 2p+16, 2p+17, ... (VEC2, k even:
// 16-byte loads) or p, p+8, ... (k odd), adds its products in ascending order and the lanes meet in an xor butterfly -- the order is a
// function of k only, and the same for both views (a product commutes exactly).  NMF_RB observations per group are in flight together.
template <bool VEC2>
__global__ void __launch_bounds__(256) nmf_residual_kernel(const ResidArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / NMF_RG, p = lane % NMF_RG;
  const int k = a.k;
  int64_t seg, b, e, first, stride;
  if (a.cols) {
    seg = blockIdx.x;
    const int64_t e0 = a.ptr[seg + 1];
    b = a.ptr[seg] + (int64_t)blockIdx.y * a.chunk;
    e = b + a.chunk;
    b = b < e0 ? b : e0;
    e = e < e0 ? e : e0;
    first = b + (int64_t)wave * NMF_WAVE_OBS;
    stride = 4 * NMF_WAVE_OBS;
  } else {
    seg = (int64_t)blockIdx.x * 4 + wave;
    if (seg >= a.nseg) return; // the whole wave
    b = a.ptr[seg];
    e = a.ptr[seg + 1];
    first = b;
    stride = NMF_WAVE_OBS;
  }
  const double* xs_ptr = a.Fseg + seg * k;
  double xs[LMAX / NMF_RG];
#pragma unroll
  for (int i = 0; i < LMAX / NMF_RG / 2; ++i) {
    if constexpr (VEC2) {
      const int c = 2 * p + 2 * NMF_RG * i;
      double2 v = make_double2(0.0, 0.0);
      if (c < k) v = *reinterpret_cast<const double2*>(xs_ptr + c);
      xs[2 * i] = v.x;
      xs[2 * i + 1] = v.y;
    } else {
      const int c0 = p + NMF_RG * (2 * i), c1 = p + NMF_RG * (2 * i + 1);
      xs[2 * i] = c0 < k ? xs_ptr[c0] : 0.0;
      xs[2 * i + 1] = c1 < k ? xs_ptr[c1] : 0.0;
    }
  }
  const double seg_scale = a.cols && a.use_scale ? a.losses[a.loss_single ? 0 : seg].scale : 1.0;
  for (int64_t t0 = first; t0 < e; t0 += stride) { // wave-uniform trips: every lane runs the butterfly
    int32_t f[NMF_RB];
    double av[NMF_RB], s[NMF_RB];
#pragma unroll
    for (int q = 0; q < NMF_RB; ++q) {
      const int64_t tt = t0 + g + (int64_t)q * (64 / NMF_RG);
      f[q] = tt < e ? a.idx[tt] : 0;
      av[q] = tt < e ? a.vals[tt] : 0.0;
      s[q] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < LMAX / NMF_RG / 2; ++i) {
      if constexpr (VEC2) {
        const int c = 2 * p + 2 * NMF_RG * i;
        if (c < k) {
          double2 y[NMF_RB];
#pragma unroll
          for (int q = 0; q < NMF_RB; ++q) y[q] = *reinterpret_cast<const double2*>(a.Fopp + (int64_t)f[q] * k + c);
#pragma unroll
          for (int q = 0; q < NMF_RB; ++q) {
            s[q] = fma(xs[2 * i], y[q].x, s[q]);
            s[q] = fma(xs[2 * i + 1], y[q].y, s[q]);
          }
        }
      } else {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const int c = p + NMF_RG * (2 * i + hh);
          if (c < k) {
            double y[NMF_RB];
#pragma unroll
            for (int q = 0; q < NMF_RB; ++q) y[q] = a.Fopp[(int64_t)f[q] * k + c];
#pragma unroll
            for (int q = 0; q < NMF_RB; ++q) s[q] = fma(xs[2 * i + hh], y[q], s[q]);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NMF_RB; ++q) {
#pragma unroll
      for (int d = 1; d < NMF_RG; d <<= 1) s[q] += __shfl_xor(s[q], d, 64);
      const int64_t tt = t0 + g + (int64_t)q * (64 / NMF_RG);
      if (p == 0 && tt < e) {
        const double sc = a.cols ? seg_scale : (a.use_scale ? a.losses[a.loss_single ? 0 : f[q]].scale : 1.0);
        a.resid[tt] = sc * av[q] - s[q];
      }
    }
  }
}

struct NmfArgs;
__device__ __forceinline__ double nmf_lowrank(const NmfArgs& a, int64_t seg, int c, double s);

// the functor of the column product (glrm_subspace.hpp): one vector per column, the residual or s_f a, the finished sum plus the rank-k term
struct NmfArgs : ProductArgs {
  const double* resid;  // nullptr in round 0: the value is s_f a
  const glrm_loss* losses;
  int loss_single, use_scale;
  const double* F;      // the rank-k term, nullptr in round 0: out[seg, :] += F[:, seg]' T  (F k x nseg, T k x l row-major)
  const double* T;
  int k;
  struct Col { static constexpr int d = 1; int64_t ys; double sc; };
  __device__ Col col(int64_t f) const { return {f, !resid && use_scale ? losses[loss_single ? 0 : f].scale : 1.0}; }
  __device__ double value(const Col& c, int, int64_t t) const { return resid ? resid[t] : c.sc * vals[t]; }
  __device__ double finish(const Col&, int64_t f, int c, double s) const { return T ? nmf_lowrank(*this, f, c, s) : s; }
};

// entry c of x_seg' T, the components in ascending order, continued from s
__device__ __forceinline__ double nmf_lowrank(const NmfArgs& a, int64_t seg, int c, double s) {
  const double* x = a.F + seg * a.k;
  for (int j = 0; j < a.k; ++j) s = fma(x[j], a.T[j * a.l + c], s);
  return s;
}

// U[e, :] = sum_{(f, v) in Omega_e} v V[f, :]  (+ x_e' T), one wave per row; the gathers of NMF_PB entries are in flight together and
// the additions keep the list's order
__global__ void __launch_bounds__(256) nmf_rows_kernel(const NmfArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= a.nseg) return;
  const int l = a.l;
  const bool lo = lane < l, hi = lane + 64 < l;
  double acc0 = 0.0, acc1 = 0.0;
  const int64_t te = a.ptr[e + 1];
  for (int64_t t = a.ptr[e]; t < te; t += NMF_PB) {
    int32_t f[NMF_PB];
    double v[NMF_PB], g0[NMF_PB], g1[NMF_PB];
#pragma unroll
    for (int q = 0; q < NMF_PB; ++q) {
      const int64_t tt = t + q;
      f[q] = tt < te ? a.idx[tt] : 0;
      v[q] = tt < te ? (a.resid ? a.resid[tt] : a.vals[tt]) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < NMF_PB; ++q) {
      const double* vr = a.in + (int64_t)f[q] * l;
      g0[q] = lo ? vr[lane] : 0.0;
      g1[q] = hi ? vr[lane + 64] : 0.0;
      if (!a.resid && a.use_scale) v[q] = a.losses[a.loss_single ? 0 : f[q]].scale * v[q];
    }
#pragma unroll
    for (int q = 0; q < NMF_PB; ++q) {
      if (t + q < te) {
        acc0 = fma(v[q], g0[q], acc0);
        acc1 = fma(v[q], g1[q], acc1);
      }
    }
  }
  if (a.T) {
    if (lo) acc0 = nmf_lowrank(a, e, lane, acc0);
    if (hi) acc1 = nmf_lowrank(a, e, lane + 64, acc1);
  }
  if (lo) a.out[e * l + lane] = acc0;
  if (hi) a.out[e * l + lane + 64] = acc1;
}

// V[f, :] = sum_{(e, v) in Omega^f} v U[e, :]  (+ y_f' T): the shared column product under this unit's names
__global__ void __launch_bounds__(256) nmf_cols_kernel(const NmfArgs a) { cols_product_kernel(a); }
__global__ void nmf_cols_reduce_kernel(const NmfArgs a) { cols_reduce_kernel(a); }

// partial products F Z of row blocks (F k x nrows column-major, Z nrows x l row-major): thread t owns the entries t, t + 256, ... of the
// k x l result, as gram_kernel does of its l x l one; the blocks are added in block order by gram_reduce_kernel
__global__ void __launch_bounds__(256) nmf_tsmm_kernel(const double* F, const double* Z, int64_t nrows, int k, int l, int64_t rows_per_block,
                                                       double* part) {
  __shared__ double tf[NMF_TROWS][LMAX + 1], tz[NMF_TROWS][LMAX + 1];
  const int kl = k * l;
  double acc[LMAX * LMAX / 256];
#pragma unroll
  for (int i = 0; i < LMAX * LMAX / 256; ++i) acc[i] = 0.0;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < nrows ? r0 + rows_per_block : nrows;
  for (int64_t r = r0; r < r1; r += NMF_TROWS) {
    __syncthreads();
    for (int i = threadIdx.x; i < NMF_TROWS * k; i += 256) {
      const int rr = i / k, c = i - rr * k;
      tf[rr][c] = r + rr < r1 ? F[(r + rr) * k + c] : 0.0;
    }
    for (int i = threadIdx.x; i < NMF_TROWS * l; i += 256) {
      const int rr = i / l, c = i - rr * l;
      tz[rr][c] = r + rr < r1 ? Z[(r + rr) * l + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LMAX * LMAX / 256; ++i) {
      const int ent = i * 256 + threadIdx.x;
      if (ent < kl) {
        const int p = ent / l, q = ent - p * l;
        double s = acc[i];
        for (int rr = 0; rr < NMF_TROWS; ++rr) s = fma(tf[rr][p], tz[rr][q], s);
        acc[i] = s;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < LMAX * LMAX / 256; ++i) {
    const int ent = i * 256 + threadIdx.x;
    if (ent < kl) part[(size_t)blockIdx.x * kl + ent] = acc[i];
  }
}

// per row block and column c < ncol of a matrix with leading dimension ld:
//   NORMS: part[blk][c] = sum of z^2 over z > 0, part[blk][ncol + c] = the same over z < 0 (the singular vectors in U / V)
//   else:  part[blk][c] = sum of z (X 1 and Y 1 of the mean)
// Thread (c, half) takes the block's rows of its parity in ascending order; the halves are added even first.
template <bool NORMS>
__global__ void __launch_bounds__(256) nmf_colstat_kernel(const double* Z, int64_t nrows, int ld, int ncol, int64_t rows_per_block, double* part) {
  __shared__ double sh[2][LMAX];
  const int c = threadIdx.x & (LMAX - 1), half = threadIdx.x >> 7;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < nrows ? r0 + rows_per_block : nrows;
  double sp = 0.0, sn = 0.0;
  if (c < ncol)
    for (int64_t r = r0 + half; r < r1; r += 2) {
      const double z = Z[r * ld + c];
      if constexpr (NORMS) {
        if (z > 0) sp = fma(z, z, sp);
        if (z < 0) sn = fma(z, z, sn);
      } else sp += z;
    }
  const int width = NORMS ? 2 * ncol : ncol;
  if (half == 1) { sh[0][c] = sp; sh[1][c] = sn; }
  __syncthreads();
  if (half == 0 && c < ncol) {
    part[(size_t)blockIdx.x * width + c] = sp + sh[0][c];
    if constexpr (NORMS) part[(size_t)blockIdx.x * width + ncol + c] = sn + sh[1][c];
  }
}

// sum over Omega of the row view's values (the residuals, or s_f a in round 0): thread g adds the entries g, g + T, ... in ascending
// order (T = all threads of the grid), butterfly, the 4 waves in order; the blocks are added in block order by gram_reduce_kernel
__global__ void __launch_bounds__(256) nmf_obs_sum_kernel(const NmfArgs a, int64_t nnz, double* part) {
  __shared__ double sh[4];
  const int64_t total = (int64_t)gridDim.x * 256;
  double s = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nnz; t += total)
    s += a.resid ? a.resid[t] : (a.use_scale ? a.losses[a.loss_single ? 0 : a.idx[t]].scale : 1.0) * a.vals[t];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// per component c: sign (+1: the positive parts were chosen), c = sqrt(sigma m+-), the norm of the chosen part of u and of v
struct SplitCoef { double sign, c, xnorm, ynorm; };

// X[c, e] = W[e, c], Y[c, j] = H[c, j]: the chosen part of the singular vector times c / norm, v0 everywhere else
__global__ void nmf_split_kernel(const double* U, int64_t m, const double* V, int64_t n, int l, int k, const SplitCoef* coef, double v0, int zeroh,
                                 double* X, double* Y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (m + n) * k; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / k;
    const int c = (int)(i - r * k);
    const SplitCoef sc = coef[c];
    if (r < m) {
      const double z = sc.sign * U[r * l + c];
      X[i] = z > 0 ? z * sc.c / sc.xnorm : v0;
    } else {
      const double z = sc.sign * V[(r - m) * l + c];
      Y[i - m * k] = zeroh ? 0.0 : (z > 0 ? z * sc.c / sc.ynorm : v0);
    }
  }
}

// T = F Z  (k x l, row-major)
void tsmm(Work& w, const double* F, const double* Z, int64_t nrows, int k, double* T) {
  int nblk;
  int64_t rpb;
  row_blocks(nrows, NMF_TROWS, nblk, rpb);
  hipLaunchKernelGGL(nmf_tsmm_kernel, dim3(nblk), dim3(256), 0, w.st, F, Z, nrows, k, w.l, rpb, w.gpart);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(16), dim3(256), 0, w.st, (const double*)w.gpart, nblk, k * w.l, T);
}

// host copy of the per-column statistics of a matrix: NORMS -> out[0 .. ncol) positive, out[ncol .. 2 ncol) negative squared norms
template <bool NORMS>
int colstat(Work& w, const double* Z, int64_t nrows, int ld, int ncol, double* dtmp, std::vector<double>& out) {
  int nblk;
  int64_t rpb;
  row_blocks(nrows, 2, nblk, rpb);
  const int width = NORMS ? 2 * ncol : ncol;
  hipLaunchKernelGGL(nmf_colstat_kernel<NORMS>, dim3(nblk), dim3(256), 0, w.st, Z, nrows, ld, ncol, rpb, w.gpart);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(16), dim3(256), 0, w.st, (const double*)w.gpart, nblk, width, dtmp);
  HIPCK(hipGetLastError());
  out.resize((size_t)width);
  HIPCK(hipMemcpyAsync(out.data(), dtmp, (size_t)width * 8, hipMemcpyDeviceToHost, w.st));
  HIPCK(hipStreamSynchronize(w.st));
  return GLRM_OK;
}

} // namespace

extern "C" int glrm_hip_init_nndsvd(glrm_handle* h, double* X, double* Y, int32_t scale, int32_t zeroh, int32_t variant, int32_t max_iters,
                                    int32_t svd_max_iter, double svd_tol, uint64_t seed, double* singular_values, double* split,
                                    int32_t* iters_done) {
  if (!h) return fail(GLRM_ERR_INVALID, "glrm_hip_init_nndsvd: NULL handle");
  GLRM_REFUSE_F32(h, "glrm_hip_init_nndsvd");
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_nndsvd works on the observation lists (create the handle without dense_A)");
  if (!glrm_single_shard(h)) return fail(GLRM_ERR_INVALID, "glrm_hip_init_nndsvd needs a single-shard handle");
  GLRM_NEED_FINALIZED(h);
  for (size_t j = 0; j < h->losses_h.size(); ++j)
    if (h->losses_h[j].dim > 1)
      return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_nndsvd: column %lld has a multi-dimensional loss (kind %d, dim %d); the reference's "
                  "glrm.Y = H is k x n and has no slot for a multi-dimensional loss", (long long)j, h->losses_h[j].kind, h->losses_h[j].dim);
  if (!X || !Y) return fail(GLRM_ERR_INVALID, "glrm_hip_init_nndsvd: X / Y are NULL");
  const int k = h->k;
  const int64_t m = h->m, n = h->n;
  if (k > LMAX) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_nndsvd supports k <= %d (k = %d)", LMAX, k);
  if (k > m || k > n) return fail(GLRM_ERR_INVALID, "glrm_hip_init_nndsvd: k = %d exceeds min(m, n): no k singular triplets", k);
  if (variant == GLRM_NNDSVD_AR)
    return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_nndsvd: variant ar fills the zeros with NMF.jl's own random draws, which cannot be restated; "
                "use std or a");
  if (variant != GLRM_NNDSVD_STD && variant != GLRM_NNDSVD_A) return fail(GLRM_ERR_INVALID, "glrm_hip_init_nndsvd: unknown variant %d", variant);
  if (max_iters < 0) return fail(GLRM_ERR_INVALID, "glrm_hip_init_nndsvd: max_iters = %d is negative", max_iters);
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  const int l = block_width(k, m, n);
  const glrm_handle::Side& rs = h->side[GLRM_ROWS];
  const glrm_handle::Side& cs = h->side[GLRM_COLS];
  hipStream_t st = h->stream;
  Work w;
  DevArena scratch;
  double *T = nullptr, *stat = nullptr, *rres = nullptr, *cres = nullptr, *dX = nullptr, *dY = nullptr;
  SplitCoef* dcoef = nullptr;
  int rc;
  if ((rc = alloc_work(w, scratch, st, l, m, n, (size_t)std::max(l * l, 2 * k))) || // Gram, F Z (k l) and the 2 k norms per block
      (rc = scratch.alloc(&T, (size_t)k * l)) || (rc = scratch.alloc(&stat, (size_t)2 * LMAX)) || (rc = scratch.alloc(&dcoef, (size_t)k)) ||
      (rc = scratch.alloc(&dX, (size_t)m * k)) || (rc = scratch.alloc(&dY, (size_t)n * k)))
    return rc;
  if (max_iters > 0) {
    char what[256];
    snprintf(what, sizeof what, "glrm_hip_init_nndsvd: out of device memory for the residual arrays of the soft-impute rounds (%lld + %lld "
             "observations x 8 bytes = %.1f MiB)", (long long)rs.nnz, (long long)cs.nnz, (double)(rs.nnz + cs.nnz) * 8.0 / 1048576.0);
    if ((rc = scratch.alloc(&rres, (size_t)rs.nnz, what)) || (rc = scratch.alloc(&cres, (size_t)cs.nnz, what))) return rc;
  }
  NmfArgs ra{}, ca{};
  ra.nseg = m; ra.ptr = rs.ptr; ra.idx = rs.idx; ra.vals = rs.vals;
  ra.losses = h->losses; ra.loss_single = h->n_losses == 1 ? 1 : 0; ra.use_scale = scale ? 1 : 0;
  ra.in = w.V; ra.out = w.U; ra.l = l; ra.nsplit = 1; ra.dmax = 1; ra.k = k;
  ca = ra;
  ca.nseg = n; ca.ptr = cs.ptr; ca.idx = cs.idx; ca.vals = cs.vals; ca.in = w.U; ca.out = w.V;
  if ((rc = chunk_product(h, scratch, ca))) return rc;
  ResidArgs rr{}, cr{};
  rr.nseg = m; rr.ptr = rs.ptr; rr.idx = rs.idx; rr.vals = rs.vals; rr.losses = h->losses; rr.loss_single = ra.loss_single; rr.use_scale = ra.use_scale;
  rr.cols = 0; rr.chunk = 0; rr.Fseg = dX; rr.Fopp = dY; rr.k = k; rr.resid = rres;
  cr = rr;
  cr.nseg = n; cr.ptr = cs.ptr; cr.idx = cs.idx; cr.vals = cs.vals; cr.cols = 1; cr.chunk = ca.chunk; cr.Fseg = dY; cr.Fopp = dX; cr.resid = cres;
  const bool vec2 = k % 2 == 0;
  auto BV = [&]() { // U = B_t V
    if (ra.T) tsmm(w, dY, w.V, n, k, T);
    hipLaunchKernelGGL(nmf_rows_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, ra);
  };
  auto BtU = [&]() { // V = B_t' U
    if (ca.T) tsmm(w, dX, w.U, m, k, T);
    hipLaunchKernelGGL(nmf_cols_kernel, dim3((unsigned)n, (unsigned)ca.nsplit), dim3(256), 0, st, ca);
    if (ca.nsplit > 1) hipLaunchKernelGGL(nmf_cols_reduce_kernel, dim3((unsigned)n), dim3(256), 0, st, ca);
  };
  std::vector<double> ritz, nu, nv, x1, y1, larger((size_t)k), smaller((size_t)k);
  std::vector<SplitCoef> coef((size_t)k);
  for (int round = 0; round <= max_iters; ++round) {
    if (round > 0) { // the residuals against the factors of the round before, once per view
      if (vec2) {
        hipLaunchKernelGGL(nmf_residual_kernel<true>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, rr);
        hipLaunchKernelGGL(nmf_residual_kernel<true>, dim3((unsigned)n, (unsigned)ca.nsplit), dim3(256), 0, st, cr);
      } else {
        hipLaunchKernelGGL(nmf_residual_kernel<false>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, rr);
        hipLaunchKernelGGL(nmf_residual_kernel<false>, dim3((unsigned)n, (unsigned)ca.nsplit), dim3(256), 0, st, cr);
      }
      HIPCK(hipGetLastError());
      ra.resid = rres; ra.F = dX; ra.T = T;
      ca.resid = cres; ca.F = dY; ca.T = T;
    }
    double v0 = 0.0;
    if (variant == GLRM_NNDSVD_A) { // mean(B_t) = (sum over Omega of the sparse part + (X 1)'(Y 1)) / (m n), before X and Y are replaced
      const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (rs.nnz + 255) / 256));
      hipLaunchKernelGGL(nmf_obs_sum_kernel, dim3(nb), dim3(256), 0, st, ra, rs.nnz, w.gpart);
      hipLaunchKernelGGL(gram_reduce_kernel, dim3(1), dim3(64), 0, st, (const double*)w.gpart, nb, 1, stat);
      HIPCK(hipGetLastError());
      double total = 0.0;
      HIPCK(hipMemcpyAsync(&total, stat, 8, hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      if (round > 0) {
        if ((rc = colstat<false>(w, dX, m, k, k, stat, x1)) || (rc = colstat<false>(w, dY, n, k, k, stat, y1))) return rc;
        double dot = 0.0;
        for (int c = 0; c < k; ++c) dot = std::fma(x1[c], y1[c], dot);
        total += dot;
      }
      v0 = total / ((double)m * (double)n);
    }
    int it = 0;
    if ((rc = subspace_iterate(w, m, n, k, svd_max_iter, svd_tol, seed, BV, BtU, ritz, it))) return rc;
    if (iters_done) iters_done[round] = it;
    // the split
    if ((rc = colstat<true>(w, w.U, m, l, k, stat, nu)) || (rc = colstat<true>(w, w.V, n, l, k, stat, nv))) return rc;
    for (int c = 0; c < k; ++c) {
      const double sigma = std::sqrt(std::max(ritz[c], 0.0));
      const double xp = std::sqrt(nu[c]), xn = std::sqrt(nu[k + c]), yp = std::sqrt(nv[c]), yn = std::sqrt(nv[k + c]);
      const double mp = xp * yp, mn = xn * yn;
      const bool pos = mp >= mn;
      coef[c].sign = pos ? 1.0 : -1.0;
      coef[c].c = std::sqrt(sigma * (pos ? mp : mn));
      coef[c].xnorm = pos ? xp : xn;
      coef[c].ynorm = pos ? yp : yn;
      larger[c] = pos ? mp : mn;
      smaller[c] = pos ? mn : mp;
    }
    HIPCK(hipMemcpyAsync(dcoef, coef.data(), (size_t)k * sizeof(SplitCoef), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(nmf_split_kernel, dim3(1024), dim3(256), 0, st, (const double*)w.U, m, (const double*)w.V, n, l, k, (const SplitCoef*)dcoef, v0,
                       zeroh ? 1 : 0, dX, dY);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(st)); // coef is reused by the next round
  }
  HIPCK(hipMemcpyAsync(X, dX, (size_t)m * k * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(Y, dY, (size_t)n * k * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  if (singular_values) for (int c = 0; c < k; ++c) singular_values[c] = std::sqrt(std::max(ritz[c], 0.0));
  if (split) for (int c = 0; c < k; ++c) { split[2 * c] = larger[c]; split[2 * c + 1] = smaller[c]; }
  return GLRM_OK;
}
