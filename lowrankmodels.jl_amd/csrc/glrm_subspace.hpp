// glrm_subspace.hpp -- the randomized subspace iteration shared by glrm_svd.hip (init_svd!) and glrm_nmf.hip (init_nndsvd!): the block
// width and the work buffers, the iteration itself (subspace_iterate), the column product V <- B'U and its chunk reduce as kernel bodies
// over a unit's own value functor (cols_product_kernel, cols_reduce_kernel), partial Gram matrices of a tall-skinny block in a fixed
// order, the host eigen-decomposition of the l x l Gram matrix (l <= LMAX), Z <- Z M, the two-pass Gram orthonormalization that also
// returns the Ritz values, and the counter-based normal draws of the start block.  Everything is in an unnamed namespace: each
// translation unit that includes it gets its own copy.
// The row products U <- B V stay two kernels, one per unit: svd_rows_kernel walks d expanded vectors per observation with one gather in
// flight, nmf_rows_kernel keeps NMF_PB gathers in flight and has d == 1; a shared body would branch on its caller.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

#include "glrm_engine.hpp"

namespace {

constexpr int LMAX = 128;

// partial Gram matrices Z'Z of row blocks: thread t owns entries t, t+256, ... of the l x l matrix
constexpr int GROWS = 32;
__global__ void __launch_bounds__(256) gram_kernel(const double* Z, int64_t nrows, int l, int64_t rows_per_block, double* part) {
  __shared__ double tile[GROWS][LMAX + 1];
  const int l2 = l * l;
  double acc[LMAX * LMAX / 256];
#pragma unroll
  for (int i = 0; i < LMAX * LMAX / 256; ++i) acc[i] = 0.0;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < nrows ? r0 + rows_per_block : nrows;
  for (int64_t r = r0; r < r1; r += GROWS) {
    __syncthreads();
    for (int i = threadIdx.x; i < GROWS * l; i += 256) {
      const int rr = i / l, c = i - rr * l;
      tile[rr][c] = r + rr < r1 ? Z[(r + rr) * l + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LMAX * LMAX / 256; ++i) {
      const int ent = i * 256 + threadIdx.x;
      if (ent < l2) {
        const int p = ent / l, q = ent - p * l;
        double s = acc[i];
        for (int rr = 0; rr < GROWS; ++rr) s = fma(tile[rr][p], tile[rr][q], s);
        acc[i] = s;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < LMAX * LMAX / 256; ++i) {
    const int ent = i * 256 + threadIdx.x;
    if (ent < l2) part[(size_t)blockIdx.x * l2 + ent] = acc[i];
  }
}

__global__ void gram_reduce_kernel(const double* part, int nblk, int l2, double* G) {
  for (int ent = blockIdx.x * blockDim.x + threadIdx.x; ent < l2; ent += gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * l2 + ent];
    G[ent] = s;
  }
}

// Z <- Z * M (l x l, row-major), one wave per row
__global__ void __launch_bounds__(256) rightmul_kernel(double* Z, int64_t nrows, int l, const double* M) {
  __shared__ double zr[4][LMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r < nrows) {
    if (lane < l) zr[wave][lane] = Z[r * l + lane];
    if (lane + 64 < l) zr[wave][lane + 64] = Z[r * l + lane + 64];
  }
  __syncthreads();
  if (r >= nrows) return;
  double o0 = 0.0, o1 = 0.0;
  for (int p = 0; p < l; ++p) {
    const double z = zr[wave][p];
    if (lane < l) o0 = fma(z, M[p * l + lane], o0);
    if (lane + 64 < l) o1 = fma(z, M[p * l + lane + 64], o1);
  }
  if (lane < l) Z[r * l + lane] = o0;
  if (lane + 64 < l) Z[r * l + lane + 64] = o1;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void randn_kernel(double* V, int64_t count, uint64_t seed) { // Box-Muller on a counter-based hash
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const double u1 = ((double)(mix64(seed ^ mix64((uint64_t)i * 2 + 1)) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(mix64(seed ^ mix64((uint64_t)i * 2 + 2)) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    V[i] = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
  }
}

// cyclic Jacobi eigen-decomposition of a symmetric n x n matrix (row-major); eigenvalues descending, eigenvectors in the
// columns of E.  n <= 128: a few hundred microseconds on the host.
void jacobi_eigh(std::vector<double>& A, int n, std::vector<double>& w, std::vector<double>& E) {
  E.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) E[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) (i == j ? diag : off) += A[(size_t)i * n + j] * A[(size_t)i * n + j];
    if (off <= 1e-30 * diag || off == 0.0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int r = 0; r < n; ++r) { // columns p, q
          const double arp = A[(size_t)r * n + p], arq = A[(size_t)r * n + q];
          A[(size_t)r * n + p] = c * arp - s * arq;
          A[(size_t)r * n + q] = s * arp + c * arq;
        }
        for (int r = 0; r < n; ++r) { // rows p, q
          const double apr = A[(size_t)p * n + r], aqr = A[(size_t)q * n + r];
          A[(size_t)p * n + r] = c * apr - s * aqr;
          A[(size_t)q * n + r] = s * apr + c * aqr;
        }
        for (int r = 0; r < n; ++r) {
          const double erp = E[(size_t)r * n + p], erq = E[(size_t)r * n + q];
          E[(size_t)r * n + p] = c * erp - s * erq;
          E[(size_t)r * n + q] = s * erp + c * erq;
        }
      }
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return A[(size_t)x * n + x] > A[(size_t)y * n + y]; });
  w.resize(n);
  std::vector<double> Es((size_t)n * n);
  for (int c = 0; c < n; ++c) {
    w[c] = A[(size_t)order[c] * n + order[c]];
    for (int r = 0; r < n; ++r) Es[(size_t)r * n + c] = E[(size_t)r * n + order[c]];
  }
  E.swap(Es);
}

// the buffers both units iterate on: V [rows of V][l], U [rows of U][l], the row-block partials of the tall-skinny reductions, G and M l x l
struct Work {
  hipStream_t st;
  int l;
  double *V = nullptr, *U = nullptr, *gpart = nullptr, *G = nullptr, *M = nullptr;
};

constexpr int NBLK_MAX = 1024; // row blocks of a tall-skinny reduction

// the block: k columns plus 8 of oversampling, no wider than LMAX or than the matrix
int block_width(int k, int64_t nu, int64_t nv) { return (int)std::min<int64_t>({(int64_t)k + 8, (int64_t)LMAX, nu, nv}); }

// gpart_per_block: the widest partial a row block of the caller writes (l * l for the Gram matrices alone)
int alloc_work(Work& w, DevArena& scratch, hipStream_t st, int l, int64_t nu, int64_t nv, size_t gpart_per_block) {
  w.st = st; w.l = l;
  int rc;
  if ((rc = scratch.alloc(&w.V, (size_t)nv * l)) || (rc = scratch.alloc(&w.U, (size_t)nu * l)) || (rc = scratch.alloc(&w.gpart, (size_t)NBLK_MAX * gpart_per_block)) ||
      (rc = scratch.alloc(&w.G, (size_t)l * l)) || (rc = scratch.alloc(&w.M, (size_t)l * l)))
    return rc;
  return GLRM_OK;
}

// the row blocks of a tall-skinny reduction: their number and size are functions of nrows only
void row_blocks(int64_t nrows, int tile, int& nblk, int64_t& rpb) {
  nblk = (int)std::min<int64_t>(NBLK_MAX, (nrows + 255) / 256);
  if (nblk < 1) nblk = 1;
  rpb = ((nrows + nblk - 1) / nblk + tile - 1) / tile * tile;
  nblk = (int)((nrows + rpb - 1) / rpb);
  if (nblk < 1) nblk = 1;
}

// G = Z'Z -> eigenpairs on the host.  Returns descending eigenvalues w and eigenvectors E (row-major, columns).
int gram_eig(Work& w, const double* Z, int64_t nrows, std::vector<double>& ev, std::vector<double>& E) {
  const int l = w.l, l2 = l * l;
  int nblk;
  int64_t rpb;
  row_blocks(nrows, GROWS, nblk, rpb);
  hipLaunchKernelGGL(gram_kernel, dim3(nblk), dim3(256), 0, w.st, Z, nrows, l, rpb, w.gpart);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(16), dim3(256), 0, w.st, w.gpart, nblk, l2, w.G);
  std::vector<double> Gh((size_t)l2);
  HIPCK(hipMemcpyAsync(Gh.data(), w.G, (size_t)l2 * 8, hipMemcpyDeviceToHost, w.st));
  HIPCK(hipStreamSynchronize(w.st));
  for (int i = 0; i < l; ++i) // symmetrise against rounding
    for (int j = i + 1; j < l; ++j) { const double s = 0.5 * (Gh[(size_t)i * l + j] + Gh[(size_t)j * l + i]); Gh[(size_t)i * l + j] = Gh[(size_t)j * l + i] = s; }
  jacobi_eigh(Gh, l, ev, E);
  return GLRM_OK;
}

int rightmul(Work& w, double* Z, int64_t nrows, const std::vector<double>& Mh) {
  HIPCK(hipMemcpyAsync(w.M, Mh.data(), (size_t)w.l * w.l * 8, hipMemcpyHostToDevice, w.st));
  hipLaunchKernelGGL(rightmul_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, w.st, Z, nrows, w.l, w.M);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(w.st)); // Mh may go out of scope
  return GLRM_OK;
}

// Z <- orthonormal basis of its column space (directions with a vanishing Gram eigenvalue become zero columns).
// Pass 1 maps Z to Z E L^-1/2: the columns come out along the principal directions of Z, by descending Gram eigenvalue
// (`ritz`, `Eout`).  Pass 2 removes the rounding left by pass 1 with the symmetric inverse square root E L^-1/2 E', which is
// the identity up to rounding and therefore keeps that order.
int orthonormalize(Work& w, double* Z, int64_t nrows, std::vector<double>* ritz = nullptr, std::vector<double>* Eout = nullptr) {
  std::vector<double> ev, E;
  const int l = w.l;
  for (int pass = 0; pass < 2; ++pass) {
    int rc = gram_eig(w, Z, nrows, ev, E);
    if (rc) return rc;
    if (pass == 0 && ritz) { *ritz = ev; if (Eout) *Eout = E; }
    std::vector<double> M((size_t)l * l, 0.0);
    const double thr = ev[0] * 1e-28;
    for (int c = 0; c < l; ++c) {
      const double s = ev[c] > thr && ev[c] > 0 ? 1.0 / std::sqrt(ev[c]) : 0.0;
      if (pass == 0) {
        for (int r = 0; r < l; ++r) M[(size_t)r * l + c] = E[(size_t)r * l + c] * s;
      } else {
        for (int r = 0; r < l; ++r)
          for (int q = 0; q < l; ++q) M[(size_t)r * l + q] += E[(size_t)r * l + c] * s * E[(size_t)q * l + c];
      }
    }
    if ((rc = rightmul(w, Z, nrows, M))) return rc;
  }
  return GLRM_OK;
}

// What a unit's product kernels are handed: a view's lists, the two blocks, and for the column product its chunks (glrm_chunk_columns).
// A unit derives its own argument struct from it; for the column product that struct is also the value functor:
//   Col col(f)                 what the kernel needs of column f; Col::d expanded vectors, the first at row Col::ys of V
//   double value(col, j, t)    entry t of the column's list in expanded vector j
//   double finish(col, f, c, s) the finished sum s of component c -> what is stored
struct ProductArgs {
  int64_t nseg;
  const int64_t* ptr;
  const int32_t* idx;
  const double* vals;
  const double* in;     // rows: V;  cols: U [m][l]
  double* out;          // rows: U [m][l];  cols: V
  int l;
  int nsplit;
  int64_t chunk;
  double* partial;      // cols with nsplit > 1: [nseg][nsplit][dmax][l]
  int dmax;
};

// V[ys_f + j, :] = finish(sum_{t in Omega^f} value(j, t) U[e_t, :])     workgroup (4 waves) per (column, chunk): wave w takes the entries
// b + w, b + w + 4, ... of the chunk in order, the waves are added ((0 + 1) + 2) + 3
template <class A>
__device__ __forceinline__ void cols_product_kernel(const A& a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t f = blockIdx.x;
  const int y = blockIdx.y;
  const int l = a.l;
  const auto col = a.col(f);
  int64_t b = a.ptr[f] + (int64_t)y * a.chunk, e = b + a.chunk;
  const int64_t e0 = a.ptr[f + 1];
  b = b < e0 ? b : e0;
  e = e < e0 ? e : e0;
  __shared__ double sh[4][LMAX];
  for (int j = 0; j < col.d; ++j) {
    if (j > 0) __syncthreads();
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t t = b + wave; t < e; t += 4) {
      const double v = a.value(col, j, t);
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
      else a.out[(col.ys + j) * l + c] = a.finish(col, f, c, s);
    }
  }
}

template <class A>
__device__ __forceinline__ void cols_reduce_kernel(const A& a) { // chunk partials in chunk order
  const int64_t f = blockIdx.x;
  const int l = a.l;
  const auto col = a.col(f);
  for (int i = threadIdx.x; i < col.d * l; i += blockDim.x) {
    const int j = i / l, c = i - j * l;
    double s = 0.0;
    for (int y = 0; y < a.nsplit; ++y) s += a.partial[(((size_t)f * a.nsplit + y) * a.dmax + j) * l + c];
    a.out[(col.ys + j) * l + c] = a.finish(col, f, c, s);
  }
}

// the chunks of the column product and, where a column takes several, its partials; one chunk covers the whole list
int chunk_product(const glrm_handle* h, DevArena& scratch, ProductArgs& ca) {
  const glrm_col_chunks cc = glrm_chunk_columns(h, 16384);
  ca.nsplit = cc.nsplit;
  ca.chunk = cc.nsplit > 1 ? cc.chunk : std::max<int64_t>(cc.longest, 1);
  return cc.nsplit > 1 ? scratch.alloc(&ca.partial, (size_t)ca.nseg * ca.nsplit * ca.dmax * ca.l) : GLRM_OK;
}

// The subspace iteration on B (nu x nv, through the caller's products BV: U <- B V and BtU: V <- B'U on w.U / w.V): a seeded normal start
// block, then U <- orth(B V), V <- orth(B'U) until the first k Ritz values move by less than tol sigma_1 or max_iter passes are done.
// Leaves the right singular vectors in w.V and the left ones in w.U (columns by descending value), the squared singular values in ritz.
template <class BVf, class BtUf>
int subspace_iterate(Work& w, int64_t nu, int64_t nv, int k, int max_iter, double tol, uint64_t seed, BVf&& BV, BtUf&& BtU,
                     std::vector<double>& ritz, int& iters) {
  if (max_iter <= 0) max_iter = 60;
  if (!(tol > 0)) tol = 1e-12;
  int rc;
  hipLaunchKernelGGL(randn_kernel, dim3(1024), dim3(256), 0, w.st, w.V, nv * w.l, seed);
  if ((rc = orthonormalize(w, w.V, nv))) return rc;
  std::vector<double> prev, E;
  int it = 0;
  for (it = 1; it <= max_iter; ++it) {
    BV();
    if ((rc = orthonormalize(w, w.U, nu))) return rc;
    BtU();
    HIPCK(hipGetLastError());
    if ((rc = orthonormalize(w, w.V, nv, &ritz, &E))) return rc; // eigenvalues of (B'U)'(B'U) = squared singular values
    bool done = !prev.empty();
    for (int c = 0; c < k && done; ++c) {
      const double s = std::sqrt(std::max(ritz[c], 0.0)), sp = std::sqrt(std::max(prev[c], 0.0)), s0 = std::sqrt(std::max(ritz[0], 0.0));
      if (std::fabs(s - sp) > tol * (s0 > 0 ? s0 : 1.0)) done = false;
    }
    prev = ritz;
    if (done) break;
  }
  iters = it > max_iter ? max_iter : it;
  // After the last pass: V = orth(B'U) = right singular vectors (columns by descending value); left ones = U E.
  return rightmul(w, w.U, nu, E);
}

} // namespace
