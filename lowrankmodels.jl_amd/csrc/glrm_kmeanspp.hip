// glrm_kmeanspp.hip -- glrm_hip_init_kmeanspp: init_kmeanspp!(glrm) (src/initialize.jl:8-33) on the resident row view.
//
// Row ll of Y never changes once it is set, so a row's distance to centre ll has the same bits in every later round: a running
// minimum best[i] equals the reference's recomputed minimum(d) bit for bit, and a round evaluates ONE new distance per row.
// Per round l = 1 .. k-1, all on the handle's stream, no host round trip:
//   km_distance_kernel    one pass over the row view (12 B per observation): dist = sum_j l_j(c[j], a) / len against the contiguous
//                         copy c of centre l-1 (row l-1 of Y: n doubles, gathered out of L2), best = min(best, dist), w = best
//                         (0 for the first centre's row, and only for it).  A row below KM_WAVE_FROM entries is summed by a
//                         KM_GROUP-lane group, a longer one by a whole wave: lane p takes the entries p, p + W, ... in ascending
//                         order, then an xor butterfly over the W lanes.  The shape is a function of the row's own length.
//                         Measured at 0.42 of the 12 B / observation stream floor; the suspected limit
//                         (no counter run yet) is the 8-byte gather of c, which moves a whole cache line out of L2 per entry.
//   km_chunk_sums_kernel  sums of KM_CHUNK consecutive rows of w (thread t: rows t, t + 256, ..; butterfly; the 4 waves in order)
//   km_sample_kernel      one workgroup: S = tree over the chunk sums, t = u S, then the walk `while cw < t && i < last` of wsample,
//                         level by level (spans of chunks, chunks, 32-row blocks, rows).  Shapes depend on m only.
//   km_scatter_*          A[c, obs(c)] into row l of Y and into c.  A column listed twice: the LARGEST list position writes (an
//                         integer atomicMax per entry, then the winner alone stores) -- the reference's last assignment.
// No floating-point atomics; two calls return the same bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/glrm_hip_init.h"
#include "glrm_blockreg.hpp" // block_sum
#include "glrm_device.hpp"
#include "glrm_engine.hpp"

namespace {

using namespace glrm;

constexpr int KM_THREADS = 256;
constexpr int KM_GROUP = 16;             // lanes that share a short row
constexpr int KM_ROWS_PER_WAVE = 64 / KM_GROUP;
constexpr int64_t KM_WAVE_FROM = 257;    // rows of at least this many entries take the whole wave
constexpr int KM_BATCH = 8;              // entries of a lane whose loads are in flight together (C4 rows: 8.2 ms per round at 1, 6.0 at 4, 5.65 at 8)
constexpr int KM_CHUNK = 1024;           // rows per chunk sum
constexpr int KM_SUB = 32;               // rows per block of the last but one level of the walk

struct KmArgs {
  const int64_t* rowptr;
  const int32_t* colidx;
  const double* rowvals;
  const glrm_loss* losses;
  int loss_single;
  int64_t m, n;
  int k;
  double* Y;                   // k x n, column-major
  double* c;                   // [n] the current centre, contiguous
  double* best;                // [m] running minimum of the distances
  int64_t* centers;            // [k]
  unsigned long long* lastpos; // [n] 1 + the largest list position of the column in the centre's row; 0 between scatters
};

// Lane p's share of a row's sum: the entries p, p + W, ... added in ascending order, then the butterfly over the W lanes.  The loads of
// KM_BATCH entries are issued together (index and value, then the gathers of c) so that a short row does not pay one dependent
// index -> gather round trip per entry; entries past the end are masked, and the order of the additions is the plain loop's.
template <int W, bool TRIG>
__device__ __forceinline__ double row_sum(const KmArgs& a, const LossDesc& l0, int64_t b, int64_t e, int p) {
  double s = 0.0;
  for (int64_t t = b + p; t < e; t += (int64_t)KM_BATCH * W) {
    int32_t j[KM_BATCH];
    double av[KM_BATCH], cv[KM_BATCH];
#pragma unroll
    for (int q = 0; q < KM_BATCH; ++q) {
      const int64_t tt = t + (int64_t)q * W;
      j[q] = tt < e ? a.colidx[tt] : 0;
      av[q] = tt < e ? a.rowvals[tt] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < KM_BATCH; ++q) cv[q] = a.c[j[q]];
#pragma unroll
    for (int q = 0; q < KM_BATCH; ++q) {
      if (t + (int64_t)q * W < e) {
        const LossDesc l = a.loss_single ? l0 : load_loss(a.losses, j[q]);
        double L, dL;
        loss_both<false, TRIG>(l, cv[q], av[q], L, dL);
        s += L;
      }
    }
  }
#pragma unroll
  for (int d = 1; d < W; d <<= 1) s += __shfl_xor(s, d, 64);
  return s;
}

template <bool TRIG>
__global__ void __launch_bounds__(KM_THREADS) km_distance_kernel(const KmArgs a, int first_round, double* w) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = ((int64_t)blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6)) * KM_ROWS_PER_WAVE;
  if (r0 >= a.m) return; // the whole wave
  const int g = lane / KM_GROUP, p = lane % KM_GROUP;
  const int64_t i = r0 + g;
  int64_t b = 0, e = 0;
  if (i < a.m) {
    b = a.rowptr[i];
    e = a.rowptr[i + 1];
  }
  const int64_t len = e - b;
  const LossDesc l0 = load_loss(a.losses, 0);
  const bool short_row = len < KM_WAVE_FROM;
  // every lane runs the butterfly; the groups of long and of missing rows walk an empty range
  double s = row_sum<KM_GROUP, TRIG>(a, l0, short_row ? b : 0, short_row ? e : 0, p);
  for (int gg = 0; gg < KM_ROWS_PER_WAVE; ++gg) { // wave-uniform control flow
    const int64_t ii = r0 + gg;
    if (ii >= a.m) break;
    const int64_t bb = a.rowptr[ii], ee = a.rowptr[ii + 1];
    if (ee - bb < KM_WAVE_FROM) continue;
    const double sl = row_sum<64, TRIG>(a, l0, bb, ee, lane);
    if (gg == g) s = sl;
  }
  if (i < a.m && p == 0) {
    const double dist = s / (double)len; // 0 / 0 = NaN for a row without observations
    const double old = first_round ? __builtin_inf() : a.best[i];
    double nb = dist < old ? dist : old;  // Julia's minimum: a NaN stays
    if (dist != dist) nb = dist;
    a.best[i] = nb;
    w[i] = i == a.centers[0] ? 0.0 : nb;  // only the first centre ever leaves possible_centers
  }
}

__global__ void __launch_bounds__(KM_THREADS) km_chunk_sums_kernel(const double* w, int64_t m, double* chunksum) {
  __shared__ double sh[KM_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * KM_CHUNK;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < KM_CHUNK / KM_THREADS; ++q) {
    const int64_t i = base + q * KM_THREADS + threadIdx.x;
    s += i < m ? w[i] : 0.0;
  }
  s = block_sum<KM_THREADS / 64>(s, sh);
  if (threadIdx.x == 0) chunksum[blockIdx.x] = s;
}

// wsample's loop on one level: the first of the cnt values at which the running sum (continued from `before`) reaches t, else the
// last; `before` becomes the running sum in front of it.  A NaN t compares false at once: index 0.
__device__ __forceinline__ int64_t km_walk(const double* v, int64_t cnt, double t, double& before) {
  int64_t i = 0;
  double cw = before + v[0];
  while (cw < t && i < cnt - 1) {
    before = cw;
    ++i;
    cw = before + v[i];
  }
  return i;
}

__global__ void __launch_bounds__(KM_THREADS) km_sample_kernel(const double* w, int64_t m, const double* chunksum, int64_t nchunks,
                                                               const double* u, int round, int64_t* centers) {
  __shared__ double sh[KM_THREADS / 64];
  __shared__ double span[KM_THREADS];
  __shared__ double rows[KM_CHUNK];
  __shared__ double sub[KM_CHUNK / KM_SUB];
  __shared__ int64_t s_chunk;
  __shared__ double s_before;
  const int tid = threadIdx.x;
  const int64_t per = (nchunks + KM_THREADS - 1) / KM_THREADS; // chunks per span
  const int64_t nspan = (nchunks + per - 1) / per;
  double s = 0.0;
  {
    const int64_t cb = (int64_t)tid * per;
    const int64_t ce = cb + per < nchunks ? cb + per : nchunks;
    for (int64_t c = cb; c < ce; ++c) s += chunksum[c];
  }
  span[tid] = s;
  const double S = block_sum<KM_THREADS / 64>(s, sh);
  const double t = u[round - 1] * S;
  if (tid == 0) {
    double before = 0.0;
    const int64_t sp = km_walk(span, nspan, t, before);
    const int64_t c0 = sp * per;
    const int64_t cnt = per < nchunks - c0 ? per : nchunks - c0;
    s_chunk = c0 + km_walk(chunksum + c0, cnt, t, before);
    s_before = before;
  }
  __syncthreads();
  const int64_t base = s_chunk * KM_CHUNK;
  const int nrows = (int)(m - base < KM_CHUNK ? m - base : KM_CHUNK);
#pragma unroll
  for (int q = 0; q < KM_CHUNK / KM_THREADS; ++q) {
    const int r = q * KM_THREADS + tid;
    rows[r] = r < nrows ? w[base + r] : 0.0;
  }
  __syncthreads();
  if (tid < KM_CHUNK / KM_SUB) {
    double ss = 0.0;
    for (int r = 0; r < KM_SUB; ++r) ss += rows[tid * KM_SUB + r];
    sub[tid] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    double before = s_before;
    const int nsub = (nrows + KM_SUB - 1) / KM_SUB;
    const int sb = (int)km_walk(sub, nsub, t, before);
    const int cnt = nrows - sb * KM_SUB < KM_SUB ? nrows - sb * KM_SUB : KM_SUB;
    const int r = (int)km_walk(rows + sb * KM_SUB, cnt, t, before);
    centers[round] = base + sb * KM_SUB + r;
  }
}

// c = row l of Y as it stands (the randn draw), and per column of the centre's list the largest list position
__global__ void __launch_bounds__(KM_THREADS) km_scatter_mark_kernel(const KmArgs a, int l) {
  const int64_t ctr = a.centers[l];
  const int64_t b = a.rowptr[ctr], e = a.rowptr[ctr + 1];
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = t0; j < a.n; j += stride) a.c[j] = a.Y[l + (int64_t)a.k * j];
  for (int64_t t = b + t0; t < e; t += stride) atomicMax(&a.lastpos[a.colidx[t]], (unsigned long long)(t - b + 1));
}

// the entry at that position stores (row l of Y, c) and clears the mark for the next scatter.  Entries that lost a duplicated column read
// lastpos[j] while the winner may be clearing it in this same launch, without atomics: they see either the winner's position + 1 or 0,
// and neither equals their own position + 1 (which is >= 1 and below the maximum), so they never store.
__global__ void __launch_bounds__(KM_THREADS) km_scatter_write_kernel(const KmArgs a, int l) {
  const int64_t ctr = a.centers[l];
  const int64_t b = a.rowptr[ctr], e = a.rowptr[ctr + 1];
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = b + t0; t < e; t += stride) {
    const int64_t j = a.colidx[t];
    if (a.lastpos[j] == (unsigned long long)(t - b + 1)) {
      const double v = a.rowvals[t];
      a.Y[l + (int64_t)a.k * j] = v;
      a.c[j] = v;
      a.lastpos[j] = 0ull;
    }
  }
}

struct KmWork {
  double *Y = nullptr, *c = nullptr, *best = nullptr, *w = nullptr, *u = nullptr, *chunksum = nullptr;
  int64_t* centers = nullptr;
  unsigned long long* lastpos = nullptr;
};

} // namespace

extern "C" int glrm_hip_init_kmeanspp(glrm_handle* h, double* Y, int64_t first_center, const double* u, int64_t* centers, double* weights) {
  if (!h) return fail(GLRM_ERR_INVALID, "glrm_hip_init_kmeanspp: NULL handle");
  GLRM_REFUSE_F32(h, "glrm_hip_init_kmeanspp");
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_kmeanspp works on the observation lists (create the handle without dense_A)");
  if (!glrm_single_shard(h)) return fail(GLRM_ERR_INVALID, "glrm_hip_init_kmeanspp needs a single-shard handle");
  GLRM_NEED_FINALIZED(h);
  for (size_t j = 0; j < h->losses_h.size(); ++j)
    if (h->losses_h[j].dim > 1)
      return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_init_kmeanspp: column %lld has a multi-dimensional loss (kind %d, dim %d); the reference's "
                  "Y = randn(k, n) has no slot for a multi-dimensional loss", (long long)j, h->losses_h[j].kind, h->losses_h[j].dim);
  if (!Y || !centers) return fail(GLRM_ERR_INVALID, "glrm_hip_init_kmeanspp: Y / centers are NULL");
  const int k = h->k;
  const int64_t m = h->m, n = h->n;
  if (k > 1 && !u) return fail(GLRM_ERR_INVALID, "glrm_hip_init_kmeanspp: u is NULL (k - 1 = %d draws are needed)", k - 1);
  if (first_center < 0 || first_center >= m)
    return fail(GLRM_ERR_INVALID, "glrm_hip_init_kmeanspp: first_center %lld outside [0, %lld)", (long long)first_center, (long long)m);
  for (int l = 0; l + 1 < k; ++l)
    if (!(u[l] >= 0.0 && u[l] < 1.0)) return fail(GLRM_ERR_INVALID, "glrm_hip_init_kmeanspp: u[%d] = %g outside [0, 1)", l, u[l]);
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  hipStream_t st = h->stream;
  const int rounds = k - 1;
  const int64_t nchunks = (m + KM_CHUNK - 1) / KM_CHUNK;
  const size_t wrounds = weights && rounds > 0 ? (size_t)rounds : 1;

  KmWork w;
  DevArena scratch;
  int rc;
  if ((rc = scratch.alloc(&w.Y, (size_t)k * n)) || (rc = scratch.alloc(&w.c, (size_t)n)) || (rc = scratch.alloc(&w.best, (size_t)m)) ||
      (rc = scratch.alloc(&w.w, wrounds * (size_t)m)) || (rc = scratch.alloc(&w.u, (size_t)std::max(rounds, 0))) || (rc = scratch.alloc(&w.chunksum, (size_t)nchunks)) ||
      (rc = scratch.alloc(&w.centers, (size_t)k)) || (rc = scratch.alloc(&w.lastpos, (size_t)n)))
    return rc;
  HIPCK(hipMemcpyAsync(w.Y, Y, (size_t)k * n * 8, hipMemcpyHostToDevice, st));
  if (rounds > 0) HIPCK(hipMemcpyAsync(w.u, u, (size_t)rounds * 8, hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(w.centers, &first_center, 8, hipMemcpyHostToDevice, st));
  HIPCK(hipMemsetAsync(w.lastpos, 0, (size_t)n * 8, st));

  KmArgs a{};
  a.rowptr = h->side[GLRM_ROWS].ptr; a.colidx = h->side[GLRM_ROWS].idx; a.rowvals = h->side[GLRM_ROWS].vals;
  a.losses = h->losses; a.loss_single = h->n_losses == 1 ? 1 : 0;
  a.m = m; a.n = n; a.k = k;
  a.Y = w.Y; a.c = w.c; a.best = w.best; a.centers = w.centers; a.lastpos = w.lastpos;

  // the centre's row length is known on the device only: grid-stride launches sized for the longest row and the n columns
  const int64_t span = std::max<int64_t>(n, h->sig.max_row_len);
  const unsigned sgrid = (unsigned)std::min<int64_t>(1024, std::max<int64_t>(1, (span + KM_THREADS - 1) / KM_THREADS));
  const unsigned dgrid = (unsigned)((m + (KM_THREADS / 64) * KM_ROWS_PER_WAVE - 1) / ((KM_THREADS / 64) * KM_ROWS_PER_WAVE));
  auto scatter = [&](int l) {
    hipLaunchKernelGGL(km_scatter_mark_kernel, dim3(sgrid), dim3(KM_THREADS), 0, st, a, l);
    hipLaunchKernelGGL(km_scatter_write_kernel, dim3(sgrid), dim3(KM_THREADS), 0, st, a, l);
  };
  scatter(0);
  for (int l = 1; l <= rounds; ++l) {
    double* wl = w.w + (weights ? (size_t)(l - 1) * m : 0);
    if (h->has_trig) hipLaunchKernelGGL(km_distance_kernel<true>, dim3(dgrid), dim3(KM_THREADS), 0, st, a, l == 1 ? 1 : 0, wl);
    else hipLaunchKernelGGL(km_distance_kernel<false>, dim3(dgrid), dim3(KM_THREADS), 0, st, a, l == 1 ? 1 : 0, wl);
    hipLaunchKernelGGL(km_chunk_sums_kernel, dim3((unsigned)nchunks), dim3(KM_THREADS), 0, st, (const double*)wl, m, w.chunksum);
    hipLaunchKernelGGL(km_sample_kernel, dim3(1), dim3(KM_THREADS), 0, st, (const double*)wl, m, (const double*)w.chunksum, nchunks,
                       (const double*)w.u, l, w.centers);
    scatter(l);
  }
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(centers, w.centers, (size_t)k * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(Y, w.Y, (size_t)k * n * 8, hipMemcpyDeviceToHost, st));
  if (weights && rounds > 0) HIPCK(hipMemcpyAsync(weights, w.w, (size_t)rounds * m * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  return GLRM_OK;
}
