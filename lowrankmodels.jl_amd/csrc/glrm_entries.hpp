// glrm_entries.hpp -- what the entry points that answer for a LIST of entries of the model share (glrm_impute_at.hip:
// include/glrm_hip_impute_at.h; glrm_sample.hip: include/glrm_hip_sample.h): the three query modes and their decode, the refusals of a
// query, the partition of a block of entries by path, the bodies of the two kernels that compute u for an entry (each unit wraps them in
// kernels of its own name), and the host side that sizes, fills and partitions a block.  What is done WITH u is the including unit's: a
// functor `fin(a, e, row, col, d, us, stride)` that the bodies call once per entry (impute_value and the error there, the draw here),
// and a functor `bad(D, l, d, us, stride)` that says whether a column can be answered at all.  One definition of the value: the
// ascending fma chain over the true k from +0.0, glrm_hip_impute's.
//
// Entries go through the device in blocks of at most IA_SCRATCH_BYTES of scratch.  Inside a block:
//   ia_count / ia_scan / ia_scatter   (models with a multi-dimensional loss only) the block's entries partitioned by path into perm: the
//                          entries of scalar-loss columns first, the others after them, each part in index order.  A count per 256-entry
//                          chunk, a one-workgroup scan, a scatter by rank: no atomics.
//   ia_fast_body           scalar-loss entries, 256 per workgroup.  The chain over c is sequential, so an entry is one lane's; what the
//                          workgroup shares is the FETCH: 16 lanes read the 16 components (128 contiguous bytes, one cache line) of a
//                          piece of one vector, 32 such loads per lane and piece (16 entries x {X, Y}) are issued back to back, and the
//                          piece goes into an LDS stage [component][entry] (IA_LD = 257: the 16 components an 8-byte store's lane group
//                          of 16 writes fall into 16 different bank pairs, and the chain's reads -- lane e reads entry e -- are
//                          consecutive doubles: both are free of bank conflicts).  The loads of piece
//                          p + 1 are issued before the chain over piece p runs, so the next gather is in flight behind the arithmetic;
//                          the registers are the second buffer.  The padding components k .. kp-1 are never added.
//   ia_general_body        entries of multi-dimensional columns, one thread per entry, the d accumulators in a per-thread LDS strip
//                          like impute_kernel's; c is the OUTER loop, so x_i is read once per entry and not once per vector of Y.
// Whether a queried column can be answered is decided per COLUMN before anything runs (ia_colbad_kernel: the verdict does not depend on
// u), so a refusal writes nothing and a bad column nobody asks for is not an error.
#pragma once

#include <algorithm>
#include <vector>

#include "../../include/glrm_hip_impute_at.h"
#include "glrm_engine.hpp"
#include "glrm_impute.hpp"
#include "glrm_xytile.hpp"

namespace glrm {
namespace entries {

constexpr size_t IA_SCRATCH_BYTES = 1ull << 30;   // device scratch of a call (the bound of glrm_recommend.hip)
constexpr int IA_THREADS = 256;                   // fast path: threads = entries per workgroup
constexpr int IA_KC = 16;                         // components staged per piece: 16 doubles = one 128-byte line
constexpr int IA_LD = IA_THREADS + 1;             // doubles per staged component (odd: see ia_fast_body above)
constexpr int IA_V = IA_THREADS / 16;             // entries a lane fetches one component of
constexpr int IA_GT = 128;                        // general path: threads = entries per workgroup
constexpr int64_t IA_SLAB_LIST_MAX = 1ll << 26;   // row / column list of a slab mode (resident for the whole call)
static_assert(IA_THREADS == 16 * IA_KC && IA_LD % 16 == 1, "stage layout");

struct IaArgs {
  const double* X;          // m vectors, ld kp
  const double* Y;          // d vectors, ld kp
  int k, kp;
  int64_t m, n;
  const glrm_loss* losses;
  int loss_single;
  const int64_t* ystart;
  const glrm_domain* domains;
  int mode;
  const int64_t* rows;      // pairs: the block's rows; row slab: every queried row
  const int32_t* cols;      // pairs: the block's columns; column slab: every queried column
  int64_t n_rows;           // row slab
  int64_t t0, nb;           // the block: entries [t0, t0 + nb)
  const int32_t* perm;      // nullptr: every entry is a scalar-loss entry, in place
  const int64_t* nfast;     // with perm: the scalar-loss entries of the block (perm[0 .. *nfast))
  double* out;              // block-local
};

// entry e of the block -> (row, column)
__device__ __forceinline__ void ia_decode(const IaArgs& a, int64_t e, int64_t& row, int64_t& col) {
  if (a.mode == GLRM_IMPUTE_AT_PAIRS) {
    row = a.rows[e]; col = a.cols[e];
  } else if (a.mode == GLRM_IMPUTE_AT_ROWS) {
    const int64_t t = a.t0 + e;
    col = t / a.n_rows; row = a.rows[t - col * a.n_rows];
  } else {
    const int64_t t = a.t0 + e, c = t / a.m;
    row = t - c * a.m; col = a.cols[c];
  }
}

__device__ __forceinline__ int ia_dim(const IaArgs& a, int64_t col) {
  const int d = a.losses[a.loss_single ? 0 : col].dim;
  return d > 1 ? d : 1;
}

// the body of a unit's fast kernel: __global__ void __launch_bounds__(IA_THREADS, 2) NAME(const IaArgs a, const Fin fin)
template <class Fin>
__device__ __forceinline__ void ia_fast_body(const IaArgs& a, const Fin& fin) {
  __shared__ double xs[IA_KC * IA_LD], ys[IA_KC * IA_LD];
  __shared__ int64_t xoff[IA_THREADS], yoff[IA_THREADS]; // element offset of every entry's vectors
  const int tid = threadIdx.x;
  const int64_t cnt = a.perm ? *a.nfast : a.nb;
  const int64_t p0 = (int64_t)blockIdx.x * IA_THREADS;
  if (p0 >= cnt) return; // the whole workgroup
  const bool mine = p0 + tid < cnt;
  const int64_t p = mine ? p0 + tid : cnt - 1; // lanes past the end fetch the last entry again and write nothing
  const int64_t e = a.perm ? (int64_t)a.perm[p] : p;
  int64_t row, col;
  ia_decode(a, e, row, col);
  xoff[tid] = row * a.kp;
  yoff[tid] = a.ystart[col] * a.kp;
  const int sc = tid & (IA_KC - 1), sr = tid >> 4; // staging: component sc of the entries sr, sr + 16, ..
  double xr[IA_V], yr[IA_V];
  __syncthreads();
  {
    const int c = sc < a.k ? sc : a.k - 1; // components past k are clamped (always inside the arrays) and never added
#pragma unroll
    for (int v = 0; v < IA_V; ++v) {
      xr[v] = a.X[xoff[sr + 16 * v] + c];
      yr[v] = a.Y[yoff[sr + 16 * v] + c];
    }
  }
  double u = 0.0;
  for (int c0 = 0; c0 < a.k; c0 += IA_KC) {
    const int kc = a.k - c0 < IA_KC ? a.k - c0 : IA_KC;
    __syncthreads(); // the chain reads of the piece before
#pragma unroll
    for (int v = 0; v < IA_V; ++v) {
      xs[sc * IA_LD + sr + 16 * v] = xr[v];
      ys[sc * IA_LD + sr + 16 * v] = yr[v];
    }
    __syncthreads();
    if (c0 + IA_KC < a.k) { // the next piece: in flight behind the chain
      const int c = c0 + IA_KC + sc < a.k ? c0 + IA_KC + sc : a.k - 1;
#pragma unroll
      for (int v = 0; v < IA_V; ++v) {
        xr[v] = a.X[xoff[sr + 16 * v] + c];
        yr[v] = a.Y[yoff[sr + 16 * v] + c];
      }
    }
    for (int cc = 0; cc < kc; ++cc) u = fma(xs[cc * IA_LD + tid], ys[cc * IA_LD + tid], u);
  }
  if (mine) fin(a, e, row, col, 1, &u, 1);
}

// the body of a unit's general kernel: __global__ void __launch_bounds__(IA_GT) NAME(const IaArgs a, const Fin fin), dmax * IA_GT doubles of LDS
template <class Fin>
__device__ __forceinline__ void ia_general_body(const IaArgs& a, const Fin& fin) {
  extern __shared__ double sm[];
  double* us = sm + threadIdx.x; // the thread's strip: us[j * IA_GT]
  const int64_t nfast = *a.nfast;
  const int64_t p = nfast + (int64_t)blockIdx.x * IA_GT + threadIdx.x;
  if (p >= a.nb) return;
  const int64_t e = a.perm[p];
  int64_t row, col;
  ia_decode(a, e, row, col);
  const int d = ia_dim(a, col);
  const double* x = a.X + row * a.kp;
  const double* y = a.Y + a.ystart[col] * a.kp;
  for (int j = 0; j < d; ++j) us[j * IA_GT] = 0.0;
  for (int c = 0; c < a.k; ++c) {
    const double xc = x[c];
    for (int j = 0; j < d; ++j) us[j * IA_GT] = fma(xc, y[(int64_t)j * a.kp + c], us[j * IA_GT]);
  }
  fin(a, e, row, col, d, us, IA_GT);
}

// ---- the partition of a block by path
__device__ __forceinline__ bool ia_is_fast(const IaArgs& a, int64_t e) {
  int64_t row, col;
  ia_decode(a, e, row, col);
  return ia_dim(a, col) == 1;
}

static __global__ void __launch_bounds__(IA_THREADS) ia_count_kernel(const IaArgs a, int32_t* counts) {
  const int64_t e = (int64_t)blockIdx.x * IA_THREADS + threadIdx.x;
  const int c = __syncthreads_count(e < a.nb && ia_is_fast(a, e));
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// one workgroup: offs[chunk] = the scalar-loss entries before the chunk, *total = all of them
static __global__ void __launch_bounds__(IA_THREADS) ia_scan_kernel(const int32_t* counts, int64_t nchunks, int64_t* offs, int64_t* total) {
  __shared__ int64_t part[IA_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = (nchunks + IA_THREADS - 1) / IA_THREADS;
  const int64_t b = (int64_t)tid * per < nchunks ? (int64_t)tid * per : nchunks, en = b + per < nchunks ? b + per : nchunks;
  int64_t s = 0;
  for (int64_t c = b; c < en; ++c) s += counts[c];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < IA_THREADS; ++t) { const int64_t v = part[t]; part[t] = run; run += v; }
    *total = run;
  }
  __syncthreads();
  s = part[tid];
  for (int64_t c = b; c < en; ++c) { offs[c] = s; s += counts[c]; }
}

static __global__ void __launch_bounds__(IA_THREADS) ia_scatter_kernel(const IaArgs a, const int64_t* offs, const int64_t* total, int32_t* perm) {
  __shared__ int wfast[IA_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t e0 = (int64_t)blockIdx.x * IA_THREADS, e = e0 + tid;
  const bool in = e < a.nb, fast = in && ia_is_fast(a, e);
  const unsigned long long bal = __ballot(fast);
  if (lane == 0) wfast[w] = __popcll(bal);
  __syncthreads();
  int before = 0; // scalar-loss entries of the chunk before this lane
  for (int q = 0; q < w; ++q) before += wfast[q];
  before += __popcll(bal & ((1ull << lane) - 1ull));
  if (!in) return;
  const int64_t fb = offs[blockIdx.x];
  if (fast) perm[fb + before] = (int32_t)e;
  else perm[*total + (e0 - fb) + (tid - before)] = (int32_t)e;
}

// can column j be answered?  bad(D, l, d, us, stride) on a zero u: the verdict does not depend on u
template <class Bad>
__global__ void __launch_bounds__(IA_GT) ia_colbad_kernel(const IaArgs a, uint8_t* colbad, const Bad bad) {
  extern __shared__ double sm[];
  double* us = sm + threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * IA_GT + threadIdx.x;
  if (j >= a.n) return;
  const int d = ia_dim(a, j);
  for (int t = 0; t < d; ++t) us[t * IA_GT] = 0.0;
  colbad[j] = bad(a.domains[j], load_loss(a.losses, a.loss_single ? 0 : j), d, us, IA_GT) ? 1 : 0;
}

// ---- the host side

// the refusals of a query that need no look at the indices (nothing is touched)
inline int ia_check_shape(const glrm_domain* domains, const int64_t* rows, int64_t n_rows, const int32_t* cols, int64_t n_cols,
                          int32_t mode, const double* out, const char* what) {
  if (mode != GLRM_IMPUTE_AT_PAIRS && mode != GLRM_IMPUTE_AT_ROWS && mode != GLRM_IMPUTE_AT_COLS)
    return fail(GLRM_ERR_INVALID, "%s: mode %d must be 0 (pairs), 1 (row slab) or 2 (column slab)", what, mode);
  if (n_rows < 0 || n_cols < 0) return fail(GLRM_ERR_INVALID, "%s: n_rows %lld / n_cols %lld is negative", what, (long long)n_rows, (long long)n_cols);
  if (mode == GLRM_IMPUTE_AT_PAIRS && n_rows != n_cols) return fail(GLRM_ERR_INVALID, "%s: pairs need n_rows %lld == n_cols %lld", what, (long long)n_rows, (long long)n_cols);
  if (mode == GLRM_IMPUTE_AT_ROWS && (cols || n_cols != 0)) return fail(GLRM_ERR_INVALID, "%s: a row slab takes cols == NULL and n_cols == 0 (every column)", what);
  if (mode == GLRM_IMPUTE_AT_COLS && (rows || n_rows != 0)) return fail(GLRM_ERR_INVALID, "%s: a column slab takes rows == NULL and n_rows == 0 (every row)", what);
  if ((n_rows > 0 && !rows) || (n_cols > 0 && !cols)) return fail(GLRM_ERR_INVALID, "%s: rows / cols is NULL", what);
  if (!domains) return fail(GLRM_ERR_INVALID, "%s: domains is NULL", what);
  if (!out) return fail(GLRM_ERR_INVALID, "%s: out is NULL", what);
  return GLRM_OK;
}

// ... and those that read the descriptors and the indices; *total = the queried entries
inline int ia_check_indices(glrm_handle* h, const glrm_domain* domains, const int64_t* rows, int64_t n_rows, const int32_t* cols, int64_t n_cols,
                            int32_t mode, int64_t block_entries, const char* what, int64_t* total) {
  const int64_t m = h->m, n = h->n;
  if (block_entries < 0) return fail(GLRM_ERR_INVALID, "%s: block_entries %lld is negative", what, (long long)block_entries);
  for (int64_t f = 0; f < n; ++f)
    if (domains[f].kind < 0 || domains[f].kind >= GLRM_DOMAIN_KIND_COUNT || domains[f].reserved != 0)
      return fail(GLRM_ERR_INVALID, "%s: domain descriptor %lld is invalid", what, (long long)f);
  for (int64_t r = 0; r < n_rows; ++r)
    if (rows[r] < 0 || rows[r] >= m) return fail(GLRM_ERR_INVALID, "%s: rows[%lld] = %lld outside [0, m = %lld)", what, (long long)r, (long long)rows[r], (long long)m);
  for (int64_t c = 0; c < n_cols; ++c)
    if (cols[c] < 0 || cols[c] >= n) return fail(GLRM_ERR_INVALID, "%s: cols[%lld] = %d outside [0, n = %lld)", what, (long long)c, cols[c], (long long)n);
  if (mode != GLRM_IMPUTE_AT_PAIRS && std::max(n_rows, n_cols) > IA_SLAB_LIST_MAX)
    return fail(GLRM_ERR_UNSUPPORTED, "%s: a slab's row / column list of %lld entries is above the limit of %lld", what, (long long)std::max(n_rows, n_cols), (long long)IA_SLAB_LIST_MAX);
  *total = mode == GLRM_IMPUTE_AT_PAIRS ? n_rows : mode == GLRM_IMPUTE_AT_ROWS ? n_rows * n : m * n_cols;
  return GLRM_OK;
}

// The model's side of the kernel arguments, the domains on the device, and the verdict on every column (bad_h, host, n flags).
// *badcol = the first queried column that cannot be answered, or -1.
template <class Bad>
int ia_columns(glrm_handle* h, DevArena& w, IaArgs& a, const glrm_domain* domains, const int32_t* cols, int64_t n_cols, int32_t mode, int64_t n_rows,
               const Bad& bad, std::vector<uint8_t>& bad_h, int64_t* badcol) {
  const int64_t n = h->n;
  hipStream_t st = h->stream;
  a.k = h->k; a.kp = h->kp; a.m = h->m; a.n = n;
  a.losses = h->losses; a.loss_single = h->n_losses == 1 ? 1 : 0; a.ystart = h->ystart;
  a.mode = mode; a.n_rows = n_rows;
  glrm_domain* ddom = nullptr;
  uint8_t* colbad = nullptr;
  int rc;
  if ((rc = w.alloc(&ddom, (size_t)n)) || (rc = w.alloc(&colbad, (size_t)n))) return rc;
  HIPCK(hipMemcpyAsync(ddom, domains, (size_t)n * sizeof(glrm_domain), hipMemcpyHostToDevice, st));
  a.domains = ddom;
  bad_h.assign((size_t)n, 0);
  hipLaunchKernelGGL(ia_colbad_kernel<Bad>, dim3((unsigned)((n + IA_GT - 1) / IA_GT)), dim3(IA_GT), (size_t)h->dmax * IA_GT * 8, st, a, colbad, bad);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(bad_h.data(), colbad, (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  *badcol = -1;
  if (std::find(bad_h.begin(), bad_h.end(), (uint8_t)1) == bad_h.end()) {
    // (the usual model: every column can be answered, the queried ones need no look)
  } else if (mode == GLRM_IMPUTE_AT_ROWS) {
    for (int64_t j = 0; j < n && *badcol < 0; ++j) if (bad_h[(size_t)j]) *badcol = j;
  } else {
    for (int64_t c = 0; c < n_cols && *badcol < 0; ++c) if (bad_h[(size_t)cols[c]]) *badcol = cols[c];
  }
  return GLRM_OK;
}

// The block size of a call and the scratch every entry list needs: the indices (pairs) or the slab's list, out, and with a
// multi-dimensional loss in the model the permutation and the chunk counts of the partition.  fixed_extra / per_entry_extra: the bytes of
// the caller's own scratch, per call and per entry of a block.
struct IaBlocks {
  bool multi = false;       // some column has a multi-dimensional loss: blocks are partitioned by path
  int64_t block = 0;        // entries per block
  int64_t *d_rows = nullptr, *offs = nullptr, *d_nfast = nullptr;
  int32_t *d_cols = nullptr, *perm = nullptr, *counts = nullptr;
  double* d_out = nullptr;
};

inline int ia_blocks_alloc(glrm_handle* h, DevArena& w, IaArgs& a, const int64_t* rows, int64_t n_rows, const int32_t* cols, int64_t n_cols, int32_t mode,
                           int64_t total, int64_t block_entries, size_t fixed_extra, size_t per_entry_extra, const char* what, IaBlocks& b) {
  const int64_t n = h->n;
  hipStream_t st = h->stream;
  int rc;
  b.multi = false;
  for (const glrm_loss& l : h->losses_h) b.multi = b.multi || l.dim > 1;
  const size_t fixed = (size_t)n * (sizeof(glrm_domain) + 1) + fixed_extra + 64 + (mode == GLRM_IMPUTE_AT_ROWS ? (size_t)n_rows * 8 : 0) +
                       (mode == GLRM_IMPUTE_AT_COLS ? (size_t)n_cols * 4 : 0);
  const size_t per_entry = 8 + (mode == GLRM_IMPUTE_AT_PAIRS ? 12 : 0) + per_entry_extra + (b.multi ? 5 : 0);
  if (fixed + per_entry * IA_THREADS > IA_SCRATCH_BYTES) return fail(GLRM_ERR_UNSUPPORTED, "%s: %lld columns leave no room for a block of entries in the scratch bound", what, (long long)n);
  const int64_t cap = std::min<int64_t>((int64_t)((IA_SCRATCH_BYTES - fixed) / per_entry), 1ll << 30);
  b.block = std::min(total, block_entries > 0 ? std::min(block_entries, cap) : cap);
  const int64_t chunks_max = (b.block + IA_THREADS - 1) / IA_THREADS;
  if (mode == GLRM_IMPUTE_AT_PAIRS) {
    if ((rc = w.alloc(&b.d_rows, (size_t)b.block)) || (rc = w.alloc(&b.d_cols, (size_t)b.block))) return rc;
  } else if (mode == GLRM_IMPUTE_AT_ROWS) {
    if ((rc = w.alloc(&b.d_rows, (size_t)n_rows))) return rc;
    HIPCK(hipMemcpyAsync(b.d_rows, rows, (size_t)n_rows * 8, hipMemcpyHostToDevice, st));
  } else {
    if ((rc = w.alloc(&b.d_cols, (size_t)n_cols))) return rc;
    HIPCK(hipMemcpyAsync(b.d_cols, cols, (size_t)n_cols * 4, hipMemcpyHostToDevice, st));
  }
  if ((rc = w.alloc(&b.d_out, (size_t)b.block))) return rc;
  if (b.multi) {
    if ((rc = w.alloc(&b.perm, (size_t)b.block)) || (rc = w.alloc(&b.counts, (size_t)chunks_max)) || (rc = w.alloc(&b.offs, (size_t)chunks_max)) ||
        (rc = w.alloc(&b.d_nfast, 1)))
      return rc;
  }
  a.rows = b.d_rows; a.cols = b.d_cols; a.out = b.d_out; a.perm = b.perm; a.nfast = b.d_nfast;
  return GLRM_OK;
}

// block [t0, t0 + nb): its indices go up (pairs) and it is partitioned by path
inline int ia_block_begin(hipStream_t st, IaArgs& a, const IaBlocks& b, const int64_t* rows, const int32_t* cols, int64_t t0, int64_t nb) {
  const unsigned chunks = (unsigned)((nb + IA_THREADS - 1) / IA_THREADS);
  a.t0 = t0; a.nb = nb;
  if (a.mode == GLRM_IMPUTE_AT_PAIRS) {
    HIPCK(hipMemcpyAsync(b.d_rows, rows + t0, (size_t)nb * 8, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(b.d_cols, cols + t0, (size_t)nb * 4, hipMemcpyHostToDevice, st));
  }
  if (b.multi) {
    hipLaunchKernelGGL(ia_count_kernel, dim3(chunks), dim3(IA_THREADS), 0, st, a, b.counts);
    hipLaunchKernelGGL(ia_scan_kernel, dim3(1), dim3(IA_THREADS), 0, st, (const int32_t*)b.counts, (int64_t)chunks, b.offs, b.d_nfast);
    hipLaunchKernelGGL(ia_scatter_kernel, dim3(chunks), dim3(IA_THREADS), 0, st, a, (const int64_t*)b.offs, (const int64_t*)b.d_nfast, b.perm);
  }
  return GLRM_OK;
}

// u of every entry of the block, and fin on each, by the unit's two kernels: both grids cover the whole block, a workgroup past its
// part's end leaves at once
template <class Fin>
inline void ia_block_launch(glrm_handle* h, const IaArgs& a, const IaBlocks& b, const Fin& fin, void (*fast)(const IaArgs, const Fin),
                            void (*general)(const IaArgs, const Fin)) {
  hipStream_t st = h->stream;
  hipLaunchKernelGGL(fast, dim3((unsigned)((a.nb + IA_THREADS - 1) / IA_THREADS)), dim3(IA_THREADS), 0, st, a, fin);
  if (b.multi) hipLaunchKernelGGL(general, dim3((unsigned)((a.nb + IA_GT - 1) / IA_GT)), dim3(IA_GT), (size_t)h->dmax * IA_GT * 8, st, a, fin);
}

} // namespace entries
} // namespace glrm
