// glrm_topk.hip -- include/glrm_hip_topk.h: glrm_hip_xy_select (the rank-th largest entry of X'Y, src/cross_validate.jl:273-274) and
// glrm_hip_precision_scan (the ordered scan for the first kprec hits, :275-297), from X and Y alone: nothing m x n is ever stored.
//
// u_ij = the ascending fma chain over the true k (the chain of dots() in glrm_impute.hip) is computed by ONE device function, xy_tile:
// a 128 x 128 tile of outputs per workgroup, 8 x 8 per lane, X and Y staged in LDS 16 components at a time.  Every kernel below that
// needs an entry calls it, so an entry has the same bits in every selection pass and in the scan.  No MFMA: its order over k is not the chain.
//
// Select: most-significant-digit radix selection over the order-preserving key of u's bit pattern (xy_key), TK_BITS = 8 bits per pass.
//   topk_hist_kernel     a fixed grid of workgroups walks the tiles (t = block, block + grid, ..); entries whose higher digits equal the
//                        prefix add 1 to counter [digit][lane & 31] of the workgroup's LDS histogram (32 copies of a digit's counter, one
//                        per bank: the lanes of a wave never meet on an address, whatever the digits are); at the end the copies are
//                        added and the workgroup stores its 256 counts to its own slot.  32-bit counters: the grid is sized so that a
//                        workgroup's share of m n stays below 2^32.
//   topk_sum_slots_kernel  256 totals (64-bit) = the slots added in slot order.  The host reads them and picks the bucket of the rank.
//   early finish         once that bucket holds at most `finish` entries (GLRM_HIP_TOPK_FINISH, default 4 Mi, 0 = never) one more pass
//                        (topk_collect_kernel) writes the bucket's keys out -- a workgroup's region starts at the exclusive sum of the
//                        counts the workgroups before it reported for that bucket, positions inside it come from an LDS counter -- a
//                        device radix sort orders them and topk_pick_kernel reads the key at the remaining rank and the extent of its
//                        run.  The order inside a region is arbitrary; the sorted keys are not.
// Integer counts only, no global atomics, no waiting between workgroups: q, n_gt and n_eq do not depend on grid, digit width or where
// the early finish happens.
//
// Scan: rows in blocks, in order.  Per block: topk_flag_kernel (xy_tile, a byte per entry with u >= q; the block's byte map is cleared
// first), topk_classify_kernel (a wave per row: for every flagged entry the wave walks the row's test list, then its train list, and
// rewrites the byte to 1 true positive / 2 false positive / 0 ignored; hits per row), topk_rowoff_kernel (exclusive sum over the block's
// rows), topk_compact_kernel (a wave per row writes its hits at the row's offset in column order: (i, j) row-major).  The host reads
// the block's total, takes what is still missing and stops launching once kprec hits are reached.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/glrm_hip_topk.h"
#include "glrm_engine.hpp"
#include "glrm_xytile.hpp"                // the tile geometry, xy_tile, xy_key, tk_wave_member, tk_check, tk_factors (shared with glrm_recommend.hip)

namespace {

constexpr int TK_BITS = 8;                // digit width
constexpr int TK_DIGITS = 1 << TK_BITS;
constexpr int TK_COPIES = 32;             // copies of a digit's counter (one per LDS bank)
// (workgroups of a selection pass -- 4 per CU, 2 are resident -- and the bucket size of the early finish: Knob::TOPK_GRID / TOPK_FINISH)
constexpr int64_t TK_BLOCK_ENTRIES = 1ll << 24; // scan: entries of a block (its byte map)
constexpr int64_t TK_BLOCK_ROWS = 1ll << 20;    // scan: rows of a block
static_assert(TK_DIGITS == TK_THREADS && 32 % TK_BITS == 0, "digit layout");

// hi = the number of low bits below the prefix (64: no prefix yet)
__device__ __forceinline__ bool tk_match(unsigned long long key, int hi, unsigned long long prefix) { return hi >= 64 || (key >> hi) == prefix; }

// What a counting pass needs of xy_key(u), in 32-bit halves (64-bit shifts and compares cost several instructions each, 64 times per
// lane and tile): does the key continue the prefix, and its digit at `shift`.  UPPER: the digit lies in the upper word (shift >= 32), where
// the lower word never matters.  prefix = the key's bits above the digit.
template <bool UPPER>
__device__ __forceinline__ bool tk_digit(double u, int shift, unsigned long long prefix, int& digit) {
  const unsigned int h = (unsigned int)__double2hiint(u), l = (unsigned int)__double2loint(u);
  const unsigned int sgn = (unsigned int)((int)h >> 31); // all ones with the sign bit set
  const bool nan = u != u;
  const unsigned int kh = nan ? ~0u : h ^ (sgn | 0x80000000u);
  if (UPPER) {
    const int s = shift - 32; // 24 (the first pass: no prefix), 16, 8, 0
    digit = (int)((kh >> s) & (TK_DIGITS - 1));
    return s == 32 - TK_BITS || (kh >> (s + TK_BITS)) == (unsigned int)prefix;
  }
  const unsigned int kl = nan ? ~0u : l ^ sgn;
  digit = (int)((kl >> shift) & (TK_DIGITS - 1));
  const int below = shift + TK_BITS; // bits of the lower word under the prefix: 8 .. 32
  if (kh != (unsigned int)(prefix >> (32 - below))) return false;
  return below == 32 || (kl >> below) == ((unsigned int)prefix & ((1u << (32 - below)) - 1u));
}

template <bool UPPER>
__global__ void __launch_bounds__(TK_THREADS, 2) topk_hist_kernel(const TkFactors f, int64_t tiles_n, int64_t ntiles, unsigned long long prefix,
                                                                  int shift, unsigned long long* slots) {
  __shared__ double xs[TK_KC * TK_LD], ys[TK_KC * TK_LD];
  __shared__ unsigned int hist[TK_DIGITS * TK_COPIES];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, copy = tid & (TK_COPIES - 1);
  for (int t = tid; t < TK_DIGITS * TK_COPIES; t += TK_THREADS) hist[t] = 0u;
  __syncthreads();
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i0 = (t / tiles_n) * TK_TILE, j0 = (t % tiles_n) * TK_TILE;
    double u[TK_R][TK_R];
    xy_tile(f, i0, f.m, j0, xs, ys, u);
#pragma unroll
    for (int a = 0; a < TK_R; ++a)
#pragma unroll
      for (int b = 0; b < TK_R; ++b) {
        int digit;
        const bool match = tk_digit<UPPER>(u[a][b], shift, prefix, digit);
        if (match && i0 + tk_slot(a, ty) < f.m && j0 + tk_slot(b, tx) < f.n) atomicAdd(&hist[digit * TK_COPIES + copy], 1u);
      }
  }
  __syncthreads();
  unsigned long long s = 0;
  for (int c = 0; c < TK_COPIES; ++c) s += hist[tid * TK_COPIES + ((c + tid) & (TK_COPIES - 1))];
  slots[(size_t)blockIdx.x * TK_DIGITS + tid] = s;
}

__global__ void __launch_bounds__(TK_THREADS) topk_sum_slots_kernel(const unsigned long long* slots, int grid, unsigned long long* totals) {
  unsigned long long s = 0;
  for (int w = 0; w < grid; ++w) s += slots[(size_t)w * TK_DIGITS + threadIdx.x];
  totals[threadIdx.x] = s;
}

// woff[w] = the entries of bucket `digit` the workgroups before w counted (woff[grid] = all of them)
__global__ void __launch_bounds__(TK_THREADS) topk_offsets_kernel(const unsigned long long* slots, int grid, int digit, unsigned long long* woff) {
  __shared__ unsigned long long part[TK_THREADS];
  const int per = (grid + TK_THREADS - 1) / TK_THREADS;
  const int b = (int)threadIdx.x * per, e = b + per < grid ? b + per : grid;
  unsigned long long s = 0;
  for (int w = b; w < e; ++w) s += slots[(size_t)w * TK_DIGITS + digit];
  part[threadIdx.x] = s;
  __syncthreads();
  unsigned long long before = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
  for (int w = b; w < e; ++w) {
    woff[w] = before;
    before += slots[(size_t)w * TK_DIGITS + digit];
  }
  if (threadIdx.x == TK_THREADS - 1) woff[grid] = before;
}

// the same walk as topk_hist_kernel (same grid): the keys under the prefix, into the workgroup's region [woff[w], woff[w + 1])
__global__ void __launch_bounds__(TK_THREADS, 2) topk_collect_kernel(const TkFactors f, int64_t tiles_n, int64_t ntiles, unsigned long long prefix,
                                                                     int hi, const unsigned long long* woff, unsigned long long* keys) {
  __shared__ double xs[TK_KC * TK_LD], ys[TK_KC * TK_LD];
  __shared__ unsigned int cursor;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  if (tid == 0) cursor = 0u;
  __syncthreads();
  const unsigned long long base = woff[blockIdx.x], room = woff[blockIdx.x + 1] - base;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i0 = (t / tiles_n) * TK_TILE, j0 = (t % tiles_n) * TK_TILE;
    double u[TK_R][TK_R];
    xy_tile(f, i0, f.m, j0, xs, ys, u);
#pragma unroll
    for (int a = 0; a < TK_R; ++a)
#pragma unroll
      for (int b = 0; b < TK_R; ++b) {
        const unsigned long long key = xy_key(u[a][b]);
        if (i0 + tk_slot(a, ty) < f.m && j0 + tk_slot(b, tx) < f.n && tk_match(key, hi, prefix)) {
          const unsigned int p = atomicAdd(&cursor, 1u);
          if (p < room) keys[base + p] = key; // (always: the region was sized by the same predicate one pass earlier)
        }
      }
  }
}

// sorted: cnt keys, descending.  out = {the key at position r - 1, the keys above it, the keys equal to it}
__global__ void topk_pick_kernel(const unsigned long long* sorted, long long cnt, long long r, unsigned long long* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long key = sorted[r - 1];
  long long lo = 0, hi = r - 1; // first position holding key
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (sorted[mid] > key) lo = mid + 1; else hi = mid;
  }
  const long long first = lo;
  lo = r - 1; hi = cnt;         // first position holding a smaller key
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (sorted[mid] >= key) lo = mid + 1; else hi = mid;
  }
  out[0] = key;
  out[1] = (unsigned long long)first;
  out[2] = (unsigned long long)(lo - first);
}

// ---- scan

__global__ void __launch_bounds__(TK_THREADS, 2) topk_flag_kernel(const TkFactors f, int64_t r0, int64_t r1, int64_t tiles_n, double q, uint8_t* codes) {
  __shared__ double xs[TK_KC * TK_LD], ys[TK_KC * TK_LD];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t t = blockIdx.x;
  const int64_t i0 = r0 + (t / tiles_n) * TK_TILE, j0 = (t % tiles_n) * TK_TILE;
  double u[TK_R][TK_R];
  xy_tile(f, i0, r1, j0, xs, ys, u);
#pragma unroll
  for (int a = 0; a < TK_R; ++a)
#pragma unroll
    for (int b = 0; b < TK_R; ++b) {
      const int64_t i = i0 + tk_slot(a, ty), j = j0 + tk_slot(b, tx);
      if (i < r1 && j < f.n && u[a][b] >= q) codes[(i - r0) * f.n + j] = 1;
    }
}

struct TkLists {
  const int64_t* train_ptr;
  const int32_t* train_idx;
  const int64_t* test_ptr;
  const int32_t* test_idx;
};

__global__ void __launch_bounds__(TK_THREADS) topk_classify_kernel(const TkLists l, int64_t r0, int64_t r1, int64_t n, uint8_t* codes, int64_t* rowcount) {
  const int lane = threadIdx.x & 63;
  const int64_t i = r0 + (int64_t)blockIdx.x * (TK_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= r1) return; // the whole wave
  const int64_t tb = l.test_ptr[i], te = l.test_ptr[i + 1], rb = l.train_ptr[i], re = l.train_ptr[i + 1];
  uint8_t* row = codes + (i - r0) * n;
  int64_t count = 0;
  for (int64_t j0 = 0; j0 < n; j0 += 64) {
    const int64_t j = j0 + lane;
    const bool flagged = j < n && row[j] != 0;
    unsigned long long todo = __ballot(flagged);
    uint8_t code = 0;
    while (todo) {
      const int who = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int32_t jj = (int32_t)(j0 + who);
      const uint8_t c = tk_wave_member(l.test_idx, tb, te, jj, lane) ? 1 : (tk_wave_member(l.train_idx, rb, re, jj, lane) ? 0 : 2);
      if (lane == who) code = c;
    }
    if (flagged) row[j] = code;
    count += __popcll(__ballot(code != 0));
  }
  if (lane == 0) rowcount[i - r0] = count;
}

// rowoff[r] = hits of the block's rows before r; rowoff[rows] = all
__global__ void __launch_bounds__(TK_THREADS) topk_rowoff_kernel(const int64_t* rowcount, int64_t rows, int64_t* rowoff) {
  __shared__ int64_t part[TK_THREADS];
  const int64_t per = (rows + TK_THREADS - 1) / TK_THREADS;
  const int64_t b = (int64_t)threadIdx.x * per < rows ? (int64_t)threadIdx.x * per : rows, e = b + per < rows ? b + per : rows;
  int64_t s = 0;
  for (int64_t r = b; r < e; ++r) s += rowcount[r];
  part[threadIdx.x] = s;
  __syncthreads();
  int64_t before = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
  for (int64_t r = b; r < e; ++r) {
    rowoff[r] = before;
    before += rowcount[r];
  }
  if (threadIdx.x == TK_THREADS - 1) rowoff[rows] = before;
}

// the first `cap` hits of the block in (i, j) row-major order: row relative to r0, column, 1 = true positive
__global__ void __launch_bounds__(TK_THREADS) topk_compact_kernel(int64_t rows, int64_t n, const uint8_t* codes, const int64_t* rowoff, int64_t cap,
                                                                  int32_t* hit_row, int32_t* hit_col, uint8_t* hit_true) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (TK_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  int64_t pos = rowoff[r];
  if (pos >= cap || rowoff[r + 1] == pos) return;
  const uint8_t* row = codes + r * n;
  for (int64_t j0 = 0; j0 < n && pos < cap; j0 += 64) {
    const int64_t j = j0 + lane;
    const uint8_t c = j < n ? row[j] : 0;
    const unsigned long long hits = __ballot(c != 0);
    const int64_t p = pos + __popcll(hits & ((1ull << lane) - 1ull));
    if (c != 0 && p < cap) {
      hit_row[p] = (int32_t)r;
      hit_col[p] = (int32_t)j;
      hit_true[p] = c == 1 ? 1 : 0;
    }
    pos += __popcll(hits);
  }
}

thread_local int32_t g_select_passes = 0;
thread_local int64_t g_select_sorted = 0;

} // namespace

extern "C" int glrm_hip_xy_select_info(int32_t* passes, int64_t* sorted_keys) {
  if (passes) *passes = g_select_passes;
  if (sorted_keys) *sorted_keys = g_select_sorted;
  return GLRM_OK;
}

extern "C" int glrm_hip_xy_select(glrm_handle* h, const double* X, const double* Y, int64_t rank, double* q, int64_t* n_gt, int64_t* n_eq) {
  int rc = tk_check(h, X, Y, "glrm_hip_xy_select");
  if (rc) return rc;
  if (!q) return fail(GLRM_ERR_INVALID, "glrm_hip_xy_select: q is NULL");
  const int64_t m = h->m, n = h->n;
  if (m <= 0 || n <= 0 || rank < 1 || (double)rank > (double)m * (double)n || rank > m * n)
    return fail(GLRM_ERR_INVALID, "glrm_hip_xy_select: rank %lld outside [1, m n = %lld x %lld] (the reference raises a BoundsError)",
                (long long)rank, (long long)m, (long long)n);
  TkFactors f{};
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  if ((rc = tk_factors(h, X, Y, f))) return rc;
  hipStream_t st = h->stream;
  const int64_t tiles_m = (m + TK_TILE - 1) / TK_TILE, tiles_n = (n + TK_TILE - 1) / TK_TILE, ntiles = tiles_m * tiles_n;
  // a workgroup's share of the entries must fit its 32-bit counters: at most 2^17 tiles of 2^14 entries
  // (GLRM_HIP_TOPK_GRID: another grid, for the tests that show the result does not depend on it)
  const int64_t want_grid = std::max(1, knob(Knob::TOPK_GRID));
  const int64_t grid64 = std::min<int64_t>(ntiles, std::max<int64_t>(want_grid, (ntiles + (1ll << 17) - 1) >> 17));
  if (grid64 > 0x7fffffffll) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_xy_select: m x n too large");
  const int grid = (int)grid64;
  const int64_t finish = knob(Knob::TOPK_FINISH);

  DevArena w;
  unsigned long long *slots = nullptr, *totals = nullptr, *woff = nullptr, *keys = nullptr, *sorted = nullptr, *picked = nullptr;
  char* tmp = nullptr;
  if ((rc = w.alloc(&slots, (size_t)grid * TK_DIGITS))) return rc;
  if ((rc = w.alloc(&totals, (size_t)TK_DIGITS))) return rc;
  if ((rc = w.alloc(&woff, (size_t)grid + 1))) return rc;
  if ((rc = w.alloc(&picked, 3))) return rc;

  unsigned long long prefix = 0, above = 0, equal = 0, key = 0;
  unsigned long long r = (unsigned long long)rank; // the rank inside the entries that still match the prefix
  int passes = 0;
  int64_t nsorted = 0;
  std::vector<unsigned long long> tot(TK_DIGITS);
  for (int shift = 64 - TK_BITS;; shift -= TK_BITS) {
    if (shift >= 32) hipLaunchKernelGGL(topk_hist_kernel<true>, dim3((unsigned)grid), dim3(TK_THREADS), 0, st, f, tiles_n, ntiles, prefix, shift, slots);
    else hipLaunchKernelGGL(topk_hist_kernel<false>, dim3((unsigned)grid), dim3(TK_THREADS), 0, st, f, tiles_n, ntiles, prefix, shift, slots);
    hipLaunchKernelGGL(topk_sum_slots_kernel, dim3(1), dim3(TK_THREADS), 0, st, (const unsigned long long*)slots, grid, totals);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(tot.data(), totals, TK_DIGITS * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    ++passes;
    int d = TK_DIGITS - 1;
    for (; d > 0 && tot[d] < r; --d) {
      r -= tot[d];
      above += tot[d];
    }
    if (tot[d] < r) return fail(GLRM_ERR_HIP, "glrm_hip_xy_select: the counts of pass %d do not cover the rank (internal error)", passes);
    prefix = (prefix << TK_BITS) | (unsigned long long)d;
    if (shift == 0) {
      key = prefix;
      equal = tot[d];
      break;
    }
    if (finish > 0 && (int64_t)tot[d] <= finish && tot[d] <= 0x7fffffffull) {
      // one more pass writes the bucket's keys out; sort, pick
      const size_t cnt = (size_t)tot[d];
      if ((rc = w.alloc(&keys, cnt))) return rc;
      if ((rc = w.alloc(&sorted, cnt))) return rc;
      hipLaunchKernelGGL(topk_offsets_kernel, dim3(1), dim3(TK_THREADS), 0, st, (const unsigned long long*)slots, grid, d, woff);
      hipLaunchKernelGGL(topk_collect_kernel, dim3((unsigned)grid), dim3(TK_THREADS), 0, st, f, tiles_n, ntiles, prefix, shift,
                         (const unsigned long long*)woff, keys);
      HIPCK(hipGetLastError());
      size_t bytes = 0;
      HIPCK(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, bytes, (const unsigned long long*)keys, sorted, (int)cnt, 0, shift, st));
      if ((rc = w.alloc(&tmp, bytes))) return rc;
      HIPCK(hipcub::DeviceRadixSort::SortKeysDescending(tmp, bytes, (const unsigned long long*)keys, sorted, (int)cnt, 0, shift, st));
      hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)sorted, (long long)cnt, (long long)r, picked);
      HIPCK(hipGetLastError());
      unsigned long long out[3];
      HIPCK(hipMemcpyAsync(out, picked, sizeof out, hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      ++passes;
      nsorted = (int64_t)cnt;
      key = out[0];
      above += out[1];
      equal = out[2];
      break;
    }
  }
  *q = xy_unkey(key);
  if (n_gt) *n_gt = (int64_t)above;
  if (n_eq) *n_eq = (int64_t)equal;
  g_select_passes = passes;
  g_select_sorted = nsorted;
  return GLRM_OK;
}

extern "C" int glrm_hip_precision_scan(glrm_handle* h, const double* X, const double* Y, double q, const int64_t* test_rowptr,
                                       const int32_t* test_colidx, int64_t kprec, int64_t block_rows, int64_t* true_pos, int64_t* false_pos,
                                       int64_t* hit_rows, int64_t* hit_cols, uint8_t* hit_is_true, int64_t* rows_scanned) {
  int rc = tk_check(h, X, Y, "glrm_hip_precision_scan");
  if (rc) return rc;
  const int64_t m = h->m, n = h->n;
  if (!true_pos || !false_pos || !test_rowptr) return fail(GLRM_ERR_INVALID, "glrm_hip_precision_scan: true_pos / false_pos / test_rowptr are NULL");
  const int nhit = (hit_rows ? 1 : 0) + (hit_cols ? 1 : 0) + (hit_is_true ? 1 : 0);
  if (nhit != 0 && nhit != 3) return fail(GLRM_ERR_INVALID, "glrm_hip_precision_scan: hit_rows, hit_cols and hit_is_true must all be given or all be NULL");
  if (block_rows < 0) return fail(GLRM_ERR_INVALID, "glrm_hip_precision_scan: block_rows %lld is negative", (long long)block_rows);
  if (test_rowptr[0] != 0) return fail(GLRM_ERR_INVALID, "glrm_hip_precision_scan: test_rowptr[0] must be 0");
  for (int64_t i = 0; i < m; ++i)
    if (test_rowptr[i + 1] < test_rowptr[i]) return fail(GLRM_ERR_INVALID, "glrm_hip_precision_scan: test_rowptr decreases at row %lld", (long long)i);
  const int64_t ntest = test_rowptr[m];
  if (ntest > 0 && !test_colidx) return fail(GLRM_ERR_INVALID, "glrm_hip_precision_scan: test_colidx is NULL");
  for (int64_t t = 0; t < ntest; ++t)
    if (test_colidx[t] < 0 || test_colidx[t] >= n)
      return fail(GLRM_ERR_INVALID, "glrm_hip_precision_scan: test_colidx[%lld] = %d outside [0, %lld)", (long long)t, test_colidx[t], (long long)n);
  *true_pos = *false_pos = 0;
  if (rows_scanned) *rows_scanned = 0;
  if (kprec <= 0) return GLRM_OK;       // the loop's first check breaks before a row is entered
  if (rows_scanned) *rows_scanned = m;
  if (q != q || m <= 0 || n <= 0) return GLRM_OK; // a NaN threshold matches nothing: the walk runs to the end

  TkFactors f{};
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  if ((rc = tk_factors(h, X, Y, f))) return rc;
  hipStream_t st = h->stream;
  DevArena lists;
  TkLists l{};
  int64_t* d_tptr = nullptr;
  int32_t* d_tidx = nullptr;
  if ((rc = lists.alloc(&d_tptr, (size_t)m + 1))) return rc;
  if ((rc = lists.alloc(&d_tidx, (size_t)ntest))) return rc;
  HIPCK(hipMemcpyAsync(d_tptr, test_rowptr, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, st));
  if (ntest > 0) HIPCK(hipMemcpyAsync(d_tidx, test_colidx, (size_t)ntest * 4, hipMemcpyHostToDevice, st));
  l.train_ptr = h->side[GLRM_ROWS].ptr; l.train_idx = h->side[GLRM_ROWS].idx; l.test_ptr = d_tptr; l.test_idx = d_tidx;

  const int64_t tiles_n = (n + TK_TILE - 1) / TK_TILE;
  const int64_t most_rows = std::max<int64_t>(1, std::min<int64_t>(TK_BLOCK_ROWS, TK_BLOCK_ENTRIES / n));
  int64_t rows = block_rows > 0 ? std::min(block_rows, most_rows) : std::min<int64_t>(TK_TILE, most_rows);
  int64_t found = 0, tp = 0, fp = 0;
  std::vector<int32_t> hr, hc;
  std::vector<uint8_t> ht;
  for (int64_t r0 = 0; r0 < m;) {
    const int64_t r1 = std::min(m, r0 + rows), nr = r1 - r0;
    const int64_t need = kprec - found, cap = std::min(need, nr * n);
    DevArena w;
    uint8_t *codes = nullptr, *d_ht = nullptr;
    int64_t *rowcount = nullptr, *rowoff = nullptr;
    int32_t *d_hr = nullptr, *d_hc = nullptr;
    if ((rc = w.alloc(&codes, (size_t)(nr * n)))) return rc;
    if ((rc = w.alloc(&rowcount, (size_t)nr))) return rc;
    if ((rc = w.alloc(&rowoff, (size_t)nr + 1))) return rc;
    if ((rc = w.alloc(&d_hr, (size_t)cap))) return rc;
    if ((rc = w.alloc(&d_hc, (size_t)cap))) return rc;
    if ((rc = w.alloc(&d_ht, (size_t)cap))) return rc;
    HIPCK(hipMemsetAsync(codes, 0, (size_t)(nr * n), st));
    const int64_t ntiles = ((nr + TK_TILE - 1) / TK_TILE) * tiles_n;
    if (ntiles > 0x7fffffffll) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_precision_scan: block too large");
    const unsigned wgrid = (unsigned)((nr + TK_THREADS / 64 - 1) / (TK_THREADS / 64));
    hipLaunchKernelGGL(topk_flag_kernel, dim3((unsigned)ntiles), dim3(TK_THREADS), 0, st, f, r0, r1, tiles_n, q, codes);
    hipLaunchKernelGGL(topk_classify_kernel, dim3(wgrid), dim3(TK_THREADS), 0, st, l, r0, r1, n, codes, rowcount);
    hipLaunchKernelGGL(topk_rowoff_kernel, dim3(1), dim3(TK_THREADS), 0, st, (const int64_t*)rowcount, nr, rowoff);
    hipLaunchKernelGGL(topk_compact_kernel, dim3(wgrid), dim3(TK_THREADS), 0, st, nr, n, (const uint8_t*)codes, (const int64_t*)rowoff, cap, d_hr, d_hc, d_ht);
    HIPCK(hipGetLastError());
    int64_t total = 0;
    HIPCK(hipMemcpyAsync(&total, rowoff + nr, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    const int64_t take = std::min(total, need);
    if (take > 0) {
      hr.resize((size_t)take); hc.resize((size_t)take); ht.resize((size_t)take);
      HIPCK(hipMemcpyAsync(hr.data(), d_hr, (size_t)take * 4, hipMemcpyDeviceToHost, st));
      HIPCK(hipMemcpyAsync(hc.data(), d_hc, (size_t)take * 4, hipMemcpyDeviceToHost, st));
      HIPCK(hipMemcpyAsync(ht.data(), d_ht, (size_t)take, hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      for (int64_t t = 0; t < take; ++t) {
        if (ht[t]) ++tp; else ++fp;
        if (hit_rows) {
          hit_rows[found + t] = r0 + hr[t];
          hit_cols[found + t] = hc[t];
          hit_is_true[found + t] = ht[t];
        }
      }
      found += take;
    }
    if (found >= kprec) { // the next row's check breaks the loop
      if (rows_scanned) *rows_scanned = r0 + hr[(size_t)take - 1] + 1;
      break;
    }
    r0 = r1;
    if (block_rows == 0) rows = std::min(most_rows, rows * 4);
  }
  *true_pos = tp;
  *false_pos = fp;
  return GLRM_OK;
}
