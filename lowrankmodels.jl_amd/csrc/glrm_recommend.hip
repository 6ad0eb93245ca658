// glrm_recommend.hip -- include/glrm_hip_recommend.h: glrm_hip_row_topk, the kper best columns of every queried row of X'Y with the
// columns of the row's resident list left out, in ONE pass over the entries.  Nothing m x n is ever stored.
//
// u_ij comes from xy_tile (glrm_xytile.hpp), the order from xy_key: key descending, then column ascending -- a strict total order, so the
// kper best of a set of candidates are the same whichever way the set is cut into pieces and in whichever order the pieces are merged.
//
//   rowtopk_gather_kernel  rows != NULL: the queried vectors of X, copied to a contiguous buffer (ld kp) xy_tile can walk
//   rowtopk_select_kernel  workgroup (band, span): 128 query rows x the span's column tiles, ascending.  Per row the LDS holds the (key,
//                          column) of its kper-th best so far (key 0 = none yet: no value has key 0).  After xy_tile a lane tests its 64
//                          entries: one fp64 compare against the threshold's value sorts out nearly all (!(u < t) holds for every entry
//                          whose key is not below t's, and for every entry when t is a NaN); the rest are compared by (key, column) and
//                          appended to the row's RT_STAGE staging slots through an LDS cursor; an entry that finds them full stays
//                          pending.  After a barrier the waves merge row by row: staged entries that can still enter the kept list and are
//                          not in the row's list (rt_members) are inserted into the row's sorted kept list -- global scratch,
//                          [span][query][kper], held by the wave two entries per lane while it works on it -- and the new threshold is
//                          written.  The round repeats (__syncthreads_or) until no lane has a pending entry: the first tile of a span
//                          and scores ascending in j drain in several rounds.
//   rowtopk_merge_kernel   a wave per query: the spans' kept lists (each sorted) merged into the final kper, best first, and the padding.
// No global atomics, no waiting between workgroups; a workgroup only writes regions it owns.  Query rows go in blocks so that the
// scratch stays below RT_SCRATCH_BYTES.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/glrm_hip_recommend.h"
#include "glrm_engine.hpp"
#include "glrm_xytile.hpp"

namespace {

constexpr int RT_STAGE = 16;                      // staging slots per row and round
constexpr int RT_WAVES = TK_THREADS / 64;
constexpr size_t RT_SCRATCH_BYTES = 1ull << 30;   // device scratch of a block of query rows
constexpr unsigned long long RT_QNAN = 0x7FF8000000000000ull;
static_assert(GLRM_ROW_TOPK_MAX == 128, "a kept list is two entries per lane of one wave");

// xy_unkey on the device
__device__ __forceinline__ double rt_unkey(unsigned long long key) {
  const unsigned long long b = key == ~0ull ? RT_QNAN : ((key >> 63) ? (key ^ (1ull << 63)) : ~key);
  return __longlong_as_double((long long)b);
}

// THE order: key descending, then column ascending
__device__ __forceinline__ bool rt_better(unsigned long long ka, int32_t ca, unsigned long long kb, int32_t cb) { return ka > kb || (ka == kb && ca < cb); }

__device__ __forceinline__ unsigned long long rt_shfl_up1(unsigned long long v) {
  const unsigned int lo = (unsigned int)__shfl_up((int)(unsigned int)v, 1), hi = (unsigned int)__shfl_up((int)(unsigned int)(v >> 32), 1);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long rt_shfl(unsigned long long v, int src) {
  const unsigned int lo = (unsigned int)__shfl((int)(unsigned int)v, src), hi = (unsigned int)__shfl((int)(unsigned int)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

// A sorted kept list (best first) held by one wave: entry `lane` in (k0, c0), entry `lane + 64` in (k1, c1); the first n are valid.
struct RtList {
  unsigned long long k0, k1;
  int32_t c0, c1;
  int n;
};

__device__ __forceinline__ void rt_load(RtList& L, const unsigned long long* keys, const int32_t* cols, int n, int lane) {
  L.n = n; L.k0 = L.k1 = 0ull; L.c0 = L.c1 = 0;
  if (lane < n) { L.k0 = keys[lane]; L.c0 = cols[lane]; }
  if (lane + 64 < n) { L.k1 = keys[lane + 64]; L.c1 = cols[lane + 64]; }
}

__device__ __forceinline__ void rt_store(const RtList& L, unsigned long long* keys, int32_t* cols, int lane) {
  if (lane < L.n) { keys[lane] = L.k0; cols[lane] = L.c0; }
  if (lane + 64 < L.n) { keys[lane + 64] = L.k1; cols[lane + 64] = L.c1; }
}

// the entries of L that are better than (key, col): its position after insertion.  Wave-uniform.
__device__ __forceinline__ int rt_rank(const RtList& L, unsigned long long key, int32_t col, int lane) {
  return __popcll(__ballot(lane < L.n && rt_better(L.k0, L.c0, key, col))) + __popcll(__ballot(lane + 64 < L.n && rt_better(L.k1, L.c1, key, col)));
}

// insert at position p < kper; a list of kper entries loses its last
__device__ __forceinline__ void rt_place(RtList& L, int p, unsigned long long key, int32_t col, int kper, int lane) {
  const unsigned long long up0k = rt_shfl_up1(L.k0), carryk = rt_shfl(L.k0, 63);
  unsigned long long up1k = rt_shfl_up1(L.k1);
  const int32_t up0c = __shfl_up(L.c0, 1), carryc = __shfl(L.c0, 63);
  int32_t up1c = __shfl_up(L.c1, 1);
  if (lane == 0) { up1k = carryk; up1c = carryc; }
  if (lane == p) { L.k0 = key; L.c0 = col; } else if (lane > p) { L.k0 = up0k; L.c0 = up0c; }
  if (lane + 64 == p) { L.k1 = key; L.c1 = col; } else if (lane + 64 > p) { L.k1 = up1k; L.c1 = up1c; }
  if (L.n < kper) ++L.n;
}

// Which of the c staged columns of a row (scol[0 .. c)) are in list [b, e) of idx?  Bit s of the wave-uniform answer: scol[s] is.
// tk_wave_member's test, for all staged columns at once and with eight 64-entry chunks of the list in flight: a merge is latency bound,
// and these loads have no address in common with the load of the row's kept list, so one round trip serves a row of up to 512
// observations however many candidates it staged.  Columns are >= 0.
__device__ __forceinline__ unsigned int rt_members(const int32_t* idx, int64_t b, int64_t e, const int32_t* scol, int c, int lane) {
  unsigned int in = 0u;
  for (int64_t t = b; t < e; t += 8 * 64) {
    int32_t v[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const int64_t p = t + 64 * w + lane;
      v[w] = p < e ? idx[p] : -1;
    }
    for (int s = 0; s < c; ++s) {
      const int32_t col = scol[s];
      bool hit = false;
#pragma unroll
      for (int w = 0; w < 8; ++w) hit |= v[w] == col;
      if (__ballot(hit)) in |= 1u << s;
    }
  }
  return in;
}

struct RtArgs {
  TkFactors f;              // X: the query vectors of the block, f.m of them; Y, n: the model's
  const int64_t* rowid;     // the model row of query q (nullptr: row0 + q)
  int64_t row0;
  const int64_t* lptr;      // the row view (exclude = 1); lidx == nullptr: no column is left out
  const int32_t* lidx;
  int kper;
  int64_t tiles_n, span_tiles;
  unsigned long long* keys; // kept lists [span][query][kper]
  int32_t* cols;
  int32_t* cnt;             // [span][query]
};

// One round over a lane's 64 entries: the entries in `pend` are tested against their row's threshold; those that pass take a staging slot
// or stay pending.  FIRST: every entry is pending, and rows / columns past the end are sorted out.  Two steps: the fp64 test of all
// entries in registers alone (nearly all fail it), then the exact test and the append for the few that are left.  ty / tx: the lane's
// position, passed in (the caller makes them opaque per tile so that nothing derived from them is kept live across xy_tile).
template <bool FIRST>
__device__ __forceinline__ void rt_offer(const double (&u)[TK_R][TK_R], unsigned long long& pend, int ty, int tx, int64_t q0, int64_t nq, int j0, int n,
                                         const unsigned long long* thr_key, const int32_t* thr_col, unsigned int* cursor,
                                         unsigned long long* st_key, int32_t* st_col) {
  unsigned long long cand = 0ull;
#pragma unroll
  for (int a = 0; a < TK_R; ++a) {
    const double tv = rt_unkey(thr_key[tk_slot(a, ty)]); // key 0 (none yet) is a NaN pattern: everything passes the fp64 test and the key test
#pragma unroll
    for (int b = 0; b < TK_R; ++b)
      if (!(u[a][b] < tv)) cand |= 1ull << (a * TK_R + b);
  }
  if (!FIRST) cand &= pend;
  pend = 0ull;
  if (cand == 0ull) return;
#pragma unroll
  for (int a = 0; a < TK_R; ++a) {
    if (!((cand >> (a * TK_R)) & 0xffull)) continue;
    const int r = tk_slot(a, ty);
    if (FIRST && q0 + r >= nq) continue;
    const unsigned long long tk = thr_key[r];
    const int32_t tc = thr_col[r];
#pragma unroll
    for (int b = 0; b < TK_R; ++b) {
      const unsigned long long bit = 1ull << (a * TK_R + b);
      if (!(cand & bit)) continue;
      const int j = j0 + tk_slot(b, tx);
      const unsigned long long key = xy_key(u[a][b]);
      if ((FIRST && j >= n) || !rt_better(key, j, tk, tc)) continue;
      const unsigned int pos = atomicAdd(&cursor[r], 1u);
      if (pos < (unsigned int)RT_STAGE) {
        st_key[r * RT_STAGE + pos] = key;
        st_col[r * RT_STAGE + pos] = j;
      } else {
        pend |= bit;
      }
    }
  }
}

// The merge of one round: wave w takes the rows w, w + 4, ..; a row's staging area, kept list and threshold are this wave's alone.
__device__ __forceinline__ void rt_merge(const RtArgs& g, unsigned long long* gkeys, int32_t* gcols, const unsigned long long* st_key,
                                         const int32_t* st_col, unsigned int* cursor, unsigned long long* thr_key, int32_t* thr_col, int32_t* kept,
                                         const int64_t* list_b, const int64_t* list_e) {
  const int lane = threadIdx.x & 63, kper = g.kper;
  for (int r = threadIdx.x >> 6; r < TK_TILE; r += RT_WAVES) {
    const int c = __builtin_amdgcn_readfirstlane((int)min(cursor[r], (unsigned int)RT_STAGE));
    if (c == 0) continue;
    RtList L; // (r is below the block's end: rows past it stage nothing)
    rt_load(L, gkeys + (size_t)r * kper, gcols + (size_t)r * kper, __builtin_amdgcn_readfirstlane(kept[r]), lane);
    const unsigned int seen = g.lidx ? rt_members(g.lidx, list_b[r], list_e[r], st_col + r * RT_STAGE, c, lane) : 0u; // the row has observed them
    bool changed = false;
    for (int s = 0; s < c; ++s) {
      if ((seen >> s) & 1u) continue;
      const unsigned long long key = st_key[r * RT_STAGE + s];
      const int32_t col = st_col[r * RT_STAGE + s];
      const int p = rt_rank(L, key, col, lane);
      if (p >= kper) continue;                                                   // kper kept entries are better by now
      rt_place(L, p, key, col, kper, lane);
      changed = true;
    }
    if (changed) {
      rt_store(L, gkeys + (size_t)r * kper, gcols + (size_t)r * kper, lane);
      if (lane == 0) kept[r] = L.n;
      if (L.n == kper) { // the kper-th best is the new threshold
        if (kper <= 64 && lane == kper - 1) { thr_key[r] = L.k0; thr_col[r] = L.c0; }
        if (kper > 64 && lane == kper - 65) { thr_key[r] = L.k1; thr_col[r] = L.c1; }
      }
    }
    if (lane == 0) cursor[r] = 0u;
  }
}

__global__ void __launch_bounds__(TK_THREADS, 2) rowtopk_select_kernel(const RtArgs g) {
  __shared__ double xs[TK_KC * TK_LD], ys[TK_KC * TK_LD];
  __shared__ unsigned long long st_key[TK_TILE * RT_STAGE], thr_key[TK_TILE];
  __shared__ int32_t st_col[TK_TILE * RT_STAGE], thr_col[TK_TILE], kept[TK_TILE];
  __shared__ unsigned int cursor[TK_TILE];
  __shared__ int64_t list_b[TK_TILE], list_e[TK_TILE]; // the extent of every row's list, fetched once
  const int tid = threadIdx.x;
  const int64_t nq = g.f.m;
  const int n = (int)g.f.n; // columns are int32 in the lists
  const int64_t q0 = (int64_t)blockIdx.x * TK_TILE;
  const int64_t t0 = (int64_t)blockIdx.y * g.span_tiles, t1 = t0 + g.span_tiles < g.tiles_n ? t0 + g.span_tiles : g.tiles_n;
  const size_t base = ((size_t)blockIdx.y * (size_t)nq + (size_t)q0) * (size_t)g.kper; // the band's kept lists of this span
  unsigned long long* const gkeys = g.keys + base;
  int32_t* const gcols = g.cols + base;
  if (tid < TK_TILE) {
    cursor[tid] = 0u; thr_key[tid] = 0ull; thr_col[tid] = 0; kept[tid] = 0;
    list_b[tid] = list_e[tid] = 0;
    if (g.lidx && q0 + tid < nq) {
      const int64_t i = g.rowid ? g.rowid[q0 + tid] : g.row0 + q0 + tid;
      list_b[tid] = g.lptr[i]; list_e[tid] = g.lptr[i + 1];
    }
  }
  __syncthreads();
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t j0 = t * TK_TILE;
    double u[TK_R][TK_R];
    xy_tile(g.f, q0, nq, j0, xs, ys, u);
    unsigned long long pend = 0ull;
    int ty = tid >> 4, tx = tid & 15;
    asm volatile("" : "+v"(ty), "+v"(tx)); // opaque per tile: what the tests derive from the lane's position is recomputed here, not carried through xy_tile
    rt_offer<true>(u, pend, ty, tx, q0, nq, (int)j0, n, thr_key, thr_col, cursor, st_key, st_col);
    // The usual tile: nothing is pending, one merge, and u is dead before it (the barriers at the head of the next xy_tile order the merge's
    // LDS writes before the next round of tests).  Otherwise rounds of merge and re-offer, with u kept, until the tile is drained.
    if (__syncthreads_or(pend != 0ull)) {
      do {
        rt_merge(g, gkeys, gcols, st_key, st_col, cursor, thr_key, thr_col, kept, list_b, list_e);
        __syncthreads();
        rt_offer<false>(u, pend, ty, tx, q0, nq, (int)j0, n, thr_key, thr_col, cursor, st_key, st_col);
      } while (__syncthreads_or(pend != 0ull));
    }
    rt_merge(g, gkeys, gcols, st_key, st_col, cursor, thr_key, thr_col, kept, list_b, list_e);
  }
  __syncthreads();
  if (tid < TK_TILE && q0 + tid < nq) g.cnt[(size_t)blockIdx.y * (size_t)nq + (size_t)(q0 + tid)] = kept[tid];
}

__global__ void __launch_bounds__(TK_THREADS) rowtopk_gather_kernel(const double* X, const int64_t* rowid, int64_t nq, int kp, double* Xq) {
  const int64_t total = nq * kp;
  for (int64_t t = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * TK_THREADS)
    Xq[t] = X[rowid[t / kp] * kp + t % kp];
}

// a wave per query: the spans' kept lists -> the final kper (best first), the padding, the count, and how many entries were read
__global__ void __launch_bounds__(TK_THREADS) rowtopk_merge_kernel(const unsigned long long* keys, const int32_t* cols, const int32_t* cnt, int64_t nq,
                                                                   int spans, int kper, int32_t* out_cols, double* out_vals, int32_t* out_count,
                                                                   int32_t* merged) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * RT_WAVES + (threadIdx.x >> 6);
  if (q >= nq) return; // the whole wave
  RtList L;
  rt_load(L, keys + (size_t)q * kper, cols + (size_t)q * kper, __builtin_amdgcn_readfirstlane(cnt[q]), lane);
  int total = L.n;
  for (int s = 1; s < spans; ++s) {
    const size_t row = (size_t)s * (size_t)nq + (size_t)q;
    const int ns = __builtin_amdgcn_readfirstlane(cnt[row]);
    total += ns;
    for (int t = 0; t < ns; ++t) {
      const unsigned long long key = keys[row * kper + t];
      const int32_t col = cols[row * kper + t];
      const int p = rt_rank(L, key, col, lane);
      if (p >= kper) break; // the span's list is sorted: what follows is worse still
      rt_place(L, p, key, col, kper, lane);
    }
  }
  if (lane < kper) {
    out_cols[(size_t)q * kper + lane] = lane < L.n ? L.c0 : -1;
    out_vals[(size_t)q * kper + lane] = lane < L.n ? rt_unkey(L.k0) : __longlong_as_double((long long)RT_QNAN);
  }
  if (lane + 64 < kper) {
    out_cols[(size_t)q * kper + lane + 64] = lane + 64 < L.n ? L.c1 : -1;
    out_vals[(size_t)q * kper + lane + 64] = lane + 64 < L.n ? rt_unkey(L.k1) : __longlong_as_double((long long)RT_QNAN);
  }
  if (lane == 0) {
    out_count[q] = L.n;
    merged[q] = total;
  }
}

thread_local int32_t g_rt_splits = 0;
thread_local int64_t g_rt_blocks = 0, g_rt_merged = 0;

} // namespace

extern "C" int glrm_hip_row_topk_info(int32_t* col_splits_used, int64_t* row_blocks, int64_t* candidates_merged) {
  if (col_splits_used) *col_splits_used = g_rt_splits;
  if (row_blocks) *row_blocks = g_rt_blocks;
  if (candidates_merged) *candidates_merged = g_rt_merged;
  return GLRM_OK;
}

extern "C" int glrm_hip_row_topk(glrm_handle* h, const double* X, const double* Y, const int64_t* rows, int64_t n_rows, int32_t kper, int32_t exclude,
                                 int32_t col_splits, int32_t* out_cols, double* out_vals, int32_t* out_count) {
  int rc = tk_check(h, X, Y, "glrm_hip_row_topk");
  if (rc) return rc;
  const int64_t m = h->m, n = h->n;
  if (n_rows < 0) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: n_rows %lld is negative", (long long)n_rows);
  if (!rows && n_rows != 0 && n_rows != m) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: rows is NULL (the rows 0 .. m-1), so n_rows %lld must be m = %lld", (long long)n_rows, (long long)m);
  if (kper < 1) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: kper %d must be at least 1", kper);
  if (kper > GLRM_ROW_TOPK_MAX) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_row_topk: kper %d is above the limit GLRM_ROW_TOPK_MAX = %d", kper, GLRM_ROW_TOPK_MAX);
  if (exclude != 0 && exclude != 1) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: exclude %d must be 0 (none) or 1 (the row's resident list)", exclude);
  if (col_splits < 0) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: col_splits %d is negative", col_splits);
  if (!out_cols || !out_vals) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: out_cols / out_vals are NULL");
  if (rows)
    for (int64_t r = 0; r < n_rows; ++r)
      if (rows[r] < 0 || rows[r] >= m) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: rows[%lld] = %lld outside [0, m = %lld)", (long long)r, (long long)rows[r], (long long)m);
  if (n_rows == 0) return GLRM_OK;
  if (exclude && (!h->side[GLRM_ROWS].ptr || !h->side[GLRM_ROWS].idx)) return fail(GLRM_ERR_INVALID, "glrm_hip_row_topk: exclude = 1 needs the handle's row view");
  if (n <= 0) { // no candidates at all
    const double pad = xy_unkey(~0ull);
    for (int64_t t = 0; t < n_rows * kper; ++t) { out_cols[t] = -1; out_vals[t] = pad; }
    if (out_count) std::fill(out_count, out_count + n_rows, 0);
    g_rt_splits = 0; g_rt_blocks = 0; g_rt_merged = 0;
    return GLRM_OK;
  }

  TkFactors f{};
  DeviceScope dg(h->device);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", h->device);
  if ((rc = tk_factors(h, X, Y, f))) return rc;
  hipStream_t st = h->stream;
  int cus = 256;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;

  // column spans: enough workgroups for two per CU when the query rows are few; whole tiles, no empty span
  const int64_t tiles_n = (n + TK_TILE - 1) / TK_TILE, bands_all = (n_rows + TK_TILE - 1) / TK_TILE;
  int64_t want = col_splits > 0 ? col_splits : (2 * (int64_t)cus + bands_all - 1) / bands_all;
  want = std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(tiles_n, 65535)));
  const int64_t span_tiles = (tiles_n + want - 1) / want;
  const int spans = (int)((tiles_n + span_tiles - 1) / span_tiles);

  // query rows per block: kept lists of every span, the outputs, and (rows != NULL) the gathered vectors and their row ids
  const size_t per_row = (size_t)spans * ((size_t)kper * 12 + 4) + (size_t)kper * 12 + 8 + (rows ? (size_t)f.kp * 8 + 8 : 0);
  const int64_t block = std::min<int64_t>(n_rows, std::max<int64_t>(TK_TILE, (int64_t)(RT_SCRATCH_BYTES / per_row) / TK_TILE * TK_TILE));

  DevArena w;
  unsigned long long* keys = nullptr;
  int32_t *cols = nullptr, *cnt = nullptr, *d_cols = nullptr, *d_count = nullptr, *d_merged = nullptr;
  double *d_vals = nullptr, *Xq = nullptr;
  int64_t* d_rowid = nullptr;
  if ((rc = w.alloc(&keys, (size_t)spans * block * kper))) return rc;
  if ((rc = w.alloc(&cols, (size_t)spans * block * kper))) return rc;
  if ((rc = w.alloc(&cnt, (size_t)spans * block))) return rc;
  if ((rc = w.alloc(&d_cols, (size_t)block * kper))) return rc;
  if ((rc = w.alloc(&d_vals, (size_t)block * kper))) return rc;
  if ((rc = w.alloc(&d_count, (size_t)block))) return rc;
  if ((rc = w.alloc(&d_merged, (size_t)block))) return rc;
  if (rows) {
    if ((rc = w.alloc(&Xq, (size_t)block * f.kp))) return rc;
    if ((rc = w.alloc(&d_rowid, (size_t)block))) return rc;
  }
  std::vector<int32_t> count_h((size_t)block), merged_h((size_t)block);

  int64_t nblocks = 0, merged_total = 0;
  for (int64_t r0 = 0; r0 < n_rows; r0 += block, ++nblocks) {
    const int64_t nq = std::min(block, n_rows - r0), bands = (nq + TK_TILE - 1) / TK_TILE;
    RtArgs a{};
    a.f = f; a.f.m = nq;
    if (rows) {
      HIPCK(hipMemcpyAsync(d_rowid, rows + r0, (size_t)nq * 8, hipMemcpyHostToDevice, st));
      const unsigned ggrid = (unsigned)std::min<int64_t>((nq * f.kp + TK_THREADS - 1) / TK_THREADS, 1 << 20);
      hipLaunchKernelGGL(rowtopk_gather_kernel, dim3(ggrid), dim3(TK_THREADS), 0, st, f.X, (const int64_t*)d_rowid, nq, f.kp, Xq);
      a.f.X = Xq; a.rowid = d_rowid;
    } else {
      a.f.X = f.X + r0 * f.kp;
    }
    a.row0 = r0;
    a.lptr = exclude ? h->side[GLRM_ROWS].ptr : nullptr;
    a.lidx = exclude ? h->side[GLRM_ROWS].idx : nullptr;
    a.kper = kper; a.tiles_n = tiles_n; a.span_tiles = span_tiles;
    a.keys = keys; a.cols = cols; a.cnt = cnt;
    hipLaunchKernelGGL(rowtopk_select_kernel, dim3((unsigned)bands, (unsigned)spans), dim3(TK_THREADS), 0, st, a);
    hipLaunchKernelGGL(rowtopk_merge_kernel, dim3((unsigned)((nq + RT_WAVES - 1) / RT_WAVES)), dim3(TK_THREADS), 0, st, (const unsigned long long*)keys,
                       (const int32_t*)cols, (const int32_t*)cnt, nq, spans, (int)kper, d_cols, d_vals, d_count, d_merged);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out_cols + r0 * kper, d_cols, (size_t)nq * kper * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(out_vals + r0 * kper, d_vals, (size_t)nq * kper * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(count_h.data(), d_count, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(merged_h.data(), d_merged, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (out_count) std::copy(count_h.begin(), count_h.begin() + nq, out_count + r0);
    for (int64_t q = 0; q < nq; ++q) merged_total += merged_h[(size_t)q];
  }
  g_rt_splits = spans; g_rt_blocks = nblocks; g_rt_merged = merged_total;
  return GLRM_OK;
}
