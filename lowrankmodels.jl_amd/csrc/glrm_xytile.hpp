// glrm_xytile.hpp -- what the translation units that walk X'Y tile by tile share (glrm_topk.hip: include/glrm_hip_topk.h; glrm_recommend.hip:
// include/glrm_hip_recommend.h): the tile geometry, THE definition of u_ij on the device (xy_tile), the order-preserving key of a value,
// the wave-wide list membership test, and the refusals and the factor upload every such entry point starts with (glrm_impute_at.hip:
// include/glrm_hip_impute_at.h takes the handle and factor parts of those alone).  One definition each: an entry of X'Y has the same bits,
// and the same place in the order, whichever kernel asks for it.
#pragma once

#include <cstring>

#include "../../include/glrm_hip_topk.h"
#include "glrm_engine.hpp"

constexpr int TK_THREADS = 256;
constexpr int TK_TILE = 128;              // outputs per workgroup: TK_TILE x TK_TILE
constexpr int TK_R = 8;                   // outputs per lane: TK_R x TK_R (16 x 16 lanes)
constexpr int TK_KC = 16;                 // components of X and Y staged per trip
constexpr int TK_LD = TK_TILE + 2;        // doubles per staged component: the 16 components a lane group stores together fall into 16 banks
static_assert(TK_TILE == 16 * TK_R && TK_THREADS == 256 && TK_THREADS == 16 * TK_KC && TK_LD % 2 == 0, "tile layout");

struct TkFactors {
  const double* X;  // m vectors, ld kp
  const double* Y;  // n vectors, ld kp
  int k, kp;
  int64_t m, n;
};

// Order-preserving key of a double under Julia's isless: -Inf < .. < -0.0 < +0.0 < .. < +Inf < NaN, every NaN one value.
__host__ __device__ __forceinline__ unsigned long long xy_key(double u) {
  if (u != u) return ~0ull;
  unsigned long long b;
#ifdef __HIP_DEVICE_COMPILE__
  b = (unsigned long long)__double_as_longlong(u);
#else
  memcpy(&b, &u, 8);
#endif
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

inline double xy_unkey(unsigned long long key) {
  unsigned long long b = key == ~0ull ? 0x7FF8000000000000ull : ((key >> 63) ? (key ^ (1ull << 63)) : ~key);
  double u;
  memcpy(&u, &b, 8);
  return u;
}

// Row / column of the a-th output of lane position p (0..15) inside a tile: pairs of neighbours, 32 apart -- a lane's two neighbours are
// one 16-byte LDS read, and the 16 positions of a wave read 256 contiguous bytes.
__device__ __forceinline__ int tk_slot(int a, int p) { return 32 * (a >> 1) + 2 * p + (a & 1); }

// THE definition of u_ij on the device: u[a][b] = fma chain, c ascending over the true k, for row i0 + tk_slot(a, ty) (below row_end) and
// column j0 + tk_slot(b, tx).  xs / ys: TK_KC x TK_LD doubles each.  Rows and columns past the end are staged as zeros; their outputs
// are never read.
__device__ __forceinline__ void xy_tile(const TkFactors& f, int64_t i0, int64_t row_end, int64_t j0, double* xs, double* ys, double (&u)[TK_R][TK_R]) {
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int sc = tid & (TK_KC - 1), sr = tid >> 4; // staging: component sc of the vectors sr, sr + 16, ..: 16 lanes read 128 contiguous bytes
#pragma unroll
  for (int a = 0; a < TK_R; ++a)
#pragma unroll
    for (int b = 0; b < TK_R; ++b) u[a][b] = 0.0;
  for (int c0 = 0; c0 < f.k; c0 += TK_KC) {
    const int kc = f.k - c0 < TK_KC ? f.k - c0 : TK_KC;
    __syncthreads(); // the reads of the trip (or tile) before
    {
      // every load is issued before the first is waited for: addresses past the end are clamped to the last vector / component (always
      // inside the arrays: i0 < row_end, j0 < n, k >= 1) and the value is replaced by zero afterwards
      const bool in = c0 + sc < f.k;
      const int c = in ? c0 + sc : f.k - 1;
      double xr[TK_TILE / 16], yr[TK_TILE / 16];
#pragma unroll
      for (int v = 0; v < TK_TILE / 16; ++v) {
        const int64_t gi = i0 + sr + 16 * v, gj = j0 + sr + 16 * v;
        xr[v] = f.X[(gi < row_end ? gi : row_end - 1) * f.kp + c];
        yr[v] = f.Y[(gj < f.n ? gj : f.n - 1) * f.kp + c];
      }
#pragma unroll
      for (int v = 0; v < TK_TILE / 16; ++v) {
        const int r = sr + 16 * v;
        xs[sc * TK_LD + r] = (in && i0 + r < row_end) ? xr[v] : 0.0;
        ys[sc * TK_LD + r] = (in && j0 + r < f.n) ? yr[v] : 0.0;
      }
    }
    __syncthreads();
    for (int cc = 0; cc < kc; ++cc) {
      double xv[TK_R], yv[TK_R];
#pragma unroll
      for (int a = 0; a < TK_R; ++a) {
        xv[a] = xs[cc * TK_LD + tk_slot(a, ty)];
        yv[a] = ys[cc * TK_LD + tk_slot(a, tx)];
      }
#pragma unroll
      for (int a = 0; a < TK_R; ++a)
#pragma unroll
        for (int b = 0; b < TK_R; ++b) u[a][b] = fma(xv[a], yv[b], u[a][b]);
    }
  }
}

// is column j in list [b, e) of idx?  The whole wave walks the list; the answer is wave-uniform.
__device__ __forceinline__ bool tk_wave_member(const int32_t* idx, int64_t b, int64_t e, int32_t j, int lane) {
  for (int64_t t = b; t < e; t += 64) {
    const bool hit = t + lane < e && idx[t + lane] == j;
    if (__ballot(hit)) return true;
  }
  return false;
}

// the refusals the entries share (nothing is touched), in three parts: the handle, the model (one vector of Y per column: what an entry
// point that walks X'Y by column needs, and glrm_hip_impute_at does not), the factors
inline int xy_check_handle(glrm_handle* h, const char* what) {
  if (!h) return fail(GLRM_ERR_INVALID, "%s: NULL handle", what);
  GLRM_REFUSE_F32(h, what);
  if (h->dense) return fail(GLRM_ERR_UNSUPPORTED, "%s works on the observation lists (create the handle without dense_A)", what);
  if (!glrm_single_shard(h)) return fail(GLRM_ERR_INVALID, "%s needs a single-shard handle", what);
  GLRM_NEED_FINALIZED(h);
  return GLRM_OK;
}

inline int xy_check_factors(glrm_handle* h, const double* X, const double* Y, const char* what) {
  if ((X == nullptr) != (Y == nullptr)) return fail(GLRM_ERR_INVALID, "%s: X and Y must both be given or both be NULL (NULL = the handle's resident factors)", what);
  if (!X && (!h->side[GLRM_ROWS].factor || !h->side[GLRM_COLS].factor)) return fail(GLRM_ERR_INVALID, "%s: no factors on the device yet (pass X and Y, or fit / glrm_hip_set_factors first)", what);
  return GLRM_OK;
}

inline int tk_check(glrm_handle* h, const double* X, const double* Y, const char* what) {
  const int rc = xy_check_handle(h, what);
  if (rc) return rc;
  for (size_t j = 0; j < h->losses_h.size(); ++j)
    if (h->losses_h[j].dim > 1)
      return fail(GLRM_ERR_UNSUPPORTED, "%s: column %lld has a multi-dimensional loss (kind %d, dim %d); XY[i,j] with j in 1:n needs one vector "
                  "of Y per data column (d == n)", what, (long long)j, h->losses_h[j].kind, h->losses_h[j].dim);
  if (h->d != h->n) return fail(GLRM_ERR_UNSUPPORTED, "%s: Y has %lld vectors for %lld columns (d != n)", what, (long long)h->d, (long long)h->n);
  return xy_check_factors(h, X, Y, what);
}

// after every argument check, inside the entry point's device scope: the factors, uploaded like glrm_hip_impute does it
inline int tk_factors(glrm_handle* h, const double* X, const double* Y, TkFactors& f) {
  if (X) {
    const int rc = glrm_hip_set_factors(h, X, Y);
    if (rc) return rc;
  }
  f.X = h->side[GLRM_ROWS].factor; f.Y = h->side[GLRM_COLS].factor; f.k = h->k; f.kp = h->kp; f.m = h->m; f.n = h->n;
  return GLRM_OK;
}
