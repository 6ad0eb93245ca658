// glrm_scale.hip -- glrm_hip_scale_columns: equilibrate_variance! / prob_scale! (src/modify_glrm.jl:31-82) on the column stream.
//
// One workgroup (4 waves) per column, in the column's list order.  Per column, each pass only for the kinds that need it:
//   (a) sum a, sum sin / cos (Periodic), #(a != 0), #(a > 0)                      -> mean and the closed-form M-estimates
//   (b) an exact order statistic (L1 / Huber / OrdinalHinge median, Quantile): MSB-first radix select, 8 bits per round, on the
//       order-preserving 64-bit key of the double with an LDS histogram per digit (integer LDS atomics: any arrival order gives the
//       same counts).  Columns of at most SC_LDS_MAX entries are staged in LDS by pass (a) and selected there; longer ones re-read
//       the stream once per digit.  The upper neighbour (even nobs / interpolation) is the same value when the final bin holds
//       more copies than the rank needs, else the minimum key above -- one more pass.
//   (c) sum (a - mean)^2 and sum l(M, a) with the device evaluator of the sweeps (glrm_device.hpp: loss_both)
// Thread t of the 256 takes the entries t, t + 256, ... in ascending order into its own accumulators; the 64 lanes of a wave are added
// by an xor butterfly, the 4 waves in ascending order.  That shape and the SC_LDS_MAX switch (which does not touch any sum) are
// functions of the column's own length: a column block gives the bits of the whole call.  No floating-point atomics.
// The rules that turn (nobs, avg_loss, variance) into scales are applied on the host below, in one place.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/glrm_hip_scale.h"
#include "glrm_device.hpp"
#include "glrm_engine.hpp"

namespace {

using namespace glrm;

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_LDS_MAX = 4096; // entries of a column staged in LDS for the selection (32 KB of keys)

struct ScaleArgs {
  const int64_t* colptr;
  const double* colvals;
  const glrm_loss* losses; // device; entry j (or 0 with loss_single) belongs to local column j
  int loss_single;
  int mode;
  int64_t nl;
  double* stats; // [4][nl]: nobs, m_est, avg_loss, variance
};

// order-preserving key: a < b <=> key(a) < key(b); the two zeros share one key
__device__ __forceinline__ uint64_t key_of(double a) {
  if (a == 0.0) a = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(a);
  return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
  const uint64_t b = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
  return __longlong_as_double((long long)b);
}

__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ uint64_t block_min(uint64_t v, uint64_t* sh) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    v = o < v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t m = sh[0];
#pragma unroll
  for (int w = 1; w < SC_WAVES; ++w) m = sh[w] < m ? sh[w] : m;
  return m;
}

// one count into the digit histogram.  The leading bytes of a column's keys (sign, exponent) are nearly constant, so most lanes of a
// wave hit one bin: two rounds of "the first lane's digit is added once for all lanes that share it" take those out before the
// remaining lanes issue their own LDS atomics.
__device__ __forceinline__ void hist_add(unsigned long long* hist, bool valid, unsigned digit) {
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long live = __ballot(valid);
    if (live == 0) return;
    const int leader = __ffsll((long long)live) - 1;
    const unsigned ld = (unsigned)__shfl((int)digit, leader, 64);
    const unsigned long long same = __ballot(valid && digit == ld);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[ld], (unsigned long long)__popcll(same));
    if (digit == ld) valid = false;
  }
  if (valid) atomicAdd(&hist[digit], 1ull);
}

template <bool TRIG>
__global__ void __launch_bounds__(SC_THREADS) scale_kernel(const ScaleArgs a) {
  __shared__ uint64_t keys[SC_LDS_MAX];
  __shared__ unsigned long long hist[256];
  __shared__ unsigned long long wtot[SC_WAVES];
  __shared__ double shd[SC_WAVES];
  __shared__ uint64_t shu[SC_WAVES];
  __shared__ uint64_t sel_prefix;
  __shared__ unsigned long long sel_rank, sel_cnt;

  const int64_t j = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LossDesc l = load_loss(a.losses, a.loss_single ? 0 : j);
  const int64_t b = a.colptr[j], N = a.colptr[j + 1] - b;
  const double* v = a.colvals + b;
  const double nan = __builtin_nan("");
  double* out_nobs = a.stats + j;
  double* out_m = a.stats + a.nl + j;
  double* out_avg = a.stats + 2 * a.nl + j;
  double* out_var = a.stats + 3 * a.nl + j;

  const int kind = l.kind;
  const bool prob = a.mode == GLRM_SCALE_PROB;
  const bool need_loss = !prob || kind == GLRM_LOSS_HUBER;
  const bool need_var = !prob || kind == GLRM_LOSS_QUAD;
  if (N <= 0 || (!need_loss && !need_var)) { // uniform over the workgroup
    if (tid == 0) {
      *out_nobs = (double)(N > 0 ? N : 0);
      *out_m = nan;
      *out_avg = nan;
      *out_var = nan;
    }
    return;
  }
  const bool need_sel = need_loss && (kind == GLRM_LOSS_L1 || kind == GLRM_LOSS_HUBER || kind == GLRM_LOSS_QUANTILE || kind == GLRM_LOSS_ORDINAL_HINGE);
  const bool staged = need_sel && N <= SC_LDS_MAX;
  const bool periodic = need_loss && kind == GLRM_LOSS_PERIODIC;
  const double dN = (double)N;

  // ---- (a) counts and first moments
  double s = 0.0, ss = 0.0, sc = 0.0, cnz = 0.0, cpos = 0.0;
  for (int64_t t = tid; t < N; t += SC_THREADS) {
    const double x = v[t];
    s += x;
    cnz += x != 0.0 ? 1.0 : 0.0;
    cpos += x > 0.0 ? 1.0 : 0.0;
    if constexpr (TRIG) {
      if (periodic) {
        const double w = 2 * M_PI * x / l.p0;
        ss += sin(w);
        sc += cos(w);
      }
    }
    if (staged) keys[t] = key_of(x);
  }
  const double mean = block_sum(s, shd) / dN;
  double M = nan;
  if (need_loss) {
    switch (kind) {
      case GLRM_LOSS_QUAD: M = mean; break;                // src/losses.jl:148
      case GLRM_LOSS_POISSON: M = log(mean); break;        // :243
      case GLRM_LOSS_LOGISTIC: {                           // :308-311
        const double d = block_sum(cnz, shd);
        M = log(dN + d) - log(dN - d);
        break;
      }
      case GLRM_LOSS_WEIGHTED_HINGE: {                     // :343-352
        const double r = dN / block_sum(cpos, shd) - 1.0;  // N / 0 = +Inf
        M = l.p0 > r ? 1.0 : (l.p0 == r ? 0.0 : -1.0);
        break;
      }
      case GLRM_LOSS_PERIODIC: {                           // :220-224
        if constexpr (TRIG) {
          ss = block_sum(ss, shd);
          sc = block_sum(sc, shd);
          M = (l.p0 / (2 * M_PI)) * atan(ss / sc) + l.p0 / 2;
        }
        break;
      }
      default: break;
    }
  }

  // ---- (b) exact order statistics
  if (need_sel) {
    int64_t k0;
    double gamma;
    if (kind == GLRM_LOSS_QUANTILE) { // Julia's quantile(a, q): h = (n-1) q, linear interpolation between a_(floor h) and its successor
      double h = (dN - 1.0) * l.p0;
      h = h > 0.0 ? h : 0.0; // also a NaN quantile
      h = h < dN - 1.0 ? h : dN - 1.0;
      const double fl = floor(h);
      k0 = (int64_t)fl;
      gamma = h - fl;
    } else {
      k0 = (N - 1) / 2;
      gamma = (N & 1) ? 0.0 : 0.5;
    }
    const bool need_hi = gamma > 0.0 && k0 + 1 < N;
    uint64_t prefix = 0;
    unsigned long long r = (unsigned long long)k0, cnt = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads(); // also orders the staging writes of pass (a) before the first read
      const uint64_t himask = shift == 56 ? 0ull : (~0ull << (shift + 8));
      for (int64_t t0 = 0; t0 < N; t0 += SC_THREADS) { // whole waves enter hist_add together
        const int64_t t = t0 + tid;
        const bool in = t < N;
        const uint64_t key = in ? (staged ? keys[t] : key_of(v[t])) : 0ull;
        hist_add(hist, in && (key & himask) == prefix, (unsigned)((key >> shift) & 255));
      }
      __syncthreads();
      const unsigned long long c = hist[tid];
      unsigned long long incl = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
      }
      if (lane == 63) wtot[wave] = incl;
      __syncthreads();
      for (int w = 0; w < wave; ++w) incl += wtot[w];
      const unsigned long long excl = incl - c;
      if (excl <= r && r < incl) { // exactly one thread: the bins partition [0, matching count)
        sel_prefix = prefix | ((uint64_t)tid << shift);
        sel_rank = r - excl;
        sel_cnt = c;
      }
      __syncthreads();
      prefix = sel_prefix;
      r = sel_rank;
      cnt = sel_cnt;
    }
    const double lo = value_of(prefix);
    double hi = lo;
    if (need_hi && r + 1 >= cnt) { // the next order statistic is the smallest key above
      uint64_t mn = ~0ull;
      for (int64_t t = tid; t < N; t += SC_THREADS) {
        const uint64_t key = staged ? keys[t] : key_of(v[t]);
        if (key > prefix && key < mn) mn = key;
      }
      hi = value_of(block_min(mn, shu));
    }
    if (kind == GLRM_LOSS_QUANTILE) M = need_hi ? lo + gamma * (hi - lo) : lo;
    else M = need_hi ? lo / 2 + hi / 2 : lo; // Julia's middle(a, b)
  }

  // ---- (c) second moment and the loss at the M-estimate
  double q = 0.0, sl = 0.0;
  for (int64_t t = tid; t < N; t += SC_THREADS) {
    const double x = v[t];
    if (need_var) {
      const double d = x - mean;
      q = fma(d, d, q);
    }
    if (need_loss) {
      double L, dL;
      loss_both<false, TRIG>(l, M, x, L, dL);
      sl += L;
    }
  }
  const double var = need_var ? block_sum(q, shd) / (dN - 1.0) : nan; // 0 / 0 = NaN for a single observation
  const double avg = need_loss ? block_sum(sl, shd) / dN : nan;
  if (tid == 0) {
    *out_nobs = dN;
    *out_m = M;
    *out_avg = avg;
    *out_var = var;
  }
}

struct ScaleWork {
  int64_t* colptr = nullptr;
  double* colvals = nullptr;
  glrm_loss* losses = nullptr;
  double* stats = nullptr;
};

} // namespace

extern "C" int glrm_hip_scale_columns(const glrm_problem* p, const glrm_options* o, int32_t mode, double* loss_scale, double* ry_scale,
                                      double* m_est, double* avg_loss, double* variance) {
  if (!p) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: NULL problem");
  if (!loss_scale || !ry_scale) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: loss_scale / ry_scale are NULL");
  if (o && o->storage == GLRM_STORAGE_F32)
    return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_scale_columns is not available with storage = f32 (glrm_options.storage = 1): it reads the fp64 column lists");
  if (mode != GLRM_SCALE_EQUILIBRATE && mode != GLRM_SCALE_PROB)
    return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: mode must be GLRM_SCALE_EQUILIBRATE (0) or GLRM_SCALE_PROB (1), got %d", (int)mode);
  if (p->dense_A)
    return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_scale_columns works on the column lists: hand the problem over without dense_A");
  if (p->n < 0 || p->col_begin < 0 || p->col_end < p->col_begin || p->col_end > p->n)
    return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: column range [%lld, %lld) outside [0, %lld)", (long long)p->col_begin,
                (long long)p->col_end, (long long)p->n);
  const int64_t nl = p->col_end - p->col_begin;
  if (!p->losses || (p->n_losses != 1 && p->n_losses != p->n)) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: n_losses must be 1 or n");
  if (!p->ry || (p->n_ry != 1 && p->n_ry != nl)) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: n_ry must be 1 or col_end - col_begin");
  if (nl > 0x7fffffffLL) return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_scale_columns: more than 2^31 - 1 columns in one call");
  const bool single = p->n_losses == 1;
  const glrm_loss* lh = p->losses + (single ? 0 : p->col_begin);
  bool trig = false;
  for (int64_t j = 0; j < (single ? 1 : nl); ++j) {
    if (lh[j].kind < 0 || lh[j].kind >= GLRM_LOSS_KIND_COUNT) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: unknown loss kind %d", lh[j].kind);
    if (lh[j].kind >= GLRM_LOSS_MULTINOMIAL)
      return fail(GLRM_ERR_UNSUPPORTED, "glrm_hip_scale_columns: column %lld has a multi-dimensional loss (kind %d); their M-estimators do not run "
                  "in the reference either", (long long)(p->col_begin + j), lh[j].kind);
    trig = trig || lh[j].kind == GLRM_LOSS_PERIODIC;
  }
  if (nl == 0) return GLRM_OK;
  if (!p->colptr || !p->colvals) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: colptr / colvals are NULL");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(GLRM_ERR_HIP, "no HIP device is visible (this engine has no CPU fallback)");
  int dev = o ? o->device_id : -1;
  if (dev < 0) HIPCK(hipGetDevice(&dev));
  if (dev >= ndev) return fail(GLRM_ERR_INVALID, "device_id %d out of range (%d devices)", dev, ndev);
  DeviceScope dg(dev);
  if (!dg.ok) return fail(GLRM_ERR_HIP, "cannot select device %d", dev);
  ScaleWork w;
  DevArena scratch;
  int rc;
  hipStream_t st = o ? (hipStream_t)o->stream : nullptr;

  ScaleArgs a{};
  if (p->flags & GLRM_PROBLEM_DEVICE_ARRAYS) {
    a.colptr = p->colptr;
    a.colvals = p->colvals;
  } else {
    if (p->colptr[0] != 0) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: colptr[0] must be 0");
    for (int64_t j = 0; j < nl; ++j)
      if (p->colptr[j + 1] < p->colptr[j]) return fail(GLRM_ERR_INVALID, "glrm_hip_scale_columns: colptr decreases at column %lld", (long long)j);
    const int64_t nnz = p->colptr[nl];
    if ((rc = scratch.alloc(&w.colptr, (size_t)nl + 1)) || (rc = scratch.alloc(&w.colvals, (size_t)std::max<int64_t>(nnz, 0)))) return rc;
    HIPCK(hipMemcpyAsync(w.colptr, p->colptr, (size_t)(nl + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) HIPCK(hipMemcpyAsync(w.colvals, p->colvals, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    a.colptr = w.colptr;
    a.colvals = w.colvals;
  }
  const int64_t nd = single ? 1 : nl;
  if ((rc = scratch.alloc(&w.losses, (size_t)nd)) || (rc = scratch.alloc(&w.stats, (size_t)nl * 4))) return rc;
  HIPCK(hipMemcpyAsync(w.losses, lh, (size_t)nd * sizeof(glrm_loss), hipMemcpyHostToDevice, st));
  a.losses = w.losses;
  a.loss_single = single ? 1 : 0;
  a.mode = mode;
  a.nl = nl;
  a.stats = w.stats;
  if (trig) hipLaunchKernelGGL(scale_kernel<true>, dim3((unsigned)nl), dim3(SC_THREADS), 0, st, a);
  else hipLaunchKernelGGL(scale_kernel<false>, dim3((unsigned)nl), dim3(SC_THREADS), 0, st, a);
  HIPCK(hipGetLastError());
  std::vector<double> stats((size_t)nl * 4);
  HIPCK(hipMemcpyAsync(stats.data(), w.stats, (size_t)nl * 4 * 8, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));

  // the rules (include/glrm_hip_scale.h), with the reference's comparisons: a NaN compares false
  const double *nobs = stats.data(), *M = nobs + nl, *avg = M + nl, *var = avg + nl;
  for (int64_t j = 0; j < nl; ++j) {
    const glrm_loss& lo = lh[single ? 0 : j];
    const double ls = lo.scale, rs = p->ry[p->n_ry == 1 ? 0 : j].scale;
    double nls = ls, nrs = rs;
    if (nobs[j] > 0) {
      if (mode == GLRM_SCALE_EQUILIBRATE) {
        if (avg[j] > 0) nls = ls / avg[j];       // src/modify_glrm.jl:44-47
        if (var[j] > 0) nrs = rs / var[j];       // :48-50
      } else if (lo.kind == GLRM_LOSS_QUAD) {
        if (var[j] > 1e-12) nls = 1 / (2 * var[j]); // :63-69, TOL = 1e-12 (src/regularizers.jl:25)
      } else if (lo.kind == GLRM_LOSS_HUBER) {
        if (avg[j] > 1e-12) nls = 1 / (2 * avg[j]); // :70-76
      } else {
        nls = 1.0;                               // :77-78
      }
    }
    loss_scale[j] = nls;
    ry_scale[j] = nrs;
    if (m_est) m_est[j] = M[j];
    if (avg_loss) avg_loss[j] = avg[j];
    if (variance) variance[j] = var[j];
  }
  return GLRM_OK;
}
