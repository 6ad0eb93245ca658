// glrm_stream.hpp -- the kernels of glrm_hip_stream_rows (include/glrm_hip_stream.h, which states the arithmetic, its order and the plan;
// this file only says how the work is dealt out).  stream_kernel<KP> runs one row body, stream_row, from two launch shapes:
//   wide   one workgroup per row of a level (rows_per_block = 1);
//   chain  ONE workgroup that walks a run of one-row levels in ascending order (grid 1, rows_per_block = the piece's rows).
// Both shapes run the same body on the same workgroup size, so the two cannot differ in a bit.  A row:
//   decay     als_threads(KP) observations at a time: lane t reads epoch[j_t], forms p = c^d and records the new epoch; then every
//             (t, component) pair divides.  In a dup row the later of two lanes that name one column stands back (a compare over the
//             chunk in LDS), so a column is divided once.  The write-back is drained (vmcnt) and a workgroup barrier passed before
//             als_gram gathers the same columns: the waves of a workgroup share one L1, which their own stores keep current.
//   solve     als_gram<KP> and als_factor_solve of glrm_als.hpp -- the ALS kernel's own Gram stage and wave-0 solve -- with the diagonal
//             shift 2 * gamma; x goes to LDS, and to X when the row is solved.
//   queries   one lane per query column: the pending decay in registers, then the dot product.
//   residual  one lane per observation for r_t (a ascending over the column, which the Gram stage has just pulled through the caches);
//             lane 0 adds r_t * r_t in order; every (t, component) pair updates Y.  A dup row first parks every r_t in the call's
//             scratch (an update must not reach a residual that still has to read the column), then wave 0 -- lane a = component a --
//             applies the updates t ascending: one lane per address, program order.
// The chain is latency-bound on one CU.  The decay and the update keep STREAM_U independent loads per lane in flight instead of one
// load-modify-store at a time; measured on an MI355X this changed nothing (about 110 us of a chain row do not
// depend on its length, and where they go has not been profiled).
// stream_flush_kernel: one lane per column, the outstanding divisions after the last row.
#pragma once

#include "../../include/glrm_hip_stream.h"
#include "glrm_als.hpp"

namespace glrm {

struct StreamArgs {
  AlsArgs g;                     // the row view, Y as opp, X as own, the losses (scale exactly 1.0), rx as regs; order / status unused
  const int32_t* order;          // position in launch order -> row - first
  const int64_t* dupoff;         // row - first -> offset of the row's residuals in `scratch`, -1: no column is named twice
  double* scratch;
  int64_t* epoch;                // divisions every column has received
  const int64_t* qptr; const int32_t* qcol; double* qout; // queries (device), or nullptr
  double* objective;             // m - first
  int8_t* status;                // m - first
  int64_t first, interval, base; // base = floor(first / interval)
  double stepsize, c;
};

constexpr int STREAM_U = 8; // (t, component) pairs a lane has in flight in the decay and in the update
// A row's chain of dependent steps decides the time of a chain launch, and wide levels are about a hundred rows, fewer than the CUs: the
// register allocation is held to 2 waves per SIMD, not to als_min_waves -- at 4 the KP = 32 body spills 176 bytes per lane to scratch.
constexpr int stream_min_waves(int) { return 2; }

// p = c^d by d - 1 multiplications, in the header's order; an infinite p stays infinite (c >= 1), so the loop may stop there
__device__ __forceinline__ double stream_pow(const double c, const int64_t d) {
  double p = c;
  for (int64_t e = 1; e < d && p <= 0x1.fffffffffffffp+1023; ++e) p = p * c;
  return p;
}

template <int KP>
__device__ __forceinline__ void stream_row(const StreamArgs& s, const int64_t r, double* const lds, double* const wl, double* const xs, double* const rl,
                                           double* const pl, int32_t* const jl, int* const stl) {
  constexpr int T = als_threads(KP);
  const AlsArgs& a = s.g;
  const int tid = threadIdx.x, k = a.k;
  const int64_t i = s.first + r;
  const int64_t lo = a.ptr[i], len = a.ptr[i + 1] - lo;
  const glrm_reg reg = a.regs[a.reg_single ? 0 : i];
  const double gamma = reg.kind == GLRM_REG_QUAD ? reg.scale : 0.0;
  const int64_t D = i / s.interval - s.base;
  const int64_t dupoff = s.dupoff[r];
  double* const Y = const_cast<double*>(a.opp);

  // ---- pending decay of the row's columns
  if (s.c != 1.0 && D > 0) {
    for (int64_t base = 0; base < len; base += T) {
      const int cnt = len - base < T ? (int)(len - base) : T;
      double p = 0.0;
      int32_t j = -1;
      if (tid < cnt) {
        j = a.idx[lo + base + tid];
        const int64_t d = D - s.epoch[j];
        if (d > 0) p = stream_pow(s.c, d);
      }
      if (dupoff >= 0) {                                     // workgroup-uniform
        jl[tid] = j;
        __syncthreads();                                     // every lane has read its epoch
        for (int t = 0; t < tid && t < cnt; ++t)
          if (jl[t] == j) p = 0.0;
      }
      if (p != 0.0) s.epoch[j] = D;
      pl[tid] = p;
      jl[tid] = j;
      __syncthreads();
      for (int q0 = tid; q0 < cnt * KP; q0 += T * STREAM_U) { // the pairs name distinct addresses: a batch's loads go out together
        double* yp[STREAM_U];
        double yv[STREAM_U], pt[STREAM_U];
#pragma unroll
        for (int u = 0; u < STREAM_U; ++u) {
          const int q = q0 + u * T, t = q / KP, comp = q % KP;
          pt[u] = q < cnt * KP && comp < k ? pl[t] : 0.0;
          yp[u] = nullptr;
          if (pt[u] != 0.0) {
            yp[u] = Y + (int64_t)jl[t] * KP + comp;
            yv[u] = *yp[u];
          }
        }
#pragma unroll
        for (int u = 0; u < STREAM_U; ++u)
          if (yp[u]) *yp[u] = yv[u] / pt[u];
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }

  // ---- the solve
  const bool shortrow = gamma == 0.0 && len < k;             // the short rule (workgroup-uniform)
  if (!shortrow) als_gram<KP>(a, lo, len, 0.0, lds, wl);
  if (tid < 64) {
    double x = 0.0;
    int st = GLRM_ALS_KEPT_SHORT;
    if (!shortrow) st = als_factor_solve(lds, lds + KP * (KP + 1) / 2, k, gamma + gamma, x);
    if (tid < k) {
      if (st == GLRM_ALS_SOLVED) a.own[i * KP + tid] = x;
      else x = a.own[i * KP + tid];                          // a kept row is used as it stands
      xs[tid] = x;
    }
    if (tid == 0) *stl = st;
  }
  __syncthreads();
  const int st = *stl;

  // ---- queries: Y as the row found it, the pending decay in registers
  if (s.qptr) {
    const int64_t qlo = s.qptr[i], nq = s.qptr[i + 1] - qlo;
    for (int64_t q = tid; q < nq; q += T) {
      const int64_t j = s.qcol[qlo + q];
      const int64_t d = D - s.epoch[j];
      const bool decay = s.c != 1.0 && d > 0;
      const double p = decay ? stream_pow(s.c, d) : 1.0;
      double acc = 0.0;
      for (int comp = 0; comp < k; ++comp) {
        double y = Y[j * KP + comp];
        if (decay) y = y / p;
        const double prod = y * xs[comp];
        acc = acc + prod;
      }
      s.qout[qlo + q] = acc;
    }
  }

  // ---- residual, objective, update
  if (st == GLRM_ALS_SOLVED) {
    double obj = 0.0;                                        // lane 0's accumulator
    for (int64_t base = 0; base < len; base += T) {
      const int cnt = len - base < T ? (int)(len - base) : T;
      if (tid < cnt) {
        const int32_t j = a.idx[lo + base + tid];
        const double* const y = Y + (int64_t)j * KP;
        double acc = 0.0;
        for (int comp = 0; comp < k; ++comp) {
          const double prod = y[comp] * xs[comp];
          acc = acc + prod;
        }
        const double res = acc - a.vals[lo + base + tid];
        rl[tid] = res;
        jl[tid] = j;
        if (dupoff >= 0) s.scratch[dupoff + base + tid] = res;
      }
      __syncthreads();
      if (tid == 0)
        for (int t = 0; t < cnt; ++t) {
          const double sq = rl[t] * rl[t];
          obj = obj + sq;
        }
      if (dupoff < 0)
        for (int q0 = tid; q0 < cnt * KP; q0 += T * STREAM_U) { // no column twice: distinct addresses, a batch's loads go out together
          double* yp[STREAM_U];
          double yv[STREAM_U], prod[STREAM_U];
#pragma unroll
          for (int u = 0; u < STREAM_U; ++u) {
            const int q = q0 + u * T, t = q / KP, comp = q % KP;
            yp[u] = nullptr;
            if (q < cnt * KP && comp < k) {
              yp[u] = Y + (int64_t)jl[t] * KP + comp;
              yv[u] = *yp[u];
              const double step = s.stepsize * rl[t];
              prod[u] = step * xs[comp];
            }
          }
#pragma unroll
          for (int u = 0; u < STREAM_U; ++u)
            if (yp[u]) *yp[u] = yv[u] - prod[u];
        }
      __syncthreads();
    }
    if (dupoff >= 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                                       // every residual is parked
      if (tid < k)
        for (int64_t t = 0; t < len; ++t) {
          double* const y = Y + (int64_t)a.idx[lo + t] * KP + tid;
          const double step = s.stepsize * s.scratch[dupoff + t];
          const double prod = step * xs[tid];
          *y = *y - prod;
        }
    }
    if (tid == 0) s.objective[r] = obj;
  } else if (tid == 0) {
    s.objective[r] = __builtin_nan("");
  }
  if (tid == 0) s.status[r] = (int8_t)st;
  // the next row of a chain gathers what this one wrote, and reuses the LDS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

template <int KP>
__global__ void __launch_bounds__(als_threads(KP), stream_min_waves(KP)) stream_kernel(const StreamArgs s, const int64_t pos, const int64_t end, const int64_t rows_per_block) {
  __shared__ __attribute__((aligned(16))) double lds[als_lds_doubles(KP)];
  __shared__ double wl[ALS_CHUNK];
  __shared__ double xs[64];
  __shared__ double rl[als_threads(KP)], pl[als_threads(KP)];
  __shared__ int32_t jl[als_threads(KP)];
  __shared__ int stl;
  const int64_t b = pos + (int64_t)blockIdx.x * rows_per_block;
  const int64_t e = b + rows_per_block < end ? b + rows_per_block : end;
  for (int64_t q = b; q < e; ++q) stream_row<KP>(s, s.order[q], lds, wl, xs, rl, pl, jl, &stl);
}

// after the last row: the divisions every column still misses, up to `total`
__global__ void __launch_bounds__(256) stream_flush_kernel(double* const Y, int64_t* const epoch, const int64_t n, const int kp, const int k, const double c, const int64_t total) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t d = total - epoch[j];
  if (d <= 0) return;
  const double p = stream_pow(c, d);
  for (int comp = 0; comp < k; ++comp) Y[j * kp + comp] = Y[j * kp + comp] / p;
  epoch[j] = total;
}

} // namespace glrm
