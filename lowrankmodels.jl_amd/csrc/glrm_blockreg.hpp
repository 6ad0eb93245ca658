// glrm_blockreg.hpp -- the regularizers of the general sweeps (csrc/glrm_multi.hpp): evaluate and prox of a k x d block that lives in LDS,
// by one workgroup; wrappers (lastentry1, lastentry_unpenalized, OrdinalReg, MNLOrdinalReg) around a base regularizer.  A header of its
// own so that the test hook (csrc/glrm_testhooks.hip) can run them without the sweep kernels.
//
// The VR = true instantiations also hold the regularizers that carry a vector (include/glrm_hip_regvec.h): the fixed-features wrappers
// GLRM_WRAP_FIXED_FIRST / GLRM_WRAP_FIXED_LAST around a base regularizer and RemQuadReg (kind GLRM_REG_REM_QUAD), on k-vectors (DO == 1).
// `rv` points at the segment's vector and `rl` is its length (nfix, or k for RemQuadReg); the VR = false instantiations never read them.
#pragma once

#include "glrm_device.hpp"
#include "../../include/glrm_hip_regvec.h"

namespace glrm {

// Sum over all threads of the workgroup; every thread returns the same value.  Wave butterfly, then the wave
// partials in wave order.
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  if constexpr (NW == 1) return v;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += red[w];
  return t;
}

// ---------------------------------------------------------------- block regularizers (block in LDS, stride S)

// evaluate(r, block): every thread returns the same value.
template <int NW, bool VR = false>
__device__ inline double block_reg_eval(const double* blk, int S, int k, int DO, glrm_reg rg, double* red, const double* rv = nullptr, int rl = 0) {
  constexpr int NT = NW * 64;
  const int tid = threadIdx.x;
  double bad = 0.0, v = 0.0;
  if constexpr (VR) {
    // fixed_latent_features / fixed_last_latent_features (src/regularizers.jl:208,229): the pinned entries must EQUAL y, entry by entry (a
    // NaN differs from everything); the base then evaluates the other k - nfix entries through the code below, as an unwrapped regularizer
    if (rg.wrap & (GLRM_WRAP_FIXED_FIRST | GLRM_WRAP_FIXED_LAST)) {
      const bool first = (rg.wrap & GLRM_WRAP_FIXED_FIRST) != 0;
      const double* pin = first ? blk : blk + (k - rl);
      for (int c = tid; c < rl; c += NT) bad += pin[c] != rv[c] ? 1.0 : 0.0;
      blk = first ? blk + rl : blk;
      k -= rl;
      rg.wrap = 0;
    }
  }
  const int kr = rg.wrap ? k - 1 : k;                                                        // rows the base regularizer sees
  const int jc = (rg.wrap & (GLRM_WRAP_ORDINAL | GLRM_WRAP_MNL_ORDINAL)) ? 1 : DO;          // evaluate(r.r, a[1:end-1, 1])
  if (rg.wrap == GLRM_WRAP_LASTENTRY1)
    for (int j = tid; j < DO; j += NT) bad += blk[j * S + k - 1] != 1.0 ? 1.0 : 0.0;
  for (int i = tid; i < kr * jc; i += NT) {
    const int j = i / kr, c = i - j * kr;
    const double x = blk[j * S + c];
    switch (rg.kind) {
      case GLRM_REG_QUAD: v = fma(x, x, v); break;
      case GLRM_REG_ONE: v += fabs(x); break;
      case GLRM_REG_NONNEG: v += x < 0 ? 1.0 : 0.0; break;
      case GLRM_REG_UNIT_ONE_SPARSE: v += x == 0 ? 0.0 : (x == 1 ? 1.0 : 4096.0); break;
      default: // the vector kinds (VR instantiations only): jc == 1, validated at create / set_regularizers
        if constexpr (VR) {
          if (rg.kind == GLRM_REG_QUAD_CONSTRAINT) v = fma(x, x, v);
          else if (rg.kind == GLRM_REG_NONNEG_ONE || rg.kind == GLRM_REG_SIMPLEX) { v += x; bad += x < 0 ? 1.0 : 0.0; }
          else if (rg.kind == GLRM_REG_ONE_SPARSE || rg.kind == GLRM_REG_K_SPARSE) v += x != 0 ? 1.0 : 0.0;
          else if (rg.kind == GLRM_REG_REM_QUAD) { const double dm = x - rv[c]; v += dm * dm; } // sum(abs2, a - m), :423 (jc == 1, unwrapped)
        }
        break;
    }
  }
  bad = block_sum<NW>(bad, red);
  v = block_sum<NW>(v, red);
  if (bad > 0) return __builtin_inf();
  switch (rg.kind) {
    case GLRM_REG_QUAD:
    case GLRM_REG_ONE: return rg.scale * v;
    case GLRM_REG_NONNEG: return v > 0 ? __builtin_inf() : 0.0;
    case GLRM_REG_UNIT_ONE_SPARSE: return (v >= 4096.0 || v > 1.0) ? __builtin_inf() : 0.0;
    default:
      if constexpr (VR) {
        switch (rg.kind) {
          case GLRM_REG_QUAD_CONSTRAINT: return sqrt(v) > rg.scale + 1e-12 ? __builtin_inf() : 0.0;
          case GLRM_REG_NONNEG_ONE: return rg.scale * v;
          case GLRM_REG_SIMPLEX: return fabs(v - 1) > 1e-12 ? __builtin_inf() : 0.0;
          case GLRM_REG_ONE_SPARSE: return v > 1.0 ? __builtin_inf() : 0.0;
          case GLRM_REG_K_SPARSE: return v > rg.scale ? __builtin_inf() : 0.0;
          case GLRM_REG_REM_QUAD: return rg.scale * v;
          default: break;
        }
      }
      return 0.0;
  }
}

// prox of a vector regularizer (QuadConstraint, OneSparse, KSparse, Simplex) on u[0 .. n), n <= 64, by ONE thread: the selection and
// the sorted prefix sum of csrc/glrm_device.hpp (select_next) as a plain loop with a 64-bit taken mask.
__device__ inline double serial_select_next(const double* u, int n, bool use_abs, uint64_t& taken) {
  double best = -__builtin_inf();
  int bi = -1;
  for (int c = 0; c < n; ++c) {
    if ((taken >> c) & 1ull) continue;
    double key = use_abs ? fabs(u[c]) : u[c];
    key = key == key ? key : -__builtin_inf(); // NaN orders last, as in select_next (csrc/glrm_device.hpp)
    if (bi < 0 || key > best) { best = key; bi = c; }
  }
  if (bi >= 0) taken |= 1ull << bi;
  return best;
}
__device__ inline void vector_prox_serial(double* u, int n, const glrm_reg rg, double alpha) {
  switch (rg.kind) {
    case GLRM_REG_QUAD_CONSTRAINT: {
      double s = 0.0;
      for (int c = 0; c < n; ++c) s += u[c] * u[c];
      const double f = rg.scale / sqrt(s);
      for (int c = 0; c < n; ++c) u[c] = f * u[c];
      break;
    }
    case GLRM_REG_ONE_SPARSE: {
      int bc = 0;
      for (int c = 1; c < n; ++c) if (u[c] > u[bc]) bc = c;
      for (int c = 0; c < n; ++c) if (c != bc) u[c] = 0.0;
      break;
    }
    case GLRM_REG_K_SPARSE: {
      const int nkeep = rg.scale < (double)n ? (int)rg.scale : n;
      uint64_t taken = 0;
      for (int p = 0; p < nkeep; ++p) (void)serial_select_next(u, n, true, taken);
      for (int c = 0; c < n; ++c) if (!((taken >> c) & 1ull)) u[c] = 0.0;
      break;
    }
    case GLRM_REG_SIMPLEX: {
      uint64_t taken = 0;
      double ysum = 0.0, t = 0.0;
      bool found = false;
      for (int p = 0; p < n && !found; ++p) {
        const double y = serial_select_next(u, n, false, taken);
        if (p >= 1) {
          const double cand = (ysum - 1) / p;
          if (cand >= y) { t = cand; found = true; }
        }
        ysum += y;
      }
      if (!found) t = (ysum - 1) / n;
      for (int c = 0; c < n; ++c) { const double a = u[c] - t; u[c] = a > 0 ? a : 0.0; }
      break;
    }
    default: break;
  }
}

// prox of the base regularizer on rows [0, kr) of DO columns.  whole: UnitOneSparse picks one entry of the whole
// sub-block (column-major first maximum), otherwise one per column.
template <int NW, bool VR = false>
__device__ inline void base_prox_region(double* blk, int S, int kr, int DO, const glrm_reg rg, double alpha, bool whole) {
  constexpr int NT = NW * 64;
  const int tid = threadIdx.x;
  switch (rg.kind) {
    case GLRM_REG_QUAD: {
      const double f = 1 / (1 + 2 * alpha * rg.scale);
      for (int i = tid; i < kr * DO; i += NT) { const int j = i / kr, c = i - j * kr; blk[j * S + c] = f * blk[j * S + c]; }
      break;
    }
    case GLRM_REG_ONE: {
      const double t = rg.scale * alpha;
      for (int i = tid; i < kr * DO; i += NT) {
        const int j = i / kr, c = i - j * kr;
        const double x = blk[j * S + c];
        blk[j * S + c] = fmax(x - t, 0.0) + fmin(x + t, 0.0);
      }
      break;
    }
    case GLRM_REG_NONNEG:
      for (int i = tid; i < kr * DO; i += NT) { const int j = i / kr, c = i - j * kr; const double x = blk[j * S + c]; blk[j * S + c] = x > 0 ? x : 0.0; }
      break;
    case GLRM_REG_UNIT_ONE_SPARSE:
      if (tid == 0 && kr > 0) {
        if (whole) {
          int bj = 0, bc = 0;
          for (int j = 0; j < DO; ++j)
            for (int c = 0; c < kr; ++c)
              if (blk[j * S + c] > blk[bj * S + bc]) { bj = j; bc = c; }
          for (int j = 0; j < DO; ++j)
            for (int c = 0; c < kr; ++c) blk[j * S + c] = 0.0;
          blk[bj * S + bc] = 1.0;
        } else {
          for (int j = 0; j < DO; ++j) {
            int bc = 0;
            for (int c = 1; c < kr; ++c) if (blk[j * S + c] > blk[j * S + bc]) bc = c;
            for (int c = 0; c < kr; ++c) blk[j * S + c] = c == bc ? 1.0 : 0.0;
          }
        }
      }
      break;
    default: // the vector kinds (VR instantiations only; DO == 1, kr <= 64): one thread walks the column in LDS, in component order
      if constexpr (VR) {
        if (rg.kind == GLRM_REG_NONNEG_ONE) {
          for (int i = tid; i < kr * DO; i += NT) { const int j = i / kr, c = i - j * kr; const double x = blk[j * S + c] - alpha; blk[j * S + c] = x > 0 ? x : 0.0; }
        } else if (rg.kind >= GLRM_REG_QUAD_CONSTRAINT && tid == 0 && kr > 0) {
          for (int j = 0; j < DO; ++j) vector_prox_serial(blk + j * S, kr, rg, alpha);
        }
      }
      break;
  }
}

// prox!(r, block, alpha) (src/regularizers.jl:34-114,163-189,295-318,356-405); ends with a workgroup barrier.
template <int NW, bool VR = false>
__device__ inline void block_prox(double* blk, int S, int k, int DO, const glrm_reg rg, double alpha, double* tmp, const double* rv = nullptr, int rl = 0) {
  constexpr int NT = NW * 64;
  const int tid = threadIdx.x;
  if constexpr (VR) { // the regularizers that carry a vector (include/glrm_hip_regvec.h): k-vectors, DO == 1
    if (rg.wrap & (GLRM_WRAP_FIXED_FIRST | GLRM_WRAP_FIXED_LAST)) {
      const int nb = k - rl; // what the base regularizer sees
      glrm_reg base = rg;
      base.wrap = 0;
      if (rg.wrap & GLRM_WRAP_FIXED_FIRST) { // [y ; prox(r, u[nfix+1:end], alpha)], :202
        base_prox_region<NW, true>(blk + rl, S, nb, 1, base, alpha, false);
        for (int c = tid; c < rl; c += NT) blk[c] = rv[c];
      } else { // [prox(r, u[nfix+1:end], alpha) ; y], :223: the base is fed the LAST k - nfix entries and its result lands in the FIRST
               // k - nfix positions; the two ranges overlap when nfix < k - nfix, so the input is read out into tmp first
        for (int c = tid; c < nb; c += NT) tmp[c] = blk[rl + c];
        __syncthreads();
        base_prox_region<NW, true>(tmp, 0, nb, 1, base, alpha, false);
        __syncthreads();
        for (int c = tid; c < nb; c += NT) blk[c] = tmp[c];
        for (int c = tid; c < rl; c += NT) blk[nb + c] = rv[c];
      }
      __syncthreads();
      return;
    }
    if (rg.kind == GLRM_REG_REM_QUAD) { // (u + 2 * alpha * scale * m) / (1 + 2 * alpha * scale), :417-418: a division per entry
      const double t = 2 * alpha * rg.scale;
      for (int c = tid; c < k; c += NT) blk[c] = (blk[c] + t * rv[c]) / (1 + t);
      __syncthreads();
      return;
    }
  }
  const int kr = rg.wrap ? k - 1 : k;
  if (rg.wrap & (GLRM_WRAP_ORDINAL | GLRM_WRAP_MNL_ORDINAL)) {
    if (tid < kr) { // um = mean(u[1:end-1, :], dims=2)
      double acc = 0.0;
      for (int j = 0; j < DO; ++j) acc += blk[j * S + tid];
      tmp[tid] = acc / DO;
    }
    __syncthreads();
    base_prox_region<NW, VR>(tmp, 0, kr, 1, rg, alpha, false);
    __syncthreads();
    for (int i = tid; i < kr * DO; i += NT) { const int j = i / kr, c = i - j * kr; blk[j * S + c] = tmp[c]; }
    if ((rg.wrap & GLRM_WRAP_MNL_ORDINAL) && tid == 0) { // decreasing, negative last row (not exactly the prox, :400-404)
      const double TOL = 1e-3;
      double* last = blk + (k - 1);
      last[0] = last[0] < -TOL ? last[0] : -TOL;
      for (int j = 1; j < DO; ++j) last[j * S] = last[j * S] < last[(j - 1) * S] - TOL ? last[j * S] : last[(j - 1) * S] - TOL;
    }
    __syncthreads();
    return;
  }
  base_prox_region<NW, VR>(blk, S, kr, DO, rg, alpha, !(rg.wrap == GLRM_WRAP_LASTENTRY1 || DO == 1));
  if (rg.wrap == GLRM_WRAP_LASTENTRY1)
    for (int j = tid; j < DO; j += NT) blk[j * S + k - 1] = 1.0;
  __syncthreads();
}

} // namespace glrm
