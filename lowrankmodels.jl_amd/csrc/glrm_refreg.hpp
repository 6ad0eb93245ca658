// glrm_refreg.hpp -- the regularizers of the reference-order validation sweeps (csrc/glrm_reforder.hip): one lane holds the whole
// k-vector in registers and walks it in component order, like the reference and the CPU oracle.  Shared with the test hook
// (csrc/glrm_testhooks.hip).
#pragma once

#include "glrm_device.hpp"

namespace glrm {

// glrm_cpu_reg_evaluate, oracle/glrm_oracle.c (src/regularizers.jl:58,74,88,95,103-112,129-136,239-253,261-276,300-316,338-346): component order, multiply then add
template <int KP>
__device__ __forceinline__ double ref_reg_eval_vector(const RegDesc& r, const double (&x)[KP], int k) {
  switch (r.kind) {
    case GLRM_REG_QUAD_CONSTRAINT: { // :74, norm = sqrt of the sum of squares in component order
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < k) s += x[c] * x[c];
      return sqrt(s) > r.scale + 1e-12 ? __builtin_inf() : 0.0;
    }
    case GLRM_REG_NONNEG_ONE:
    case GLRM_REG_SIMPLEX: { // :129-136 / :338-346
      double s = 0.0;
      bool neg = false;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < k) {
          s += x[c];
          neg = neg || x[c] < 0;
        }
      if (neg) return __builtin_inf();
      if (r.kind == GLRM_REG_NONNEG_ONE) return r.scale * s;
      return fabs(s - 1) > 1e-12 ? __builtin_inf() : 0.0;
    }
    case GLRM_REG_ONE_SPARSE:
    case GLRM_REG_K_SPARSE: { // :239-253 / :261-276
      int nz = 0;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < k && x[c] != 0) ++nz;
      return (double)nz > (r.kind == GLRM_REG_ONE_SPARSE ? 1.0 : r.scale) ? __builtin_inf() : 0.0;
    }
    default:
      return 0.0;
  }
}

// VR: the vector kinds (>= GLRM_REG_QUAD_CONSTRAINT) are compiled in (csrc/glrm_device.hpp: the same split as reg_prox / reg_eval)
template <int KP, bool VR = false>
__device__ __forceinline__ double ref_reg_eval(const RegDesc& r, const double (&x)[KP], int k) {
  switch (r.kind) {
    case GLRM_REG_QUAD: {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < k) s += x[c] * x[c];
      return r.scale * s;
    }
    case GLRM_REG_ONE: {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < k) s += fabs(x[c]);
      return r.scale * s;
    }
    case GLRM_REG_NONNEG: {
      bool neg = false;
#pragma unroll
      for (int c = 0; c < KP; ++c) neg = neg || (c < k && x[c] < 0);
      return neg ? __builtin_inf() : 0.0;
    }
    case GLRM_REG_UNIT_ONE_SPARSE: {
      int ones = 0;
      bool other = false;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < k && x[c] != 0) {
          if (x[c] == 1) ++ones; else other = true;
        }
      return (other || ones > 1) ? __builtin_inf() : 0.0;
    }
    default:
      if constexpr (VR) return ref_reg_eval_vector<KP>(r, x, k);
      return 0.0;
  }
}

// One step of an ordered selection on a register vector: the not yet taken component c < k with the largest key (|u_c| or u_c), lowest
// index among equal keys; marks it in the mask and returns the key.  Register indices stay compile-time constants (the sweeps exist up to KP = 64).
template <int KP, bool ABS>
__device__ __forceinline__ double ref_select_next(const double (&u)[KP], int k, uint64_t& taken) {
  static_assert(KP <= 64, "one 64-bit mask");
  double best = -__builtin_inf();
  int bi = -1;
#pragma unroll
  for (int c = 0; c < KP; ++c) {
    const bool free_c = !((taken >> c) & 1ull);
    double key = ABS ? fabs(u[c]) : u[c];
    key = key == key ? key : -__builtin_inf(); // NaN orders last, as in select_next (csrc/glrm_device.hpp)
    if (c < k && free_c && (bi < 0 || key > best)) { best = key; bi = c; }
  }
  if (bi >= 0) taken |= 1ull << bi;
  return best;
}

template <int KP>
__device__ __forceinline__ void ref_reg_prox_vector(const RegDesc& r, double (&u)[KP], int k, double alpha) {
  switch (r.kind) {
    case GLRM_REG_QUAD_CONSTRAINT: {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < k) s += u[c] * u[c];
      const double f = r.scale / sqrt(s);
#pragma unroll
      for (int c = 0; c < KP; ++c) u[c] = f * u[c];
      break;
    }
    case GLRM_REG_NONNEG_ONE: {
#pragma unroll
      for (int c = 0; c < KP; ++c) {
        const double a = u[c] - alpha;
        u[c] = a > 0 ? a : 0.0;
      }
      break;
    }
    case GLRM_REG_K_SPARSE: {
      const int nkeep = r.scale < (double)k ? (int)r.scale : k;
      uint64_t taken = 0;
      for (int p = 0; p < nkeep; ++p) (void)ref_select_next<KP, true>(u, k, taken);
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (!((taken >> c) & 1ull)) u[c] = 0.0;
      break;
    }
    case GLRM_REG_SIMPLEX: {
      uint64_t taken = 0;
      double ysum = 0.0, t = 0.0;
      bool found = false;
      for (int p = 0; p < k && !found; ++p) {
        const double y = ref_select_next<KP, false>(u, k, taken);
        if (p >= 1) {
          const double cand = (ysum - 1) / p;
          if (cand >= y) { t = cand; found = true; }
        }
        ysum += y;
      }
      if (!found) t = (ysum - 1) / k;
#pragma unroll
      for (int c = 0; c < KP; ++c) {
        const double a = u[c] - t;
        u[c] = a > 0 ? a : 0.0;
      }
      break;
    }
    case GLRM_REG_ONE_SPARSE: { // u[argmax u] e_{argmax u}, first maximal index
      uint64_t taken = 0;
      (void)ref_select_next<KP, false>(u, k, taken);
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (!((taken >> c) & 1ull)) u[c] = 0.0;
      break;
    }
    default:
      break;
  }
}

// glrm_cpu_reg_prox (src/regularizers.jl:34,56,72,83-86,93,103,122,237,277-283,297,325-337)
template <int KP, bool VR = false>
__device__ __forceinline__ void ref_reg_prox(const RegDesc& r, double (&u)[KP], int k, double alpha) {
  switch (r.kind) {
    case GLRM_REG_QUAD: {
      const double f = 1 / (1 + 2 * alpha * r.scale);
#pragma unroll
      for (int c = 0; c < KP; ++c) u[c] = f * u[c];
      break;
    }
    case GLRM_REG_ONE: {
      const double t = r.scale * alpha;
#pragma unroll
      for (int c = 0; c < KP; ++c) u[c] = fmax(u[c] - t, 0.0) + fmin(u[c] + t, 0.0);
      break;
    }
    case GLRM_REG_NONNEG: {
#pragma unroll
      for (int c = 0; c < KP; ++c) u[c] = u[c] > 0 ? u[c] : 0.0;
      break;
    }
    case GLRM_REG_UNIT_ONE_SPARSE: { // e_{argmax u}, first maximal index
      int idx = 0;
      double best = u[0];
#pragma unroll
      for (int c = 1; c < KP; ++c)
        if (c < k && u[c] > best) { best = u[c]; idx = c; }
#pragma unroll
      for (int c = 0; c < KP; ++c) u[c] = c == idx ? 1.0 : 0.0;
      break;
    }
    default:
      if constexpr (VR) ref_reg_prox_vector<KP>(r, u, k, alpha);
      break;
  }
#pragma unroll
  for (int c = 0; c < KP; ++c)
    if (c >= k) u[c] = 0.0; // the padding stays exactly zero
}

} // namespace glrm
