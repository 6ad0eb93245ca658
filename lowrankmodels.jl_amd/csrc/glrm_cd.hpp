// glrm_cd.hpp -- the kernel of glrm_hip_cd_solve (include/glrm_hip_cd.h, which states the arithmetic and its order; this file only says how
// the work is dealt out).  One workgroup per segment, longest first.  The Gram stage is als_gram (glrm_als.hpp), shared with
// als_solve_kernel: it leaves the packed lower triangle of G and the right-hand side b in LDS in front of wave 0.  The tail is the new work:
//   lanes       lane i of wave 0 holds x_i, g_i, G_ii and M_ii in registers; no value is reduced across lanes.
//   coordinate  x_a, g_a, G_aa and M_aa reach every lane by a shuffle from lane a (a is wave-uniform).  Every lane computes rho, new and d
//               redundantly, so the skip branch and the early exit are wave-uniform and cost no vote.
//   update      lane i reads G_ia from the packed triangle, tri(max(i, a), min(i, a)): lanes i <= a read consecutive doubles of row a,
//               lanes i > a read down column a at the triangle's growing stride.
//   result      x_i goes out from lane i; the status bits and sweeps_run from lane 0, with vector stores.
#pragma once

#include "../../include/glrm_hip_cd.h"
#include "glrm_als.hpp"

namespace glrm {

struct CdArgs {
  AlsArgs g;           // the Gram stage's view of the segment lists; g.status: the status bits
  int32_t* sweeps_run; // per local segment
  int sweeps;
};

template <int KP>
__global__ void __launch_bounds__(als_threads(KP), als_min_waves(KP)) cd_solve_kernel(const CdArgs c) {
  __shared__ __attribute__((aligned(16))) double lds[als_lds_doubles(KP)];
  __shared__ double wl[ALS_CHUNK];

  const AlsArgs& a = c.g;
  const int tid = threadIdx.x, k = a.k;
  const int64_t seg = a.order[blockIdx.x];
  const int64_t lo = a.ptr[seg], len = a.ptr[seg + 1] - lo;
  const glrm_reg reg = a.regs[a.reg_single ? 0 : seg];
  const double wseg = a.side == GLRM_COLS ? a.losses[a.loss_single ? 0 : seg].scale : 0.0;
  als_gram<KP>(a, lo, len, wseg, lds, wl);
  if (tid >= 64) return;

  // wave 0: lane i = coordinate i
  const double* const tri = lds;
  const double* const rhs = lds + KP * (KP + 1) / 2;
  const int i = tid, kind = reg.kind;
  const bool row = i < k;
  const double gamma = reg.scale;
  const double gii = row ? tri[als_tri(i, i)] : 0.0;
  const double mii = kind == GLRM_REG_QUAD ? gii + gamma : gii;
  double maxd = __shfl(mii, 0, 64);
  for (int b = 1; b < k; ++b) {
    const double d = __shfl(mii, b, 64);
    if (d > maxd) maxd = d;
  }
  const double tol = ((double)k * 0x1p-52) * maxd;
  const bool one_to_zero = kind == GLRM_REG_ONE && gamma > 0.0; // what a skipped coordinate of the lasso does
  const double half = 0.5 * gamma;

  double x = row ? a.own[seg * KP + i] : 0.0;
  if (kind == GLRM_REG_NONNEG) x = x > 0.0 ? x : 0.0;
  double g = row ? rhs[i] : 0.0;
  for (int b = 0; b < k; ++b) {                                 // the residual b - G x, one product at a time
    const double xb = __shfl(x, b, 64);
    if (row) {
      const double prod = tri[i >= b ? als_tri(i, b) : als_tri(b, i)] * xb;
      g = g - prod;
    }
  }

  int status = 0, run = 0;
  while (run < c.sweeps) {
    bool changed = false;
    for (int b = 0; b < k; ++b) {
      const double xb = __shfl(x, b, 64), gb = __shfl(g, b, 64), gbb = __shfl(gii, b, 64), mbb = __shfl(mii, b, 64);
      double nw;
      if (!(mbb > tol)) {                                       // the denominator rule (wave-uniform)
        status |= GLRM_CD_SKIPPED;
        if (!one_to_zero) continue;
        nw = 0.0;
      } else {
        const double prod = gbb * xb;
        const double rho = gb + prod;
        if (kind == GLRM_REG_ONE) {
          nw = rho > half ? (rho - half) / mbb : rho < -half ? (rho + half) / mbb : 0.0;
        } else {
          nw = rho / mbb;
          if (kind == GLRM_REG_NONNEG) nw = nw > 0.0 ? nw : 0.0;
        }
      }
      const double d = nw - xb;
      if (!(d == 0.0)) changed = true;
      if (row) {
        const double prod = tri[i >= b ? als_tri(i, b) : als_tri(b, i)] * d;
        g = g - prod;
      }
      if (i == b) x = nw;
    }
    ++run;
    if (!changed) {
      status |= GLRM_CD_CONVERGED;
      break;
    }
  }
  if (row) a.own[seg * KP + i] = x;
  if (i == 0) {
    a.status[seg] = (int8_t)status;
    c.sweeps_run[seg] = run;
  }
}

} // namespace glrm
