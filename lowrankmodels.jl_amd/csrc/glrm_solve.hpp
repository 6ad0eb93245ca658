// glrm_solve.hpp -- glrm_hip_solve_x (include/glrm_hip_transform.h): T X half-steps of a row with Y held fixed, in ONE launch of the
// register variant of the cached row sweep (glrm_cached.hpp).  Y does not change between a row's steps, so what regcached_sweep_kernel
// fetches for one step -- the row's (index, value) list, its opposing vectors, its descriptors, its point and its stepsize -- is
// fetched once and serves all T: one gather of the row's vectors instead of T x (1 + trials), one launch instead of T, and the row's
// chain of dependent round trips (row pointer -> list -> vectors) once per T steps.  Templates over the storage type like the sweep:
// glrm_solve.hip instantiates ST = double, glrm_solve_f32.hip ST = float.
#pragma once

#include "glrm_cached.hpp"

namespace glrm {

// One row per workgroup, two waves per row (the order of regcached_sweep_kernel<.., WAVES = 2>: wave w holds the observations
// (t * 2 + w) * (64 / G) + group).  A trip of the loop is that kernel between its gathers and its stores: the gradient pass at the current
// point, Jold recomputed from it (never carried over from the accepted trial: that is what T launches do, and it keeps the bits), the
// line search.  A row that gave up carries on from min_stepsize * 1.1 with the next trip, as the reference's inner loop does
// (proxgrad.jl:117-156).  x, the stepsize and the counters are stored once, behind the last trip.  `inner` >= 1 is uniform.
// There is no fixed-stepsize form.  The step is written out here beside regcached_sweep_kernel's, not shared with it through a device
// function: with the step factored out the sweep kernels' registers moved (profiles/transform_resusage_diff.txt), so that kernel stays
// exactly as it was and the two statements are held together by the bit-for-bit tests (tests/test_gpu_transform.py).
template <int G, int R, int LOSS, int MAXT, bool VR = false, class ST = double>
__global__ void __launch_bounds__(128) regcached_solve_kernel(const CachedArgs a, const int inner) {
  using P = typename Pair<ST>::type;
  constexpr int WAVES = 2, KP = G * R, NG = (64 / G) * WAVES;
  __shared__ __attribute__((aligned(16))) double red[WAVES * (KP + 2)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t seg = cached_segment(a, blockIdx.x);
  if (seg < 0) return;
  const int j = lane % G, gi = wave * (64 / G) + lane / G;
  const int64_t beg = a.ptr[seg];
  const int len = (int)(a.ptr[seg + 1] - beg);
  const int64_t gseg = a.own_offset + seg;
  P* ownp = reinterpret_cast<P*>(reinterpret_cast<ST*>(a.own) + gseg * KP);
  const ST* vals = reinterpret_cast<const ST*>(a.vals);
  int cc[MAXT];
  ST av[MAXT];
  P y[MAXT][R / 2];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) { // the group's entries (clamped: lanes past the end re-read the last entry and are masked)
    int tt = t * NG + gi;
    tt = tt < len ? tt : (len > 0 ? len - 1 : 0);
    cc[t] = len > 0 ? a.idx[beg + tt] : 0;
    av[t] = len > 0 ? vals[beg + tt] : (ST)0.0;
  }
  Vec<G, R> x, g;
#pragma unroll
  for (int i = 0; i < R / 2; ++i) x.v[i] = widen(ownp[i * G + j]);
  const P* __restrict__ other2 = reinterpret_cast<const P*>(a.other);
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if (t * NG + wave * (64 / G) < len) { // wave-uniform
      const P* yp = other2 + (int64_t)cc[t] * (KP / 2) + j;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) y[t][i] = yp[i * G];
    } else {
#pragma unroll
      for (int i = 0; i < R / 2; ++i) y[t][i] = P{0, 0};
    }
  }
  const RegDesc rd = load_reg(a.regs, a.reg_single ? 0 : seg);
  LossDesc segloss = LossDesc{0, 1.0, 0.0, 0.0};
  if constexpr (loss_mode(LOSS) != LOSS_PER_OBS) segloss = load_loss(a.losses, 0);
  double alpha = a.alpha[seg];
  const double l = (double)len + 1.0;
  int ntrials = 0, naccepted = 0;
  for (int it = 0; it < inner; ++it) {
    double Jold = reg_pass<G, R, LOSS, MAXT, true, WAVES, ST>(a, y, av, cc, x, g, len, gi, segloss);
    Jold = row_combine<G, R, WAVES, true>(Jold, g, red, wave, lane);
    Jold += reg_eval<G, R, VR>(rd, x, j, a.k);
    while (alpha > a.min_stepsize) {
      const double s = alpha / l;
      Vec<G, R> xn, dummy;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        xn.v[i].x = fma(-s, g.v[i].x, x.v[i].x);
        xn.v[i].y = fma(-s, g.v[i].y, x.v[i].y);
      }
      reg_prox<G, R, VR>(rd, xn, s, j, a.k);
      round_trial<ST>(xn);
      double Jn = reg_pass<G, R, LOSS, MAXT, false, WAVES, ST>(a, y, av, cc, xn, dummy, len, gi, segloss);
      Jn = row_combine<G, R, WAVES, false>(Jn, dummy, red, wave, lane);
      Jn += reg_eval<G, R, VR>(rd, xn, j, a.k);
      ++ntrials;
      if (Jn < Jold) {
        x = xn;
        alpha *= 1.05;
        ++naccepted;
        break;
      }
      alpha *= .7;
      if (alpha < a.min_stepsize) {
        alpha = a.min_stepsize * 1.1;
        break;
      }
    }
  }
  if (naccepted > 0 && gi == 0) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) store_pair<ST>(&ownp[i * G + j], x.v[i]);
  }
  if (lane == 0 && wave == 0) {
    a.alpha[seg] = alpha;
    if (a.trials) {
      a.trials[seg] += ntrials;
      a.accepts[seg] += naccepted;
    }
  }
}

// a.cap = trips of one wave the longest row of the launch needs (64 / G observations each); MAXT as launch_reg_inst picks it for the
// two-wave sweep (MAXT only adds empty trips: the order of a row's sums does not depend on it)
template <int G, int R, int LOSS, bool VR, class ST = double>
int launch_solve_inst(const CachedArgs& a, int inner, hipStream_t st) {
  if ((a.cap + 1) / 2 <= 4) {
    hipLaunchKernelGGL((regcached_solve_kernel<G, R, LOSS, 4, VR, ST>), dim3((unsigned)a.nseg), dim3(128), 0, st, a, inner);
  } else {
    hipLaunchKernelGGL((regcached_solve_kernel<G, R, LOSS, 7, VR, ST>), dim3((unsigned)a.nseg), dim3(128), 0, st, a, inner);
  }
  return GLRM_OK;
}

} // namespace glrm

// the float instantiations (glrm_solve_f32.hip): layouts (4, 8) and (8, 8), the five loss variants, VR = false
int glrm_launch_solve_f32(const glrm::CachedArgs& a, int G, int loss, int inner, hipStream_t st);
