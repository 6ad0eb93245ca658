// glrm_sweep.hpp -- the gather sweeps: one HIP kernel per factor half-step over a CSR / CSC view (sweep_kernel), the penalty kernel and
// the ladder from run-time layout / wave count / loss variant to their template arguments.  Templates over the STORAGE type ST of the
// observation values and the factors (include/glrm_hip_storage.h): glrm_hip.hip instantiates ST = double, glrm_storage.hip ST = float
// (VR = false only).  ST changes loads, stores and one rounding after the prox step; every sum is fp64 in the same order for both.
#pragma once

#include <hip/hip_runtime.h>

#include "glrm_device.hpp"
#include "glrm_engine.hpp"
#include "glrm_launch.hpp"

namespace glrm {

struct SweepArgs {
  int64_t nseg;          // local segments
  const int64_t* ptr;    // nseg+1 offsets into idx/vals
  const int32_t* idx;    // index into the opposing factor (global id)
  const void* vals;      // A values (ST)
  void* own;             // factor being updated (global array of ST, leading dimension KP)
  int64_t own_offset;    // global id of local segment 0
  const void* other;     // opposing factor (global array of ST, leading dimension KP)
  double* alpha;         // per local segment step size
  double* obj;           // per GLOBAL segment objective (nullable)
  const glrm_loss* losses;
  int loss_by_segment;   // LOSS==1: 1 -> losses[own_offset+seg], 0 -> losses[0]
  const glrm_reg* regs;
  int reg_single;        // 1 -> regs[0], 0 -> regs[seg]
  int k;
  int eval_only;         // 1: obj[seg] = sum of losses (no regularizer), nothing else is written
  double fixed_alpha;    // > 0: one prox-gradient step with this global step size, no line search (SparseProxGradParams)
  double min_stepsize;
  int32_t* trials;       // per local segment accumulators (nullable)
  int32_t* accepts;
  const int32_t* seglist; // nullable: the launch covers the local segments seglist[0..nseg) instead of 0..nseg -- the segments of ONE
                          // wave class when the shard holds several (glrm_class_plan::list) -- restricted to [seg_lo, seg_hi)
  int64_t seg_lo, seg_hi; // (glrm_hip_step_x_range on such a shard; otherwise [0, local segments))
  int vecreg;            // 1: a descriptor of this side names a vector regularizer -- the VR = true kernels (csrc/glrm_device.hpp)
  int storage;           // GLRM_STORAGE_*: the type ST behind vals / own / other, i.e. which instantiation the launch takes
};

// (Pair, widen, stored, store_pair -- two components as the storage holds them -- are glrm_device.hpp's: the pass kernels use them too.)

// One pass over the segment for one wave: J = sum of losses at u = <xv, other[idx]>, and (GRAD)
// g = sum of dL * other[idx].  Returns wave-level totals replicated in every lane.
// U observations per group are in flight per loop trip (U x R/2 16-byte loads per lane); a group
// always handles the observations t == gg (mod TG) in ascending order, so the result bits do not
// depend on U.
template <int G, int R, int WAVES, int LOSS, int U, bool GRAD, class ST = double>
__device__ __forceinline__ double sweep_pass(const SweepArgs& a, const Vec<G, R>& xv, Vec<G, R>& g, int64_t beg,
                                             int64_t len, int gg, int j, const LossDesc& segloss) {
  constexpr int KP = G * R, NG = 64 / G, TG = NG * WAVES;
  constexpr bool SCATTER = G == 4 && U == 4 && LOSS != LOSS_QUAD_UNIFORM;
  constexpr int LM = loss_mode(LOSS);
  constexpr bool TRIG = loss_trig(LOSS);
  double J = 0.0;
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) g.v[i] = make_double2(0.0, 0.0);
  }
  using P = typename Pair<ST>::type;
  const P* __restrict__ other2 = reinterpret_cast<const P*>(a.other);
  const int32_t* __restrict__ idx = a.idx + beg;
  const ST* __restrict__ vals = reinterpret_cast<const ST*>(a.vals) + beg;
  // Software pipeline: the indices/values of trip t+1 are requested while trip t computes, so the
  // dependent chain per trip is only the factor gather.  The trip count is wave-uniform; lanes past
  // the end of the segment re-read its last entry and are masked by `valid`.
  int c[U];
  double av_next[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    c[u] = 0;
    av_next[u] = 0.0;
    if (len > 0) {
      int64_t tt = gg + (int64_t)u * TG;
      tt = tt < len ? tt : len - 1;
      c[u] = idx[tt];
      av_next[u] = vals[tt];
    }
  }
  for (int64_t t0 = 0; t0 < len; t0 += (int64_t)TG * U) {
    P y[U][R / 2];
    double av[U];
    int ccur[U];
    bool valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      valid[u] = t0 + (int64_t)u * TG + gg < len;
      const P* __restrict__ yp = other2 + (int64_t)c[u] * (KP / 2) + j;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) y[u][i] = yp[i * G];
      av[u] = av_next[u];
      ccur[u] = c[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int64_t tn = t0 + (int64_t)(U + u) * TG + gg;
      tn = tn < len ? tn : len - 1;
      c[u] = idx[tn];
      av_next[u] = vals[tn];
    }
    if constexpr (SCATTER) {
      // Four observations per group and trip, one loss evaluation per LANE: the partial dot products are reduce-scattered in
      // two butterfly steps (the pairings of group_sum, hence its bits), lane u evaluates observation u, and the derivatives
      // come back by quad broadcasts.  The loop is wave-uniform, so every DPP source lane is active.
      double p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        p[u] = 0.0;
#pragma unroll
        for (int i = 0; i < R / 2; ++i) {
          p[u] = fma(xv.v[i].x, (double)y[u][i].x, p[u]);
          p[u] = fma(xv.v[i].y, (double)y[u][i].y, p[u]);
        }
      }
      const bool odd = (j & 1) != 0, hi2 = (j & 2) != 0;
      const double qa = (odd ? p[1] : p[0]) + dpp_f64<DPP_XOR1>(odd ? p[0] : p[1]);
      const double qb = (odd ? p[3] : p[2]) + dpp_f64<DPP_XOR1>(odd ? p[2] : p[3]);
      const double dot = (hi2 ? qb : qa) + dpp_f64<DPP_XOR2>(hi2 ? qa : qb); // observation u == j
      const double am = hi2 ? (odd ? av[3] : av[2]) : (odd ? av[1] : av[0]);
      const bool vm = hi2 ? (odd ? valid[3] : valid[2]) : (odd ? valid[1] : valid[0]);
      double L, dL;
      if constexpr (LM == LOSS_SEGMENT) {
        loss_both<GRAD, TRIG>(segloss, dot, am, L, dL);
      } else {
        const int cm = hi2 ? (odd ? ccur[3] : ccur[2]) : (odd ? ccur[1] : ccur[0]);
        const LossDesc lo = load_loss(a.losses, cm);
        loss_both<GRAD, TRIG>(lo, dot, am, L, dL);
      }
      if (!vm) {
        L = 0.0;
        dL = 0.0;
      }
      J += L; // lane-partial: summed over the group after the loop
      if (GRAD) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double d = group_bcast_f64<G>(dL, u, j);
#pragma unroll
          for (int i = 0; i < R / 2; ++i) {
            g.v[i].x = fma(d, (double)y[u][i].x, g.v[i].x);
            g.v[i].y = fma(d, (double)y[u][i].y, g.v[i].y);
          }
        }
      }
    } else {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double dot = 0.0;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        dot = fma(xv.v[i].x, (double)y[u][i].x, dot);
        dot = fma(xv.v[i].y, (double)y[u][i].y, dot);
      }
      dot = group_sum<G>(dot);
      double L, dL;
      if constexpr (LOSS == LOSS_QUAD_UNIFORM) {
        const double d = dot - av[u];
        L = segloss.scale * (d * d);
        dL = 2 * d * segloss.scale;
      } else if constexpr (LM == LOSS_SEGMENT) {
        loss_both<GRAD, TRIG>(segloss, dot, av[u], L, dL);
      } else {
        const LossDesc lo = load_loss(a.losses, ccur[u]);
        loss_both<GRAD, TRIG>(lo, dot, av[u], L, dL);
      }
      if (!valid[u]) {
        L = 0.0;
        dL = 0.0;
      }
      J += L;
      if (GRAD) {
#pragma unroll
        for (int i = 0; i < R / 2; ++i) {
          g.v[i].x = fma(dL, (double)y[u][i].x, g.v[i].x);
          g.v[i].y = fma(dL, (double)y[u][i].y, g.v[i].y);
        }
      }
    }
    }
  }
  if constexpr (SCATTER) J = group_sum<G>(J);
  J = across_groups_sum<G>(J);
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) {
      g.v[i].x = across_groups_sum<G>(g.v[i].x);
      g.v[i].y = across_groups_sum<G>(g.v[i].y);
    }
  }
  return J;
}

// Combine the per-wave totals of a multi-wave segment through LDS, in wave order, so that every
// thread of the block ends with the same bits.
template <int G, int R, int WAVES, bool GRAD>
__device__ __forceinline__ double block_combine(double J, Vec<G, R>& g, double* red, int wave, int lane) {
  constexpr int KP = G * R, STRIDE = KP + 2;
  if constexpr (WAVES == 1) return J;
  const int j = lane % G;
  __syncthreads(); // previous readers of `red` are done
  if (lane < G) {
    if (GRAD) {
#pragma unroll
      for (int i = 0; i < R / 2; ++i) *reinterpret_cast<double2*>(&red[wave * STRIDE + i * 2 * G + 2 * j]) = g.v[i];
    }
    if (lane == 0) red[wave * STRIDE + KP] = J;
  }
  __syncthreads();
  double Js = 0.0;
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) g.v[i] = make_double2(0.0, 0.0);
  }
  for (int w = 0; w < WAVES; ++w) {
    Js += red[w * STRIDE + KP];
    if (GRAD) {
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        const double2 p = *reinterpret_cast<const double2*>(&red[w * STRIDE + i * 2 * G + 2 * j]);
        g.v[i].x += p.x;
        g.v[i].y += p.y;
      }
    }
  }
  return Js;
}

// EVAL = true is the one-pass objective evaluation (obj[seg] = sum of losses); it is a separate
// instantiation so that profiles list it apart from the two-pass half-step sweeps.
template <int G, int R, int WAVES, int LOSS, int U, bool EVAL, bool VR = false, class ST = double>
__global__ void __launch_bounds__(WAVES == 1 ? 256 : WAVES * 64) sweep_kernel(const SweepArgs a) {
  using P = typename Pair<ST>::type;
  constexpr int KP = G * R, NG = 64 / G;
  __shared__ __attribute__((aligned(16))) double red[WAVES == 1 ? 2 : WAVES * (KP + 2)];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform -> SGPR
  const int64_t slot = WAVES == 1 ? (int64_t)blockIdx.x * 4 + wave : (int64_t)blockIdx.x;
  if (slot >= a.nseg) return; // wave-uniform (WAVES==1) or block-uniform
  int64_t seg = slot;
  if (a.seglist) {
    seg = (int64_t)a.seglist[slot];
    if (seg < a.seg_lo || seg >= a.seg_hi) return; // wave-uniform (WAVES==1) or block-uniform
  }
  const int j = lane % G, gi = lane / G;
  const int gg = (WAVES == 1 ? 0 : wave * NG) + gi;
  const int64_t beg = a.ptr[seg], len = a.ptr[seg + 1] - beg;
  const int64_t gseg = a.own_offset + seg;
  P* ownp = reinterpret_cast<P*>(reinterpret_cast<ST*>(a.own) + gseg * KP);

  Vec<G, R> x, g;
#pragma unroll
  for (int i = 0; i < R / 2; ++i) x.v[i] = widen(ownp[i * G + j]);
  const RegDesc rd = load_reg(a.regs, a.reg_single ? 0 : seg);
  LossDesc segloss;
  if constexpr (loss_mode(LOSS) != LOSS_PER_OBS) segloss = load_loss(a.losses, a.loss_by_segment ? gseg : 0);
  else segloss = LossDesc{0, 1.0, 0.0, 0.0};

  // pass 1: gradient + objective at the current point (proxgrad.jl:122-135 / :165-178)
  double Jold = sweep_pass<G, R, WAVES, LOSS, U, true, ST>(a, x, g, beg, len, gg, j, segloss);
  Jold = block_combine<G, R, WAVES, true>(Jold, g, red, wave, lane);
  if constexpr (EVAL) {
    if (threadIdx.x == (WAVES == 1 ? wave * 64 : 0) && a.obj) a.obj[gseg] = Jold;
    return;
  }
  if (a.fixed_alpha > 0.0) { // src/algorithms/sparse_proxgrad.jl:72-77 / :94-99: g *= -alpha/l; x += g; prox!(r, x, alpha/l)
    const double s = a.fixed_alpha / ((double)len + 1.0);
    Vec<G, R> xn;
#pragma unroll
    for (int i = 0; i < R / 2; ++i) {
      xn.v[i].x = x.v[i].x + g.v[i].x * (-s);
      xn.v[i].y = x.v[i].y + g.v[i].y * (-s);
    }
    reg_prox<G, R, VR>(rd, xn, s, j, a.k);
    if (wave == (WAVES == 1 ? wave : 0) && gi == 0) {
#pragma unroll
      for (int i = 0; i < R / 2; ++i) store_pair<ST>(&ownp[i * G + j], make_double2(stored<ST>(xn.v[i].x), stored<ST>(xn.v[i].y)));
    }
    return;
  }
  Jold += reg_eval<G, R, VR>(rd, x, j, a.k);

  // backtracking line search (proxgrad.jl:136-155 / :179-200); g is NOT recomputed between trials
  double alpha = a.alpha[seg];
  const double l = (double)len + 1.0;
  int ntrials = 0;
  bool accepted = false;
  while (alpha > a.min_stepsize) {
    const double s = alpha / l;
    Vec<G, R> xn, dummy;
#pragma unroll
    for (int i = 0; i < R / 2; ++i) { // axpy!(-stepsize, g, newx)
      xn.v[i].x = fma(-s, g.v[i].x, x.v[i].x);
      xn.v[i].y = fma(-s, g.v[i].y, x.v[i].y);
    }
    reg_prox<G, R, VR>(rd, xn, s, j, a.k); // prox!(r, newx, stepsize)
    if constexpr (sizeof(ST) == 4) { // the trial point is the point the storage will hold: the search compares objectives of stored factors
#pragma unroll
      for (int i = 0; i < R / 2; ++i) xn.v[i] = make_double2(stored<ST>(xn.v[i].x), stored<ST>(xn.v[i].y));
    }
    double Jn = sweep_pass<G, R, WAVES, LOSS, U, false, ST>(a, xn, dummy, beg, len, gg, j, segloss);
    Jn = block_combine<G, R, WAVES, false>(Jn, dummy, red, wave, lane);
    Jn += reg_eval<G, R, VR>(rd, xn, j, a.k);
    ++ntrials;
    if (Jn < Jold) { // strict; false for NaN and for Inf < Inf
      x = xn;
      alpha *= 1.05;
      Jold = Jn;
      accepted = true;
      break;
    }
    alpha *= .7;
    if (alpha < a.min_stepsize) {
      alpha = a.min_stepsize * 1.1;
      break;
    }
  }

  if (accepted && wave == (WAVES == 1 ? wave : 0) && gi == 0) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) store_pair<ST>(&ownp[i * G + j], x.v[i]);
  }
  if (lane == 0 && (WAVES == 1 || wave == 0)) {
    a.alpha[seg] = alpha;
    if (a.obj) a.obj[gseg] = Jold;
    if (a.trials) {
      a.trials[seg] += ntrials;
      a.accepts[seg] += accepted ? 1 : 0;
    }
  }
}

// evaluate(r, factor[:,seg]) for every local segment (calc_penalty, src/evaluate_fit.jl:91-104)
template <class ST = double>
__global__ void penalty_kernel(const ST* fac, int ld, int k, int64_t offset, int64_t nseg, const glrm_reg* regs,
                               int reg_single, double* out) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const struct { const ST* p; __device__ double operator[](int c) const { return (double)p[c]; } } x{fac + (offset + s) * ld};
  const glrm_reg r = regs[reg_single ? 0 : s];
  double v = 0.0;
  switch (r.kind) {
    case GLRM_REG_QUAD: {
      double acc = 0.0;
      for (int c = 0; c < k; ++c) acc += x[c] * x[c];
      v = r.scale * acc;
      break;
    }
    case GLRM_REG_ONE: {
      double acc = 0.0;
      for (int c = 0; c < k; ++c) acc += fabs(x[c]);
      v = r.scale * acc;
      break;
    }
    case GLRM_REG_NONNEG:
      for (int c = 0; c < k; ++c)
        if (x[c] < 0) v = __builtin_inf();
      break;
    case GLRM_REG_UNIT_ONE_SPARSE: {
      int ones = 0, other = 0;
      for (int c = 0; c < k; ++c) {
        if (x[c] == 0) continue;
        if (x[c] == 1) ++ones; else ++other;
      }
      if (other > 0 || ones > 1) v = __builtin_inf();
      break;
    }
    case GLRM_REG_QUAD_CONSTRAINT: {
      double acc = 0.0;
      for (int c = 0; c < k; ++c) acc += x[c] * x[c];
      if (sqrt(acc) > r.scale + 1e-12) v = __builtin_inf();
      break;
    }
    case GLRM_REG_NONNEG_ONE:
    case GLRM_REG_SIMPLEX: {
      double acc = 0.0;
      bool neg = false;
      for (int c = 0; c < k; ++c) {
        acc += x[c];
        neg = neg || x[c] < 0;
      }
      if (neg) v = __builtin_inf();
      else if (r.kind == GLRM_REG_NONNEG_ONE) v = r.scale * acc;
      else if (fabs(acc - 1) > 1e-12) v = __builtin_inf();
      break;
    }
    case GLRM_REG_ONE_SPARSE:
    case GLRM_REG_K_SPARSE: {
      int nz = 0;
      for (int c = 0; c < k; ++c)
        if (x[c] != 0) ++nz;
      if ((double)nz > (r.kind == GLRM_REG_ONE_SPARSE ? 1.0 : r.scale)) v = __builtin_inf();
      break;
    }
    default:
      break;
  }
  out[offset + s] = v;
}

// ------------------------------------------------------------------ sweep launch

// Observations per lane group in flight (a group adds its observations in ascending order whatever the count: the bits do not depend on it)
template <class ST, int G, int R, int WAVES>
void launch_sweep_loss(int loss, int side, const SweepArgs& a, hipStream_t st) {
  const unsigned grid = (unsigned)(WAVES == 1 ? (a.nseg + 3) / 4 : a.nseg);
  const dim3 block(WAVES == 1 ? 256 : WAVES * 64);
  auto launch = [&](auto LOSS, auto U) {
    if (a.eval_only) hipLaunchKernelGGL((sweep_kernel<G, R, WAVES, LOSS, 1, true, false, ST>), dim3(grid), block, 0, st, a); // losses only: no regularizer
    else if constexpr (sizeof(ST) == 8) { // the VR = true kernels exist for double storage only (a float handle refuses vector regularizers)
      if (a.vecreg) hipLaunchKernelGGL((sweep_kernel<G, R, WAVES, LOSS, U, false, true, ST>), dim3(grid), block, 0, st, a);
      else hipLaunchKernelGGL((sweep_kernel<G, R, WAVES, LOSS, U, false, false, ST>), dim3(grid), block, 0, st, a);
    } else hipLaunchKernelGGL((sweep_kernel<G, R, WAVES, LOSS, U, false, false, ST>), dim3(grid), block, 0, st, a);
    return GLRM_OK;
  };
  // One 8-wave workgroup per very long segment (the diverted columns of a power-law view: 880 000 observations at the C2-Zipf recipe) is
  // bound by the latency of its factor gathers: with one observation per lane group in flight the longest column alone took 13.7 ms of a
  // 15.7 ms Y half-step (profiles/r06_c2_zipf_kernel_stats.csv).  Eight per group in flight -- session r6_26.
  // G == 4, one wave: four observations per trip, one loss evaluation per lane (C5-family row sweep 169 -> 115 ms); the 4-wave sweeps of
  // long same-loss segments are bound by the factor gather and keep the leaner one-observation body.
  constexpr int U_SEG = WAVES == 8 ? 8 : (G == 4 && WAVES == 1 ? 4 : 1), U_OBS = WAVES == 8 ? 8 : (G == 4 ? 4 : 1);
  auto by_loss = [&](auto LOSS) {
    if constexpr (LOSS == LOSS_QUAD_UNIFORM) {
      if constexpr (WAVES == 1) { // two observations in flight on the row view: -20 % on the L2-latency-bound row sweep
        return side == GLRM_ROWS ? launch(LOSS, glrm_const<2>{}) : launch(LOSS, glrm_const<1>{});
      } else {
        return launch(LOSS, glrm_const<(WAVES == 8 ? 8 : 1)>{});
      }
    } else {
      return launch(LOSS, glrm_const<(loss_mode(LOSS) == 1 ? U_SEG : U_OBS)>{});
    }
  };
  glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
}

// (lanes per observation G, components per lane R) with G*R == kp: the layouts of pick_layout
template <class ST>
void launch_sweep_st(int G, int R, int waves, int loss, int side, const SweepArgs& a, hipStream_t st) {
  auto by_layout = [&](auto g, auto r) {
    constexpr int GG = decltype(g)::value, RR = decltype(r)::value;
    auto by_waves = [&](auto W) { launch_sweep_loss<ST, GG, RR, decltype(W)::value>(loss, side, a, st); return GLRM_OK; };
    return glrm_dispatch<1, 4>(waves, by_waves, [&] { return by_waves(glrm_const<8>{}); });
  };
  glrm_dispatch_layout<8, 16, 32, 64>(G, R, by_layout, [&] { return by_layout(glrm_const<16>{}, glrm_const<8>{}); });
}

// the penalty kernel over a side's local segments (the caller has checked that there are some)
template <class ST>
void launch_penalty_st(const glrm_handle* h, int side) {
  const glrm_handle::Side& v = h->side[side];
  hipLaunchKernelGGL(penalty_kernel<ST>, dim3((unsigned)((v.nseg + 255) / 256)), dim3(256), 0, h->stream, reinterpret_cast<const ST*>(v.factor), h->kp, h->k,
                     v.begin, v.nseg, v.regs, v.n_regs == 1 ? 1 : 0, v.obj);
}

} // namespace glrm
