// glrm_cached.hpp -- the REGISTER variant of the cached row sweep (see glrm_cached.hip for the family): its argument struct, the pass over
// a row held in registers, the one-row-per-workgroup kernel, the persistent kernel and their launch.  Templates over the STORAGE type ST
// of the observation values and the factors (include/glrm_hip_storage.h), the way glrm_sweep.hpp has it for the gather sweeps:
// glrm_cached.hip instantiates ST = double, glrm_cached_f32.hip ST = float (two waves per row, VR = false, line search only).  ST changes
// loads, stores, the width of the row's vectors in registers and one rounding after the prox step; every sum is fp64 in the same order.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "glrm_device.hpp"
#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_sweep.hpp" // Pair, widen, stored, store_pair

namespace glrm {

struct CachedArgs {
  int64_t nseg;
  const int64_t* ptr;
  const int32_t* idx;
  const double* vals; // (ST behind the double* type, as in glrm_handle)
  double* own;
  int64_t own_offset;
  const double* other;
  double* alpha;
  const glrm_loss* losses;
  const glrm_reg* regs;
  int reg_single;
  int k;
  double fixed_alpha;
  double min_stepsize;
  int32_t* trials;
  int32_t* accepts;
  int cap; // LDS variant: vectors a wave's buffer holds (a multiple of the vectors one DMA instruction moves);
           // register variant: trips of 64 / G observations the longest row of this launch needs
  const int32_t* seglist; // nullable: the launch covers the local rows seglist[0..nseg) -- the rows short enough for the cached
                          // sweep when the shard also holds longer ones -- restricted to [seg_lo, seg_hi) (glrm_hip_step_x_range)
  int64_t seg_lo, seg_hi;
  int vecreg;            // 1: some rx names a vector regularizer -- the VR = true kernels
};

__device__ __forceinline__ int64_t cached_segment(const CachedArgs& a, int64_t slot) { // -1: nothing to do for this workgroup
  if (slot >= a.nseg) return -1;
  if (!a.seglist) return slot;
  const int64_t seg = a.seglist[slot];
  return (seg < a.seg_lo || seg >= a.seg_hi) ? -1 : seg;
}

// A stored element as the double the fma takes.  The float form converts at EVERY use and the compiler must not see through it: the
// row's vectors are read by the gradient pass and by every trial of the line search, so an ordinary conversion is hoisted out of the
// search loop and the row is then held in registers as doubles beside the floats -- the registers the float form exists to save.
__device__ __forceinline__ double cached_wide(double v) { return v; }
__device__ __forceinline__ double cached_wide(float v) {
  double d;
  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d) : "v"(v));
  return d;
}

// ---- the row's vectors in REGISTERS ---------------------------------------------------------------------------------------------
// A 64-thread workgroup may use 512 VGPRs per lane: at k = 64 a row of up to MAXT * 8 observations is MAXT * 16 VGPRs per lane in the
// lane layout of the gather sweeps (lane group gi holds the vectors of observations gi, gi + NG, ...).  The row's vectors are loaded
// ONCE -- all MAXT * R / 2 16-byte loads of a lane in flight together -- and the gradient pass, the prox and every line-search trial run
// from registers: no LDS, four waves per CU, every trip of a pass independent of the others (the compiler interleaves them).
// (WAVES = 2: two waves share a row, wave w holds the observations (t * WAVES + w) * NG + gi; `gi0` = w * NG + gi and the stride NG * WAVES)
// (ST = float: a chunk is one 8-byte float2, MAXT * 8 VGPRs at k = 64, widened in the fma that uses it)
template <int G, int R, int LOSS, int MAXT, bool GRAD, int WAVES = 1, class ST = double>
__device__ __forceinline__ double reg_pass(const CachedArgs& a, const typename Pair<ST>::type (&y)[MAXT][R / 2], const ST (&av)[MAXT], const int (&cc)[MAXT],
                                           const Vec<G, R>& xv, Vec<G, R>& g, int len, int gi, const LossDesc& segloss) {
  constexpr int NG = (64 / G) * WAVES, LM = loss_mode(LOSS);
  constexpr bool TRIG = loss_trig(LOSS);
  double J = 0.0;
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) g.v[i] = make_double2(0.0, 0.0);
  }
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if (t * NG + (gi & ~(64 / G - 1)) < len) { // wave-uniform: gi = wave * (64 / G) + group
      double dot = 0.0;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        dot = fma(xv.v[i].x, cached_wide(y[t][i].x), dot);
        dot = fma(xv.v[i].y, cached_wide(y[t][i].y), dot);
      }
      dot = group_sum<G>(dot);
      double L, dL;
      if constexpr (LOSS == LOSS_QUAD_UNIFORM) {
        const double d = dot - (double)av[t];
        L = segloss.scale * (d * d);
        dL = 2 * d * segloss.scale;
      } else if constexpr (LM == LOSS_SEGMENT) {
        loss_both<GRAD, TRIG>(segloss, dot, (double)av[t], L, dL);
      } else {
        const LossDesc lo = load_loss(a.losses, cc[t]);
        loss_both<GRAD, TRIG>(lo, dot, (double)av[t], L, dL);
      }
      if (!(t * NG + gi < len)) {
        L = 0.0;
        dL = 0.0;
      }
      J += L;
      if (GRAD) {
#pragma unroll
        for (int i = 0; i < R / 2; ++i) {
          g.v[i].x = fma(dL, cached_wide(y[t][i].x), g.v[i].x);
          g.v[i].y = fma(dL, cached_wide(y[t][i].y), g.v[i].y);
        }
      }
    }
  }
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

// Per-wave totals of a row shared by WAVES waves, combined through LDS in wave order: every wave ends with the same bits.
template <int G, int R, int WAVES, bool GRAD>
__device__ __forceinline__ double row_combine(double J, Vec<G, R>& g, double* red, int wave, int lane) {
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

// the trial point as the storage will hold it (glrm_sweep.hpp: stored): the search compares objectives of stored factors
template <class ST, int G, int R>
__device__ __forceinline__ void round_trial(Vec<G, R>& xn) {
  if constexpr (sizeof(ST) == 4) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) xn.v[i] = make_double2(stored<ST>(xn.v[i].x), stored<ST>(xn.v[i].y));
  }
}

// WAVES waves (= one workgroup) per row; wave w holds the observations (t * WAVES + w) * (64 / G) + group, t = 0 .. MAXT - 1.
template <int G, int R, int LOSS, int MAXT, int WAVES, bool VR = false, class ST = double>
__global__ void __launch_bounds__(WAVES * 64) regcached_sweep_kernel(const CachedArgs a) {
  using P = typename Pair<ST>::type;
  constexpr int KP = G * R, NG = (64 / G) * WAVES;
  __shared__ __attribute__((aligned(16))) double red[WAVES == 1 ? 2 : WAVES * (KP + 2)];
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

  double Jold = reg_pass<G, R, LOSS, MAXT, true, WAVES, ST>(a, y, av, cc, x, g, len, gi, segloss);
  Jold = row_combine<G, R, WAVES, true>(Jold, g, red, wave, lane);
  if constexpr (sizeof(ST) == 8) { // (a float handle has no fixed-stepsize fit: glrm_hip_fit_sparse refuses it)
    if (a.fixed_alpha > 0.0) {
      const double s = a.fixed_alpha / ((double)len + 1.0);
      Vec<G, R> xn;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        xn.v[i].x = x.v[i].x + g.v[i].x * (-s);
        xn.v[i].y = x.v[i].y + g.v[i].y * (-s);
      }
      reg_prox<G, R, VR>(rd, xn, s, j, a.k);
      if (gi == 0) {
#pragma unroll
        for (int i = 0; i < R / 2; ++i) store_pair<ST>(&ownp[i * G + j], xn.v[i]);
      }
      return;
    }
  }
  Jold += reg_eval<G, R, VR>(rd, x, j, a.k);
  double alpha = a.alpha[seg];
  const double l = (double)len + 1.0;
  int ntrials = 0;
  bool accepted = false;
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
  if (accepted && gi == 0) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) store_pair<ST>(&ownp[i * G + j], x.v[i]);
  }
  if (lane == 0 && wave == 0) {
    a.alpha[seg] = alpha;
    if (a.trials) {
      a.trials[seg] += ntrials;
      a.accepts[seg] += accepted ? 1 : 0;
    }
  }
}

// Waves per SIMD the persistent kernel is compiled for (the second argument of its __launch_bounds__).  The fp64 C4 instantiation
// <8, 8, LOSS_QUAD_UNIFORM, 7> takes the 256 VGPRs two waves leave it.  The float one needs 205 without scratch: the row's vectors are 56
// VGPRs instead of 112, but three waves per SIMD would leave 168, and compiled for that it spills (144 bytes of scratch per lane,
// among them addresses on the row's chain).  So two for both (profiles/storage_f32_cached_resusage.txt).
template <class ST> constexpr int cached_persist_waves_per_simd() { return 2; }

// ---- persistent form: a workgroup walks rows slot, slot + gridDim.x, ... and hands the NEXT row's record -- its (index, value) list and
// its stored stepsize -- over while it works on the current one.  In the one-row-per-workgroup kernel above a row's life is three
// dependent memory round trips -- row pointer -> list -> opposing vectors -- before the first FMA, a fourth for the stepsize between the
// gradient pass and the first trial, and two more for the counters at its end, with two waves per SIMD to hide them (244 VGPRs).  Here
// the pointers of the next row are scalar loads issued one row ahead; its list and stepsize are requested right behind the current row's
// gathers (3 * PF + 2 dwords per lane, live until the gradient pass has been combined) and reach the lanes through the OTHER of two
// record buffers in LDS; the counters are result-less atomic adds.  The chain per row is ONE round trip, the gathers, and a row ends
// with its stores and one barrier: nothing waits for a store.  Which lane group adds which observation, and in which order, is
// unchanged: same bits as the kernel above.
// Reading alpha[seg_n] a row early is safe: a row's stepsize is written once per launch, by the workgroup that owns the row (the long
// rows on the gather sweep write only their own), so until this workgroup reaches the row nobody has written it.
template <int G, int R, int LOSS, int MAXT, bool VR = false, class ST = double>
__global__ void __launch_bounds__(128, cached_persist_waves_per_simd<ST>()) regcached_persist_kernel(const CachedArgs a) {
  using P = typename Pair<ST>::type;
  constexpr int WAVES = 2, KP = G * R, NG = (64 / G) * WAVES, MAXLEN = MAXT * NG, PF = (MAXLEN + 127) / 128;
  // ONE shared array (a second __shared__ object makes hipcc drain the load queue before every LDS read, cdna_hip_programming.md):
  // [combine buffer: WAVES * (KP + 2) doubles] 2 x [values: PF * 128 ST][stepsize: 128 doubles][indices: PF * 128 ints]
  // (the stepsize once per thread: every thread parks the copy it loaded and takes it back itself, so no thread skips the wait for its
  // loads -- with one writer the others would reach the end of the row with a load the compiler still counts, and wait there)
  constexpr int VW = (int)sizeof(ST) / 4;              // dwords per value
  constexpr int VALD = PF * 128 * VW / 2;              // the value part of a record, in doubles
  constexpr int RED = WAVES * (KP + 2), REC = VALD + 128 + PF * 64;
  __shared__ __attribute__((aligned(16))) double sh[RED + 2 * REC];
  double* red = sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane % G, gi = wave * (64 / G) + lane / G;
  const RegDesc rd0 = load_reg(a.regs, 0);
  LossDesc segloss = LossDesc{0, 1.0, 0.0, 0.0};
  if constexpr (loss_mode(LOSS) != LOSS_PER_OBS) segloss = load_loss(a.losses, 0);
  const P* __restrict__ other2 = reinterpret_cast<const P*>(a.other);
  const ST* gvals = reinterpret_cast<const ST*>(a.vals);

  // The row pointers and the row list are read through the constant address space: nothing writes them while the kernel runs, and a
  // uniform load from there is a SCALAR load.  As ordinary global loads they come out as vector loads inside the row loop (the loop's
  // stores might alias them), each waited for on the spot -- a round trip at the head of every row that also drains the row's stores.
  const auto* kptr = (const __attribute__((address_space(4))) int64_t*)a.ptr;
  const auto* klist = (const __attribute__((address_space(4))) int32_t*)a.seglist;
  // segment of a slot (-1: none / filtered out; cached_segment), its record
  auto seg_of = [&](int64_t slot) -> int64_t {
    if (slot >= a.nseg) return -1;
    if (!a.seglist) return slot;
    const int64_t s = klist[slot];
    return (s < a.seg_lo || s >= a.seg_hi) ? -1 : s;
  };
  auto rec_vals = [&](int buf) -> ST* { return reinterpret_cast<ST*>(sh + RED + buf * REC); };
  auto rec_alpha = [&](int buf) -> double* { return sh + RED + buf * REC + VALD; };
  auto rec_idx = [&](int buf) -> int* { return reinterpret_cast<int*>(sh + RED + buf * REC + VALD + 128); };
  auto fetch_rec = [&](int64_t sg, int64_t beg, int len, int (&pi)[PF], int (&pv)[VW * PF], double& pa) { // this lane's share, clamped
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      int e = q * 128 + tid;
      e = e < len ? e : (len > 0 ? len - 1 : 0);
      pi[q] = len > 0 ? a.idx[beg + e] : 0;
      if constexpr (VW == 2) {
        const int2 v = len > 0 ? *reinterpret_cast<const int2*>(gvals + beg + e) : make_int2(0, 0);
        pv[2 * q] = v.x; pv[2 * q + 1] = v.y;
      } else {
        pv[q] = len > 0 ? *reinterpret_cast<const int*>(gvals + beg + e) : 0;
      }
    }
    pa = a.alpha[sg >= 0 ? sg : 0]; // an empty row still runs its line search; no row: some valid address, never used
  };
  auto store_rec = [&](int buf, const int (&pi)[PF], const int (&pv)[VW * PF], double pa) {
    int* li = rec_idx(buf);
    int* lv = reinterpret_cast<int*>(rec_vals(buf));
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      li[q * 128 + tid] = pi[q];
      if constexpr (VW == 2) {
        lv[2 * (q * 128 + tid)] = pv[2 * q];
        lv[2 * (q * 128 + tid) + 1] = pv[2 * q + 1];
      } else {
        lv[q * 128 + tid] = pv[q];
      }
    }
    rec_alpha(buf)[tid] = pa;
  };

  int64_t slot = blockIdx.x;
  int64_t seg = seg_of(slot), seg_n = seg_of(slot + gridDim.x);
  int64_t beg = seg >= 0 ? kptr[seg] : 0, beg_n = seg_n >= 0 ? kptr[seg_n] : 0; // (a.nseg >= 1: ptr[0] and ptr[1] exist)
  int len = seg >= 0 ? (int)(kptr[seg + 1] - beg) : 0, len_n = seg_n >= 0 ? (int)(kptr[seg_n + 1] - beg_n) : 0;
  {
    int pi[PF], pv[VW * PF];
    double pa;
    fetch_rec(seg, beg, len, pi, pv, pa);
    store_rec(0, pi, pv, pa);
  }
  __syncthreads();
  int cur = 0; // the record buffer of the current row; the next row's is written into the other one
  for (; slot < a.nseg; slot += gridDim.x) { // block-uniform
    // the row after the next one: pointers only (scalar loads, consumed an iteration from now; issued behind the gathers, where the wait
    // for them falls into the gathers' shadow)
    int64_t seg_nn, beg_nn;
    int len_nn;
    auto next_pointers = [&] {
      seg_nn = seg_of(slot + 2 * (int64_t)gridDim.x);
      const int64_t p0 = kptr[seg_nn >= 0 ? seg_nn : 0], p1 = kptr[(seg_nn >= 0 ? seg_nn : 0) + 1];
      beg_nn = seg_nn >= 0 ? p0 : 0;
      len_nn = seg_nn >= 0 ? (int)(p1 - p0) : 0;
    };
    if (seg < 0) { // a slot the row range filters out: only the hand-over
      int pi[PF], pv[VW * PF];
      double pa;
      fetch_rec(seg_n, beg_n, len_n, pi, pv, pa);
      next_pointers();
      store_rec(cur ^ 1, pi, pv, pa);
    } else {
      const ST* lvals = rec_vals(cur);
      const int* lidx = rec_idx(cur);
      int cc[MAXT];
      ST av[MAXT];
      P y[MAXT][R / 2];
#pragma unroll
      for (int t = 0; t < MAXT; ++t) { // the group's entries out of LDS (clamped: lanes past the end re-read the last entry and are masked)
        int tt = t * NG + gi;
        tt = tt < len ? tt : (len > 0 ? len - 1 : 0);
        cc[t] = lidx[tt];
        av[t] = lvals[tt];
      }
      const int64_t gseg = a.own_offset + seg;
      P* ownp = reinterpret_cast<P*>(reinterpret_cast<ST*>(a.own) + gseg * KP);
      Vec<G, R> x, g;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) x.v[i] = widen(ownp[i * G + j]);
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
      // the next row's record rides behind the gathers
      int pi[PF], pv[VW * PF];
      double pa;
      fetch_rec(seg_n, beg_n, len_n, pi, pv, pa);
      next_pointers();
      const RegDesc rd = a.reg_single ? rd0 : load_reg(a.regs, seg);

      double Jold = reg_pass<G, R, LOSS, MAXT, true, WAVES, ST>(a, y, av, cc, x, g, len, gi, segloss);
      Jold = row_combine<G, R, WAVES, true>(Jold, g, red, wave, lane);
      // hand the next row's record over now: the loads above are the youngest in the queue and none of this row's stores is in it yet.
      // The other buffer's readers (the previous row) are behind the barrier that ended their row.
      store_rec(cur ^ 1, pi, pv, pa);
      bool fixed = false; // (a float handle has no fixed-stepsize fit: glrm_hip_fit_sparse refuses it)
      if constexpr (sizeof(ST) == 8) fixed = a.fixed_alpha > 0.0;
      if (fixed) {
        const double s = a.fixed_alpha / ((double)len + 1.0);
        Vec<G, R> xn;
#pragma unroll
        for (int i = 0; i < R / 2; ++i) {
          xn.v[i].x = x.v[i].x + g.v[i].x * (-s);
          xn.v[i].y = x.v[i].y + g.v[i].y * (-s);
        }
        reg_prox<G, R, VR>(rd, xn, s, j, a.k);
        if (gi == 0) {
#pragma unroll
          for (int i = 0; i < R / 2; ++i) store_pair<ST>(&ownp[i * G + j], xn.v[i]);
        }
      } else {
        Jold += reg_eval<G, R, VR>(rd, x, j, a.k);
        double alpha = rec_alpha(cur)[tid]; // fetched a row ago
        const double l = (double)len + 1.0;
        int ntrials = 0;
        bool accepted = false;
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
        if (accepted && gi == 0) {
#pragma unroll
          for (int i = 0; i < R / 2; ++i) store_pair<ST>(&ownp[i * G + j], x.v[i]);
        }
        if (tid == 0) {
          a.alpha[seg] = alpha;
          if (a.trials) { // int32 adds on counters only this workgroup touches in this launch: same values as +=, and nothing to wait for
            atomicAdd(&a.trials[seg], ntrials);
            atomicAdd(&a.accepts[seg], accepted ? 1 : 0);
          }
        }
      }
    }
    __syncthreads(); // the next row's record is in place; everybody is done with this row's (and with the combine buffer)
    cur ^= 1;
    seg = seg_n; beg = beg_n; len = len_n;
    seg_n = seg_nn; beg_n = beg_nn; len_n = len_nn;
  }
}

template <int G, int R, int LOSS, bool VR, class ST = double>
int launch_reg_inst(const CachedArgs& a, hipStream_t st, glrm_handle* h) { // a.cap = trips of one wave the longest row needs (64 / G observations each)
  // Two waves per row (each holds every other trip's vectors: half the registers, two waves per SIMD, so one wave's loads overlap the
  // other's arithmetic).  Measured at C4, X half-step: one wave per row 101.5 ms, two 85.4 ms, four 130.3 ms (phase-aligned passes 120.6).
  // ALWAYS two, also for rows one wave could hold: the wave count fixes the order of the sums, and it must not depend on the
  // longest row of the launch (MAXT only adds empty trips).  GLRM_HIP_CACHED_WAVES = 1 | 4 are the experiment switches (fp64 only:
  // the float form exists for two waves).
  constexpr bool F32 = sizeof(ST) == 4;
  const int waves = h->cached_waves; // (what set-up read: the wave count fixes the order of the sums)
  if (waves == 2 && knob(Knob::CACHED_PERSIST)) { // the persistent form of the two-wave kernel (same bits)
    // resident grid per handle (its device's CU count, its loss variant's occupancy, the fill percentage at its first sweep); the float
    // kernels have an occupancy of their own, hence slots of their own
    const bool small = (a.cap + 1) / 2 <= 4;
    int& cache = h->cached_grid[(small ? 1 : 0) + (VR ? 2 : 0) + (F32 ? 4 : 0)];
    int nb = cache;
    if (nb == 0) {
      int per_cu = 0;
      hipDeviceProp_t prop;
      const void* k = small ? (const void*)regcached_persist_kernel<G, R, LOSS, 4, VR, ST> : (const void*)regcached_persist_kernel<G, R, LOSS, 7, VR, ST>;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 128, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
      int cus = 256;
      if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
      nb = per_cu * cus; // the resident grid
      if (nb < 1) nb = 1;
      cache = nb;
    }
    const unsigned grid = (unsigned)std::min<int64_t>(a.nseg, nb);
    if (small) hipLaunchKernelGGL((regcached_persist_kernel<G, R, LOSS, 4, VR, ST>), dim3(grid), dim3(128), 0, st, a);
    else hipLaunchKernelGGL((regcached_persist_kernel<G, R, LOSS, 7, VR, ST>), dim3(grid), dim3(128), 0, st, a);
    return GLRM_OK;
  }
  if constexpr (!F32) {
    if (waves == 4 && (a.cap + 3) / 4 <= 4) {
      hipLaunchKernelGGL((regcached_sweep_kernel<G, R, LOSS, 4, 4, VR, ST>), dim3((unsigned)a.nseg), dim3(256), 0, st, a);
      return GLRM_OK;
    }
    if (waves == 1) {
      if (a.cap <= 7) hipLaunchKernelGGL((regcached_sweep_kernel<G, R, LOSS, 7, 1, VR, ST>), dim3((unsigned)a.nseg), dim3(64), 0, st, a);
      else hipLaunchKernelGGL((regcached_sweep_kernel<G, R, LOSS, 13, 1, VR, ST>), dim3((unsigned)a.nseg), dim3(64), 0, st, a);
      return GLRM_OK;
    }
  }
  if ((a.cap + 1) / 2 <= 4) {
    hipLaunchKernelGGL((regcached_sweep_kernel<G, R, LOSS, 4, 2, VR, ST>), dim3((unsigned)a.nseg), dim3(128), 0, st, a);
  } else {
    hipLaunchKernelGGL((regcached_sweep_kernel<G, R, LOSS, 7, 2, VR, ST>), dim3((unsigned)a.nseg), dim3(128), 0, st, a);
  }
  return GLRM_OK;
}

} // namespace glrm

// the float instantiations (glrm_cached_f32.hip): layouts (4, 8) and (8, 8), the five loss variants, two waves per row
int glrm_launch_cached_f32(const glrm::CachedArgs& a, int G, int loss, hipStream_t st, glrm_handle* h);
