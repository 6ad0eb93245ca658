// glrm_cached.hip -- row sweep with the row's opposing vectors fetched ONCE per half-step ("cached gather sweep").
//
// Where the opposing factor is far beyond L2 and a row is short (BASELINE config 4: 100 observations per row, rank 64, Y = 51 MB), the
// gather sweeps are bound by the k-vector gathers -- 512 B per observation and PASS, gradient pass and every line-search trial alike
// (the X half-step at C4: 2 x 1e9 x 512 B at the 8.2 TB/s the Infinity Cache delivers for such reads = 121 ms).  But all passes of
// a row's half-step read the SAME vectors: Y does not change during the X half-step.  So the row's vectors are fetched once and kept
// on chip for the gradient pass, the prox and every trial of the backtracking line search; the gather traffic of the half-step drops
// from (1 + trials) passes to one.  Two homes for the row:
//   registers (regcached_sweep_kernel, the default; rows of <= 13 trips of the lane layout): a 64-lane
//             wave may use 512 VGPRs per lane; two waves share a row, each holding every other trip's vectors, all loads of a wave
//             in flight together; the passes are straight-line code over registers.  C4 X half-step 120.6 -> 85.4 ms.
//   LDS       (cached_sweep_kernel; rows up to the LDS budget): one wave per row, the row gathered with LDS-DMA.  C4: 110.5 ms.
//
// Applies to the ROW view; index lists in any order.  Summation: a lane group takes its observations in ascending order, the groups of
// a wave are combined by the butterfly of the gather sweeps (glrm_hip.hip: sweep_pass), the waves of a row in wave order.
// The register variant and its persistent form are templates over the storage type (glrm_cached.hpp); this unit holds their double
// instantiations and the LDS variant, which has no float form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "glrm_device.hpp"
#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_cached.hpp"

using namespace glrm;

namespace {

// One pass over the row out of LDS: J = sum of losses at u = <xv, y_t>, and (GRAD) g = sum of dL * y_t.
template <int G, int R, int LOSS, bool GRAD>
__device__ __forceinline__ double cached_pass(const CachedArgs& a, const char* __restrict__ ybuf, const double* __restrict__ lval,
                                              const int32_t* __restrict__ lidx, const Vec<G, R>& xv, Vec<G, R>& g, int len, int gi, int j,
                                              const LossDesc& segloss) {
  constexpr int KPB = G * R * 8, NG = 64 / G, LM = loss_mode(LOSS), U = 4; // U: observations per group in flight per trip (2: 111.9 ms, 4: 109.6 ms at C4)
  constexpr bool TRIG = loss_trig(LOSS);
  double J = 0.0;
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) g.v[i] = make_double2(0.0, 0.0);
  }
  for (int t0 = 0; t0 < len; t0 += NG * U) { // wave-uniform trip count; U observations per group in flight
    double2 y[U][R / 2];
    double av[U];
    int cc[U];
    bool valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u * NG + gi;
      valid[u] = t < len;
      const int tt = valid[u] ? t : len - 1;
      const char* yp = ybuf + tt * KPB + j * 16;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) y[u][i] = *reinterpret_cast<const double2*>(yp + i * (G * 16));
      av[u] = lval[tt];
      cc[u] = lidx[tt];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double dot = 0.0;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        dot = fma(xv.v[i].x, y[u][i].x, dot);
        dot = fma(xv.v[i].y, y[u][i].y, dot);
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
        const LossDesc lo = load_loss(a.losses, cc[u]);
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
          g.v[i].x = fma(dL, y[u][i].x, g.v[i].x);
          g.v[i].y = fma(dL, y[u][i].y, g.v[i].y);
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

// One wave (= one workgroup) per row.  Dynamic LDS: [cap vectors][cap values][cap indices].
template <int G, int R, int LOSS, bool VR = false>
__global__ void __launch_bounds__(64) cached_sweep_kernel(const CachedArgs a) {
  constexpr int KP = G * R, KPB = KP * 8, CPV = KPB / 16, VPI = 64 / CPV; // 16-byte chunks per vector, vectors per DMA instruction
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int lane = threadIdx.x;
  const int64_t seg = cached_segment(a, blockIdx.x);
  if (seg < 0) return;
  const int j = lane % G, gi = lane / G;
  const int64_t beg = a.ptr[seg];
  const int len = (int)(a.ptr[seg + 1] - beg);
  const int64_t gseg = a.own_offset + seg;
  double2* ownp = reinterpret_cast<double2*>(a.own + gseg * KP);
  char* ybuf = lds;
  double* lval = reinterpret_cast<double*>(lds + (size_t)a.cap * KPB);
  int32_t* lidx = reinterpret_cast<int32_t*>(lds + (size_t)a.cap * (KPB + 8));

  // the row's (index, value) list -> LDS
  for (int t = lane; t < len; t += 64) {
    lidx[t] = a.idx[beg + t];
    lval[t] = a.vals[beg + t];
  }
  __syncthreads(); // one wave: orders the LDS writes above before the reads below
  Vec<G, R> x, g;
#pragma unroll
  for (int i = 0; i < R / 2; ++i) x.v[i] = ownp[i * G + j];
  const RegDesc rd = load_reg(a.regs, a.reg_single ? 0 : seg);
  LossDesc segloss = LossDesc{0, 1.0, 0.0, 0.0};
  if constexpr (loss_mode(LOSS) != LOSS_PER_OBS) segloss = load_loss(a.losses, 0);
  const double alpha0 = a.alpha[seg];
  // gather the row's opposing vectors into LDS with LDS-DMA: lane l of instruction `it` moves chunk l % CPV of vector it * VPI + l / CPV.
  // No VGPRs, the whole row in flight at once.  Measured alternatives at C4 (X half-step; phase-aligned passes 120 ms): this 112 ms;
  // the gradient pass streamed behind the DMA with counted vmcnt waits 124 ms; 26 ordinary 16-byte loads per lane in flight, then
  // ds_write 129 ms.
  if (len > 0) {
    const int vsub = lane / CPV, chunk = lane % CPV;
    const char* obase = reinterpret_cast<const char*>(a.other) + chunk * 16;
    for (int it = 0; it * VPI < len; ++it) {
      int s = it * VPI + vsub;
      s = s < len ? s : len - 1; // the tail re-reads the last vector into an unused slot
      const char* src = obase + (int64_t)lidx[s] * KPB;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(ybuf + it * 1024), 16, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the gathered vectors have landed
  __syncthreads();

  // pass 1: gradient + objective at the current point (proxgrad.jl:122-135)
  double Jold = cached_pass<G, R, LOSS, true>(a, ybuf, lval, lidx, x, g, len, gi, j, segloss);
  if (a.fixed_alpha > 0.0) { // src/algorithms/sparse_proxgrad.jl:72-77: g *= -alpha/l; x += g; prox!(r, x, alpha/l)
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
      for (int i = 0; i < R / 2; ++i) ownp[i * G + j] = xn.v[i];
    }
    return;
  }
  Jold += reg_eval<G, R, VR>(rd, x, j, a.k);

  // backtracking line search (proxgrad.jl:136-155); every trial reads the cached vectors
  double alpha = alpha0;
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
    double Jn = cached_pass<G, R, LOSS, false>(a, ybuf, lval, lidx, xn, dummy, len, gi, j, segloss);
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
  if (accepted && gi == 0) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) ownp[i * G + j] = x.v[i];
  }
  if (lane == 0) {
    a.alpha[seg] = alpha;
    if (a.trials) {
      a.trials[seg] += ntrials;
      a.accepts[seg] += accepted ? 1 : 0;
    }
  }
}

template <int G, int R, int LOSS, bool VR>
int launch_inst(const CachedArgs& a, hipStream_t st) {
  const int lds = a.cap * (G * R * 8 + 12);
  if (lds > 65536)
    HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(cached_sweep_kernel<G, R, LOSS, VR>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL((cached_sweep_kernel<G, R, LOSS, VR>), dim3((unsigned)a.nseg), dim3(64), lds, st, a);
  return GLRM_OK;
}

} // namespace

// What the family asks of a problem before any size comes into it: `want` (the CACHED knob: -1 auto, 0 off, 1 wherever the rows fit) is
// not off, the rows are not LDS-tiled, the row view holds an observation, and the lane layout is (4, 8) or (8, 8).
static bool cached_admits(const glrm_handle* h, int want) {
  if (want == 0 || h->side[GLRM_ROWS].tiled || h->sig.nnz_rows <= 0) return false;
  return (h->G == 4 || h->G == 8) && h->R == 8;
}
// the variant: 2 registers, 1 LDS (GLRM_HIP_CACHED_REGS=0; fp64 only -- the LDS variant has no float form); the waves that share a row of
// the register variant: two (GLRM_HIP_CACHED_WAVES = 1 | 4 are experiment switches of the fp64 kernels)
static void cached_variant_of(const glrm_handle* h, int* variant, int* waves) {
  const bool f32 = h->storage == GLRM_STORAGE_F32;
  *variant = (f32 || knob(Knob::CACHED_REGS)) ? 2 : 1;
  *waves = *variant != 2 ? 1 : f32 ? 2 : knob(Knob::CACHED_WAVES);
}

// Does the WHOLE problem run its short rows on the cached sweep (glrm_handle::cached_want)?  Auto (GLRM_HIP_CACHED unset): the rows
// are not LDS-tiled, the opposing factor is beyond the sizes where the plain gathers already do well (> 32 MB) and the row view
// holds >= 1e8 observations -- all read from glrm_signature and (m, n, k), never from the shard.  WHICH rows it takes is a
// function of the row's own length (glrm_handle::cached_maxlen): registers hold up to 13 trips of the lane layout (104 observations at
// k = 64, 208 at k <= 32); the LDS variant (GLRM_HIP_CACHED_REGS=0) up to its buffer.  Longer rows run the gather sweep with the
// waves their length asks for.  A row is therefore always summed in the same order, whatever shard holds it.
// A float handle (glrm_options.storage = 1): the register variant only (glrm_handle::cached_variant), the same rows, and the auto rule is the
// fp64 one on the same (n, kp, nnz_rows) -- the factor counted in 8-byte elements -- so that one problem runs its rows on the same
// family in both storages.  GLRM_CACHED_F32_AUTO says whether the measurement adopted it.
int glrm_setup_cached(glrm_handle* h) {
  h->cached_row = h->cached_want = 0;
  // glrm_hip_solve_x (glrm_handle::solve_ok): could the handle run the two-wave register variant here?  The same predicate without what
  // decides the family of step_x -- glrm_options.tiled = 1 as the knob's default, and the auto rule's sizes below.  (The phase-aligned
  // passes are set up after this; solve_x asks the handle's family when it is called.)
  int variant, waves;
  cached_variant_of(h, &variant, &waves);
  h->solve_ok = cached_admits(h, knob_or(Knob::CACHED, -1)) && variant == 2 && waves == 2;
  const int want = knob_or(Knob::CACHED, h->tiled_opt == 1 ? 0 : -1); // -1 auto, 0 off, 1 wherever the rows fit
  if (!cached_admits(h, want)) return GLRM_OK;
  if (want < 0) {
    if (h->storage == GLRM_STORAGE_F32 && !GLRM_CACHED_F32_AUTO) return GLRM_OK;
    const double opp_bytes = (double)h->n * h->kp * 8;
    if (opp_bytes <= 32.0 * 1024 * 1024 || (double)h->sig.nnz_rows < 1e8) return GLRM_OK;
  }
  h->cached_want = 1;
  h->cached_row = h->cached_variant = variant;
  h->cached_waves = waves;
  // longest row the sweep takes
  if (h->cached_variant == 2) {
    h->cached_maxlen = glrm_cached_reg_maxlen(h->G);
  } else {
    const int vpi = 64 / (h->kp * 8 / 16);
    const int64_t budget = want > 0 ? 160 * 1024 : 53 * 1024; // auto: three waves per CU
    h->cached_maxlen = budget / (h->kp * 8 + 12) / vpi * vpi;
  }
  return GLRM_OK;
}

// the launch parameter of the cached kernels for a longest row of `maxlen` observations: trips of the lane layout (variant 2, registers),
// vectors in LDS (variant 1)
int glrm_cached_cap(int variant, int G, int kp, int64_t maxlen) {
  if (variant == 2) {
    const int ng = 64 / G;
    return (int)((maxlen + ng - 1) / ng);
  }
  const int vpi = 64 / (kp * 8 / 16);
  return std::max(vpi, (int)((maxlen + vpi - 1) / vpi * vpi));
}

// An X half-step (never an evaluation) of the request.  seglist == nullptr: every local row (restricted to the request's row range, if it
// has one); otherwise the rows listed.  cap: glrm_class_plan::cap of the row plan
int glrm_run_cached(glrm_handle* h, const glrm_step& step, const int32_t* seglist, int64_t nlist, int cap, hipStream_t st) {
  const int loss = step.loss;
  CachedArgs a{};
  glrm_fill_side(a, h, step);
  a.cap = cap;
  a.seg_lo = 0;
  a.seg_hi = h->side[GLRM_ROWS].nseg;
  if (seglist) {
    a.seglist = seglist;
    a.nseg = nlist;
    if (step.ranged()) { a.seg_lo = step.row_begin; a.seg_hi = step.row_end; }
    if (a.nseg <= 0 || a.seg_hi <= a.seg_lo) return GLRM_OK;
  } else if (step.ranged()) {
    glrm_apply_row_range(a, step);
    if (a.nseg <= 0) return GLRM_OK;
  }
  if (h->storage == GLRM_STORAGE_F32) { // the float instantiations live in a unit of their own
    const int rc = glrm_launch_cached_f32(a, h->G, loss, st, h);
    if (rc) return rc;
    HIPCK(hipGetLastError());
    return GLRM_OK;
  }
  // layouts (4, 8) and (8, 8) only (glrm_setup_cached); register variant (cached_row == 2) or LDS variant
  auto by_layout = [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    auto by_loss = [&](auto LOSS) {
      constexpr int L = decltype(LOSS)::value;
      if (a.vecreg) return h->cached_row == 2 ? launch_reg_inst<G, R, L, true>(a, st, h) : launch_inst<G, R, L, true>(a, st);
      return h->cached_row == 2 ? launch_reg_inst<G, R, L, false>(a, st, h) : launch_inst<G, R, L, false>(a, st);
    };
    return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
  };
  const int rc = glrm_dispatch_layout<32>(h->G, 8, by_layout, [&] { return by_layout(glrm_const<8>{}, glrm_const<8>{}); });
  if (rc) return rc;
  HIPCK(hipGetLastError());
  return GLRM_OK;
}
