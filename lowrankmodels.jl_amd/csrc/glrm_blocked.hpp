// glrm_blocked.hpp -- the launch side of the phase-aligned gather passes (glrm_blocked.hip has the family's story): launch constants, the
// slice a launch covers, and the ladder from run-time layout / loss variant to tiled_col_pass_kernel<..., L2 = true, false, ST>.  Templates
// over the storage type ST (include/glrm_hip_storage.h), the way glrm_sweep.hpp / glrm_cached.hpp have it: glrm_blocked.hip instantiates
// ST = double, glrm_blocked_f32.hip ST = float.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include <chrono>
#include <thread>

#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_tiled.hpp"

namespace glrm {

// Waves per workgroup.  ONE: the finest grain the dispatcher can spread over the CUs and retire -- C4 Y half-step, same box, with the
// half-residency launch slices below: 138.5 (4 waves) / 134.9 (2) / 129.6 ms (1); at full-residency slices 150.7 / 146.3 / 144.4
// (profiles/r03_c4_blocked_knobs.txt).  Changes no sum (a lane group owns a segment whatever workgroup it sits in).
constexpr int BNW = 1;                                                     // waves per workgroup
// GLRM_HIP_BLOCKED_GATE: phase gate of the passes in rows (tiled_pass, L2 = true), 0 = off.  Off is NOT the kernel of round 6: the gated
// loop is compiled in either way (134 instead of 118 VGPRs and 3 waves per SIMD when it was built), and C4's Y half-step ran 134.1 ms with
// the gate off against 129.6 on the round-6 kernel and 119.2 at the default (profiles/r07_c4_ab.txt).  Since the 32-bit gather offsets the
// rank-64 QuadLoss gradient kernel is built for 128 VGPRs and 4 waves per SIMD again, gate included (pass_waves_per_simd, glrm_tiled.hpp).
// The default was 8 192 rows (round 7: the 4 MB of an XCD's L2 at rank 64, chosen when both passes ran 3 waves per SIMD).  With both passes
// at 4 waves per SIMD and 16 384 columns per launch the optimum sits lower -- C4 Y half-step at 4 096 / 5 120 / 5 632 / 6 144 / 6 656 /
// 7 168 / 8 192 rows: 109.7 / 107.9 / 108.3 / 108.9 / 109.4 / 110.0 / 110.9 ms (profiles/r14_c4_ab.txt).  Changes no sum.
constexpr int BLOCKED_GATE_DEFAULT = 5120;
// The float kernels' own default (glrm_options.storage = 1, glrm_blocked_f32.hip).  A row of the opposing factor is half the bytes, so the
// window of rows the groups in flight may spread over before they fall out of the L2 is at least twice the fp64 one -- C4 Y half-step of an
// f32 handle at 5 120 / 8 192 / 10 240 / 16 384 / 24 576 / 32 768 / 65 536 rows: 81.6 / 72.2 / 70.3 / 68.4 / 68.8 / 69.8 / 71.2 ms, round to round
// within 0.2 ms (profiles/storage_f32_blocked_c4.json, tests/perf/bench_storage_blocked.py --gates).  Changes no sum.
constexpr int BLOCKED_GATE_DEFAULT_F32 = 16384;

// segments one launch may cover: what the chip holds at once (every group of the launch then starts its walk together)
template <typename K>
static int64_t slice_capacity(K kernel, int device, int spb) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, BNW * 64, 0) != hipSuccess || nb < 1) { (void)hipGetLastError(); nb = 1; }
  hipDeviceProp_t prop;
  int cus = 256;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  const int64_t cap = (int64_t)nb * cus * spb;
  // percent of the residency one launch covers.  Half: the next launch's workgroups fill the CUs the current one's stragglers have left
  // (launches of one stream overlap at their tails), which a slice of exactly the residency cannot do -- C4 Y half-step 143.2 -> 138.4 ms
  // with four-wave workgroups (25 / 33 / 66 / 100 / 200 %: 149.0 / 148.1 / 141.6 / 143.2 / 144.1), and with one-wave workgroups
  // 25 / 33 / 40 / 50 / 60 / 75 / 100 %: 139.7 / 137.0 / 135.6 / 131.0 / 133.0 / 136.9 / 144.4 (profiles/r03_c4_blocked_knobs.txt).
  // With the gradient pass at 4 waves per SIMD (16 384 columns per launch in both passes) 40 / 50 / 60 / 75 %: 116.1 / 110.8 / 117.2 /
  // 119.7 ms (profiles/r13_c4_ab.txt): half stays.  Changes no sum.
  const int pct = knob(Knob::BLOCKED_FILL);
  return std::max<int64_t>(spb, cap * pct / 100 / spb * spb);
}

template <int G, int R, int LOSS, bool GRAD, class ST>
static int launch_blocked_inst(glrm_handle* h, TiledArgs a, int side, glrm_arrivals* arr, const std::vector<int>& sup_order) {
  constexpr int KP = G * R, T = glrm_tile_rows(KP), SPB = BNW * (64 / G);
  auto kernel = tiled_col_pass_kernel<G, R, BNW, T, LOSS, GRAD, true, false, ST>;
  // per handle, view and pass kind: the row passes (LOSS_PER_OBS* instantiations of a heterogeneous model) and the column passes
  // (LOSS_SEGMENT*) of one handle are different kernels with their own occupancy; the CU count is the handle's device's, the fill
  // percentage the environment's at the handle's first sweep
  int64_t& cap_slot = h->side[side].blocked_cap[GRAD ? 0 : 1];
  if (cap_slot == 0) cap_slot = slice_capacity(kernel, h->device, SPB);
  const int64_t cap = cap_slot;
  // phase gate in rows of the opposing factor (tiled_pass, L2 = true): read at every pass, so that one handle can be timed under several
  // settings.  Changes no sum.
  a.gate = std::max(0, knob_or(Knob::BLOCKED_GATE, sizeof(ST) == 4 ? BLOCKED_GATE_DEFAULT_F32 : BLOCKED_GATE_DEFAULT));
  const int64_t nseg = a.npass > 0 ? a.npass : a.nseg;
  // equal slices: ceil(nseg / cap) launches per super-tile, all of the same size (a last slice of a few percent of the others is a launch
  // that cannot fill the chip)
  const int64_t nslices = (nseg + cap - 1) / cap;
  const int64_t per = nslices > 0 ? ((nseg + nslices - 1) / nslices + SPB - 1) / SPB * SPB : cap;
  if (!knob(Knob::BLOCKED_SUPPOS)) a.suppos = nullptr; // (the per-pass drop: same bits)
  // glrm_hip_step_y_arrival: the gradient pass of the column view walks the super-tiles in the order their rows of X arrive, each behind
  // the events of the blocks it touches (arr and sup_order, from glrm_run_blocked; arr == nullptr: X is complete); the partial sums are
  // per (segment, super-tile) and col_reduce adds them in super-tile order, so the launch order changes no bit
  const bool ordered = GRAD && arr;
  const int64_t rows_per_sup = (int64_t)a.tiles_per_sup * T;
  auto launch_sup = [&](int sup) -> int { // one super-tile: behind the events of the blocks it touches (ordered), slice by slice
    if (ordered) {
      const int rcw = glrm_arrival_wait(h, *arr, sup * rows_per_sup, std::min<int64_t>((sup + 1) * rows_per_sup, a.n_other));
      if (rcw) return rcw;
    }
    for (int64_t s0 = 0; s0 < nseg; s0 += per) {
      a.sup_fixed = sup;
      a.seg_begin = s0;
      a.nseg_slice = std::min(per, nseg - s0);
      hipLaunchKernelGGL(kernel, dim3((unsigned)((a.nseg_slice + SPB - 1) / SPB)), dim3(BNW * 64), 0, h->stream, a);
    }
    return GLRM_OK;
  };
  std::vector<int> pend;
  if (ordered) pend = sup_order;
  else for (int si = 0; si < a.nsup; ++si) pend.push_back(si);
  if (ordered && !h->arrival_static && knob(Knob::ARRIVAL_DYNAMIC)) {
    // TRUE arrival order.  The fixed order above is the order blocks arrive in when every peer keeps pace; behind a lagging peer the
    // in-order stream would stand in front of its block while super-tiles further down the list are ready.  So the host enqueues a
    // super-tile only once the events of ALL its blocks have fired (hipEventQuery), the ready ones in list order, and polls for the
    // rest: the stream never stands in a wait while work is ready.  An event that cannot be queried (or 5 s without any progress) hands
    // the remaining super-tiles -- and every later call on this handle -- to the in-stream waits below.  Which order the super-tiles run in changes no bit.
    std::vector<char> fired((size_t)arr->n, 0);
    bool unknown = false;
    auto ready = [&](int sup) {
      const int64_t lo = sup * rows_per_sup, hi = std::min<int64_t>((sup + 1) * rows_per_sup, a.n_other);
      for (int b = 0; b < arr->n; ++b) {
        const glrm_arrival& blk = arr->blocks[b];
        if (fired[b] || !blk.event || blk.end <= lo || blk.begin >= hi) continue;
        const hipError_t q = hipEventQuery((hipEvent_t)blk.event);
        if (q == hipSuccess) { fired[b] = 1; continue; }
        (void)hipGetLastError();
        if (q != hipErrorNotReady) unknown = true;
        return false;
      }
      return true;
    };
    auto t_progress = std::chrono::steady_clock::now();
    // the host polls where the stream used to wait: with glrm_options.profile the time in which NO super-tile was ready is booked as exposed
    // exchange time (glrm_kernel_stats.ms_wait_y, ADVICE r5: in true arrival order the in-stream waits are ~0 and this time was counted nowhere).
    // An upper bound on what the device stood idle for: super-tiles enqueued earlier may still be running while the host finds nothing ready.
    double idle_s = 0.0;
    while (!pend.empty() && !unknown) {
      bool progressed = false;
      for (size_t i = 0; i < pend.size() && !unknown;) {
        if (!ready(pend[i])) { ++i; continue; }
        const int rcl = launch_sup(pend[i]);
        if (rcl) return rcl;
        pend.erase(pend.begin() + (long)i);
        progressed = true;
      }
      const auto now = std::chrono::steady_clock::now();
      if (progressed) t_progress = now;
      else if (std::chrono::duration<double>(now - t_progress).count() > 5.0) break;
      else {
        std::this_thread::sleep_for(std::chrono::microseconds(20));
        idle_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - now).count();
      }
    }
    if (h->profile) h->ms_wait += idle_s * 1e3;
    if (!pend.empty()) h->arrival_static = true; // gave up: this handle keeps to the in-stream waits (no 5 s stall per iteration)
  }
  for (int sup : pend) {
    const int rcl = launch_sup(sup);
    if (rcl) return rcl;
  }
  HIPCK(hipGetLastError());
  return GLRM_OK;
}


template <class ST>
static int launch_blocked_st(glrm_handle* h, int loss, bool grad, const TiledArgs& a, int side, glrm_arrivals* arr, const std::vector<int>& sup_order) {
  auto by_layout = [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    auto by_loss = [&](auto LOSS) {
      constexpr int L = decltype(LOSS)::value;
      return grad ? launch_blocked_inst<G, R, L, true, ST>(h, a, side, arr, sup_order) : launch_blocked_inst<G, R, L, false, ST>(h, a, side, arr, sup_order);
    };
    return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
  };
  return glrm_dispatch_layout<8, 16, 32, 64, 128>(h->G, h->R, by_layout,
                                                  [&] { return fail(GLRM_ERR_UNSUPPORTED, "no phase-aligned pass kernel for lane layout G=%d R=%d", h->G, h->R); });
}

// reduce (stage = 0) / decide (stage = 1) of a float handle's passes: col_reduce_kernel / col_decide_kernel<G, R, false, float>
template <class ST>
static void launch_col_small_st(int kp, int stage, const TiledArgs& a, hipStream_t st) {
  auto by_layout = [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    const unsigned gx = (unsigned)((a.nseg + 4 * (64 / G) - 1) / (4 * (64 / G)));
    if (stage == 0) hipLaunchKernelGGL((col_reduce_kernel<G, R, false, ST>), dim3(gx), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((col_decide_kernel<G, R, false, ST>), dim3(gx), dim3(256), 0, st, a);
    return GLRM_OK;
  };
  glrm_dispatch_layout<8, 16, 32, 64>(glrm_layout_g(kp), glrm_layout_r(kp), by_layout, [&] { return by_layout(glrm_const<16>{}, glrm_const<8>{}); });
}

} // namespace glrm
