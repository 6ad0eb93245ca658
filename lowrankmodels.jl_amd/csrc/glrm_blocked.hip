// glrm_blocked.hip -- phase-aligned gather passes: the sweep family for problems whose opposing factor is far larger than the 4 MB
// L2 of an XCD and whose segments meet too few observations per LDS tile for the tiled sweeps (BASELINE config 4: 10M x 100k,
// rank 64, 100 observations per row).
//
// Why.  The one-kernel gather sweep (glrm_hip.hip) fetches one k-vector per observation from wherever the opposing factor lives:
// measured 6.5 TB/s from HBM (X, 5.1 GB) and 8.2 TB/s from the Infinity Cache (Y, 51 MB) -- the ceilings of random 512-byte reads at
// those levels (profiles/r02_ubench_gather.txt).  The same reads served by the L2 of the XCD run at ~30 TB/s.  The index lists are
// sorted, so a lane group that owns a segment walks the opposing factor front to back; if every group in flight starts at the same
// time and works at the same rate, all of them read the same ~2 MB window of the factor at any moment and that window stays in L2.
//
// How.  The pass structure of the LDS-tiled column sweep (glrm_tiled.hpp: pass over one super-tile, partials per (segment,
// super-tile), reduce in super-tile order, trial passes, decide) with the LDS tile taken out (tiled_pass<..., L2 = true>):
//   * a lane group (G lanes) owns one segment, its factor vector and gradient live in registers, its observations are consumed in
//     list order (the reference's summation order);
//   * one launch = one super-tile x one SLICE of the segments, the slice being what the chip holds at once (occupancy x CUs), so
//     all groups of a launch start together; launches are issued super-tile by super-tile;
//   * a super-tile is ~128 MB of the opposing factor (64 L2 windows): short enough that the groups have not drifted apart by the
//     end of it, long enough that the partial sums (k + 2 doubles per segment and super-tile) are a few percent of the traffic.
//     Its size is a function of (number of opposing vectors, kp) only, so the summation order does not depend on the sharding.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include <chrono>
#include <thread>

#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_tiled.hpp"

using namespace glrm;

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

// suppos[seg * nsup + sup] = lower_bound_idx(segment seg's list, first row of super-tile sup) - ptr[seg]: the pass kernel's own search, so
// that lists ordered by tile only get exactly the position the kernel would find.  *too_long is set where a segment does not fit int32.
static __global__ void __launch_bounds__(256) suppos_kernel(const int64_t* ptr, const int32_t* idx, int64_t nseg, int nsup, int64_t rows_per_sup,
                                                            int32_t* suppos, unsigned int* too_long) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nseg * nsup) return;
  const int64_t seg = t / nsup, b = ptr[seg], e = ptr[seg + 1];
  const int sup = (int)(t - seg * nsup);
  if (e - b > 0x7fffffff) { *too_long = 1; return; }
  suppos[t] = (int32_t)(lower_bound_idx<1>(idx, b, e, sup * rows_per_sup) - b);
}

// Start table of one side (PassBuffers::suppos), built once: Omega never changes for the life of a handle, and every launch of the passes
// began with the same ~14 dependent loads per lane group (624 launches per C4 iteration), which also let the groups of a launch start their
// walks microseconds apart.  GLRM_HIP_BLOCKED_SUPPOS (read here and at every pass): 0 the kernels search, 1 (default) the table where it
// takes at most 1/16 of the view's list bytes (C4 columns: 15.6 MB beside 12 GB), 2 the table whatever its size (tests on tiny shapes).
// Measured, C4, same box (profiles/r09_c4_ab.txt, r09_c4_launch_split_*.md): every launch 5-6 us shorter (full super-tile 176.9 -> 170.6 us,
// the last one 38.8 -> 33.9 us), Y half-step 118.0 -> 114.1 ms, iteration 192.9 -> 188.8 ms; the L2 hit rate hardly moves (0.29 -> 0.29 / 0.30
// -> 0.31).  Changes no sum.
static int build_suppos(glrm_handle* h, int side) {
  const glrm_handle::Side& v = h->side[side];
  glrm_handle::PassBuffers& b = h->side[side].pass;
  const int mode = env_int("GLRM_HIP_BLOCKED_SUPPOS", 1);
  const int64_t nseg = v.nseg, nnz = v.nnz, cells = nseg * b.nsup;
  const bool fits = (double)cells * 4.0 * 16.0 <= 12.0 * (double)nnz;
  const bool build = mode != 0 && cells > 0 && (fits || mode >= 2);
  if (build) {
    unsigned int too_long = 0;
    if (const int rc = h->mem.alloc(&b.suppos, (size_t)cells)) return rc;
    HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
    hipLaunchKernelGGL(suppos_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->stream, v.ptr, v.idx, nseg, b.nsup, (int64_t)b.tiles_per_sup * glrm_tile_rows(h->kp), b.suppos, h->nactive);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(&too_long, h->nactive, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    if (too_long) return fail(GLRM_ERR_UNSUPPORTED, "phase-aligned passes: a %s holds 2^31 observations or more", side == GLRM_ROWS ? "row" : "column");
  }
  if (env_int("GLRM_HIP_BLOCKED_TRACE", 0))
    fprintf(stderr, "[glrm blocked] %s view: %d super-tiles x %lld segments, start table %s (%.1f MB, lists %.1f MB)\n", side == GLRM_ROWS ? "row" : "column", b.nsup,
            (long long)nseg, build ? "built" : (mode == 0 ? "off: the passes search" : "over 1/16 of the lists: the passes search"), (double)cells * 4e-6, 12e-6 * (double)nnz);
  return GLRM_OK;
}

int glrm_setup_blocked(glrm_handle* h) {
  for (glrm_handle::Side& v : h->side) v.blocked = 0;
  const int want = env_int("GLRM_HIP_BLOCKED", h->tiled_opt == 1 ? 0 : -1); // -1 auto, else bit0 rows, bit1 columns (glrm_options.tiled = 1: gather sweeps only)
  if (want == 0 || h->kp < 8) return GLRM_OK;
  hipDeviceProp_t prop;
  HIPCK(hipGetDeviceProperties(&prop, h->device));
  const int64_t cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  const int T = glrm_tile_rows(h->kp);
  auto decide = [&](int side) -> bool {
    // Everything below is read from the WHOLE problem (m, n, k, glrm_signature, options), never from the shard, so that every
    // shard count runs the same family (the families differ in summation order).
    if (h->side[side].tiled) return false;         // the LDS-tiled sweep already owns this view
    if (side == GLRM_ROWS && h->cached_want) return false;                      // the short rows run on the cached sweep (glrm_cached.hip)
    if (!h->side[side].sorted) return false;   // a group must meet the opposing factor front to back
    const int64_t nnz = side == GLRM_ROWS ? h->sig.nnz_rows : h->sig.nnz_cols, nopp = h->side[side ^ 1].nglob;
    if (nnz <= 0) return false;
    if (want > 0) return ((want >> side) & 1) != 0;
    const double opp_bytes = (double)nopp * h->kp * 8;
    const int64_t nseg_glob = h->side[side].nglob;
    const double mean_len = (double)nnz / (double)nseg_glob;
    if (opp_bytes <= 32.0 * 1024 * 1024 || mean_len * (double)nseg_glob < 2e8) return false; // small factor: LDS tiles or plain L2 hits do better
    // observations that meet one vector of the opposing factor while the groups the chip holds (4 waves per SIMD) walk past it, per XCD
    const double resident = std::min<double>((double)nseg_glob, (double)cus * 16 * (64 / h->G));
    const double reuse = resident * mean_len / (double)nopp / 8.0;
    return reuse >= 2.0;
  };
  const bool blocked[2] = {decide(GLRM_ROWS), decide(GLRM_COLS)};
  int rc;
  auto buffers = [&](int side) { // super-tile geometry and pass buffers of one side
    const int64_t nopp = h->side[side ^ 1].nglob;
    const int64_t ntiles = (nopp + T - 1) / T;
    int64_t t = ((int64_t)128 * 1024 * 1024) / ((int64_t)T * h->kp * 8); // ~128 MB of the opposing factor per super-tile
    t = env_int("GLRM_HIP_BLOCKED_TPS", (int)(t < 1 ? 1 : t));
    // the passes address an observation's vector by a 32-bit byte offset from the first row of its super-tile (tiled_pass, L2 = true)
    if ((double)std::min<int64_t>(t * T, nopp) * h->kp * 8 >= 4294967296.0)
      return fail(GLRM_ERR_UNSUPPORTED, "phase-aligned passes: GLRM_HIP_BLOCKED_TPS=%lld makes a super-tile of 4 GiB or more of the opposing factor", (long long)t);
    h->side[side].pass.tiles_per_sup = (int)t;
    h->side[side].pass.nsup = (int)((ntiles + t - 1) / t);
    return glrm_alloc_pass_buffers(h, side);
  };
  for (int s = 0; s < 2; ++s) {
    if (!blocked[s]) continue;
    if ((rc = buffers(s))) return rc;
    if ((rc = build_suppos(h, s))) return rc;
    h->side[s].blocked = 1;
  }
  if (blocked[GLRM_COLS]) { // columns only: the diverted long columns
    HIPCK(hipMemsetAsync(h->side[GLRM_COLS].pass.active, 0, (size_t)(h->side[GLRM_COLS].nseg > 0 ? h->side[GLRM_COLS].nseg : 1) * 4, h->stream)); // diverted columns are never touched by col_reduce: they must read "not searching"
    // Skewed column lengths (power-law Omega; round 5).  A launch covers one super-tile x a slice of the columns, one lane group per column:
    // a column 100 x the mean keeps its group walking 100 x longer than the others of its launch, alone and latency bound (C4 recipe with
    // Zipf degrees: Y half-step 2.6 s against 0.13 s).  (i) The passes hand the columns out LONGEST FIRST, so the groups of a slice walk
    // lists of like length (and of like density: they also advance through the super-tile at the same rate).  (ii) Columns of at least
    // long_from = max(4 096, 2 x the whole problem's mean column length) observations leave the passes for the 8-wave gather sweep, which
    // spreads one column over 64 lane groups; it runs beside the passes on the side stream.  Both are functions of the column's own
    // length and of the whole problem's signature: shard-invariant.  Which slot a column sits in changes no sum; the diverted columns
    // add in the gather sweep's order (reported: glrm_sum_order.long_from).  Measured, C4 recipe with Zipf(0.5) degrees (995e6
    // observations, longest column 1.37e6 against a mean of 9 950; profiles/r05_c4_zipf_*): Y half-step 2 622 ms before, 207 ms with
    // long_from = 16 x mean, 168 / 154 / 151 ms with 8 / 4 / 2 x mean; the uniform recipe (no column reaches 2 x mean) is untouched.
    const int64_t mean_len = h->sig.nnz_cols / (h->n > 0 ? h->n : 1);
    h->blk_long_from = env_int("GLRM_HIP_BLOCKED_LONG_FROM", 0) > 0 ? env_int("GLRM_HIP_BLOCKED_LONG_FROM", 0)
                                                                     : std::max<int64_t>(4096, 2 * mean_len);
    if (h->side[GLRM_COLS].nseg > 0 && h->blk_long_from > 0) {
      std::vector<int64_t> ptr;
      std::vector<int32_t> shortl, longl;
      if ((rc = glrm_host_ptr(h, GLRM_COLS, ptr))) return rc;
      glrm_split_by_length(ptr, h->blk_long_from, shortl, longl);
      h->blk_nshort_c = (int64_t)shortl.size();
      if ((rc = glrm_upload_list(h, shortl, &h->blk_perm_c))) return rc;
      if ((rc = glrm_set_long_columns(h, longl))) return rc;
    }
  }
  return GLRM_OK;
}

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
  const int pct = env_int("GLRM_HIP_BLOCKED_FILL", 50);
  return std::max<int64_t>(spb, cap * pct / 100 / spb * spb);
}

template <int G, int R, int LOSS, bool GRAD>
static int launch_blocked_inst(glrm_handle* h, TiledArgs a, int side) {
  constexpr int KP = G * R, T = glrm_tile_rows(KP), SPB = BNW * (64 / G);
  auto kernel = tiled_col_pass_kernel<G, R, BNW, T, LOSS, GRAD, true>;
  // per handle, view and pass kind: the row passes (LOSS_PER_OBS* instantiations of a heterogeneous model) and the column passes
  // (LOSS_SEGMENT*) of one handle are different kernels with their own occupancy; the CU count is the handle's device's, the fill
  // percentage the environment's at the handle's first sweep
  int64_t& cap_slot = h->side[side].blocked_cap[GRAD ? 0 : 1];
  if (cap_slot == 0) cap_slot = slice_capacity(kernel, h->device, SPB);
  const int64_t cap = cap_slot;
  // phase gate in rows of the opposing factor (tiled_pass, L2 = true): read at every pass, so that one handle can be timed under several
  // settings.  Changes no sum.
  a.gate = std::max(0, env_int("GLRM_HIP_BLOCKED_GATE", BLOCKED_GATE_DEFAULT));
  const int64_t nseg = a.npass > 0 ? a.npass : a.nseg;
  // equal slices: ceil(nseg / cap) launches per super-tile, all of the same size (a last slice of a few percent of the others is a launch
  // that cannot fill the chip)
  const int64_t nslices = (nseg + cap - 1) / cap;
  const int64_t per = nslices > 0 ? ((nseg + nslices - 1) / nslices + SPB - 1) / SPB * SPB : cap;
  if (!env_int("GLRM_HIP_BLOCKED_SUPPOS", 1)) a.suppos = nullptr;
  // glrm_hip_step_y_arrival: the gradient pass of the column view walks the super-tiles in the order their rows of X arrive, each behind
  // the events of the blocks it touches (h->sup_order, glrm_run_blocked); the partial sums are per (segment, super-tile) and col_reduce
  // adds them in super-tile order, so the launch order changes no bit
  const bool ordered = GRAD && side == GLRM_COLS && h->n_arrival > 0 && (int)h->sup_order.size() == a.nsup;
  const int64_t rows_per_sup = (int64_t)a.tiles_per_sup * T;
  auto launch_sup = [&](int sup) -> int { // one super-tile: behind the events of the blocks it touches (ordered), slice by slice
    if (ordered) {
      const int rcw = glrm_arrival_wait(h, sup * rows_per_sup, std::min<int64_t>((sup + 1) * rows_per_sup, a.n_other));
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
  if (ordered) pend = h->sup_order;
  else for (int si = 0; si < a.nsup; ++si) pend.push_back(si);
  if (ordered && !h->arrival_static && env_int("GLRM_HIP_ARRIVAL_DYNAMIC", 1)) {
    // TRUE arrival order.  The fixed order above is the order blocks arrive in when every peer keeps pace; behind a lagging peer the
    // in-order stream would stand in front of its block while super-tiles further down the list are ready.  So the host enqueues a
    // super-tile only once the events of ALL its blocks have fired (hipEventQuery), the ready ones in list order, and polls for the
    // rest: the stream never stands in a wait while work is ready.  An event that cannot be queried (or 5 s without any progress) hands
    // the remaining super-tiles -- and every later call on this handle -- to the in-stream waits below.  Which order the super-tiles run in changes no bit.
    std::vector<char> fired((size_t)h->n_arrival, 0);
    bool unknown = false;
    auto ready = [&](int sup) {
      const int64_t lo = sup * rows_per_sup, hi = std::min<int64_t>((sup + 1) * rows_per_sup, a.n_other);
      for (int b = 0; b < h->n_arrival; ++b) {
        const glrm_arrival& blk = h->arrival[b];
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


static int launch_blocked(glrm_handle* h, int loss, bool grad, const TiledArgs& a, int side) {
  auto by_layout = [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    auto by_loss = [&](auto LOSS) {
      constexpr int L = decltype(LOSS)::value;
      return grad ? launch_blocked_inst<G, R, L, true>(h, a, side) : launch_blocked_inst<G, R, L, false>(h, a, side);
    };
    return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
  };
  return glrm_dispatch_layout<8, 16, 32, 64, 128>(h->G, h->R, by_layout,
                                                  [&] { return fail(GLRM_ERR_UNSUPPORTED, "no phase-aligned pass kernel for lane layout G=%d R=%d", h->G, h->R); });
}

int glrm_run_blocked(glrm_handle* h, int side, int loss, int loss_by_segment, double min_stepsize, int eval_only) {
  TiledArgs a{};
  glrm_fill_side(a, h, side, min_stepsize, eval_only);
  a.loss_by_segment = loss_by_segment;
  const bool range = side == GLRM_ROWS && h->rng_e >= 0; // glrm_hip_step_x_range: local rows [rng_b, rng_e)
  glrm_bind_pass_buffers(a, h, side, range ? h->rng_b : 0);
  if (side == GLRM_COLS && h->blk_perm_c) { // length-sorted slots; the columns at or above long_from run on the gather sweep (run_sweep, glrm_hip.hip)
    a.segperm = h->blk_perm_c;
    a.npass = h->blk_nshort_c;
    a.long_from = h->blk_long_from;
    if (a.npass == 0) { // every local column is diverted: nothing for the passes (npass = 0 would mean "all")
      HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
      return GLRM_OK;
    }
  }
  if (range) {
    glrm_apply_row_range(a, h->rng_b, h->rng_e);
    if (a.nseg <= 0) return GLRM_OK;
  }
  int rc;
  HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
  h->sup_order.clear();
  if (side == GLRM_COLS && h->n_arrival > 0 && !eval_only) {
    // a super-tile can run once the LAST (in the host's order) of the blocks it touches is there: sort the super-tiles by that position
    const int64_t rows_per_sup = (int64_t)a.tiles_per_sup * glrm_tile_rows(h->kp);
    std::vector<std::pair<int, int>> key((size_t)a.nsup);
    for (int sup = 0; sup < a.nsup; ++sup) {
      const int64_t lo = sup * rows_per_sup, hi = std::min<int64_t>((sup + 1) * rows_per_sup, a.n_other);
      int last = 0;
      for (int b = 0; b < h->n_arrival; ++b)
        if (h->arrival[b].begin < hi && h->arrival[b].end > lo && h->arrival[b].event) last = std::max(last, b + 1);
      key[sup] = {last, sup};
    }
    std::sort(key.begin(), key.end());
    for (auto& kv : key) h->sup_order.push_back(kv.second);
  }
  if ((rc = launch_blocked(h, loss, true, a, side))) return rc;  // gradient + loss partials, super-tile by super-tile
  glrm_launch_col_small(h->kp, 0, a, h->stream);                 // reduce in super-tile order, J_old, first trial point
  HIPCK(hipGetLastError());
  if (eval_only || a.fixed_alpha > 0.0) return GLRM_OK;
  return glrm_run_rounds(
      h, a, min_stepsize, glrm_act_lists{},
      [&](int, unsigned int, int32_t*) { return launch_blocked(h, loss, false, a, side); },  // loss partials at the trial points of the searching segments
      [&](const TiledArgs& d) { glrm_launch_col_small(h->kp, 1, d, h->stream); });           // accept / shrink / give up, next trial point
}
