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

#include "glrm_blocked.hpp"

using namespace glrm;

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
  const int mode = knob(Knob::BLOCKED_SUPPOS);
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
  if (knob(Knob::BLOCKED_TRACE))
    fprintf(stderr, "[glrm blocked] %s view: %d super-tiles x %lld segments, start table %s (%.1f MB, lists %.1f MB)\n", side == GLRM_ROWS ? "row" : "column", b.nsup,
            (long long)nseg, build ? "built" : (mode == 0 ? "off: the passes search" : "over 1/16 of the lists: the passes search"), (double)cells * 4e-6, 12e-6 * (double)nnz);
  return GLRM_OK;
}

int glrm_setup_blocked(glrm_handle* h) {
  for (glrm_handle::Side& v : h->side) v.blocked = 0;
  int want = knob_or(Knob::BLOCKED, h->tiled_opt == 1 ? 0 : -1); // -1 auto, else bit0 rows, bit1 columns (glrm_options.tiled = 1: gather sweeps only)
  const bool f32 = h->storage == GLRM_STORAGE_F32;
  if (f32) {
    // A float handle takes the family only where GLRM_HIP_BLOCKED asks for it (tiled = 1 handles included: the variable outranks the option
    // in both storages) until the auto rule is adopted: GLRM_BLOCKED_F32_AUTO.  Its finalize branch runs no glrm_setup_tiled, which is
    // where an fp64 handle learns whether its lists are in tile order.
    if (want < 0 && !GLRM_BLOCKED_F32_AUTO) want = 0;
    h->side[GLRM_ROWS].sorted = !h->sig.rows_unordered;
    h->side[GLRM_COLS].sorted = !h->sig.cols_unordered;
  }
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
    const double opp_bytes = (double)nopp * h->kp * 8; // (the fp64 rule on the same (nopp, kp, nnz), counted in 8-byte elements, in both storages)
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
    t = knob_or(Knob::BLOCKED_TPS, (int)(t < 1 ? 1 : t));
    // the passes address an observation's vector by a 32-bit byte offset from the first row of its super-tile (tiled_pass, L2 = true)
    if ((double)std::min<int64_t>(t * T, nopp) * h->kp * (f32 ? 4 : 8) >= 4294967296.0) // (the geometry above is the 8-byte one in both storages: one problem, one order)
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
    h->blk_long_from = (int64_t)knob_positive(Knob::BLOCKED_LONG_FROM, (double)std::max<int64_t>(4096, 2 * mean_len));
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

int glrm_run_blocked(glrm_handle* h, const glrm_step& step) {
  const int side = step.side, loss = step.loss;
  TiledArgs a{};
  glrm_fill_side(a, h, step);
  a.loss_by_segment = step.loss_by_segment;
  glrm_bind_pass_buffers(a, h, side, step.ranged() ? step.row_begin : 0);
  if (side == GLRM_COLS && h->blk_perm_c) { // length-sorted slots; the columns at or above long_from run on the gather sweep (run_sweep, glrm_hip.hip)
    a.segperm = h->blk_perm_c;
    a.npass = h->blk_nshort_c;
    a.long_from = h->blk_long_from;
    if (a.npass == 0) { // every local column is diverted: nothing for the passes (npass = 0 would mean "all")
      HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
      return GLRM_OK;
    }
  }
  if (step.ranged()) {
    glrm_apply_row_range(a, step);
    if (a.nseg <= 0) return GLRM_OK;
  }
  int rc;
  HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
  // glrm_hip_step_y_arrival: the order in which the gradient pass walks the super-tiles (launch_blocked_inst); empty without arriving blocks
  glrm_arrivals* const arr = step.arrivals;
  std::vector<int> sup_order;
  if (arr) {
    // a super-tile can run once the LAST (in the host's order) of the blocks it touches is there: sort the super-tiles by that position
    const int64_t rows_per_sup = (int64_t)a.tiles_per_sup * glrm_tile_rows(h->kp);
    std::vector<std::pair<int, int>> key((size_t)a.nsup);
    for (int sup = 0; sup < a.nsup; ++sup) {
      const int64_t lo = sup * rows_per_sup, hi = std::min<int64_t>((sup + 1) * rows_per_sup, a.n_other);
      int last = 0;
      for (int b = 0; b < arr->n; ++b)
        if (arr->blocks[b].begin < hi && arr->blocks[b].end > lo && arr->blocks[b].event) last = std::max(last, b + 1);
      key[sup] = {last, sup};
    }
    std::sort(key.begin(), key.end());
    for (auto& kv : key) sup_order.push_back(kv.second);
  }
  // a float handle (glrm_options.storage = 1) takes the ST = float kernels of glrm_blocked_f32.hip: the same launches over the same buffers
  const bool f32 = h->storage == GLRM_STORAGE_F32;
  auto pass = [&](bool grad) { return f32 ? glrm_launch_blocked_f32(h, loss, grad, a, side, arr, sup_order) : launch_blocked_st<double>(h, loss, grad, a, side, arr, sup_order); };
  auto small = [&](int stage, const TiledArgs& d) { f32 ? glrm_launch_col_small_f32(h->kp, stage, d, h->stream) : glrm_launch_col_small(h->kp, stage, d, h->stream); };
  if ((rc = pass(true))) return rc;  // gradient + loss partials, super-tile by super-tile
  small(0, a);                       // reduce in super-tile order, J_old, first trial point
  HIPCK(hipGetLastError());
  if (step.eval_only || step.fixed()) return GLRM_OK;
  return glrm_run_rounds(
      h, a, step.min_stepsize, glrm_act_lists{},
      [&](int, unsigned int, int32_t*) { return pass(false); },  // loss partials at the trial points of the searching segments
      [&](const TiledArgs& d) { small(1, d); });                 // accept / shrink / give up, next trial point
}
