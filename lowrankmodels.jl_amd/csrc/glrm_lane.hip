// glrm_lane.hip -- host side + instantiations of the lane-per-segment LDS-tiled passes (kernels and rationale: glrm_lane.hpp).
//
// A side (rows / columns) of a handle runs this family instead of the four-lane tiled kernels when glrm_setup_tiled chose the LDS tiles for it
// and (all functions of the WHOLE problem's signature and of (k, losses, options), never of the shard -- the two families add in different
// orders): padded rank 32; one loss descriptor per segment or per model, or -- rows of a model with a loss per column -- at most 256 distinct
// descriptors in the model; at most 2e9 (columns) / 6e9 (rows) observations in the view (the SELL copy is 12 B x its padding per observation on
// top of the lists; GLRM_HIP_LANE_MAX_NNZ_M / _ROWS_M).
// The half-step is the pass machinery of the tiled column sweep on BOTH sides: gradient pass -> col_reduce (J_old, first trial point, list of
// searching segments) -> rounds of (trial pass, col_decide); rows run it with ONE super-tile (nothing is re-added).  The first trial of a
// half-step walks the SELL layout over the full grid (idle segments masked); later rounds run whichever of the kernel's three forms fits
// the fraction of segments that still searches (glrm_run_lane): the same sums in the same order, so which form ran changes no bit.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_lane.hpp"

using namespace glrm;

namespace {

constexpr int LANE_NW = 8; // 8 waves x 64 segments per workgroup, 256 VGPRs per lane

template <int LOSS, bool GRAD, int FORM, bool COMPACT = false>
int launch_lane_inst(const TiledArgs& a, const LaneArgs& la, int64_t nblocks, hipStream_t st) {
  constexpr int KP = 32, T = glrm_tile_rows(KP);
  const int LDSB = T * KP * 8 + (loss_mode(LOSS) == 2 ? a.n_udesc * 32 : 0);
  auto k = lane_pass_kernel<KP, LANE_NW, T, LOSS, GRAD, FORM, COMPACT>;
  HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDSB)); // (per device: a process may drive several)
  const unsigned gx = (unsigned)((nblocks + LANE_NW - 1) / LANE_NW);
  if (gx == 0) return GLRM_OK;
  hipLaunchKernelGGL(k, dim3(gx, (unsigned)(a.nsup_launch > 0 ? a.nsup_launch : a.nsup)), dim3(LANE_NW * 64), LDSB, st, a, la);
  return GLRM_OK;
}

// The family instantiates the scalar-loss variants; its compact stream (sides without a descriptor id in the offset word) the per-segment ones.
template <bool GRAD, int FORM>
int launch_lane_loss(int loss, const TiledArgs& a, const LaneArgs& la, int64_t nblocks, hipStream_t st) {
  if constexpr (FORM == 0 || (FORM == 2 && !GRAD)) {
    if (la.off16) {
      if (FORM == 2 && !la.sval) return fail(GLRM_ERR_UNSUPPORTED, "lane-per-segment passes: the gathered form needs the step bases of the compact stream");
      return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG>(
          loss, [&](auto LOSS) { return launch_lane_inst<decltype(LOSS)::value, GRAD, FORM, true>(a, la, nblocks, st); },
          [&] { return fail(GLRM_ERR_UNSUPPORTED, "lane-per-segment passes, compact stream: no kernel for loss variant %d", loss); });
    }
  }
  return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS, LOSS_PER_OBS_NOTRIG>(
      loss, [&](auto LOSS) { return launch_lane_inst<decltype(LOSS)::value, GRAD, FORM>(a, la, nblocks, st); },
      [&] { return fail(GLRM_ERR_UNSUPPORTED, "lane-per-segment passes: no kernel for loss variant %d", loss); });
}

// a wave per (segment, super-tile), no tile: the tail rounds (glrm_lane.hpp: lane_tail_kernel)
constexpr int LANE_TAIL_CAP = 2048; // terms it parks in LDS at a time
int launch_lane_tail(int loss, const TiledArgs& a, const int32_t* list, int64_t nact, hipStream_t st) {
  constexpr int KP = 32, T = glrm_tile_rows(KP);
  nact *= a.nsup; // waves of the round
  const unsigned gx = (unsigned)((nact + 1) / 2);
  return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS, LOSS_PER_OBS_NOTRIG>(
      loss,
      [&](auto LOSS) {
        hipLaunchKernelGGL((lane_tail_kernel<KP, decltype(LOSS)::value, LANE_TAIL_CAP>), dim3(gx), dim3(128), 0, st, a, list, nact, T);
        return GLRM_OK;
      },
      [&] { return fail(GLRM_ERR_UNSUPPORTED, "lane-per-segment passes: no tail kernel for loss variant %d", loss); });
}

// the small kernels of the pass machinery in the two-lane layout the family's sums are reported in
void launch_small(int stage, const TiledArgs& a, hipStream_t st) {
  constexpr int G = 2, R = 16;
  const unsigned gx = (unsigned)((a.nseg + 4 * (64 / G) - 1) / (4 * (64 / G)));
  if (stage == 0 && a.vecreg) hipLaunchKernelGGL((col_reduce_kernel<G, R, true>), dim3(gx), dim3(256), 0, st, a);
  else if (stage == 0) hipLaunchKernelGGL((col_reduce_kernel<G, R>), dim3(gx), dim3(256), 0, st, a);
  else if (a.vecreg) hipLaunchKernelGGL((col_decide_kernel<G, R, true>), dim3(gx), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((col_decide_kernel<G, R>), dim3(gx), dim3(256), 0, st, a);
}

} // namespace

// (a loss per observation -- rows of a model with a loss per column -- needs the one-byte descriptor ids: at most 256 distinct descriptors)
bool glrm_lane_loss_ok(const glrm_handle* h, int loss) {
  return loss == LOSS_QUAD_UNIFORM || loss == LOSS_SEGMENT || loss == LOSS_SEGMENT_NOTRIG ||
         ((loss == LOSS_PER_OBS || loss == LOSS_PER_OBS_NOTRIG) && h->rowdescid && h->n_udesc > 0 && h->n_udesc <= 256);
}

// at most 256 distinct loss descriptors in the model (what TiledArgs::descid can number)?  Host-side, from the descriptors alone.
bool glrm_lane_few_descriptors(const glrm_handle* h) {
  std::vector<glrm_loss> uniq;
  for (const glrm_loss& l : h->losses_h) {
    size_t u = 0;
    for (; u < uniq.size(); ++u)
      if (uniq[u].kind == l.kind && uniq[u].dim == l.dim && uniq[u].scale == l.scale && uniq[u].p0 == l.p0 && uniq[u].p1 == l.p1) break;
    if (u == uniq.size()) {
      if (uniq.size() == 256) return false;
      uniq.push_back(l);
    }
  }
  return true;
}

// what does not depend on the buffers: padded rank, losses, view size -- all of the WHOLE problem
static bool lane_wants(const glrm_handle* h, int side, int cmode) {
  const int want = knob(Knob::LANE); // bit0 rows, bit1 columns
  if (!((want >> side) & 1) || h->kp != 32 || h->multi || h->dense || h->sum_order_opt) return false;
  // a loss per column: the row view meets a descriptor per observation -- through one-byte ids, i.e. at most 256 distinct descriptors.
  // Default since session r6_33 (GLRM_HIP_LANE_PER_OBS=0 keeps such rows on the four-lane kernels): with the trial rounds read out of the
  // SELL layout (glrm_run_lane) the C5 recipe's X half-step is 42.5 against 46.6 ms at 1M rows and 194 against 215 ms at its stated size.
  // (Session r6_19/20, rounds on the CSR form: 64.4 against 45.8 ms -- opt-in then.)
  if (side == GLRM_ROWS && h->n_losses > 1 && (!knob(Knob::UDESC) || !knob(Knob::LANE_PER_OBS) || !glrm_lane_few_descriptors(h))) return false;
  // the SELL copy is 12 B x its padding per observation on top of the lists: a memory policy per view (rows: the copy REPLACES the kind-grouped
  // private row view of such models, and rows pad little; columns pad x 1.5-1.8).  C5 at its stated size: 5e9 observations per view
  // (columns beyond 2e9 observations: the COMPACT form of the stream -- 2-byte offsets, unpadded values, 11.5 instead of 21 B per observation at
  // x 1.76 padding; GLRM_HIP_LANE_COMPACT = 0 never, 1 every side it serves, 2 (default) views beyond 2e9 observations)
  const int64_t max_nnz = (int64_t)(side == GLRM_ROWS ? knob(Knob::LANE_MAX_NNZ_ROWS_M) : knob_or(Knob::LANE_MAX_NNZ_M, cmode ? 6000 : 2000)) * 1000000ll;
  return (side == GLRM_ROWS ? h->sig.nnz_rows : h->sig.nnz_cols) <= max_nnz;
}

// Set-up, once, before anything asks (glrm_setup_tiled): does the whole problem admit the family on a side (given that the side runs the LDS
// tiles), and does the side's stream take the compact form?  Functions of the whole problem (view size, losses, options) and the knobs.
void glrm_lane_decide(glrm_handle* h) {
  const int cmode = knob(Knob::LANE_COMPACT);
  for (int side = 0; side < 2; ++side) {
    glrm_handle::Side& v = h->side[side];
    v.lane_want = lane_wants(h, side, cmode);
    v.lane_compact = !(side == GLRM_ROWS && h->n_losses > 1) && (cmode == 1 || (cmode == 2 && (side == GLRM_ROWS ? h->sig.nnz_rows : h->sig.nnz_cols) > 2000000000ll)) &&
                     64 * (side == GLRM_ROWS ? h->sig.max_row_len : h->sig.max_col_len) < ((int64_t)1 << 31); // (a wave block's values are counted in 31 bits: LaneArgs::sval)
  }
}

// finalize, after glrm_setup_tiled has chosen the LDS tiles and built the slot permutations: decide the family per side and build its SELL layout
int glrm_setup_lane(glrm_handle* h) {
  for (glrm_handle::Side& v : h->side) v.lane = 0;
  int64_t gseg_max = 0;
  const int T = glrm_tile_rows(h->kp);
  hipStream_t st = h->stream;
  for (int side = 0; side < 2; ++side) {
    glrm_handle::Side& v = h->side[side];
    if (!v.lane_want) continue;
    if (side == GLRM_ROWS ? !(v.tiled && (h->tile_rounds & 1) && h->actlist && v.pass.part) : !v.tiled) continue;
    if (side == GLRM_ROWS && h->n_losses > 1 && !(h->rowdescid && h->n_udesc > 0)) continue;
    v.lane = 1;
    const int64_t nseg = v.nseg;
    const int64_t nslots = side == GLRM_ROWS ? nseg : (h->blk_nlong_c > 0 ? h->blk_nshort_c : nseg);
    const int64_t nother = h->side[side ^ 1].nglob;
    const int ntiles = (int)((nother + T - 1) / T);
    const int64_t nwb = (nslots + 63) / 64;
    v.lane_nwb = nwb;
    v.lane_ntiles = ntiles;
    if (nwb == 0 || ntiles == 0) continue;
    const int64_t ncell = nwb * ntiles;
    if (ncell > (int64_t)1 << 30) { v.lane = 0; continue; } // (cannot happen at shapes the LDS tiles are chosen for)
    const bool compact = v.lane_compact; // (a function of the whole problem, like the family itself: glrm_lane_decide)
    int64_t *cnt = nullptr, *scan = nullptr, *vcnt = nullptr;
    char* tmp = nullptr;
    DevArena scratch; // the counts and scans of this side's build
    int rc;
    if ((rc = scratch.alloc(&cnt, (size_t)ncell)) || (rc = scratch.alloc(&scan, (size_t)ncell)) || (compact && (rc = scratch.alloc(&vcnt, (size_t)ncell)))) return rc;
    hipLaunchKernelGGL(lane_count_kernel, dim3((unsigned)nwb), dim3(64), 0, st, v.ptr, v.idx, v.perm, nslots, T, ntiles, cnt, vcnt);
    size_t bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, cnt, scan, (int)ncell, st) != hipSuccess) return fail(GLRM_ERR_HIP, "scan (size query) failed");
    if ((rc = scratch.alloc(&tmp, bytes))) return rc;
    if (hipcub::DeviceScan::ExclusiveSum(tmp, bytes, cnt, scan, (int)ncell, st) != hipSuccess) return fail(GLRM_ERR_HIP, "scan failed");
    const int64_t nb = nwb * (ntiles + 1);
    if ((rc = h->mem.alloc(&v.lane_bptr, (size_t)nb))) return rc;
    hipLaunchKernelGGL(lane_bptr_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, scan, cnt, nwb, ntiles, v.lane_bptr);
    int64_t last[2] = {0, 0};
    if (hipMemcpyAsync(&last[0], scan + ncell - 1, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync(&last[1], cnt + ncell - 1, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return fail(GLRM_ERR_HIP, "lane layout: copy failed");
    const int64_t steps = last[0] + last[1];
    v.lane_steps = steps;
    const int64_t s1 = steps > 0 ? steps : 1;
    if (compact) {
      // values before every (wave block, tile): the same scan over the observation counts (the step scan's scratch serves again)
      if (hipcub::DeviceScan::ExclusiveSum(tmp, bytes, vcnt, scan, (int)ncell, st) != hipSuccess) return fail(GLRM_ERR_HIP, "scan failed");
      if ((rc = h->mem.alloc(&v.lane_vptr, (size_t)nb))) return rc;
      hipLaunchKernelGGL(lane_bptr_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, scan, vcnt, nwb, ntiles, v.lane_vptr);
      const int64_t nv = std::max<int64_t>(1, v.nnz);
      const bool ok = !h->mem.alloc(&v.lane_off16, (size_t)s1 * 64) && !h->mem.alloc(&v.lane_sval, (size_t)s1) && !h->mem.alloc(&v.lane_val, (size_t)nv);
      if (!ok) {
        // No room for the stream beside the lists: the side stays on the four-lane kernels.  (The only family choice that can depend on
        // the device rather than on the problem; glrm_hip_sum_order reports what runs, and the super-tile geometry is already fixed.)
        (void)hipGetLastError();
        h->mem.release(&v.lane_off16); h->mem.release(&v.lane_sval); h->mem.release(&v.lane_val); h->mem.release(&v.lane_vptr); h->mem.release(&v.lane_bptr);
        v.lane = 0;
        v.lane_steps = 0;
        fprintf(stderr, "[glrm lane] no device memory for the compact stream of the %s view (%.1f GB): the view stays on the four-lane LDS-tiled kernels\n", side == GLRM_ROWS ? "row" : "column",
                ((double)s1 * 128 + (double)nv * 8) / 1e9);
        continue;
      }
      hipLaunchKernelGGL(lane_fill_compact_kernel, dim3((unsigned)nwb), dim3(64), 0, st, v.ptr, v.idx, v.vals, v.perm, nslots, T, ntiles, v.lane_bptr, v.lane_vptr,
                         v.lane_off16, v.lane_sval, v.lane_val);
    } else {
      char oom[160];
      snprintf(oom, sizeof oom, "out of device memory for the lane-per-segment stream of the %s view (%lld steps of 64 entries)", side == GLRM_ROWS ? "row" : "column", (long long)steps);
      if ((rc = h->mem.alloc(&v.lane_off, (size_t)s1 * 64, oom)) || (rc = h->mem.alloc(&v.lane_val, (size_t)s1 * 64, oom))) return rc;
      hipLaunchKernelGGL(lane_fill_kernel, dim3((unsigned)nwb), dim3(64), 0, st, v.ptr, v.idx, v.vals, (side == GLRM_ROWS && h->n_losses > 1) ? h->rowdescid : nullptr, v.perm, nslots, T, ntiles,
                         h->kp * 8, v.lane_bptr, v.lane_off, v.lane_val);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(GLRM_ERR_HIP, "lane layout: build failed");
    scratch.free_all();
    if (v.perm) { // FORM 2 of the rounds finds a segment's slot through the inverse of the slot permutation
      if ((rc = h->mem.alloc(&v.lane_inv, (size_t)nseg))) return rc;
      HIPCK(hipMemsetAsync(v.lane_inv, 0xFF, (size_t)nseg * 4, st));
      hipLaunchKernelGGL(lane_inv_kernel, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, st, v.perm, nslots, v.lane_inv);
      HIPCK(hipGetLastError());
    }
    if (nseg > gseg_max) gseg_max = nseg;
    if (knob(Knob::LANE_TRACE))
      fprintf(stderr, "[glrm lane] %s view: %lld slots in %lld wave blocks x %d tiles, %lld steps of 64 = %.3f x the %lld observations%s\n", side == GLRM_ROWS ? "row" : "column",
              (long long)nslots, (long long)nwb, ntiles, (long long)steps, (double)steps * 64.0 / (double)std::max<int64_t>(1, v.nnz),
              (long long)v.nnz, compact ? " (compact stream: 2-byte offsets padded, values unpadded)" : "");
  }
  if (gseg_max > 0 && !h->lane_glist) { // the wave lists of the rounds (one set serves both sides: a half-step at a time)
    h->lane_gchunks = (gseg_max + LANE_CC - 1) / LANE_CC;
    h->lane_gcap = h->lane_gchunks * 16; // waves: a chunk holds at most 64 segments of a class
    int rc;
    if ((rc = h->mem.alloc(&h->lane_gcnt, (size_t)h->lane_gchunks)) || (rc = h->mem.alloc(&h->lane_gbase, (size_t)h->lane_gchunks)) || (rc = h->mem.alloc(&h->lane_gtotal, 1)) ||
        (rc = h->mem.alloc(&h->lane_glist, (size_t)h->lane_gcap * 64)))
      return rc;
  }
  return GLRM_OK;
}

// One half-step (or the evaluation pass of the column view) on the lane-per-segment passes.  `a` comes prepared by glrm_run_tiled: the side's
// views, factors, pass buffers, slot permutation and -- rows of a sub-range sweep -- everything offset to the range's first row.
int glrm_run_lane(glrm_handle* h, const glrm_step& step, const TiledArgs& a_in) {
  const int side = step.side, loss = step.loss;
  TiledArgs a = a_in;
  hipStream_t st = h->stream;
  LaneArgs la{};
  const glrm_handle::Side& v = h->side[side];
  la.bptr = v.lane_bptr; la.off = v.lane_off; la.val = v.lane_val;
  la.off16 = v.lane_off16; la.vptr = v.lane_vptr; la.sval = v.lane_sval;
  la.ntiles = v.lane_ntiles; la.nwb = v.lane_nwb;
  la.slot0 = 0;
  la.inv = v.lane_inv;
  la.glist = h->lane_glist;
  la.gwaves = 0;
  // does the SELL layout cover this launch?  It was built on the side's full slot space (slot permutation included); a row sub-range
  // (glrm_hip_step_x_range) is covered when the slots are the rows themselves: its wave blocks run with the lanes outside the range masked
  const bool sell_ok = !step.ranged() || v.perm == nullptr;
  if (step.ranged()) la.slot0 = step.row_begin;
  const int64_t nslots = a.npass > 0 ? a.npass : a.nseg;
  const int64_t blk_lo = la.slot0 / 64, blk_hi = (la.slot0 + nslots + 63) / 64;
  int rc;
  const glrm_act_lists lists = glrm_active_lists(h, side, a.nseg);
  HIPCK(hipMemsetAsync(h->nactive, 0, 4, st));
  a.actlist_out = lists.list[0];
  auto csr_args = [&](const TiledArgs& t) { // the CSR form numbers its slots from 0 over t.nseg (a compact list or a plain range)
    LaneArgs c = la;
    c.slot0 = 0;
    c.gwaves = 0;
    return c;
  };
  // gradient pass: under glrm_hip_step_y_arrival (columns) in runs of super-tiles, each behind the blocks of X it reads (announced order)
  auto grad = [&](int s0, int s1) {
    TiledArgs r = a;
    r.sup0 = s0;
    r.nsup_launch = s1 - s0;
    if (sell_ok) return launch_lane_loss<true, 0>(loss, r, la, blk_hi - blk_lo, st);
    r.npass = 0;
    return launch_lane_loss<true, 1>(loss, r, csr_args(r), (r.nseg + 63) / 64, st);
  };
  rc = side == GLRM_ROWS ? grad(0, a.nsup) : glrm_for_sup_runs_in_arrival_order(h, step.arrivals, a.nsup, (int64_t)a.tiles_per_sup * glrm_tile_rows(h->kp), grad); // (rows read Y: complete)
  if (rc) return rc;
  launch_small(0, a, st);
  HIPCK(hipGetLastError());
  if (step.eval_only) return GLRM_OK;
  const TiledArgs full = a;
  const bool gather = knob(Knob::LANE_ROUNDS) != 0 && sell_ok && h->lane_glist && la.bptr && h->side[side].lane_steps > 0 &&
                      full.nseg <= h->lane_gchunks * (int64_t)LANE_CC;
  // the round's trial pass in whichever form fits the fraction of segments that still searches; `list` holds them (nullptr without lists)
  auto trial = [&](int round, unsigned int nact, int32_t* list) -> int {
    TiledArgs t = full;
    const int trace = knob(Knob::LANE_TRACE);
    // Three forms of the trial pass, all adding the same terms in the same order (tests/test_gpu_families.py forces each of them on every
    // round).  FORM 0 walks the SELL layout over the full grid (idle segments masked): the cost of a whole pass whatever the fraction that
    // searches -- from 70 % up (sweep at C5's stated size, session r6_50: 55 / 70 / 85 % = 344.5 / 341.6 / 340.5 ms: flat).  FORM 2 reads the layout through gathered waves (glrm_lane.hpp): waves built chunk by chunk of 1 024
    // segments (or SLOTS, where the layout's slots are permuted: they were dealt out class by class) so that a wave's lanes share lines,
    // packed from the decide kernel's compact list and spread over the chip for the tail rounds.  On the compact stream a lane finds its
    // value through the rank in its offset word and the step's base.  The CSR form (one lane walks its own list: the address translation
    // of 512 lists far apart, 3-5 ms for any tail round) is what remains for sub-ranges the layout does not
    // cover.  C5 recipe, 1M rows, X half-step (profiles/r06_c5family_lane_rounds_trace.txt): full grid 9.85 ms; gathered 7.8 ms at 55 %,
    // 5.4 at 32 %, 3.1 at 12 %, 1.5-2.1 for the tails.
    const int64_t pct = (int64_t)nact * 100 / (full.nseg > 0 ? full.nseg : 1);
    // Tail rounds: a wave per (segment, super-tile) instead of a lane's serial walk through every tile (rows: 1.5-9 ms per round at C5's stated
    // size, eight to ten of them per X half-step) -- below GLRM_HIP_LANE_TAIL / GLRM_HIP_LANE_TAIL_COLS percent of the segments
    if (list && (int64_t)nact * 100 < full.nseg * (int64_t)knob(full.nsup == 1 ? Knob::LANE_TAIL : Knob::LANE_TAIL_COLS)) {
      if (trace >= 2) fprintf(stderr, "[glrm lane] %s round %d: %u of %lld segments search: a wave per segment\n", side == GLRM_ROWS ? "row" : "column", round, nact, (long long)full.nseg);
      return launch_lane_tail(loss, full, list, (int64_t)nact, st);
    }
    bool packed = list && (int64_t)nact * 100 < full.nseg * knob(Knob::LANE_GATHER_PACKED);
    // (sides with permuted slots: chunk lists over the SLOTS, which were dealt out class by class -- make_segperm)
    const int32_t* gperm = la.inv ? full.segperm : nullptr;
    const bool chunks_ok = !la.inv || (v.lane_dealt && gperm && knob(Knob::LANE_GATHER_SLOTS));
    bool use_gather = gather && (chunks_ok || packed) && pct >= knob(Knob::LANE_GATHER_FROM) && pct < knob(Knob::LANE_GATHER_TO);
    int32_t gwaves = 0;
    if (use_gather) {
      const int off16 = (int)(full.own_offset & 15);
      if (packed) {
        const int spread = knob(Knob::LANE_GATHER_SPREAD); // searching segments per step of q: ~2 048 waves before a wave takes more per class
        int q = (int)(((int64_t)nact + spread - 1) / spread);
        q = q < 1 ? 1 : (q > 4 ? 4 : q);
        hipLaunchKernelGGL(lane_compact_list_kernel, dim3(1), dim3(1024), 0, st, list, (int)nact, off16, q, (int)h->lane_gcap, h->lane_glist, h->lane_gtotal);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(&gwaves, h->lane_gtotal, 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        if (gwaves < 0) { // (one class holds nearly every entry: the waves would not fit the list)
          packed = false;
          if (!chunks_ok) use_gather = false;
        }
      }
      if (use_gather && !packed) {
        const int64_t nitems = gperm ? (full.npass > 0 ? full.npass : full.nseg) : full.nseg;
        const int64_t nchunks = (nitems + LANE_CC - 1) / LANE_CC;
        const unsigned cg = (unsigned)((nchunks + 3) / 4);
        hipLaunchKernelGGL(lane_compact_count_kernel, dim3(cg), dim3(256), 0, st, full.active, nitems, nchunks, gperm, h->lane_gcnt);
        hipLaunchKernelGGL(lane_compact_scan_kernel, dim3(1), dim3(1024), 0, st, h->lane_gcnt, nchunks, h->lane_gbase, h->lane_gtotal);
        hipLaunchKernelGGL(lane_compact_fill_kernel, dim3(cg), dim3(256), 0, st, full.active, nitems, nchunks, gperm ? 0 : off16, gperm, h->lane_gbase, h->lane_glist);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(&gwaves, h->lane_gtotal, 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
      }
    }
    if (use_gather) {
      la.gwaves = gwaves;
      if (trace >= 2) fprintf(stderr, "[glrm lane] %s round %d: %u of %lld segments search: SELL gathered%s, %d waves\n", side == GLRM_ROWS ? "row" : "column", round, nact, (long long)full.nseg, packed ? " (packed)" : "", (int)gwaves);
      t.npass = 0;
      return launch_lane_loss<false, 2>(loss, t, la, (int64_t)gwaves, st);
    }
    // (measured cross-over of the two older forms at about a sixth of the segments, session r6_20)
    const bool compact = list && ((int64_t)nact * 100 < full.nseg * knob(Knob::LANE_CSR_BELOW) || !sell_ok);
    if (trace >= 2) fprintf(stderr, "[glrm lane] %s round %d: %u of %lld segments search: %s\n", side == GLRM_ROWS ? "row" : "column", round, nact, (long long)full.nseg, compact ? "CSR" : "SELL full grid");
    if (compact) {
      // (tried in session r6_45/46 and taken out again: this form over class-aware wave lists -- conflict-free tile reads -- measured the same at
      // full waves and worse spread over the chip; nor did batching its list reads move it.  A CSR round costs 2.8 x the full grid's time
      // per workgroup and tile at C5's stated size: 512 lanes walk 512 lists 1.2 MB apart, which is an address-translation pattern, not a
      // bandwidth or bank pattern.  Cross-over with the full grid stays at a sixth of the segments.)
      t.segperm = list;
      t.nseg = nact;
      t.npass = 0;
      return launch_lane_loss<false, 1>(loss, t, csr_args(t), ((int64_t)nact + 63) / 64, st);
    }
    if (sell_ok) return launch_lane_loss<false, 0>(loss, t, la, blk_hi - blk_lo, st);
    t.npass = 0;
    return launch_lane_loss<false, 1>(loss, t, csr_args(t), (t.nseg + 63) / 64, st);
  };
  return glrm_run_rounds(h, full, step.min_stepsize, lists, trial, [&](const TiledArgs& d) { launch_small(1, d, st); });
}
