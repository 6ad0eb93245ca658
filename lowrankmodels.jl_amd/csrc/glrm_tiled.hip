// glrm_tiled.hip -- host side + instantiations of the LDS-tiled sweeps (kernels in glrm_tiled.hpp).
// Separate translation unit so that the two kernel families compile in parallel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "glrm_engine.hpp"
#include "glrm_launch.hpp"
#include "glrm_tiled.hpp"

using namespace glrm;

// ------------------------------------------------------------------ LDS-tiled sweeps: setup and launch

static bool tile_rot_rt(int G, int R) { return (G == 4 || G == 8) && R == 8; }

// slot -> segment permutation of a tiled sweep: segments sorted by (loss kind of the column,) descending length, so that the 16
// lane groups of a wave meet one loss formula and lists of similar length.  nullptr when the natural order is already that
// (one loss kind and lengths within 25 % of each other: the synthetic BASELINE workloads).
// long_from > 0 (columns): segments of at least that many observations are left out of the slots (they run on the 8-wave gather sweep
// beside the passes, glrm_hip.hip: run_sweep) and listed in *longs; *nshort = slots handed out
static int make_segperm(glrm_handle* h, int side, int32_t** out, int64_t long_from = 0, std::vector<int32_t>* longs = nullptr, int64_t* nshort = nullptr) {
  *out = nullptr;
  const int64_t nseg = h->side[side].nseg;
  if (nshort) *nshort = nseg;
  if (nseg <= 1 || !knob(Knob::SEGPERM)) return GLRM_OK;
  std::vector<int64_t> ptr;
  int rc = glrm_host_ptr(h, side, ptr);
  if (rc) return rc;
  int64_t lmin = INT64_MAX, lmax = 0;
  for (int64_t s = 0; s < nseg; ++s) { const int64_t l = ptr[s + 1] - ptr[s]; lmin = l < lmin ? l : lmin; lmax = l > lmax ? l : lmax; }
  const bool kinds = side == GLRM_COLS && h->n_losses > 1;
  const bool divert = long_from > 0 && longs && lmax >= long_from;
  if (!kinds && !divert && lmax * 4 <= lmin * 5) return GLRM_OK;
  std::vector<int32_t> perm, none;
  glrm_split_by_length(ptr, divert ? long_from : 0, perm, divert ? *longs : none); // by descending length
  const int64_t nslots = (int64_t)perm.size();
  if (nshort) *nshort = nslots;
  if (kinds) { // loss kind first (stable: by descending length inside a kind)
    const glrm_loss* lt = h->losses_h.data() + h->side[GLRM_COLS].begin;
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return lt[x].kind < lt[y].kind; });
  }
  const bool lane_side = h->side[side].tiled && h->side[side].lane_want && knob(Knob::LANE_DEAL);
  if (lane_side) {
    // The lane-per-segment passes (glrm_lane.hpp) read their tiles conflict free when the 16 lanes of an LDS cycle hold 16 different
    // classes (global id) & 15 -- true when slot s holds a segment of class s & 15.  In natural order that is given; a sorted list is dealt
    // out class by class (the 16 classes are equally frequent, so a wave still meets segments of one kind and similar length; a class
    // that runs dry is filled from the longest remaining queue: costs conflicts at the tail, never bits).  Measured before (session r6_35,
    // C5 recipe at 1M rows, columns sorted by kind and length): bank conflicts in 48 % of the column passes' LDS cycles.
    std::vector<int32_t> q[16];
    const int64_t g0 = h->side[side].begin;
    h->side[side].lane_dealt = 1;
    for (int32_t sgm : perm) q[(g0 + sgm) & 15].push_back(sgm);
    size_t head[16] = {0};
    for (int64_t slot = 0; slot < nslots; ++slot) {
      int c = (int)(slot & 15);
      if (head[c] >= q[c].size()) {
        size_t best = 0;
        for (int d = 0; d < 16; ++d)
          if (q[d].size() - head[d] > best) { best = q[d].size() - head[d]; c = d; }
      }
      perm[(size_t)slot] = q[c][head[c]++];
    }
  } else if (side == GLRM_COLS && tile_rot_rt(h->G, h->R)) {
    // the column passes read their tiles conflict-free (glrm_tiled.hpp: tile_rot) when slot s holds a segment of class (s & 7) >> 1,
    // class = ((global id) & 7) >> 1: deal the sorted list out class by class, two per block of eight slots -- the four classes are
    // equally frequent, so every wave still meets segments of one kind and similar length; a class that runs dry is filled from the
    // longest remaining queue (costs bank conflicts at the tail, never bits)
    std::vector<int32_t> q[4];
    for (int32_t sgm : perm) q[tile_rot_of(h->side[GLRM_COLS].begin + sgm)].push_back(sgm);
    size_t head[4] = {0, 0, 0, 0};
    for (int64_t slot = 0; slot < nslots; ++slot) {
      int c = tile_rot_of(slot); // the class the slot's position wants
      if (head[c] >= q[c].size()) {
        size_t best = 0;
        for (int d = 0; d < 4; ++d)
          if (q[d].size() - head[d] > best) { best = q[d].size() - head[d]; c = d; }
      }
      perm[(size_t)slot] = q[c][head[c]++];
    }
  }
  return glrm_upload_list(h, perm, out);
}

// create phase: the lane layout of the tiled kernels and whether this shard's lists are in tile order (glrm_signature::rows_unordered /
// cols_unordered): the entries of staged tile t must precede those of tile t+1
int glrm_prepare_tiled(glrm_handle* h) {
  hipStream_t st = h->stream;
  h->tG = h->G;
  h->tR = h->R;
  const int T = glrm_tile_rows(h->kp);
  if (const int rc = h->mem.alloc(&h->dflag, 2)) return rc;
  HIPCK(hipMemsetAsync(h->dflag, 0, 2 * sizeof(int), st));
  for (int s = 0; s < 2; ++s) { // a block per segment: 64 threads for a row's list, 256 for a column's (columns are the long ones)
    const glrm_handle::Side& v = h->side[s];
    if (v.nseg > 0) hipLaunchKernelGGL(check_sorted_kernel, dim3((unsigned)v.nseg), dim3(s == GLRM_ROWS ? 64 : 256), 0, st, v.ptr, v.idx, v.nseg, T, h->dflag + s);
  }
  HIPCK(hipGetLastError());
  int flags[2] = {0, 0};
  HIPCK(hipMemcpyAsync(flags, h->dflag, sizeof flags, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  h->sig_local.rows_unordered = flags[0] != 0;
  h->sig_local.cols_unordered = flags[1] != 0;
  return GLRM_OK;
}

// finalize phase.  Everything that selects a family is read from h->sig -- the signature of the WHOLE problem -- and from (m, n, k,
// options): every shard of a sharded fit lands on the same family.
int glrm_setup_tiled(glrm_handle* h) {
  hipStream_t st = h->stream;
  int rc0 = GLRM_OK;
  glrm_handle::Side &rows = h->side[GLRM_ROWS], &cols = h->side[GLRM_COLS];
  rows.sorted = !h->sig.rows_unordered;
  cols.sorted = !h->sig.cols_unordered;

  const int T = glrm_tile_rows(h->kp);
  // expected observations of one segment inside one tile; the tiled sweeps pay off when a staged
  // vector is reused by several of the workgroup's segments
  const double per_tile_r = (double)h->sig.nnz_rows / (double)h->m * T / (double)h->n;
  const double per_tile_c = (double)h->sig.nnz_cols / (double)h->n * T / (double)h->m;
  // h->tiled_opt (glrm_options.tiled): 0 auto, 1 gather sweeps only, 2 tiled wherever the index lists are sorted.
  // GLRM_HIP_TILED (tuning): bit0 rows, bit1 columns; overrides the option.
  int want = h->tiled_opt == 1 ? 0 : (h->tiled_opt == 2 ? 3 : -1);
  want = knob_or(Knob::TILED, want);
  // Auto choice (measured on MI355X, tests/perf/bench_small.py): the tiled sweeps need enough workgroups to fill 256 CUs and
  // enough observations to amortise their per-tile barriers; below ~2e7 observations per view the gather sweeps win (100k x 5k
  // at 1e7 observations: 1.06 vs 1.23 ms per iteration; 300k x 3k at 4.5e7: 4.6 vs 3.1 ms).
  const int spb_auto = 16 * (64 / h->tG);
  const bool big_r = h->sig.nnz_rows >= 20000000 && h->m >= (int64_t)512 * spb_auto;
  const bool big_c = h->sig.nnz_cols >= 20000000 && h->n >= 256;
  bool want_row = want < 0 ? (per_tile_r >= 4.0 && big_r) : (want & 1) != 0;
  bool want_col = want < 0 ? (per_tile_c >= 4.0 && big_c) : ((want >> 1) & 1) != 0;
  // Lists in arbitrary order (obs tuples pushed in sampling order): the engine's private copy is brought into tile order by a
  // stable segmented sort, so such inputs run the tiled sweeps too.  Only when the auto choice wants the tiled sweeps -- an
  // explicit tiled = 2 keeps its meaning "wherever the lists allow" (GLRM_HIP_TILE_SORT=0 disables, =2 sorts for tiled = 2 as well).
  const int tsort = knob(Knob::TILE_SORT);
  const bool may_sort = tsort == 2 || (tsort == 1 && want < 0);
  // (a shard whose own lists are already in tile order gets them back unchanged -- the sort is stable -- so the decision may be
  // taken for the whole problem; a list too long for the segmented sort anywhere keeps every shard on the gather sweeps)
  const int64_t sort_limit = (int64_t)knob_positive(Knob::TILE_SORT_BATCH, 1.5e9);
  const bool want_side[2] = {want_row, want_col}, unordered_here[2] = {h->sig_local.rows_unordered != 0, h->sig_local.cols_unordered != 0};
  const int64_t max_len[2] = {h->sig.max_row_len, h->sig.max_col_len};
  for (int s = 0; s < 2; ++s) {
    glrm_handle::Side& v = h->side[s];
    if (want_side[s] && !v.sorted && may_sort && max_len[s] <= sort_limit) {
      if (unordered_here[s]) {
        const int rc = glrm_tile_sort_view(st, v.ptr, v.nseg, v.nnz, T, h->side[s ^ 1].nglob, &v.idx, &v.vals, h->mem);
        if (rc) return rc;
      }
      v.sorted = true;
    }
    v.tiled = (v.sorted && want_side[s]) ? 1 : 0;
  }
  // (rows on the lane-per-segment passes -- glrm_lane.hpp -- keep the caller's order: every lane evaluates its own observation's loss, so
  // there is no wave-wide formula to align, and the grouped copy would cost 12 B per observation beside the SELL stream)
  h->tile_rounds = knob(Knob::TILE_ROUNDS); // bit0 rows, bit1 columns (below: the rounds' lists and pass buffers)
  glrm_lane_decide(h);
  const bool lane_rows = rows.tiled && (h->tile_rounds & 1) && rows.lane_want;
  if (rows.tiled && h->n_losses > 1 && rows.nnz > 0 && knob(Knob::GROUP_KINDS) && !lane_rows) {
    DevArena scratch;
    int32_t* oidx = nullptr;
    double* ovals = nullptr;
    if ((rc0 = scratch.alloc(&oidx, (size_t)rows.nnz)) || (rc0 = scratch.alloc(&ovals, (size_t)rows.nnz))) return rc0;
    hipLaunchKernelGGL(group_rows_by_kind_kernel, dim3((unsigned)rows.nseg), dim3(64), 0, st, rows.ptr, rows.idx, rows.vals, rows.nseg, T, h->losses, oidx, ovals);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(st));
    h->mem.release(&rows.idx); // (a borrowed view is not the arena's: it stays the caller's)
    h->mem.release(&rows.vals);
    rows.idx = oidx;
    rows.vals = ovals;
    scratch.move_to(h->mem, oidx);
    scratch.move_to(h->mem, ovals);
    rows.grouped = true;
  }
  if (rows.tiled && h->n_losses > 1 && rows.nnz > 0 && knob(Knob::UDESC)) {
    // distinct loss descriptors of the model; with at most 256 of them every entry of the row view carries a one-byte id and the
    // row sweep reads descriptors from an LDS table (TiledArgs::descid)
    std::vector<glrm_loss> uniq;
    std::vector<uint8_t> colid((size_t)h->n);
    bool ok = true;
    for (int64_t f = 0; f < h->n && ok; ++f) {
      const glrm_loss& l = h->losses_h[(size_t)f];
      size_t u = 0;
      for (; u < uniq.size(); ++u)
        if (uniq[u].kind == l.kind && uniq[u].dim == l.dim && uniq[u].scale == l.scale && uniq[u].p0 == l.p0 && uniq[u].p1 == l.p1) break;
      if (u == uniq.size()) {
        if (uniq.size() == 256) { ok = false; break; }
        uniq.push_back(l);
      }
      colid[(size_t)f] = (uint8_t)u;
    }
    if (ok) {
      DevArena scratch;
      uint8_t* dcolid = nullptr;
      if ((rc0 = scratch.alloc(&dcolid, (size_t)h->n)) || (rc0 = h->mem.alloc(&h->udesc, uniq.size())) || (rc0 = h->mem.alloc(&h->rowdescid, (size_t)rows.nnz))) return rc0;
      HIPCK(hipMemcpyAsync(dcolid, colid.data(), (size_t)h->n, hipMemcpyHostToDevice, st));
      HIPCK(hipMemcpyAsync(h->udesc, uniq.data(), uniq.size() * sizeof(glrm_loss), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(entry_descid_kernel, dim3(4096), dim3(256), 0, st, rows.idx, rows.nnz, dcolid, h->rowdescid);
      HIPCK(hipGetLastError());
      HIPCK(hipStreamSynchronize(st)); // colid / uniq are locals
      h->n_udesc = (int)uniq.size();
    }
  }
  // super-tiles of ~32k rows: a function of (m, tile) only -- never of the shard layout -- so the partial-sum order
  // (and the result bits) do not depend on the GPU count, while long columns still spread over enough workgroups
  const int64_t ntiles = (h->m + T - 1) / T;
  {
    // enough (column group, super-tile) workgroups to fill the chip a few times over: the column groups come from the GLOBAL n
    // (256 columns per 16-wave workgroup at G=4), so the super-tile size -- hence the order of the partial sums -- is a function
    // of (m, n, tile) only, never of the shard layout
    // (the lane-per-segment form of the passes holds 512 columns per workgroup and stages its tiles of X at ~3 TB/s with nothing to overlap
    // them: more, shorter super-tiles even the workgroups out -- C2 Y half-step 7.6 -> 7.0 ms at twice the workgroups, session r6_09; the
    // family is a function of the whole problem's signature, so this still is)
    const bool lane_c = cols.tiled && cols.lane_want;
    const int spb = lane_c ? 512 : 16 * (64 / h->tG);
    const int64_t groups = (h->n + spb - 1) / spb;
    const int64_t want_wg = knob_or(Knob::COL_WORKGROUPS, lane_c ? 2048 : 1024);
    int64_t nsup_target = (want_wg + groups - 1) / groups;
    if (nsup_target < 1) nsup_target = 1;
    int64_t tps = ntiles / nsup_target;
    const int64_t tps_max = 32768 / T > 1 ? 32768 / T : 1; // at most ~32k rows per super-tile (long columns still spread out)
    if (tps > tps_max) tps = tps_max;
    if (tps < 1) tps = 1;
    cols.pass.tiles_per_sup = (int)tps;
  }
  cols.pass.nsup = (int)((ntiles + cols.pass.tiles_per_sup - 1) / cols.pass.tiles_per_sup);
  if (cols.tiled) {
    if ((rc0 = glrm_alloc_pass_buffers(h, GLRM_COLS))) return rc0;
    HIPCK(hipMemsetAsync(cols.pass.active, 0, (size_t)(cols.nseg > 0 ? cols.nseg : 1) * 4, st)); // diverted columns are never touched by col_reduce: "not searching"
    // Skewed column lengths (round 5, like the phase-aligned passes: glrm_blocked.hip).  The columns are already handed out sorted by
    // length; a workgroup's 256 columns walk a tile in lockstep (one barrier per tile), so ONE column many times the others keeps its
    // workgroup on every tile for its own entries alone, and the few workgroups of the head of the sorted list are the makespan (C2
    // recipe with Zipf(0.5) degrees: Y half-step 22.1 ms against 9.0).  Columns of at least long_from = max(4 096, 4 x the whole problem's
    // mean column length) observations leave the passes for the 8-wave gather sweep on the side stream: a function of the column's own
    // length and the whole problem's signature (shard-invariant), reported in glrm_sum_order.long_from.  Measured at C2-Zipf (mean 50 266,
    // longest 879 189): Y half-step 27.5 / 19.0 / 16.2 / 17.1 ms at 1 / 2 / 4 / 8 x mean (profiles/r05_c2_zipf_long_from_sweep.txt): the
    // gather sweep pays 536 B per update where the tiles pay a fraction, so only the head of the distribution is worth diverting.
    const int64_t mean_len = h->sig.nnz_cols / (h->n > 0 ? h->n : 1);
    const int long_from = knob(Knob::TILED_LONG_FROM);
    h->blk_long_from = long_from >= 0 ? long_from : std::max<int64_t>(4096, 4 * mean_len);
    std::vector<int32_t> longl;
    if ((rc0 = make_segperm(h, GLRM_COLS, &cols.perm, h->blk_long_from, &longl, &h->blk_nshort_c))) return rc0;
    if ((rc0 = glrm_set_long_columns(h, longl))) return rc0;
  }
  if (rows.tiled && (rc0 = make_segperm(h, GLRM_ROWS, &rows.perm))) return rc0;
  // Line-search rounds over the still-searching segments only (glrm_tiled.hpp: TiledArgs::actlist_out).  Columns: the passes after the
  // first trial; rows: everything after the first trial, which stays fused with the gradient pass in one kernel (GLRM_HIP_TILE_ROUNDS,
  // read above into tile_rounds; 0 = the round-3 forms).  Two lists (the decide kernel reads one and writes the next).
  if ((rows.tiled && (h->tile_rounds & 1)) || (cols.tiled && (h->tile_rounds & 2))) {
    const int64_t cap = std::max<int64_t>(1, std::max(rows.tiled ? rows.nseg : 0, cols.tiled ? cols.nseg : 0));
    if ((rc0 = h->mem.alloc(&h->actlist, (size_t)cap * 2))) return rc0;
    h->actlist_cap = cap;
  }
  // the pass buffers of the row rounds: ONE super-tile (nothing is re-added: the bits of the one-kernel sweep)
  if (rows.tiled && (h->tile_rounds & 1)) {
    const int64_t nt = (h->n + T - 1) / T;
    rows.pass.tiles_per_sup = (int)(nt > 0 ? nt : 1);
    rows.pass.nsup = 1;
    if ((rc0 = glrm_alloc_pass_buffers(h, GLRM_ROWS))) return rc0;
  }
  return glrm_setup_lane(h); // the lane-per-segment form of the passes where it applies (glrm_lane.hip)
}

template <typename K>
static int set_lds(K kernel, int bytes) {
  if (bytes > 65536) HIPCK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return GLRM_OK;
}

// kind: 0 = whole sweep (tiled_sweep_kernel), 1 = column pass 1, 2 = column trial pass, 3 = row sweep in rounds form (gradient pass +
// first trial, the rest handed to the rounds), 4 = trial pass of the row rounds
template <int G, int R, int NW, int TILE, int LOSS>
static int launch_tiled_inst(int kind, const TiledArgs& a, hipStream_t st) {
  constexpr int SPB = NW * (64 / G);
  const int lds = tile_lds_bytes<G, R, TILE>() + (loss_mode(LOSS) == 2 && a.descid ? a.n_udesc * 32 : 0);
  const unsigned gx = (unsigned)(((a.npass > 0 ? a.npass : a.nseg) + SPB - 1) / SPB);
  int rc = GLRM_OK;
  auto sweep = [&](auto FIXED, auto ROUNDS) { // the whole-sweep kernel; VR: the side has vector regularizers (csrc/glrm_device.hpp)
    auto go = [&](auto kernel) {
      if ((rc = set_lds(kernel, lds))) return;
      hipLaunchKernelGGL(kernel, dim3(gx), dim3(NW * 64), lds, st, a);
    };
    if (a.vecreg) go(tiled_sweep_kernel<G, R, NW, TILE, LOSS, decltype(FIXED)::value, decltype(ROUNDS)::value, true>);
    else go(tiled_sweep_kernel<G, R, NW, TILE, LOSS, decltype(FIXED)::value, decltype(ROUNDS)::value>);
  };
  if (kind == 0 && a.fixed_alpha > 0.0) {
    sweep(std::true_type{}, std::false_type{});
    if (rc) return rc;
  } else if (kind == 0) {
    sweep(std::false_type{}, std::false_type{});
    if (rc) return rc;
  } else if (kind == 3) {
    sweep(std::false_type{}, std::true_type{});
    if (rc) return rc;
  } else if (kind == 4) {
    if ((rc = set_lds(tiled_col_pass_kernel<G, R, NW, TILE, LOSS, false, false, true>, lds))) return rc;
    hipLaunchKernelGGL((tiled_col_pass_kernel<G, R, NW, TILE, LOSS, false, false, true>), dim3(gx, (unsigned)(a.nsup_launch > 0 ? a.nsup_launch : a.nsup)), dim3(NW * 64), lds, st, a);
  } else if (kind == 1) {
    if ((rc = set_lds(tiled_col_pass_kernel<G, R, NW, TILE, LOSS, true, false>, lds))) return rc;
    hipLaunchKernelGGL((tiled_col_pass_kernel<G, R, NW, TILE, LOSS, true, false>), dim3(gx, (unsigned)(a.nsup_launch > 0 ? a.nsup_launch : a.nsup)), dim3(NW * 64), lds, st, a);
  } else {
    if ((rc = set_lds(tiled_col_pass_kernel<G, R, NW, TILE, LOSS, false, false>, lds))) return rc;
    hipLaunchKernelGGL((tiled_col_pass_kernel<G, R, NW, TILE, LOSS, false, false>), dim3(gx, (unsigned)(a.nsup_launch > 0 ? a.nsup_launch : a.nsup)), dim3(NW * 64), lds, st, a);
  }
  return GLRM_OK;
}

// 16 waves and one ~150 KB tile per CU
static int launch_tiled(glrm_handle* h, int loss, int kind, const TiledArgs& a) {
  auto by_layout = [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value, T = glrm_tile_rows(G * R);
    auto by_loss = [&](auto LOSS) { return launch_tiled_inst<G, R, 16, T, decltype(LOSS)::value>(kind, a, h->stream); };
    return glrm_dispatch<LOSS_QUAD_UNIFORM, LOSS_SEGMENT, LOSS_SEGMENT_NOTRIG, LOSS_PER_OBS_NOTRIG>(loss, by_loss, [&] { return by_loss(glrm_const<LOSS_PER_OBS>{}); });
  };
  return glrm_dispatch_layout<8, 16, 32, 64, 128>(h->tG, h->tR, by_layout, [&] { return fail(GLRM_ERR_UNSUPPORTED, "no tiled kernel for lane layout G=%d R=%d", h->tG, h->tR); });
}

void glrm_launch_col_small(int kp, int stage, const TiledArgs& a, hipStream_t st) {
  auto by_layout = [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    const unsigned gx = (unsigned)((a.nseg + 4 * (64 / G) - 1) / (4 * (64 / G)));
    if (stage == 0 && a.vecreg) hipLaunchKernelGGL((col_reduce_kernel<G, R, true>), dim3(gx), dim3(256), 0, st, a);
    else if (stage == 0) hipLaunchKernelGGL((col_reduce_kernel<G, R>), dim3(gx), dim3(256), 0, st, a);
    else if (a.vecreg) hipLaunchKernelGGL((col_decide_kernel<G, R, true>), dim3(gx), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((col_decide_kernel<G, R>), dim3(gx), dim3(256), 0, st, a);
    return GLRM_OK;
  };
  glrm_dispatch_layout<8, 16, 32, 64>(glrm_layout_g(kp), glrm_layout_r(kp), by_layout, [&] { return by_layout(glrm_const<16>{}, glrm_const<8>{}); });
}

// The tiled variants of run_sweep's launch.  Rows: one kernel.  Columns: pass 1 -> reduce -> rounds of
// (trial pass, decide) until no column is still searching (the count is read back once per round).
int glrm_run_tiled(glrm_handle* h, const glrm_step& step) {
  const int side = step.side, loss = step.loss;
  TiledArgs a{};
  glrm_fill_side(a, h, step);
  a.loss_by_segment = step.loss_by_segment;
  a.descid = side == GLRM_ROWS ? h->rowdescid : nullptr;
  a.udesc = h->udesc;
  a.n_udesc = h->n_udesc;
  if (step.ranged()) {
    glrm_apply_row_range(a, step);
    if (a.nseg <= 0) return GLRM_OK;
  }
  const glrm_act_lists lists = glrm_active_lists(h, side, a.nseg);
  const bool row_rounds = side == GLRM_ROWS && (h->tile_rounds & 1) && !step.eval_only && !step.fixed() && h->actlist;
  // lane-per-segment passes (glrm_lane.hpp): the ProxGradParams half-steps and the evaluation pass of the sides that run that family
  const bool lane_here = h->side[side].lane && glrm_lane_loss_ok(h, loss) && !step.fixed() && (side == GLRM_ROWS ? row_rounds : true);
  a.segperm = step.ranged() ? nullptr : h->side[side].perm; // a sub-range sweep keeps the natural order
  if (side == GLRM_ROWS && !row_rounds) return launch_tiled(h, loss, 0, a);
  glrm_bind_pass_buffers(a, h, side, step.ranged() ? step.row_begin : 0); // (rows: one super-tile, glrm_setup_tiled)
  if (side == GLRM_COLS && h->blk_nlong_c > 0) { // the columns at or above long_from run on the gather sweep beside the passes (run_sweep, glrm_hip.hip)
    a.long_from = h->blk_long_from;
    a.npass = h->blk_nshort_c;
    if (a.npass == 0) { // every local column is diverted
      HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
      return GLRM_OK;
    }
  }
  if (lane_here) return glrm_run_lane(h, step, a);
  int rc;
  HIPCK(hipMemsetAsync(h->nactive, 0, 4, h->stream));
  a.actlist_out = lists.list[0]; // the list the kernels of this stage append to
  if (side == GLRM_ROWS) {
    if ((rc = launch_tiled(h, loss, 3, a))) return rc; // gradient pass + first trial; rejected rows are listed
  } else {
    // gradient pass: under glrm_hip_step_y_arrival in runs of super-tiles, each behind the blocks of X it reads (announced order)
    rc = glrm_for_sup_runs_in_arrival_order(h, step.arrivals, a.nsup, (int64_t)a.tiles_per_sup * glrm_tile_rows(h->kp), [&](int s0, int s1) {
      TiledArgs r = a;
      r.sup0 = s0;
      r.nsup_launch = s1 - s0;
      return launch_tiled(h, loss, 1, r);
    });
    if (rc) return rc;
    glrm_launch_col_small(h->kp, 0, a, h->stream);
  }
  HIPCK(hipGetLastError());
  if (step.eval_only || step.fixed()) return GLRM_OK;
  return glrm_run_rounds(
      h, a, step.min_stepsize, lists,
      [&](int, unsigned int nact, int32_t* list) {
        TiledArgs t = a;
        // the trial pass: over the listed segments when they are the minority (a full grid keeps the length / kind order of segperm, which
        // pays while nearly every segment still takes part: the first trial of the columns)
        if (list && (side == GLRM_ROWS || (int64_t)nact * 4 < a.nseg * 3)) {
          t.segperm = list;
          t.nseg = nact;
          t.npass = 0;
        }
        return launch_tiled(h, loss, side == GLRM_ROWS ? 4 : 2, t);
      },
      [&](const TiledArgs& d) { glrm_launch_col_small(h->kp, 1, d, h->stream); });
}
