// glrm_tiled.hpp -- LDS-tiled sweeps: the opposing factor is staged through LDS tile by tile and every
// lane group owns ONE segment (row or column) whose observations it walks in list order.
//
// Why: in the gather sweeps (glrm_hip.hip) every observation fetches its own k-vector of the opposing
// factor from L2 / Infinity Cache / HBM (2 x 128-byte lines at k=32), which is what bounds them
// (profiles/r01_baseline_pmc_summary.md).  Here a workgroup of NW waves owns SPB = NW*64/G segments; it
// loops over tiles of TILE consecutive opposing vectors, copies the tile into LDS once (coalesced 16-byte
// loads) and every group consumes the observations of its segment that fall into the tile from LDS.  A
// factor vector is thus read from memory once per (workgroup, pass) instead of once per observation, and
// the per-observation traffic left is the 12-byte (index, value) stream.
//
// Requirements: the segment's index list is ordered by tile -- the entries of tile t come before those of tile t+1; a
// non-decreasing list (`findall` / sparse input, src/glrm.jl:46-48) is the common case.  Checked at create, otherwise the
// gather sweeps are used.  Duplicates are fine.
//
// Summation order: a group accumulates its segment's losses and gradient sequentially in the order of the engine's private
// list (the caller's list order unless the engine had to tile-sort or kind-group it) --
// the reference's own order (src/algorithms/proxgrad.jl:122-132, src/evaluate_fit.jl:28-32).  The column
// sweep additionally splits the rows into NSUP super-tiles whose partial sums are added in order; NSUP
// depends only on (m, TILE), never on the shard layout, so results stay independent of the GPU count.
#pragma once

#include "glrm_device.hpp"

namespace glrm {

struct TiledArgs {
  int64_t nseg;          // local segments
  const int64_t* ptr;    // nseg+1
  const int32_t* idx;    // non-decreasing inside every segment
  const double* vals;
  double* own;           // factor being updated (global array, ld = KP)
  int64_t own_offset;    // global id of local segment 0
  const double* other;   // opposing factor (global array, ld = KP)
  int64_t n_other;       // number of opposing vectors
  double* alpha;         // per local segment
  double* obj;           // per GLOBAL segment (nullable)
  const glrm_loss* losses;
  int loss_by_segment;
  const glrm_reg* regs;
  int reg_single;
  int k;
  double min_stepsize;
  int32_t* trials;
  int32_t* accepts;
  // column sweep (split over super-tiles)
  int nsup;              // number of super-tiles
  int tiles_per_sup;     // tiles per super-tile
  double* part;          // [nseg][nsup][KP+2]: partial gradient (KP), partial loss sum, pad
  double* gsum;          // [nseg][KP]   reduced gradient (kept for later trials)
  double* trial;         // [nseg][KP]   current trial point
  double* jold;          // [nseg]
  double* jloss;         // [nseg] nullable: col_reduce stores the loss sum at the current point (dense path, quad_gram trials)
  int32_t* active;       // [nseg] 1 while the segment's line search is still running
  int32_t* ntrial;       // [nseg] trials taken in this sweep
  unsigned int* nactive; // device counter of still-active segments
  int eval_only;         // col_reduce: obj = sum of losses, nothing else
  int64_t dense_len;     // ptr == nullptr (dense problem): every segment has this many observations
  double fixed_alpha;    // > 0: one prox-gradient step with this global step size, no line search
  // heterogeneous row sweep (a loss descriptor per observation): the DISTINCT descriptors of the model (at most 256) sit in LDS behind
  // the tile and every entry of the row view carries the id of its column's descriptor, so the step reads its descriptor from LDS
  // with the batch instead of waiting for a dependent global load of losses[column] (nullptr: table lookups)
  const uint8_t* descid;  // per entry of the view
  const glrm_loss* udesc; // n_udesc distinct descriptors
  int n_udesc;
  // phase-aligned gather passes (tiled_col_pass_kernel<..., L2 = true>): the launch covers segments [seg_begin, seg_begin + nseg_slice)
  // of super-tile sup_fixed
  int64_t seg_begin, nseg_slice;
  int sup_fixed;
  int nsup_launch;       // > 0: super-tiles this launch covers (grid y); 0 = all nsup
  int sup0;              // LDS-tiled / lane column passes: the launch covers super-tiles sup0 .. sup0 + gridDim.y - 1 (arrival order, round 6)
  const int32_t* segperm; // lane-group slot -> local segment (nullptr = identity).  Which segment a group works on changes no sum:
                          // columns are handed out sorted by (loss kind, length), rows by length, so that the 16 groups of a wave
                          // evaluate the same loss formula and finish their lists together.
  // Line-search rounds over the segments that are STILL SEARCHING only (round 4).  A workgroup stages every tile of the opposing factor
  // per pass whether one of its 256 segments needs the pass or all of them: with the search inside the kernel (rows) or a pass over
  // every workgroup that holds an active segment (columns), a few percent of rejected first trials made EVERY workgroup run another
  // pass (C2: 4 % of the rows, 1.4 % of the columns; C5: the tail of rows on their 3rd .. 6th trial).  Whoever leaves a segment searching
  // appends it to `actlist_out` (slot = the old value of *nactive); the next trial pass runs over that list (`segperm` = the list,
  // nseg = its length: ceil(count / 256) workgroups) and the decide kernel reads it as `actlist_in`.  Which slot a segment sits in
  // changes no sum (see segperm), so the bits are those of the uncompacted rounds.
  // Phase-aligned column passes on skewed data (round 5): the pass launches cover the first `npass` slots of `segperm` (the segments
  // below `long_from` observations, longest first, so that the groups of a launch slice walk lists of like length); segments of at
  // least `long_from` observations are swept by the 8-wave gather sweep beside the passes and are skipped by col_reduce / col_decide.
  int64_t npass;              // 0 = every segment
  int64_t long_from;          // 0 = no segment is diverted
  int32_t* actlist_out;       // nullable
  const int32_t* actlist_in;  // col_decide_kernel: nullable; the segments to decide (nact_in of them) instead of all nseg
  int64_t nact_in;
  int gate;                   // phase-aligned passes (tiled_pass<..., L2 = true>): a lane group whose next observation lies more than `gate` rows
                              // past the wave's trailing group sits the step out (0 = off; see tiled_pass)
  const int32_t* suppos;      // phase-aligned passes: [nseg][nsup] offset inside the segment's list of its first entry of the super-tile, i.e.
                              // what lower_bound_idx finds at every launch (the lists never change); nullptr = search
  int vecreg;            // 1: a descriptor of this side names a vector regularizer -- the VR = true kernels (csrc/glrm_device.hpp)
};

// v from lane (lane ^ X) for X = 4 or 8 (ds_swizzle bit-mask mode: and 0x1F, or 0, xor X; no LDS memory touched)
template <int X>
__device__ __forceinline__ double swizzle_xor_f64(double v) {
  const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), (X << 10) | 0x1F);
  const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), (X << 10) | 0x1F);
  return __hiloint2double(hi, lo);
}

// lane gets v from lane (u0 + (lane & 1)) of its group: the observation "owned" by the lane's parity
template <int G>
__device__ __forceinline__ double pair_bcast_f64(double v, int u0, int lane) {
  if constexpr (G == 4) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    if (u0 == 0) { // quad_perm:[0,1,0,1]
      lo = __builtin_amdgcn_mov_dpp(lo, 0x44, 0xF, 0xF, false);
      hi = __builtin_amdgcn_mov_dpp(hi, 0x44, 0xF, 0xF, false);
    } else { // quad_perm:[2,3,2,3]
      lo = __builtin_amdgcn_mov_dpp(lo, 0xEE, 0xF, 0xF, false);
      hi = __builtin_amdgcn_mov_dpp(hi, 0xEE, 0xF, 0xF, false);
    }
    return __hiloint2double(hi, lo);
  } else {
    return __shfl(v, (lane & ~(G - 1)) + u0 + (lane & 1), 64);
  }
}

// ---- conflict-free tile reads in the column passes (G = 4 or 8 lanes, four 16-byte chunks per lane) ---------------------------
// ds_read_b128 serves a wave in four LDS cycles of 16 lanes -- {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32
// (MI355X_MICROARCH.md, LDS) -- i.e. four lane groups (G = 4) per cycle, each reading 64 contiguous bytes of ITS row.  With rows
// padded by 16 B those four 16-bank windows start at random banks and overlap: 52 % of the LDS cycles of the C2 sweeps were conflict
// cycles, and random row reads reach 63 TB/s against 118 TB/s conflict-free (tools/ubench_lanerow.hip,
// profiles/r02_ubench_lanerow.txt).  With ROT the staged rows are NOT padded (every row starts at bank 0) and a lane group walks its
// row's chunks in the order i ^ p, p = ((global segment id) & 7) >> 1: the four groups of an LDS cycle sit at positions {0,3,5,6}
// or {1,2,4,7} of their half wave, whose p are all different when segments occupy the slots in order, so at every instruction they
// read four DIFFERENT bank quarters -- SQ_LDS_BANK_CONFLICT = 0, whatever rows they read.  Register i of a lane then holds chunk
// i ^ p of x, g and y alike (dot products and axpys pair equal registers; loads, stores and masks go by the chunk id).  p depends
// on the segment only, never on where it runs, so sums are formed in the same order under any shard layout or slot permutation (a
// slot order that breaks the pattern costs conflicts, not bits; make_segperm keeps the pattern).
// Measured (profiles/r02_rot_pmc_c2.md, r02_rot_ab.txt; same box A/B): conflicts 1.43e9 -> 0 and LDS-busy cycles halved in every tiled
// kernel, SQ_WAIT_INST_LDS / 20 -- but the sweeps are not LDS-bound.  Row sweeps: QuadLoss 8.56 vs 8.48 ms, heterogeneous 407 vs 387 ms
// (three more address XORs per observation, a few more spilled registers).  Column passes: QuadLoss 9.80 vs 9.67 ms, heterogeneous
// 47.96 vs 50.08 ms.  So only the column passes of models with non-quadratic losses (LOSS != 0) use it.
template <int G, int R>
constexpr bool tile_rot() { return (G == 4 || G == 8) && R == 8; }
__host__ __device__ __forceinline__ int tile_rot_of(int64_t gseg) { return ((int)gseg & 7) >> 1; }

template <int G, int R>
constexpr int tile_row_bytes() { return G * R * 8 + 16; } // LDS budget per staged row: +16 B pad, consecutive rows start 4 banks apart
template <int G, int R, bool ROT>
constexpr int tile_row_stride() { return ROT ? G * R * 8 : tile_row_bytes<G, R>(); } // ROT: unpadded rows inside the same budget

template <int G, int R, int TILE>
constexpr int tile_lds_bytes() { return TILE * tile_row_bytes<G, R>(); } // the staged tile; the descriptor table sits behind

// Staging by LDS-DMA from all waves (round 3): every 16-byte piece of the tile image is one lane of a global_load_lds_dwordx4 -- all
// pieces of the tile in flight at once (nine instructions per wave for the 149 KB tile of k = 32), no VGPRs, no ds_write pass -- where the
// load / ds_write staging of rounds 1-2 kept four loads per thread in flight and needed three rounds of load -> wait -> write.  Lanes past
// the end of the image are masked off (an inactive lane writes nothing).  Padded rows: piece c = row c / 17, piece c % 17 of it (the pad
// piece re-reads the 16th); ROT rows are unpadded and the image is a plain copy.  Measured on one box (profiles/r03_tile_dma_all_ab.txt):
// C5-family row sweep 63.2 -> 54.0 ms, C2 column passes 9.92 -> 9.00 ms, identical objectives.
template <int G, int R, int NW, bool ROT>
__device__ __forceinline__ void dma_tile_all(const double* __restrict__ other, int64_t lo, int64_t hi, char* buf, int wave, int lane) {
  constexpr int KPB = G * R * 8, ROWB = tile_row_stride<G, R, ROT>(), CPR = ROWB / 16;
  const int rows = (int)(hi - lo), total = rows * CPR;
  const char* src0 = reinterpret_cast<const char*>(other) + lo * KPB;
  for (int base = wave * 64; base < total; base += NW * 64) {
    const int c = base + lane;
    if (c < total) {
      const char* src;
      if constexpr (ROT) {
        src = src0 + c * 16;
      } else {
        const int row = c / CPR;
        int cc = c - row * CPR;
        cc = cc < CPR - 1 ? cc : CPR - 2; // the pad piece
        src = src0 + row * KPB + cc * 16;
      }
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(buf + base * 16), 16, 0, 0);
    }
  }
}

// chunk held by register i of a lane whose first chunk sits at byte `ro` of the tile (ro carries the lane's 16-byte slot and, with
// ROT, its rotation in the chunk field, which register index i then flips: chunk i ^ rot)
template <bool ROT, int CB, class P = double2>
__device__ __forceinline__ P tile_chunk(const char* tile, int ro, int i) {
  return *reinterpret_cast<const P*>(tile + (ROT ? (ro ^ (i * CB)) : ro + i * CB));
}

// One pass of every group of the workgroup over tiles [tile_begin, tile_end).
//   xv      the point at which the segment's losses are evaluated
//   g, J    outputs: gradient (GRAD) and loss sum of the segment's observations inside those tiles
//   pos     in/out: position in the segment's list (first entry with idx >= tile_begin*TILE on entry)
//   active  group-uniform; inactive groups only take part in staging and barriers
//
// L2 = true is the same walk WITHOUT the LDS tile: the group reads the opposing vectors of its observations straight from memory
// (one 16-byte load per lane and 2G components) and [tile_begin, tile_end) is one range that is walked in a single go, with no
// barrier.  It is what the phase-aligned pass kernels below run: when every group in flight walks its sorted list through the same
// super-tile at the same time, those reads hit the 4 MB L2 of the XCD (~30 TB/s) instead of the Infinity Cache / HBM (6.5-8 TB/s,
// profiles/r02_ubench_gather.txt).
template <int G, int R, int NW, int TILE, int LOSS, bool GRAD, bool L2 = false, bool ROTK = false, class ST = double>
__device__ __forceinline__ void tiled_pass(const TiledArgs& a, char* lds, const Vec<G, R>& xv, Vec<G, R>& g, double& J,
                                           bool active, int64_t& pos, int64_t end, int tile_begin, int tile_end,
                                           const LossDesc& segloss, int lane, int j, int rot = 0) {
  constexpr bool ROT = ROTK && !L2 && tile_rot<G, R>(); // register i holds chunk i ^ rot (see tile_rot)
  static_assert(L2 || sizeof(ST) == 8, "the LDS tile has no float form");
  using P = typename Pair<ST>::type;            // a lane's chunk as the storage holds it: 16 bytes (double) or 8 (float)
  constexpr int PB = (int)sizeof(P);
  constexpr int ROWB = L2 ? G * R * (int)sizeof(ST) : tile_row_stride<G, R, ROT>();
  constexpr int CB = G * PB;                    // bytes per chunk row of the group
  const int jrot = j * PB + (ROT ? rot * CB : 0);
  // the whole batch of G observations per step (below) for every model but the uniform QuadLoss one: its two-observation step already
  // keeps eight LDS reads in flight on two interleaved chains (the four-observation step there: C2 15.70 -> 19.05 ms, LABNOTES round 4)
  constexpr bool FOUR = (G == 4 || G == 8) && LOSS != 0;
  const double two_scale = 2 * segloss.scale;
  J = 0.0;
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) g.v[i] = make_double2(0.0, 0.0);
  }
  const int32_t* __restrict__ idx = a.idx;
  const ST* __restrict__ vals = reinterpret_cast<const ST*>(a.vals); // (float storage: floats behind the double* field)
  // current batch: lane j of the group holds entry pos + j.  Batch loads are UNCONDITIONAL (address clamped
  // into the segment, validity applied when the entry is used) so that the compiler can keep the prefetch of
  // the next batch in flight with a counted s_waitcnt instead of draining the queue at every branch merge.
  const int64_t last = end > 0 ? end - 1 : 0; // idx/vals always hold at least one element
  constexpr bool UDESC = FOUR && loss_mode(LOSS) == 2 && !L2; // descriptor ids travel with the entries (see TiledArgs::descid)
  const uint8_t* __restrict__ descid = a.descid;
  const bool have_ids = UDESC && descid != nullptr;    // uniform
  const char* udesc_lds = lds + tile_lds_bytes<G, R, TILE>(); // the kernel staged the distinct descriptors there
  auto load_entry = [&](int64_t p, int& c, double& av, int& did) {
    const int64_t q = p < last ? p : last;
    c = idx[q];
    av = vals[q];
    did = 0;
    if constexpr (UDESC) {
      if (have_ids) did = descid[q];
    }
  };
  int cb, db;
  double ab;
  load_entry(pos + j, cb, ab, db);
  if (!(active && pos + j < end)) cb = 0x7fffffff;
  // Phase gate (L2 only; a.gate rows, 0 = off).  The groups of a wave start together but drift apart in rows (a step consumes G
  // observations, whose row gaps are random), and the band of rows the groups in flight read from grows past what the L2 holds.  With the
  // gate, a group whose next observation lies more than a.gate rows past the wave's TRAILING group (the least next-observation row among
  // the groups still walking) sits the step out.  A step is skipped whole -- pos, the batch and every accumulator stay as they are -- so
  // each accumulator still receives the same terms in the same order: the bits do not depend on the gate.  The trailing group is never
  // held back, so the walk ends whatever the order of the list inside a tile.
  // (The same gate as a wave reduction over the lanes still inside a divergent loop -- the gate-off loop's shape, 4 fewer VGPRs -- did not
  // pay: Y half-step 133.7 ms at any gate width against 129.9 without it, LABNOTES round 7.)
  const int gate = L2 ? a.gate : 0; // wave-uniform
  for (int t = tile_begin; t < (L2 ? tile_begin + 1 : tile_end); ++t) {
    const int64_t lo = (int64_t)t * TILE;
    const int64_t hi_ = L2 ? (int64_t)tile_end * TILE : lo + TILE;
    const int64_t hi = hi_ < a.n_other ? hi_ : a.n_other;
    // L2, two-observation step of the uniform QuadLoss model: sup_base is the wave-uniform address of the super-tile's first row, and an
    // observation's vector sits at a 32-BIT byte offset from it, (row - lo) * ROWB + j * 16, instead of a 64-bit multiply-add per
    // observation (what kept the rank-64 gradient kernel a wave per SIMD lower, see pass_waves_per_simd).  row >= lo for every consumed
    // entry -- pos starts at the first entry of the super-tile and the lists are in tile order -- and glrm_setup_blocked refuses a
    // super-tile of 4 GiB or more.
    const char* const mem = L2 ? reinterpret_cast<const char*>(a.other) : lds;
    const char* const sup_base = mem + (L2 ? lo * ROWB : 0);
    if constexpr (!L2) {
      __syncthreads(); // everybody is done with the previous tile
      dma_tile_all<G, R, NW, ROT>(a.other, lo, hi, lds, (int)(threadIdx.x >> 6), lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    bool done = !active;
    for (;;) {
      if (gate > 0) {
        // Every lane of the wave runs this loop until all groups are done (with the gate on, no lane leaves it alone), so the minimum
        // can be formed over all 64 lanes.  Each lane offers its GROUP's next row c0 (its first lane's entry), never its own: the lists
        // are only ordered by tile, so another lane of the group may hold a smaller row.  A done group offers INT_MAX, a walking one at
        // most INT_MAX - 1 (c0 is INT_MAX past the end of its list).
        const int c0 = group_bcast_i32<G>(cb, 0, lane);
        int trail = done ? 0x7fffffff : min(c0, 0x7ffffffe);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) trail = min(trail, __shfl_xor(trail, o, 64));
        if (trail == 0x7fffffff) break; // every group of the wave is done (wave-uniform)
        // The trailing group has c0 - trail <= 0 and steps, and a step either consumes an observation or ends the group's walk: the loop
        // ends for any list the family admits.  A waiting (or done) lane's iteration changes none of its own values; the volatile asm
        // keeps the compiler from taking that for an endless loop without side effects (undefined behaviour it may assume away: it then
        // drops the gate or miscompiles the loop).
        if (done || (c0 < (int)hi && c0 - trail > gate)) { // 0 <= trail <= c0 < hi: no overflow
          asm volatile("" ::: "memory");
          continue;
        }
      } else if (done) {
        break;
      }
      int cn, dn; // prefetch the next batch while this one is consumed
      double an;
      load_entry(pos + G + j, cn, an, dn);
      const bool next_ok = pos + G + j < end;
      int nproc = 0;
      // Two observations of the batch per step.  Every lane forms its partial dot products for BOTH observations;
      // the first butterfly step is a reduce-scatter (even lanes keep observation u0, odd lanes u0+1), the remaining
      // steps reduce one value; loss and derivative are then evaluated once per lane for "its" observation and the
      // derivative of the other one comes back with one DPP move.  ~30 % (gradient pass) / ~45 % (trial pass) fewer
      // VALU instructions than one observation per step.
      const bool odd = (j & 1) != 0;
      if constexpr (FOUR) {
        // Losses with transcendental or branchy formulas (everything but the uniform QuadLoss model), G = 4 or 8: the whole
        // batch of G observations per step, one loss evaluation per LANE.  The partial dot products of all G observations are
        // reduce-scattered in log2(G) butterfly steps (same pairings as below, so the same bits), lane u evaluates observation
        // u, and the G derivatives come back by broadcasts.  The opposing vectors are re-read from LDS for the gradient update
        // instead of being kept live across the loss evaluation (which is what made this kernel spill).
        int c[G];
        bool ok[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          c[u] = group_bcast_i32<G>(cb, u, lane);
          ok[u] = (u == 0 || ok[u - 1]) && c[u] < (int)hi; // c == INT_MAX past the end of the segment
        }
        if (ok[0]) {
          const char* rp[G]; // L2: address of the lane's first chunk
          int ro[G];         // LDS tile: its byte offset in the tile
          double p[G];
          bool mine = false;
#pragma unroll
          for (int u = 0; u < G; ++u) {
            if constexpr (L2) rp[u] = mem + j * PB + (int64_t)(ok[u] ? c[u] : c[0]) * ROWB;
            else ro[u] = ((ok[u] ? c[u] : c[0]) - (int)lo) * ROWB + jrot;
            mine = (j == u) ? ok[u] : mine;
            p[u] = 0.0;
          }
          // chunk-major: the G reads of a chunk are issued together and feed G INDEPENDENT fma chains (round 4: the observation-major
          // order compiled to sixteen serialized LDS round trips per step -- one read in flight, `s_waitcnt lgkmcnt(0)` after each --
          // because the scheduler minimises registers in a kernel at its VGPR cap).  Every p[u] still adds its chunks in ascending order.
#pragma unroll
          for (int i = 0; i < R / 2; ++i) {
            P yv[G];
#pragma unroll
            for (int u = 0; u < G; ++u) yv[u] = L2 ? *reinterpret_cast<const P*>(rp[u] + i * CB) : tile_chunk<ROT, CB, P>(mem, ro[u], i);
#pragma unroll
            for (int u = 0; u < G; ++u) {
              p[u] = fma(xv.v[i].x, (double)yv[u].x, p[u]);
              p[u] = fma(xv.v[i].y, (double)yv[u].y, p[u]);
            }
          }
          const bool hi2 = (j & 2) != 0;
          double q[G / 2]; // q[i]: observation 2i + odd, summed over lanes {j, j^1}
#pragma unroll
          for (int i = 0; i < G / 2; ++i) q[i] = (odd ? p[2 * i + 1] : p[2 * i]) + dpp_f64<DPP_XOR1>(odd ? p[2 * i] : p[2 * i + 1]);
          double dot;
          if constexpr (G == 4) {
            dot = (hi2 ? q[1] : q[0]) + dpp_f64<DPP_XOR2>(hi2 ? q[0] : q[1]); // observation j
          } else {
            const bool hi4 = (j & 4) != 0;
            const double r0 = (hi2 ? q[1] : q[0]) + dpp_f64<DPP_XOR2>(hi2 ? q[0] : q[1]); // observation (j & 3)
            const double r1 = (hi2 ? q[3] : q[2]) + dpp_f64<DPP_XOR2>(hi2 ? q[2] : q[3]); // observation 4 + (j & 3)
            dot = (hi4 ? r1 : r0) + swizzle_xor_f64<4>(hi4 ? r0 : r1);                     // observation j
          }
          double L, dL;
          if constexpr (LOSS == 0) { // one QuadLoss descriptor (src/losses.jl:144,146)
            const double dq = dot - ab;
            L = segloss.scale * (dq * dq);
            dL = dq * two_scale;
          } else if constexpr (loss_mode(LOSS) == 1) {
            loss_both<GRAD, loss_trig(LOSS)>(segloss, dot, ab, L, dL);
          } else {
            LossDesc lo_;
            if (have_ids) { // 32-byte descriptor from the LDS table (glrm_loss layout: kind, dim, scale, p0, p1)
              const char* dp = udesc_lds + db * 32;
              const int2 kd = *reinterpret_cast<const int2*>(dp);
              const double sc = *reinterpret_cast<const double*>(dp + 8);
              const double2 pp = *reinterpret_cast<const double2*>(dp + 16);
              lo_ = LossDesc{kd.x, sc, pp.x, pp.y};
            } else {
              lo_ = load_loss(a.losses, mine ? cb : c[0]);
            }
            loss_both<GRAD, loss_trig(LOSS)>(lo_, dot, ab, L, dL);
          }
          if (!mine) {
            L = 0.0;
            dL = 0.0;
          }
          J += L; // every observation once
          if (GRAD) {
            asm volatile("" ::: "memory"); // the reads below are real re-reads, not the values of the first ones kept in VGPRs
            double dv[G]; // observations past the tile window carry a zero derivative
#pragma unroll
            for (int u = 0; u < G; ++u) dv[u] = group_bcast_f64<G>(dL, u, lane);
#pragma unroll
            for (int i = 0; i < R / 2; ++i) { // chunk-major like the dot products; every component still adds its terms in list order
              P yv[G];
#pragma unroll
              for (int u = 0; u < G; ++u) yv[u] = L2 ? *reinterpret_cast<const P*>(rp[u] + i * CB) : tile_chunk<ROT, CB, P>(mem, ro[u], i);
#pragma unroll
              for (int u = 0; u < G; ++u) {
                g.v[i].x = fma(dv[u], (double)yv[u].x, g.v[i].x);
                g.v[i].y = fma(dv[u], (double)yv[u].y, g.v[i].y);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < G; ++u) nproc += ok[u] ? 1 : 0;
          if (!ok[G - 1]) done = true;
        } else {
          done = true;
        }
      } else {
#pragma unroll
      for (int u0 = 0; u0 < G; u0 += 2) {
        const int c0 = group_bcast_i32<G>(cb, u0, lane);
        const int c1 = group_bcast_i32<G>(cb, u0 + 1, lane);
        const bool ok0 = !done && c0 < (int)hi; // c == INT_MAX past the end of the segment
        const bool ok1 = ok0 && c1 < (int)hi;
        if (ok0) {
          P y0[R / 2], y1[R / 2];
          if constexpr (L2) {
            const int c1v = ok1 ? c1 : c0; // a clamped lane re-reads the row of a valid entry
            const char *rp0, *rp1;
            if constexpr (LOSS == 0) {
              rp0 = sup_base + ((uint32_t)(c0 - (int)lo) * (uint32_t)ROWB + (uint32_t)(j * PB));
              rp1 = sup_base + ((uint32_t)(c1v - (int)lo) * (uint32_t)ROWB + (uint32_t)(j * PB));
            } else { // rank 128 with a loss per column: the 32-bit form costs these kernels SGPR spills
              rp0 = mem + (int64_t)c0 * ROWB + j * PB;
              rp1 = mem + (int64_t)c1v * ROWB + j * PB;
            }
#pragma unroll
            for (int i = 0; i < R / 2; ++i) y0[i] = *reinterpret_cast<const P*>(rp0 + i * CB);
#pragma unroll
            for (int i = 0; i < R / 2; ++i) y1[i] = *reinterpret_cast<const P*>(rp1 + i * CB);
          } else {
            const int ro0 = (c0 - (int)lo) * ROWB + jrot, ro1 = ((ok1 ? c1 : c0) - (int)lo) * ROWB + jrot;
#pragma unroll
            for (int i = 0; i < R / 2; ++i) y0[i] = tile_chunk<ROT, CB>(mem, ro0, i);
#pragma unroll
            for (int i = 0; i < R / 2; ++i) y1[i] = tile_chunk<ROT, CB>(mem, ro1, i);
          }
          double p0 = 0.0, p1 = 0.0;
#pragma unroll
          for (int i = 0; i < R / 2; ++i) {
            p0 = fma(xv.v[i].x, (double)y0[i].x, p0);
            p0 = fma(xv.v[i].y, (double)y0[i].y, p0);
          }
#pragma unroll
          for (int i = 0; i < R / 2; ++i) {
            p1 = fma(xv.v[i].x, (double)y1[i].x, p1);
            p1 = fma(xv.v[i].y, (double)y1[i].y, p1);
          }
          const double keep = odd ? p1 : p0, send = odd ? p0 : p1;
          double dot = keep + dpp_f64<DPP_XOR1>(send); // lane pair sum for observation u0 + odd
          // remaining butterfly steps must keep the lane parity (mirrors would mix the two observations)
          if constexpr (G >= 4) dot += dpp_f64<DPP_XOR2>(dot);
          if constexpr (G >= 8) dot += swizzle_xor_f64<4>(dot);
          if constexpr (G >= 16) dot += swizzle_xor_f64<8>(dot);
          double av = pair_bcast_f64<G>(ab, u0, lane);
          double L, dL;
          if constexpr (LOSS == 0) {
            const double d = dot - av;
            L = segloss.scale * (d * d);
            dL = d * two_scale; // == (2*d)*scale bit for bit: doubling is exact
          } else if constexpr (loss_mode(LOSS) == 1) {
            loss_both<GRAD, loss_trig(LOSS)>(segloss, dot, av, L, dL);
          } else {
            const LossDesc lo_ = load_loss(a.losses, odd ? (ok1 ? c1 : c0) : c0);
            loss_both<GRAD, loss_trig(LOSS)>(lo_, dot, av, L, dL);
          }
          if (odd && !ok1) {
            L = 0.0;
            dL = 0.0;
          }
          J += L; // every observation is accumulated by G/2 lanes; the caller rescales the group sum by 2/G (exact)
          if (GRAD) {
            // list order: u0 first, then u0+1.  Even lanes hold the derivative of u0, odd lanes that of u0+1: two quad
            // broadcasts ([0,0,2,2] / [1,1,3,3]) instead of an exchange plus two selects
            const double d0 = group_bcast_f64<2>(dL, 0, lane), d1 = group_bcast_f64<2>(dL, 1, lane);
#pragma unroll
            for (int i = 0; i < R / 2; ++i) {
              g.v[i].x = fma(d0, (double)y0[i].x, g.v[i].x);
              g.v[i].y = fma(d0, (double)y0[i].y, g.v[i].y);
            }
#pragma unroll
            for (int i = 0; i < R / 2; ++i) {
              g.v[i].x = fma(d1, (double)y1[i].x, g.v[i].x);
              g.v[i].y = fma(d1, (double)y1[i].y, g.v[i].y);
            }
          }
          nproc += ok1 ? 2 : 1;
          if (!ok1) done = true;
        } else {
          done = true;
        }
      }
      }
      pos += nproc;
      if (!done) { // the whole batch was consumed: continue with the prefetched one
        cb = next_ok ? cn : 0x7fffffff;
        ab = an;
        db = dn;
      } else if (nproc > 0) { // stopped inside the batch: re-anchor the batch at the new position
        load_entry(pos + j, cb, ab, db);
        if (!(pos + j < end)) cb = 0x7fffffff;
      }
    }
  }
  J = group_sum<G>(J) * (FOUR ? 1.0 : 2.0 / G); // two per step: lanes hold parity-partial sums, each observation counted G/2 times
}

// distinct loss descriptors -> LDS behind the tile (read after the first tile barrier of tiled_pass); see TiledArgs::descid
template <int G, int R, int NW, int TILE, int LOSS>
__device__ __forceinline__ void stage_udesc(const TiledArgs& a, char* lds) {
  if constexpr (loss_mode(LOSS) == 2) {
    if (a.descid) {
      const int words = a.n_udesc * 8; // 32 bytes each
      const int* src = reinterpret_cast<const int*>(a.udesc);
      int* dst = reinterpret_cast<int*>(lds + tile_lds_bytes<G, R, TILE>());
      for (int w = threadIdx.x; w < words; w += NW * 64) dst[w] = src[w];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// X half-step (and any sweep whose segments are plentiful): whole sweep in one kernel.
// Workgroup = NW waves, SPB = NW*64/G segments; each pass streams the WHOLE opposing factor through LDS.
// FIXED = true is the SparseProxGradParams step (one gradient pass, x <- prox(x - (alpha/l) g), no line search); it is a
// separate instantiation so that the line-search kernel keeps its register budget.
// ROUNDS = true (round 4, the default): the kernel makes the gradient pass and the FIRST trial; a segment whose first trial is rejected
// leaves its state -- gradient, J_old, shrunk step size, next trial point -- in the pass buffers (gsum, jold, alpha, trial, ntrial,
// active) and its id in actlist_out, and the host runs the remaining trials as rounds of (tiled_col_pass_kernel<GRAD = false, ROWS> over
// the listed segments, col_decide_kernel): only workgroups made of still-searching rows stage tiles again.  Same sums, same bits.
template <int G, int R, int NW, int TILE, int LOSS, bool FIXED, bool ROUNDS = false, bool VR = false>
__global__ void __launch_bounds__(NW * 64, 4) tiled_sweep_kernel(const TiledArgs a) {
  constexpr int KP = G * R, NGW = 64 / G, SPB = NW * NGW;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane % G, gi = lane / G;
  const int64_t slot = (int64_t)blockIdx.x * SPB + wave * NGW + gi;
  const bool have = slot < a.nseg;
  const int64_t seg = (have && a.segperm) ? (int64_t)a.segperm[slot] : slot; // segments of similar length share a wave (skewed data)
  const int64_t beg = have ? a.ptr[seg] : 0, end = have ? a.ptr[seg + 1] : 0;
  const int64_t gseg = a.own_offset + (have ? seg : 0);
  double2* ownp = reinterpret_cast<double2*>(a.own + gseg * KP);
  const int ntiles = (int)((a.n_other + TILE - 1) / TILE);
  stage_udesc<G, R, NW, TILE, LOSS>(a, lds);

  Vec<G, R> g, xn;
  const RegDesc rd = load_reg(a.regs, (a.reg_single || !have) ? 0 : seg);
  LossDesc segloss = LossDesc{0, 1.0, 0.0, 0.0};
  if constexpr (loss_mode(LOSS) != 2) segloss = load_loss(a.losses, (a.loss_by_segment && have) ? gseg : 0);
  const double l = (double)(end - beg) + 1.0;

  double Jold;
  int64_t pos = beg;
  {
    Vec<G, R> x;
#pragma unroll
    for (int i = 0; i < R / 2; ++i) x.v[i] = have ? ownp[i * G + j] : make_double2(0.0, 0.0);
    tiled_pass<G, R, NW, TILE, LOSS, true>(a, lds, x, g, Jold, have, pos, end, 0, ntiles, segloss, lane, j);
    if constexpr (FIXED) { // src/algorithms/sparse_proxgrad.jl:72-78: g *= -alpha/l; x += g; prox!(r, x, alpha/l)
      const double s = a.fixed_alpha / l;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        xn.v[i].x = x.v[i].x + g.v[i].x * (-s);
        xn.v[i].y = x.v[i].y + g.v[i].y * (-s);
      }
      reg_prox<G, R, VR>(rd, xn, s, j, a.k);
      if (have) {
#pragma unroll
        for (int i = 0; i < R / 2; ++i) ownp[i * G + j] = xn.v[i];
      }
      return;
    }
    Jold += reg_eval<G, R, VR>(rd, x, j, a.k);
  }

  // Backtracking line search.  The current point is NOT kept in registers across the trial passes: it is re-read
  // from the factor array when the next trial point is formed (32 B per lane per trial) and the accepted point is
  // written back at once, which frees R VGPRs per lane inside the pass.
  double alpha = have ? a.alpha[seg] : 0.0;
  int ntrials = 0;
  bool accepted = false;
  bool searching = have && alpha > a.min_stepsize;
  bool first = true;
  while ((!ROUNDS || first) && __syncthreads_or(searching ? 1 : 0)) {
    first = false;
    const double s = alpha / l;
#pragma unroll
    for (int i = 0; i < R / 2; ++i) {
      const double2 xi = have ? ownp[i * G + j] : make_double2(0.0, 0.0);
      xn.v[i].x = fma(-s, g.v[i].x, xi.x);
      xn.v[i].y = fma(-s, g.v[i].y, xi.y);
    }
    reg_prox<G, R, VR>(rd, xn, s, j, a.k);
    double Jn;
    Vec<G, R> dummy;
    pos = beg;
    tiled_pass<G, R, NW, TILE, LOSS, false>(a, lds, xn, dummy, Jn, searching, pos, end, 0, ntiles, segloss, lane, j);
    Jn += reg_eval<G, R, VR>(rd, xn, j, a.k);
    if (searching) {
      ++ntrials;
      if (Jn < Jold) {
#pragma unroll
        for (int i = 0; i < R / 2; ++i) ownp[i * G + j] = xn.v[i];
        alpha *= 1.05;
        Jold = Jn;
        accepted = true;
        searching = false;
      } else {
        alpha *= .7;
        if (alpha < a.min_stepsize) {
          alpha = a.min_stepsize * 1.1;
          searching = false;
        } else if (!(alpha > a.min_stepsize)) {
          searching = false; // `while alpha > min_stepsize` (proxgrad.jl:136): alpha == min_stepsize ends the search (min_stepsize = 0: alpha underflowed to 0)
        }
      }
    }
  }
  if constexpr (ROUNDS) {
    if (have) {
      if (searching) { // first trial rejected, step size still above the minimum: hand the segment over to the rounds
        const double s = alpha / l;
#pragma unroll
        for (int i = 0; i < R / 2; ++i) {
          const double2 xi = ownp[i * G + j];
          xn.v[i].x = fma(-s, g.v[i].x, xi.x);
          xn.v[i].y = fma(-s, g.v[i].y, xi.y);
        }
        reg_prox<G, R, VR>(rd, xn, s, j, a.k);
        double2* gp = reinterpret_cast<double2*>(a.gsum + seg * (int64_t)KP);
        double2* tp = reinterpret_cast<double2*>(a.trial + seg * (int64_t)KP);
#pragma unroll
        for (int i = 0; i < R / 2; ++i) {
          gp[i * G + j] = g.v[i];
          tp[i * G + j] = xn.v[i];
        }
        if (j == 0) {
          a.alpha[seg] = alpha;
          a.jold[seg] = Jold;
          a.ntrial[seg] = ntrials;
          a.active[seg] = 1;
          const unsigned slot_out = atomicAdd(a.nactive, 1u);
          a.actlist_out[slot_out] = (int32_t)seg;
        }
        return; // col_decide_kernel books trials / accepts when the segment's search ends
      }
      if (j == 0) a.active[seg] = 0;
    }
  }
  if (have && j == 0) {
    a.alpha[seg] = alpha;
    if (a.obj) a.obj[gseg] = Jold;
    if (a.trials) {
      a.trials[seg] += ntrials;
      a.accepts[seg] += accepted ? 1 : 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Y half-step when columns are few and long: rows are split into NSUP super-tiles, one workgroup per
// (column group, super-tile); partial sums are reduced in super-tile order by col_reduce_kernel /
// col_decide_kernel, and the line search runs as rounds of (pass, decide) launches.

template <int G>
__device__ __forceinline__ int64_t lower_bound_idx(const int32_t* idx, int64_t b, int64_t e, int64_t key) {
  while (b < e) {
    const int64_t mid = b + ((e - b) >> 1);
    if ((int64_t)idx[mid] < key) b = mid + 1; else e = mid;
  }
  return b;
}

// GRAD = true: pass 1 (gradient + loss partials at the current point a.own);
// GRAD = false: trial pass (loss partials at a.trial for the still-active segments).
//
// L2 = true: the phase-aligned gather pass (no LDS tile, tiled_pass<..., L2>).  One launch covers ONE super-tile (a.sup_fixed) and
// a slice [a.seg_begin, a.seg_begin + a.nseg_slice) of the segments that is at most what the chip holds at once, so every group of
// the launch starts its walk through the super-tile at the same moment; the host issues the launches super-tile by super-tile.
//
// Waves per SIMD an instantiation is BUILT for (the second launch bound).  The LDS-tiled kernels: 4.  The phase-aligned ones take whatever
// their registers allow (1), except the GRADIENT pass of the uniform-QuadLoss model at rank 64 and 32: with 32-bit gather offsets
// (tiled_pass) it fits 128 VGPRs without scratch (132 unbound at rank 64), i.e. 4 waves per SIMD instead of 3, and slice_capacity
// (glrm_blocked.hip) turns the occupancy into columns per launch -- more columns walking the same window of the opposing factor on an XCD
// (C4 Y half-step 114.1 -> 110.8 ms).  The trial pass stays at what its 98 / 89 VGPRs give, 4 / 5 waves: held to 96 VGPRs and 5 waves the
// rank-64 one is clean too, but LOSES (113.0 ms; LABNOTES "phase-aligned passes at 4 / 5 waves per SIMD").  Every other instantiation
// spills at such bounds (rank 128: 20 / 12 B, LOSS != 0: 28-252 B) and keeps its own; no kernel gains scratch or loses a wave.
//
// ST = float (glrm_options.storage = 1; L2 = true only, instantiated in glrm_blocked_f32.hip): a.vals, a.own and a.other hold floats
// (leading dimension KP floats, the same zero padding), a lane's chunk is one 8-byte float2 load widened at the fma, the gather offset is
// (row - lo) * KP * 4 + j * 8; part, gsum, trial, jold, alpha, every accumulator and every loss evaluation stay fp64, so every sum adds
// the terms of the fp64 kernel in its order.  The bound of the float kernels comes from their own registers, and those are NOT half the
// fp64 ones: the compiler widens a gathered float2 once and keeps the doubles for the dot product and the gradient update, so unbound the
// rank-64 / rank-32 QuadLoss gradient kernels take 132 / 128 VGPRs and the trial kernels 96 / 88 (fp64: 132 / 128 and 98 / 89).  The
// gradient pair is built for 4 waves per SIMD like its fp64 twin (128 VGPRs, no scratch); at 5 both spill (148 / 160 B), and forcing the
// second widening (a register barrier on the floats between dot product and update) spills at 4 already.  The trial kernels take what
// their registers give, 5 waves.  GLRM_BLOCKED_F32_GRAD_WAVES: the bound of that pair in a variant build (tests/perf/bench_storage_blocked.py
// measures 1 = unbound, 3 waves, against 4).  profiles/storage_f32_blocked_resusage.txt, DESIGN 4.13.
#ifndef GLRM_BLOCKED_F32_GRAD_WAVES
#define GLRM_BLOCKED_F32_GRAD_WAVES 4
#endif
template <int G, int R, int LOSS, bool GRAD>
constexpr int pass_waves_per_simd_f32() { return (LOSS == 0 && R == 8 && (G == 8 || G == 4) && GRAD) ? GLRM_BLOCKED_F32_GRAD_WAVES : 1; }

template <int G, int R, int LOSS, bool GRAD, bool L2, class ST = double>
constexpr int pass_waves_per_simd() {
  if (!L2) return 4;
  if (sizeof(ST) == 4) return pass_waves_per_simd_f32<G, R, LOSS, GRAD>();
  if (LOSS == 0 && R == 8 && (G == 8 || G == 4) && GRAD) return 4;
  return 1;
}

template <int G, int R, int NW, int TILE, int LOSS, bool GRAD, bool L2 = false, bool ROWS = false, class ST = double>
__global__ void __launch_bounds__(NW * 64, (pass_waves_per_simd<G, R, LOSS, GRAD, L2, ST>())) tiled_col_pass_kernel(const TiledArgs a) {
  using P = typename Pair<ST>::type;
  constexpr int KP = G * R, NGW = 64 / G, SPB = NW * NGW, PSTRIDE = KP + 2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane % G, gi = lane / G;
  const int64_t slot = (L2 ? a.seg_begin : 0) + (int64_t)blockIdx.x * SPB + wave * NGW + gi;
  const int sup = L2 ? a.sup_fixed : a.sup0 + (int)blockIdx.y;
  bool have = slot < (L2 ? a.seg_begin + a.nseg_slice : (a.npass > 0 ? a.npass : a.nseg));
  const int64_t seg = (have && a.segperm) ? (int64_t)a.segperm[slot] : slot; // which column a group works on does not change any sum
  if (!GRAD && have) have = a.active[seg] != 0;
  if (!GRAD && !__syncthreads_or(have ? 1 : 0)) return; // nothing left to evaluate in this column group
  if constexpr (!L2) stage_udesc<G, R, NW, TILE, LOSS>(a, lds);
  const int64_t beg = have ? a.ptr[seg] : 0, end = have ? a.ptr[seg + 1] : 0;
  const int64_t gseg = a.own_offset + (have ? seg : 0);
  const int ntiles = (int)((a.n_other + TILE - 1) / TILE);
  const int tb = sup * a.tiles_per_sup;
  const int te = tb + a.tiles_per_sup < ntiles ? tb + a.tiles_per_sup : ntiles;
  // ROWS: the trial rounds of the row view (the row sweep's own passes read padded tiles without rotation: the same bits here)
  constexpr bool ROT = !ROWS && !L2 && LOSS != 0 && tile_rot<G, R>();
  const int rot = ROT ? tile_rot_of(gseg) : 0; // register i <-> chunk i ^ rot (conflict-free tile reads, see tile_rot)
  Vec<G, R> x, g;
  if constexpr (GRAD && sizeof(ST) == 4) { // the current point as the storage holds it; the trial point below is fp64 in both storages
    const P* xp = reinterpret_cast<const P*>(reinterpret_cast<const ST*>(a.own) + gseg * KP);
#pragma unroll
    for (int i = 0; i < R / 2; ++i) x.v[i] = have ? widen(xp[i * G + j]) : make_double2(0.0, 0.0);
  } else {
    const double2* xp = reinterpret_cast<const double2*>(GRAD ? a.own + gseg * KP : a.trial + (have ? seg : 0) * (int64_t)KP);
#pragma unroll
    for (int i = 0; i < R / 2; ++i) x.v[i] = have ? xp[(i ^ rot) * G + j] : make_double2(0.0, 0.0);
  }
  LossDesc segloss = LossDesc{0, 1.0, 0.0, 0.0};
  if constexpr (loss_mode(LOSS) != 2) segloss = load_loss(a.losses, (a.loss_by_segment && have) ? gseg : 0);
  int64_t pos = 0; // first entry of the super-tile: from the start table where the side has one (L2), else the search
  if (have) {
    if (L2 && a.suppos) pos = beg + a.suppos[seg * (int64_t)a.nsup + sup];
    else pos = lower_bound_idx<G>(a.idx, beg, end, (int64_t)tb * TILE);
  }
  double J;
  tiled_pass<G, R, NW, TILE, LOSS, GRAD, L2, ROT, ST>(a, lds, x, g, J, have, pos, end, tb, te, segloss, lane, j, rot);
  if (have) {
    double* p = a.part + ((int64_t)seg * a.nsup + sup) * PSTRIDE;
    if (GRAD) {
#pragma unroll
      for (int i = 0; i < R / 2; ++i) *reinterpret_cast<double2*>(p + (i ^ rot) * 2 * G + 2 * j) = g.v[i];
    }
    if (j == 0) p[KP] = J;
  }
}

// After pass 1: reduce the partials in super-tile order, J_old = loss + r(y), first trial point.
// ST = float (the phase-aligned passes of a float handle): a.own holds floats, and the trial point is rounded to the value the storage
// will hold right after the prox -- before it is written to `trial` and before col_decide evaluates r on it -- so that the search
// compares objectives of stored factors and an accepted point is stored exactly.  No fixed_alpha branch (refused for f32).
template <int G, int R, bool VR = false, class ST = double>
__global__ void __launch_bounds__(256) col_reduce_kernel(const TiledArgs a) {
  using P = typename Pair<ST>::type;
  constexpr int KP = G * R, NGW = 64 / G, PSTRIDE = KP + 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane % G, gi = lane / G;
  const int64_t seg = ((int64_t)blockIdx.x * 4 + wave) * NGW + gi;
  if (seg >= a.nseg) return; // group-uniform
  if (a.long_from > 0 && a.ptr && a.ptr[seg + 1] - a.ptr[seg] >= a.long_from) return; // swept by the gather sweep beside the passes
  const int64_t gseg = a.own_offset + seg;
  Vec<G, R> g, y, yn;
  double J = 0.0;
#pragma unroll
  for (int i = 0; i < R / 2; ++i) g.v[i] = make_double2(0.0, 0.0);
  for (int s = 0; s < a.nsup; ++s) {
    const double* p = a.part + ((int64_t)seg * a.nsup + s) * PSTRIDE;
#pragma unroll
    for (int i = 0; i < R / 2; ++i) {
      const double2 v = *reinterpret_cast<const double2*>(p + i * 2 * G + 2 * j);
      g.v[i].x += v.x;
      g.v[i].y += v.y;
    }
    J += p[KP];
  }
  if (a.eval_only) {
    if (j == 0 && a.obj) a.obj[gseg] = J;
    return;
  }
  const P* yp = reinterpret_cast<const P*>(reinterpret_cast<const ST*>(a.own) + gseg * KP);
#pragma unroll
  for (int i = 0; i < R / 2; ++i) y.v[i] = widen(yp[i * G + j]);
  const RegDesc rd = load_reg(a.regs, a.reg_single ? 0 : seg);
  if (sizeof(ST) == 8 && a.fixed_alpha > 0.0) { // SparseProxGradParams step on this segment, no trial rounds
    const double l0 = (double)(a.ptr ? a.ptr[seg + 1] - a.ptr[seg] : a.dense_len) + 1.0;
    const double s0 = a.fixed_alpha / l0;
#pragma unroll
    for (int i = 0; i < R / 2; ++i) {
      yn.v[i].x = y.v[i].x + g.v[i].x * (-s0);
      yn.v[i].y = y.v[i].y + g.v[i].y * (-s0);
    }
    reg_prox<G, R, VR>(rd, yn, s0, j, a.k);
    double2* yw = reinterpret_cast<double2*>(a.own + gseg * KP);
#pragma unroll
    for (int i = 0; i < R / 2; ++i) yw[i * G + j] = yn.v[i];
    if (j == 0) a.active[seg] = 0;
    return;
  }
  const double Jold = J + reg_eval<G, R, VR>(rd, y, j, a.k);
  if (a.jloss && j == 0) a.jloss[seg] = J;
  const double alpha = a.alpha[seg];
  const double l = (double)(a.ptr ? a.ptr[seg + 1] - a.ptr[seg] : a.dense_len) + 1.0;
  const bool searching = alpha > a.min_stepsize;
  const double s = alpha / l;
#pragma unroll
  for (int i = 0; i < R / 2; ++i) {
    yn.v[i].x = fma(-s, g.v[i].x, y.v[i].x);
    yn.v[i].y = fma(-s, g.v[i].y, y.v[i].y);
  }
  reg_prox<G, R, VR>(rd, yn, s, j, a.k);
  if constexpr (sizeof(ST) == 4) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) yn.v[i] = make_double2(stored<ST>(yn.v[i].x), stored<ST>(yn.v[i].y));
  }
  double2* gp = reinterpret_cast<double2*>(a.gsum + seg * (int64_t)KP);
  double2* tp = reinterpret_cast<double2*>(a.trial + seg * (int64_t)KP);
#pragma unroll
  for (int i = 0; i < R / 2; ++i) {
    gp[i * G + j] = g.v[i];
    tp[i * G + j] = yn.v[i];
  }
  if (j == 0) {
    a.jold[seg] = Jold;
    a.active[seg] = searching ? 1 : 0;
    a.ntrial[seg] = 0;
    if (a.obj) a.obj[gseg] = Jold;
    if (searching) {
      const unsigned slot = atomicAdd(a.nactive, 1u);
      if (a.actlist_out) a.actlist_out[slot] = (int32_t)seg;
    }
  }
}

// After a trial pass: J' = sum of partial losses + r(y'); accept / shrink / give up; next trial point (ST = float: rounded, see col_reduce).
template <int G, int R, bool VR = false, class ST = double>
__global__ void __launch_bounds__(256) col_decide_kernel(const TiledArgs a) {
  using P = typename Pair<ST>::type;
  constexpr int KP = G * R, NGW = 64 / G, PSTRIDE = KP + 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane % G, gi = lane / G;
  int64_t seg = ((int64_t)blockIdx.x * 4 + wave) * NGW + gi;
  if (a.actlist_in) { // the still-searching segments only
    if (seg >= a.nact_in) return;
    seg = a.actlist_in[seg];
  }
  if (seg >= a.nseg) return;
  if (a.active[seg] == 0) return; // group-uniform
  const int64_t gseg = a.own_offset + seg;
  double Jn = 0.0;
  for (int s = 0; s < a.nsup; ++s) Jn += a.part[((int64_t)seg * a.nsup + s) * PSTRIDE + KP];
  Vec<G, R> y, yn, g;
  P* yp = reinterpret_cast<P*>(reinterpret_cast<ST*>(a.own) + gseg * KP);
  double2* tp = reinterpret_cast<double2*>(a.trial + seg * (int64_t)KP);
  const double2* gp = reinterpret_cast<const double2*>(a.gsum + seg * (int64_t)KP);
#pragma unroll
  for (int i = 0; i < R / 2; ++i) yn.v[i] = tp[i * G + j];
  const RegDesc rd = load_reg(a.regs, a.reg_single ? 0 : seg);
  Jn += reg_eval<G, R, VR>(rd, yn, j, a.k);
  const double Jold = a.jold[seg];
  double alpha = a.alpha[seg];
  int still = 0, acc = 0;
  if (Jn < Jold) {
#pragma unroll
    for (int i = 0; i < R / 2; ++i) store_pair<ST>(&yp[i * G + j], yn.v[i]);
    alpha *= 1.05;
    acc = 1;
    if (j == 0 && a.obj) a.obj[gseg] = Jn;
  } else {
    alpha *= .7;
    if (alpha < a.min_stepsize) {
      alpha = a.min_stepsize * 1.1;
    } else if (alpha > a.min_stepsize) { // `while alpha > min_stepsize` (proxgrad.jl:136,180): alpha == min_stepsize ends the search without the 1.1 reset
      still = 1;
      const double l = (double)(a.ptr ? a.ptr[seg + 1] - a.ptr[seg] : a.dense_len) + 1.0;
      const double s = alpha / l;
#pragma unroll
      for (int i = 0; i < R / 2; ++i) {
        y.v[i] = widen(yp[i * G + j]);
        g.v[i] = gp[i * G + j];
        yn.v[i].x = fma(-s, g.v[i].x, y.v[i].x);
        yn.v[i].y = fma(-s, g.v[i].y, y.v[i].y);
      }
      reg_prox<G, R, VR>(rd, yn, s, j, a.k);
#pragma unroll
      for (int i = 0; i < R / 2; ++i) tp[i * G + j] = make_double2(stored<ST>(yn.v[i].x), stored<ST>(yn.v[i].y));
    }
  }
  if (j == 0) {
    a.alpha[seg] = alpha;
    a.active[seg] = still;
    const int nt = a.ntrial[seg] + 1;
    a.ntrial[seg] = nt;
    if (still) {
      const unsigned slot = atomicAdd(a.nactive, 1u);
      if (a.actlist_out) a.actlist_out[slot] = (int32_t)seg;
    } else if (a.trials) {
      a.trials[seg] += nt;
      a.accepts[seg] += acc;
    }
  }
}

// 1 if some segment's list is not ordered by TILE: the tiled sweeps need the entries of tile t to precede those of tile t+1
// (order inside a tile is free: the tile sits in LDS); a non-decreasing index list is the common special case.
static __global__ void check_sorted_kernel(const int64_t* ptr, const int32_t* idx, int64_t nseg, int tile, int* unsorted) {
  const int64_t seg = (int64_t)blockIdx.x;
  if (seg >= nseg) return;
  const int64_t b = ptr[seg], e = ptr[seg + 1];
  int bad = 0;
  for (int64_t t = b + 1 + threadIdx.x; t < e; t += blockDim.x) bad |= idx[t] / tile < idx[t - 1] / tile;
  if (bad) *unsorted = 1;
}

// Heterogeneous models (a loss descriptor per column): inside every tile window of a row, group the entries by loss kind
// (stable).  The lane groups of a wave walk their windows in lockstep, so most steps then meet ONE loss formula instead of all
// of them.  Only the engine's private copy of the row view is reordered; the sums change by rounding only.
static __global__ void __launch_bounds__(64) group_rows_by_kind_kernel(const int64_t* ptr, const int32_t* idx, const double* vals, int64_t nseg, int tile,
                                                                        const glrm_loss* losses, int32_t* oidx, double* ovals) {
  const int64_t seg = (int64_t)blockIdx.x;
  if (seg >= nseg) return;
  const int64_t b = ptr[seg], e = ptr[seg + 1];
  for (int64_t t = b + threadIdx.x; t < e; t += 64) {
    const int c = idx[t], tl = c / tile, kind = losses[c].kind;
    int64_t wb = t, we = t + 1; // window of the entry's tile (windows hold a few dozen entries)
    while (wb > b && idx[wb - 1] / tile == tl) --wb;
    while (we < e && idx[we] / tile == tl) ++we;
    int64_t rank = 0;
    for (int64_t u = wb; u < we; ++u) {
      const int ku = losses[idx[u]].kind;
      rank += (ku < kind) || (ku == kind && u < t);
    }
    oidx[wb + rank] = c;
    ovals[wb + rank] = vals[t];
  }
}

// descid[t] = colid[idx[t]]: the id of the column's loss descriptor among the model's distinct descriptors
static __global__ void entry_descid_kernel(const int32_t* idx, int64_t nnz, const uint8_t* colid, uint8_t* descid) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * blockDim.x) descid[t] = colid[idx[t]];
}

} // namespace glrm
