// glrm_engine.hpp -- host-side declarations shared by the translation units of libglrm_hip.so:
//   glrm_hip.hip        C ABI, gather sweeps, the shared host helpers declared below
//   glrm_tiled.hip      LDS-tiled sweeps            glrm_lane.hip       lane-per-segment LDS-tiled passes
//   glrm_blocked.hip    phase-aligned gather passes glrm_cached.hip     cached gather row sweep
//   glrm_dense.hip      MFMA path                   glrm_multi.hip      multi-dimensional losses / block regularizers
//   glrm_reforder.hip   reference-order sweeps      glrm_tilesort.hip   segmented sort of a view into tile order
//   glrm_transpose.hip  row view from column view   glrm_subset.hip     child handles (cross-validation)
//   glrm_svd.hip        SVD initialisation          glrm_impute.hip     imputation
//   glrm_multigpu.hip   sharded fits                glrm_testhooks.hip  test hooks (constant in the product library)
//   glrm_storage.hip    fp32 storage: the float gather sweeps, narrowing / widening copies (include/glrm_hip_storage.h)
//   glrm_cached_f32.hip fp32 storage: the float instantiations of the cached row sweep's register variant (glrm_cached.hpp)
//   glrm_blocked_f32.hip fp32 storage: the float instantiations of the phase-aligned passes (glrm_blocked.hpp, glrm_tiled.hpp)
//   glrm_regvec.hip     regularizers that carry a vector (include/glrm_hip_regvec.h): checks, the handle's tables, the two entry points
//   glrm_topk.hip       the rank-th largest entry of X'Y and the ordered scan of precision_at_k (include/glrm_hip_topk.h)
//   glrm_recommend.hip  the kper best columns of every queried row of X'Y, observed ones left out (include/glrm_hip_recommend.h); shares
//                       the tile function, the key and the refusals of glrm_topk.hip through glrm_xytile.hpp
//   glrm_nmf.hip        init_nndsvd!: NNDSVD and its soft-impute rounds on the resident lists (include/glrm_hip_nmf.h); shares the subspace
//                       iteration of glrm_svd.hip through glrm_subspace.hpp
//   glrm_solve.hip      the fused row solver of glrm_hip_solve_x (include/glrm_hip_transform.h): T X half-steps of a row in one launch of the
//                       register kernel (glrm_solve.hpp); glrm_solve_f32.hip holds its float instantiations
//   glrm_als.hip        the exact half-step of a quadratic model (include/glrm_hip_als.h): one workgroup per segment accumulates the Gram
//                       triangle in registers and one wave factorises it in LDS (glrm_als.hpp)
//   glrm_cd.hip         coordinate-descent sweeps for ZeroReg / QuadReg / OneReg / NonNegConstraint under QuadLoss (include/glrm_hip_cd.h):
//                       the Gram stage of glrm_als.hpp, then one wave sweeps the coordinates with x and the residual in registers (glrm_cd.hpp)
//   glrm_devmem.hpp     DeviceScope (the one device guard) and DevArena (the one owner of device memory: glrm_handle::mem, a shard's replica, local scratch)
// The launch layer the run functions of every family go through (side description, rounds driver, dispatch) is glrm_launch.hpp.
// Below: glrm_handle describes a model -- what exists once per view in side[GLRM_ROWS] / side[GLRM_COLS] (host functions take `int side`,
// the opposing side is side ^ 1); glrm_step is what ONE half-step is asked to do, built by the entry point and passed down as an argument
// (the handle holds nothing about a call in flight); glrm_side_family is the one place that says which kernel family runs a side;
// glrm_segment_class is the one rule for the class of a segment on the gather family and glrm_class_plan the plan made from it.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../include/glrm_hip.h"
#include "../../include/glrm_hip_storage.h"
#include "../../include/glrm_hip_regvec.h"
#include "../../include/glrm_hip_transform.h"

// kernel variants by loss model.  The *_NOTRIG variants are compiled without PeriodicLoss (its sin / cos with full range reduction
// costs ~60 VGPRs of pressure in every kernel that merely CONTAINS the case); models without a PeriodicLoss column use them.
enum { LOSS_QUAD_UNIFORM = 0, LOSS_SEGMENT = 1, LOSS_PER_OBS = 2, LOSS_SEGMENT_NOTRIG = 3, LOSS_PER_OBS_NOTRIG = 4 };
constexpr int loss_mode(int loss) { return loss >= 3 ? loss - 2 : loss; }
constexpr bool loss_trig(int loss) { return loss < 3; }

// opposing vectors per LDS tile (rows padded by 16 B, ~150 KB: one 16-wave workgroup per CU): the tile of the LDS-tiled and lane passes,
// the unit of the tile-order check and of the super-tiles of the phase-aligned passes
constexpr int glrm_tile_rows(int kp) { return ((150 * 1024) / (kp * 8 + 16)) / 16 * 16; }

extern thread_local char g_err[768];

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIPCK(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return fail(e_ == hipErrorOutOfMemory ? GLRM_ERR_OOM : GLRM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                  hipGetErrorString(e_), __FILE__, __LINE__);                                         \
  } while (0)

#include "glrm_devmem.hpp"
#include "glrm_knobs.hpp"

// which side of the factorization: glrm_handle::side[] and every `int side` argument are indexed by it; the opposing side is side ^ 1
enum { GLRM_ROWS = 0, GLRM_COLS = 1 }; // rows = row view, X half-step; columns = column view, Y half-step

// The class plan of one view on the gather family (glrm_hip.hip: build_class_plan fills it, glrm_for_each_class launches it).  n counts the
// local segments per class of glrm_segment_class (0: the rows a cached kernel holds on chip); when more than one class is populated, list
// holds the local segments class by class (ascending ids inside a class) and each class gets its own launch -- nullptr: one class holds
// every local segment.  cap is the launch parameter of class 0 (glrm_cached_cap of its longest row).
struct glrm_class_plan {
  int32_t* list = nullptr;
  int64_t n[4] = {0, 0, 0, 0};
  int cap = 0;
  bool built = false;
};

struct glrm_handle {
  int device = 0;
  DevArena mem;                       // every device allocation the handle keeps (borrowed arrays never enter it); glrm_hip_destroy releases it
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int64_t m = 0, n = 0;
  int k = 0, kp = 0, G = 4, R = 2;
  int tiled_opt = 0;                  // glrm_options.tiled
  int tG = 4, tR = 2;                 // lane layout of the tiled kernels (kp = tG*tR)
  int tile_rounds = 0;                // LDS-tiled sweeps: line-search rounds over the still-searching segments only (bit0 rows, bit1 columns)
  int32_t* actlist = nullptr;         // two lists of actlist_cap segment ids (glrm_tiled.hpp: TiledArgs::actlist_out / actlist_in)
  int64_t actlist_cap = 0;
  // per-segment buffers of the multi-pass families (LDS-tiled, lane, phase-aligned, dense): TiledArgs::part ... ntrial
  // and the super-tile geometry they were sized for (glrm_alloc_pass_buffers / glrm_bind_pass_buffers)
  struct PassBuffers {
    double *part = nullptr, *gsum = nullptr, *trial = nullptr, *jold = nullptr;
    int32_t *active = nullptr, *ntrial = nullptr;
    int nsup = 0, tiles_per_sup = 0;
    // phase-aligned passes (glrm_blocked.hip).  suppos[seg * nsup + sup]: offset inside segment seg's list of its first entry of super-tile
    // sup (what the pass kernel's search would find; nullptr = the kernel searches)
    int32_t* suppos = nullptr;
  };
  // Everything that exists once per view: side[GLRM_ROWS] is the row view and the X half-step, side[GLRM_COLS] the column view and the Y
  // half-step.  A "segment" is a row of the one and a column of the other.
  struct Side {
    // range and size: global segments [begin, end) of nglob (= m / n) are this shard's, nseg = end - begin, nnz observations
    int64_t begin = 0, end = 0, nseg = 0, nglob = 0, nnz = 0;
    // the view: segment offsets, opposing index and value of every observation
    // (GLRM_PROBLEM_BORROW_DEVICE_ARRAYS: these arrays are the caller's -- not in `mem`, never freed, never written by the engine -- until
    // a view has to be reordered: the private copy then replaces the borrowed pointer)
    int64_t* ptr = nullptr; int32_t* idx = nullptr; double* vals = nullptr;
    bool sorted = false;              // LDS-tiled sweeps (glrm_tiled.hpp): every list is in tile order
    int32_t* perm = nullptr;          // tiled sweeps: segments sorted by length (columns: by (loss kind, length))
    // regularizer descriptors (rx / ry): device, count, host copy (what glrm_hip_subset needs to build a child handle)
    glrm_reg* regs = nullptr; int64_t n_regs = 0; std::vector<glrm_reg> regs_h;
    bool vecreg = false;              // some descriptor of this side is a vector regularizer (kind >= GLRM_REG_QUAD_CONSTRAINT): VR kernels
    // regularizers that carry a vector (include/glrm_hip_regvec.h, glrm_regvec.hip): nullptr / empty while the side has none.
    // regvec: k x count doubles (ld k), reglen: count lengths, indexed like regs; regs_h then holds the descriptors WITH the new codes
    double* regvec = nullptr; int32_t* reglen = nullptr;
    std::vector<double> regvec_h; std::vector<int32_t> reglen_h;
    // per-segment state.  factor / obj are in use (bound or owned), own_factor / own_obj owned; factor is X / Y (GLRM_STORAGE_F32: it, like
    // vals, holds FLOATS behind the double* type, see glrm_handle::storage), obj is obj_by_row / obj_by_col
    double* alpha = nullptr;
    int32_t *trials = nullptr, *accepts = nullptr;
    double *factor = nullptr, *own_factor = nullptr, *obj = nullptr, *own_obj = nullptr;
    // family state
    int tiled = 0;                    // 0 = gather sweep, 1 = LDS-tiled
    bool grouped = false;             // LDS-tiled rows: the private copy was regrouped by loss kind inside the tile windows (set where the copy is made)
    int blocked = 0;                  // phase-aligned gather passes (glrm_blocked.hip) instead of the one-kernel gather sweep
    // lane-per-segment LDS-tiled passes (glrm_lane.hpp): family flag and the SELL layout of the view
    int lane = 0;
    bool lane_want = false, lane_compact = false; // glrm_lane_decide: the whole problem admits the family on this side / its stream takes the compact form
    int64_t* lane_bptr = nullptr; int32_t* lane_off = nullptr; double* lane_val = nullptr;
    int64_t lane_nwb = 0, lane_steps = 0; int lane_ntiles = 0;
    uint16_t* lane_off16 = nullptr; int64_t* lane_vptr = nullptr; int32_t* lane_sval = nullptr; // the compact form of the stream (glrm_lane.hpp: LaneArgs::off16 / vptr) of the sides that run it
    int lane_dealt = 0;               // the side's sorted slot permutation was dealt out by class (make_segperm): slot s holds a segment of class s & 15
    int32_t* lane_inv = nullptr;      // local segment -> slot of the layout (sides whose slots are permuted); -1 = not in the layout
    PassBuffers pass;
    int64_t blocked_cap[2] = {0, 0};  // phase-aligned passes: segments per launch slice, [gradient / trial instantiation]
    // Gather sweeps: the waves that share a segment are a function of the segment's OWN length (1 below 1536 observations, 4 below
    // 98304, else 8; glrm_options.waves_* pins one count for all), so the order of a segment's sums never depends on which shard
    // holds it.  Class 0 = rows the cached sweep holds on chip.  plan: what finalize found on this shard.
    int waves = 1;                    // the class most local segments fall into (reported by glrm_hip_kernel_stats); columns start at 4
    glrm_class_plan plan;
    // dense MFMA path (glrm_dense.hip)
    double* A = nullptr; int64_t lda = 0; // packed, zero padded: [nseg_pad][lda]
    int64_t vps = 0;                  // opposing vectors per super-tile
    double* jloss = nullptr;          // loss sum at the current point, per local segment
    int64_t launches = 0; double ms = 0; // counters of glrm_hip_kernel_stats
  } side[2];
  glrm_handle() { side[GLRM_COLS].waves = 4; }
  unsigned int* nactive = nullptr;    // segments still searching (one counter: a half-step at a time)
  int* dflag = nullptr;
  // rows only: the heterogeneous tiled row sweep
  uint8_t* rowdescid = nullptr;       // id of the loss descriptor of every entry of the row view
  glrm_loss* udesc = nullptr;         // the model's distinct loss descriptors (<= 256), device
  int n_udesc = 0;
  // trial rounds read out of the SELL layout (lane_pass_kernel FORM 2): the still-searching segments class by class, rebuilt every round
  int32_t *lane_gcnt = nullptr, *lane_gbase = nullptr, *lane_gtotal = nullptr, *lane_glist = nullptr;
  int64_t lane_gcap = 0, lane_gchunks = 0;
  // general sweeps: multi-dimensional losses / wrapped regularizers (glrm_multi.hip)
  bool multi = false;
  // columns only: the embedding of Y and the split Y half-step of the general sweeps
  int64_t d = 0;                      // vectors of Y = sum of embedding dimensions (= n for scalar losses)
  int dmax = 1;
  int multi_kmask = 0;                // loss kinds of the model: bit `kind` per multi-dimensional kind, bit 0 = some scalar loss (glrm_multi.hpp: MULTI_KM_*)
  int64_t* ystart = nullptr;          // device, n+1
  int64_t ys_cb = 0;                  // ystart[side[GLRM_COLS].begin]: first vector of the shard's column block
  int col_nsplit = 1;                 // > 1: the Y half-step runs as split passes + decide rounds
  int64_t col_chunk = 0;
  double *mtrial = nullptr, *mpart_loss = nullptr, *mpart_G = nullptr, *mgtot = nullptr, *mobjold = nullptr;
  int32_t* mactive = nullptr;
  unsigned int* mnactive = nullptr;
  // dense MFMA path (glrm_dense.hip)
  bool dense = false;
  double dense_scale = 1.0;
  // rows only: the cached gather row sweep
  int cached_row = 0;                 // cached gather row sweep (glrm_cached.hip): 0 off, 1 LDS, 2 registers
  int cached_want = 0;                // the whole problem runs its short rows on the cached sweep (decided from glrm_signature, never from the shard)
  // what glrm_setup_cached decided for the whole problem (they hold on a shard whose cached_row fell to 0, too): the variant (2 registers --
  // always, for float storage -- or 1 LDS), the waves that share a row of the register variant, the longest row the sweep takes
  int cached_variant = 0, cached_waves = 2;
  int64_t cached_maxlen = -1;
  // glrm_hip_solve_x (include/glrm_hip_transform.h; glrm_solve.hpp).  solve_ok: set-up found that the handle COULD run the two-wave register
  // variant of the cached row sweep on this problem (glrm_setup_cached: its predicate without the auto rule's sizes) -- whether step_x
  // runs it or not.  A handle whose rows are not on that family gets a row plan of its own at its first solve_x: solve_plan, with the
  // rows the register kernel takes as class 0.  solve_fused .. solve_loop_rows: what the last solve_x did (-1: none yet).
  int solve_ok = 0;
  glrm_class_plan solve_plan;
  int solve_fused = -1;
  int64_t solve_fused_rows = 0, solve_loop_rows = 0;
  // glrm_hip_als_solve (include/glrm_hip_als.h; glrm_als.hip), per side, made at the side's first solve: the local segments longest first
  // (a permutation of its own: Side::perm leaves out the columns diverted to the 8-wave sweep) and the status of every local segment
  // after the last solve.  solved: glrm_hip_als_info has something to report
  struct Als { int32_t* order = nullptr; int8_t* status = nullptr; bool solved = false; } als[2];
  // glrm_hip_cd_solve (include/glrm_hip_cd.h; glrm_cd.hip), per side, made at the side's first solve: the same longest-first order, and
  // the status bits and the sweeps run of every local segment after the last solve
  struct Cd { int32_t* order = nullptr; int8_t* status = nullptr; int32_t* sweeps_run = nullptr; bool solved = false; } cd[2];
  // glrm_hip_stream_rows (include/glrm_hip_stream.h; glrm_stream.hip): the divisions every column has received (n counts, made at the first
  // call and zeroed by every call), and what the last call did -- the status of every streamed row and the figures of its plan.
  // ran: glrm_hip_stream_info has something to report
  struct Stream {
    int64_t* epoch = nullptr;
    std::vector<int8_t> status;
    int64_t rows = 0, nlevels = 0, nlaunches = 0, max_width = 0;
    double plan_ms = 0.0;
    bool ran = false;
  } stream_state;
  // glrm_options.quad_gram: trials from the quadratic form (glrm_dense.hpp: dense_gram_*)
  bool dense_gram = false;
  double *gramH = nullptr, *gram_part = nullptr; // [kp*kp], [GRAM_BLOCKS][kp*kp]
  glrm_loss* losses = nullptr;
  int64_t n_losses = 0;
  bool loss_quad_uniform = false;
  bool has_trig = false; // some column carries a PeriodicLoss
  double *partials = nullptr, *dscalar = nullptr;
  unsigned long long* dcount = nullptr;
  bool finalized = false;             // false between a GLRM_PROBLEM_DEFER_SETUP create and glrm_hip_finalize
  bool finalize_failed = false;       // glrm_hip_finalize ran and failed half way: the handle can only be destroyed
  // columns only.  Phase-aligned column passes on skewed data: slot -> column for the passes (columns below blk_long_from observations,
  // longest first), the columns at or above it (8-wave gather sweep on the side stream), and the threshold (from the WHOLE problem's mean)
  int32_t *blk_perm_c = nullptr, *blk_long_c = nullptr;
  int64_t blk_nshort_c = 0, blk_nlong_c = 0, blk_long_from = 0;
  // launch geometry of the persistent / sliced kernels, per handle (device and fill percentage at finalize; a process may drive devices
  // with different CU counts, and the knobs are read per handle): 0 = not computed yet
  int cached_grid[6] = {0, 0, 0, 0, 0, 0}; // persistent cached row sweep: resident workgroups of the MAXT = 7 / 4 instantiation; [2], [3]: of their VR = true twins; [4], [5]: of the float ones
  glrm_signature sig_local{}, sig{};  // this shard's contribution / the whole problem's
  hipStream_t side_stream = nullptr;  // the launches of the minority classes run beside the main launch
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int profile = 0;
  // columns only, glrm_hip_step_y_arrival (the blocks themselves are the call's: glrm_arrivals below)
  bool arrival_static = false; // true arrival order gave up once (an event that cannot be queried, 5 s without progress): in-stream waits from then on
  double ms_wait = 0;                 // profile: time the launch stream stood in the waits for arriving blocks
  int sum_order_opt = 0;              // glrm_options.sum_order (1: reference-order validation sweeps, glrm_reforder.hip)
  // glrm_options.storage.  GLRM_STORAGE_F32: Side::vals / factor / own_factor hold FLOATS behind their double* type (the same
  // element counts); only the float gather sweeps, the float cached row sweep (glrm_cached_f32.hip), the float phase-aligned passes
  // (glrm_blocked_f32.hip) and the copy kernels of glrm_storage.hip read them, every other family is refused.
  int storage = 0;
  // hipGraph of one outer iteration (gather sweeps on a private stream): small fits are launch bound
  hipGraph_t iter_graph = nullptr;
  hipGraphExec_t iter_exec = nullptr;
  double* pinned_obj = nullptr;       // host-pinned scalar the graph copies sum(obj_by_col) into
  int64_t graph_ix = 0, graph_iy = 0; // inner iteration counts the graph was captured for
  double graph_min = 0.0, graph_step = 0.0;
  // what glrm_hip_subset needs to build a child handle: the options and host copies of the descriptors (Side::regs_h)
  glrm_options opts{};
  std::vector<glrm_loss> losses_h;
  struct Ev { hipEvent_t a, b; int slot; }; // slot: the side whose half-step the pair times, 2 = a wait for arriving blocks (ms_wait)
  std::vector<Ev> pending, pool;
};

// glrm_hip_step_y_arrival: the blocks of X that are still arriving and which of them the launch stream has already been made to wait for.
// Lives on that entry point's stack, for that call only.
struct glrm_arrivals {
  const glrm_arrival* blocks; int n;
  std::vector<char> waited;
};
// What ONE call of run_sweep is asked to do: built by the entry point from its own arguments, const from there down.  `side` is an int that
// is only ever assigned GLRM_ROWS / GLRM_COLS (a `true` would mean columns: the functions of glrm_hip.hip that build every request refuse a bool).
struct glrm_step {
  int side;
  double min_stepsize = 0.0;
  bool eval_only = false;               // the loss evaluation of glrm_hip_col_losses / the objective
  double fixed_alpha = 0.0;             // > 0: the SparseProxGradParams step, no line search
  int64_t row_begin = 0, row_end = -1;  // glrm_hip_step_x_range: local rows [row_begin, row_end); row_end < 0 = every local row
  glrm_arrivals* arrivals = nullptr;    // glrm_hip_step_y_arrival; nullptr = X is complete
  int loss = 0, loss_by_segment = 0;    // the loss variant (LOSS_*), chosen once by run_sweep (loss_variant)
  bool ranged() const { return side == GLRM_ROWS && row_end >= 0; }
  bool fixed() const { return fixed_alpha > 0.0 && !eval_only; }
};

// The kernel family that runs a side's half-step (eval_only: the loss evaluation of glrm_hip_col_losses / the objective).  The ONE statement
// of the precedence among families: run_sweep dispatches on it, glrm_hip_sum_order describes it, the arrival and graph decisions ask it.
// The raw flags are not exclusive -- glrm_hip_set_regularizers can move a finalized tiled handle to multi while tiled stays set -- so the
// precedence is spelled nowhere else.  The flags are still read by the set-up functions (they run before the flags are final), for the
// lane refinement of TILED and the cached class of GATHER (decided where those families run) and by glrm_hip_kernel_stats.
enum glrm_family { GLRM_FAM_REFERENCE, GLRM_FAM_GENERAL, GLRM_FAM_DENSE, GLRM_FAM_TILED, GLRM_FAM_BLOCKED, GLRM_FAM_GATHER };
inline glrm_family glrm_side_family(const glrm_handle* h, int side, bool eval_only) {
  if (h->sum_order_opt) return GLRM_FAM_REFERENCE;
  if (h->multi) return GLRM_FAM_GENERAL;
  if (h->dense) return GLRM_FAM_DENSE;
  const bool passes = side == GLRM_COLS || !eval_only; // the row passes have no evaluation form: the gather sweep evaluates
  if (h->side[side].tiled && passes) return GLRM_FAM_TILED;
  if (h->side[side].blocked && passes) return GLRM_FAM_BLOCKED;
  return GLRM_FAM_GATHER;
}

// refusals shared by the entry points (the single-shard message is the entry point's own)
#define GLRM_NEED_FINALIZED(h) \
  do { if (!(h)->finalized) return fail(GLRM_ERR_INVALID, "the handle was created with GLRM_PROBLEM_DEFER_SETUP: call glrm_hip_finalize first"); } while (0)
inline bool glrm_single_shard(const glrm_handle* h) { return h->side[GLRM_ROWS].begin == 0 && h->side[GLRM_ROWS].end == h->m && h->side[GLRM_COLS].begin == 0 && h->side[GLRM_COLS].end == h->n; }

namespace glrm { struct TiledArgs; }

// the two halves of "sum the counts, max the rest" (include/glrm_hip.h: glrm_signature): what a sharding host adds up over its shards, and
// what glrm_hip_finalize holds the result to
inline void glrm_signature_add(glrm_signature& whole, const glrm_signature& local) {
  whole.nnz_rows += local.nnz_rows; whole.nnz_cols += local.nnz_cols;
  whole.max_row_len = std::max(whole.max_row_len, local.max_row_len); whole.max_col_len = std::max(whole.max_col_len, local.max_col_len);
  whole.rows_unordered = std::max(whole.rows_unordered, local.rows_unordered); whole.cols_unordered = std::max(whole.cols_unordered, local.cols_unordered);
}
inline bool glrm_signature_covers(const glrm_signature& whole, const glrm_signature& local) {
  return whole.nnz_rows >= local.nnz_rows && whole.nnz_cols >= local.nnz_cols && whole.max_row_len >= local.max_row_len &&
         whole.max_col_len >= local.max_col_len && whole.rows_unordered >= local.rows_unordered && whole.cols_unordered >= local.cols_unordered;
}

// structural check of a host array of nseg + 1 segment offsets (name: "rowptr" / "colptr")
inline int glrm_check_offsets(const char* name, const int64_t* ptr, int64_t nseg) {
  if (ptr[0] != 0) return fail(GLRM_ERR_INVALID, "%s[0] must be 0", name);
  for (int64_t s = 0; s < nseg; ++s)
    if (ptr[s + 1] < ptr[s]) return fail(GLRM_ERR_INVALID, "%s is not monotone at %lld", name, (long long)s);
  return GLRM_OK;
}

// The chunks of a kernel that gives every column gridDim.y = nsplit workgroups of `chunk` entries each and adds their partials in chunk
// order (the init_svd / init_nndsvd column products, error_metric): base_chunk entries, doubled until the longest column fits gridDim.y.
// The longest column is the handle's own record: create_impl takes sig_local.max_col_len from the very colptr array side[GLRM_COLS].ptr
// points to (view_stats; a subset child and a rows-from-cols handle go through create_impl too) and nothing writes that array afterwards
// (the set-up re-orders idx / vals inside a segment only).  Not h->sig: glrm_hip_finalize accepts a covering signature that may be larger.
struct glrm_col_chunks { int64_t longest, chunk; int nsplit; };
inline glrm_col_chunks glrm_chunk_columns(const glrm_handle* h, int64_t base_chunk) {
  glrm_col_chunks c{h->sig_local.max_col_len, base_chunk, 1};
  while ((c.longest + c.chunk - 1) / c.chunk > 65535) c.chunk *= 2; // gridDim.y
  c.nsplit = (int)std::max<int64_t>(1, (c.longest + c.chunk - 1) / c.chunk);
  return c;
}

// ---- the bookkeeping of the ProxGrad outer loop (src/algorithms/proxgrad.jl), shared by glrm_hip_fit and glrm_hip_multi_fit
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// norm(Y) == 0 guard (proxgrad.jl:45-48: the reference would hit an UndefVarError; sparse_proxgrad.jl:41-43: it would re-randomise Y)
inline bool glrm_all_zero(const double* v, int64_t count) {
  double norm2 = 0.0;
  for (int64_t i = 0; i < count; ++i) norm2 += v[i] * v[i];
  return norm2 == 0.0;
}
// Y: k x d, dense
inline int glrm_check_fit_args(const glrm_params* prm, int64_t cap, const double* Y, int64_t k, int64_t d) {
  if (prm->max_iter < 0 || cap < prm->max_iter + 1) return fail(GLRM_ERR_INVALID, "objective/seconds capacity must be >= max_iter+1");
  if (prm->inner_iter_X < 1 || prm->inner_iter_Y < 1) return fail(GLRM_ERR_INVALID, "inner iteration counts must be >= 1");
  if (glrm_all_zero(Y, k * d)) return fail(GLRM_ERR_INVALID, "Y is all zeros (the reference cannot start from Y == 0)");
  return GLRM_OK;
}
// ConvergenceHistory (src/convergence.jl:22-26) and the stopping rule of proxgrad.jl:210-213.  start() records the initial objective and
// starts the clock; record() closes iteration i -- the clock restarts after the entry is written -- and says whether the fit stops.
struct glrm_trace {
  double *objective, *seconds;
  double scaled_abs_tol, rel_tol;      // abs_tol * observations (:72), rel_tol
  int64_t nrec = 0;
  double t = 0.0;
  glrm_trace(double* objective, double* seconds, const glrm_params* prm, int64_t nnz)
      : objective(objective), seconds(seconds), scaled_abs_tol(prm->abs_tol * (double)nnz), rel_tol(prm->rel_tol) {}
  void start(double obj0) {                                              // update_ch!(ch, 0, objective(...)) :76
    objective[0] = obj0;
    seconds[0] = 0.0;
    nrec = 1;
    t = now_s();
  }
  bool record(int64_t i, double obj) {
    const double dt = now_s() - t;
    objective[nrec] = obj;
    seconds[nrec] = seconds[nrec - 1] + dt;                              // update_ch!
    ++nrec;
    t = now_s();
    const double dec = objective[nrec - 2] - obj;                        // :210
    return i > 10 && (dec < scaled_abs_tol || dec / obj < rel_tol);      // :211-213
  }
};

// per-segment class of the gather sweeps (see glrm_class_plan)
constexpr int64_t GLRM_WAVES4_FROM = 1536, GLRM_WAVES8_FROM = 98304;
__host__ __device__ inline int glrm_wave_class(int64_t len) { return len < GLRM_WAVES4_FROM ? 1 : (len < GLRM_WAVES8_FROM ? 2 : 3); }
constexpr int glrm_class_waves(int cls) { return cls <= 1 ? 1 : (cls == 2 ? 4 : 8); }
// the class glrm_options.waves_row / waves_col pins for every segment of a side (1 / 4 / 8 waves), 0 for any other value: none
inline int glrm_forced_class(const glrm_handle* h, int side) {
  const int waves = side == GLRM_ROWS ? h->opts.waves_row : h->opts.waves_col;
  return waves == 1 ? 1 : (waves == 4 ? 2 : (waves == 8 ? 3 : 0));
}
// THE class of a segment of `len` observations: 0 where a cached kernel takes it (len <= cached_maxlen; cached_maxlen < 0: no segment),
// else the pinned class (forced > 0), else the one its own length asks for
__host__ __device__ inline int glrm_segment_class(int64_t len, int64_t cached_maxlen, int forced) {
  return (cached_maxlen >= 0 && len <= cached_maxlen) ? 0 : (forced > 0 ? forced : glrm_wave_class(len));
}
// rows the register-cached sweep takes: at most 13 trips of the lane layout, 64 / G observations each
inline int64_t glrm_cached_reg_maxlen(int G) { return (int64_t)13 * (64 / G); }

// LDS-tiled sweeps (glrm_tiled.hip).  prepare: lane layout + the tile-order check of this shard's lists (create);
// setup: family choice from h->sig and buffers (finalize)
int glrm_prepare_tiled(glrm_handle* h);
int glrm_setup_tiled(glrm_handle* h);
int glrm_run_tiled(glrm_handle* h, const glrm_step& step);

// lane-per-segment LDS-tiled passes (glrm_lane.hip): setup decides lane[] from the whole problem's signature and builds the SELL layouts;
// run takes the TiledArgs glrm_run_tiled prepared (glrm_tiled.hpp)
void glrm_lane_decide(glrm_handle* h);                 // set-up, once: Side::lane_want / lane_compact from the whole problem's shape / losses / options and the knobs
int glrm_setup_lane(glrm_handle* h);
bool glrm_lane_loss_ok(const glrm_handle* h, int loss);
bool glrm_lane_few_descriptors(const glrm_handle* h);
int glrm_run_lane(glrm_handle* h, const glrm_step& step, const glrm::TiledArgs& a);

// phase-aligned gather passes (glrm_blocked.hip): setup decides Side::blocked and allocates the pass buffers
int glrm_setup_blocked(glrm_handle* h);
int glrm_run_blocked(glrm_handle* h, const glrm_step& step);

// glrm_hip_step_y_arrival (glrm_hip.hip): make h->stream wait for every block of `arr` that intersects rows [lo, hi) of X and has
// not been waited for yet
int glrm_arrival_wait(glrm_handle* h, glrm_arrivals& arr, int64_t lo, int64_t hi);
// LDS-tiled / lane column passes under glrm_hip_step_y_arrival (round 6): runs of super-tiles in the order their rows of X are announced --
// launch(sup_lo, sup_hi) is called once per run, behind the in-stream waits for the blocks the run touches; without arrival blocks (arr ==
// nullptr): one call over all super-tiles.  Partial sums are per (column, super-tile) and are reduced in super-tile order: which run went first changes no bit.
int glrm_for_sup_runs_in_arrival_order(glrm_handle* h, glrm_arrivals* arr, int nsup, int64_t rows_per_sup, const std::function<int(int, int)>& launch);

// stable segmented sort of a view by tile index (glrm_tilesort.hip)
int glrm_tile_sort_view(hipStream_t st, const int64_t* ptr, int64_t nseg, int64_t nnz, int tile, int64_t n_other, int32_t** idx, double** vals, DevArena& owner);

// reference-order validation sweeps (glrm_reforder.hip; glrm_options.sum_order = 1)
// test hooks (csrc/glrm_testhooks.hip): constant in the product library, environment-driven in the test build (-DGLRM_HIP_TESTING)
int glrm_test_fail_finalize();                        // 1 = glrm_hip_finalize fails half way (the set-up-failed latch cannot be reached otherwise)
int glrm_check_regularizers(const glrm_handle* h, const glrm_reg* rx, int64_t n_rx, const glrm_reg* ry, int64_t n_ry); // set_regularizers' refusals, no side effect
// include/glrm_hip_regvec.h (glrm_regvec.hip): everything glrm_hip_set_regularizers_vec refuses, no side effect / the descriptors of the
// handle with the vector codes taken out (what glrm_hip_create accepts) / the parent's descriptors and vectors installed on a fresh child /
// the tables dropped (plain set_regularizers, destroy)
int glrm_check_regularizers_vec(const glrm_handle* h, const glrm_reg* rx, int64_t n_rx, const glrm_regvec* vx, const glrm_reg* ry, int64_t n_ry, const glrm_regvec* vy);
bool glrm_regvec_carries(const glrm_reg& r);
void glrm_regvec_placeholders(const std::vector<glrm_reg>& in, std::vector<glrm_reg>& out);
int glrm_regvec_inherit(glrm_handle* child, const glrm_handle* parent);
void glrm_regvec_drop(glrm_handle* h);
int glrm_setup_reforder(glrm_handle* h);               // finalize: refuses what the mode does not cover
int glrm_run_reforder(glrm_handle* h, const glrm_step& step);
int glrm_reforder_sum(glrm_handle* h, const void* dvec, int64_t n, double* out); // Julia's pairwise sum(::Vector{Float64})
int glrm_reforder_objective(glrm_handle* h, int include_reg, double* out);       // objective(): ONE accumulator over all observations, then the penalties

// fp32 storage (glrm_storage.hip).  An entry point that reads fp64 lists or factors refuses a float handle before it touches it:
#define GLRM_REFUSE_F32(h, what) \
  do { if ((h) && (h)->storage == GLRM_STORAGE_F32) return fail(GLRM_ERR_UNSUPPORTED, "%s is not available with storage = f32 (glrm_options.storage = 1): %s", what, "it reads or reverts fp64 lists and factors"); } while (0)
namespace glrm { struct SweepArgs; }
int glrm_check_storage(const glrm_problem* p, const glrm_options* o);   // create: the option's range and everything a float handle refuses
int glrm_check_storage_regs(const glrm_reg* rx, int64_t n_rx, const glrm_reg* ry, int64_t n_ry); // wrapped / vector regularizers
int glrm_narrow_views(glrm_handle* h);                                  // end of create: both views' vals double -> float arrays of the handle's own
int glrm_narrow_factor(glrm_handle* h, const double* host, void* dev, int64_t nvec); // host k x nvec doubles -> device floats, ld kp, zero padded
int glrm_widen_factor(glrm_handle* h, const void* dev, double* host, int64_t nvec);  // and back
int glrm_check_narrowable(const char* name, const double* v, int64_t n);             // GLRM_ERR_NONFINITE for a finite value beyond float's range
void glrm_launch_sweep_f32(int G, int R, int waves, int loss, int side, const glrm::SweepArgs& a, hipStream_t st);
void glrm_launch_penalty_f32(glrm_handle* h, int side);
// the float instantiations of the phase-aligned passes and of their reduce / decide kernels (glrm_blocked_f32.hip); arr / sup_order: see
// launch_blocked_inst (glrm_blocked.hpp)
int glrm_launch_blocked_f32(glrm_handle* h, int loss, bool grad, const glrm::TiledArgs& a, int side, glrm_arrivals* arr, const std::vector<int>& sup_order);
void glrm_launch_col_small_f32(int kp, int stage, const glrm::TiledArgs& a, hipStream_t st);

// GLRM_PROBLEM_ROWS_FROM_COLS (glrm_transpose.hip): the row view derived on the device from the uploaded column view
int glrm_rows_from_cols(glrm_handle* h);

// cached gather row sweep (glrm_cached.hip)
int glrm_setup_cached(glrm_handle* h);                 // finalize: cached_want / cached_row from h->sig
// float storage, GLRM_HIP_CACHED unset: 1 = the fp64 auto rule applies, 0 = the family stays behind GLRM_HIP_CACHED=1
constexpr int GLRM_CACHED_F32_AUTO = 0;
// float storage, GLRM_HIP_BLOCKED unset: 1 = the fp64 auto rule of the phase-aligned passes applies, 0 = the family stays behind
// GLRM_HIP_BLOCKED (turning it on changes which kernels, and which summation order, existing float handles take)
constexpr int GLRM_BLOCKED_F32_AUTO = 0;
int glrm_cached_cap(int variant, int G, int kp, int64_t maxlen); // the launch parameter of a variant's kernels for a longest row of maxlen
int glrm_run_cached(glrm_handle* h, const glrm_step& step, const int32_t* seglist, int64_t nlist, int cap, hipStream_t st);
// the fused row solver of glrm_hip_solve_x (glrm_solve.hip): `inner` X half-steps of the listed rows in one launch
int glrm_run_solve(glrm_handle* h, const glrm_step& step, const int32_t* seglist, int64_t nlist, int cap, int inner, hipStream_t st);
// dense MFMA path (glrm_dense.hip)
int glrm_setup_dense(glrm_handle* h, const glrm_problem* p);
int glrm_run_dense(glrm_handle* h, const glrm_step& step);

// general sweeps (glrm_multi.hip)
int glrm_setup_multi(glrm_handle* h, const glrm_problem* p);
int glrm_setup_multi_split(glrm_handle* h);            // finalize (or the set_regularizers call that moves a handle here): split long columns or not
int glrm_run_multi(glrm_handle* h, const glrm_step& step);
int glrm_run_multi_penalty(glrm_handle* h, int side);

// per-segment reduce (stage = 0) / decide (stage = 1) kernels of glrm_tiled.hpp for a kp-wide factor
void glrm_launch_col_small(int kp, int stage, const glrm::TiledArgs& a, hipStream_t st);

// ---- shared host helpers (glrm_hip.hip)
// the pass buffers of one side for the local segments and side[side].pass.nsup super-tiles, and nactive
int glrm_alloc_pass_buffers(glrm_handle* h, int side);
// side stream + fork / join events (created once): launches that run beside the main stream's
int glrm_ensure_side_stream(glrm_handle* h);
int glrm_fork_side_stream(glrm_handle* h);        // the side stream continues behind what h->stream holds
hipError_t glrm_join_side_stream(glrm_handle* h); // h->stream continues behind the side stream; g_err is left as it was (joins also run on error paths)
// host copy of a view's segment offsets (nseg + 1)
int glrm_host_ptr(glrm_handle* h, int side, std::vector<int64_t>& ptr);
// a host list as a device array of its own (at least one element is allocated); synchronizes, so the list may be a local
int glrm_upload_list(glrm_handle* h, const std::vector<int32_t>& list, int32_t** out);
// segments split at long_from observations (<= 0: none is long): the short ones by descending length (stable), the long ones by id
void glrm_split_by_length(const std::vector<int64_t>& ptr, int64_t long_from, std::vector<int32_t>& shorts, std::vector<int32_t>& longs);
// the columns that leave the passes for the 8-wave gather sweep on the side stream (blk_long_c / blk_nlong_c)
int glrm_set_long_columns(glrm_handle* h, const std::vector<int32_t>& longs);
