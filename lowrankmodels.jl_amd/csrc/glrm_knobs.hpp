// glrm_knobs.hpp -- every environment variable the library reads, once: name, kind, default, read time, build, meaning.  The only file
// under csrc/ that spells a variable's name or calls getenv (tests/test_knobs.py holds the tree to that, and DESIGN.md's table to this one).
//   kind     INT, FLOAT (knob_positive) or PATH (knob_path)
//   default  a fixed value, or AUTO where the site computes it and passes it to knob_or (the meaning then says from what)
//   read     SETUP: decides what set-up builds, which family or summation order runs, or what glrm_hip_sum_order / glrm_hip_kernel_stats
//            report -- read inside glrm_hip_create / glrm_hip_finalize / glrm_hip_multi_create (and the calls that redo set-up) only; what
//            it decided is kept on the handle and asked from the handle afterwards.  CALL: chooses among launch forms that give the same
//            bits (or traces); read where it is used, so that one live handle can be timed under several settings.
//   build    ANY, or TESTING: the variable exists in libglrm_hip_testing.so (-DGLRM_HIP_TESTING) only
// The accessors call getenv when they are asked: nothing is cached per process.  (static: the two builds' tables differ, and the test
// build links objects of both.)
#pragma once

#include <cstdlib>

// clang-format off
#define GLRM_KNOBS(X) GLRM_KNOBS_ANY(X) GLRM_KNOBS_TESTING(X)
#define GLRM_KNOBS_ANY(X) \
  X(HIP, TILED,               INT,   AUTO,       SETUP, ANY,     "LDS-tiled sweeps: bit0 rows, bit1 columns; overrides glrm_options.tiled (AUTO: 0 for tiled = 1, 3 for tiled = 2, else the measured rule of glrm_setup_tiled).") \
  X(HIP, TILE_SORT,           INT,   1,          SETUP, ANY,     "Tile-sort the private copy of lists in arbitrary order: 0 never, 1 where the auto choice wants the LDS tiles, 2 for an explicit tiled = 2 as well.") \
  X(HIP, TILE_SORT_BATCH,     INT,   0,          SETUP, ANY,     "Entries per batch of the segmented tile sort; 0 or unset: 1.5e9 (tests lower it to exercise the batching).") \
  X(HIP, TILE_ROUNDS,         INT,   3,          SETUP, ANY,     "LDS-tiled sweeps: line-search rounds over the still-searching segments only, bit0 rows, bit1 columns; 0 = the one-kernel forms (kept in glrm_handle::tile_rounds).") \
  X(HIP, GROUP_KINDS,         INT,   1,          SETUP, ANY,     "Heterogeneous LDS-tiled rows: regroup every row's entries by loss kind inside the tile windows (kept in Side::grouped; reported as private_order = 2).") \
  X(HIP, UDESC,               INT,   1,          SETUP, ANY,     "Heterogeneous LDS-tiled rows: one-byte ids into a table of the model's distinct loss descriptors (at most 256; kept in glrm_handle::udesc); 0 also keeps such rows off the lane passes.") \
  X(HIP, SEGPERM,             INT,   1,          SETUP, ANY,     "LDS-tiled sweeps: hand the segments out sorted by (loss kind,) descending length; 0 keeps the natural order.") \
  X(HIP, COL_WORKGROUPS,      INT,   AUTO,       SETUP, ANY,     "LDS-tiled column passes: (column group, super-tile) workgroups the super-tile size aims at (AUTO: 2048 where the columns run the lane passes, else 1024).") \
  X(HIP, TILED_LONG_FROM,     INT,   -1,         SETUP, ANY,     "LDS-tiled column passes: columns of at least this many observations run on the 8-wave gather sweep; negative or unset: max(4096, 4 x the whole problem's mean column length); 0 = none.") \
  X(HIP, LANE,                INT,   3,          SETUP, ANY,     "Lane-per-segment form of the LDS-tiled passes at k = 32: bit0 rows, bit1 columns (the wish is kept in Side::lane_want, what runs in Side::lane).") \
  X(HIP, LANE_PER_OBS,        INT,   1,          SETUP, ANY,     "Lane passes for rows that meet a loss per observation; 0 keeps such rows on the four-lane kernels.") \
  X(HIP, LANE_COMPACT,        INT,   2,          SETUP, ANY,     "Compact form of the lane stream (2-byte offsets, unpadded values): 0 never, 1 every side it serves, 2 views beyond 2e9 observations (kept in Side::lane_compact).") \
  X(HIP, LANE_MAX_NNZ_M,      INT,   AUTO,       SETUP, ANY,     "Lane passes, column view: largest view in millions of observations (AUTO: 6000 where LANE_COMPACT is not 0, else 2000).") \
  X(HIP, LANE_MAX_NNZ_ROWS_M, INT,   6000,       SETUP, ANY,     "Lane passes, row view: largest view in millions of observations.") \
  X(HIP, LANE_DEAL,           INT,   1,          SETUP, ANY,     "Lane passes: deal a sorted slot permutation out by class (global id & 15) so that a wave reads its tiles conflict free; changes no sum.") \
  X(HIP, LANE_ROUNDS,         INT,   1,          CALL,  ANY,     "Lane passes: trial rounds read out of the SELL layout through gathered waves; 0 = full grid / CSR forms only (same bits).") \
  X(HIP, LANE_TAIL,           INT,   5,          CALL,  ANY,     "Lane row passes: below this percentage of searching segments a round runs a wave per segment (same bits).") \
  X(HIP, LANE_TAIL_COLS,      INT,   3,          CALL,  ANY,     "Lane column passes: below this percentage of searching segments a round runs a wave per (segment, super-tile) (same bits).") \
  X(HIP, LANE_GATHER_PACKED,  INT,   4,          CALL,  ANY,     "Lane passes: below this percentage the gathered waves are packed from the decide kernel's compact list (same bits).") \
  X(HIP, LANE_GATHER_SLOTS,   INT,   1,          CALL,  ANY,     "Lane passes: chunk lists over the dealt slots of a side whose slots are permuted (same bits).") \
  X(HIP, LANE_GATHER_FROM,    INT,   0,          CALL,  ANY,     "Lane passes: lowest percentage of searching segments at which a round runs gathered waves (same bits).") \
  X(HIP, LANE_GATHER_TO,      INT,   70,         CALL,  ANY,     "Lane passes: percentage of searching segments from which a round walks the full grid instead (same bits).") \
  X(HIP, LANE_GATHER_SPREAD,  INT,   32768,      CALL,  ANY,     "Lane passes: searching segments per step of the packed waves' fill (about 2048 waves before a wave takes more per class; same bits).") \
  X(HIP, LANE_CSR_BELOW,      INT,   16,         CALL,  ANY,     "Lane passes: below this percentage an ungathered round runs the CSR form instead of the full grid (same bits).") \
  X(HIP, LANE_TRACE,          INT,   0,          CALL,  ANY,     "Lane passes: 1 layout figures at set-up, 2 the form of every round, on stderr.") \
  X(HIP, CACHED,              INT,   AUTO,       SETUP, ANY,     "Cached gather row sweep: 0 off, 1 wherever the rows fit (and the LDS variant's 160 KB budget instead of 53 KB), AUTO: 0 for tiled = 1, else -1 = the measured rule of glrm_setup_cached.") \
  X(HIP, CACHED_REGS,         INT,   1,          SETUP, ANY,     "Cached row sweep: 1 the register variant, 0 the LDS variant (fp64 only; kept in glrm_handle::cached_variant).") \
  X(HIP, CACHED_WAVES,        INT,   2,          SETUP, ANY,     "Cached register sweep: waves that share a row; 1 and 4 are experiment switches of the fp64 kernels (another summation order; kept in glrm_handle::cached_waves).") \
  X(HIP, CACHED_PERSIST,      INT,   1,          CALL,  ANY,     "Cached register sweep: the persistent form of the two-wave kernel (same bits).") \
  X(HIP, BLOCKED,             INT,   AUTO,       SETUP, ANY,     "Phase-aligned gather passes: bit0 rows, bit1 columns, 0 off (AUTO: 0 for tiled = 1, else -1 = the measured rule of glrm_setup_blocked; a float handle takes them only where asked).") \
  X(HIP, BLOCKED_TPS,         INT,   AUTO,       SETUP, ANY,     "Phase-aligned passes: tiles per super-tile (AUTO: about 128 MB of the opposing factor).") \
  X(HIP, BLOCKED_LONG_FROM,   INT,   0,          SETUP, ANY,     "Phase-aligned column passes: columns of at least this many observations run on the 8-wave gather sweep; 0 or unset: max(4096, 2 x the whole problem's mean column length).") \
  X(HIP, BLOCKED_SUPPOS,      INT,   1,          SETUP, ANY,     "Phase-aligned passes: start table per (segment, super-tile): 0 the kernels search, 1 built where it takes at most 1/16 of the list bytes, 2 built whatever its size; 0 at a pass also drops the table for that pass (the one per-call read: same bits).") \
  X(HIP, BLOCKED_FILL,        INT,   50,         SETUP, ANY,     "Phase-aligned passes: percent of the chip's residency one launch covers; read at the handle's first sweep of each pass kind, into Side::blocked_cap (changes no sum).") \
  X(HIP, BLOCKED_GATE,        INT,   AUTO,       CALL,  ANY,     "Phase-aligned passes: phase gate in rows of the opposing factor (AUTO: 5120 for fp64 storage, 16384 for f32; changes no sum).") \
  X(HIP, BLOCKED_TRACE,       INT,   0,          CALL,  ANY,     "Phase-aligned passes: super-tile and start-table figures at set-up, on stderr.") \
  X(HIP, ARRIVAL,             INT,   1,          CALL,  ANY,     "glrm_hip_step_y_arrival: the column pass families start super-tile by super-tile on the blocks of X that have arrived; 0 waits for all of X (same bits).") \
  X(HIP, ARRIVAL_DYNAMIC,     INT,   1,          CALL,  ANY,     "glrm_hip_step_y_arrival, phase-aligned passes: enqueue super-tiles in true arrival order (host polls the events); 0 = the announced order (same bits).") \
  X(HIP, GRAPH,               INT,   1,          CALL,  ANY,     "glrm_hip_fit: one outer iteration of the gather sweeps as a hipGraph (same launches).") \
  X(HIP, ROCTX,               INT,   1,          CALL,  ANY,     "roctx ranges around every half-step; read once per process, at the first half-step.") \
  X(HIP, MULTI_CHUNK,         INT,   8192,       SETUP, ANY,     "General sweeps: observations per chunk of a column that is swept by several workgroups (the grouping of its partial sums); 0 = never split.") \
  X(HIP, MULTI_KINDS,         INT,   1,          CALL,  ANY,     "General sweeps: kernels specialised by the model's loss kinds; 0 = the all-kinds kernels (same bits).") \
  X(HIP, MULTI_REGS,          INT,   1,          CALL,  ANY,     "General row sweep: blocks of at most 8 vectors held in registers (same bits).") \
  X(HIP, TOPK_GRID,           INT,   1024,       CALL,  ANY,     "glrm_hip_xy_select: workgroups of a selection pass (4 per CU; the result does not depend on it).") \
  X(HIP, TOPK_FINISH,         INT,   4194304,    CALL,  ANY,     "glrm_hip_xy_select: early finish once the bucket holds at most this many entries (the result does not depend on it).") \
  X(HIP, TRANSPOSE_CHUNK,     INT,   1500000000, SETUP, ANY,     "GLRM_PROBLEM_ROWS_FROM_COLS: entries per row range of the device transpose (values outside (0, 1.5e9] mean 1.5e9).") \
  X(HIP, TRANSPOSE_TRACE,     INT,   0,          CALL,  ANY,     "GLRM_PROBLEM_ROWS_FROM_COLS: step times on stderr (every step drains the stream).") \
  X(HIP, EXCHANGE_RCCL,       INT,   AUTO,       SETUP, ANY,     "Sharded fits: 1 = exchange the factors through RCCL (AUTO: glrm_multi_options.exchange).") \
  X(HIP, MULTI_ARRIVAL,       INT,   AUTO,       SETUP, ANY,     "Sharded fits: Y half-steps start on the blocks of X as they arrive (AUTO: 1 unless glrm_multi_options.arrival = 2).") \
  X(EXCHANGE, EMULATE_GBPS,   FLOAT, 0,          SETUP, TESTING, "Link emulator: rate of one direct-exchange link in GB/s; 0 or unset = off (the one TESTING row the product library knows: it refuses a positive value).")
// the rows that exist in libglrm_hip_testing.so only: the product library does not even hold their names (tests/test_abi.py)
#ifdef GLRM_HIP_TESTING
#define GLRM_KNOBS_TESTING(X) \
  X(HIP, RCCL_LIB,            PATH,  AUTO,       SETUP, TESTING, "Library opened instead of librccl.so (the suite's stand-in); read once per process (AUTO: librccl.so).") \
  X(HIP, RCCL_ALLOW_SHARED,   INT,   0,          SETUP, TESTING, "Lets shards that share a device use the RCCL path (the suite's stand-in library).") \
  X(HIP, TEST_FAIL_FINALIZE,  INT,   0,          SETUP, TESTING, "Not 0: glrm_hip_finalize fails half way (the set-up-failed latch cannot be reached otherwise).") \
  X(EXCHANGE, EMULATE_DILATE, INT,   AUTO,       SETUP, TESTING, "Link emulator: factor the rate is divided by (AUTO: the largest number of shards that share a device).") \
  X(EXCHANGE, EMULATE_MODE,   INT,   AUTO,       SETUP, TESTING, "Link emulator: 1 stream wait-value, 2 delay kernels (AUTO: 1 where the device supports hipStreamWaitValue64).")
#else
#define GLRM_KNOBS_TESTING(X)
#endif
// clang-format on

enum class Knob : int {
#define X(prefix, suffix, kind, dflt, when, build, doc) suffix,
  GLRM_KNOBS(X)
#undef X
};

namespace glrm_knobs {
enum Kind { INT, FLOAT, PATH };
constexpr double AUTO = 0; // (an AUTO row's default is the site's: knob_or / knob_path)
struct Row { const char* name; Kind kind; double dflt; };
constexpr Row table[] = {
#define X(prefix, suffix, kind, dflt, when, build, doc) {"GLRM_" #prefix "_" #suffix, kind, dflt},
    GLRM_KNOBS(X)
#undef X
};
static inline const char* text(Knob k) { // the variable's value; nullptr where it is unset or empty
  const char* v = getenv(table[(int)k].name);
  return (v && *v) ? v : nullptr;
}
} // namespace glrm_knobs

// an INT row: the variable's value, or `computed` (the AUTO rows) / the table's default
static inline int knob_or(Knob k, int computed) {
  const char* v = glrm_knobs::text(k);
  return v ? atoi(v) : computed;
}
static inline int knob(Knob k) { return knob_or(k, (int)glrm_knobs::table[(int)k].dflt); }
// "set and positive": the variable's value where it is, else `otherwise` (the *_LONG_FROM / *_BATCH / *_CHUNK rows and the FLOAT row)
static inline double knob_positive(Knob k, double otherwise) {
  const char* v = glrm_knobs::text(k);
  const double x = !v ? 0.0 : glrm_knobs::table[(int)k].kind == glrm_knobs::FLOAT ? atof(v) : (double)atoi(v);
  return x > 0.0 ? x : otherwise;
}
// the PATH row: the variable's value, or nullptr
static inline const char* knob_path(Knob k) { return glrm_knobs::text(k); }
