/*
 * glrm_hip_stream.h -- the streaming extension of libglrm_hip.so: the reference's one-pass streaming_fit! / streaming_impute!
 * (src/algorithms/quad_streaming.jl) on the device.  glrm_hip_stream_rows visits the rows first .. m-1 (0-based) once, in ascending order
 * wherever two rows share a column: each row is solved against Y as it stands, reports its residual, and moves its columns of Y by one
 * gradient step; every `interval` rows all of Y is divided by a constant.
 *
 * An extension header like glrm_hip_als.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and the CPU
 * oracle has no counterpart.  A host that never calls it is unaffected: no existing entry point, option, default, kernel choice or
 * summation order changes.  It adds no environment knob.  This header is the specification: a host can restate it bit for bit
 * (tests/stream_ref.py does, in numpy).
 *
 * Two things are done differently from the reference's loop; neither changes what it computes.
 *   DECAY IS LAZY.  The reference divides all of Y every `interval` rows.  Here a column carries the number of divisions it has received
 *   (epoch[j], 0 at the start of a call) and receives the ones it missed at the moment a row reads it, as ONE division by p = c^d.  This is
 *   the reference's d successive divisions up to rounding; p may overflow to +Inf (y / p = 0) where the reference underflows to 0.
 *   ROWS RUN BY LEVEL.  Rows are "strictly one after another" only where they share a column.  THE PLAN below gives every row a level;
 *   rows of one level share no written column and run side by side, levels run in stream order.
 *
 * THE PLAN (glrm_hip_stream_plan: pure host code; glrm_hip_stream_rows builds the same plan from the handle's row view in the handle's own
 * order).  lastw[j] = lastr[j] = 0 for every column.  Then, for each row i = first .. m-1 in ascending order:
 *   L = 1 + max(lastw[j], lastr[j] over the row's observed columns; lastw[j] over its query columns);  L = 1 for a row with neither.
 *   lastw[j] = L for each observed column;  lastr[j] = max(lastr[j], L) for each query column.
 * With sequential = 1, row first + t has level t + 1.  A row whose list names a column twice is a dup row.
 * Launches: every maximal run of consecutive levels that hold one row each is one chain launch -- one workgroup walking its rows in
 * ascending order (it may be cut into pieces of bounded length so that no kernel runs for seconds); every other level is one launch, one
 * workgroup per row.  nlaunches counts runs and levels, not pieces.  Order between launches is stream order and nothing else: no flags,
 * no spinning, no cooperative launch, no graph capture; no kernel ever waits on another workgroup.
 *
 * A ROW'S ARITHMETIC, in fp64, every operation rounded on its own (a multiply then an add, never an fma).  The list is (j_t, a_t),
 * t = 0 .. L-1, in the order the handle holds it (the rule of glrm_hip_als.h).  gamma is the scale of rx[i] (0 for ZeroReg), sy the common
 * scale of ry.
 *   Decay constant  c = 1 + ((2 * stepsize) * (double)interval) * sy.
 *   Decay count     row i has the 1-based number i1 = i + 1 and must see  D(i) = floor((i1 - 1) / interval) - floor(first / interval)
 *                   divisions on each of its columns.
 *   Pending decay   with d = D(i) - epoch[j] > 0:  p = c, then p = p * c repeated d - 1 times, then y_a = y_a / p for every component, and
 *                   epoch[j] = D(i).  c == 1.0 skips all of it.
 *   Solve           G and b exactly as in glrm_hip_als.h with w_t = 1;  M_aa = G_aa + 2 * gamma -- the reference's system
 *                   (quad_streaming.jl:53), not the ALS one.  The Cholesky, the pivot rule, the short rule and the substitutions are those
 *                   of glrm_hip_als.h, word for word (the short rule: gamma == 0 with L < k).
 *   Queries         each query column j of the row gives  sum_a y'_a * x_a,  a ascending from +0.0, where y' is the column with its
 *                   pending decay applied in registers and NOT written back (a reader owns no column) and x the row after its solve.
 *                   This runs before the row's update.
 *   Residual        r_t = (sum_a v_ta * x_a, a ascending from +0.0) - a_t;  objective[i - first] = sum_t r_t * r_t, t ascending from
 *                   +0.0, one accumulator.
 *   Update          y_a = y_a - (stepsize * r_t) * x_a for every t (v_t is read before any update of the row).  The updates of one
 *                   column that is named twice are applied in ascending t.  Dup rows are the only place where this and the decay can
 *                   race, and the plan flags them.
 *   Kept row        (GLRM_ALS_KEPT_SHORT or GLRM_ALS_KEPT_PIVOT) X keeps every bit, there is no update, objective = NaN; its queries
 *                   use the row as it stands.
 *   After the last row every column receives its outstanding divisions up to floor(m / interval) - floor(first / interval).
 *   NOT written: rows of X below first, both step-size arrays, the trial / accept counters, obj_by_row / obj_by_col; glrm_kernel_stats is
 *   not touched; components k .. ld-1 of both factors stay as they are.
 *
 * REFUSALS, nothing written.  GLRM_ERR_INVALID: a NULL handle, a handle that is not finalized, no factors on the device yet, first
 * outside 1 .. m, interval < 1, a stepsize that is not finite and > 0, half-given query pointers (qptr, qcol and qout go together),
 * query offsets that do not ascend from 0, a query column outside 0 .. n-1, glrm_hip_stream_info before a run.  GLRM_ERR_UNSUPPORTED,
 * naming what was found: a loss that is not QuadLoss; a QuadLoss scale that is not exactly 1.0 (the reference's loop ignores the scale);
 * rx or ry not plain QuadReg with scale >= 0 (ZeroReg is taken as scale 0); ry scales that are not all equal; k > GLRM_STREAM_MAX_K;
 * dense (dense_A), storage = f32 and shard handles; a model on the general sweeps.
 *
 * NOT BUILT.  Sharded, f32-storage and dense handles.  The plan is built on the host (one pass over the row view, reported as plan_ms).
 * One row is one workgroup's work: a long row is never split over workgroups.
 */
#ifndef GLRM_HIP_STREAM_H
#define GLRM_HIP_STREAM_H

#include "glrm_hip.h"
#include "glrm_hip_als.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLRM_STREAM_MAX_K 64

/* The plan of rows first .. m-1 of a CSR row view (duplicates allowed), with the queries of every row (qptr: m + 1 offsets, qcol:
 * qptr[m] columns) or NULL, NULL.  Pure host code: needs no device, touches no handle.  level: m - first entries, levels from 1, or NULL.
 * Any other output pointer may be NULL too. */
int glrm_hip_stream_plan(int64_t m, int64_t n, int64_t first, const int64_t* rowptr, const int32_t* colidx, const int64_t* qptr, const int32_t* qcol,
                         int32_t sequential, int64_t* level, int64_t* nlevels, int64_t* nlaunches, int64_t* max_width, int64_t* dup_rows);

/* Streams rows first .. m-1 over X and Y as they stand on the device; rows below first are the caller's initial block and are not
 * touched.  qptr / qcol / qout (host; NULL, NULL, NULL for none): the queries of every row as above and qptr[m] results.  objective
 * (host, m - first entries, or NULL).  The call synchronises, copies qout and objective down, then returns. */
int glrm_hip_stream_rows(glrm_handle* h, int64_t first, double stepsize, int64_t interval, int32_t sequential, const int64_t* qptr, const int32_t* qcol,
                         double* qout, double* objective);

/* What the last glrm_hip_stream_rows did: the rows per status (GLRM_ALS_SOLVED / _KEPT_SHORT / _KEPT_PIVOT), the plan's levels, launches
 * and widest level, the host time the plan took, and with `status` (host memory, one byte per streamed row, or NULL) each row's own.
 * Any pointer may be NULL. */
int glrm_hip_stream_info(glrm_handle* h, int64_t* solved, int64_t* kept_short, int64_t* kept_pivot, int64_t* nlevels, int64_t* nlaunches, int64_t* max_width,
                         double* plan_ms, int8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_STREAM_H */
