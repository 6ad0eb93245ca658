/*
 * glrm_hip_als.h -- the ALS extension of libglrm_hip.so: the EXACT half-step of a quadratic model.  glrm_hip_als_solve replaces every
 * local row of X (or every local column of Y) by the closed-form minimiser of its part of the objective with the opposing factor as it
 * stands -- the row solve inside the reference's streaming_fit! (src/algorithms/quad_streaming.jl:53), for every segment at once.
 * streaming_fit! itself is glrm_hip_stream_rows (include/glrm_hip_stream.h), which runs this solve row after row.
 *
 * An extension header like glrm_hip_transform.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected: no existing entry point, option, default, kernel choice
 * or summation order changes.  It adds no environment knob.  This header is the specification: a host can restate it bit for bit
 * (tests/als_ref.py does, in numpy).
 *
 * WHAT A SOLVE COMPUTES.  A segment is a row (side 0) or a column (side 1).  Its list is (index_t, a_t), t = 0 .. L-1, in the order the
 * handle holds it (the caller's order; a view the engine had to tile-sort is read in that private, tile-sorted order).  v_t is the
 * opposing vector index_t names (a column of Y for side 0, of X for side 1), w_t the QuadLoss scale of the observation's column (side 1:
 * the segment's own column, constant), gamma the scale of the segment's own regularizer, QuadReg(gamma), or 0 for ZeroReg.  The new point
 * x minimises   sum_t w_t (v_t.x - a_t)^2 + gamma |x|^2,   the engine's own objective for the segment (evaluate = scale * sum abs2,
 * src/regularizers.jl:58, src/losses.jl:144), so   (G + gamma I) x = b,  G = sum_t w_t v_t v_t',  b = sum_t w_t a_t v_t.
 * This is NOT the streaming file's `2 * rx[i].scale * I`: that system does not minimise the objective the reference reports.
 *
 * THE ARITHMETIC, in fp64, every operation rounded on its own (a multiply then an add, never an fma):
 *   Gram          u_t = w_t * v_t (componentwise).  For a >= b:  G_ab = sum_t u_ta * v_tb,  and  b_a = sum_t u_ta * a_t;  every sum starts
 *                 from +0.0, runs over t ascending and has ONE accumulator per entry.  Only the lower triangle exists.  No lane layout, wave
 *                 count, staging chunk or grid size changes a bit.
 *   Diagonal      M_aa = G_aa + gamma;  M_ab = G_ab otherwise.
 *   Cholesky      left-looking, column j ascending, rows i = j .. k-1:  s = M_ij;  s = s - L_ic * L_jc  for c = 0 .. j-1 ascending;
 *                 L_jj = sqrt(s) on the diagonal, L_ij = s / L_jj below it.
 *   Pivot rule    tol = (k * 2^-52) * maxd, where maxd = M_00 and then, for a = 1 .. k-1, maxd = M_aa if M_aa > maxd.  A diagonal s that is
 *                 not greater than tol (`!(s > tol)`: a NaN fails, and everything fails when maxd = 0) ends the segment as
 *                 GLRM_ALS_KEPT_PIVOT -- the usual n * eps * max-diagonal rank tolerance.
 *   Short rule    before any arithmetic: gamma == 0 with L < k is GLRM_ALS_KEPT_SHORT (the system has no unique solution; without the rule
 *                 a rank-64 segment of 63 observations passes every pivot at condition 3e18 and returns garbage).
 *   Substitution  forward  z_i = (b_i - sum_{c < i, ascending} L_ic z_c) / L_ii,  back  x_i = (z_i - sum_{c > i, descending} L_ci x_c) / L_ii,
 *                 each subtracting one product at a time from the running value.
 *   Kept segments keep every bit of their point.  An empty segment with gamma > 0 solves to exactly +0.0 (no special case); with gamma = 0
 *   it is GLRM_ALS_KEPT_SHORT.  Components k .. ld-1 of the factor (glrm_hip_factor_ld) stay zero.
 *   NOT written: the opposing factor, both step-size arrays, the trial / accept counters, obj_by_row / obj_by_col; glrm_kernel_stats is
 *   not touched.
 *
 * REFUSALS, nothing written.  GLRM_ERR_INVALID: a NULL handle, a side outside {0, 1}, a handle that is not finalized, no factors on the
 * device yet, glrm_hip_als_info before the first solve of that side.  GLRM_ERR_UNSUPPORTED, naming what was found: a column whose loss is
 * not QuadLoss; a descriptor of the SOLVED side that is not a plain QuadReg or ZeroReg (wrapped, offset or vector regularizers, a negative
 * or NaN scale; the other side's regularizers do not enter the system and are not looked at); k > GLRM_ALS_MAX_K; dense (dense_A),
 * storage = f32 and shard handles (a glrm_multi is another type and has no such entry point); a model on the general sweeps.
 *
 * NOT BUILT.  One segment is one workgroup's work: a list is never split over workgroups (a Zipf head column of 50 000 observations and a
 * 3-observation column are the same kernel, scheduled longest first; as in glrm_hip_scale_columns).  The Gram matrix is accumulated on
 * the vector units: the fp64 matrix cores add in an internal order (GLRM_ORDER_OTHER) that cannot be restated, which would forfeit the
 * contract above.
 */
#ifndef GLRM_HIP_ALS_H
#define GLRM_HIP_ALS_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLRM_ALS_MAX_K 64
/* status of a segment after a solve */
#define GLRM_ALS_SOLVED 0
#define GLRM_ALS_KEPT_SHORT 1 /* penalty scale 0 and fewer than k observations: the system has no unique solution */
#define GLRM_ALS_KEPT_PIVOT 2 /* a pivot failed the rule above */

/* side 0: every local row of X against Y as it stands; side 1: every local column of Y against X as it stands.  Asynchronous on the
 * handle's stream, like glrm_hip_step_x. */
int glrm_hip_als_solve(glrm_handle* h, int32_t side);

/* What the last glrm_hip_als_solve of `side` did (synchronises): the segments per status, and with `status` (host memory, one byte per
 * local segment, or NULL) each segment's own.  Any pointer may be NULL. */
int glrm_hip_als_info(glrm_handle* h, int32_t side, int64_t* solved, int64_t* kept_short, int64_t* kept_pivot, int8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_ALS_H */
