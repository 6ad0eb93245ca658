/*
 * glrm_hip_cd.h -- the coordinate-descent extension of libglrm_hip.so: a step-size-free half-step for QuadLoss models whose regularizer
 * is ZeroReg, QuadReg, OneReg (the lasso) or NonNegConstraint (NNMF).  glrm_hip_cd_solve runs `sweeps` cyclic coordinate-descent sweeps
 * on every local row of X (or every local column of Y) with the opposing factor as it stands.  Each coordinate update is the EXACT
 * minimiser of the segment's part of the objective in that coordinate, so a sweep cannot raise the objective and there is no step size and
 * no line search.  This is the solver scikit-learn's NMF and lasso use by default; the reference has no counterpart.
 *
 * An extension header like glrm_hip_als.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and the CPU
 * oracle has no counterpart.  A host that never calls it is unaffected: no existing entry point, option, default, kernel choice or
 * summation order changes (glrm_hip_als_solve included).  It adds no environment knob.  This header is the specification: a host can
 * restate it bit for bit (tests/cd_ref.py does, in numpy).
 *
 * WHAT A SOLVE COMPUTES.  A segment, its list (index_t, a_t), v_t and w_t are those of glrm_hip_als.h.  The segment's own regularizer has
 * a kind and a scale gamma; the accepted kinds are GLRM_REG_ZERO, GLRM_REG_QUAD, GLRM_REG_ONE and GLRM_REG_NONNEG, all with wrap == 0.
 * The segment's part of the objective is   sum_t w_t (v_t.x - a_t)^2 + r(x) = x'Gx - 2 b'x + const + r(x),   r(x) = 0 (ZERO),
 * gamma |x|^2 (QUAD), gamma sum|x_a| (ONE: the engine's evaluate is scale * sum abs), or the indicator of x >= 0 (NONNEG).
 *
 * THE ARITHMETIC, in fp64, every operation rounded on its own (a multiply then an add, never an fma):
 *   Gram          G (lower triangle) and b are exactly those of glrm_hip_als.h:  u_t = w_t * v_t,  G_ab = sum_t u_ta * v_tb (a >= b),
 *                 b_a = sum_t u_ta * a_t,  one accumulator per entry, from +0.0, t ascending.  G_ic with c > i is read as G_ci.
 *   Diagonal      M_aa = G_aa + gamma for QUAD, M_aa = G_aa otherwise.
 *   Tolerance     tol = (k * 2^-52) * maxd, where maxd = M_00 and then, for a = 1 .. k-1, maxd = M_aa if M_aa > maxd (the ALS pivot rule's).
 *   Start         x is the segment's point as stored; for NONNEG every component is first replaced by  x_a > 0 ? x_a : +0.0.
 *   Residual      g_i = b_i;  then for c = 0 .. k-1 ascending  g_i = g_i - G_ic * x_c,  one product at a time.
 *   Sweep         for a = 0 .. k-1 ascending:
 *                   if !(M_aa > tol)  (a NaN fails, and everything fails when maxd = 0) the coordinate is SKIPPED and the GLRM_CD_SKIPPED
 *                     bit of the segment is set: ZERO, QUAD and NONNEG keep the value and go to the next coordinate (no d exists);  ONE
 *                     with gamma > 0 takes new = +0.0 and goes through the update below (ONE with gamma == 0 keeps the value).
 *                   otherwise  rho = g_a + G_aa * x_a  and
 *                     ZERO, QUAD   new = rho / M_aa
 *                     NONNEG       q = rho / M_aa;  new = q > 0 ? q : +0.0
 *                     ONE          h = 0.5 * gamma;  new = rho > h ? (rho - h) / M_aa : rho < -h ? (rho + h) / M_aa : +0.0
 *                                  (the minimiser of G_aa x^2 - 2 rho x + gamma |x|)
 *                   update       d = new - x_a;  for every i:  g_i = g_i - G_ia * d;  then x_a = new.
 *   Stop          at most `sweeps` sweeps.  If every d of a sweep is == 0.0 (a sweep whose coordinates were all kept has none) the solve
 *                 stops after that sweep, sets the GLRM_CD_CONVERGED bit and counts the sweep in sweeps_run.
 *   Components k .. ld-1 of the factor (glrm_hip_factor_ld) stay zero.  An empty segment falls under these rules with no special case:
 *   QUAD and ONE (gamma > 0) give exactly +0.0, ZERO and NONNEG keep the (projected) point and set GLRM_CD_SKIPPED.
 *   NOT written: the opposing factor, both step-size arrays, the trial / accept counters, obj_by_row / obj_by_col; glrm_kernel_stats is
 *   not touched.
 *
 * REFUSALS, nothing written, in the order of glrm_hip_als_solve's.  GLRM_ERR_INVALID: a NULL handle, a side outside {0, 1}, a handle that
 * is not finalized, no factors on the device yet, sweeps outside [1, GLRM_CD_MAX_SWEEPS], glrm_hip_cd_info before the first solve of that
 * side.  GLRM_ERR_UNSUPPORTED, naming what was found: a column whose loss is not QuadLoss; a descriptor of the SOLVED side outside the
 * four kinds, or one that is wrapped or carries a vector; a QUAD or ONE scale that is negative or NaN (the other side's regularizers are
 * not looked at); k > GLRM_CD_MAX_K; dense (dense_A), storage = f32 and shard handles; a model on the general sweeps.
 *
 * NOT BUILT.  As in glrm_hip_als.h: a list is never split over workgroups, and the Gram matrix is accumulated on the vector units.
 */
#ifndef GLRM_HIP_CD_H
#define GLRM_HIP_CD_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLRM_CD_MAX_K 64
#define GLRM_CD_MAX_SWEEPS 256
/* status bits of a segment after a solve */
#define GLRM_CD_CONVERGED 1 /* a whole sweep changed no bit and the solve stopped there */
#define GLRM_CD_SKIPPED 2   /* at least one coordinate failed the denominator rule */

/* side 0: every local row of X against Y as it stands; side 1: every local column of Y against X as it stands.  Asynchronous on the
 * handle's stream, like glrm_hip_step_x. */
int glrm_hip_cd_solve(glrm_handle* h, int32_t side, int32_t sweeps);

/* What the last glrm_hip_cd_solve of `side` did (synchronises): the segments that carry each bit, the sweeps run summed over the
 * segments, and with `status` (one byte per local segment) and `sweeps_run` (one int32 per local segment), both host memory, each
 * segment's own.  Any pointer may be NULL. */
int glrm_hip_cd_info(glrm_handle* h, int32_t side, int64_t* converged, int64_t* skipped, int64_t* sweeps_total, int8_t* status,
                     int32_t* sweeps_run);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_CD_H */
