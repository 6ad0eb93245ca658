/*
 * glrm_hip_scale.h -- the scaling extension of libglrm_hip.so: `scale=true` of the GLRM constructor, computed on the device.
 *
 * An extension header like glrm_synth.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected.
 *
 * Reference interfaces replaced (paths relative to the LowRankModels.jl tree):
 *   GLRM_SCALE_EQUILIBRATE <- equilibrate_variance!(glrm, columns)   src/modify_glrm.jl:34-53
 *   GLRM_SCALE_PROB        <- prob_scale!(glrm, columns)             src/modify_glrm.jl:60-82
 *   M-estimates, avgerror  <- M_estimator(l, a), avgerror(l, a)      src/losses.jl:116-352
 */
#ifndef GLRM_HIP_SCALE_H
#define GLRM_HIP_SCALE_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLRM_SCALE_EQUILIBRATE 0 /* equilibrate_variance!, src/modify_glrm.jl:34-53 */
#define GLRM_SCALE_PROB 1        /* prob_scale!,           src/modify_glrm.jl:60-82 */

/*
 * The new loss and Y-regularizer scales of the columns [col_begin, col_end) of a problem DESCRIPTION.  Stateless: the scales must be
 * known before glrm_hip_create, which bakes the loss scales into the handle.  The caller applies the returned values with its own
 * mul!(l, s) / mul!(r, s) (which SET the scale, src/losses.jl:61-64) and creates its handle afterwards.
 *
 * Read from `p`: colptr / colvals (the column view), losses / n_losses (1 or n, indexed by GLOBAL column), ry / n_ry (1 or
 * col_end - col_begin), col_begin / col_end, flags bit 0 and dense_A; from `o` (may be NULL): device_id and stream (NULL = the default
 * stream; the call returns after the work on it has finished).  Everything else, the row view included, is ignored and may be NULL.
 * With GLRM_PROBLEM_DEVICE_ARRAYS the lists are read in place; host lists are uploaded for the call and freed.
 *
 * Per column, with nobs = its number of listed entries, M = the M-estimate of its loss over them, avg_loss = (1/nobs) sum l(M, a)
 * at the descriptor's CURRENT scale and variance = the corrected (1/(nobs-1)) sample variance (NaN for nobs == 1).  The
 * comparisons are the reference's; a NaN compares false:
 *   nobs == 0                       both scales unchanged
 *   EQUILIBRATE                     loss_scale = scale / avg_loss   if avg_loss > 0,  else unchanged
 *                                   ry_scale   = scale / variance   if variance > 0,  else unchanged
 *   PROB, QuadLoss                  loss_scale = 1 / (2 variance)   if variance > 1e-12, else unchanged
 *   PROB, HuberLoss                 loss_scale = 1 / (2 avg_loss)   if avg_loss > 1e-12, else unchanged
 *   PROB, every other kind          loss_scale = 1
 *   PROB                            ry_scale unchanged
 * prob_scale! takes its statistics over skipmissing(A[:, i]); here they run over the listed entries of the column.  The two coincide
 * when Omega is the set of non-missing entries.  (For an EMPTY Quad / Huber column the reference's prob_scale! falls through to
 * mul!(l, 1); this entry point leaves every empty column alone.)
 *
 * M-estimates (src/losses.jl): Quad mean; L1 / Huber / OrdinalHinge median (even nobs: a/2 + b/2 of the two middle order statistics);
 * Quantile Julia's default quantile, h = (nobs-1) q, a_(floor h) + (h - floor h)(a_(floor h + 1) - a_(floor h)); Periodic
 * (T/2pi) atan(sum sin / sum cos) + T/2; Poisson log(mean); Logistic log(N+d) - log(N-d) with d = #(a != 0) (the reference's formula,
 * kept although it is not the minimiser); WeightedHinge +1 / 0 / -1 as case_weight_ratio is above / at / below r = N / #(a > 0) - 1
 * (+Inf when no value is positive).  Order statistics are exact data values; -0.0 and +0.0 compare equal, as in a sort, and an order
 * statistic that is a zero is returned as +0.0.  Non-finite M-estimates (an all-true Logistic column, an all-zero Poisson column) flow
 * through IEEE arithmetic into the comparisons above.
 *
 * Every sum is a fixed-shape tree whose shape depends on the column's own length only: two calls, a call on a column block of the
 * problem and a call with host instead of device arrays return the same bits.
 *
 * loss_scale, ry_scale: col_end - col_begin doubles each (host).  m_est, avg_loss, variance: the same length, or NULL; entries that the
 * mode does not need for a column (and every entry of an empty column) are NaN.
 *
 * Errors: GLRM_ERR_UNSUPPORTED for a multi-dimensional loss (kind >= GLRM_LOSS_MULTINOMIAL: their M-estimators do not run in the
 * reference either) among the requested columns and for a dense_A problem; GLRM_ERR_INVALID for NULL outputs / lists and inconsistent
 * sizes; the message is in glrm_hip_last_error().
 */
int glrm_hip_scale_columns(const glrm_problem* p, const glrm_options* o, int32_t mode, double* loss_scale, double* ry_scale,
                           double* m_est, double* avg_loss, double* variance);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_SCALE_H */
