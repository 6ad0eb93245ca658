/*
 * glrm_hip_transform.h -- the transform extension of libglrm_hip.so: embedding rows against a FIXED Y.  glrm_hip_solve_x runs
 * inner_iter X half-steps of every local row with Y as it stands -- the row side of one outer iteration of the reference's alternating
 * minimisation (src/algorithms/proxgrad.jl:117-158), which is all of the iteration once Y is held fixed (ScikitLearnBase.transform,
 * src/scikitlearn.jl:94-102) -- and where it can, it runs them in ONE launch that fetches a row's opposing vectors once.
 *
 * An extension header like glrm_hip_topk.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart (a host loops glrm_cpu_step_x there).  A host that never calls it is unaffected: no existing entry
 * point, option, default, kernel choice or summation order changes.
 */
#ifndef GLRM_HIP_TRANSFORM_H
#define GLRM_HIP_TRANSFORM_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * inner_iter X half-steps (glrm_hip_step_x) of every local row, Y as it stands.
 *
 *   Valid on every handle on which glrm_hip_step_x is valid.  inner_iter < 1 (or above 2^31 - 1) is GLRM_ERR_INVALID.
 *   The row step sizes are NOT reset: the caller does that (glrm_hip_reset_stepsizes), as the reference does at the top of an outer
 *   iteration.  Y is never written.
 *   Counters and profile time count what inner_iter calls of glrm_hip_step_x would: glrm_kernel_stats.launches_x grows by inner_iter,
 *   trials_x / accepts_x by the same totals.
 *
 * Two paths; glrm_hip_solve_x_info says which one ran.
 *
 *   FUSED  Taken when the handle COULD run the register variant of the cached row sweep with two waves per row on this problem,
 *          whether or not glrm_hip_step_x runs it there: the row view is not LDS-tiled, not phase-aligned, not dense and not on the
 *          general sweeps; glrm_options.sum_order = 0; rank k in 17 .. 64 (lane layouts (4, 8) and (8, 8)); the row view holds an
 *          observation; GLRM_HIP_CACHED is not 0, and -- fp64 storage -- GLRM_HIP_CACHED_REGS is not 0 and GLRM_HIP_CACHED_WAVES is
 *          unset or 2 (read at create / finalize).  The size thresholds of the cached sweep's auto rule and glrm_options.tiled = 1 are
 *          NOT part of it: they decide what glrm_hip_step_x runs.  So a float handle (glrm_options.storage = 1) gets it without an
 *          environment switch.
 *            Rows of at most 104 observations (k <= 32: 208) run all inner_iter steps in one launch of a register kernel: the row's
 *          (index, value) list, its opposing vectors, its point and its step size are fetched once; every step is the gradient pass at
 *          the current point, the objective recomputed from it, and the backtracking line search; a row that gives up
 *          (step size below min_stepsize) carries on from min_stepsize * 1.1 with its next step; the point, the step size and the
 *          counters are stored once.
 *            Longer rows run inner_iter launches of the gather sweep with the waves their own length asks for, beside that launch.
 *          ORDER of the sums, in words (glrm_hip_sum_order still describes glrm_hip_step_x and is unchanged): GLRM_ORDER_STRIDED with
 *          cached_waves = 2 and cached_maxlen = 104 / 208 -- a lane group adds its observations in ascending order, the groups of a
 *          wave by the butterfly, the two waves of a short row in wave order; a longer row as glrm_sum_order describes the strided
 *          family for its length.
 *          CONTRACT: X, the row step sizes and the trial / accept counters are left with exactly the bits that inner_iter calls of
 *          glrm_hip_step_x leave on a handle of the same problem and storage created under GLRM_HIP_CACHED=1.
 *
 *   LOOP   Every other handle: inner_iter times what glrm_hip_step_x does.  CONTRACT: the bits inner_iter calls of glrm_hip_step_x
 *          leave on the handle itself.
 */
int glrm_hip_solve_x(glrm_handle* h, int64_t inner_iter, double min_stepsize);

/*
 * What the last successful glrm_hip_solve_x on the handle did (GLRM_ERR_INVALID before the first): fused = 1 / 0 for the path,
 * fused_rows = local rows that ran in the register kernel, loop_rows = local rows that ran inner_iter sweep launches (fused = 0: all of
 * them).  Any pointer may be NULL.  It exists so that a caller -- a test -- can tell a fallback from the fused path.
 */
int glrm_hip_solve_x_info(glrm_handle* h, int32_t* fused, int64_t* fused_rows, int64_t* loop_rows);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_TRANSFORM_H */
