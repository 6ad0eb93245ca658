/*
 * glrm_hip_storage.h -- the storage extension of libglrm_hip.so: glrm_options.storage = 1 keeps A, X and Y in fp32 and computes in
 * fp64.  Three kernel families have a float form: the gather sweeps (both views),
 * the register variant of the cached row sweep (rows of at most 104 observations at padded rank 64, 208 at padded rank 32) and the
 * phase-aligned gather passes (both views, every padded rank), the last only where GLRM_HIP_BLOCKED asks for them at create.
 *
 * An extension header like glrm_hip_scale.h and glrm_hip_init.h: include/glrm_hip.h keeps its entry points, GLRM_HIP_ABI_VERSION
 * and every struct size (glrm_options.storage is the field that was `reserved0`, must be 0, at the same offset), and the CPU oracle
 * has no counterpart.  A host that leaves the field 0 is unaffected.
 *
 * What storage = GLRM_STORAGE_F32 means -- it changes what is STORED, not how anything is added:
 *   stored as float   the observation values of both views; X and Y, with the same leading dimension glrm_hip_factor_ld(h) and the
 *                     same zero padding, counted in floats.
 *   staying double    the step sizes, objcol / objrow and the penalties, every accumulator, every loss and regularizer evaluation,
 *                     the line search.
 *   narrowing         C's (float) conversion, round to nearest even: at create for A, in set_factors / fit / objective for factors
 *                     handed in as doubles.  The NaN check on A runs before narrowing.  A finite double that narrows to +-Inf is
 *                     GLRM_ERR_NONFINITE, for A and for factors (factors are checked on the host before the handle is touched).
 *                     Widening on the way out is exact, so everything get_factors and fit return is float-representable.
 *   the half-step     is the fp64 kernel's, with one addition: after the prox step every component of the trial point is rounded,
 *                     xn = (double)(float)xn, BEFORE the trial pass and before the regularizer is evaluated.  The line search
 *                     compares objectives at the point that will be stored; an accepted point is stored exactly; the recorded
 *                     objective is the objective of the stored factors and the strict-decrease test keeps its meaning.
 *   summation order   unchanged: the same lane layout, waves per segment, observations in flight, butterfly and wave combine as the
 *                     fp64 kernels of the same family.  A lane's chunk of a factor vector is one 8-byte load instead of a 16-byte
 *                     one, widened in the fma that uses it.
 *   families          Columns run on the gather sweeps.  Rows run on the gather sweeps (glrm_hip_sum_order: GLRM_ORDER_STRIDED,
 *                     cached_maxlen = -1; short rows on one wave) unless the handle takes the cached row sweep: then rows of at most
 *                     cached_maxlen = 104 / 208 observations are summed by two waves (cached_waves = 2, kernel_stats.tiled bit 64),
 *                     exactly as on an fp64 handle of that family, and longer rows stay on the gather sweep.  GLRM_HIP_CACHED=1 at
 *                     create takes the family wherever the layout allows (padded rank 32 or 64), =0 never.  Unset: DESIGN.md
 *                     section 4.13 says which rule the measurement left.  The LDS variant of the family, its 1- / 4-wave experiment
 *                     kernels (GLRM_HIP_CACHED_REGS, GLRM_HIP_CACHED_WAVES) have no float form and are ignored on a float handle.
 *                     GLRM_HIP_BLOCKED at create (bit 0 rows, bit 1 columns, as for fp64; glrm_options.tiled = 1 handles included)
 *                     puts a view whose lists are in tile order on the phase-aligned gather passes: kernel_stats.tiled bits 16 / 32,
 *                     glrm_hip_sum_order reports GLRM_ORDER_WINDOWED with the super-tile geometry (in rows) and the long_from of an
 *                     fp64 handle on the same problem, the GLRM_HIP_BLOCKED_* knobs work as for fp64, rows the cached sweep wants stay
 *                     with it, and columns of at least long_from observations run on the float 8-wave gather sweep.  Unset, a float
 *                     handle never takes that family (no auto rule is adopted: DESIGN.md section 4.13).
 *   memory            the handle keeps NO fp64 copy of the values or the factors: the float values of both views (the double arrays
 *                     are released at the end of create), float X and Y.  set_factors / get_factors stage one unpadded factor in
 *                     doubles on the device for the duration of the call.  GLRM_PROBLEM_BORROW_DEVICE_ARRAYS is honoured for
 *                     reading only: the handle copies the index arrays and narrows the values into arrays of its own.
 *   buffers           glrm_hip_bind_buffers: dX and dY are float buffers of ld*m and ld*n elements; dObjCol, dObjRow stay doubles.
 *
 * Supported on such a handle: create / destroy, signature, fit, objective, factor_ld, bind_buffers, set_factors / get_factors,
 * reset_stepsizes, step_x / step_y, col_losses, row_penalties / col_penalties, set_regularizers (scales and element-wise kinds),
 * sum, synchronize, kernel_stats, sum_order, storage.  glrm_options.tiled = 0 and 1 both mean the families above (the LDS-tiled
 * family has no float form); waves_row / waves_col work as for fp64.
 *
 * Refused with GLRM_ERR_UNSUPPORTED, with a message that names the storage mode, before the handle is touched:
 *   dense_A hand-over; any loss with dim > 1; wrapped regularizers and vector regularizers (kinds >= GLRM_REG_QUAD_CONSTRAINT), at
 *   create or in set_regularizers; sum_order = 1; tiled = 2; quad_gram = 1; GLRM_PROBLEM_DEFER_SETUP and glrm_hip_multi_create;
 *   step_x_range, step_y_arrival; gradstep_x / gradstep_y, fit_sparse; subset; init_svd; impute, error_metric;
 *   glrm_hip_scale_columns; glrm_hip_init_kmeanspp.
 * These read or revert fp64 lists and factors, or run kernel families that have no fp32 form.
 */
#ifndef GLRM_HIP_STORAGE_H
#define GLRM_HIP_STORAGE_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLRM_STORAGE_F64 0
#define GLRM_STORAGE_F32 1

/* The handle's storage (GLRM_STORAGE_*), or GLRM_ERR_INVALID for a NULL handle. */
int glrm_hip_storage(glrm_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_STORAGE_H */
