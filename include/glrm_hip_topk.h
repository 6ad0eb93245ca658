/*
 * glrm_hip_topk.h -- the top-k extension of libglrm_hip.so: the r-th largest entry of X'Y and the ordered scan for the first hits
 * of precision_at_k, computed from X and Y alone.  Nothing of size m x n is ever resident.
 *
 * An extension header like glrm_hip_init.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected.
 *
 * Reference lines replaced (paths relative to the LowRankModels.jl tree), both inside precision_at_k:
 *   glrm_hip_xy_select      <- XY = X'*Y; q = sort(XY[:], rev=true)[ntrain]      src/cross_validate.jl:273-274
 *   glrm_hip_precision_scan <- the double loop over XY[i,j] >= q                  src/cross_validate.jl:275-297
 *
 * Common to both entries
 *   Handle   a finalized, unsharded list handle.  GLRM_ERR_UNSUPPORTED for a dense (dense_A) handle, for a float-storage handle
 *            (glrm_options.storage = 1) and for a model with a multi-dimensional loss (d != n: the reference's XY[i,j] with
 *            j in 1:n only has a meaning when Y has one vector per data column).  GLRM_ERR_INVALID for a NULL, deferred or sharded
 *            handle.  The message is in glrm_hip_last_error().
 *   Factors  X, Y: host, k x m and k x n, column-major (X[c + k i]); uploaded through glrm_hip_set_factors, as glrm_hip_impute does.
 *            Both NULL: the factors resident in the handle (after a fit or glrm_hip_set_factors).  One NULL and one non-NULL is
 *            GLRM_ERR_INVALID.
 *   u_ij     is defined once:   u = +0.0;  for c in 0 .. k-1:  u = fma(X[c,i], Y[c,j], u)
 *            -- the ascending fma chain over the true k, the chain of glrm_hip_impute.  One device function computes it for every
 *            selection pass and for the scan, so an entry has the same bits everywhere.  The matrix cores are not used: their
 *            internal order over k is not this chain.
 */
#ifndef GLRM_HIP_TOPK_H
#define GLRM_HIP_TOPK_H

#include "glrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * q = the rank-th largest (1-based) of all m n values u_ij = sort(XY[:], rev=true)[rank].
 *
 * Order: Julia's isless -- -0.0 < +0.0, NaN is greatest; all NaNs are one value (q comes back as the quiet NaN 0x7FF8000000000000)
 * and count as equal.  Concretely the entries are ordered by the order-preserving 64-bit key of their bit pattern b:
 *     key = all ones for a NaN;  b | 2^63 for a value with the sign bit clear;  ~b for a value with the sign bit set.
 *   n_gt   out or NULL: the number of entries whose key is above key(q)
 *   n_eq   out or NULL: the number of entries whose key equals key(q);  n_gt < rank <= n_gt + n_eq
 * rank outside [1, m n] is GLRM_ERR_INVALID (the reference raises a BoundsError).
 *
 * Mechanism: most-significant-digit radix selection over the keys, 8 bits per pass.  A pass recomputes every u_ij from tiles of X and
 * Y staged in LDS (128 x 128 outputs per workgroup, 8 x 8 per lane); a workgroup counts one digit of the entries whose higher digits
 * equal the prefix found so far in integer counters in LDS and stores its 256 counts to a slot of its own; a second kernel adds the
 * slots; the host reads 256 totals and picks the bucket that holds the rank.  No global atomics, no waiting between workgroups;
 * the counts are integers, so q, n_gt and n_eq cannot depend on the launch shape.  Once the bucket holds few enough entries (4 Mi)
 * one more pass writes its keys out and a device sort finishes; the result does not depend on whether or where that happens.
 * Cost: m n k fma per pass, at most 8 passes.
 */
int glrm_hip_xy_select(glrm_handle* h, const double* X, const double* Y, int64_t rank, double* q, int64_t* n_gt, int64_t* n_eq);

/*
 * Diagnostics of the calling thread's last successful glrm_hip_xy_select (like glrm_hip_last_error, per thread): the number of passes
 * over X'Y it made (counting passes, plus one if a write-out pass finished it) and the number of keys that write-out pass sorted
 * (0: the counting passes ran through all eight digits).  Either pointer may be NULL.
 */
int glrm_hip_xy_select_info(int32_t* passes, int64_t* sorted_keys);

/*
 * The loop of src/cross_validate.jl:275-297, taken literally: walk i = 0 .. m-1, then j = 0 .. n-1, and stop as soon as kprec entries
 * have counted.  An entry with u_ij >= q (IEEE compare: a NaN q matches nothing) is
 *     a true positive   if j is in the test list of row i            -- it counts;
 *     a false positive  else if j is not in the train list of row i  -- it counts;
 *     ignored           otherwise.
 * The train lists are the handle's own resident row view (membership does not depend on list order); the test lists are uploaded for
 * the call.  Duplicates and empty rows are legal in both.
 *   train         the handle of the TRAIN model
 *   q             the threshold, usually from glrm_hip_xy_select
 *   test_rowptr   host, m + 1 offsets, 0-based, test_rowptr[0] == 0, non-decreasing
 *   test_colidx   host, test_rowptr[m] column indices in [0, n)
 *   kprec         hits to find; kprec <= 0 returns true_pos = false_pos = rows_scanned = 0 at once
 *   block_rows    0: the engine chooses (rows go in blocks, in order; blocks grow geometrically to bound the round trips, and the host
 *                 stops launching once kprec hits are reached).  > 0: every block has that many rows (for tests).  Counts and hits are
 *                 identical for every value.
 *   true_pos, false_pos   out: the counts when the walk stopped
 *   hit_rows, hit_cols, hit_is_true   out or NULL, capacity kprec each: the entries that counted, in the order of the walk (0-based)
 *   rows_scanned  out or NULL: the index after the last row the reference's loop would have entered (m if it never stops)
 * GLRM_ERR_INVALID for NULL true_pos / false_pos / test_rowptr, a malformed test list, and hit arrays of which only some are NULL.
 */
int glrm_hip_precision_scan(glrm_handle* train, const double* X, const double* Y, double q,
                            const int64_t* test_rowptr, const int32_t* test_colidx, int64_t kprec, int64_t block_rows,
                            int64_t* true_pos, int64_t* false_pos, int64_t* hit_rows, int64_t* hit_cols, uint8_t* hit_is_true,
                            int64_t* rows_scanned);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_TOPK_H */
