/*
 * glrm_hip_impute_at.h -- the impute_at extension of libglrm_hip.so: the imputed values of a LIST of entries of the model (pairs, whole
 * rows or whole columns), and optionally their errors against given values, computed on the device without anything m x n.
 * glrm_hip_impute writes the full matrix; this answers "what does the model predict for these (row, column) pairs, and how far is that
 * from these held-out values" at sizes where the matrix cannot exist.
 *
 * An extension header like glrm_hip_recommend.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected.
 *
 *   Handle   as in glrm_hip_topk.h: a finalized, unsharded list handle.  GLRM_ERR_UNSUPPORTED for a dense (dense_A) handle and for a
 *            float-storage handle (glrm_options.storage = 1); GLRM_ERR_INVALID for a NULL, deferred or sharded handle.  Models with
 *            multi-dimensional losses are served (unlike glrm_hip_row_topk).
 *   Factors  as in glrm_hip_topk.h: X, Y host, k x m and k x d, column-major, uploaded through glrm_hip_set_factors; both NULL: the
 *            factors resident in the handle; one NULL and one non-NULL is GLRM_ERR_INVALID.
 *   Value    u = +0.0; for c in 0 .. k-1: u = fma(X[c,i], Y[c,v], u) for each of the d vectors v of column j, then the imputation rule
 *            of glrm_hip_impute (the same device function): every output has the bits the same entry has in glrm_hip_impute's matrix.
 */
#ifndef GLRM_HIP_IMPUTE_AT_H
#define GLRM_HIP_IMPUTE_AT_H

#include "glrm_hip.h"

#define GLRM_IMPUTE_AT_PAIRS 0
#define GLRM_IMPUTE_AT_ROWS 1
#define GLRM_IMPUTE_AT_COLS 2

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The imputed value of every queried entry, in index order t = 0 .. T-1.
 *
 *   mode  GLRM_IMPUTE_AT_PAIRS  n_rows == n_cols == T; entry t is (rows[t], cols[t]); any order, repeats allowed
 *         GLRM_IMPUTE_AT_ROWS   cols == NULL, n_cols == 0; the queried rows x all n columns, T = n_rows * n, column-major like
 *                               glrm_hip_impute: entry r + j * n_rows is (rows[r], j)
 *         GLRM_IMPUTE_AT_COLS   rows == NULL, n_rows == 0; all m rows x the queried columns, T = m * n_cols: entry i + c * m is (i, cols[c])
 *   rows, cols     host, 0-based, in [0, m) and [0, n)
 *   domains        host, n descriptors, as for glrm_hip_impute
 *   truth          host, T values, or NULL.  With it, err[t] = error_metric(domains[j], losses[j], u, truth[t]) -- the squared error or
 *                  misclassification of the imputed value, the term glrm_hip_error_metric adds per observation -- and *err_total is
 *                  the sum of err in index order, added by the fixed-order device sum behind glrm_hip_sum: a function of the inputs,
 *                  not of block_entries.  No standardization, no per-column grouping: those stay with the caller.
 *   block_entries  0: the engine chooses how many entries go through the device at a time;  > 0: that many (for tests; capped so that
 *                  the scratch of a block stays below 1 GiB)
 *   out            host, T values
 *   err, err_total host, T values / one value; each may be NULL; both must be NULL when truth is NULL
 *
 * Refusals (nothing is written): everything listed under Handle and Factors above;  GLRM_ERR_INVALID for an unknown mode, a negative
 * count, counts or pointers that do not fit the mode, an index outside its range, NULL domains or out, err / err_total without truth,
 * block_entries < 0, or an invalid domain descriptor;  GLRM_ERR_UNSUPPORTED if a QUERIED entry lies in a column whose (domain, loss)
 * pair has no imputation rule in the reference (such a column that no queried entry touches is not an error), or for a row / column
 * list of a slab mode above 2^26 entries.  T == 0 returns GLRM_OK and writes only *err_total = 0.0 (where asked for).
 *
 * Mechanism: entries go through the device in blocks; inside a block they are partitioned on the device into scalar-loss entries
 * (a workgroup gathers the k-vectors of 256 entries with whole-cache-line loads into an LDS stage, one lane per entry runs the chain)
 * and entries of multi-dimensional columns (one thread per entry, x_i read once).  No waiting between workgroups, no global atomics.
 */
int glrm_hip_impute_at(glrm_handle* h, const double* X, const double* Y, const glrm_domain* domains,
                       const int64_t* rows, int64_t n_rows, const int32_t* cols, int64_t n_cols, int32_t mode,
                       const double* truth, int64_t block_entries,
                       double* out, double* err, double* err_total);

/*
 * Diagnostics of the calling thread's last successful glrm_hip_impute_at: the blocks the entries went through the device in, and how
 * many entries took the scalar-loss path and the multi-dimensional path.  Any pointer may be NULL.
 */
int glrm_hip_impute_at_info(int64_t* blocks, int64_t* entries_fast, int64_t* entries_general);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_IMPUTE_AT_H */
