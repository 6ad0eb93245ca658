/*
 * glrm_hip_recommend.h -- the recommend extension of libglrm_hip.so: for every queried row, the kper columns with the highest
 * score u_ij of X'Y, the columns the row has already observed left out -- computed from X, Y and the handle's resident lists in one
 * pass over the entries (m n k fma).  Nothing of size m x n is ever resident.
 *
 * An extension header like glrm_hip_topk.h: include/glrm_hip.h, GLRM_HIP_ABI_VERSION and every struct layout are unchanged, and
 * the CPU oracle has no counterpart.  A host that never calls it is unaffected.
 *
 *   Handle   as in glrm_hip_topk.h: a finalized, unsharded list handle.  GLRM_ERR_UNSUPPORTED for a dense (dense_A) handle, for a
 *            float-storage handle (glrm_options.storage = 1) and for a model with a multi-dimensional loss (d != n).
 *            GLRM_ERR_INVALID for a NULL, deferred or sharded handle.  The message is in glrm_hip_last_error().
 *   Factors  as in glrm_hip_topk.h: X, Y host, k x m and k x n, column-major, uploaded through glrm_hip_set_factors; both NULL: the
 *            factors resident in the handle; one NULL and one non-NULL is GLRM_ERR_INVALID.
 *   u_ij     the definition of glrm_hip_topk.h (u = +0.0; for c in 0 .. k-1: u = fma(X[c,i], Y[c,j], u)), computed by the same device
 *            function: an entry has the bits it has in glrm_hip_xy_select, glrm_hip_precision_scan and glrm_hip_impute.
 */
#ifndef GLRM_HIP_RECOMMEND_H
#define GLRM_HIP_RECOMMEND_H

#include "glrm_hip.h"

/* the largest kper: the kept list of a row is held by one wave, two entries per lane */
#define GLRM_ROW_TOPK_MAX 128

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The kper best candidates of every query r = 0 .. n_rows-1 (row i = rows[r]).
 *
 * Order: the candidates of query r are all columns j in [0, n), minus -- with exclude = 1 -- the columns in row i's resident row-view
 * (train) list; membership is by value, list order and duplicates do not matter.  Candidates are ranked by the key of u_ij descending,
 * then by column ascending.  The key is the one of glrm_hip_topk.h (Julia's isless): NaN greatest, every NaN one value, -0.0 below
 * +0.0.  So a NaN score ranks first.  The order is strict and total: the answer is a function of X, Y and the lists and of nothing else
 * -- not of col_splits, not of how the query rows are blocked, not of the order in which workgroups finish.
 *
 *   rows        host, n_rows row indices in [0, m), in any order, repeats allowed (every occurrence gets its own output row);
 *               NULL: the rows 0 .. m-1, n_rows must be m
 *   kper        candidates per row, 1 .. GLRM_ROW_TOPK_MAX
 *   exclude     0: no column is left out;  1: the columns in the row's resident (train) list are
 *   col_splits  0: the engine chooses;  > 0: that many column spans (clamped to the number of 128-column tiles; for tests)
 *   out_cols, out_vals   host, n_rows x kper, row-major: out[r * kper + t] is the t-th best candidate of query r, best first (0-based
 *               column, its u_ij; a NaN score comes back as the quiet NaN 0x7FF8000000000000).
 *               Padding: if a row has c < kper candidates, positions t >= c hold column -1 and the quiet NaN 0x7FF8000000000000.
 *   out_count   host, n_rows, or NULL: min(kper, c)
 *
 * Refusals (nothing is touched): everything listed under Handle and Factors above;  GLRM_ERR_INVALID for a row index outside [0, m),
 * n_rows < 0 (or != m with rows == NULL), kper < 1, exclude outside {0, 1}, col_splits < 0, or NULL out_cols / out_vals;
 * GLRM_ERR_UNSUPPORTED for kper > GLRM_ROW_TOPK_MAX.  n_rows == 0 returns GLRM_OK and writes nothing.
 *
 * Mechanism: a workgroup owns a band of 128 query rows and one span of column tiles, computes 128 x 128 tiles of u with the tile
 * function of the top-k extension and tests every entry against its row's current kper-th best (key, column); the few that pass are
 * staged in LDS and merged, after the exclusion test, into the row's sorted kept list in scratch memory.  A second kernel merges the
 * spans' lists of a row and writes the padding.  No global atomics, no waiting between workgroups.  Query rows go in blocks so that
 * scratch memory stays below 1 GiB.
 */
int glrm_hip_row_topk(glrm_handle* h, const double* X, const double* Y, const int64_t* rows, int64_t n_rows, int32_t kper, int32_t exclude,
                      int32_t col_splits, int32_t* out_cols, double* out_vals, int32_t* out_count);

/*
 * Diagnostics of the calling thread's last successful glrm_hip_row_topk (like glrm_hip_xy_select_info, per thread): the column spans
 * its first block of query rows ran with, the blocks of query rows, and the entries of the spans' kept lists the final merge read
 * (at most col_splits_used x kper per query).  Any pointer may be NULL.
 */
int glrm_hip_row_topk_info(int32_t* col_splits_used, int64_t* row_blocks, int64_t* candidates_merged);

#ifdef __cplusplus
}
#endif
#endif /* GLRM_HIP_RECOMMEND_H */
