"""numpy restatement of glrm_hip_row_topk (include/glrm_hip_recommend.h): per queried row, every column that is not in the row's list,
ranked by the key of tests/precision_ref.py descending and then by column ascending; the first kper, padded with column -1 and the
quiet NaN 0x7FF8000000000000."""
import numpy as np

import precision_ref as R


def row_topk(XY, rows, kper, lists=None):
    """XY: the m x n matrix of scores; rows: the queried rows (None: all); lists: per MODEL row the columns to leave out (None: none).
    Returns (cols int32 [n_rows, kper], vals float64 [n_rows, kper], count int32 [n_rows])."""
    XY = np.asarray(XY, dtype=np.float64)
    m, n = XY.shape
    rows = np.arange(m) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    cols = np.full((len(rows), kper), -1, dtype=np.int32)
    vals = np.full((len(rows), kper), 0, dtype=np.uint64)
    vals[...] = R.QNAN
    count = np.zeros(len(rows), dtype=np.int32)
    for r, i in enumerate(rows):
        cand = np.ones(n, dtype=bool)
        if lists is not None and len(lists[i]):
            cand[np.asarray(lists[i], dtype=np.int64)] = False
        j = np.flatnonzero(cand)
        key = R.keys(XY[i, j])
        order = np.lexsort((j, ~key))[:kper]                         # key descending (~key ascending), then column ascending
        c = len(order)
        cols[r, :c] = j[order]
        # a NaN score comes back as THE quiet NaN (every NaN is one value), anything else with its own bits
        v = XY[i, j[order]]
        vals[r, :c] = np.where(np.isnan(v), R.QNAN, np.ascontiguousarray(v).view(np.uint64))
        count[r] = c
    return cols, vals.view(np.float64), count


def same(got, ref):
    """Columns and counts as integers, values by their bits."""
    return (np.array_equal(got[0], ref[0]) and got[0].dtype == np.int32 and R.same_bits(got[1], ref[1]) and np.array_equal(got[2], ref[2]))
