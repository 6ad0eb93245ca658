"""recommend: which unobserved columns score highest for a row?

The question a fitted recommender is asked, answered on the device from the model's resident lists by ``glrm_hip_row_topk``
(include/glrm_hip_recommend.h): one pass over the entries of X'Y (m n k fma) selects, for every queried row, the k
best columns, with the columns the row has already observed left out.  Nothing of size m x n exists, on the host or on the device, and
the resident lists -- the only copy of "what has this row already seen" -- are never left.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .fit import _ensure_handle
from .params import HipProxGradParams


def recommend(glrm, rows=None, k=10, *, exclude_observed=True, X=None, Y=None, params=None, engine=None):
    """recommend(glrm, rows=None, k=10; exclude_observed, X, Y, params) -> (cols, scores): the ``k`` best columns of every queried row.

    The candidates of a row are all columns j in [0, n), minus -- with ``exclude_observed`` -- the columns in the row's
    ``observed_features``.  They are ranked by the key of the score u_ij descending, then by column ascending, where u_ij is the engine's
    one definition of an entry of X'Y (the ascending fma chain over k, the value ``impute`` returns for a QuadLoss / RealDomain model)
    and the key is the one ``precision_at_k`` sorts by (Julia's isless: NaN greatest, every NaN one value, -0.0 below +0.0).  So a NaN
    score ranks first.  The order is strict and total: the answer depends on X, Y and the lists and on nothing else.

    ``rows``: 0-based row indices in any order, repeats allowed (every occurrence gets its own output row); None: every row.
    ``X``, ``Y``: k x m and k x n factors; None: ``glrm.X`` / ``glrm.Y``.
    Returns ``cols`` (int32, n_rows x k, best first) and ``scores`` (float64, n_rows x k).  Padding: a row with c < k candidates holds
    column -1 and NaN (the quiet NaN 0x7FF8000000000000) at the positions t >= c.

    Refusals (``GLRMError``): a row index outside [0, m) and k < 1 are ERR_INVALID; k > 128 (GLRM_ROW_TOPK_MAX), a model with a
    multi-dimensional loss, fp32 storage and an engine without the extension (the CPU oracle) are ERR_UNSUPPORTED.

    The model's cached LIST handle is used (created on first use).  A fully observed QuadLoss model is fitted on the dense handle by
    default, which the engine refuses here: fit it with ``HipProxGradParams(dense=False)`` and pass the same ``params`` here, as for
    ``precision_at_k``, and the fit and the queries share one resident handle.
    """
    api = engine if engine is not None else _capi.hip_api()
    params = HipProxGradParams() if params is None else params
    X = np.asfortranarray(glrm.X if X is None else X, dtype=np.float64)
    Y = np.asfortranarray(glrm.Y if Y is None else Y, dtype=np.float64)
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    api._recommend("row_topk")                                       # an engine without the extension is refused before a handle is made
    h = _ensure_handle(glrm, api, params, allow_dense=False)[0]
    cols, scores, _ = api.row_topk(h, X, Y, rows, k, exclude=bool(exclude_observed))
    return cols, scores
