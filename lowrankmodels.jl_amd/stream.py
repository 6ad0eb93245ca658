"""The reference's streaming method (src/algorithms/quad_streaming.jl) on the device: ``keep_rows``, ``streaming_fit``,
``streaming_impute`` and ``streaming_impute_at`` over glrm_hip_stream_rows (include/glrm_hip_stream.h, which is the specification of the
plan and of the arithmetic).

The first T0 rows initialise Y and their rows of X (init_svd! of keep_rows(glrm, T0)); rows T0 .. m-1 are then visited once.  The history
gets one entry per streamed row -- the squared residual of the row after its solve, NaN for a row the solve kept -- and, as in the
reference, ``ch.times`` is left alone.

A model the engine would refuse is refused here, before a handle exists, with the engine's words.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .convergence import ConvergenceHistory
from .losses import pack_losses
from .params import StreamingParams
from .regularizers import _collapse

HEADER = "include/glrm_hip_stream.h"
_WHAT = "glrm_hip_stream_rows"
QUAD_LOSS, REG_ZERO, REG_QUAD = 0, 0, 1     # include/glrm_hip.h: GLRM_LOSS_QUAD, GLRM_REG_ZERO, GLRM_REG_QUAD


def check_model(glrm):
    """Raise GLRMError(ERR_UNSUPPORTED) for a model glrm_hip_stream_rows refuses -- the messages of csrc/glrm_stream.hip, in its order."""
    def refuse(msg):
        raise _capi.GLRMError(_capi.ERR_UNSUPPORTED, f"{_WHAT}{msg} ({HEADER})")
    if glrm.k > _capi.STREAM_MAX_K:
        refuse(f": rank k = {glrm.k} is above GLRM_STREAM_MAX_K = {_capi.STREAM_MAX_K}")
    for j, l in enumerate(pack_losses(glrm.losses)):
        if int(l["kind"]) != QUAD_LOSS:
            refuse(f": column {j} has loss kind {int(l['kind'])}; the streaming pass needs QuadLoss (kind {QUAD_LOSS}) on every column")
        if float(l["scale"]) != 1.0:
            refuse(f": column {j} is QuadLoss with scale {float(l['scale']):g}; the streaming pass needs a scale of exactly 1 (the reference's loop "
                   "ignores the scale)")
    descs = {"rx": _collapse(glrm.rx)[1], "ry": _collapse(glrm.ry)[1]}
    for name in ("rx", "ry"):
        for s, (kind, wrap, scale) in enumerate(descs[name]):
            if kind not in (REG_QUAD, REG_ZERO) or wrap != 0:
                refuse(f": {name}[{s}] has regularizer kind {kind}, wrap {wrap}; the streaming pass needs a plain QuadReg (kind {REG_QUAD}) or "
                       f"ZeroReg (kind {REG_ZERO})")
            if kind == REG_QUAD and not scale >= 0.0:
                refuse(f": {name}[{s}] is QuadReg with scale {scale:g}; the streaming pass needs a scale >= 0")
    sy = [scale if kind == REG_QUAD else 0.0 for kind, _, scale in descs["ry"]]
    for s in range(1, len(sy)):
        if sy[s] != sy[0]:
            refuse(f": ry[{s}] has scale {sy[s]:g} and ry[0] has {sy[0]:g}; the streaming pass divides all of Y by one constant and needs equal scales")
    if glrm.d != glrm.n:
        refuse(": the model runs on the general sweeps (multi-dimensional losses, wrapped or vector regularizers); the streaming pass does not")


def _check_params(glrm, params):
    if not isinstance(params, StreamingParams):
        raise TypeError("params must be a StreamingParams")
    if not 1 <= params.T0 <= glrm.m:
        raise _capi.GLRMError(_capi.ERR_INVALID, f"{_WHAT}: first must be in 1 .. m = {glrm.m}, got {params.T0}")
    if params.Y_update_interval < 1:
        raise _capi.GLRMError(_capi.ERR_INVALID, f"{_WHAT}: interval must be at least 1, got {params.Y_update_interval}")
    if not (np.isfinite(params.stepsize) and params.stepsize > 0):
        raise _capi.GLRMError(_capi.ERR_INVALID, f"{_WHAT}: stepsize must be finite and > 0, got {params.stepsize:g}")


def keep_rows(glrm, r):
    """keep_rows(glrm, r) (quad_streaming.jl:141-156): a new model on the rows ``r`` of ``glrm`` -- an int T for the first T rows, or a
    ``range`` / (start, stop) of 0-based rows -- with the same losses, ry and rank, the rows' own rx and their observations in order."""
    from .glrm import GLRM
    if isinstance(r, (int, np.integer)):
        b, e = 0, int(r)
    elif isinstance(r, range):
        if r.step != 1:
            raise ValueError("keep_rows takes a contiguous range of rows")
        b, e = r.start, r.stop
    else:
        b, e = (int(v) for v in r)
    if not 0 <= b < e <= glrm.m:
        raise ValueError(f"keep_rows: rows [{b}, {e}) are not a non-empty range inside the model's {glrm.m} rows")
    lo, hi = int(glrm._rowptr[b]), int(glrm._rowptr[e])
    I = np.repeat(np.arange(e - b, dtype=np.int64), np.diff(glrm._rowptr[b:e + 1]))
    J = glrm._colidx[lo:hi].astype(np.int64)
    return GLRM(glrm.A[b:e], list(glrm.losses), list(glrm.rx[b:e]), list(glrm.ry), glrm.k, obs=(I, J), X=glrm.X[:, b:e].copy(), Y=glrm.Y.copy())


def _stream(glrm, params, api, verbose, qptr=None, qcol=None):
    """The pass itself -> (objective per streamed row, query results or None); glrm.X / glrm.Y are updated in place."""
    from .fit import _ensure_handle
    from .initialize import init_svd_
    check_model(glrm)
    _check_params(glrm, params)
    if not api.has_stream:
        api._stream("stream_rows")                                  # refuses by name
    T0 = params.T0
    init = keep_rows(glrm, T0)                                      # quad_streaming.jl:31-35
    try:
        init_svd_(init, engine=api)
    finally:
        init.close()
    glrm.Y[...] = init.Y
    glrm.X[:, :T0] = init.X
    h = _ensure_handle(glrm, api, params, allow_dense=False)[0]
    X = np.asfortranarray(glrm.X, dtype=np.float64)
    Y = np.asfortranarray(glrm.Y, dtype=np.float64)
    if verbose:
        print("Fitting GLRM")
    api.set_factors(h, X, Y)
    obj, qout = api.stream_rows(h, glrm.m, T0, params.stepsize, params.Y_update_interval, sequential=params.sequential, qptr=qptr, qcol=qcol)
    glrm._stream_info = api.stream_info(h)
    api.get_factors(h, X, Y)
    glrm.X[...] = X
    glrm.Y[...] = Y
    return obj, qout


def streaming_fit(glrm, params=None, ch=None, verbose=True, *, engine=None):
    """streaming_fit!(glrm, params; ch, verbose) -> (glrm.X, glrm.Y, ch) (quad_streaming.jl:22-75).  ``ch.objective`` is extended by one
    value per streamed row; ``ch.times`` is left alone, as in the reference.  ``glrm._stream_info`` keeps what the pass did (rows per
    status, levels, launches, widest level, the plan's host time).  ``engine`` is a test hook (an ``_capi.Api``)."""
    params = StreamingParams() if params is None else params
    ch = ConvergenceHistory("StreamingGLRM") if ch is None else ch
    api = engine if engine is not None else _capi.hip_api()
    obj, _ = _stream(glrm, params, api, verbose)
    ch.objective.extend(float(v) for v in obj)
    return glrm.X, glrm.Y, ch


def streaming_impute_at(glrm, rows, cols, params=None, *, engine=None, verbose=False):
    """The imputed values of the streaming pass at the listed entries (0-based ``rows`` >= T0, ``cols``), in any order -> values in the
    caller's order.  Each value is x_i . y_j with x_i the row after its solve and Y as row i found it (quad_streaming.jl:113-118, one
    entry at a time: nothing m x n is formed).  The pass runs as in ``streaming_fit``: glrm.X and glrm.Y are updated."""
    params = StreamingParams() if params is None else params
    api = engine if engine is not None else _capi.hip_api()
    rows, cols = np.asarray(rows, dtype=np.int64).ravel(), np.asarray(cols, dtype=np.int64).ravel()
    if rows.shape != cols.shape:
        raise ValueError("rows and cols must list the same number of entries")
    if rows.size and (rows.min() < params.T0 or rows.max() >= glrm.m):
        raise ValueError(f"streaming_impute_at takes entries of the streamed rows {params.T0} .. {glrm.m - 1}")
    if cols.size and (cols.min() < 0 or cols.max() >= glrm.n):
        raise ValueError(f"streaming_impute_at: a column is outside 0 .. {glrm.n - 1}")
    order = np.argsort(rows, kind="stable")                        # per-row query lists, each in the caller's order
    qptr = np.zeros(glrm.m + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=glrm.m), out=qptr[1:])
    qcol = cols[order].astype(np.int32)
    _, qout = _stream(glrm, params, api, verbose, qptr=qptr, qcol=qcol)
    values = np.empty(rows.size)
    values[order] = qout
    return values


def streaming_impute(glrm, params=None, *, engine=None, verbose=False):
    """streaming_impute!(glrm, params) -> Ahat (quad_streaming.jl:78-139): a copy of A in which every unobserved entry of a streamed row
    holds its imputed value.  The result is a dense m x n matrix and the unobserved entries of the streamed rows are listed one by one:
    for small problems only -- ``streaming_impute_at`` is the form that forms nothing m x n."""
    params = StreamingParams() if params is None else params
    A = glrm.A.toarray() if hasattr(glrm.A, "toarray") else np.asarray(glrm.A)
    Ahat = np.array(A, dtype=np.float64)
    observed = np.zeros((glrm.m, glrm.n), dtype=bool)
    observed[np.repeat(np.arange(glrm.m), np.diff(glrm._rowptr)), glrm._colidx] = True
    T0 = min(max(params.T0, 0), glrm.m)
    rows, cols = np.nonzero(~observed[T0:])
    rows = rows + T0
    Ahat[rows, cols] = streaming_impute_at(glrm, rows, cols, params, engine=engine, verbose=verbose)
    return Ahat
