"""impute_at / error_metric_at: what does the model predict for THESE entries, and how far is that from these held-out values?

``impute`` answers for every entry at once and returns the m x n matrix, which does not exist at the sizes the engine is built for.
``impute_at`` answers for a list of (row, column) pairs, for whole rows or for whole columns through ``glrm_hip_impute_at``
(include/glrm_hip_impute_at.h): the entries go through the device in blocks, nothing of size m x n exists on
the host or on the device, and every value has the bits the same entry has in ``impute``'s matrix.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .domains import BoolDomain, CategoricalDomain, PeriodicDomain, _resolve, pack_domains, pos_mod
from .fit import _ensure_handle
from .params import HipProxGradParams


def _query(glrm, rows, cols):
    """(rows, cols, shape) of a query: both given = pairs, one given = a slab of whole rows / whole columns."""
    if rows is None and cols is None:
        raise ValueError("impute_at needs rows, cols or both; every entry of the model is impute(glrm)")
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if len(rows) and (rows.min() < 0 or rows.max() >= glrm.m):
            raise _capi.GLRMError(_capi.ERR_INVALID, f"impute_at: a row index is outside [0, m = {glrm.m})")
    if cols is not None:
        cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
        if len(cols) and (cols.min() < 0 or cols.max() >= glrm.n):
            raise _capi.GLRMError(_capi.ERR_INVALID, f"impute_at: a column index is outside [0, n = {glrm.n})")
        cols = cols.astype(np.int32)
    if rows is not None and cols is not None:
        if len(rows) != len(cols):
            raise ValueError(f"pairs need as many rows as cols, got {len(rows)} and {len(cols)}")
        return rows, cols, (len(rows),)
    return rows, cols, ((len(rows), glrm.n) if cols is None else (glrm.m, len(cols)))


def _index_full(Ahat, rows, cols):
    if rows is not None and cols is not None:
        return Ahat[rows, cols]
    return np.asfortranarray(Ahat[rows, :] if cols is None else Ahat[:, cols])


def _run(glrm, rows, cols, truth, X, Y, domains, params, engine):
    api = engine if engine is not None else _capi.hip_api()
    params = HipProxGradParams() if params is None else params
    rows, cols, shape = _query(glrm, rows, cols)
    doms = _resolve(glrm, domains)
    if len(doms) != glrm.n:
        raise ValueError(f"{len(doms)} domains for {glrm.n} columns")
    if truth is not None:
        truth = np.asfortranarray(truth, dtype=np.float64)
        if truth.shape != shape:
            raise ValueError(f"truth has shape {truth.shape}, the queried entries {shape}")
    X = np.asfortranarray(glrm.X if X is None else X, dtype=np.float64)
    Y = np.asfortranarray(glrm.Y if Y is None else Y, dtype=np.float64)
    h = _ensure_handle(glrm, api, params, allow_dense=False)[0]
    if api.has_impute_at:
        return api.impute_at(h, X, Y, pack_domains(doms), glrm.m, glrm.n, rows, cols, truth)
    # An engine without the extension (the CPU oracle of the tests): the full matrix, indexed.  A small-model path only -- it forms
    # the m x n matrix this module exists to avoid.
    out = _index_full(api.impute(h, X, Y, pack_domains(doms), glrm.m, glrm.n), rows, cols)
    if truth is None:
        return out
    J = cols if rows is not None and cols is not None else np.broadcast_to(np.arange(glrm.n) if cols is None else cols, shape)
    err = np.empty(shape, order="F")
    for t in np.ndindex(*shape):
        D, imp, a = doms[int(J[t])], float(out[t]), float(truth[t])
        if isinstance(D, (BoolDomain, CategoricalDomain)):
            err[t] = float(imp != a)
        elif isinstance(D, PeriodicDomain):
            err[t] = (pos_mod(D.T, imp) - pos_mod(D.T, a)) ** 2
        else:
            err[t] = (imp - a) ** 2
    return out, err, float(np.sum(err.reshape(-1, order="F")))


def impute_at(glrm, rows=None, cols=None, *, X=None, Y=None, domains=None, params=None, engine=None):
    """impute_at(glrm, rows, cols; X, Y, domains, params): the imputed values of the queried entries.

    ``rows`` and ``cols`` (0-based, equal lengths): the pairs (rows[t], cols[t]), in any order, repeats allowed; returns a vector.
    Only ``rows``: those rows x all n columns, shape (len(rows), n).  Only ``cols``: all m rows x those columns, shape (m, len(cols)).
    Neither: ValueError -- every entry of the model is ``impute(glrm)``.  Slabs come back Fortran-ordered.

    Every value is ``impute(glrm, X, Y, domains)[i, j]`` bit for bit (Bool columns as 1.0 / 0.0): the engine's one definition of an
    entry of X'Y and the same imputation rule.  ``X``, ``Y``: k x m and k x d factors; None: ``glrm.X`` / ``glrm.Y``.  ``domains``: one
    per column; None: each loss's default domain, as for ``impute``.

    Refusals (``GLRMError``): an index outside [0, m) / [0, n) is ERR_INVALID; a QUERIED column whose (domain, loss) pair has no
    imputation rule in the reference is ERR_UNSUPPORTED (``impute`` refuses such a column wherever it is; here a column nobody asks for
    is not an error); fp32 storage is ERR_UNSUPPORTED.

    The model's cached LIST handle is used (created on first use), as for ``recommend``: fit a fully observed QuadLoss model with
    ``HipProxGradParams(dense=False)`` and pass the same ``params`` here, and the fit and the queries share one resident handle.
    An engine without the extension (the CPU oracle of the tests) answers by indexing its full ``impute``: small models only."""
    return _run(glrm, rows, cols, None, X, Y, domains, params, engine)


def error_metric_at(glrm, rows, cols, truth, *, X=None, Y=None, domains=None, params=None, engine=None):
    """error_metric_at(glrm, rows, cols, truth; X, Y, domains, params) -> (err, total): the error of the imputed value of every queried
    entry against ``truth`` (of the shape ``impute_at`` returns for the same ``rows`` / ``cols``), and their sum.

    err[t] = error_metric(domains[j], losses[j], u, truth[t]) of the reference (src/impute_and_err.jl): the squared error of the imputed
    value, the 0-1 misclassification for Bool and Categorical domains, the squared distance on the circle for a Periodic domain -- the
    term ``error_metric`` adds per observation.  ``total`` is the sum of err in index order, added on the device in a fixed order: a
    function of the inputs alone.  No standardization and no per-column grouping: with held-out entries those are the caller's to
    define (``error_metric`` keeps doing them for the model's own observations)."""
    _, err, total = _run(glrm, rows, cols, truth, X, Y, domains, params, engine)
    return err, total
