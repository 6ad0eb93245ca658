"""sample_at / sample_missing_at / sample / sample_missing: DRAWS from the fitted model, where ``impute_at`` gives point predictions.

``sample(glrm)`` and ``sample_missing(glrm)`` of the reference (src/sample.jl) through ``glrm_hip_sample_at``
(include/glrm_hip_sample.h, which is the specification): one device pass returns draws for listed (row, column)
pairs, whole rows or whole columns, nothing of size m x n exists anywhere, and every draw is a pure function of
(seed, row, column, X, Y, lists) -- not of the blocking, the order of the query or its mode.  A pair queried twice gets the same draw;
a fresh replicate needs a fresh seed.

The rules, by (domain, loss): Real x QuadLoss draws u + z sd_j (Gaussian); Bool x LogisticLoss a Bernoulli with p = 1 / (1 + exp(-u));
Categorical x MultinomialLoss a level with weights exp(u_v); Ordinal or Categorical x another multi-dimensional loss a level with
weights exp(-evaluate(loss, u, level)); every other pair returns ``impute_at``'s value, as the reference's fallback does.

Deviations from the reference: the level walk returns ``D.min + index`` (the reference the 1-based index: the same wherever
``D.min = 1``); Bool x a multi-dimensional loss is refused; a Real column is never switched to Ordinal for integer-typed data (pass
``domains``); the model's loss scales are never written; ``noise="residual"`` (the default) uses the residual spread sd_j = sqrt(v_j)
the reference's comment intends, ``noise="reference"`` the 1 / sqrt(v_j) its literal line computes.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .domains import _resolve, pack_domains
from .fit import _ensure_handle
from .params import HipProxGradParams
from .predict import _query

__all__ = ["sample_at", "sample_missing_at", "sample", "sample_missing"]

HEADER = "include/glrm_hip_sample.h"


def _seed(seed, rng):
    if (seed is None) == (rng is None):
        raise ValueError("exactly one of seed (an integer) and rng (a numpy Generator) is required: a draw is a function of the seed")
    if seed is not None:
        return int(seed) & 0xFFFFFFFFFFFFFFFF
    return int(rng.integers(0, 2 ** 64, dtype=np.uint64))             # one 64-bit integer


def _run(glrm, rows, cols, seed, rng, noise, noise_sd, keep_observed, X, Y, domains, params, engine):
    api = engine if engine is not None else _capi.hip_api()
    params = HipProxGradParams() if params is None else params
    api._sample("sample_at")                                          # an engine without the extension is refused by name
    if rows is None and cols is None:
        raise ValueError("sample_at needs rows, cols or both; every entry of the model is sample(glrm)")
    seed = _seed(seed, rng)
    rows, cols, shape = _query(glrm, rows, cols)
    doms = _resolve(glrm, domains)
    if len(doms) != glrm.n:
        raise ValueError(f"{len(doms)} domains for {glrm.n} columns")
    if noise_sd is not None:
        noise = "given"
    if noise not in _capi.SAMPLE_NOISE:
        raise ValueError(f"noise must be one of {sorted(_capi.SAMPLE_NOISE)}, got {noise!r}")
    if noise == "given" and noise_sd is None:
        raise ValueError('noise="given" needs noise_sd, one value per column')
    X = np.asfortranarray(glrm.X if X is None else X, dtype=np.float64)
    Y = np.asfortranarray(glrm.Y if Y is None else Y, dtype=np.float64)
    h = _ensure_handle(glrm, api, params, allow_dense=False)[0]
    out, kept, sd = api.sample_at(h, X, Y, pack_domains(doms), glrm.m, glrm.n, rows, cols, seed=seed, noise=noise, noise_sd=noise_sd,
                                  keep_observed=keep_observed)
    return out, kept, sd, seed, api.sample_at_info()


def sample_at(glrm, rows=None, cols=None, *, seed=None, rng=None, noise="residual", noise_sd=None, keep_observed=False, X=None, Y=None,
              domains=None, params=None, engine=None):
    """sample_at(glrm, rows, cols; seed | rng, noise, noise_sd, keep_observed, X, Y, domains, params): a draw at every queried entry.

    ``rows`` / ``cols`` and the shape of the result as for ``impute_at``: both (0-based, equal lengths) = pairs, a vector; only
    ``rows`` = those rows x all columns; only ``cols`` = all rows x those columns (slabs Fortran-ordered).  Neither: ValueError --
    every entry of the model is ``sample(glrm)``.

    Exactly one of ``seed`` (an integer, taken mod 2^64) and ``rng`` (a numpy Generator, from which ONE 64-bit integer is drawn) is
    required.  ``noise``: "residual" (default; sd_j = sqrt(v_j), v_j the mean squared residual of column j over the handle's
    column-view list), "reference" (1 / sqrt(v_j)) or "given" with ``noise_sd`` (n values; passing ``noise_sd`` implies "given").
    ``keep_observed``: an entry whose column is in its row's resident row-view list keeps the stored value (``sample_missing``).

    Refusals (``GLRMError``): as for ``impute_at``; a QUERIED column that cannot be sampled is ERR_UNSUPPORTED.  An engine without the
    extension (the CPU oracle of the tests) is refused by name with the header's path."""
    return _run(glrm, rows, cols, seed, rng, noise, noise_sd, keep_observed, X, Y, domains, params, engine)[0]


def sample_missing_at(glrm, rows=None, cols=None, **kw):
    """``sample_at(..., keep_observed=True)``: observed entries keep their stored value, the others are drawn."""
    kw["keep_observed"] = True
    return sample_at(glrm, rows, cols, **kw)


def sample(glrm, *, seed=None, rng=None, noise="residual", noise_sd=None, keep_observed=False, X=None, Y=None, domains=None, params=None,
           engine=None):
    """sample(glrm): the full m x n matrix of draws, through the rows slab -- for small models, as ``impute`` is.  Records
    ``glrm._sample_info``: the seed, ``noise_sd`` (the sd_j that were used) and the counters of ``glrm_hip_sample_at_info``."""
    out, kept, sd, seed, info = _run(glrm, np.arange(glrm.m), None, seed, rng, noise, noise_sd, keep_observed, X, Y, domains, params, engine)
    glrm._sample_info = dict(info, seed=seed, noise_sd=sd)
    return out


def sample_missing(glrm, **kw):
    """sample_missing(glrm): ``sample`` with the observed entries (the resident row view's) keeping their stored values."""
    kw["keep_observed"] = True
    return sample(glrm, **kw)
