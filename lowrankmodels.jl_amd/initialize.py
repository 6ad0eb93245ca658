"""The reference's initializers (src/initialize.jl) on the engine.

init_kmeanspp! (src/initialize.jl:8-33): k-means++ seeding over the observed entries, on the device from the model's resident handle
(``glrm_hip_init_kmeanspp``, include/glrm_hip_init.h); the host only draws the random numbers and glrm.Y is overwritten.

init_svd! (src/initialize.jl:35-132): the standardized, real-valued expansion of the observed
entries is decomposed on the device from the model's resident handle (``glrm_hip_init_svd``); glrm.X / glrm.Y are overwritten
with sqrt(S) U' and sqrt(S) V' diag(std).

init_nndsvd! (src/initialize_nmf.jl): NNDSVD of the scaled observed entries with optional soft-impute rounds, on the device from the
model's resident handle (``glrm_hip_init_nndsvd``, include/glrm_hip_nmf.h); glrm.X / glrm.Y are overwritten with W' and H."""
from __future__ import annotations

import numpy as np

from . import _capi
from .fit import _ensure_handle
from .params import HipProxGradParams
from .regularizers import lastentry1


def _views_agree(glrm):
    """The expanded MATRIX of the reference has one entry per observed (e, f): the two lists must hold the same entries once."""
    m = glrm.m
    I = np.repeat(np.arange(m, dtype=np.int64), np.diff(glrm._rowptr))
    rk = I + m * glrm._colidx.astype(np.int64)
    J = np.repeat(np.arange(glrm.n, dtype=np.int64), np.diff(glrm._colptr))
    ck = glrm._rowidx.astype(np.int64) + m * J
    rk.sort()
    ck.sort()
    return len(rk) == len(ck) and (len(rk) < 2 or np.all(rk[1:] != rk[:-1])) and np.array_equal(rk, ck)


def init_svd_(glrm, offset=True, scale=True, TOL=1e-10, *, max_iter=0, tol=1e-10, seed=1, engine=None, check=True):
    """init_svd!(glrm; offset, scale, TOL) -> glrm.

    ``offset`` only takes effect in the reference when ``typeof(glrm.rx) == lastentry1`` (src/initialize.jl:37) -- glrm.rx is a
    Vector there, so the branch never runs; the same holds here (glrm.rx is a list), and ``scale`` depends on ``offset``.
    ``tol`` / ``max_iter`` / ``seed`` steer the subspace iteration that replaces Arpack's svds."""
    offset = offset and type(glrm.rx) is lastentry1  # never true, as in the reference
    scale = scale and offset
    if TOL != 1e-10:
        raise NotImplementedError("the engine uses the reference's default TOL = 1e-10 for vanishing standard deviations")
    if check and not _views_agree(glrm):
        raise ValueError("init_svd! works on the matrix of observed entries: observed_features and observed_examples must list "
                         "the same entries, each once")
    api = engine if engine is not None else _capi.hip_api()
    h = _ensure_handle(glrm, api, HipProxGradParams(), allow_dense=False)[0]
    X = np.zeros((glrm.k, glrm.m), order="F")
    Y = np.zeros((glrm.k, glrm.d), order="F")
    sv, iters = api.init_svd(h, X, Y, max_iter=max_iter, tol=tol, seed=seed)
    glrm.X[...] = X
    glrm.Y[...] = Y
    glrm._init_svd_info = dict(singular_values=sv, iterations=iters)
    return glrm


def _duplicated_pair(ptr, idx, count):
    """The first (segment, opposing index) a view lists twice, or None."""
    seg = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    key = np.sort(seg * int(count) + np.asarray(idx, dtype=np.int64))
    dup = np.flatnonzero(key[1:] == key[:-1])
    return None if len(dup) == 0 else (int(key[dup[0]] // count), int(key[dup[0]] % count))


def init_nndsvd_(glrm, scale=True, zeroh=False, variant="std", max_iters=0, *, svd_max_iter=0, svd_tol=1e-10, seed=1, engine=None):
    """init_nndsvd!(glrm; scale, zeroh, variant, max_iters) -> glrm  (src/initialize_nmf.jl).

    NNDSVD (Boutsidis & Gallopoulos 2007) of the matrix that holds ``losses[j].scale * A[i, j]`` (``scale``) on the observed pairs and 0
    elsewhere, followed by ``max_iters`` soft-impute rounds in which the missing entries are ``X'Y`` of the round before.  The reference
    calls NMF.jl's ``nndsvd``, which is not part of its tree; the routine is specified in include/glrm_hip_nmf.h and runs on the device
    from the model's resident handle (``glrm_hip_init_nndsvd``) without a dense m x n matrix.  ``variant``: ``"std"`` (zeros stay 0) or
    ``"a"`` (zeros become the mean of the matrix); ``"ar"`` is refused, its random draws are NMF.jl's own.  ``svd_max_iter`` / ``svd_tol``
    / ``seed`` steer the subspace iteration, as ``max_iter`` / ``tol`` / ``seed`` do in :func:`init_svd_`.

    glrm.Y = H is k x n, so a model with a multi-dimensional loss is refused; the reference assigns the observed entries into a matrix,
    so a pair listed twice -- which the device products would add twice -- is refused too.  Both before anything is touched.  The
    singular values, the (larger, smaller) split products and the subspace iterations per round are kept in ``glrm._init_nndsvd_info``."""
    if glrm.d != glrm.n:
        raise NotImplementedError("init_nndsvd! with multi-dimensional losses: the reference's glrm.Y = H is k x n and has no slot for them")
    if variant == "ar":
        raise NotImplementedError("init_nndsvd! variant ar fills the zeros with NMF.jl's own random draws, which cannot be restated; "
                                  "use variant 'std' or 'a'")
    if variant not in ("std", "a"):
        raise ValueError(f"variant must be 'std', 'a' or 'ar', got {variant!r}")
    if max_iters < 0:
        raise ValueError(f"max_iters = {max_iters} is negative")
    for what, ptr, idx, count in (("observed_features", glrm._rowptr, glrm._colidx, glrm.n), ("observed_examples", glrm._colptr, glrm._rowidx, glrm.m)):
        dup = _duplicated_pair(ptr, idx, count)
        if dup is not None:
            raise ValueError(f"init_nndsvd! assigns the observed entries into a matrix: {what}[{dup[0]}] lists {dup[1]} twice (0-based), "
                             "which the device products would count twice")
    if not _views_agree(glrm):
        raise ValueError("init_nndsvd! works on the matrix of observed entries: observed_features and observed_examples must list the same entries")
    api = engine if engine is not None else _capi.hip_api()
    h = _ensure_handle(glrm, api, HipProxGradParams(), allow_dense=False)[0]
    X = np.zeros((glrm.k, glrm.m), order="F")
    Y = np.zeros((glrm.k, glrm.n), order="F")
    info = api.init_nndsvd(h, X, Y, scale=scale, zeroh=zeroh, variant=variant, max_iters=max_iters, svd_max_iter=svd_max_iter, svd_tol=svd_tol, seed=seed)
    glrm.X[...] = X
    glrm.Y[...] = Y
    glrm._init_nndsvd_info = info
    return glrm


KMEANSPP_WEIGHTS_MAX = 1 << 22 # (k - 1) m entries: above this the per-round weights (a diagnostic) are not copied out


def init_kmeanspp_(glrm, rng=None, *, first=None, uniforms=None, engine=None):
    """init_kmeanspp!(glrm) -> glrm.

    The reference draws ``glrm.Y = randn(k, n)``, the first centre ``sample(1:m)`` and one ``rand()`` per later centre (inside
    ``wsample``); here they come from ``rng`` (a numpy Generator, default ``default_rng()``) in that order: ``standard_normal((k, n))``,
    ``integers(m)``, ``random(k - 1)``.  ``first`` (0-based) and ``uniforms`` replace the last two draws.  Y is k x n in the reference,
    indexed by data column, so a model with a multi-dimensional loss is refused before anything is touched.  The chosen rows and the
    sampling weights of every round ((k-1) x m; None above KMEANSPP_WEIGHTS_MAX entries) are kept in ``glrm._init_kmeanspp_info``; X
    is left alone."""
    if glrm.d != glrm.n:
        raise NotImplementedError("init_kmeanspp! with multi-dimensional losses: the reference's Y = randn(k, n) has no slot for them "
                                  "(src/initialize.jl:12,16 index Y by data column)")
    api = engine if engine is not None else _capi.hip_api()
    rng = np.random.default_rng() if rng is None else rng
    k, m, n = glrm.k, glrm.m, glrm.n
    Y = np.asfortranarray(rng.standard_normal((k, n)))
    first = int(rng.integers(m)) if first is None else int(first)
    uniforms = rng.random(k - 1) if uniforms is None else np.asarray(uniforms, dtype=np.float64)
    h = _ensure_handle(glrm, api, HipProxGradParams(), allow_dense=False)[0]
    centers, weights = api.init_kmeanspp(h, Y, first, uniforms, want_weights=(k - 1) * m <= KMEANSPP_WEIGHTS_MAX, m=m)
    glrm.Y[...] = Y
    glrm._init_kmeanspp_info = dict(centers=centers, weights=weights)
    return glrm
