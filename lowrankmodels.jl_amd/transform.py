"""transform: embed new rows into a fitted model with Y held fixed (reference: ScikitLearnBase.transform, src/scikitlearn.jl:94-102 --
whose own version builds ``ry_fixed`` and never passes it on, so it refits Y from a random start; this one does what it says).

The driver is the reference's outer loop (src/algorithms/proxgrad.jl:107-217) without STEP 2: per outer iteration ``inner_iter_X`` X
half-steps against the fitted Y, the objective over the new rows, the stopping rule.  On the HIP engine the half-steps of an iteration
are ONE call, glrm_hip_solve_x (include/glrm_hip_transform.h): rows of at most 104 observations (208 at k <= 32) fetch their vectors
of Y once for all of them.  An engine without that extension (the CPU oracle of the tests) runs the same iteration as a loop of
``step_x`` calls.
"""
from __future__ import annotations

import copy as _copy
import time

import numpy as np

from . import _capi
from .convergence import ConvergenceHistory, update_ch
from .fit import _ensure_handle, _should_stop
from .glrm import GLRM
from .params import AlsParams, HipProxGradParams
from .regularizers import Regularizer, _collapse


def _row_regularizer(glrm, rx):
    """``rx`` of the new rows: the caller's, else the fitted model's when all of its rows carry the same one."""
    if rx is not None:
        return rx
    same = _collapse(glrm.rx)[0]
    if len(same) != 1:
        raise ValueError("rx is required: the fitted model's rows do not all carry the same regularizer, so there is no one to give the new rows")
    return _copy.copy(same[0])


def _objective_buffers(api, params, n, m):
    """(keep-alive, address of obj_by_col, address of obj_by_row): the per-column / per-row values the engine writes and ``api.sum`` adds,
    in the engine's memory (device arrays for the HIP engine, host arrays for a host engine)."""
    if api.device_type == "cuda":
        import torch
        dev = torch.device("cuda", params.device_id if params.device_id >= 0 else torch.cuda.current_device())
        oc, orow = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)  # the engine launches on a stream of its own
        return (oc, orow), oc.data_ptr(), orow.data_ptr()
    oc, orow = np.zeros(n), np.zeros(m)
    return (oc, orow), oc.ctypes.data, orow.ctypes.data


def transform(glrm, A_new, params=None, *, obs=None, rx=None, X0=None, rng=None, api=None, exact=False):
    """Embed the rows of ``A_new`` (m_new x n, the fitted model's columns) into the fitted ``glrm``: minimise over X alone the objective of
    ``GLRM(A_new, glrm.losses, rx, glrm.ry, glrm.k, obs=obs, X=X0, Y=glrm.Y)``.  Returns ``(X_new, ch)``: X_new is k x m_new float64
    (float-representable under ``storage="f32"``), ch the ConvergenceHistory.  ``glrm`` and its Y are not written.

    ``rx``      the new rows' regularizer (one, or one per row); default: the fitted model's, when all its rows carry the same one.
    ``X0``      the start; default ``rng.standard_normal((k, m_new))``, the constructor's default in the reference.
    ``params``  a HipProxGradParams (``storage="f32"`` is honoured; ``ngpus > 1`` raises): stepsize, max_iter, inner_iter_X, abs_tol,
                rel_tol and min_stepsize mean what they mean to ``fit!``; inner_iter_Y is not used.
    ``api``     a test hook (an ``_capi.Api``); the product default is the HIP library.
    ``exact``   True: the fitted model is quadratic (QuadLoss columns; the new rows carry a QuadReg or ZeroReg) and the embedding is ONE
                glrm_hip_als_solve(h, 0) on the new rows' handle (include/glrm_hip_als.h): every row lands on the exact minimiser, no
                step size, no iteration.  ``params`` may then also be an AlsParams; only its device_id is used.  ``ch`` holds the full
                objective at the start and at the end; ``X0`` only matters for the rows the solve keeps (fewer than k observations under
                ZeroReg, or a rank-deficient system).  A model the engine would refuse is refused before a handle exists.

    ``ch.objective[0]`` is the full objective at the start, as ``fit_b`` records it; every later entry is the column losses plus the
    column penalties after the iteration, which is what ``fit!`` records (proxgrad.jl:205).  The stopping rule is proxgrad.jl:210-213 with
    ``abs_tol`` scaled by the new rows' observation count."""
    params = HipProxGradParams() if params is None else params
    if exact and isinstance(params, AlsParams):
        params = HipProxGradParams(device_id=params.device_id)
    if not isinstance(params, HipProxGradParams):
        raise TypeError("params must be a HipProxGradParams")
    if getattr(params, "ngpus", 1) > 1:
        raise ValueError("transform runs on one device (ngpus must be 1): rows are embedded independently, shard A_new instead")
    if rx is not None and not isinstance(rx, Regularizer):
        rx = list(rx)
    rx = _row_regularizer(glrm, rx)
    api = api if api is not None else _capi.hip_api()
    if np.linalg.norm(glrm.Y) == 0:
        raise ValueError("Y is all zeros: the model has not been fitted")
    new = GLRM(A_new, [_copy.copy(l) for l in glrm.losses], rx, [_copy.copy(r) for r in glrm.ry], glrm.k, obs=obs, X=X0, Y=glrm.Y, rng=rng)
    if exact:
        return _transform_exact(new, params, api)
    ch = ConvergenceHistory("ProxGradGLRM-transform")
    try:
        h = _ensure_handle(new, api, params, allow_dense=False)[0]
        X = np.asfortranarray(new.X, dtype=np.float64)
        Y = np.asfortranarray(new.Y, dtype=np.float64)
        keep, p_col, p_row = _objective_buffers(api, params, new.n, new.m)
        api.bind_buffers(h, None, None, p_col, p_row)
        api.set_factors(h, X, Y)
        api.reset_stepsizes(h, params.stepsize)                     # proxgrad.jl:69-70
        scaled_abs_tol = params.abs_tol * float(new._rowptr[-1])    # :72, the new rows' observations

        def col_sum(fill):
            fill(h)
            return api.sum(h, p_col, new.n)
        loss = col_sum(api.col_losses)
        api.row_penalties(h)
        px = api.sum(h, p_row, new.m)
        py = col_sum(api.col_penalties)
        update_ch(ch, 0, loss + (px + py))                          # update_ch!(ch, 0, objective(...)) :76
        fused = api.has_transform
        t = time.time()
        for i in range(1, params.max_iter + 1):                     # :107
            if params.inner_iter_X > 1:
                api.reset_stepsizes(h, params.stepsize)             # :112-115
            if fused:
                api.solve_x(h, params.inner_iter_X, params.min_stepsize)   # :117-158, one call
            else:
                for _ in range(params.inner_iter_X):
                    api.step_x(h, params.min_stepsize)
            obj = col_sum(api.col_losses) + col_sum(api.col_penalties)     # obj = sum(obj_by_col) :205
            update_ch(ch, time.time() - t, obj)
            t = time.time()
            if _should_stop(i, ch.objective[-2], obj, scaled_abs_tol, params.rel_tol):   # :210-213
                break
        api.get_factors(h, X, Y)
    finally:
        new.close()                                                 # (the handle goes before the buffers it was bound to)
    return X, ch


def _transform_exact(new, params, api):
    """``transform(exact=True)``: one exact X half-step of the new rows' model -> (X_new, ch); closes ``new``'s handle."""
    from .als import _Objective, check_model
    ch = ConvergenceHistory("AlsGLRM-transform")
    try:
        check_model(new, sides=(0,))
        h = _ensure_handle(new, api, params, allow_dense=False)[0]
        X = np.asfortranarray(new.X, dtype=np.float64)
        Y = np.asfortranarray(new.Y, dtype=np.float64)
        full = _Objective(api, h, params.device_id, new.m, new.n)
        try:
            api.set_factors(h, X, Y)
            update_ch(ch, 0, full())
            t = time.time()
            api.als_solve(h, 0)
            update_ch(ch, time.time() - t, full())
            api.get_factors(h, X, Y)
        finally:
            full.close()
    finally:
        new.close()
    return X, ch


def inverse_transform(glrm, X_new):
    """``X_new' * glrm.Y`` (src/scikitlearn.jl:107): the model's reconstruction of the embedded rows, on the host."""
    return np.asarray(X_new, dtype=np.float64).T @ glrm.Y
