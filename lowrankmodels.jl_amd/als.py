"""Exact alternating least squares for quadratic models: the driver behind ``fit_b(glrm, AlsParams())`` and ``transform(..., exact=True)``.

An iteration is glrm_hip_als_solve(h, 0) then glrm_hip_als_solve(h, 1) (include/glrm_hip_als.h, which is the specification of the
arithmetic): every row of X, then every column of Y, lands on the exact minimiser of its part of the objective.  The history records the
FULL objective -- column losses + row penalties + column penalties, through the entry points ``fit_b`` uses for its first entry -- after
every iteration: an exact half-step cannot raise it, and the history shows that (proxgrad's later entries leave the row penalties out).

A model the engine would refuse is refused here, before a handle exists, with the engine's words.
"""
from __future__ import annotations

import time

import numpy as np

from . import _capi
from .convergence import update_ch
from .losses import pack_losses
from .regularizers import _carrier, _collapse

HEADER = "include/glrm_hip_als.h"
_WHAT = "glrm_hip_als_solve"
QUAD_LOSS, REG_ZERO, REG_QUAD = 0, 0, 1     # include/glrm_hip.h: GLRM_LOSS_QUAD, GLRM_REG_ZERO, GLRM_REG_QUAD


def check_model(glrm, sides=(0, 1)):
    """Raise GLRMError(ERR_UNSUPPORTED) for a model glrm_hip_als_solve refuses on one of ``sides`` (0: rows, 1: columns) -- the messages
    of csrc/glrm_als.hip, in its order."""
    def refuse(msg):
        raise _capi.GLRMError(_capi.ERR_UNSUPPORTED, f"{_WHAT}{msg} ({HEADER})")
    if glrm.k > _capi.ALS_MAX_K:
        refuse(f": rank k = {glrm.k} is above GLRM_ALS_MAX_K = {_capi.ALS_MAX_K}")
    for j, l in enumerate(pack_losses(glrm.losses)):
        if int(l["kind"]) != QUAD_LOSS:
            refuse(f": column {j} has loss kind {int(l['kind'])}; the closed-form solve needs QuadLoss (kind {QUAD_LOSS}) on every column")
    descs = {0: _collapse(glrm.rx)[1], 1: _collapse(glrm.ry)[1]}
    for side in sides:
        name = "rx" if side == 0 else "ry"
        for s, (kind, wrap, scale) in enumerate(descs[side]):
            if kind not in (REG_QUAD, REG_ZERO) or wrap != 0:
                refuse(f": {name}[{s}] has regularizer kind {kind}, wrap {wrap}; the solved side needs a plain QuadReg (kind {REG_QUAD}) or "
                       f"ZeroReg (kind {REG_ZERO})")
            if kind == REG_QUAD and not scale >= 0.0:
                refuse(f": {name}[{s}] is QuadReg with scale {scale:g}; the system needs a scale >= 0")
    if any(d[1] != 0 or _carrier(d) for side in (0, 1) for d in descs[side]) or glrm.d != glrm.n:
        refuse(": the model runs on the general sweeps (multi-dimensional losses, wrapped or vector regularizers); the closed-form solve does not")


class _Objective:
    """The full objective of the handle's resident factors through col_losses / row_penalties / col_penalties / sum, in buffers bound to the
    handle for the life of this object (``close`` hands the handle its own again: the buffers die with this object)."""

    def __init__(self, api, h, device_id, m, n):
        from .transform import _objective_buffers

        class _P:
            pass
        p = _P()
        p.device_id = device_id
        self.api, self.h, self.m, self.n = api, h, m, n
        self.keep, self.p_col, self.p_row = _objective_buffers(api, p, n, m)
        api.bind_buffers(h, None, None, self.p_col, self.p_row)

    def __call__(self):
        api, h = self.api, self.h
        api.col_losses(h)
        loss = api.sum(h, self.p_col, self.n)
        api.row_penalties(h)
        px = api.sum(h, self.p_row, self.m)
        api.col_penalties(h)
        py = api.sum(h, self.p_col, self.n)
        return loss + (px + py)                                     # err += calc_penalty(...), src/evaluate_fit.jl:19-21

    def close(self):
        self.api.synchronize(self.h)
        self.api.bind_buffers(self.h, None, None, None, None)
        self.keep = None


def fit_als(glrm, params, ch, verbose, api):
    """``fit_b`` for AlsParams on one device -> (glrm.X, glrm.Y, ch); ``glrm._als_info`` keeps the last solve's counts per side."""
    from .fit import _ensure_handle, _should_stop
    check_model(glrm)
    h = _ensure_handle(glrm, api, params, allow_dense=False)[0]
    X = np.asfortranarray(glrm.X, dtype=np.float64)
    Y = np.asfortranarray(glrm.Y, dtype=np.float64)
    if verbose:
        print("Fitting GLRM")
    full = _Objective(api, h, params.device_id, glrm.m, glrm.n)
    try:
        api.set_factors(h, X, Y)
        scaled_abs_tol = params.abs_tol * float(glrm._rowptr[-1])   # proxgrad.jl:72
        update_ch(ch, 0, full())                                    # update_ch!(ch, 0, objective(...)) :76
        t = time.time()
        for i in range(1, params.max_iter + 1):
            api.als_solve(h, 0)
            api.als_solve(h, 1)
            obj = full()
            update_ch(ch, time.time() - t, obj)
            t = time.time()
            if _should_stop(i, ch.objective[-2], obj, scaled_abs_tol, params.rel_tol):   # :210-213
                break
            if verbose and i % 10 == 0:
                print(f"Iteration {i}: objective value = {obj}")
        if len(ch.objective) > 1:
            glrm._als_info = {0: api.als_info(h, 0), 1: api.als_info(h, 1)}
        api.get_factors(h, X, Y)
    finally:
        full.close()
    glrm.X[...] = X
    glrm.Y[...] = Y
    return glrm.X, glrm.Y, ch
