"""Alternating cyclic coordinate descent for QuadLoss models with ZeroReg / QuadReg / OneReg / NonNegConstraint regularizers: the driver
behind ``fit_b(glrm, CdParams())``.

An iteration is glrm_hip_cd_solve(h, 0, sweeps) then glrm_hip_cd_solve(h, 1, sweeps) (include/glrm_hip_cd.h, which is the specification
of the arithmetic): every coordinate of every row of X, then of every column of Y, is set to the exact minimiser of the segment's part of
the objective with everything else held.  The history records the FULL objective -- column losses + row penalties + column penalties --
after every iteration, as the ALS driver does (als.py): a coordinate update cannot raise it.  A NonNegConstraint start with a negative
entry has an infinite first entry; the solve projects the point first, so the second entry is finite.

A model the engine would refuse is refused here, before a handle exists, with the engine's words.
"""
from __future__ import annotations

import time

import numpy as np

from . import _capi
from .als import _Objective
from .convergence import update_ch
from .losses import pack_losses
from .regularizers import _carrier, _collapse

HEADER = "include/glrm_hip_cd.h"
_WHAT = "glrm_hip_cd_solve"
QUAD_LOSS = 0                                       # include/glrm_hip.h: GLRM_LOSS_QUAD
REG_ZERO, REG_QUAD, REG_ONE, REG_NONNEG = 0, 1, 2, 3  # GLRM_REG_ZERO, GLRM_REG_QUAD, GLRM_REG_ONE, GLRM_REG_NONNEG
KINDS = (REG_ZERO, REG_QUAD, REG_ONE, REG_NONNEG)


def check_model(glrm, sides=(0, 1)):
    """Raise GLRMError(ERR_UNSUPPORTED) for a model glrm_hip_cd_solve refuses on one of ``sides`` (0: rows, 1: columns) -- the messages of
    csrc/glrm_cd.hip, in its order."""
    def refuse(msg):
        raise _capi.GLRMError(_capi.ERR_UNSUPPORTED, f"{_WHAT}{msg} ({HEADER})")
    if glrm.k > _capi.CD_MAX_K:
        refuse(f": rank k = {glrm.k} is above GLRM_CD_MAX_K = {_capi.CD_MAX_K}")
    for j, l in enumerate(pack_losses(glrm.losses)):
        if int(l["kind"]) != QUAD_LOSS:
            refuse(f": column {j} has loss kind {int(l['kind'])}; the coordinate update needs QuadLoss (kind {QUAD_LOSS}) on every column")
    descs = {0: _collapse(glrm.rx)[1], 1: _collapse(glrm.ry)[1]}
    for side in sides:
        name = "rx" if side == 0 else "ry"
        for s, (kind, wrap, scale) in enumerate(descs[side]):
            if kind not in KINDS or wrap != 0:
                refuse(f": {name}[{s}] has regularizer kind {kind}, wrap {wrap}; the solved side needs a plain ZeroReg (kind {REG_ZERO}), "
                       f"QuadReg (kind {REG_QUAD}), OneReg (kind {REG_ONE}) or NonNegConstraint (kind {REG_NONNEG})")
            if kind in (REG_QUAD, REG_ONE) and not scale >= 0.0:
                refuse(f": {name}[{s}] is {'QuadReg' if kind == REG_QUAD else 'OneReg'} with scale {scale:g}; the coordinate update needs a "
                       "scale >= 0")
    if any(d[1] != 0 or _carrier(d) for side in (0, 1) for d in descs[side]) or glrm.d != glrm.n:
        refuse(": the model runs on the general sweeps (multi-dimensional losses, wrapped or vector regularizers); coordinate descent does not")


def check_sweeps(sweeps):
    if not 1 <= sweeps <= _capi.CD_MAX_SWEEPS:
        raise _capi.GLRMError(_capi.ERR_INVALID, f"{_WHAT}: sweeps must be in [1, GLRM_CD_MAX_SWEEPS = {_capi.CD_MAX_SWEEPS}], got {sweeps}")


def fit_cd(glrm, params, ch, verbose, api):
    """``fit_b`` for CdParams on one device -> (glrm.X, glrm.Y, ch); ``glrm._cd_info`` keeps the last solve's counts per side."""
    from .fit import _ensure_handle, _should_stop
    check_model(glrm)
    check_sweeps(params.sweeps)
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
            api.cd_solve(h, 0, params.sweeps)
            api.cd_solve(h, 1, params.sweeps)
            obj = full()
            update_ch(ch, time.time() - t, obj)
            t = time.time()
            if _should_stop(i, ch.objective[-2], obj, scaled_abs_tol, params.rel_tol):   # :210-213
                break
            if verbose and i % 10 == 0:
                print(f"Iteration {i}: objective value = {obj}")
        if len(ch.objective) > 1:
            glrm._cd_info = {0: api.cd_info(h, 0), 1: api.cd_info(h, 1)}
        api.get_factors(h, X, Y)
    finally:
        full.close()
    glrm.X[...] = X
    glrm.Y[...] = Y
    return glrm.X, glrm.Y, ch
