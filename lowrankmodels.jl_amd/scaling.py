"""equilibrate_variance! / prob_scale! (reference: src/modify_glrm.jl:31-82) on the engine: the per-column M-estimates, average
losses and variances are one device pass over the column view (``glrm_hip_scale_columns``, include/glrm_hip_scale.h); the host only
applies the returned scales with ``mul_`` -- which SETS the scale, like the reference's mul!."""
from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import ProblemArrays
from .losses import pack_losses
from .regularizers import pack_regs


def column_view(glrm) -> ProblemArrays:
    """The part of the model the scaling pass reads: the column view and the loss / Y-regularizer descriptors (no row view)."""
    return ProblemArrays(glrm.m, glrm.n, glrm.k, None, None, None, np.ascontiguousarray(glrm._colptr), None,
                         np.ascontiguousarray(glrm._colvals), pack_losses(glrm.losses), pack_regs(glrm.rx[:1]), pack_regs(glrm.ry))


def _rescale(glrm, mode, columns_to_scale, engine):
    if glrm.d != glrm.n:
        raise NotImplementedError("scale=true with multi-dimensional losses: their M-estimators do not run in the reference either")
    api = engine if engine is not None else _capi.hip_api()
    loss_scale, ry_scale = api.scale_columns(column_view(glrm), mode)
    for i in (range(glrm.n) if columns_to_scale is None else columns_to_scale):
        glrm.losses[i].mul_(loss_scale[i])
        if mode == _capi.SCALE_EQUILIBRATE:
            glrm.ry[i].mul_(ry_scale[i])
    glrm.close()  # the descriptors of a cached engine handle are stale now
    return glrm


def equilibrate_variance_(glrm, columns_to_scale=None, engine=None):
    """equilibrate_variance!(glrm, columns_to_scale): every column's loss is divided by its average loss at the column's M-estimate
    and its Y regularizer by the variance of its observed values (src/modify_glrm.jl:34-53)."""
    return _rescale(glrm, _capi.SCALE_EQUILIBRATE, columns_to_scale, engine)


def prob_scale_(glrm, columns_to_scale=None, engine=None):
    """prob_scale!(glrm, columns_to_scale): Quad / Huber columns get the scale of the -log-likelihood at the estimated width, every
    other loss scale 1 (src/modify_glrm.jl:60-82).  The statistics run over the observed entries of each column."""
    return _rescale(glrm, _capi.SCALE_PROB, columns_to_scale, engine)
