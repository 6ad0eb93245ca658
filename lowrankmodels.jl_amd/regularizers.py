"""Regularizers named by the north star (reference: src/regularizers.jl), host descriptors.

``evaluate``/``prox`` restate the reference's array methods for API parity; inside the fit the
prox step runs fused in the HIP sweep kernels.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from ._capi import REG_DTYPE, bump_epoch as _bump_epoch

ZERO, QUAD, ONE, NONNEG, UNIT_ONE_SPARSE = range(5)
QUAD_CONSTRAINT, NONNEG_ONE, ONE_SPARSE, K_SPARSE, SIMPLEX = range(5, 10)  # the vector regularizers (GLRM_REG_KIND_END = 10)
TOL = 1e-12  # src/regularizers.jl:25


class Regularizer:
    kind = -1

    def __setattr__(self, name, value):  # any change of a descriptor field invalidates cached packed descriptors
        object.__setattr__(self, name, value)
        _bump_epoch()

    def __init__(self, scale=1.0):
        self.scale = float(scale)

    def mul_(self, newscale):  # mul!(r, newscale), src/regularizers.jl:38
        self.scale = float(newscale)
        return self

    def __rmul__(self, newscale):  # *(newscale, r): scale(r)*newscale on a fresh copy, :40
        r = _copy.copy(self)
        r.mul_(self.scale * newscale)
        return r

    wrap = 0

    def descriptor(self):
        return (self.kind, self.wrap, self.scale)

    def __repr__(self):
        return f"{type(self).__name__}({self.scale})"


class QuadReg(Regularizer):  # :52-58
    kind = QUAD

    def __init__(self, scale=1):
        super().__init__(scale)

    def evaluate(self, a):
        return self.scale * float(np.sum(np.abs(np.asarray(a, dtype=float)) ** 2))

    def prox(self, u, alpha):
        return 1 / (1 + 2 * alpha * self.scale) * np.asarray(u, dtype=float)


class OneReg(Regularizer):  # :79-88
    kind = ONE

    def __init__(self, scale=1):
        super().__init__(scale)

    def evaluate(self, a):
        return self.scale * float(np.sum(np.abs(a)))

    def prox(self, u, alpha):
        u = np.asarray(u, dtype=float)
        t = self.scale * alpha
        return np.maximum(u - t, 0) + np.minimum(u + t, 0)


class _Unscaled(Regularizer):
    def __init__(self):
        super().__init__(1.0)

    def mul_(self, newscale):  # mul!(r::ZeroReg/NonNeg/UnitOneSparse, _) is a no-op (:97,:114,:318)
        return self

    def descriptor(self):
        return (self.kind, 0, 1.0)

    def __repr__(self):
        return f"{type(self).__name__}()"


class ZeroReg(_Unscaled):  # :91-97
    kind = ZERO

    def evaluate(self, a):
        return 0

    def prox(self, u, alpha):
        return np.asarray(u, dtype=float)


class NonNegConstraint(_Unscaled):  # :101-114
    kind = NONNEG

    def evaluate(self, a):
        return float("inf") if np.any(np.asarray(a) < 0) else 0

    def prox(self, u, alpha=1):
        return np.maximum(np.asarray(u, dtype=float), 0)


class UnitOneSparseConstraint(_Unscaled):  # :295-318
    kind = UNIT_ONE_SPARSE

    def evaluate(self, a):
        oneflag = False
        for ai in np.asarray(a).ravel():
            if ai == 0:
                continue
            if ai == 1:
                if oneflag:
                    return float("inf")
                oneflag = True
            else:
                return float("inf")
        return 0

    def prox(self, u, alpha=0):
        u = np.asarray(u, dtype=float)
        v = np.zeros_like(u)
        v[int(np.argmax(u))] = 1
        return v


# ------------------------------------------------------------------------- vector regularizers (kinds 5-9)
# They act on a k-vector: every rx, the ry of a scalar-loss column, and the base of lastentry1 / lastentry_unpenalized.  The engine refuses
# them on the k x d block of a multi-dimensional column and under OrdinalReg / MNLOrdinalReg (the reference's sort / partialsortperm throw
# on a matrix).  For all five `mul!` is a no-op and scale() is 1 (src/regularizers.jl:75-76,137-138,254-255,347-348; KSparseConstraint has
# no `scale` field at all), and `newscale * r` builds `typeof(r)()` (:40), i.e. an object with the DEFAULT parameter.


class _VectorReg(Regularizer):
    def mul_(self, newscale):  # mul!(r, newscale) = 1: nothing changes
        return self

    def __rmul__(self, newscale):  # *(newscale, r) = typeof(r)() followed by the no-op mul! (:40)
        return type(self)()


class QuadConstraint(_VectorReg):  # :68-76
    """Indicator of the ball ||x|| <= max_2norm (max-norm regularization).  ``prox`` rescales ONTO the sphere, always -- also from inside the
    ball -- and turns the zero vector into NaN (:72); ``mul_`` is a no-op (:76) and ``newscale * r`` is ``QuadConstraint()``, which
    resets max_2norm to 1 (:40,:71)."""
    kind = QUAD_CONSTRAINT

    def __init__(self, max_2norm=1):
        object.__setattr__(self, "max_2norm", float(max_2norm))
        _bump_epoch()

    scale = property(lambda self: 1.0)  # scale(r::QuadConstraint) = 1, :75

    def descriptor(self):
        return (self.kind, 0, self.max_2norm)

    def evaluate(self, u):
        u = np.asarray(u, dtype=float).ravel()
        return float("inf") if np.sqrt(np.sum(u * u)) > self.max_2norm + TOL else 0

    def prox(self, u, alpha=0):
        u = np.asarray(u, dtype=float)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (self.max_2norm / np.sqrt(np.sum(u * u))) * u

    def __repr__(self):
        return f"QuadConstraint({self.max_2norm})"


class NonNegOneReg(_VectorReg):  # :118-138
    """scale * sum(a) on the nonnegative orthant (sparse NNMF).  ``prox`` is max(u - alpha, 0): the reference leaves ``scale`` out of it
    (:122); ``mul_`` is a no-op (:138) and ``newscale * r`` is ``NonNegOneReg()``, which resets the parameter to 1 (:40,:121)."""
    kind = NONNEG_ONE

    def __init__(self, scale=1):
        object.__setattr__(self, "param", float(scale))
        _bump_epoch()

    scale = property(lambda self: 1.0)  # scale(r::NonNegOneReg) = 1 (:137); the struct field is `param` here

    def descriptor(self):
        return (self.kind, 0, self.param)

    def evaluate(self, a):
        a = np.asarray(a, dtype=float).ravel()
        return float("inf") if np.any(a < 0) else self.param * float(np.sum(a))

    def prox(self, u, alpha):
        return np.maximum(np.asarray(u, dtype=float) - alpha, 0)

    def __repr__(self):
        return f"NonNegOneReg({self.param})"


class OneSparseConstraint(_VectorReg):  # :235-255
    """Indicator of vectors with at most one nonzero entry (orthogonal NNMF).  ``prox`` keeps the first LARGEST SIGNED entry (argmax u, not
    argmax |u|, :237); ``mul_`` is a no-op (:255) and ``newscale * r`` is a fresh ``OneSparseConstraint()`` (:40)."""
    kind = ONE_SPARSE

    def __init__(self):
        pass

    scale = property(lambda self: 1.0)

    def descriptor(self):
        return (self.kind, 0, 1.0)

    def evaluate(self, a):
        return float("inf") if np.count_nonzero(np.asarray(a, dtype=float)) > 1 else 0

    def prox(self, u, alpha=0):
        u = np.asarray(u, dtype=float)
        v = np.zeros_like(u)
        i = int(np.argmax(u))
        v.flat[i] = u.flat[i]
        return v

    def __repr__(self):
        return "OneSparseConstraint()"


class KSparseConstraint(_VectorReg):  # :258-291
    """Indicator of vectors with at most r nonzero entries.  ``prox`` keeps the r entries of largest |u|; among equal |u| the lower index
    stays (the reference's partialsortperm leaves ties open).  The reference defines neither ``scale`` nor ``mul!`` nor a zero-argument
    constructor for it: ``mul_`` is a no-op here and ``newscale * r`` raises, like ``typeof(r)()`` does (:40)."""
    kind = K_SPARSE

    def __init__(self, k):
        if int(k) != k:
            raise TypeError("KSparseConstraint(k): k::Int")
        object.__setattr__(self, "k", int(k))
        _bump_epoch()

    scale = property(lambda self: 1.0)

    def __rmul__(self, newscale):
        raise TypeError("no method matching KSparseConstraint() (src/regularizers.jl:40)")

    def descriptor(self):
        return (self.kind, 0, float(self.k))

    def evaluate(self, a):
        return float("inf") if np.count_nonzero(np.asarray(a, dtype=float)) > self.k else 0

    def prox(self, u, alpha=0):
        u = np.asarray(u, dtype=float)
        ids = np.argsort(-np.abs(u.ravel()), kind="stable")[: self.k]
        if len(ids) < self.k:
            raise IndexError("KSparseConstraint: k exceeds the length of the vector (BoundsError)")
        v = np.zeros_like(u)
        v.flat[ids] = u.flat[ids]
        return v

    def __repr__(self):
        return f"KSparseConstraint({self.k})"


class SimplexConstraint(_VectorReg):  # :323-348
    """Indicator of the probability simplex (soft k-means).  ``prox`` is Chen & Ye's projection exactly as the reference computes it: sort
    descending, SEQUENTIAL cumulative sum, first index whose running threshold reaches the next entry (:325-337); ``mul_`` is a no-op
    (:348) and ``newscale * r`` is a fresh ``SimplexConstraint()`` (:40)."""
    kind = SIMPLEX

    def __init__(self):
        pass

    scale = property(lambda self: 1.0)

    def descriptor(self):
        return (self.kind, 0, 1.0)

    def evaluate(self, a):
        a = np.asarray(a, dtype=float).ravel()
        if abs(float(np.sum(a)) - 1) > TOL:
            return float("inf")
        return float("inf") if np.any(a < 0) else 0

    def prox(self, u, alpha=0):
        u = np.asarray(u, dtype=float)
        y = np.sort(u.ravel())[::-1]
        n = len(y)
        ysum = 0.0
        t = None
        for i in range(n):  # ysum = y[0] + ... + y[i-1], one term per step
            if i >= 1 and (ysum - 1) / i >= y[i]:
                t = (ysum - 1) / i
                break
            ysum += float(y[i])
        if t is None:
            t = (ysum - 1) / n
        return np.maximum(u - t, 0)

    def __repr__(self):
        return "SimplexConstraint()"


# ------------------------------------------------------------------------- wrappers / block regularizers
WRAP_LASTENTRY1, WRAP_LASTENTRY_UNPENALIZED, WRAP_ORDINAL, WRAP_MNL_ORDINAL = 1, 2, 4, 8


class _Wrapper(Regularizer):
    """A regularizer around a base regularizer r (one of the kinds above).  Arrays are k-vectors or k x d blocks
    (first axis = latent component), like the views the reference passes."""
    wrap = 0

    def __init__(self, r=None):
        r = ZeroReg() if r is None else r
        if isinstance(r, _Wrapper) or r.kind < 0:
            raise NotImplementedError("nested wrappers are outside the accelerated path")
        self.r = r

    kind = property(lambda self: self.r.kind)
    scale = property(lambda self: self.r.scale)

    def mul_(self, newscale):
        self.r.mul_(newscale)
        return self

    def descriptor(self):
        return (self.r.kind, self.wrap, self.r.descriptor()[2])

    def __repr__(self):
        return f"{type(self).__name__}({self.r!r})"


class lastentry1(_Wrapper):  # src/regularizers.jl:163-175
    wrap = WRAP_LASTENTRY1

    def evaluate(self, a):
        a = np.asarray(a, dtype=float)
        return self.r.evaluate(a[:-1]) if np.all(a[-1] == 1) else float("inf")

    def prox(self, u, alpha=1):
        u = np.array(u, dtype=float)
        u[:-1] = self.r.prox(u[:-1], alpha)
        u[-1] = 1
        return u


class lastentry_unpenalized(_Wrapper):  # src/regularizers.jl:177-189
    wrap = WRAP_LASTENTRY_UNPENALIZED

    def __new__(cls, r=None):
        if isinstance(r, (OrdinalReg, MNLOrdinalReg)):  # "make sure we don't add two offsets", :386,:411
            return r
        return super().__new__(cls)

    def evaluate(self, a):
        return self.r.evaluate(np.asarray(a, dtype=float)[:-1])

    def prox(self, u, alpha=1):
        u = np.array(u, dtype=float)
        u[:-1] = self.r.prox(u[:-1], alpha)
        return u


class OrdinalReg(_Wrapper):  # src/regularizers.jl:356-386
    wrap = WRAP_ORDINAL

    def evaluate(self, a):
        a = np.asarray(a, dtype=float).reshape(len(a), -1)
        return self.r.evaluate(a[:-1, 0])

    def prox(self, u, alpha):
        u = np.array(u, dtype=float)
        u2 = u.reshape(len(u), -1)
        um = np.asarray(self.r.prox(np.mean(u2[:-1, :], axis=1), alpha), dtype=float)
        u2[:-1, :] = um[:, None]
        return u


class MNLOrdinalReg(OrdinalReg):  # src/regularizers.jl:388-411
    wrap = WRAP_MNL_ORDINAL

    def prox(self, u, alpha, TOL=1e-3):
        u = OrdinalReg.prox(self, u, alpha)
        u2 = u.reshape(len(u), -1)
        u2[-1, 0] = min(-TOL, u2[-1, 0])
        for j in range(1, u2.shape[1]):
            u2[-1, j] = min(u2[-1, j], u2[-1, j - 1] - TOL)
        return u


def prox(r, u, alpha):
    return r.prox(u, alpha)


def pack_regs(regs):
    descs = [r.descriptor() for r in regs]
    if len(set(descs)) == 1:
        descs = descs[:1]
    return np.array(descs, dtype=REG_DTYPE)
