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
        if r.kind == REM_QUAD:
            raise NotImplementedError("RemQuadReg under a wrapper is outside the accelerated path")
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


# ------------------------------------------------------------------------- regularizers that carry a vector (include/glrm_hip_regvec.h)
# fixed_latent_features / fixed_last_latent_features (src/regularizers.jl:193-231) and RemQuadReg (:412-423), on k-vectors.  Their vector
# travels beside the 16-byte descriptor through glrm_hip_set_regularizers_vec; ``descriptor()`` holds the codes only that entry point takes.
REM_QUAD = 10
WRAP_FIXED_FIRST, WRAP_FIXED_LAST = 16, 32


def _frozen_vector(y):
    """A private read-only float64 copy: the contents change only by assigning a new array, which ``__setattr__`` sees (``_bump_epoch``)."""
    v = np.array(y, dtype=np.float64).reshape(-1)
    v.setflags(write=False)
    return v


class _FixedFeatures(_Wrapper):
    """Common part of the two fixed-features wrappers: base r, pinned values y (n = len(y)).  ``mul_`` and ``scale`` forward to the base
    (:209-210,230-231)."""

    def __init__(self, r, y):
        super().__init__(r)  # nesting with the other wrappers, or RemQuadReg as the base, raises NotImplementedError there
        self.y = y

    def __rmul__(self, newscale):  # typeof(r)() has no method (:40)
        raise TypeError(f"no method matching {type(self).__name__}() (src/regularizers.jl:40)")

    def __setattr__(self, name, value):
        if name == "y":
            value = _frozen_vector(value)
        Regularizer.__setattr__(self, name, value)

    n = property(lambda self: len(self.y))

    def vector(self):
        return self.y

    def _base_prox(self, sub, alpha):
        """prox(r.r, sub, alpha).  With n = k the base sees an EMPTY vector: in the reference every base then returns the empty vector,
        except the argmax / partialsortperm kinds, which throw (they are left to raise here; the engine refuses them)."""
        if len(sub) == 0 and self.r.kind not in (UNIT_ONE_SPARSE, ONE_SPARSE, K_SPARSE):
            return sub
        return np.asarray(self.r.prox(sub, alpha), dtype=float)

    def __repr__(self):
        return f"{type(self).__name__}({self.r!r}, {self.y.tolist()})"


class fixed_latent_features(_FixedFeatures):  # src/regularizers.jl:193-210
    """The first n entries are fixed to y, the other k - n are regularized by r."""
    wrap = WRAP_FIXED_FIRST

    def prox(self, u, alpha):  # [r.y; prox(r.r, u[(r.n+1):end], alpha)], :202
        u = np.asarray(u, dtype=float)
        return np.concatenate([self.y, self._base_prox(u[self.n:], alpha)])

    def evaluate(self, a):  # a[1:r.n] == r.y ? evaluate(r.r, a[(r.n+1):end]) : Inf, :208
        a = np.asarray(a, dtype=float)
        return self.r.evaluate(a[self.n:]) if np.array_equal(a[:self.n], self.y) else float("inf")


class fixed_last_latent_features(_FixedFeatures):  # src/regularizers.jl:214-231
    """The last n entries are fixed to y.  ``prox`` is the reference's, literally (:223): the base is fed ``u[n:]`` -- the LAST k - n entries of
    u -- and its result becomes the FIRST k - n entries.  Reproduced, not repaired."""
    wrap = WRAP_FIXED_LAST

    def prox(self, u, alpha):  # [prox(r.r, u[(r.n+1):end], alpha); r.y], :223
        u = np.asarray(u, dtype=float)
        return np.concatenate([self._base_prox(u[self.n:], alpha), self.y])

    def evaluate(self, a):  # a[length(a)-r.n+1:end] == r.y ? evaluate(r.r, a[1:length(a)-r.n]) : Inf, :229
        a = np.asarray(a, dtype=float)
        cut = len(a) - self.n
        return self.r.evaluate(a[:cut]) if np.array_equal(a[cut:], self.y) else float("inf")


def FixedLatentFeaturesConstraint(y):  # :200
    return fixed_latent_features(ZeroReg(), y)


def FixedLastLatentFeaturesConstraint(y):  # :221
    return fixed_last_latent_features(ZeroReg(), y)


class RemQuadReg(Regularizer):  # src/regularizers.jl:412-423
    """Quadratic regularization with a non-zero mean: ``RemQuadReg(m)`` or ``RemQuadReg(scale, m)`` (:416).  ``mul_`` sets ``scale`` (the
    generic mul!, :38); ``newscale * r`` raises, like ``typeof(r)()`` does (:40)."""
    kind = REM_QUAD

    def __init__(self, *args):
        if len(args) == 1:
            scale, m = 1, args[0]
        elif len(args) == 2:
            scale, m = args
        else:
            raise TypeError("RemQuadReg(m) or RemQuadReg(scale, m)")
        super().__init__(scale)
        self.m = m

    def __setattr__(self, name, value):
        if name == "m":
            value = _frozen_vector(value)
        Regularizer.__setattr__(self, name, value)

    def __rmul__(self, newscale):
        raise TypeError("no method matching RemQuadReg() (src/regularizers.jl:40)")

    def vector(self):
        return self.m

    def prox(self, u, alpha):  # (u + 2 * alpha * r.scale * r.m) / (1 + 2 * alpha * r.scale), :417-418
        u = np.asarray(u, dtype=float)
        t = 2 * alpha * self.scale
        return (u + t * self.m) / (1 + t)

    def evaluate(self, a):  # r.scale * sum(abs2, a - r.m), :423
        return self.scale * float(np.sum((np.asarray(a, dtype=float) - self.m) ** 2))

    def __repr__(self):
        return f"RemQuadReg({self.scale}, {self.m.tolist()})"


def prox(r, u, alpha):
    return r.prox(u, alpha)


_FIXED = WRAP_FIXED_FIRST | WRAP_FIXED_LAST


def _carrier(desc):
    return desc[0] == REM_QUAD or (desc[1] & _FIXED) != 0


def _collapse(regs):
    """(regularizers, descriptors) as they go over: ONE when every entry is the same regularizer (descriptor and vector alike), else one
    per entry."""
    regs = list(regs)
    descs = [r.descriptor() for r in regs]
    if len(set(descs)) == 1 and (not _carrier(descs[0]) or len({r.vector().tobytes() for r in regs}) == 1):
        return regs[:1], descs[:1]
    return regs, descs


def pack_regs(regs):
    """The descriptors glrm_hip_create / glrm_hip_set_regularizers take.  A regularizer that carries a vector appears as its PLACEHOLDER (the
    base kind without the fixed-features flag; ZeroReg for RemQuadReg) with the count ``pack_reg_vectors`` uses: creation goes through the
    placeholders and is followed by glrm_hip_set_regularizers_vec."""
    descs = _collapse(regs)[1]
    if any(_carrier(d) for d in descs):
        descs = [(ZERO, 0, 1.0) if d[0] == REM_QUAD else (d[0], d[1] & ~_FIXED, d[2]) for d in descs]
    return np.array(descs, dtype=REG_DTYPE)


def pack_reg_vectors(regs, k):
    """None when no regularizer of ``regs`` carries a vector; else (descriptors with the codes of include/glrm_hip_regvec.h, the k x count
    column-major table of their vectors as a flat array, the int32 lengths) -- one side's arguments of glrm_hip_set_regularizers_vec."""
    regs, descs = _collapse(regs)
    if not any(_carrier(d) for d in descs):
        return None
    k = int(k)
    table = np.zeros((len(regs), k))
    lens = np.zeros(len(regs), dtype=np.int32)
    for i, r in enumerate(regs):
        if _carrier(descs[i]):
            v = r.vector()
            lens[i] = len(v)
            table[i, :min(len(v), k)] = v[:k]
    return np.array(descs, dtype=REG_DTYPE), np.ascontiguousarray(table.reshape(-1)), lens


def carries_vector(regs):
    return any(_carrier(r.descriptor()) for r in regs)
