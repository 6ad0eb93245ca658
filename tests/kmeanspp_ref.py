"""A numpy transcription of init_kmeanspp! (reference: src/initialize.jl:8-33) with the caller's draws, in the REFERENCE's order:
sequential sums in list order and the distance vector d recomputed for every centre in every round (no running minimum -- so the
engine's identity `best = min(best, newest distance)` is what the comparison tests).

wsample(1:m, w) is StatsBase's, written from memory (it is not in the reference tree): t = rand() * sum(w);
i = 1; cw = w[1]; while cw < t && i < m: i += 1; cw += w[i]; return i.  One uniform draw per call.

Everything is 0-based.  The lists are the ABI's row view (rowptr, colidx, rowvals): a column listed twice in a row may carry two
different values there, and the assignment `Y[l, obs] = A[i, obs]` then leaves the LAST one."""
import math

import numpy as np


def wsample(w, u):
    """-> (index, margin): margin = min(t - c_{i-1}, c_i - t) / S, the distance of the draw from the nearest boundary of the
    cumulative weights next to the chosen row, relative to the total.  It is +Inf for a draw that no rounding can move: t == 0
    (u == 0 or S == 0) and a NaN t fail `cw < t` at once whatever the last bits of w and S are, so row 0 is returned."""
    m = len(w)
    S = 0.0
    for x in w:          # sum(w): its rounding differs from Julia's pairwise sum by O(m eps), far inside the margins asserted
        S += float(x)
    t = u * S
    i, before, cw = 0, 0.0, float(w[0])
    while cw < t and i < m - 1:
        i += 1
        before = cw
        cw += float(w[i])
    if t == 0 or t != t:
        return i, math.inf
    return i, min(t - before, cw - t) / S


def init_kmeanspp(m, n, k, rowptr, colidx, rowvals, losses, Y0, first, uniforms):
    """losses: n Loss objects (scalar).  Y0: the randn(k, n) draw.  first: the first centre.  uniforms: k-1 draws.
    -> dict(Y, centers, weights [(k-1) x m], margins [k-1])."""
    Y = np.array(Y0, dtype=np.float64, order="F")
    assert Y.shape == (k, n)
    obs = [np.asarray(colidx[rowptr[i]:rowptr[i + 1]], dtype=np.int64) for i in range(m)]
    val = [np.asarray(rowvals[rowptr[i]:rowptr[i + 1]], dtype=np.float64) for i in range(m)]

    def assign(l, i):
        for j, a in zip(obs[i], val[i]):   # in list order: a repeated column is assigned again
            Y[l, j] = a

    possible = set(range(m))
    possible.discard(first)                # setdiff!(possible_centers, i): the only removal there is
    centers = [int(first)]
    assign(0, first)
    weights = np.zeros((max(k - 1, 0), m))
    margins = np.zeros(max(k - 1, 0))
    for l in range(1, k):
        w = np.zeros(m)
        for i in possible:
            d = [0.0] * l
            for j, a in zip(obs[i], val[i]):
                for ll in range(l):
                    d[ll] += float(losses[j].evaluate(float(Y[ll, j]), float(a)))
            mn = math.nan if any(x != x for x in d) else min(d)   # Julia's minimum propagates a NaN
            w[i] = mn / len(obs[i]) if len(obs[i]) else math.nan  # 0 / 0
        weights[l - 1] = w
        nxt, margins[l - 1] = wsample(w, float(uniforms[l - 1]))
        centers.append(nxt)
        assign(l, nxt)
    return dict(Y=Y, centers=np.array(centers, dtype=np.int64), weights=weights, margins=margins)
