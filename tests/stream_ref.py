"""A numpy restatement of include/glrm_hip_stream.h, literally: ``plan`` is the header's plan, ``stream_rows`` one row's arithmetic after
another (numpy's float64 ``*``, ``+``, ``-``, ``/`` each round once and nothing here is fused; the Gram matrix, the Cholesky and the
substitutions are als_ref's, which restate glrm_hip_als.h).  Rows are walked in ascending order: the level schedule only says which of them
may run side by side.  ``HostEngine`` answers ``stream_rows`` / ``stream_info`` for the CPU oracle, so that the drivers (streaming_fit,
streaming_impute_at, streaming_impute) can be tested without a GPU.

Also here: ``literal``, a transcription of src/algorithms/quad_streaming.jl as it stands -- np.linalg.solve, one division of all of Y per
interval, a dense Ahat -- which the restatement is compared with up to rounding."""
import numpy as np

import als_ref as A_
from lowrankmodels.jl_amd import _capi

SOLVED, KEPT_SHORT, KEPT_PIVOT = A_.SOLVED, A_.KEPT_SHORT, A_.KEPT_PIVOT


def plan(m, n, first, rowptr, colidx, qptr=None, qcol=None, sequential=False):
    """-> dict(level, nlevels, nlaunches, max_width, dup_rows), the header's plan"""
    lastw, lastr = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    level, dup = np.zeros(m - first, dtype=np.int64), 0
    for i in range(first, m):
        obs = np.asarray(colidx[rowptr[i]:rowptr[i + 1]], dtype=np.int64)
        q = np.zeros(0, dtype=np.int64) if qptr is None else np.asarray(qcol[qptr[i]:qptr[i + 1]], dtype=np.int64)
        L = 1 + max([0] + list(np.maximum(lastw[obs], lastr[obs])) + list(lastw[q]))
        lastw[obs] = L
        lastr[q] = np.maximum(lastr[q], L)
        level[i - first] = i - first + 1 if sequential else L
        dup += len(set(obs.tolist())) < len(obs)
    width = np.bincount(level)[1:] if len(level) else np.zeros(0, dtype=np.int64)
    one = width == 1                                                 # a maximal run of one-row levels is ONE launch
    launches = int(np.sum(~one)) + int(np.sum(one & ~np.concatenate([[False], one[:-1]])))
    return dict(level=level, nlevels=len(width), nlaunches=launches, max_width=int(width.max()) if len(width) else 0, dup_rows=dup)


def power(c, d):
    """p = c, then p = p * c repeated d - 1 times"""
    p = float(c)
    with np.errstate(over="ignore"):
        for _ in range(int(d) - 1):
            p = float(np.float64(p) * np.float64(c))
            if np.isinf(p):
                break                                                # c >= 1: it stays there
    return p


def dots(V, x):
    """sum_a V[:, a] * x[a], a ascending from +0.0, one accumulator per row of V"""
    acc = np.zeros(V.shape[0])
    for a in range(len(x)):
        acc = acc + V[:, a] * x[a]
    return acc


def stream_rows(pa, X, Y, first, stepsize, interval, qptr=None, qcol=None, trace=None):
    """glrm_hip_stream_rows on the problem ``pa`` (a ProblemArrays, lists as the handle holds them) with factors X (k x m), Y (k x n)
    -> dict(X, Y, objective, status, qout).  The inputs are not written.  ``trace`` (a list) receives, per row, what the solve saw: dict(i, V, a, gamma, status)."""
    m, n, k = pa.m, pa.n, pa.k
    X, Y = np.array(X, dtype=np.float64, order="F", copy=True), np.array(Y, dtype=np.float64, order="F", copy=True)
    gam = A_.gammas(pa.rx, m)
    sy = float(A_.gammas(pa.ry, n)[0])
    c = 1.0 + ((2.0 * stepsize) * float(interval)) * sy
    epoch = np.zeros(n, dtype=np.int64)
    objective, status = np.full(m - first, np.nan), np.zeros(m - first, dtype=np.int8)
    qout = None if qptr is None else np.full(int(qptr[m]), np.nan)
    with np.errstate(all="ignore"):
        for i in range(first, m):
            lo, hi = int(pa.rowptr[i]), int(pa.rowptr[i + 1])
            obs, a = np.asarray(pa.colidx[lo:hi], dtype=np.int64), np.asarray(pa.rowvals[lo:hi], dtype=np.float64)
            D = i // interval - first // interval
            if c != 1.0:                                             # the pending decay of the row's columns
                for j in dict.fromkeys(obs.tolist()):
                    d = D - epoch[j]
                    if d > 0:
                        Y[:, j] = Y[:, j] / power(c, d)
                        epoch[j] = D
            V = np.ascontiguousarray(Y[:, obs].T)
            if gam[i] == 0.0 and len(obs) < k:
                st, x = KEPT_SHORT, None
            else:
                G, b = A_.gram(V, a, np.ones(len(obs)))
                M = G.copy()
                for d_ in range(k):
                    M[d_, d_] = G[d_, d_] + (gam[i] + gam[i])
                st, x = A_.cholesky_solve(M, b)
            status[i - first] = st
            if trace is not None:
                trace.append(dict(i=i, V=V, a=a, gamma=gam[i], status=st))
            if st == SOLVED:
                X[:, i] = x
            x = X[:, i].copy()
            if qptr is not None:                                     # Y as the row found it; a reader writes nothing back
                for e in range(int(qptr[i]), int(qptr[i + 1])):
                    j = int(qcol[e])
                    y, d = Y[:, j], D - epoch[j]
                    if c != 1.0 and d > 0:
                        y = y / power(c, d)
                    qout[e] = dots(y[None, :], x)[0]
            if st != SOLVED:
                continue
            r = dots(V, x) - a
            acc = 0.0
            for t in range(len(obs)):
                acc = acc + r[t] * r[t]
            objective[i - first] = acc
            for t in range(len(obs)):
                Y[:, obs[t]] = Y[:, obs[t]] - (stepsize * r[t]) * x
        total = m // interval - first // interval
        if c != 1.0:
            for j in range(n):
                if total - epoch[j] > 0:
                    Y[:, j] = Y[:, j] / power(c, total - epoch[j])
    return dict(X=X, Y=Y, objective=objective, status=status, qout=qout)


def literal(pa, X, Y, T0, stepsize, interval, A=None):
    """src/algorithms/quad_streaming.jl:47-72 / :104-136 as written: -> dict(X, Y, objective, Ahat); Ahat (with ``A``, the dense m x n
    matrix) as streaming_impute! fills it."""
    m, n, k = pa.m, pa.n, pa.k
    X, Y = np.array(X, dtype=np.float64, copy=True), np.array(Y, dtype=np.float64, copy=True)
    gam = A_.gammas(pa.rx, m)
    sy = float(A_.gammas(pa.ry, n)[0])
    Ahat = None if A is None else np.array(A, dtype=np.float64, copy=True)
    objective = []
    for i1 in range(T0 + 1, m + 1):
        i = i1 - 1
        obs = np.asarray(pa.colidx[pa.rowptr[i]:pa.rowptr[i + 1]], dtype=np.int64)
        Yobs, Aobs = Y[:, obs], np.asarray(pa.rowvals[pa.rowptr[i]:pa.rowptr[i + 1]], dtype=np.float64)
        X[:, i] = np.linalg.solve(Yobs @ Yobs.T + 2 * gam[i] * np.eye(k), Yobs @ Aobs)
        xi = X[:, i]
        if Ahat is not None:
            not_obs = np.setdiff1d(np.arange(n), obs)
            if len(not_obs) > 0:
                ahat = xi @ Y
                Ahat[i, not_obs] = ahat[not_obs]
        r = Yobs.T @ xi - Aobs
        objective.append(np.linalg.norm(r) ** 2)
        for jj in range(len(obs)):
            Y[:, obs[jj]] -= stepsize * r[jj] * xi
        if i1 % interval == 0:
            Y /= (1 + 2 * stepsize * interval * sy)
    return dict(X=X, Y=Y, objective=np.array(objective), Ahat=Ahat)


def pattern(m, n, q, seed):
    """q distinct columns per row from ONE generator: -> the rows' column lists"""
    rng = np.random.default_rng(seed)
    return [rng.choice(n, q, replace=False) for _ in range(m)]


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    idx = np.concatenate([np.asarray(l, dtype=np.int32) for l in lists] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    return ptr, idx


def model(lists, n, k, seed, rx_scales=(0.1, 0.5, 2.5), sy=0.3):
    """A seeded QuadLoss model over the rows' column lists (a column may be named twice in a row): per-row QuadReg scales drawn from
    ``rx_scales`` (0: ZeroReg), one ry scale (0: ZeroReg).  Every row's list goes over in ascending order, the order every family of
    the engine then holds.  -> (glrm, X0, Y0)"""
    import lowrankmodels.jl_amd as L
    rng = np.random.default_rng(50_000 + seed)
    m = len(lists)
    I = np.concatenate([np.full(len(l), i) for i, l in enumerate(lists)] + [np.zeros(0)]).astype(np.int64)
    J = np.concatenate([np.sort(np.asarray(l)) for l in lists] + [np.zeros(0)]).astype(np.int64)
    X0, Y0 = rng.standard_normal((k, m)), rng.standard_normal((k, n))
    A = X0.T @ Y0 + 0.1 * rng.standard_normal((m, n))
    rx = [L.QuadReg(g) if g > 0 else L.ZeroReg() for g in rng.choice(rx_scales, size=m)]
    g = L.GLRM(A, L.QuadLoss(), rx, L.QuadReg(sy) if sy > 0 else L.ZeroReg(), k, obs=(I, J), X=rng.standard_normal((k, m)), Y=Y0 + 0.05 * rng.standard_normal((k, n)))
    return g, np.asfortranarray(g.X.copy()), np.asfortranarray(g.Y.copy())


class HostEngine(A_.HostEngine):
    """als_ref.HostEngine (the CPU oracle's Api, which keeps the problem arrays given to ``create``) with ``stream_rows`` / ``stream_info``
    answered by the restatement: get_factors -> stream_rows -> set_factors."""

    has_stream = True

    def __init__(self, api):
        super().__init__(api)
        self._stream_last = {}

    def stream_rows(self, h, m, first, stepsize, interval, sequential=False, qptr=None, qcol=None, want_objective=True):
        pa = self._pa[h.value]
        if not 1 <= first <= pa.m:
            raise _capi.GLRMError(_capi.ERR_INVALID, f"glrm_hip_stream_rows: first must be in 1 .. m = {pa.m}, got {first}")
        X, Y = np.zeros((pa.k, pa.m), order="F"), np.zeros((pa.k, pa.n), order="F")
        self._api.get_factors(h, X, Y)
        out = stream_rows(pa, X, Y, first, stepsize, interval, qptr, qcol)
        self._api.set_factors(h, np.asfortranarray(out["X"]), np.asfortranarray(out["Y"]))
        p = plan(pa.m, pa.n, first, pa.rowptr, pa.colidx, qptr, qcol, sequential)
        self._stream_last[h.value] = dict(A_.counts(out["status"]), nlevels=p["nlevels"], nlaunches=p["nlaunches"], max_width=p["max_width"], plan_ms=0.0,
                                          status=out["status"])
        return (out["objective"] if want_objective else None), out["qout"]

    def stream_info(self, h, rows=None):
        if h.value not in self._stream_last:
            raise _capi.GLRMError(_capi.ERR_INVALID, "glrm_hip_stream_info: glrm_hip_stream_rows has not run on this handle")
        out = dict(self._stream_last[h.value])
        status = out.pop("status")
        if rows is not None:
            out["status"] = status.copy()
        return out
