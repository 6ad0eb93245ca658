"""A numpy restatement of include/glrm_hip_als.h, literally: the Gram matrix as a loop over t of ``G += np.outer(u, v)`` (one accumulator per
entry, t ascending; numpy's float64 ``*``, ``+``, ``-``, ``/`` and ``sqrt`` each round once, and nothing here is fused), scalar loops for the
left-looking Cholesky and the two substitutions, the pivot and short rules in the header's words.  ``solve_side`` applies it to every
segment of a problem in the ABI's layout; ``HostEngine`` answers ``als_solve`` / ``als_info`` for the CPU oracle, so that the driver
(fit_b with AlsParams, transform(exact=True)) can be tested without a GPU.

Also here: the derived backward-error bound the tests hold a solve to (``residual_ratio``)."""
import numpy as np

from lowrankmodels.jl_amd import _capi

SOLVED, KEPT_SHORT, KEPT_PIVOT = _capi.ALS_SOLVED, _capi.ALS_KEPT_SHORT, _capi.ALS_KEPT_PIVOT
EPS = 2.0 ** -52


def gram(V, a, w):
    """V: L x k opposing vectors in list order, a: L values, w: L weights -> (G lower triangle in a full k x k array, b)."""
    L, k = V.shape
    G, b = np.zeros((k, k)), np.zeros(k)
    for t in range(L):
        u = w[t] * V[t]                      # rounded
        G += np.outer(u, V[t])               # G_ab += u_ta * v_tb: a multiply, then an add, per entry
        b += u * a[t]
    return np.tril(G), b


def pivot_tolerance(M):
    k = M.shape[0]
    maxd = M[0, 0]
    for a in range(1, k):
        if M[a, a] > maxd:
            maxd = M[a, a]
    return (k * EPS) * maxd


def cholesky_solve_scalar(M, b):
    """M: k x k, lower triangle used, diagonal already M_aa = G_aa + gamma -> (status, x or None).  The header's loops, one scalar at a time."""
    k = len(b)
    tol = pivot_tolerance(M)
    Lm = np.zeros((k, k))
    with np.errstate(all="ignore"):
        for j in range(k):
            for i in range(j, k):
                s = M[i, j]
                for c in range(j):
                    s = s - Lm[i, c] * Lm[j, c]
                if i == j:
                    if not s > tol:
                        return KEPT_PIVOT, None
                    Lm[j, j] = np.sqrt(s)
                else:
                    Lm[i, j] = s / Lm[j, j]
        z = np.zeros(k)
        for i in range(k):
            s = b[i]
            for c in range(i):
                s = s - Lm[i, c] * z[c]
            z[i] = s / Lm[i, i]
        x = np.zeros(k)
        for i in range(k - 1, -1, -1):
            s = z[i]
            for c in range(k - 1, i, -1):
                s = s - Lm[c, i] * x[c]
            x[i] = s / Lm[i, i]
    return SOLVED, x


def cholesky_solve(M, b):
    """The same operations on the same operands in the same order PER ENTRY as cholesky_solve_scalar, dealt out differently: the rows of a
    column together, and the substitutions column by column (entry i still subtracts its products c ascending / descending, one at a
    time).  Bit for bit the scalar form (tests/test_als.py holds it to that); what the tests with hundreds of segments run."""
    k = len(b)
    tol = pivot_tolerance(M)
    Lm = np.zeros((k, k))
    with np.errstate(all="ignore"):
        for j in range(k):
            s = M[j:, j].copy()
            for c in range(j):
                s = s - Lm[j:, c] * Lm[j, c]
            if not s[0] > tol:
                return KEPT_PIVOT, None
            d = np.sqrt(s[0])
            Lm[j, j] = d
            Lm[j + 1:, j] = s[1:] / d
        s = np.array(b, dtype=np.float64)
        for c in range(k):
            s[c] = s[c] / Lm[c, c]
            s[c + 1:] = s[c + 1:] - Lm[c + 1:, c] * s[c]
        for c in range(k - 1, -1, -1):
            s[c] = s[c] / Lm[c, c]
            s[:c] = s[:c] - Lm[c, :c] * s[c]
    return SOLVED, s


def solve_segment(V, a, w, gamma):
    """One segment -> (status, x or None)."""
    L, k = V.shape
    if gamma == 0.0 and L < k:
        return KEPT_SHORT, None
    G, b = gram(np.asarray(V, dtype=np.float64), np.asarray(a, dtype=np.float64), np.asarray(w, dtype=np.float64))
    M = G.copy()
    for d in range(k):
        M[d, d] = G[d, d] + gamma
    return cholesky_solve(M, b)


def gammas(regs, nseg):
    """REG_DTYPE descriptors (1 or nseg) -> the penalty scale of every segment."""
    regs = np.asarray(regs)
    g = np.where(regs["kind"] == 1, regs["scale"], 0.0).astype(np.float64)
    return np.full(nseg, g[0]) if len(g) == 1 else g


def loss_scales(losses, n):
    s = np.asarray(losses)["scale"].astype(np.float64)
    return np.full(n, s[0]) if len(s) == 1 else s


def solve_side(pa, side, X, Y):
    """glrm_hip_als_solve(h, side) on the problem ``pa`` (a ProblemArrays, lists as the handle holds them) with factors X (k x m), Y (k x n)
    -> (new factor of the side, int8 status per segment).  The inputs are not written."""
    w_col = loss_scales(pa.losses, pa.n)
    if side == 0:
        ptr, idx, vals, own, opp, regs = pa.rowptr, pa.colidx, pa.rowvals, X, Y, pa.rx
    else:
        ptr, idx, vals, own, opp, regs = pa.colptr, pa.rowidx, pa.colvals, Y, X, pa.ry
    nseg = len(ptr) - 1
    g = gammas(regs, nseg)
    out = np.array(own, dtype=np.float64, order="F", copy=True)
    status = np.zeros(nseg, dtype=np.int8)
    for s in range(nseg):
        j = np.asarray(idx[ptr[s]:ptr[s + 1]], dtype=np.int64)
        w = w_col[j] if side == 0 else np.full(len(j), w_col[s])
        st, x = solve_segment(np.ascontiguousarray(opp[:, j].T), vals[ptr[s]:ptr[s + 1]], w, g[s])
        status[s] = st
        if st == SOLVED:
            out[:, s] = x
    return out, status


def counts(status):
    return dict(solved=int(np.sum(status == SOLVED)), kept_short=int(np.sum(status == KEPT_SHORT)), kept_pivot=int(np.sum(status == KEPT_PIVOT)))


def residual_ratio(V, a, w, gamma, x):
    """max over the entries of |(G + gamma I) x - b| / bound, the bound being (L + 3k + 2) 2^-52 (k (|G|_abs + gamma I) |x| + |b|_abs) with
    |G|_abs = sum_t |w_t| |v_t| |v_t|' and |b|_abs = sum_t |w_t a_t| |v_t|: the dot-product bound of the L-term sums of the Gram matrix and
    the right-hand side plus Higham's bound for a Cholesky solve (Accuracy and Stability of Numerical Algorithms, theorem 10.4:
    |dA| <= gamma_{3k+1} |R'||R|, and |R'||R| <= k (|A|) entrywise up to higher order).  Residuals in np.longdouble."""
    ld = np.longdouble
    V, a, w, x = (np.asarray(v, dtype=ld) for v in (V, a, w, x))
    L, k = V.shape
    G = (V * w[:, None]).T @ V
    b = (V * (w * a)[:, None]).sum(axis=0)
    Gabs = (np.abs(V) * np.abs(w)[:, None]).T @ np.abs(V)
    babs = (np.abs(V) * np.abs(w * a)[:, None]).sum(axis=0)
    res = np.abs(G @ x + ld(gamma) * x - b)
    bound = ld((L + 3 * k + 2) * EPS) * (k * (Gabs @ np.abs(x) + ld(gamma) * np.abs(x)) + babs)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, res / bound, np.where(res == 0, 0.0, np.inf))
    return float(np.max(r))


class HostEngine:
    """The CPU oracle's Api with ``als_solve`` / ``als_info`` answered by the restatement: get_factors -> solve_side -> set_factors.  It keeps
    the problem arrays given to ``create`` (the oracle does not hand its lists back).  Every other attribute is the oracle's."""

    def __init__(self, api):
        self._api = api
        self._pa = {}
        self._info = {}
        self.created = 0

    def __getattr__(self, name):
        return getattr(self._api, name)

    has_als = True

    def create(self, prob, **kw):
        h = self._api.create(prob, **kw)
        self.created += 1
        self._pa[h.value] = prob
        return h

    def destroy(self, h):
        if h is not None and h.value:
            self._pa.pop(h.value, None)
            self._info = {k: v for k, v in self._info.items() if k[0] != h.value}
        self._api.destroy(h)

    def als_solve(self, h, side):
        if side not in (0, 1):
            raise _capi.GLRMError(_capi.ERR_INVALID, "glrm_hip_als_solve: side must be 0 (rows of X) or 1 (columns of Y)")
        pa = self._pa[h.value]
        X, Y = np.zeros((pa.k, pa.m), order="F"), np.zeros((pa.k, pa.n), order="F")
        self._api.get_factors(h, X, Y)
        new, status = solve_side(pa, side, X, Y)
        self._api.set_factors(h, new if side == 0 else X, Y if side == 0 else new)
        self._info[(h.value, side)] = status

    def als_info(self, h, side, nseg=None):
        if (h.value, side) not in self._info:
            raise _capi.GLRMError(_capi.ERR_INVALID, f"glrm_hip_als_info: glrm_hip_als_solve has not run on side {side} of this handle")
        status = self._info[(h.value, side)]
        out = counts(status)
        if nseg is not None:
            out["status"] = status.copy()
        return out
