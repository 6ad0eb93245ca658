"""A numpy restatement of include/glrm_hip_cd.h, literally.  The Gram matrix is als_ref.gram (the header says: exactly that of
glrm_hip_als.h).  The rules -- diagonal, tolerance, start, residual, sweep, stop -- are written twice: ``sweeps_scalar``, the header's
loops one scalar at a time, and ``sweeps_vector``, the same operations on the same operands in the same order per entry with the residual
updated as one array expression (numpy's float64 ``*``, ``+``, ``-`` and ``/`` each round once, nothing here is fused);
tests/test_cd.py holds the two to each other bit for bit and the scalar form to brute force.  ``solve_side`` applies the vectorised
form to every segment of a problem in the ABI's layout; ``HostEngine`` answers ``cd_solve`` / ``cd_info`` (and ``als_solve`` /
``als_info``) for the CPU oracle, so that the driver (fit_b with CdParams) can be tested without a GPU; given the summation order a
handle of the HIP engine reports, it also adds the recorded objective as that engine does (``engine_col_losses``, ``engine_sum``)."""
import ctypes

import numpy as np

import als_ref
from als_ref import EPS, gram, loss_scales
from lowrankmodels.jl_amd import _capi

CONVERGED, SKIPPED = _capi.CD_CONVERGED, _capi.CD_SKIPPED
ZERO, QUAD, ONE, NONNEG = 0, 1, 2, 3            # include/glrm_hip.h: GLRM_REG_*
KINDS = (ZERO, QUAD, ONE, NONNEG)


def full(G):
    """The lower triangle -> the symmetric matrix (G_ic with c > i is read as G_ci)."""
    return G + np.tril(G, -1).T


def diagonal(G, kind, gamma):
    k = G.shape[0]
    M = np.zeros(k)
    for a in range(k):
        M[a] = G[a, a] + gamma if kind == QUAD else G[a, a]
    return M


def tolerance(M):
    k = len(M)
    maxd = M[0]
    for a in range(1, k):
        if M[a] > maxd:
            maxd = M[a]
    return (k * EPS) * maxd


def start(x, kind):
    x = np.array(x, dtype=np.float64)
    if kind == NONNEG:
        for a in range(len(x)):
            x[a] = x[a] if x[a] > 0 else 0.0
    return x


def new_value(kind, gamma, rho, Maa):
    """The minimiser of the segment's objective in one coordinate (the header's three formulas)."""
    if kind == ONE:
        h = 0.5 * gamma
        return (rho - h) / Maa if rho > h else (rho + h) / Maa if rho < -h else np.float64(0.0)
    q = rho / Maa
    if kind == NONNEG:
        return q if q > 0 else np.float64(0.0)
    return q


def sweeps_scalar(G, b, kind, gamma, x0, sweeps):
    """G: k x k with the lower triangle filled, b, the stored point -> (x, status bits, sweeps run).  The header's loops."""
    k = len(b)
    gamma = np.float64(gamma)
    M = diagonal(G, kind, gamma)
    tol = tolerance(M)
    x = start(x0, kind)
    S = lambda i, c: G[i, c] if i >= c else G[c, i]
    with np.errstate(all="ignore"):
        g = np.array(b, dtype=np.float64)
        for i in range(k):
            for c in range(k):
                g[i] = g[i] - S(i, c) * x[c]
        status, run = 0, 0
        while run < sweeps:
            changed = False
            for a in range(k):
                if not M[a] > tol:
                    status |= SKIPPED
                    if not (kind == ONE and gamma > 0):
                        continue
                    new = np.float64(0.0)
                else:
                    rho = g[a] + G[a, a] * x[a]
                    new = new_value(kind, gamma, rho, M[a])
                d = new - x[a]
                if not d == 0.0:
                    changed = True
                for i in range(k):
                    g[i] = g[i] - S(i, a) * d
                x[a] = new
            run += 1
            if not changed:
                status |= CONVERGED
                break
    return x, status, run


def sweeps_vector(G, b, kind, gamma, x0, sweeps):
    """The same operations per entry as sweeps_scalar; the residual's k entries are updated together."""
    k = len(b)
    gamma = np.float64(gamma)
    M = diagonal(G, kind, gamma)
    tol = tolerance(M)
    x = start(x0, kind)
    F = full(G)
    dg = np.diag(G).copy()
    one_to_zero = kind == ONE and gamma > 0
    ok = [bool(M[a] > tol) for a in range(k)]
    with np.errstate(all="ignore"):
        g = np.array(b, dtype=np.float64)
        for c in range(k):
            g = g - F[:, c] * x[c]
        status, run = 0, 0
        if not all(ok):
            status |= SKIPPED
        while run < sweeps:
            changed = False
            for a in range(k):
                if not ok[a]:
                    if not one_to_zero:
                        continue
                    new = np.float64(0.0)
                else:
                    new = new_value(kind, gamma, g[a] + dg[a] * x[a], M[a])
                d = new - x[a]
                if not d == 0.0:
                    changed = True
                g = g - F[:, a] * d
                x[a] = new
            run += 1
            if not changed:
                status |= CONVERGED
                break
    return x, status, run


def solve_segment(V, a, w, kind, gamma, x0, sweeps, form=sweeps_vector):
    """One segment -> (x, status bits, sweeps run)."""
    G, b = gram(np.asarray(V, dtype=np.float64), np.asarray(a, dtype=np.float64), np.asarray(w, dtype=np.float64))
    return form(G, b, kind, gamma, x0, sweeps)


def kinds_and_scales(regs, nseg):
    """REG_DTYPE descriptors (1 or nseg) -> (kind, scale) of every segment."""
    regs = np.asarray(regs)
    kind, scale = regs["kind"].astype(np.int64), regs["scale"].astype(np.float64)
    if len(kind) == 1:
        kind, scale = np.full(nseg, kind[0]), np.full(nseg, scale[0])
    assert np.all(np.isin(kind, KINDS)) and not np.any(regs["wrap"])
    return kind, scale


def solve_side_each(pa, side, X, Y, sweeps_list):
    """solve_side for every sweep count of ``sweeps_list`` from the same start, with each segment's Gram matrix formed once
    -> {sweeps: (factor, status, sweeps_run)}."""
    w_col = loss_scales(pa.losses, pa.n)
    if side == 0:
        ptr, idx, vals, own, opp, regs = pa.rowptr, pa.colidx, pa.rowvals, X, Y, pa.rx
    else:
        ptr, idx, vals, own, opp, regs = pa.colptr, pa.rowidx, pa.colvals, Y, X, pa.ry
    nseg = len(ptr) - 1
    kind, scale = kinds_and_scales(regs, nseg)
    res = {sw: (np.array(own, dtype=np.float64, order="F", copy=True), np.zeros(nseg, dtype=np.int8), np.zeros(nseg, dtype=np.int32)) for sw in sweeps_list}
    for s in range(nseg):
        j = np.asarray(idx[ptr[s]:ptr[s + 1]], dtype=np.int64)
        w = w_col[j] if side == 0 else np.full(len(j), w_col[s])
        G, b = gram(np.ascontiguousarray(opp[:, j].T, dtype=np.float64), np.asarray(vals[ptr[s]:ptr[s + 1]], dtype=np.float64), w)
        for sw, (out, status, run) in res.items():
            out[:, s], status[s], run[s] = sweeps_vector(G, b, int(kind[s]), scale[s], own[:, s], sw)
    return res


def solve_side(pa, side, X, Y, sweeps):
    """glrm_hip_cd_solve(h, side, sweeps) on the problem ``pa`` (a ProblemArrays, lists as the handle holds them) with factors X (k x m),
    Y (k x n) -> (new factor of the side, int8 status bits per segment, int32 sweeps run per segment).  The inputs are not written."""
    return solve_side_each(pa, side, X, Y, (sweeps,))[sweeps]


def counts(status, run):
    return dict(converged=int(np.sum((status & CONVERGED) != 0)), skipped=int(np.sum((status & SKIPPED) != 0)), sweeps_total=int(np.sum(run)))


def segment_objective(V, a, w, kind, gamma, x):
    """sum_t w_t (v_t.x - a_t)^2 + r(x) in np.longdouble (the brute force of tests/test_cd.py compares candidates with it)."""
    ld = np.longdouble
    V, a, w, x = (np.asarray(v, dtype=ld) for v in (V, a, w, x))
    r = V @ x - a
    val = np.sum(w * r * r)
    if kind == QUAD:
        val = val + ld(gamma) * np.sum(x * x)
    elif kind == ONE:
        val = val + ld(gamma) * np.sum(np.abs(x))
    elif kind == NONNEG and np.any(x < 0):
        return np.inf
    return float(val)


def engine_sum(v):
    """glrm_hip_sum's fixed order (csrc/glrm_hip.hip: sum_stage1 / sum_stage2): element i is added, i ascending, into accumulator
    (i mod 65536) of 256 blocks x 256 threads; every block is folded as a tree (t += t + s for s = 128, 64, ... 1), and the 256 block
    sums are folded the same way."""
    v = np.asarray(v, dtype=np.float64)
    acc = np.zeros(65536)
    for s in range(0, len(v), 65536):
        c = v[s:s + 65536]
        acc[:len(c)] = acc[:len(c)] + c
    acc = acc.reshape(256, 256)
    for level in (acc, None):
        if level is None:
            acc = acc[:, 0].copy()[None, :]
        s = 128
        while s > 0:
            acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
            s >>= 1
    return float(acc[0, 0])


def engine_col_losses(pa, X, Y, order):
    """glrm_hip_col_losses of a handle whose column view adds in the STRIDED order ``order`` (a CSumOrder, include/glrm_hip.h:
    GLRM_ORDER_STRIDED): the column sweep in evaluation mode, through the lane-by-lane simulation tests/lane_orders.py keeps of it."""
    import lane_orders
    assert order.family == 1 and order.batch == 1 and order.lanes * order.comps >= pa.k, order.asdict()
    w_col = loss_scales(pa.losses, pa.n)
    rows = [X[:, i] for i in range(pa.m)]
    out = np.zeros(pa.n)
    for j in range(pa.n):
        lo, hi = pa.colptr[j], pa.colptr[j + 1]
        waves = order.waves or (1 if hi - lo < order.waves4_from else 4 if hi - lo < order.waves8_from else 8)
        out[j] = lane_orders.strided_pass(pa.rowidx[lo:hi], pa.colvals[lo:hi], Y[:, j], rows, pa.k, order.lanes, order.comps, waves, w_col[j], False)[0]
    return out


class HostEngine(als_ref.HostEngine):
    """als_ref.HostEngine with ``cd_solve`` / ``cd_info`` answered by the restatement: get_factors -> solve_side -> set_factors.

    ``column_order``: the CSumOrder a handle of the HIP engine reports for its column view (Api.sum_order(h, 1)).  With it the objective
    entry points the drivers record their history with -- ``col_losses`` into the bound buffer and ``sum`` -- add in THAT engine's
    orders (engine_col_losses, engine_sum) where the oracle adds in the reference's, so that a history can be compared bit for bit;
    the penalties are the oracle's (a k-term sum per segment that both engines form alike).  Without it everything is the oracle's."""

    has_cd = True

    def __init__(self, api, column_order=None):
        super().__init__(api)
        self._cd = {}
        self._order = column_order
        self._bound = {}

    def bind_buffers(self, h, dX, dY, p_col, p_row):
        self._bound[h.value] = p_col
        self._api.bind_buffers(h, dX, dY, p_col, p_row)

    def col_losses(self, h):
        if self._order is None or not self._bound.get(h.value):
            return self._api.col_losses(h)
        pa = self._pa[h.value]
        X, Y = np.zeros((pa.k, pa.m), order="F"), np.zeros((pa.k, pa.n), order="F")
        self._api.get_factors(h, X, Y)
        np.ctypeslib.as_array((ctypes.c_double * pa.n).from_address(int(self._bound[h.value])))[:] = engine_col_losses(pa, X, Y, self._order)

    def sum(self, h, vec, n):
        if self._order is None:
            return self._api.sum(h, vec, n)
        return engine_sum(np.ctypeslib.as_array((ctypes.c_double * int(n)).from_address(int(vec))))

    def destroy(self, h):
        if h is not None and h.value:
            self._cd = {k: v for k, v in self._cd.items() if k[0] != h.value}
        super().destroy(h)

    def cd_solve(self, h, side, sweeps):
        if side not in (0, 1):
            raise _capi.GLRMError(_capi.ERR_INVALID, "glrm_hip_cd_solve: side must be 0 (rows of X) or 1 (columns of Y)")
        if not 1 <= sweeps <= _capi.CD_MAX_SWEEPS:
            raise _capi.GLRMError(_capi.ERR_INVALID, f"glrm_hip_cd_solve: sweeps must be in [1, GLRM_CD_MAX_SWEEPS = {_capi.CD_MAX_SWEEPS}], got {sweeps}")
        pa = self._pa[h.value]
        X, Y = np.zeros((pa.k, pa.m), order="F"), np.zeros((pa.k, pa.n), order="F")
        self._api.get_factors(h, X, Y)
        new, status, run = solve_side(pa, side, X, Y, sweeps)
        self._api.set_factors(h, new if side == 0 else X, Y if side == 0 else new)
        self._cd[(h.value, side)] = (status, run)

    def cd_info(self, h, side, nseg=None):
        if (h.value, side) not in self._cd:
            raise _capi.GLRMError(_capi.ERR_INVALID, f"glrm_hip_cd_info: glrm_hip_cd_solve has not run on side {side} of this handle")
        status, run = self._cd[(h.value, side)]
        out = counts(status, run)
        if nseg is not None:
            out["status"], out["sweeps_run"] = status.copy(), run.copy()
        return out
