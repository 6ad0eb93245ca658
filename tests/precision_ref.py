"""numpy restatement of precision_at_k (src/cross_validate.jl:243-304): the dense XY, the full sort, the literal double loop.

The pieces are exposed one by one because the engine's extension (include/glrm_hip_topk.h) is tested piece by piece:
  xy_chain     the value u_ij as the header defines it (u = +0.0; u = x_c y_c + u, c ascending), unfused.  It has the bits of the fma
               chain whenever every product is exact (factors that are small multiples of 1/2, powers of two) and for k = 1, where
               fma(x, y, +0.0) is the rounded product -- with the sign of a zero product resolved the same way (-0.0 + +0.0 = +0.0);
  select       sort(XY[:], rev=true)[rank] under Julia's isless (-0.0 < +0.0, NaN greatest, every NaN one value), with the counts above / equal;
  scan         the double loop of :275-297;
  precision_at_k  the driver, with its fits run through the engine it is given and everything after the fit in numpy.
"""
import numpy as np

import lowrankmodels.jl_amd as L

SIGN = np.uint64(1) << np.uint64(63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
QNAN = np.uint64(0x7FF8000000000000)


def xy_chain(X, Y):
    """X: k x m, Y: k x n -> m x n."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    u = np.zeros((X.shape[1], Y.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(X.shape[0]):
            u = X[c][:, None] * Y[c][None, :] + u
    return u


def keys(u):
    """The order-preserving 64-bit key of include/glrm_hip_topk.h."""
    u = np.ascontiguousarray(u, dtype=np.float64)
    b = u.view(np.uint64)
    k = np.where((b >> np.uint64(63)).astype(bool), ~b, b | SIGN)
    return np.where(np.isnan(u), ONES, k)


def unkey(k):
    k = np.uint64(k)
    b = QNAN if k == ONES else ((k ^ SIGN) if (k >> np.uint64(63)) else ~k)
    return np.array([b], dtype=np.uint64).view(np.float64)[0]


class Sorted:
    """All keys of a matrix, sorted once (descending); select(rank) -> (q, n_gt, n_eq)."""

    def __init__(self, XY):
        self.desc = np.sort(keys(XY).ravel())[::-1]
        self.asc = self.desc[::-1]

    def select(self, rank):
        if not 1 <= rank <= len(self.desc):
            raise IndexError("BoundsError")
        k = self.desc[rank - 1]
        n = len(self.asc)
        n_gt = n - int(np.searchsorted(self.asc, k, side="right"))
        n_eq = n - int(np.searchsorted(self.asc, k, side="left")) - n_gt
        return unkey(k), n_gt, n_eq


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def scan(XY, q, train_lists, test_lists, kprec):
    """The loop of :275-297 (0-based).  Returns (true_pos, false_pos, hits [(i, j, is_true)], rows_scanned) with rows_scanned = the index
    after the last row the loop entered."""
    m, n = XY.shape
    true_pos = false_pos = kfound = 0
    hits, rows_scanned = [], 0
    for i in range(m):
        if kfound >= kprec:
            break
        rows_scanned = i + 1
        test_i, train_i = set(int(j) for j in test_lists[i]), set(int(j) for j in train_lists[i])
        for j in range(n):
            if kfound >= kprec:
                break
            if XY[i, j] >= q:
                if j in test_i:
                    true_pos += 1
                    kfound += 1
                    hits.append((i, j, True))
                elif j not in train_i:
                    false_pos += 1
                    kfound += 1
                    hits.append((i, j, False))
    return true_pos, false_pos, hits, rows_scanned


def precision_at_k(train_glrm, test_observed_features, params, reg_params, kprec, rng, engine):
    """:243-304 with the fits and the two objectives on ``engine`` and XY, the sort and the loop in numpy."""
    m, n, k = train_glrm.m, train_glrm.n, train_glrm.k
    ntrain = sum(len(r) for r in train_glrm.observed_features)
    train_lists = train_glrm.observed_features
    nparams = len(reg_params)
    train_error, test_error, prec, train_time = (np.full(nparams, np.nan) for _ in range(4))
    solution = np.full((nparams, 2), np.nan)
    test_glrm = L.GLRM(train_glrm.A, train_glrm.losses, train_glrm.rx, train_glrm.ry, k, X=train_glrm.X.copy(), Y=train_glrm.Y.copy(),
                       observed_features=test_observed_features)
    ch = L.ConvergenceHistory("reg_path")
    for ip, reg_param in enumerate(reg_params):
        for r in list(train_glrm.rx) + list(train_glrm.ry):
            r.mul_(reg_param)
        train_glrm.X[...] = rng.standard_normal((k, m))
        train_glrm.Y[...] = rng.standard_normal((k, n))
        X, Y, ch = L.fit_b(train_glrm, params, ch=ch, verbose=False, engine=engine)
        train_time[ip] = ch.times[-1]
        train_error[ip] = L.objective(train_glrm, X, Y, include_regularization=False, engine=engine) / ntrain
        test_error[ip] = L.objective(test_glrm, X, Y, include_regularization=False, engine=engine) / ntrain
        XY = xy_chain(X, Y)
        q = Sorted(XY).select(ntrain)[0]
        true_pos, false_pos, _, _ = scan(XY, q, train_lists, test_observed_features, kprec)
        with np.errstate(divide="ignore", invalid="ignore"):
            prec[ip] = np.float64(true_pos) / np.float64(true_pos + false_pos)
        solution[ip] = (np.sum(X) + np.sum(Y), np.sum(np.abs(X)) + np.sum(np.abs(Y)))
    test_glrm.close()
    return train_error, test_error, prec, train_time, np.asarray(reg_params, dtype=float), solution
