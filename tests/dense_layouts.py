"""Storage layouts and launch-shape problems for the dense hand-over tests (tests/test_gpu_dense_shapes.py, tests/test_dense_layouts.py).

`relayout` re-stores the matrix of a dense ProblemArrays the way another host would hand it over: row-major or column-major (what
julia/HipGLRM.jl passes), with a leading dimension larger than the matrix, on the host or on the device.  The padding between the runs
is NaN: the library must never read it (a read would poison the objective) and its NaN check must not look at it.

`dense_problem` builds a fully observed QuadLoss problem twice without going through a GLRM: as the dense hand-over for the engine and as
the explicit `fill(1:n, m)` lists the oracle runs on."""
import copy

import numpy as np

from lowrankmodels.jl_amd import _capi

QUADREG, NONNEG, ZEROREG = (1, 0, 0.1), (3, 0, 1.0), (0, 0, 1.0)   # glrm_reg descriptors (kind, wrap, scale)


def relayout(pa, colmajor, pad, device=False):
    """The dense ProblemArrays `pa` (row-major, ld = n: what GLRM.problem_arrays(dense=True, ...) returns) with dense_A re-stored
    row-major with ld = n + pad (colmajor = 0) or column-major with ld = m + pad (colmajor = 1), on the host (a numpy buffer) or on
    the device (a torch tensor, flags |= PROBLEM_DEVICE_ARRAYS).  The returned object keeps the buffer alive (`.dense_keep`)."""
    assert pa.dense_A is not None and not pa.dense_colmajor and isinstance(pa.dense_A, np.ndarray)
    m, n = pa.m, pa.n
    A = np.asarray(pa.dense_A, dtype=np.float64).reshape(m, pa.dense_ld)[:, :n]
    runs, run = (n, m) if colmajor else (m, n)
    buf = np.full((runs, run + pad), np.nan)
    buf[:, :run] = A.T if colmajor else A
    assert not np.isnan(buf[:, :run]).any() and np.isnan(buf[:, run:]).all()
    out = copy.copy(pa)
    out.dense_ld, out.dense_colmajor = run + pad, 1 if colmajor else 0
    if device:
        import torch
        t = torch.from_numpy(buf).to("cuda")
        torch.cuda.synchronize()   # the handle reads it from a stream of its own
        out.dense_A, out.dense_keep = t.data_ptr(), t
        out.flags = pa.flags | _capi.PROBLEM_DEVICE_ARRAYS
    else:
        out.dense_A = out.dense_keep = buf
    return out


def logical(pa):
    """The m x n matrix a HOST dense ProblemArrays describes, read entry by entry through the ABI's indexing rule
    (A(i,j) = dense_A[i + j*ld] if dense_colmajor else dense_A[i*ld + j], include/glrm_hip.h)."""
    flat = np.asarray(pa.dense_A).reshape(-1)
    i, j = np.meshgrid(np.arange(pa.m, dtype=np.int64), np.arange(pa.n, dtype=np.int64), indexing="ij")
    return flat[i + j * pa.dense_ld] if pa.dense_colmajor else flat[i * pa.dense_ld + j]


def dense_problem(A, k, scale, rx, ry):
    """(dense ProblemArrays, list ProblemArrays) of the fully observed model QuadLoss(scale) on A with one regularizer descriptor per
    side: the same model as the matrix and as the reference constructor's default lists (every row lists 0..n-1, every column 0..m-1)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    m, n = A.shape
    loss = np.array([(0, 0, float(scale), 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    rxa, rya = np.array([rx], dtype=_capi.REG_DTYPE), np.array([ry], dtype=_capi.REG_DTYPE)
    dense = _capi.ProblemArrays(m, n, k, None, None, None, None, None, None, loss, rxa, rya, dense_A=A, dense_ld=n, dense_colmajor=0)
    lists = _capi.ProblemArrays(m, n, k, np.arange(m + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int32), m), A.reshape(-1).copy(),
                                np.arange(n + 1, dtype=np.int64) * m, np.tile(np.arange(m, dtype=np.int32), n),
                                np.ascontiguousarray(A.T).reshape(-1), loss, rxa, rya)
    return dense, lists


# ---- the launch-shape problems --------------------------------------------------------------------------------------------------
# launch_dense_any (csrc/glrm_dense.hip) takes the 16-wave workgroup when nseg * nsup >= 256 * 256 and pick_sup cuts the opposing
# dimension into ceil(n_other / 32768) super-tiles.  65 573 = 256 * 256 + 37 segments put one half-step on the 16-wave kernel with a
# last workgroup of 37 segments, and, as the opposing dimension of the other half-step, give it three super-tiles of 21 888 vectors,
# the last one holding 21 797 (a multiple of neither 64 nor 16).
BIG, SMALL = 65573, 40
LAUNCH_SHAPES = [(BIG, SMALL, 12), (BIG, SMALL, 32), (BIG, SMALL, 64), (SMALL, BIG, 12), (SMALL, BIG, 64)]
LOSS_SCALE = 2.5


def launch_case(m, n, k, seed=0):
    """A, X0 (k x m), Y0 (k x n), rx, ry of one launch-shape problem: a rank-4 signal plus noise, QuadReg on the long side's factor and
    NonNegConstraint on the short side's (whose start is non-negative, so that the line search decides on finite objectives)."""
    rng = np.random.default_rng(7000 + m + 3 * n + 5 * k + seed)
    A = rng.standard_normal((m, 4)) @ rng.standard_normal((4, n)) / 2.0 + 0.1 * rng.standard_normal((m, n))
    X0, Y0 = rng.standard_normal((k, m)) / np.sqrt(k), rng.standard_normal((k, n)) / np.sqrt(k)
    if m >= n:
        rx, ry, Y0 = QUADREG, NONNEG, np.abs(Y0)
    else:
        rx, ry, X0 = NONNEG, QUADREG, np.abs(X0)
    return A, np.asfortranarray(X0), np.asfortranarray(Y0), rx, ry


def mixed_activity_case(k=32):
    """A 65 573 x 40 problem on which the rows of one X half-step need 8 to 23 trials, 16-segment wave by wave.  The step a row's line
    search accepts depends on where its gradient lies in the spectrum of Y Y', which all rows share, and not on the row's magnitude
    (the model is homogeneous in it).  So Y0 is non-negative with Y0 Y0' diagonal and eigenvalues over three decades (component c on
    column c alone, 7.4 x 10^(-(c % 4) / 2); columns 32..39 of Y0 and of A are zero, so those columns never find a better point),
    A = Xt' Y0, and the start of row i is Xt plus a perturbation along component (i // 16) % k alone: an eigenvector, another one for
    every wave.  Xt, and with it the rows of A and of X0, is scaled by 10^((i // 64) % 4 - 2), four decades."""
    assert k <= SMALL
    m, n = BIG, SMALL
    rng = np.random.default_rng(4)
    Y0 = np.zeros((k, n))
    Y0[np.arange(k), np.arange(k)] = 7.4 * 10.0 ** (-(np.arange(k) % 4) / 2.0)
    i = np.arange(m)
    mag = 10.0 ** ((i // 64) % 4 - 2)
    Xt = rng.standard_normal((k, m)) / np.sqrt(k) * mag
    A = Xt.T @ Y0
    X0 = Xt.copy()
    X0[(i // 16) % k, i] += mag
    return A, np.asfortranarray(X0), np.asfortranarray(Y0), QUADREG, NONNEG


# ---- the half-step in extended precision ----------------------------------------------------------------------------------------

def longdouble_terms(A, X, Y, scale, stride=32):
    """Column losses and both gradients of the fully observed QuadLoss model in numpy longdouble, each with the sum of the absolute
    values of its terms (the scale of its rounding error; fp64 is enough for that).  Every sum over the long dimension is evaluated;
    of the segments of the long side, whose sums have 40 terms, every `stride`-th and the last 37 (longdouble products run at ~1e8
    multiply-adds per second).  Returns (rows, cols, (closs[cols], |.|), (GX[:, rows], |.|), (GY[:, cols], |.|))."""
    ld = np.longdouble
    m, n = A.shape
    pick = lambda c: np.arange(c) if c <= 4096 else np.unique(np.concatenate([np.arange(0, c, stride), np.arange(c - 37, c)]))
    rows, cols = pick(m), pick(n)
    Xl, Yl = X.astype(ld), Y.astype(ld)
    Rc = Xl.T @ Yl[:, cols] - A[:, cols].astype(ld)          # m x |cols|: the columns' sums run over all rows
    Rr = Rc[rows] if len(cols) == n else Xl[:, rows].T @ Yl - A[rows].astype(ld)   # |rows| x n
    closs = ld(scale) * np.sum(Rc * Rc, axis=0)
    GX, GY = ld(2 * scale) * (Yl @ Rr.T), ld(2 * scale) * (Xl @ Rc)
    GXa = 2 * scale * (np.abs(Y) @ np.abs(Rr.astype(np.float64)).T)
    GYa = 2 * scale * (np.abs(X) @ np.abs(Rc.astype(np.float64)))
    return rows, cols, (closs, closs), (GX, GXa), (GY, GYa)
