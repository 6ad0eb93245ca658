"""-m gpu: the persistent cached row sweep (csrc/glrm_cached.hip: regcached_persist_kernel) walks several rows per workgroup and hands the
next row's record -- list AND stored stepsize -- over through LDS a row ahead; its counters are atomic adds.  Every case here runs with
GLRM_HIP_CACHED=1 and compares, bit for bit, X, Y, the objective of every iteration and the trial / accept totals of the X half-steps
  (a) with the same run under GLRM_HIP_CACHED_PERSIST=0 (the one-row-per-workgroup kernel, which loads the stepsize where it is used), and
  (b) with the oracle adding in the order the engine reports: X, Y and the totals equal.  The objective entry point is a separate
      evaluation that the two sides sum in different orders, from equal factors: OBJ_TOL = 1e-10.  A term (u - a)^2 with |u| ~ 1,
      |u - a| ~ 0.1 carries at most 2 * 64 eps * |u| / |u - a| = 1.4e-13 from the order of its 64-term dot product, and a sum of
      n = 1.8e5 non-negative terms at most n eps = 2e-11 from its own order, on either side; a wrong or missing term is far above that.
Shapes: m = 5 003 rows is more than four times the resident grid of 1 024 workgroups, so every workgroup walks at least four rows and the
last round is ragged; n = 257; QuadLoss + NonNeg.  Row lengths come from {0, 1, 7, 8, 9, 16, 17, 63, 100, 104} plus twenty long rows that
go to the gather sweep and bring the `seglist` form of the launch.  At rank 64 (layout 8 x 8) those are 105 .. 300 observations (a row of
more than 257 repeats columns) and the cached rows run the MAXT = 7 kernel; at rank 32 (layout 4 x 8) registers hold rows of up to 208,
so the cached rows are held to <= 64 observations (the MAXT = 4 kernel) and the long ones are 209 .. 300."""
import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
from test_gpu_parity import TOL, hip

pytestmark = pytest.mark.gpu
CACHED = 64
OBJ_TOL = 1e-10
LENGTHS = (0, 1, 7, 8, 9, 16, 17, 63, 100, 104)
N = 257
_problems = {}


def problem(m, k, long_rows=20):
    """Seeded; built once per (m, k) and shared (nothing writes to it)."""
    key = (m, k, long_rows)
    if key in _problems:
        return _problems[key]
    rng = np.random.default_rng(1000 * k + m)
    pool = [l for l in LENGTHS if k == 64 or l <= 64]
    lens = rng.choice(pool, size=m)
    if m >= len(pool):
        lens[: len(pool)] = pool                                    # every length occurs
    else:
        lens[:] = 100
    long_rows = min(long_rows, m // 4)
    where = rng.choice(m, size=long_rows, replace=False)
    lo = 105 if k == 64 else 209
    lens[where] = np.linspace(lo, 300, long_rows).astype(int) if long_rows else []
    I, J = [], []
    for i, l in enumerate(lens):
        cols = rng.permutation(N)[: min(l, N)]
        if l > N:
            cols = np.concatenate([cols, rng.integers(0, N, l - N)])
        I.append(np.full(l, i)); J.append(np.sort(cols))
    I, J = np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)
    # columns of two sizes: a row's curvature is the mean |y|^2 of its columns, so short rows on the large columns need a stepsize below
    # 0.5 and short rows on the small ones do not (test_rejections_shrink_rows_and_rows_give_up)
    X0, Y0 = np.abs(rng.standard_normal((k, m))) / 8.0, np.abs(rng.standard_normal((k, N))) * rng.choice([0.125, 0.5], size=N)
    A = X0.T @ Y0 + 0.1 * rng.standard_normal((m, N))
    g = L.GLRM(A, L.QuadLoss(), L.NonNegConstraint(), L.NonNegConstraint(), k, obs=(I, J), X=X0, Y=Y0)
    _problems[key] = (g.problem_arrays(), np.asfortranarray(X0), np.asfortranarray(Y0), lens)
    return _problems[key]


def iterate(api, pa, X0, Y0, iters, stepsize, min_stepsize, orders=None, rows=None, **create_kw):
    """`iters` times: the X half-step (all rows, or the range `rows`), the Y half-step, the objective.  -> X, Y, objectives, stats, orders"""
    h = api.create(pa, **create_kw)
    try:
        got = None
        if orders is not None:
            for w, o in enumerate(orders):
                O.set_sum_order(h, w, o)
        else:
            assert api.kernel_stats(h)["tiled"] & CACHED
            got = [api.sum_order(h, 0), api.sum_order(h, 1)]
            assert got[0].cached_waves == 2 and got[0].cached_maxlen == (104 if pa.k == 64 else 208), got[0].asdict()
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, stepsize)
        X, Y, objs = np.zeros_like(X0), np.zeros_like(Y0), []
        for _ in range(iters):
            if rows is None:
                api.step_x(h, min_stepsize)
            else:
                api.step_x_range(h, rows[0], rows[1], min_stepsize)
            api.step_y(h, min_stepsize)
            api.get_factors(h, X, Y)
            objs.append(api.objective(h, X, Y))
        st = api.kernel_stats(h)
    finally:
        api.destroy(h)
    return X, Y, np.array(objs), st, got


def three_ways(monkeypatch, pa, X0, Y0, iters=3, stepsize=1.0, min_stepsize=0.01, rows=None):
    """persistent kernel == one-row-per-workgroup kernel == oracle in the engine's order; returns the persistent run's stats"""
    monkeypatch.setenv("GLRM_HIP_CACHED", "1")
    monkeypatch.setenv("GLRM_HIP_CACHED_PERSIST", "1")
    Xp, Yp, op, sp, orders = iterate(hip(), pa, X0, Y0, iters, stepsize, min_stepsize, rows=rows, tiled=1)
    monkeypatch.setenv("GLRM_HIP_CACHED_PERSIST", "0")
    Xr, Yr, orf, sr, _ = iterate(hip(), pa, X0, Y0, iters, stepsize, min_stepsize, rows=rows, tiled=1)
    monkeypatch.setenv("GLRM_HIP_CACHED_PERSIST", "1")
    assert np.array_equal(Xp, Xr), ("X differs from the one-row-per-workgroup kernel", np.flatnonzero(np.any(Xp != Xr, axis=0))[:12])
    assert np.array_equal(Yp, Yr) and np.array_equal(op, orf), (op, orf)
    assert (sp["trials_x"], sp["accepts_x"]) == (sr["trials_x"], sr["accepts_x"]), (sp, sr)
    O.set_threads(O.usable_cores())
    Xc, Yc, oc, sc, _ = iterate(O.oracle_api(), pa, X0, Y0, iters, stepsize, min_stepsize, orders=orders, rows=rows)
    assert np.array_equal(Xp, Xc), ("X differs from the oracle in the engine's order", np.flatnonzero(np.any(Xp != Xc, axis=0))[:12])
    assert np.array_equal(Yp, Yc)
    assert (sp["trials_x"], sp["accepts_x"]) == (sc["trials_x"], sc["accepts_x"]), (sp, sc)
    assert cases.rel_err(op, oc) < OBJ_TOL, (op, oc)
    return sp


@pytest.mark.parametrize("k", [64, 32])
def test_several_rows_per_workgroup(monkeypatch, k):
    """Three iterations: a stored stepsize is read back -- a row ahead of its use -- twice."""
    pa, X0, Y0, lens = problem(5003, k)
    st = three_ways(monkeypatch, pa, X0, Y0)
    assert st["trials_x"] >= st["accepts_x"] > 0


@pytest.mark.parametrize("k", [64, 32])
def test_rejections_shrink_rows_and_rows_give_up(monkeypatch, k):
    pa, X0, Y0, lens = problem(5003, k)
    # first trials at stepsize 1e3 fail: rows shrink several times before they accept
    st = three_ways(monkeypatch, pa, X0, Y0, stepsize=1e3)
    assert st["trials_x"] > st["accepts_x"] > 0, st
    assert st["trials_x"] > 3 * st["accepts_x"], st              # several trials per accepted row
    # min_stepsize = 0.5: rows whose stepsize falls below it give up at 1.1 * min_stepsize without accepting
    st = three_ways(monkeypatch, pa, X0, Y0, stepsize=1e3, min_stepsize=0.5)
    assert 0 < st["accepts_x"] < 3 * int(np.count_nonzero(lens)), (st, "every non-empty row accepted in every iteration")


@pytest.mark.parametrize("m", [1, 1023, 1024, 1025])
def test_edges_of_the_walk(monkeypatch, m):
    """One row; one row per workgroup, and no next row for some or all of them."""
    pa, X0, Y0, lens = problem(m, 64, long_rows=0)
    st = three_ways(monkeypatch, pa, X0, Y0)
    assert st["trials_x"] > 0


def test_row_range_filters_slots_of_the_listed_form(monkeypatch):
    """glrm_hip_step_x_range over [1 000, 3 001) with long rows in the shard: the launch walks the list of short rows and skips the slots
    outside the range (no row, but still a hand-over)."""
    pa, X0, Y0, lens = problem(5003, 64)
    st = three_ways(monkeypatch, pa, X0, Y0, rows=(1000, 3001))
    assert 0 < st["accepts_x"] <= 3 * 2001


def test_fixed_stepsize_path_of_the_sparse_solver(monkeypatch):
    """One fit_sparse iteration: no line search, neither the stepsize nor the counters are touched.  (Stepsize 0.1: the solver keeps an
    iteration only if the objective fell, and on this problem's large columns it does not at the default of 1.)"""
    pa, X0, Y0, lens = problem(5003, 64)
    monkeypatch.setenv("GLRM_HIP_CACHED", "1")
    sp = L.SparseProxGradParams(0.1, max_iter=1)
    outs = []
    for persist in ("1", "0"):
        monkeypatch.setenv("GLRM_HIP_CACHED_PERSIST", persist)
        h = hip().create(pa, tiled=1)
        try:
            assert hip().kernel_stats(h)["tiled"] & CACHED
            X, Y = np.array(X0, order="F"), np.array(Y0, order="F")
            obj, _ = hip().fit_sparse(h, sp, X, Y)
            st = hip().kernel_stats(h)
        finally:
            hip().destroy(h)
        outs.append((np.array(obj), X, Y, st))
    (o1, X1, Y1, s1), (o0, X0_, Y0_, s0) = outs
    assert np.array_equal(o1, o0) and np.array_equal(X1, X0_) and np.array_equal(Y1, Y0_)
    assert (s1["trials_x"], s1["accepts_x"]) == (s0["trials_x"], s0["accepts_x"])
    assert len(o1) == 3 and o1[1] < o1[0] and not np.array_equal(X1, X0)   # the iteration was kept: X1 is the kernel's output
    ho = O.oracle_api().create(pa)
    try:
        Xc, Yc = np.array(X0, order="F"), np.array(Y0, order="F")
        oc, _ = O.oracle_api().fit_sparse(ho, sp, Xc, Yc)
    finally:
        O.oracle_api().destroy(ho)
    assert len(oc) == len(o1) and cases.rel_err(o1, oc) < TOL and cases.fro_err(X1, Xc) < TOL and cases.fro_err(Y1, Yc) < TOL
