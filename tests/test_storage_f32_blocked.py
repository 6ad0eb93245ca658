"""The host reference of the storage = f32 phase-aligned passes (tests/storage_f32_blocked_ref.py) is pinned before anything runs on a device:
without the rounding it is the fp64 family, and the CPU oracle adding in the windowed order an fp64 handle on the family reports
(one walk per super-tile, partial sums in super-tile order: tests/test_sum_order.py::test_windowed_order_of_the_phase_aligned_passes)
must land on the same factors, objectives and trial counts bit for bit over two outer iterations -- at the engine's own tile size, so that
rows and columns cross a super-tile edge.  Once with the uniform QuadLoss model (two observations per step) and once with a loss per column
(the whole batch of G observations per step) over the kinds a host restatement reproduces exactly: Huber, L1 and Hinge."""
import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
import storage_f32_blocked_ref as B
from lowrankmodels.jl_amd import _capi
from test_sum_order import small_problem


def oracle_iterations(pa, X0, Y0, order_r, order_c, iters):
    api = O.oracle_api()
    h = api.create(pa)
    out = []
    try:
        O.set_sum_order(h, 0, order_r)
        O.set_sum_order(h, 1, order_c)
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        for _ in range(iters):
            api.step_x(h, 0.01)
            X1, Y1 = np.zeros_like(X0), np.zeros_like(Y0)
            api.get_factors(h, X1, Y1)
            api.step_y(h, 0.01)
            X2, Y2 = np.zeros_like(X0), np.zeros_like(Y0)
            api.get_factors(h, X2, Y2)
            st = api.kernel_stats(h)
            out.append((X1, Y2, st["trials_x"], st["trials_y"]))
    finally:
        api.destroy(h)
    return out


def per_column_problem(m, n, k, lens, seed, reg):
    """small_problem with a descriptor per column: HuberLoss, L1Loss and HingeLoss in turn (Boolean values under the hinge)."""
    pa, X0, Y0 = small_problem(m, n, k, lens, seed, reg=reg)
    kinds = [L.HuberLoss(1.1, crossover=0.7), L.L1Loss(0.6), L.HingeLoss(1.2)]
    losses = np.array([kinds[f % 3].descriptor() for f in range(n)], dtype=_capi.LOSS_DTYPE)
    hinge_r, hinge_c = pa.colidx % 3 == 2, np.repeat(np.arange(n), np.diff(pa.colptr)) % 3 == 2
    rowvals, colvals = pa.rowvals.copy(), pa.colvals.copy()
    rowvals[hinge_r] = rowvals[hinge_r] > 0
    colvals[hinge_c] = colvals[hinge_c] > 0
    return _capi.ProblemArrays(m, n, k, pa.rowptr, pa.colidx, rowvals, pa.colptr, pa.rowidx, colvals, losses, pa.rx, pa.ry), X0, Y0


@pytest.mark.parametrize("model", ["quad", "per_column"])
def test_without_rounding_the_reference_is_the_oracle_in_the_windowed_order(model):
    """Both dimensions span two one-tile super-tiles (T + 12 vectors), so every list of more than one entry may cross the edge."""
    if model == "quad":
        k, G, R, reg, losses = 64, 8, 8, (B.S.REG_QUAD, 0, 0.3), None
    else:
        k, G, R, reg, losses = 20, 4, 8, (B.S.REG_QUAD, 0, 0.3), True
    T = B.tile_rows(G * R)
    m = n = T + 12
    lens = [0, 1, 2, 9] if model == "quad" else [0, 1, 3, 4, 5, 11]
    if losses:
        pa, X0, Y0 = per_column_problem(m, n, k, lens, 40 + k, reg)
        losses = pa.losses
    else:
        pa, X0, Y0 = small_problem(m, n, k, lens, 40 + k, reg=reg)
    assert np.diff(pa.colptr).max() > G and pa.rowidx.max() >= T and pa.colidx.max() >= T
    o = O.make_sum_order("windowed", G, R, window=T, windows_per_sup=1, batch=G if losses is not None else 2)
    want = oracle_iterations(pa, X0, Y0, o, o, 2)
    got = B.trajectory(pa, X0, Y0, G, R, reg, 2, (1, 1), losses=losses, rounding=False)
    for it, ((X1, Y2, tx, ty), g) in enumerate(zip(want, got)):
        assert np.array_equal(g[0], X1), (it, np.abs(g[0] - X1).max())
        assert np.array_equal(g[1], Y2), (it, np.abs(g[1] - Y2).max())
        assert (g[3], g[4]) == (tx, ty), it
    assert want[-1][2] > 2 * m and want[-1][3] > 2 * n   # some first trial was rejected: the search ran past one round


def test_no_decision_of_the_nine_kinds_problem_sits_near_a_tie():
    """The condition tests/test_gpu_storage_f32_blocked.py states for its comparison of an f32 and an fp64 handle on all nine scalar loss
    kinds: at its seed and stepsize every evaluated trial of one step_x and one step_y differs from J_old by at least 1e-4 relative."""
    pa, X0, Y0, objs = B.nine_kinds_problem(11)
    T = B.tile_rows(8)
    assert pa.m > T and pa.n > T and B.S.is_f32(X0) and B.S.is_f32(Y0) and B.S.is_f32(pa.rowvals)
    assert len({int(d[0]) for d in pa.losses}) == 9
    assert B.least_decision_margin(pa, X0, Y0, objs, stepsize=1.0) >= 1e-4


def test_the_rounding_is_after_the_prox_and_only_there():
    """With the rounding on, the same problem ends on float-representable factors that differ from the fp64 family's by rounding only."""
    k, G, R, reg = 64, 8, 8, (B.S.REG_QUAD, 0, 0.3)
    pa, X0, Y0 = small_problem(40, 30, k, [0, 1, 2, 9], 7, reg=reg)
    f = lambda a: np.asfortranarray(np.asarray(a).astype(np.float32).astype(np.float64))  # noqa: E731
    pa.rowvals[:], pa.colvals[:] = f(pa.rowvals), f(pa.colvals)
    X0, Y0 = f(X0), f(Y0)
    r32 = B.trajectory(pa, X0, Y0, G, R, reg, 1, (1, 1))[0]
    r64 = B.trajectory(pa, X0, Y0, G, R, reg, 1, (1, 1), rounding=False)[0]
    assert B.S.is_f32(r32[0]) and B.S.is_f32(r32[1]) and not B.S.is_f32(r64[0])
    assert np.array_equal(r32[0], f(r64[0]))   # one half-step from the same point: the same unrounded trial points
    assert np.abs(r32[1] - r64[1]).max() < 1e-6
