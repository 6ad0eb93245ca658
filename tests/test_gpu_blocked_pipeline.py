"""-m gpu: the two-observation step of the phase-aligned passes (tiled_pass<..., L2 = true>, uniform QuadLoss, rank 64 and rank 32;
csrc/glrm_tiled.hpp) at the places where a re-scheduling of its gathers can go wrong.  A step takes a batch of G observations as G / 2
pairs; any form of the step that requests a pair's vectors before the pair in front of it is done (the software-pipelined steps of
LABNOTES "Two gather pairs in flight per wave", measured and dropped) has to request them for entries the step will NOT consume -- past
the end of the list, past the end of the super-tile, in a group that sits the step out at the phase gate -- and must leave every
accumulator with exactly the terms it gets today, in the same order.  So every comparison here is np.array_equal: against the oracle
adding in the order the engine reports, against the searching prologue, and across the settings of the phase gate.  The cases hold for
the step as it is and are the check any later variant of it has to pass; what they cannot show is that anything got faster."""
import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
import shapes
from lowrankmodels.jl_amd import _capi
from shapes import Seg
from test_gpu_blocked_gate import force_blocked, shuffle_inside_windows
from test_gpu_sum_order import engine_and_oracle_in_its_order, problem

pytestmark = pytest.mark.gpu
BLOCKED_R, BLOCKED_C = 16, 32
BOTH = BLOCKED_R | BLOCKED_C
FAMILIES = ("windowed", "windowed")
NONNEG = (3, 0, 1.0)
# observations of a listed segment inside ONE super-tile: an odd last pair (1, 3, 7, 9, 15, 17), a batch that ends inside the step (G = 8:
# 1 .. 7, 9, 15, 17; G = 4: 1, 2, 3, 7, 9, 15, 17), a pair without a valid entry behind a consumed one (1, 2, 9 ...), a list that ends exactly at a batch
# boundary (8, 16; G = 4 also 0 mod 4), and no entry at all
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17)


def on_the_family(monkeypatch, tps="1", fill="3", suppos="2"):
    force_blocked(monkeypatch, tps, fill)
    monkeypatch.setenv("GLRM_HIP_BLOCKED_SUPPOS", suppos)
    monkeypatch.delenv("GLRM_HIP_BLOCKED_GATE", raising=False)


def fit_bits(pa, X0, Y0, prm):
    obj, X, Y, st = cases.run_engine(_capi.hip_api(), pa, X0, Y0, prm, tiled=1)
    assert st["tiled"] & BOTH == BOTH, st["tiled"]
    return np.asarray(obj), X, Y, st


def assert_same_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), what
    for key in ("trials_x", "trials_y", "accepts_x", "accepts_y"):
        assert a[3][key] == b[3][key], (what, key, a[3][key], b[3][key])


def params(iters, stepsize=1.0):
    return L.ProxGradParams(stepsize, max_iter=iters, abs_tol=-1e300, rel_tol=-1e300)


@pytest.mark.parametrize("tps,fill", [("1", "3"), ("3", "100")])
@pytest.mark.parametrize("k", [64, 32])
def test_oracle_in_the_engines_order(monkeypatch, k, tps, fill):
    """The C4 recipe, 8 iterations, rows and columns on the family, many launch slices of one-tile super-tiles and one slice of three-tile
    ones: X, Y, every accept / reject decision and the objectives."""
    on_the_family(monkeypatch, tps, fill)
    pa, X0, Y0 = problem(20000, 2000, k, 100, NONNEG, value_model=1)
    engine_and_oracle_in_its_order(pa, X0, Y0, 8, BOTH, FAMILIES, tiled=1)


def boundary_shape(k):
    kp, _ = shapes.padded_rank(k)
    T = shapes.tile_rows(kp)
    m, n = 3 * T + 5, 2 * T + 3
    segs = [Seg(f"c{n_}", "col", i, n_, "window", 1) for i, n_ in enumerate(LENGTHS)]
    segs += [Seg(f"r{n_}", "row", i, n_, "window", 1) for i, n_ in enumerate(LENGTHS)]
    # the same lengths split over two neighbouring super-tiles: the batch that holds the last entries of one also holds the first of the next
    segs += [Seg(f"cs{n_}", "col", 20 + i, n_, "straddle", T) for i, n_ in enumerate(LENGTHS)]
    return shapes.build(m, n, k, segs, fill=4, reg="nonneg", seed=300 + k), T


@pytest.mark.parametrize("k", [64, 32])
def test_pair_and_batch_boundaries(monkeypatch, k):
    """Columns and rows with exactly 0, 1, 2, 3, 7, 8, 9, 15, 16 and 17 observations in a super-tile (and none in the others): the start table
    against the searching prologue, and both against the oracle."""
    sh, T = boundary_shape(k)
    for name, n_ in zip((f"c{x}" for x in LENGTHS), LENGTHS):
        rows = sh.indices("col", sh.seg(name).index)
        assert len(rows) == n_ and all(T <= r < 2 * T for r in rows), (name, rows)
    on_the_family(monkeypatch, suppos="2")
    table = fit_bits(sh.pa, sh.X0, sh.Y0, params(6))
    engine_and_oracle_in_its_order(sh.pa, sh.X0, sh.Y0, 6, BOTH, FAMILIES, tiled=1)
    on_the_family(monkeypatch, suppos="0")
    assert_same_bits(fit_bits(sh.pa, sh.X0, sh.Y0, params(6)), table, "searching prologue against the start table")


@pytest.mark.parametrize("k", [64, 32])
def test_super_tile_edges_under_every_gate(monkeypatch, k):
    """m = 2 T + 7: a partial last super-tile.  One column ends in the last row of a super-tile, another begins in the first row of the
    next, others hold both (the batch then holds a row at or beyond the end of the super-tile being walked) or the last row of X; the
    gate off, at one row and at its default give the same bits, and they are the oracle's."""
    kp, G = shapes.padded_rank(k)
    T = shapes.tile_rows(kp)
    m, n = 2 * T + 7, T + 9
    segs = [Seg("last_of_sup0", "col", 0, 1, "range", (T - 1, T)), Seg("first_of_sup1", "col", 1, 1, "range", (T, T + 1)),
            Seg("both", "col", 2, 2, "straddle", T), Seg("across", "col", 3, G + 3, "straddle", T), Seg("across2", "col", 4, G + 5, "straddle", 2 * T),
            Seg("last_row", "col", 5, 1, "range", (m - 1, m)), Seg("tail", "col", 6, G + 1, "range", (m - G - 1, m)),
            Seg("last_col", "row", 0, 1, "range", (n - 1, n)), Seg("row_across", "row", 1, G + 3, "straddle", T)]
    sh = shapes.build(m, n, k, segs, fill=4, reg="nonneg", seed=400 + k)
    assert list(sh.indices("col", 0)) == [T - 1] and list(sh.indices("col", 1)) == [T] and list(sh.indices("col", 2)) == [T - 1, T]
    assert list(sh.indices("col", 5)) == [m - 1] and sh.indices("col", 6)[-1] == m - 1 and list(sh.indices("row", 0)) == [n - 1]
    on_the_family(monkeypatch)
    runs = {}
    for gate in (None, "0", "1"):
        if gate is not None:
            monkeypatch.setenv("GLRM_HIP_BLOCKED_GATE", gate)
        runs[gate] = fit_bits(sh.pa, sh.X0, sh.Y0, params(6))
    assert_same_bits(runs["0"], runs[None], "gate off against the default")
    assert_same_bits(runs["1"], runs[None], "one-row gate against the default")
    monkeypatch.delenv("GLRM_HIP_BLOCKED_GATE")
    engine_and_oracle_in_its_order(sh.pa, sh.X0, sh.Y0, 6, BOTH, FAMILIES, tiled=1)


@pytest.mark.parametrize("k", [64, 32])
def test_one_row_gate_on_lists_shuffled_inside_windows(monkeypatch, k):
    """Lists in tile order only, the tightest gate: almost every group sits almost every step out, with a batch it has not consumed, and
    a lane may hold a smaller row than its group's next one.  Same bits as with the gate off, and the walk ends."""
    m, n, q = 4000, 400, 100
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(m, n, k, q, value_model=1)
    rng = np.random.default_rng(13)
    colidx2, rowvals2 = shuffle_inside_windows(rowptr, colidx, rowvals, rng)
    rowidx2, colvals2 = shuffle_inside_windows(colptr, rowidx, colvals, rng)
    assert not np.array_equal(rowidx2, rowidx) and not np.array_equal(colidx2, colidx)
    one = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([NONNEG], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx2, rowvals2, colptr, rowidx2, colvals2, one, reg, reg)
    X0, Y0 = np.asfortranarray(np.abs(X0) / 8.0), np.asfortranarray(np.abs(Y0) / 8.0)
    on_the_family(monkeypatch, "1", "5")
    monkeypatch.setenv("GLRM_HIP_BLOCKED_GATE", "1")
    tight = fit_bits(pa, X0, Y0, params(6))
    monkeypatch.setenv("GLRM_HIP_BLOCKED_GATE", "0")
    assert_same_bits(fit_bits(pa, X0, Y0, params(6)), tight, "gate off against the one-row gate")
    monkeypatch.setenv("GLRM_HIP_BLOCKED_GATE", "1")
    engine_and_oracle_in_its_order(pa, X0, Y0, 6, BOTH, FAMILIES, tiled=1)


@pytest.mark.parametrize("k", [64, 32])
def test_trial_rounds_on_active_lists(monkeypatch, k):
    """A step size for which many columns reject their first trial: the trial pass then runs again over the list of still-searching
    columns (slots permuted, inactive groups beside walking ones in a wave).  The oracle must see rejected trials, or the case is void."""
    on_the_family(monkeypatch, "1", "3")
    pa, X0, Y0 = problem(6000, 1200, k, 60, (1, 0, 1.0), value_model=0)
    prm = params(4, stepsize=40.0)
    oapi = O.oracle_api()
    O.set_threads(O.usable_cores())
    ho = oapi.create(pa)
    try:
        Xr, Yr = X0.copy(order="F"), Y0.copy(order="F")
        oapi.fit(ho, prm, Xr, Yr)
        st_ref = oapi.kernel_stats(ho)
    finally:
        oapi.destroy(ho)
    assert st_ref["trials_y"] > st_ref["accepts_y"] and st_ref["trials_x"] > st_ref["accepts_x"], st_ref
    api = _capi.hip_api()
    h = api.create(pa, tiled=1)
    try:
        assert api.kernel_stats(h)["tiled"] & BOTH == BOTH
        orders = [api.sum_order(h, 0), api.sum_order(h, 1)]
        Xg, Yg = X0.copy(order="F"), Y0.copy(order="F")
        og, _ = api.fit(h, prm, Xg, Yg)
        st_g = api.kernel_stats(h)
    finally:
        api.destroy(h)
    ho = oapi.create(pa)
    try:
        for w, o in enumerate(orders):
            O.set_sum_order(ho, w, o)
        Xc, Yc = X0.copy(order="F"), Y0.copy(order="F")
        oc, _ = oapi.fit(ho, prm, Xc, Yc)
        st_c = oapi.kernel_stats(ho)
    finally:
        oapi.destroy(ho)
    assert st_c["trials_y"] > st_c["accepts_y"], st_c
    assert np.array_equal(Xg, Xc) and np.array_equal(Yg, Yc)
    for key in ("trials_x", "trials_y", "accepts_x", "accepts_y"):
        assert st_g[key] == st_c[key], (key, st_g[key], st_c[key])
    assert cases.rel_err(og[1:], oc[1:]) < 1e-13  # the recorded objective: only the final sum over columns differs (test_gpu_sum_order)
