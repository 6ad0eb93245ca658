"""-m gpu: the super-tile start table of the phase-aligned passes (GLRM_HIP_BLOCKED_SUPPOS; csrc/glrm_blocked.hip, tiled_col_pass_kernel<...,
L2 = true> in csrc/glrm_tiled.hpp).  The table holds what the pass kernel's search finds at the start of every launch, so nothing may move:
objectives, factors, trial and accept counts and the reported summation order are compared with np.array_equal, no tolerance -- on whole
fits, on the X half-step in ragged glrm_hip_step_x_range chunks and on glrm_hip_step_y_arrival with the blocks announced last to first.

The per-XCD pacing of the waves of a launch that was built and measured with the table (GLRM_HIP_BLOCKED_XGATE) lost at every setting and
was removed with its tests (LABNOTES "Round 9"); this file keeps the name the work was planned under.

What these tests cannot show is that the table is faster than the search: that is what the C4 A/B runs and kernel traces under
profiles/r09_* are for.  That the table is built where expected is read from the family's trace line (GLRM_HIP_BLOCKED_TRACE)."""
import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
import shapes
from lowrankmodels.jl_amd import _capi, synth
from test_gpu_blocked_gate import c4_recipe, force_blocked, shuffle_inside_windows

pytestmark = pytest.mark.gpu
BLOCKED = 16 | 32
KNOBS = ("GLRM_HIP_BLOCKED_SUPPOS",)


def set_knobs(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)


def run_under(monkeypatch, envs, pa, X0, Y0, params, **create_kw):
    api = _capi.hip_api()
    out = []
    for env in envs:
        set_knobs(monkeypatch, env)
        obj, X, Y, st = cases.run_engine(api, pa, X0, Y0, params, **create_kw)
        assert st["tiled"] & BLOCKED == BLOCKED, (env, st["tiled"])
        h = api.create(pa, **create_kw)
        try:
            order = [api.sum_order(h, v).asdict() for v in (0, 1)]
        finally:
            api.destroy(h)
        out.append((env, np.asarray(obj), X, Y, st, order))
    return out


def assert_same_bits(runs):
    _, obj0, X0, Y0, st0, order0 = runs[0]
    for env, obj, X, Y, st, order in runs[1:]:
        assert np.array_equal(obj, obj0), (env, obj, obj0)
        assert np.array_equal(X, X0) and np.array_equal(Y, Y0), env
        for key in ("trials_x", "trials_y", "accepts_x", "accepts_y"):
            assert st[key] == st0[key], (env, key, st[key], st0[key])
        assert order == order0, (env, order, order0)


def table_envs(on):
    return ({"GLRM_HIP_BLOCKED_SUPPOS": "0"}, {"GLRM_HIP_BLOCKED_SUPPOS": on})


def assert_table_built(capfd, views=2):
    """the second of the two runs built the table of both views (two handles each: the fit and the sum_order query)"""
    err = capfd.readouterr().err
    assert err.count("start table off") == 2 * views and err.count("start table built") == 2 * views, err


def loss_per_column(k):
    m, n, q = 2500, 2000, 100
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(m, n, k, q, value_model=0, loss_mix=1)
    kinds = [L.QuadLoss().descriptor(), L.LogisticLoss().descriptor(), L.OrdinalHingeLoss(1, 5).descriptor()]
    losses = np.array([kinds[f % 3] for f in range(n)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([(1, 0, 1.0)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx, rowvals, colptr, rowidx, colvals, losses, reg, reg)
    return pa, np.asfortranarray(0.3 * X0), np.asfortranarray(0.3 * Y0)


def power_law():
    m, n, k = 30000, 3000, 32
    w = synth.ZipfWorkload(m, n, k, 3_000_000, s_rows=0.8, s_cols=0.8, seed=5, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0), chunk=1 << 20)
    pa = w.host_problem()
    X0, Y0 = w.init_factors(k)
    X0, Y0 = X0.numpy().reshape(m, k).T, Y0.numpy().reshape(n, k).T
    return pa, np.asfortranarray(np.abs(X0) / k ** 0.5), np.asfortranarray(np.abs(Y0) / k ** 0.5)


C4_SHAPES = [(64, "1", "3"), (64, "3", "100"), (32, "2", "7")]


# ------------------------------------------------------------------------------------------------ 1. table against search

@pytest.mark.parametrize("k,tps,fill", C4_SHAPES)
def test_table_gives_the_bits_of_the_search_on_the_c4_recipe(monkeypatch, capfd, k, tps, fill):
    """42 super-tiles x many slices, three-tile super-tiles at full residency, the four-lane layout."""
    force_blocked(monkeypatch, tps, fill)
    monkeypatch.setenv("GLRM_HIP_BLOCKED_TRACE", "1")
    pa, X0, Y0 = c4_recipe(12000, 1500, 100, k)
    assert_same_bits(run_under(monkeypatch, table_envs("1"), pa, X0, Y0, L.ProxGradParams(max_iter=8), tiled=1))
    assert_table_built(capfd)


def test_table_gives_the_bits_of_the_search_with_a_loss_per_column(monkeypatch, capfd):
    force_blocked(monkeypatch, "1", "5")
    monkeypatch.setenv("GLRM_HIP_BLOCKED_TRACE", "1")
    pa, X0, Y0 = loss_per_column(64)
    assert_same_bits(run_under(monkeypatch, table_envs("1"), pa, X0, Y0, L.ProxGradParams(max_iter=6), tiled=1))
    assert_table_built(capfd)


def test_table_gives_the_bits_of_the_search_on_a_power_law_omega(monkeypatch, capfd):
    """Zipf degrees: the passes hand the columns out longest first (segperm) and the longest run on the gather sweep beside them.  The
    table is indexed by segment, not by slot."""
    force_blocked(monkeypatch, "2", "5")
    monkeypatch.setenv("GLRM_HIP_BLOCKED_TRACE", "1")
    pa, X0, Y0 = power_law()
    assert_same_bits(run_under(monkeypatch, table_envs("1"), pa, X0, Y0, L.ProxGradParams(max_iter=5, abs_tol=0.0, rel_tol=-1.0)))
    assert_table_built(capfd)


def test_table_gives_the_bits_of_the_search_on_lists_in_tile_order_only(monkeypatch, capfd):
    """Lists shuffled inside 16-row windows are not sorted, so a binary search's answer is not "the first entry >= key" by itself: the
    table is built with the kernel's own search and holds exactly what that finds."""
    force_blocked(monkeypatch, "1", "5")
    monkeypatch.setenv("GLRM_HIP_BLOCKED_TRACE", "1")
    m, n, q, k = 4000, 400, 100, 64
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(m, n, k, q, value_model=1)
    rng = np.random.default_rng(11)
    colidx2, rowvals2 = shuffle_inside_windows(rowptr, colidx, rowvals, rng)
    rowidx2, colvals2 = shuffle_inside_windows(colptr, rowidx, colvals, rng)
    assert not np.array_equal(rowidx2, rowidx) and not np.array_equal(colidx2, colidx)
    one = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([(3, 0, 1.0)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx2, rowvals2, colptr, rowidx2, colvals2, one, reg, reg)
    runs = run_under(monkeypatch, table_envs("1"), pa, np.asfortranarray(np.abs(X0) / 8.0), np.asfortranarray(np.abs(Y0) / 8.0), L.ProxGradParams(max_iter=6), tiled=1)
    assert_same_bits(runs)
    assert_table_built(capfd)


def test_table_gives_the_bits_of_the_search_on_explicit_shapes(monkeypatch, capfd):
    """Columns with no observation, with all of them in one super-tile, all in the last (partial) super-tile, on every row of a
    super-tile (its first and its last included), and with adjacent duplicates; one tile unit per super-tile.  The shape is tiny, so the
    table is forced (2): at 1 it would exceed 1/16 of the lists and the search would stay."""
    force_blocked(monkeypatch, "1", "3")
    monkeypatch.setenv("GLRM_HIP_BLOCKED_TRACE", "1")
    k = 64
    T = shapes.tile_rows(64)
    m, n = 3 * T + 100, 48
    segs = [shapes.Seg("empty", "col", 3, 0),
            shapes.Seg("one_sup", "col", 7, 40, "window", 1),
            shapes.Seg("last_partial", "col", 12, 30, "last_tile"),
            shapes.Seg("edges", "col", 20, T, "range", (T, 2 * T)),
            shapes.Seg("dups", "col", 33, 41, "dups"),
            shapes.Seg("uniform", "col", 40, 200)]
    sh = shapes.build(m, n, k, segs, fill=2, reg="nonneg")
    rows = sh.indices("col", 20)
    assert len(sh.indices("col", 3)) == 0 and rows[0] == T and rows[-1] == 2 * T - 1 and sh.indices("col", 12).min() >= 3 * T
    d = sh.indices("col", 33)
    assert (d[1:] == d[:-1]).any()
    # at 1 the condition keeps the search on this shape
    set_knobs(monkeypatch, {"GLRM_HIP_BLOCKED_SUPPOS": "1"})
    cases.run_engine(_capi.hip_api(), sh.pa, sh.X0, sh.Y0, L.ProxGradParams(max_iter=1), tiled=1)
    assert "over 1/16 of the lists" in capfd.readouterr().err
    assert_same_bits(run_under(monkeypatch, table_envs("2"), sh.pa, sh.X0, sh.Y0, L.ProxGradParams(max_iter=6), tiled=1))
    assert_table_built(capfd)


# ------------------------------------------------------------------------------------------------ 2. sub-ranges and arrival order

SEARCH, TABLE = {"GLRM_HIP_BLOCKED_SUPPOS": "0"}, {"GLRM_HIP_BLOCKED_SUPPOS": "2"}


def test_row_chunks_give_the_bits_of_the_whole_half_step(monkeypatch):
    """glrm_hip_step_x_range in three ragged chunks: the table is bound at the chunk's first row."""
    force_blocked(monkeypatch, "1", "3")
    pa, X0, Y0 = c4_recipe(6000, 1500, 100, 64)
    api = _capi.hip_api()
    res = []
    for env, chunks in ((SEARCH, None), (TABLE, None), (TABLE, [(0, 1001), (1001, 4099), (4099, 6000)])):
        set_knobs(monkeypatch, env)
        h = api.create(pa, tiled=1)
        try:
            assert api.kernel_stats(h)["tiled"] & BLOCKED == BLOCKED
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, 1.0)
            for _ in range(3):
                if chunks is None:
                    api.step_x(h, 0.01)
                else:
                    for b, e in chunks:
                        api.step_x_range(h, b, e, 0.01)
                api.step_y(h, 0.01)
            X, Y = np.zeros_like(X0), np.zeros_like(Y0)
            api.get_factors(h, X, Y)
            st = api.kernel_stats(h)
        finally:
            api.destroy(h)
        res.append((X, Y, [st[key] for key in ("trials_x", "trials_y", "accepts_x", "accepts_y")]))
    for X, Y, counts in res[1:]:
        assert np.array_equal(X, res[0][0]) and np.array_equal(Y, res[0][1]) and counts == res[0][2]


def test_reversed_arrival_order_gives_the_bits_of_step_y(monkeypatch):
    """glrm_hip_step_y_arrival with the blocks announced last to first: the super-tiles are launched in that order, each launch
    reading its own column of the table."""
    import torch
    force_blocked(monkeypatch, "1", "3")
    pa, X0, Y0 = c4_recipe(6000, 600, 100, 64)
    api = _capi.hip_api()
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for env, arrival in ((SEARCH, False), (TABLE, False), (TABLE, True)):
        set_knobs(monkeypatch, env)
        h = api.create(pa, stream=stream)
        try:
            assert api.kernel_stats(h)["tiled"] & 32
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, 1.0)
            for _ in range(3):
                api.step_x(h, 0.01)
                if arrival:
                    blocks, keep = [], []
                    for lo in range(5250, -1, -750):  # the last rows of X first
                        ev = torch.cuda.Event()
                        ev.record()
                        keep.append(ev)
                        blocks.append((lo, lo + 750, ev.cuda_event))
                    api.step_y_arrival(h, 0.01, blocks)
                else:
                    api.step_y(h, 0.01)
            X, Y = np.zeros_like(X0), np.zeros_like(Y0)
            api.get_factors(h, X, Y)
            st = api.kernel_stats(h)
        finally:
            api.destroy(h)
        res.append((X, Y, [st[key] for key in ("trials_x", "trials_y", "accepts_x", "accepts_y")]))
    for X, Y, counts in res[1:]:
        assert np.array_equal(X, res[0][0]) and np.array_equal(Y, res[0][1]) and counts == res[0][2]
