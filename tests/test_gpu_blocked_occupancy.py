"""-m gpu: the phase-aligned passes of the uniform-QuadLoss model at rank 64 and 32 address an observation's vector by a 32-bit byte
offset from the first row of its super-tile, and their gradient pass is built for 4 waves per SIMD (tiled_pass<..., L2 = true> and
pass_waves_per_simd in csrc/glrm_tiled.hpp), so a launch covers a larger slice of the columns.  Neither may move a bit: every comparison here is np.array_equal -- against the CPU oracle
adding in the engine's reported order, against the searching prologue and the gate settings on rows at the edges of a super-tile,
beyond 4 GiB of opposing factor (where a 32-bit offset taken from the factor's start would wrap), and on sub-ranges and arrival order.

What these tests cannot show is that the kernels are faster: that is what the C4 A/B runs and traces under profiles/r13_* are for."""
import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
import shapes
from lowrankmodels.jl_amd import _capi
from test_gpu_blocked_gate import c4_recipe, force_blocked, shuffle_inside_windows
from test_gpu_sum_order import engine_and_oracle_in_its_order, problem

pytestmark = pytest.mark.gpu
BLOCKED_R, BLOCKED_C = 16, 32
BLOCKED = BLOCKED_R | BLOCKED_C
COUNTS = ("trials_x", "trials_y", "accepts_x", "accepts_y")


# ------------------------------------------------------------------------------------------------ 1. the oracle in the engine's order

@pytest.mark.parametrize("k,tps,fill", [(64, "1", "3"), (64, "3", "100"), (32, "1", "3"), (32, "3", "100"), (128, "1", "3")])
def test_engine_lands_on_the_oracle_in_its_order(monkeypatch, k, tps, fill):
    """X, Y and the trial / accept totals bit for bit over 8 iterations.  ("1", "3"): many super-tiles whose first row is not row 0 and many
    launch slices; ("3", "100"): slices of the full residency.  Rank 128 runs the kernels that kept their launch bound."""
    force_blocked(monkeypatch, tps, fill)
    pa, X0, Y0 = problem(20000, 2000, k, 100, (3, 0, 1.0), value_model=1)
    engine_and_oracle_in_its_order(pa, X0, Y0, 8, BLOCKED, ("windowed", "windowed"), tiled=1)


# ------------------------------------------------------------------------------------------------ 2. rows at the edges of a super-tile

def fits_under(monkeypatch, envs, pa, X0, Y0, iters):
    api = _capi.hip_api()
    out = []
    for env in envs:
        for key in ("GLRM_HIP_BLOCKED_SUPPOS", "GLRM_HIP_BLOCKED_GATE"):
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        obj, X, Y, st = cases.run_engine(api, pa, X0, Y0, L.ProxGradParams(max_iter=iters), tiled=1)
        assert st["tiled"] & BLOCKED == BLOCKED, (env, st["tiled"])
        out.append((env, np.asarray(obj), X, Y, [st[key] for key in COUNTS]))
    return out


def assert_same_bits(runs):
    _, obj0, X0, Y0, counts0 = runs[0]
    for env, obj, X, Y, counts in runs[1:]:
        assert np.array_equal(obj, obj0), (env, obj, obj0)
        assert np.array_equal(X, X0) and np.array_equal(Y, Y0), env
        assert counts == counts0, (env, counts, counts0)


# the table (forced: the shapes are tiny) at the default gate, the searching prologue, the gate off and at its tightest
EDGE_ENVS = ({"GLRM_HIP_BLOCKED_SUPPOS": "2"}, {"GLRM_HIP_BLOCKED_SUPPOS": "0"}, {"GLRM_HIP_BLOCKED_SUPPOS": "2", "GLRM_HIP_BLOCKED_GATE": "0"},
             {"GLRM_HIP_BLOCKED_SUPPOS": "2", "GLRM_HIP_BLOCKED_GATE": "1"})


def test_rows_at_the_edges_of_a_super_tile(monkeypatch):
    """Columns with no observation, all in one super-tile, all in the last (partial) super-tile, on every row of a super-tile (offset 0 and
    the last offset of it) and with adjacent duplicates; one tile unit per super-tile."""
    force_blocked(monkeypatch, "1", "3")
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
    assert_same_bits(fits_under(monkeypatch, EDGE_ENVS, sh.pa, sh.X0, sh.Y0, 6))


@pytest.mark.parametrize("k", [32, 64])
def test_lists_shuffled_inside_sixteen_row_windows(monkeypatch, k):
    """Lists in tile order only: a lane of a group may hold a smaller row than the group's next observation, but never one below the
    super-tile's first row (a super-tile starts on a multiple of 16 rows)."""
    force_blocked(monkeypatch, "1", "5")
    m, n, q = 4000, 400, 100
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(m, n, k, q, value_model=1)
    rng = np.random.default_rng(11)
    colidx2, rowvals2 = shuffle_inside_windows(rowptr, colidx, rowvals, rng)
    rowidx2, colvals2 = shuffle_inside_windows(colptr, rowidx, colvals, rng)
    assert not np.array_equal(rowidx2, rowidx) and not np.array_equal(colidx2, colidx)
    one = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([(3, 0, 1.0)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, colidx2, rowvals2, colptr, rowidx2, colvals2, one, reg, reg)
    assert_same_bits(fits_under(monkeypatch, EDGE_ENVS, pa, np.asfortranarray(np.abs(X0) / 8.0), np.asfortranarray(np.abs(Y0) / 8.0), 6))


# ------------------------------------------------------------------------------------------------ 3. beyond 4 GiB of factor

def test_rows_beyond_four_gib_of_the_opposing_factor(monkeypatch):
    """m = 2^23 + 600 rows at rank 64: X is 4.3 GB and byte 2^32 of it is the start of row 2^23.  16 columns of 40 observations, half of
    them in the first super-tile and half in the rows 2^23 - 300 .. 2^23 + 599 (one super-tile at the default size, which starts below
    byte 2^32 and ends beyond it).  Two iterations; the column view on the passes, the row view on the gather sweep.

    Cut for time: of X only the rows that hold an observation are compared (and 1 000 rows that hold none, which must stay zero); the
    oracle runs once, in the engine's order."""
    k, n, per = 64, 16, 20
    m = (1 << 23) + 600
    monkeypatch.setenv("GLRM_HIP_BLOCKED", "2")
    monkeypatch.setenv("GLRM_HIP_CACHED", "0")
    for key in ("GLRM_HIP_BLOCKED_TPS", "GLRM_HIP_BLOCKED_FILL", "GLRM_HIP_BLOCKED_GATE", "GLRM_HIP_BLOCKED_SUPPOS"):
        monkeypatch.delenv(key, raising=False)
    rng = np.random.default_rng(7)
    T = shapes.tile_rows(64)
    rows_per_sup = (128 * 1024 * 1024 // (T * k * 8)) * T
    assert ((1 << 23) - 300) // rows_per_sup == ((1 << 23) + 599) // rows_per_sup and rows_per_sup * k * 8 < 1 << 32
    I, J = [], []
    for f in range(n):
        low = np.sort(rng.choice(rows_per_sup, per, replace=False))
        high = np.sort(rng.choice(900, per, replace=False)) + (1 << 23) - 300
        if f == 0:  # the first and the last row of the factor's tail, and the rows on either side of byte 2^32
            low[0], low[-1] = 0, rows_per_sup - 1
            high[0], high[-1] = (1 << 23) - 300, m - 1
            high[per // 2 - 1], high[per // 2] = (1 << 23) - 1, 1 << 23
            high = np.unique(high)
        I.append(np.concatenate([low, high]))
        J.append(np.full(len(I[-1]), f, np.int64))
    I, J = np.concatenate(I), np.concatenate(J)
    vals = rng.standard_normal(len(I))
    o_r, o_c = np.lexsort((J, I)), np.lexsort((I, J))
    rowptr = np.zeros(m + 1, np.int64)
    np.add.at(rowptr, I + 1, 1)
    rowptr = np.cumsum(rowptr)
    colptr = np.zeros(n + 1, np.int64)
    np.add.at(colptr, J + 1, 1)
    colptr = np.cumsum(colptr)
    one = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    reg = np.array([(3, 0, 1.0)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, np.ascontiguousarray(J[o_r], dtype=np.int32), np.ascontiguousarray(vals[o_r]), colptr,
                             np.ascontiguousarray(I[o_c], dtype=np.int32), np.ascontiguousarray(vals[o_c]), one, reg, reg)
    touched = np.unique(I)
    assert touched.max() == m - 1 and (touched >= 1 << 23).sum() > 100 and (touched < 1 << 23).sum() > 100
    untouched = np.setdiff1d(np.arange((1 << 23) - 500, (1 << 23) + 500), touched)
    X0 = np.zeros((k, m), order="F")
    X0[:, touched] = np.abs(rng.standard_normal((k, len(touched)))) / 8.0
    Y0 = np.asfortranarray(np.abs(rng.standard_normal((k, n))) / 8.0)
    prm = L.ProxGradParams(max_iter=2, abs_tol=-1e300, rel_tol=-1e300)

    api, oapi = _capi.hip_api(), O.oracle_api()
    h = api.create(pa, tiled=1)
    try:
        flags = api.kernel_stats(h)["tiled"]
        assert flags & BLOCKED_C and not flags & BLOCKED_R, flags
        orders = [api.sum_order(h, 0), api.sum_order(h, 1)]
        assert orders[1].asdict()["family_name"] == "windowed"
        Xg, Yg = X0.copy(order="F"), Y0.copy(order="F")
        api.fit(h, prm, Xg, Yg)
        st_g = api.kernel_stats(h)
    finally:
        api.destroy(h)
    Xg_t, Xg_u = Xg[:, touched].copy(), Xg[:, untouched].copy()
    del Xg
    O.set_threads(O.usable_cores())
    ho = oapi.create(pa)
    try:
        for w, o in enumerate(orders):
            O.set_sum_order(ho, w, o)
        Xc, Yc = X0, Y0.copy(order="F")  # X0 is not needed again
        oapi.fit(ho, prm, Xc, Yc)
        st_c = oapi.kernel_stats(ho)
    finally:
        oapi.destroy(ho)
    assert np.array_equal(Xg_t, Xc[:, touched]), np.abs(Xg_t - Xc[:, touched]).max()
    assert not Xg_u.any() and not Xc[:, untouched].any()
    assert np.array_equal(Yg, Yc), np.abs(Yg - Yc).max()
    assert not np.array_equal(Yg, Y0)
    for key in COUNTS:
        assert st_g[key] == st_c[key], (key, st_g[key], st_c[key])

    # a super-tile that spans the whole factor cannot be addressed by 32-bit offsets: refused at create, by name
    monkeypatch.setenv("GLRM_HIP_BLOCKED_TPS", str((m + T - 1) // T))
    with pytest.raises(_capi.GLRMError) as err:
        api.destroy(api.create(pa, tiled=1))
    assert err.value.code == _capi.ERR_UNSUPPORTED and "GLRM_HIP_BLOCKED_TPS" in err.value.message, err.value


# ------------------------------------------------------------------------------------------------ 4. sub-ranges and arrival order

def half_steps(api, pa, X0, Y0, step_x, step_y, **create_kw):
    h = api.create(pa, **create_kw)
    try:
        assert api.kernel_stats(h)["tiled"] & BLOCKED == BLOCKED
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, 1.0)
        for _ in range(3):
            step_x(h)
            step_y(h)
        X, Y = np.zeros_like(X0), np.zeros_like(Y0)
        api.get_factors(h, X, Y)
        st = api.kernel_stats(h)
    finally:
        api.destroy(h)
    return X, Y, [st[key] for key in COUNTS]


def test_row_chunks_give_the_bits_of_the_whole_half_step(monkeypatch):
    """glrm_hip_step_x_range in three ragged chunks at rank 64."""
    force_blocked(monkeypatch, "1", "3")
    pa, X0, Y0 = c4_recipe(6000, 1500, 100, 64)
    api = _capi.hip_api()

    def chunked(h):
        for b, e in ((0, 1001), (1001, 4099), (4099, 6000)):
            api.step_x_range(h, b, e, 0.01)

    whole = half_steps(api, pa, X0, Y0, lambda h: api.step_x(h, 0.01), lambda h: api.step_y(h, 0.01), tiled=1)
    parts = half_steps(api, pa, X0, Y0, chunked, lambda h: api.step_y(h, 0.01), tiled=1)
    assert np.array_equal(parts[0], whole[0]) and np.array_equal(parts[1], whole[1]) and parts[2] == whole[2]


def with_a_full_column(pa, j):
    """pa with column j observing every row (the entries it lacked get the value 0.5)."""
    I, J, V = np.repeat(np.arange(pa.m), np.diff(pa.rowptr)), pa.colidx.astype(np.int64), pa.rowvals
    new = np.setdiff1d(np.arange(pa.m), I[J == j])
    I, J, V = np.concatenate([I, new]), np.concatenate([J, np.full(len(new), j)]), np.concatenate([V, np.full(len(new), 0.5)])
    o_r, o_c = np.lexsort((J, I)), np.lexsort((I, J))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=pa.m))]).astype(np.int64)
    colptr = np.concatenate([[0], np.cumsum(np.bincount(J, minlength=pa.n))]).astype(np.int64)
    return _capi.ProblemArrays(pa.m, pa.n, pa.k, rowptr, np.ascontiguousarray(J[o_r], dtype=np.int32), np.ascontiguousarray(V[o_r]), colptr,
                               np.ascontiguousarray(I[o_c], dtype=np.int32), np.ascontiguousarray(V[o_c]), pa.losses, pa.rx, pa.ry)


def reversed_arrival(monkeypatch, long_column):
    import torch
    force_blocked(monkeypatch, "1", "3")
    pa, X0, Y0 = c4_recipe(6000, 600, 100, 64)
    if long_column:
        pa = with_a_full_column(pa, 17)
    api = _capi.hip_api()
    stream = torch.cuda.current_stream().cuda_stream
    h = api.create(pa, stream=stream)
    try:  # does a column leave the passes?  (every column from glrm_sum_order.long_from observations on)
        assert (np.diff(pa.colptr).max() >= api.sum_order(h, 1).asdict()["long_from"]) == long_column
    finally:
        api.destroy(h)

    def arrival(h):
        blocks, keep = [], []
        for lo in range(5250, -1, -750):  # the last rows of X first
            ev = torch.cuda.Event()
            ev.record()
            keep.append(ev)
            blocks.append((lo, lo + 750, ev.cuda_event))
        api.step_y_arrival(h, 0.01, blocks)

    plain = half_steps(api, pa, X0, Y0, lambda h: api.step_x(h, 0.01), lambda h: api.step_y(h, 0.01), stream=stream)
    late = half_steps(api, pa, X0, Y0, lambda h: api.step_x(h, 0.01), arrival, stream=stream)
    assert np.array_equal(late[0], plain[0]) and np.array_equal(late[1], plain[1]) and late[2] == plain[2]


def test_reversed_arrival_order_gives_the_bits_of_step_y(monkeypatch):
    """glrm_hip_step_y_arrival with the blocks announced last to first at rank 64: the super-tiles run from the last one down, each from
    its own base."""
    reversed_arrival(monkeypatch, False)


def test_reversed_arrival_order_with_a_diverted_long_column(monkeypatch):
    """The same with one column that observes every row: it leaves the passes for the gather sweep on the side stream (no column of the
    recipe itself does), which reads all of X and so stands behind every announced block, beside the passes."""
    reversed_arrival(monkeypatch, True)


def test_sparse_solver_with_a_diverted_long_column(monkeypatch):
    """fit!(::SparseProxGradParams) on the same problem: the fixed-step form of the passes and, beside them, of the gather sweep that
    takes the long column, against the oracle (1e-5 relative, the bound of the sparse-solver tests of the other families)."""
    force_blocked(monkeypatch, "1", "3")
    pa, X0, Y0 = c4_recipe(6000, 600, 100, 64)
    pa = with_a_full_column(pa, 17)
    sp = L.SparseProxGradParams(max_iter=12)
    outs = []
    for api in (O.oracle_api(), _capi.hip_api()):
        h = api.create(pa)
        try:
            if len(outs) == 1:  # the engine
                assert api.kernel_stats(h)["tiled"] & BLOCKED == BLOCKED
                assert np.diff(pa.colptr).max() >= api.sum_order(h, 1).asdict()["long_from"]
            X, Y = np.array(X0, order="F"), np.array(Y0, order="F")
            obj, _ = api.fit_sparse(h, sp, X, Y)
        finally:
            api.destroy(h)
        outs.append((np.array(obj), X, Y))
    assert len(outs[0][0]) == len(outs[1][0]) and cases.rel_err(outs[1][0], outs[0][0]) < 1e-5
    assert cases.fro_err(outs[1][1], outs[0][1]) < 1e-5 and cases.fro_err(outs[1][2], outs[0][2]) < 1e-5
