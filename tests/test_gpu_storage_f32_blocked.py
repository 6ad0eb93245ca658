"""-m gpu: glrm_options.storage = 1 on the phase-aligned gather passes (csrc/glrm_blocked_f32.hip) -- the float
instantiations of tiled_col_pass_kernel<..., L2 = true>, col_reduce_kernel and col_decide_kernel: A, X and Y stored as floats, every sum
and the line search in fp64, the trial point rounded to float after the prox.

The family is opt-in for a float handle (GLRM_HIP_BLOCKED), so every test forces it the way tests/test_gpu_blocked_pipeline.py does.  The
half-steps are held to the lane-by-lane host reference bit for bit (tests/storage_f32_blocked_ref.py, anchored to the CPU oracle by
tests/test_storage_f32_blocked.py); what that reference does not model -- the transcendental loss kinds, the objective and penalty kernels
-- is held to an fp64 handle on the same family and the same float-representable data, where the two must agree bit for bit."""
import functools

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
import shapes
import storage_f32_blocked_ref as B
import storage_f32_ref as S
import test_gpu_blocked_pipeline as P
import test_gpu_storage_f32 as F
from lowrankmodels.jl_amd import _capi
from shapes import Seg
from test_gpu_sum_order import engine_and_oracle_in_its_order
from test_sum_order import small_problem

pytestmark = pytest.mark.gpu

BLOCKED_R, BLOCKED_C, BOTH = P.BLOCKED_R, P.BLOCKED_C, P.BOTH
REGS = {"quad": (S.REG_QUAD, 0, 0.3), "nonneg": (S.REG_NONNEG, 0, 1.0), "zero": (S.REG_ZERO, 0, 1.0)}
QUAD_SCALE = 0.9   # shapes.column_loss: the one QuadLoss descriptor of a shapes.build model
ORDER_FIELDS = ("family_name", "lanes", "comps", "batch", "rotate", "window", "windows_per_sup", "long_from", "private_order")


def with_regs(pa, reg):
    r = np.array([reg], dtype=_capi.REG_DTYPE)
    return _capi.ProblemArrays(pa.m, pa.n, pa.k, pa.rowptr, pa.colidx, pa.rowvals, pa.colptr, pa.rowidx, pa.colvals, pa.losses, r, r)


def edge_shape(k, reg):
    """m = 3 T + 5, n = 2 T + 3 (a partial last super-tile in both views).  Full list (ranks 64 and 32): columns and rows with 0 .. 17
    observations inside one super-tile and straddling two, a column ending in the last row of a super-tile, one beginning in the first row
    of the next, one holding the last row of X and one ending there.  Reduced list (ranks 5 and 100): 0, 1, G, G + 1 and a straddler."""
    kp, G = shapes.padded_rank(k)
    T = shapes.tile_rows(kp)
    m, n = 3 * T + 5, 2 * T + 3
    if kp in (64, 32):
        lens = P.LENGTHS
        segs = [Seg(f"c{x}", "col", i, x, "window", 1) for i, x in enumerate(lens)]
        segs += [Seg(f"r{x}", "row", i, x, "window", 1) for i, x in enumerate(lens)]
        segs += [Seg(f"cs{x}", "col", 20 + i, x, "straddle", T) for i, x in enumerate(lens)]
        segs += [Seg(f"rs{x}", "row", 20 + i, x, "straddle", T) for i, x in enumerate(lens)]
        segs += [Seg("last_of_sup0", "col", 40, 1, "range", (T - 1, T)), Seg("first_of_sup1", "col", 41, 1, "range", (T, T + 1)),
                 Seg("last_row", "col", 42, 1, "range", (m - 1, m)), Seg("tail", "col", 43, G + 1, "range", (m - G - 1, m))]
    else:
        lens = (0, 1, G, G + 1)
        segs = [Seg(f"c{x}", "col", i, x, "window", 1) for i, x in enumerate(lens)]
        segs += [Seg(f"r{x}", "row", i, x, "window", 1) for i, x in enumerate(lens)]
        segs += [Seg("cs", "col", 10, G + 3, "straddle", T), Seg("rs", "row", 10, G + 3, "straddle", T)]
    sh = shapes.build(m, n, k, segs, fill=1 if kp == 8 else 2, reg="nonneg" if reg == "nonneg" else "quad", seed=500 + k)
    pa, X0, Y0 = F.make_representable(with_regs(sh.pa, REGS[reg]), sh.X0, sh.Y0, nonneg=reg == "nonneg")
    if kp in (64, 32):
        assert list(sh.indices("col", 40)) == [T - 1] and list(sh.indices("col", 41)) == [T] and list(sh.indices("col", 42)) == [m - 1]
        cs9 = sh.indices("col", 20 + lens.index(9))
        assert len(cs9) == 9 and cs9.min() < T <= cs9.max()
    return pa, X0, Y0, T


CASES = {"k64-quad": (64, 8, 8, "quad"), "k32-nonneg": (32, 4, 8, "nonneg"), "k5-zero": (5, 4, 2, "zero"), "k100-quad": (100, 16, 8, "quad")}


@functools.lru_cache(maxsize=None)
def case(name):
    """(pa, X0, Y0, G, R, the host reference's two iterations): computed once, shared, never written to."""
    k, G, R, reg = CASES[name]
    pa, X0, Y0, _ = edge_shape(k, reg)
    want = B.trajectory(pa, X0, Y0, G, R, REGS[reg], 2, (1, 1), loss_scale=QUAD_SCALE)
    return pa, X0, Y0, G, R, want


def float_handle(pa, want_flags=BOTH):
    b = F.Bound(pa, 1, tiled=1)
    flags = b.api.kernel_stats(b.h)["tiled"]
    if flags & BOTH != want_flags:
        b.close()
        raise AssertionError(f"kernel_stats.tiled = {flags}: the float handle is not on the phase-aligned passes (bits 16 / 32)")
    return b


def half_steps(b, X0, Y0, iters=2):
    """[(X after step_x, Y after step_y, objcol, trials_x, trials_y)] of `iters` outer iterations on the bound handle, and Y before each."""
    api, h = b.api, b.h
    api.set_factors(h, X0, Y0)
    api.reset_stepsizes(h, 1.0)
    out = []
    for _ in range(iters):
        api.step_x(h, 0.01)
        X1, Y1 = b.factors()
        tx = api.kernel_stats(h)["trials_x"]
        api.step_y(h, 0.01)
        X2, Y2 = b.factors()
        st = api.kernel_stats(h)
        out.append((X1, Y2, b.objcol(), tx, st["trials_y"], Y1, X2))
    return out


def assert_equals_reference(got, want, Y0):
    for it, (g, w) in enumerate(zip(got, want)):
        X1, Y2, objcol, tx, ty, Ybefore, Xafter = g
        assert (tx, ty) == (w[3], w[4]), ("trial totals", it, (tx, ty), (w[3], w[4]))
        assert np.array_equal(X1, w[0]), ("X after step_x", it, np.abs(X1 - w[0]).max())
        assert np.array_equal(Ybefore, want[it - 1][1] if it else Y0), ("step_x touched Y", it)
        assert np.array_equal(Y2, w[1]), ("Y after step_y", it, np.abs(Y2 - w[1]).max())
        assert np.array_equal(Xafter, w[0]), ("step_y touched X", it)
        assert np.array_equal(objcol, w[2]), ("objective by column", it, np.abs(objcol - w[2]).max())
        assert S.is_f32(X1) and S.is_f32(Y2)


# ------------------------------------------------------------------ 1. flags and order

def test_a_float_handle_takes_the_family_where_the_switch_asks_and_reports_the_fp64_order(monkeypatch):
    pa, X0, Y0, _ = edge_shape(64, "quad")
    api = _capi.hip_api()
    P.on_the_family(monkeypatch)
    h32, h64 = api.create(pa, storage=1, tiled=1), api.create(pa, tiled=1)
    try:
        assert api.storage(h32) == _capi.STORAGE_F32 and api.storage(h64) == _capi.STORAGE_F64
        assert api.kernel_stats(h64)["tiled"] & BOTH == BOTH
        assert api.kernel_stats(h32)["tiled"] & BOTH == BOTH, api.kernel_stats(h32)["tiled"]
        for which in (0, 1):
            o32, o64 = api.sum_order(h32, which).asdict(), api.sum_order(h64, which).asdict()
            assert o64["family_name"] == "windowed"
            for f in ORDER_FIELDS:
                assert o32[f] == o64[f], (which, f, o32[f], o64[f])
            assert o32 == o64, (which, o32, o64)
    finally:
        api.destroy(h32)
        api.destroy(h64)
    monkeypatch.setenv("GLRM_HIP_BLOCKED", "2")
    h = api.create(pa, storage=1, tiled=1)
    try:
        assert api.kernel_stats(h)["tiled"] & BOTH == BLOCKED_C
        assert [api.sum_order(h, w).asdict()["family_name"] for w in (0, 1)] == ["strided", "windowed"]
    finally:
        api.destroy(h)
    monkeypatch.delenv("GLRM_HIP_BLOCKED")
    for kw in ({"tiled": 1}, {}):   # unset: what a float handle is today
        h = api.create(pa, storage=1, **kw)
        try:
            assert api.kernel_stats(h)["tiled"] == 0
            for which in (0, 1):
                o = api.sum_order(h, which).asdict()
                assert (o["family_name"], o["cached_maxlen"], o["long_from"]) == ("strided", -1, 0), o
        finally:
            api.destroy(h)


# ------------------------------------------------------------------ 2. bit for bit against the host reference

@pytest.mark.parametrize("name", list(CASES))
def test_half_steps_equal_the_host_reference_bit_for_bit(monkeypatch, name):
    """X, Y, the bound dObjCol and the trial totals after every half-step of two iterations; then the bound float buffers themselves."""
    pa, X0, Y0, G, R, want = case(name)
    P.on_the_family(monkeypatch)
    b = float_handle(pa)
    try:
        for which in (0, 1):
            o = b.api.sum_order(b.h, which).asdict()
            assert (o["family_name"], o["lanes"], o["comps"], o["windows_per_sup"], o["window"]) == ("windowed", G, R, 1, B.tile_rows(G * R)), o
        assert_equals_reference(half_steps(b, X0, Y0), want, Y0)
        dX = b.dX.cpu().numpy().reshape(pa.m, b.ld)
        dY = b.dY.cpu().numpy().reshape(pa.n, b.ld)
        assert b.ld == G * R
        assert np.array_equal(dX[:, :pa.k].astype(np.float64), want[-1][0].T) and not dX[:, pa.k:].any()
        assert np.array_equal(dY[:, :pa.k].astype(np.float64), want[-1][1].T) and not dY[:, pa.k:].any()
    finally:
        b.close()


# ------------------------------------------------------------------ 3. knobs that change no sum

def test_gate_start_table_and_fill_change_no_bit(monkeypatch):
    pa, X0, Y0, G, R, want = case("k64-quad")

    def run(**env):
        P.on_the_family(monkeypatch)
        for key, v in env.items():
            monkeypatch.setenv("GLRM_HIP_BLOCKED_" + key, v)
        b = float_handle(pa)
        try:
            return half_steps(b, X0, Y0)
        finally:
            b.close()
    for env in ({}, {"GATE": "0"}, {"GATE": "1"}, {"GATE": "37"}, {"SUPPOS": "0"}, {"FILL": "100"}):
        assert_equals_reference(run(**env), want, Y0)


# ------------------------------------------------------------------ 4. the diverted long column

def test_a_long_column_leaves_the_passes_for_the_eight_wave_gather_sweep(monkeypatch):
    k, G, R, reg = 64, 8, 8, REGS["quad"]
    T = shapes.tile_rows(64)
    m, n = T + 40, 24
    segs = [Seg("long", "col", 0, 64 + 9, "uniform"), Seg("almost", "col", 1, 63, "uniform"), Seg("empty", "col", 2, 0, "uniform")]
    sh = shapes.build(m, n, k, segs, fill=2, reg="quad", seed=77)
    pa, X0, Y0 = F.make_representable(with_regs(sh.pa, reg), sh.X0, sh.Y0)
    lens = np.diff(pa.colptr)
    assert lens[0] == 73 and lens[1] == 63 and (lens[3:] < 64).all()
    want = B.trajectory(pa, X0, Y0, G, R, reg, 2, (1, 1), long_from=64, loss_scale=QUAD_SCALE)
    P.on_the_family(monkeypatch)
    monkeypatch.setenv("GLRM_HIP_BLOCKED_LONG_FROM", "64")
    b = float_handle(pa)
    try:
        assert b.api.sum_order(b.h, 1).asdict()["long_from"] == 64
        assert_equals_reference(half_steps(b, X0, Y0), want, Y0)
    finally:
        b.close()


# ------------------------------------------------------------------ 5. every scalar loss kind, against an fp64 handle on the family

NINE_KINDS_SEED, NINE_KINDS_STEPSIZE = 11, 1.0


def test_every_scalar_loss_kind_equals_an_fp64_handle_on_the_family(monkeypatch):
    """The nine scalar kinds by column on float-representable A, X0, Y0 (storage_f32_blocked_ref.nine_kinds_problem): LOSS_SEGMENT by segment
    on the column view, LOSS_PER_OBS with the whole batch of G = 4 observations per step on the row view, two one-tile super-tiles each.
    (a) objective, col_losses and row_penalties agree bit for bit.  (b) One step_x, and one step_y, from the same start on fresh handles:
    both storages form the same gradient and the same unrounded trial points, so X32 == f32r(X64) and Y32 == f32r(Y64) bit for bit and the
    trial / accept totals agree -- provided no accept / reject decision sits within rounding of a tie.  Condition on the inputs, established
    on the CPU for this seed and stepsize (storage_f32_blocked_ref.least_decision_margin, asserted by tests/test_storage_f32_blocked.py):
    every evaluated trial of every segment has |J_trial - J_old| >= 1e-4 max(|J_old|, 1e-300)."""
    pa, X0, Y0, _ = B.nine_kinds_problem(NINE_KINDS_SEED)
    P.on_the_family(monkeypatch)

    def pair():
        b32, b64 = float_handle(pa), F.Bound(pa, 0, tiled=1)
        assert b64.api.kernel_stats(b64.h)["tiled"] & BOTH == BOTH
        return b32, b64
    b32, b64 = pair()
    api = b32.api
    try:
        for reg in (True, False):
            assert api.objective(b32.h, X0, Y0, reg) == api.objective(b64.h, X0, Y0, reg)
        for b in (b32, b64):
            api.col_losses(b.h)
            api.row_penalties(b.h)
        assert np.array_equal(b32.objcol(), b64.objcol()) and np.array_equal(b32.objrow(), b64.objrow())
    finally:
        b32.close()
        b64.close()
    for step, keys, which in ((api.step_x, ("trials_x", "accepts_x"), 0), (api.step_y, ("trials_y", "accepts_y"), 1)):
        b32, b64 = pair()
        try:
            res = []
            for b in (b32, b64):
                api.set_factors(b.h, X0, Y0)
                api.reset_stepsizes(b.h, NINE_KINDS_STEPSIZE)
                step(b.h, 0.01)
                res.append((b.factors()[which], api.kernel_stats(b.h)))
            for key in keys:
                assert res[0][1][key] == res[1][1][key], ("a line-search decision fell the other way", key, res[0][1][key], res[1][1][key])
            assert res[0][1][keys[1]] > 0
            assert np.array_equal(res[0][0], F.f32r(res[1][0])), (which, np.abs(res[0][0] - F.f32r(res[1][0])).max())
            assert not np.array_equal(res[0][0], (X0, Y0)[which])
        finally:
            b32.close()
            b64.close()


# ------------------------------------------------------------------ 6. the Python layer

def test_fit_nnmf_through_the_python_layer_with_the_family_on(monkeypatch):
    P.on_the_family(monkeypatch)
    rng = np.random.default_rng(7)
    m, n, k = 300, 200, 8
    A = np.abs(rng.standard_normal((m, k))) @ np.abs(rng.standard_normal((k, n))) + 0.05 * np.abs(rng.standard_normal((m, n)))
    obs = np.nonzero(rng.random((m, n)) < 0.1)
    g = L.GLRM(A, L.QuadLoss(), L.NonNegConstraint(), L.NonNegConstraint(), k, obs=obs, X=np.abs(rng.standard_normal((k, m))),
               Y=np.abs(rng.standard_normal((k, n))))
    api = _capi.hip_api()
    try:
        _, _, ch = L.fit_b(g, L.HipProxGradParams(storage="f32", tiled=1, max_iter=20, abs_tol=-1e300, rel_tol=-1e300), verbose=False)
        h = g._handle_cache[1]
        assert api.storage(h) == _capi.STORAGE_F32 and api.kernel_stats(h)["tiled"] & BOTH == BOTH
        obj = ch.objective
        assert len(obj) == 21 and np.all(np.isfinite(obj))
        assert all(obj[i + 1] <= obj[i] for i in range(1, 20)), obj
        assert S.is_f32(g.X) and S.is_f32(g.Y) and g.X.min() >= 0 and g.Y.min() >= 0
        first = h.value
        _, _, ch2 = L.fit_b(g, L.HipProxGradParams(storage="f32", tiled=1, max_iter=5, abs_tol=-1e300, rel_tol=-1e300), verbose=False)  # warm start
        assert g._handle_cache[1].value == first and ch2.objective[-1] <= ch2.objective[0] <= obj[-1]
    finally:
        g.close()
    # afterwards an fp64 handle on the family in the same process is what it was: the oracle in its order, bit for bit
    sh, _ = P.boundary_shape(64)
    engine_and_oracle_in_its_order(sh.pa, sh.X0, sh.Y0, 4, BOTH, P.FAMILIES, tiled=1)


# ------------------------------------------------------------------ 7. trajectory against the fp64 oracle

#: max_i |J32_i - J64_i| / J64_i over the 50 iterations below with both views on the family, measured once on the MI355X
TRAJECTORY_MEASURED = 8.713e-06


def test_trajectory_stays_near_the_fp64_oracle(monkeypatch):
    """The recipe of test_gpu_storage_f32.py: QuadLoss, QuadReg(0.1), 2 000 x 500, k = 32, 10 % observed, 50 iterations, against the fp64 CPU
    oracle in reference order.  The bound is 4 x the measured value: the margin for one line-search decision falling the other way."""
    P.on_the_family(monkeypatch)
    rowptr, colidx, rowvals, colptr, rowidx, colvals, X0, Y0 = O.synth_cpu(2000, 500, 32, 50)
    losses = np.array([(0, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)
    r = np.array([(S.REG_QUAD, 0, 0.1)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(2000, 500, 32, rowptr, colidx, rowvals, colptr, rowidx, colvals, losses, r, r)
    X0, Y0 = np.asfortranarray(0.3 * X0), np.asfortranarray(0.3 * Y0)
    prm = L.ProxGradParams(max_iter=50, abs_tol=-1e300, rel_tol=-1e300)
    api, oapi = _capi.hip_api(), O.oracle_api()
    h = api.create(pa, storage=1, tiled=1)
    try:
        assert api.kernel_stats(h)["tiled"] & BOTH == BOTH
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        j32, _ = api.fit(h, prm, X, Y)
    finally:
        api.destroy(h)
    O.set_threads(O.usable_cores())
    ho = oapi.create(pa)
    try:
        X, Y = X0.copy(order="F"), Y0.copy(order="F")
        j64, _ = oapi.fit(ho, prm, X, Y)
    finally:
        oapi.destroy(ho)
    assert len(j32) == len(j64) == 51
    dev = float(np.max(np.abs(j32 - j64) / j64))
    print(f"storage f32 on the phase-aligned passes vs fp64 oracle, max relative objective deviation over 50 iterations: {dev:.3e}")
    assert dev <= 4 * TRAJECTORY_MEASURED, (dev, TRAJECTORY_MEASURED)


# ------------------------------------------------------------------ 8. refusals and memory

def test_refusals_hold_with_the_family_on(monkeypatch):
    P.on_the_family(monkeypatch)
    pa, _, _ = small_problem(12, 20, 5, [3, 9], seed=3, reg=(S.REG_QUAD, 0, 0.3))   # the problem of the refusal test: on the family here
    api = _capi.hip_api()
    h = api.create(pa, storage=1)
    try:
        assert api.kernel_stats(h)["tiled"] & BOTH == BOTH
    finally:
        api.destroy(h)
    F.test_refusals_name_the_mode_and_leave_the_handle_usable()


def test_lists_out_of_tile_order_leave_a_gather_sweep_side(monkeypatch):
    """Row lists in sampling order over three tiles of columns: the row view stays on the gather sweep in both storages, the (sorted) column
    view takes the family.  (The other way out of the family, a padded rank below 8, is not reachable: the smallest layout is kp = 8.)"""
    P.on_the_family(monkeypatch)
    api = _capi.hip_api()
    reg = (S.REG_QUAD, 0, 0.3)
    for k, sorted_lists in ((64, False),):
        pa, X0, Y0 = small_problem(8, 700, k, [5, 40, 90], seed=10 + k, reg=reg, sorted_lists=sorted_lists)
        pa, X0, Y0 = F.make_representable(pa, X0, Y0)
        b32, b64 = F.Bound(pa, 1, tiled=1), F.Bound(pa, 0, tiled=1)
        try:
            want64 = api.kernel_stats(b64.h)["tiled"] & BOTH
            flags = api.kernel_stats(b32.h)["tiled"] & BOTH
            assert flags == want64, (k, flags, want64)          # the float handle gives up the family exactly where the fp64 one does
            assert flags & BLOCKED_R == 0, (k, flags)
            assert api.sum_order(b32.h, 0).asdict()["family_name"] == "strided"
            api.set_factors(b32.h, X0, Y0)
            api.reset_stepsizes(b32.h, 1.0)
            api.step_x(b32.h, 0.01)
            api.step_y(b32.h, 0.01)
            X, Y = b32.factors()
            assert S.is_f32(X) and S.is_f32(Y) and not np.array_equal(X, X0) and not np.array_equal(Y, Y0)
        finally:
            b32.close()
            b64.close()


def test_create_and_destroy_release_the_device_memory(monkeypatch):
    import torch
    P.on_the_family(monkeypatch)
    pa, X0, Y0 = F.nnmf_problem()
    api = _capi.hip_api()

    def cycle():
        h = api.create(pa, storage=1, tiled=1)
        try:
            assert api.kernel_stats(h)["tiled"] & BOTH == BOTH
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, 1.0)
            api.step_x(h, 0.01)
            api.step_y(h, 0.01)
            X, Y = np.zeros_like(X0), np.zeros_like(Y0)
            api.get_factors(h, X, Y)
            api.objective(h, X, Y)
        finally:
            api.destroy(h)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    cycle()
    cycle()
    levels = [free_bytes()]
    for _ in range(2):       # two windows of ten: a leak loses memory in both, a one-off growth of a runtime pool in one
        for _ in range(10):
            cycle()
        levels.append(free_bytes())
    lost = [levels[i] - levels[i + 1] for i in range(2)]
    assert min(lost) < 4 << 20, f"device memory lost per window of 10 create / destroy cycles (MiB): {[round(x / 2**20, 2) for x in lost]}"
