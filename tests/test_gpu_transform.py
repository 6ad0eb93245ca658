"""-m gpu: glrm_hip_solve_x (include/glrm_hip_transform.h; csrc/glrm_solve.hpp: regcached_solve_kernel) and the transform driver.

The contract: on the FUSED path solve_x(T) leaves X, the row step sizes and the trial / accept counters with exactly the bits that T calls
of step_x leave on a handle of the same problem and storage created under GLRM_HIP_CACHED=1; on the LOOP path the bits T step_x calls leave
on the handle itself.  Every comparison below is bit for bit -- the same pass in the same order, so there is no allowance -- except
  * the objective entry point against the oracle's, evaluated on EQUAL factors in two orders: OBJ_TOL = 1e-10, derived in
    tests/test_gpu_cached_chain.py's docstring (64-term dot products and a sum of < 1.8e5 non-negative terms);
  * transform against an ordinary fit on the general sweeps (another family, another order): the project's TOL = 1e-5
    (tests/test_gpu_parity.py).  That fit carries ry = fixed_latent_features(Y[:, j]), whose penalty is 0 where transform records the
    fitted model's column penalties: a constant, py = sum_j evaluate(ry_j, Y[:, j]), evaluated on the host and taken off transform's side
    before the relative comparison (which only makes the denominator smaller).
The stored step sizes are covered by one further step on both sides: step_x on the handle that stepped, solve_x(1) on the handle that
solved -- step_x itself would run that handle's own family there (one wave per short row where the contract's order has two), which the
contract does not hold to any bits.  solve_x_info is asserted in every case, so no case can pass on a
silent fallback.

Problems (the recipe of tests/test_gpu_cached_chain.py::problem): n = 257, m = 600 -- one row per workgroup, so m only has to cover the
lengths -- row lengths from {0, 1, 7, 8, 9, 16, 17, 63, 100, 104}, every one present, and twelve long rows that go to the gather sweep in
its listed form.  Rank 64 (layout 8 x 8, QuadLoss + NonNeg): long rows 105 .. 300, the MAXT = 7 kernel.  Rank 32 (4 x 8, QuadReg): cached
rows <= 64, long rows 209 .. 300, MAXT = 4.  Rank 20 (kp = 32, ZeroReg; the padding must stay zero): also rows of 150 and 208, the
MAXT = 7 kernel of the 4 x 8 layout.  The nine-kinds / no-trig / one-Huber models are tests/test_gpu_storage_f32_cached.py::kinds_problem."""
import functools

import numpy as np
import pytest

import cases
import family_env
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from test_gpu_cached_chain import LENGTHS, N, OBJ_TOL
from test_gpu_parity import TOL, hip
from test_gpu_storage_f32 import Bound
from test_gpu_storage_f32_cached import kinds_problem

pytestmark = pytest.mark.gpu
CACHED = 64
ENV_KEYS = ("GLRM_HIP_CACHED", "GLRM_HIP_CACHED_PERSIST", "GLRM_HIP_BLOCKED", "GLRM_HIP_CACHED_REGS", "GLRM_HIP_CACHED_WAVES")
REGS = {64: L.NonNegConstraint, 32: lambda: L.QuadReg(0.1), 20: L.ZeroReg}


@functools.lru_cache(maxsize=None)
def problem(m, k, long_rows=12):
    """Seeded; built once per shape and shared (nothing writes to it).  -> (ProblemArrays, X0, Y0, row lengths)"""
    rng = np.random.default_rng(1000 * k + m)
    pool = [l for l in LENGTHS if k != 32 or l <= 64] + ([150, 208] if k == 20 else [])
    maxlen = 104 if k == 64 else 208
    lens = rng.choice(pool, size=m)
    if m >= len(pool):
        lens[: len(pool)] = pool                                    # every length occurs
    else:
        lens[:] = 100
    long_rows = min(long_rows, m // 4)
    if long_rows:
        lens[rng.choice(np.arange(len(pool), m), size=long_rows, replace=False)] = np.linspace(maxlen + 1, 300, long_rows).astype(int)
    return from_lengths(rng, lens, k)


def from_lengths(rng, lens, k):
    """The problem whose row i holds lens[i] observations (a row longer than N repeats columns).  -> (ProblemArrays, X0, Y0, lens)"""
    m = len(lens)
    I, J = [], []
    for i, l in enumerate(lens):
        cols = rng.permutation(N)[: min(l, N)]
        if l > N:
            cols = np.concatenate([cols, rng.integers(0, N, l - N)])
        I.append(np.full(l, i)); J.append(np.sort(cols))
    I, J = np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)
    X0, Y0 = np.abs(rng.standard_normal((k, m))) / 8.0, np.abs(rng.standard_normal((k, N))) * rng.choice([0.125, 0.5], size=N)
    A = X0.T @ Y0 + 0.1 * rng.standard_normal((m, N))
    g = L.GLRM(A, L.QuadLoss(), REGS[k](), REGS[k](), k, obs=(I, J), X=X0, Y=Y0)
    X0, Y0 = np.asfortranarray(X0), np.asfortranarray(Y0)
    for a in (X0, Y0):
        a.setflags(write=False)
    return g.problem_arrays(), X0, Y0, lens


def run(monkeypatch, env, pa, X0, Y0, T, *, solve, stepsize=1.0, min_stepsize=0.01, storage=0, tiled=1, api=None, orders=None, waves_row=0):
    """Create under `env`, T X half-steps (one solve_x(T), or T step_x calls), then ONE further step (solve_x(1) / step_x).  -> dict"""
    api = api or hip()
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    family_env.setenv(monkeypatch, env)
    h = api.create(pa, tiled=tiled, storage=storage, waves_row=waves_row) if api is hip() else api.create(pa)
    try:
        out = {}
        if orders is not None:
            for w, o in enumerate(orders):
                O.set_sum_order(h, w, o)
        else:
            out["tiled"] = api.kernel_stats(h)["tiled"]
            out["orders"] = [api.sum_order(h, 0), api.sum_order(h, 1)]
        api.set_factors(h, X0, Y0)
        api.reset_stepsizes(h, stepsize)
        if solve:
            api.solve_x(h, T, min_stepsize)
            out["info"] = api.solve_x_info(h)
        else:
            for _ in range(T):
                api.step_x(h, min_stepsize)
        X, Y = np.zeros_like(X0), np.zeros_like(Y0)
        api.get_factors(h, X, Y)
        st = api.kernel_stats(h)
        out.update(X=X, Y=Y, trials=st["trials_x"], accepts=st["accepts_x"], launches=st["launches_x"])
        api.solve_x(h, 1, min_stepsize) if solve else api.step_x(h, min_stepsize)
        X2, Y2 = np.zeros_like(X0), np.zeros_like(Y0)
        api.get_factors(h, X2, Y2)
        st = api.kernel_stats(h)
        out.update(X2=X2, trials2=st["trials_x"], accepts2=st["accepts_x"])
    finally:
        api.destroy(h)
    return out


def same(a, b, what, stored=True):
    bad = np.flatnonzero(np.any(a["X"] != b["X"], axis=0))
    assert bad.size == 0, (what, "rows", bad[:12])
    assert (a["trials"], a["accepts"]) == (b["trials"], b["accepts"]), (what, a["trials"], a["accepts"], b["trials"], b["accepts"])
    assert a["Y"].tobytes() == b["Y"].tobytes(), what
    if stored:  # one further step: the stored step sizes
        assert np.array_equal(a["X2"], b["X2"]) and (a["trials2"], a["accepts2"]) == (b["trials2"], b["accepts2"]), (what, "after one more step")


def fused_counts(lens, k):
    maxlen = 104 if k == 64 else 208
    return dict(fused=1, fused_rows=int(np.sum(lens <= maxlen)), loop_rows=int(np.sum(lens > maxlen)))


# ------------------------------------------------------------------ 1, 2. a handle that did not pick the family; the oracle

@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("k", [64, 32, 20])
def test_fused_path_on_a_handle_off_the_family_equals_T_steps_of_a_cached_handle_and_the_oracle(monkeypatch, k, T):
    pa, X0, Y0, lens = problem(600, k)
    got = run(monkeypatch, {}, pa, X0, Y0, T, solve=True)
    assert got["tiled"] & CACHED == 0, got["tiled"]
    assert got["info"] == fused_counts(lens, k) and got["info"]["loop_rows"] == 12, got["info"]
    assert got["launches"] == T and got["accepts"] > 0
    assert np.array_equal(got["Y"], Y0) and not np.array_equal(got["X"], X0)
    row = run(monkeypatch, family_env.cached(persist=False), pa, X0, Y0, T, solve=False)
    assert row["tiled"] & CACHED
    o = row["orders"][0].asdict()
    assert (o["family_name"], o["cached_waves"], o["cached_maxlen"]) == ("strided", 2, 104 if k == 64 else 208), o
    same(got, row, "one-row-per-workgroup kernel")
    same(got, run(monkeypatch, family_env.cached(), pa, X0, Y0, T, solve=False), "persistent kernel")
    # the oracle, adding in the orders the cached handle reports
    O.set_threads(O.usable_cores())
    orc = run(monkeypatch, {}, pa, X0, Y0, T, solve=False, api=O.oracle_api(), orders=row["orders"])
    same(got, orc, "oracle in the engine's order")
    h, ho = hip().create(pa, tiled=1), O.oracle_api().create(pa)
    try:
        obj = (hip().objective(h, got["X"], got["Y"]), O.oracle_api().objective(ho, orc["X"], orc["Y"]))
    finally:
        hip().destroy(h)
        O.oracle_api().destroy(ho)
    print(f"k={k} T={T}: objective {obj[0]!r} (engine) {obj[1]!r} (oracle), rel {cases.rel_err([obj[0]], [obj[1]]):.3g}")
    assert cases.rel_err([obj[0]], [obj[1]]) < OBJ_TOL, obj


def test_rank_20_padding_stays_zero(monkeypatch):
    """kp = 32: the twelve lanes' worth of padding behind k = 20 is stored by the fused kernel and must still be exactly zero."""
    pa, X0, Y0, lens = problem(600, 20)
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for storage in (0, 1):
        b = Bound(pa, storage, tiled=1)
        try:
            b.api.set_factors(b.h, X0, Y0)
            b.api.reset_stepsizes(b.h, 1.0)
            b.api.solve_x(b.h, 3, 0.01)
            assert b.api.solve_x_info(b.h)["fused"] == 1
            b.api.synchronize(b.h)
            dX = b.dX.cpu().numpy().reshape(pa.m, b.ld)
            assert b.ld == 32 and not dX[:, 20:].any() and dX[:, :20].any()
            assert np.array_equal(dX[:, :20].astype(np.float64), b.factors()[0].T)
        finally:
            b.close()


# ------------------------------------------------------------------ 3. T = 1 on a cached handle

@pytest.mark.parametrize("k", [64, 32])
def test_solve_x_1_on_a_cached_handle_is_step_x(monkeypatch, k):
    pa, X0, Y0, lens = problem(600, k)
    for env in (family_env.cached(), family_env.cached(persist=False)):
        got = run(monkeypatch, env, pa, X0, Y0, 1, solve=True)
        assert got["tiled"] & CACHED and got["info"] == fused_counts(lens, k)
        same(got, run(monkeypatch, env, pa, X0, Y0, 1, solve=False), env)


# ------------------------------------------------------------------ 4. line-search edges

@pytest.mark.parametrize("m", [600, 1, 127])
@pytest.mark.parametrize("min_stepsize", [0.01, 0.5])
def test_rejections_and_rows_that_give_up(monkeypatch, m, min_stepsize):
    """From stepsize 1e3 a row shrinks several times before it accepts; with min_stepsize = 0.5 rows give up without accepting and carry on
    from min_stepsize * 1.1 with their next step, inside the one launch."""
    T = 5
    pa, X0, Y0, lens = problem(m, 64)
    got = run(monkeypatch, {}, pa, X0, Y0, T, solve=True, stepsize=1e3, min_stepsize=min_stepsize)
    assert got["info"] == fused_counts(lens, 64), got["info"]
    ref = run(monkeypatch, family_env.cached(persist=False), pa, X0, Y0, T, solve=False, stepsize=1e3, min_stepsize=min_stepsize)
    same(got, ref, (m, min_stepsize))
    if min_stepsize == 0.01:
        assert got["trials"] > 3 * got["accepts"] > 0, (got["trials"], got["accepts"])      # several trials per accepted step
    elif m == 600:
        assert 0 < got["accepts"] < T * int(np.count_nonzero(lens)), (got["accepts"], "every non-empty row accepted in every step")


# ------------------------------------------------------------------ 5. losses and regularizers

def periodic_problem():
    pa, X0, Y0 = kinds_problem("one-huber")
    lo = np.array([L.PeriodicLoss(2.5, 0.8).descriptor()], dtype=_capi.LOSS_DTYPE)
    return _capi.ProblemArrays(pa.m, pa.n, pa.k, pa.rowptr, pa.colidx, pa.rowvals, pa.colptr, pa.rowidx, pa.colvals, lo, pa.rx, pa.ry), X0, Y0


def simplex_problem():
    """fp64 only: SimplexConstraint on the rows is a prox over the whole vector -- the VR = true kernels"""
    rng = np.random.default_rng(41)
    m, n, k = 300, 131, 64
    X0 = rng.random((k, m)); X0 /= X0.sum(axis=0)
    Y0 = rng.standard_normal((k, n))
    A = X0.T @ Y0 + 0.1 * rng.standard_normal((m, n))
    rows = [np.sort(rng.choice(n, 1 + (7 * e) % 104, replace=False)) for e in range(m)]
    I, J = np.repeat(np.arange(m), [len(r) for r in rows]), np.concatenate(rows)
    g = L.GLRM(A, L.QuadLoss(), L.SimplexConstraint(), L.QuadReg(0.1), k, obs=(I, J), X=X0, Y=Y0)
    return g.problem_arrays(), np.asfortranarray(X0), np.asfortranarray(Y0)


MODELS = {"nine-kinds": lambda: kinds_problem("nine-kinds"), "eight-kinds-no-trig": lambda: kinds_problem("eight-kinds-no-trig"),
          "one-huber": lambda: kinds_problem("one-huber"), "one-periodic": periodic_problem, "simplex-rows": simplex_problem}


@pytest.mark.parametrize("model", list(MODELS))
def test_every_loss_variant_and_the_vector_prox_kernels(monkeypatch, model):
    """solve_x(3) against 3 step_x calls on the cached handle: the five loss variants of the kernels (a loss per observation with and
    without PeriodicLoss, one loss per model with and without it; QuadLoss is every other case) and VR = true."""
    pa, X0, Y0 = MODELS[model]()
    got = run(monkeypatch, {}, pa, X0, Y0, 3, solve=True)
    assert got["info"] == dict(fused=1, fused_rows=pa.m, loop_rows=0) and got["accepts"] > 0, (got["info"], got["accepts"])
    assert not np.array_equal(got["X"], X0)
    same(got, run(monkeypatch, family_env.cached(), pa, X0, Y0, 3, solve=False), model)


# ------------------------------------------------------------------ 6. f32

@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("k", [64, 20])
def test_f32_handle_takes_the_fused_path_without_an_environment_switch(monkeypatch, k, T):
    pa, X0, Y0, lens = problem(600, k)
    got = run(monkeypatch, {}, pa, X0, Y0, T, solve=True, storage=1)
    assert got["tiled"] & CACHED == 0 and got["info"] == fused_counts(lens, k), (got["tiled"], got["info"])
    ref = run(monkeypatch, family_env.cached(), pa, X0, Y0, T, solve=False, storage=1)
    assert ref["tiled"] & CACHED
    same(got, ref, "f32 cached handle")
    assert np.array_equal(got["X"], got["X"].astype(np.float32).astype(np.float64)) and not np.array_equal(got["X"], X0)
    assert got["accepts"] > 0


# ------------------------------------------------------------------ 7. the loop path

def tiled_problem():
    rng = np.random.default_rng(17)
    m, n, k = 3000, 300, 16
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n))
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), k, obs=np.nonzero(rng.random((m, n)) < 0.5))
    return g.problem_arrays(), np.asfortranarray(g.X), np.asfortranarray(g.Y), 2, 1


def dense_problem():
    rng = np.random.default_rng(18)
    g = L.GLRM(rng.standard_normal((512, 256)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), 32)
    return g.problem_arrays(dense=True), np.asfortranarray(g.X), np.asfortranarray(g.Y), 0, 4


def multidim_problem():
    kwargs, _ = cases.build_multidim_case("categorical_mix")
    g = L.GLRM(**kwargs)
    return g.problem_arrays(), np.asfortranarray(g.X), np.asfortranarray(g.Y), 0, 8


def gather_problem():
    pa, X0, Y0, _ = problem(600, 64)
    return pa, X0, Y0, 1, 0


@pytest.mark.parametrize("kind", ["gather", "lds-tiled", "dense", "multidim"])
def test_loop_path_equals_T_steps_on_the_handle_itself(monkeypatch, kind):
    pa, X0, Y0, tiled, flag = {"gather": gather_problem, "lds-tiled": tiled_problem, "dense": dense_problem, "multidim": multidim_problem}[kind]()
    env = family_env.GATHER if kind == "gather" else {}
    got = run(monkeypatch, env, pa, X0, Y0, 3, solve=True, tiled=tiled)
    assert got["tiled"] & flag == flag and got["tiled"] & CACHED == 0, got["tiled"]
    assert got["info"] == dict(fused=0, fused_rows=0, loop_rows=pa.m), got["info"]
    assert got["launches"] == 3 and not np.array_equal(got["X"], X0)
    same(got, run(monkeypatch, env, pa, X0, Y0, 3, solve=False, tiled=tiled), kind)


def test_inner_iter_below_one_is_invalid():
    pa, X0, Y0, _ = problem(600, 64)
    api = hip()
    h = api.create(pa, tiled=1)
    try:
        api.set_factors(h, X0, Y0)
        for bad in (0, -3):
            with pytest.raises(_capi.GLRMError) as ei:
                api.solve_x(h, bad, 0.01)
            assert ei.value.code == _capi.ERR_INVALID
        with pytest.raises(_capi.GLRMError) as ei:
            api.solve_x_info(h)                                        # nothing has run yet
        assert ei.value.code == _capi.ERR_INVALID
    finally:
        api.destroy(h)


# ------------------------------------------------------------------ 8. transform end to end

@functools.lru_cache(maxsize=None)
def fitted_model():
    rng = np.random.default_rng(8)
    m, n, k = 300, 40, 20
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n)) + 0.1 * rng.standard_normal((m, n))
    g = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), k, X=rng.standard_normal((k, m)), Y=rng.standard_normal((k, n)))
    L.fit_b(g, L.HipProxGradParams(max_iter=20), verbose=False)
    g.close()
    return g, A, np.asfortranarray(rng.standard_normal((k, m)))


def api_loop(monkeypatch, g, A, X0, p, storage):
    """the hand-written loop of the step-level entry points on a GLRM_HIP_CACHED=1 handle (step_x calls, never solve_x)"""
    import torch
    family_env.setenv(monkeypatch, family_env.cached())
    api = hip()
    new = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), g.k, X=X0, Y=g.Y)
    h = api.create(new.problem_arrays(), tiled=1, storage=storage)
    try:
        assert api.kernel_stats(h)["tiled"] & CACHED
        oc, orow = torch.zeros(new.n, dtype=torch.float64, device="cuda"), torch.zeros(new.m, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        api.bind_buffers(h, None, None, oc.data_ptr(), orow.data_ptr())
        X, Y = np.array(X0, order="F"), np.array(g.Y, order="F")
        api.set_factors(h, X, Y)
        api.reset_stepsizes(h, p.stepsize)
        api.col_losses(h)
        loss = api.sum(h, oc.data_ptr(), new.n)
        api.row_penalties(h)
        px = api.sum(h, orow.data_ptr(), new.m)
        api.col_penalties(h)
        objs = [loss + (px + api.sum(h, oc.data_ptr(), new.n))]
        for _ in range(p.max_iter):
            api.reset_stepsizes(h, p.stepsize)
            for _ in range(p.inner_iter_X):
                api.step_x(h, p.min_stepsize)
            api.col_losses(h)
            loss = api.sum(h, oc.data_ptr(), new.n)
            api.col_penalties(h)
            objs.append(loss + api.sum(h, oc.data_ptr(), new.n))
        api.get_factors(h, X, Y)
    finally:
        api.destroy(h)
        for key in ENV_KEYS:
            monkeypatch.delenv(key, raising=False)
    return X, np.array(objs)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_transform_end_to_end(monkeypatch, storage):
    g, A, X0 = fitted_model()
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    p = L.HipProxGradParams(1.0, max_iter=8, inner_iter_X=5, abs_tol=0.0, rel_tol=0.0, tiled=1, storage=storage)
    Ybytes = g.Y.tobytes()
    X, ch = L.transform(g, A, p, X0=X0)
    objs = np.array(ch.objective)
    assert g.Y.tobytes() == Ybytes and X.shape == (g.k, 300) and len(objs) == 9
    Xl, ol = api_loop(monkeypatch, g, A, X0, p, 1 if storage == "f32" else 0)
    assert np.array_equal(X, Xl) and np.array_equal(objs, ol), (np.abs(X - Xl).max(), objs, ol)
    assert np.all(np.diff(objs[1:]) <= 0) and objs[-1] < objs[1], objs
    if storage == "f32":
        assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
        return
    # an ordinary fit of the same rows with every column of Y fixed: existing code, on the general sweeps
    ry = [L.fixed_latent_features(L.QuadReg(0.1), g.Y[:, j]) for j in range(g.n)]
    fix = L.GLRM(A, L.QuadLoss(), L.QuadReg(0.1), ry, g.k, X=X0, Y=g.Y)
    try:
        _, _, chf = L.fit_b(fix, p, verbose=False)
        assert np.array_equal(fix.Y, g.Y)
        of = np.array(chf.objective)
        py = sum(r.evaluate(g.Y[:, j]) for j, r in enumerate(g.ry))      # what the fixed-features penalty does not count (docstring)
        print("transform - py:", objs - py, "fit:", of, "rel", cases.rel_err(objs - py, of), "X", cases.fro_err(X, fix.X))
        assert len(of) == len(objs) and cases.rel_err(objs - py, of) < TOL, (objs - py, of)
    finally:
        fix.close()


# ------------------------------------------------------------------ 9. leaks

def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_no_device_memory_leak_over_create_solve_destroy_cycles(monkeypatch):
    """tests/test_gpu_leaks.py's method: warm up, then windows of cycles; a leak loses memory in every window.  20 cycles in two windows,
    on a handle that builds the solver's own class plan (a list of rows on the device, and the side stream for its long rows)."""
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    pa, X0, Y0, _ = problem(600, 64)
    api = hip()

    def cycle():
        h = api.create(pa, tiled=1)
        try:
            api.set_factors(h, X0, Y0)
            api.reset_stepsizes(h, 1.0)
            api.solve_x(h, 2, 0.01)
            assert api.solve_x_info(h)["fused"] == 1
            api.synchronize(h)
        finally:
            api.destroy(h)
    cycle()
    cycle()
    levels = [free_bytes()]
    for _ in range(2):
        for _ in range(10):
            cycle()
        levels.append(free_bytes())
    lost = [levels[i] - levels[i + 1] for i in range(2)]
    assert min(lost) < 4 << 20, f"device memory lost per window of 10 cycles (MiB): {[round(x / 2**20, 1) for x in lost]}"


# ------------------------------------------------------------------ 10. corners of the class plan and of the class-by-class launcher

@functools.lru_cache(maxsize=None)
def class_problem(name):
    """k = 64, built once and shared.  "three-classes": 48 rows the register kernel takes (0 .. 104 observations, both ends present), 12
    one-wave rows (105 .. 300) and 4 four-wave rows (1536 .. 1700), shuffled so that every class list skips rows.  "all-long": 8 rows of
    105 .. 300 -- no row for the register kernel."""
    rng = np.random.default_rng({"three-classes": 64064, "all-long": 64008}[name])
    if name == "three-classes":
        short = rng.integers(0, 105, 48)
        short[:2] = 0, 104
        lens = np.concatenate([short, np.linspace(105, 300, 12).astype(int), np.linspace(1536, 1700, 4).astype(int)])
        rng.shuffle(lens)
    else:
        lens = np.linspace(105, 300, 8).astype(int)
    return from_lengths(rng, lens, 64)


@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("k", [64, 32])
def test_solve_x_T_on_a_cached_handle_equals_T_step_x_calls(monkeypatch, k, T):
    """the handle's own plan (class 0 plus 12 one-wave rows), T > 1: the longer rows take T launches beside the one fused launch"""
    pa, X0, Y0, lens = problem(600, k)
    for env in (family_env.cached(), family_env.cached(persist=False)):
        got = run(monkeypatch, env, pa, X0, Y0, T, solve=True)
        assert got["tiled"] & CACHED and got["info"] == fused_counts(lens, k) and got["launches"] == T, (got["tiled"], got["info"], got["launches"])
        same(got, run(monkeypatch, env, pa, X0, Y0, T, solve=False), (env, T))


def test_three_classes_in_one_plan(monkeypatch):
    pa, X0, Y0, lens = class_problem("three-classes")
    assert (np.sum(lens <= 104), np.sum((lens >= 105) & (lens <= 300)), np.sum((lens >= 1536) & (lens <= 1700))) == (48, 12, 4)
    got = run(monkeypatch, {}, pa, X0, Y0, 3, solve=True)
    assert got["tiled"] & CACHED == 0 and got["info"] == dict(fused=1, fused_rows=48, loop_rows=16), (got["tiled"], got["info"])
    assert got["launches"] == 3 and got["accepts"] > 0
    ref = run(monkeypatch, family_env.cached(), pa, X0, Y0, 3, solve=False)
    assert ref["tiled"] & CACHED
    same(got, ref, "three classes")


def test_no_row_for_the_register_kernel(monkeypatch):
    """every row is long: the fused path runs no fused launch, and the cached handle it is held to fell back to the gather sweep"""
    pa, X0, Y0, lens = class_problem("all-long")
    assert lens.min() >= 105 and lens.max() <= 300 and len(lens) == 8
    got = run(monkeypatch, {}, pa, X0, Y0, 3, solve=True)
    assert got["info"] == dict(fused=1, fused_rows=0, loop_rows=8), got["info"]
    assert got["launches"] == 3 and got["accepts"] > 0
    ref = run(monkeypatch, family_env.cached(), pa, X0, Y0, 3, solve=False)
    assert ref["tiled"] & CACHED == 0, ref["tiled"]                   # cached_row fell to 0: the shard holds no class-0 row
    same(got, ref, "no class-0 row")


def test_pinned_waves_reach_both_plans(monkeypatch):
    """waves_row = 4: the twelve longer rows run the four-wave sweep, in the plan solve_x builds and in the cached handle's own"""
    pa, X0, Y0, lens = problem(600, 64)
    got = run(monkeypatch, {}, pa, X0, Y0, 2, solve=True, waves_row=4)
    assert got["tiled"] & CACHED == 0 and got["info"] == fused_counts(lens, 64), (got["tiled"], got["info"])
    ref = run(monkeypatch, family_env.cached(), pa, X0, Y0, 2, solve=False, waves_row=4)
    assert ref["tiled"] & CACHED
    assert got["orders"][0].waves == 4 and ref["orders"][0].waves == 4, (got["orders"][0].waves, ref["orders"][0].waves)
    same(got, ref, "waves_row = 4")
