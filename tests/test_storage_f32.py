"""glrm_options.storage = 1 (include/glrm_hip_storage.h), the CPU side: the host reference of the f32 gather sweeps
(tests/storage_f32_ref.py) is anchored to the CPU oracle, the rounding it adds has the properties the mode promises, and the boundary
kept its shape.  The GPU part is tests/test_gpu_storage_f32.py."""
import ctypes as C
import importlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import lane_orders as LO
import lowrankmodels.jl_amd as L
import oracle as O
import storage_f32_ref as S
from lowrankmodels.jl_amd import _capi
from test_sum_order import small_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_libm_fma_is_the_exact_fma_of_the_lane_simulation():
    rnd = random.Random(3)
    for _ in range(2000):
        a, b, c = (rnd.uniform(-2, 2) * 2.0 ** rnd.randint(-30, 30) for _ in range(3))
        if rnd.random() < 0.3:
            c = -a * b  # cancellation: the case a product rounded before the add gets wrong
        assert S.libm_fma(a, b, c) == LO.fma(a, b, c)


def oracle_iterations(pa, X0, Y0, order, iters):
    api = O.oracle_api()
    h = api.create(pa)
    out = []
    try:
        O.set_sum_order(h, 0, order)
        O.set_sum_order(h, 1, order)
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


@pytest.mark.parametrize("k,G,R,waves", [(10, 4, 4, 1), (20, 4, 8, 4)])
def test_without_rounding_the_reference_is_the_oracle_in_the_strided_order(k, G, R, waves):
    """Two outer iterations, so that the per-segment step sizes carried from one iteration to the next are part of what is compared."""
    pa, X0, Y0 = small_problem(8, 60, k, [3, 17, 40, 150], seed=k, reg=(1, 0, 0.3))
    want = oracle_iterations(pa, X0, Y0, O.make_sum_order("strided", G, R, waves=waves), 2)
    got = S.trajectory(pa, X0, Y0, G, R, (1, 0, 0.3), 2, waves=waves, rounding=False)
    for (X1, Y2, tx, ty), (Xs, Ys, _, sx, sy, _) in zip(want, got):
        assert np.array_equal(Xs, X1) and np.array_equal(Ys, Y2)
        assert (sx, sy) == (tx, ty)


@pytest.fixture(scope="module")
def rounded_run():
    """8 x 24, k = 10, rows of 0 / 1 / 16 / 33 observations, float-representable data, six iterations with and without rounding."""
    pa, X0, Y0 = small_problem(8, 24, 10, [0, 1, 16, 33], seed=11, reg=(1, 0, 0.3))
    pa.rowvals[:] = pa.rowvals.astype(np.float32)
    pa.colvals[:] = pa.colvals.astype(np.float32)
    X0, Y0 = (np.asfortranarray(a.astype(np.float32).astype(np.float64)) for a in (X0, Y0))
    sims = {}
    for rounding in (True, False):
        sim = S.Simulation(pa, X0, Y0, 4, 4, (1, 0, 0.3), waves=1, rounding=rounding)
        steps = []
        for _ in range(6):
            sim.step_x()
            steps.append((sim.X.copy(), sim.Y.copy(), sim.obj[0].copy(), None))
            sim.step_y()
            steps.append((sim.X.copy(), sim.Y.copy(), None, sim.obj[1].copy()))
        sims[rounding] = steps
    return sims


def test_with_rounding_every_iterate_is_float_representable(rounded_run):
    for X, Y, _, _ in rounded_run[True]:
        assert S.is_f32(X) and S.is_f32(Y)
    assert not all(S.is_f32(X) and S.is_f32(Y) for X, Y, _, _ in rounded_run[False])  # (the property is the rounding's, not the data's)
    Xr, Yr = rounded_run[True][-1][:2]
    Xu, Yu = rounded_run[False][-1][:2]
    assert 0 < np.abs(Xr - Xu).max() < 1e-5 and 0 < np.abs(Yr - Yu).max() < 1e-5


def test_with_rounding_no_segment_objective_increases(rounded_run):
    """The trial is evaluated at the rounded point, so an accepted step is a strict decrease of the objective of what is stored.  Between two
    half-steps of one side the other factor moved, which only lowers the total: checked per segment inside a half-step pair by the totals."""
    steps = rounded_run[True]
    tot_prev = None
    for i in range(1, len(steps), 2):
        objcol = steps[i][3]
        objrow = steps[i - 1][2]
        assert np.all(np.isfinite(objcol)) and np.all(np.isfinite(objrow))
        tot = objcol.sum()
        if tot_prev is not None:
            assert tot <= tot_prev
        tot_prev = tot
    # per segment: a half-step's recorded objective never exceeds the objective at the point it started from
    pa, X0, Y0 = small_problem(8, 24, 10, [0, 1, 16, 33], seed=11, reg=(1, 0, 0.3))
    pa.rowvals[:] = pa.rowvals.astype(np.float32)
    pa.colvals[:] = pa.colvals.astype(np.float32)
    X0, Y0 = (np.asfortranarray(a.astype(np.float32).astype(np.float64)) for a in (X0, Y0))
    sim = S.Simulation(pa, X0, Y0, 4, 4, (1, 0, 0.3), waves=1)
    regfn, _ = S.reg_fns((1, 0, 0.3), 10, 4, 4, True)
    for _ in range(3):
        for rows in (True, False):
            ptr, idx, vals = (pa.rowptr, pa.colidx, pa.rowvals) if rows else (pa.colptr, pa.rowidx, pa.colvals)
            own, fac = (sim.X, sim.Y) if rows else (sim.Y, sim.X)
            facl = [list(fac[:, i]) for i in range(fac.shape[1])]
            before = []
            for s in range(len(ptr) - 1):
                b, e = int(ptr[s]), int(ptr[s + 1])
                x = [float(v) for v in own[:, s]]
                J, _ = LO.strided_pass([int(v) for v in idx[b:e]], [float(v) for v in vals[b:e]], x, facl, 10, 4, 4, 1, 0.75, False)
                before.append(J + regfn(x))
            (sim.step_x if rows else sim.step_y)()
            assert np.all(sim.obj[0 if rows else 1] <= np.array(before))


def test_options_struct_keeps_its_shape():
    assert C.sizeof(_capi.COptions) == 48
    assert _capi.COptions.storage.offset == 40 and _capi.COptions.reserved.offset == 44
    assert [f for f, _ in _capi.COptions._fields_][-3:] == ["sum_order", "storage", "reserved"]
    hdr = open(os.path.join(ROOT, "include", "glrm_hip.h")).read()
    assert re.search(r"int32_t\s+storage;", hdr) and "reserved0" not in hdr
    jl = open(os.path.join(ROOT, "julia", "HipGLRM.jl")).read()
    assert "sum_order::Int32; storage::Int32; reserved::Int32" in jl


def test_boundary_header_still_declares_37_entry_points():
    hdr = open(os.path.join(ROOT, "include", "glrm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(glrm_hip_\w+)\s*\(", hdr))
    assert len(names) == 37 == len(_capi.ABI_SYMBOLS), sorted(names)
    assert names == {"glrm_hip_" + s for s in _capi.ABI_SYMBOLS}
    assert "storage" not in _capi.ABI_SYMBOLS and _capi.STORAGE_SYMBOLS == ("storage",)
    ext = open(os.path.join(ROOT, "include", "glrm_hip_storage.h")).read()
    assert re.search(r"#define\s+GLRM_STORAGE_F64\s+0", ext) and re.search(r"#define\s+GLRM_STORAGE_F32\s+1", ext)
    assert re.search(r"int\s+glrm_hip_storage\s*\(\s*glrm_handle\s*\*\s*h\s*\)\s*;", ext)


@pytest.mark.parametrize("path", [_capi.HIP_LIB_PATH, _capi.HIP_TESTING_LIB_PATH])
def test_libraries_export_glrm_hip_storage(path):
    assert os.path.exists(path), path + " is missing: build it with `python __graft_entry__.py`"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT glrm_hip_storage$", out, flags=re.M)


def test_params_validation():
    assert L.HipProxGradParams().storage == "f64"
    assert L.HipProxGradParams(storage="f32").storage == "f32"
    for bad in ("f16", "fp32", 1, None, "F32"):
        with pytest.raises(ValueError):
            L.HipProxGradParams(storage=bad)
    with pytest.raises(ValueError):
        L.HipProxGradParams(storage="f32", ngpus=2)
    with pytest.raises(ValueError):
        L.HipProxGradParams(storage="f32", mode="reference_order")
    F = importlib.import_module("lowrankmodels.jl_amd.fit")  # (the package re-exports the function `fit` under the same name)
    assert F._engine_opts(L.HipProxGradParams(storage="f32"))["storage"] == 1
    assert F._engine_opts(L.HipProxGradParams())["storage"] == 0 == F._engine_opts(L.ProxGradParams())["storage"]
    p = L.HipProxGradParams()
    p.storage = "f16"  # assigned after construction: the fit refuses it as well
    with pytest.raises(ValueError):
        F._engine_opts(p)
    p = L.HipProxGradParams(storage="f32")
    p.ngpus = 2
    g = L.GLRM(np.ones((4, 3)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 2)
    with pytest.raises(ValueError):
        L.fit_b(g, p, verbose=False, engine=O.oracle_api())  # refused before any engine is asked
