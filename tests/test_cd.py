"""The coordinate-descent extension (include/glrm_hip_cd.h) without a GPU.

  * The built libraries export what the header declares, the boundary header still declares 37 symbols, an engine without the extension is
    refused by name, and the Julia shim (julia/HipGLRMCd.jl, which cannot run here) is held to the C prototypes.
  * The numpy restatement (tests/cd_ref.py) -- the reference of tests/test_gpu_cd.py -- exists in two forms that are held to each other bit
    for bit, and the scalar form is held to BRUTE FORCE: for k <= 5 every support (NonNegConstraint) or sign pattern (OneReg) is solved with
    np.linalg.solve and the feasible, sign-consistent candidate of least objective is the answer.  No library solver is involved.
  * The rules of the header one by one: a zero denominator, an empty segment, a negative non-negative start.
  * The driver (fit_b with CdParams) runs on the CPU oracle wrapped by cd_ref.HostEngine.
"""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest

import cd_ref as R
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.fit import _should_stop
from test_abi import PKG, ROOT, declared, ensure_built

HEADER = "glrm_hip_cd.h"
EPS = 2.0 ** -52


# ------------------------------------------------------------------ the boundary

def test_libraries_export_every_symbol_the_header_declares():
    ensure_built()
    names = declared(HEADER, "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.CD_SYMBOLS) and len(names) == 2
    assert not set(_capi.CD_SYMBOLS) & set(_capi.ABI_SYMBOLS)           # outside the 37-symbol boundary
    assert len(declared("glrm_hip.h", "glrm_hip_")) == 37 == len(_capi.ABI_SYMBOLS)
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)


def test_the_header_states_the_limits_and_the_rules():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    for name, val in (("GLRM_CD_MAX_K", _capi.CD_MAX_K), ("GLRM_CD_MAX_SWEEPS", _capi.CD_MAX_SWEEPS), ("GLRM_CD_CONVERGED", _capi.CD_CONVERGED),
                      ("GLRM_CD_SKIPPED", _capi.CD_SKIPPED)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", txt), name
    assert (_capi.CD_MAX_K, _capi.CD_MAX_SWEEPS, _capi.CD_CONVERGED, _capi.CD_SKIPPED) == (64, 256, 1, 2)
    assert "tol = (k * 2^-52) * maxd" in txt and "!(M_aa > tol)" in txt                            # the denominator rule
    assert "rho = g_a + G_aa * x_a" in txt and "d = new - x_a" in txt and "g_i = g_i - G_ia * d" in txt
    assert "rho > h ? (rho - h) / M_aa : rho < -h ? (rho + h) / M_aa : +0.0" in txt                 # the lasso's coordinate
    assert not re.findall(r"#define\s+GLRM_HIP_(?!CD_H\b)\w+", txt)                                 # no name tests/test_knobs.py would take for a knob


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    assert not api.has_cd
    for call in (lambda: api.cd_solve(None, 0, 4), lambda: api.cd_info(None, 0)):
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "glrm_cpu_cd_" in ei.value.message and "include/glrm_hip_cd.h" in ei.value.message


def test_the_names_are_part_of_the_package():
    assert "CdParams" in L.__all__ and issubclass(L.CdParams, L.AbstractParams)
    p = L.CdParams()
    assert (p.max_iter, p.sweeps, p.abs_tol, p.rel_tol, p.device_id) == (100, 4, 1e-5, 1e-4, -1)
    assert L.CdParams(7, sweeps=2).max_iter == 7 and "sweeps=2" in repr(L.CdParams(7, sweeps=2))


# ---- julia/HipGLRMCd.jl

def shim():
    return re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "HipGLRMCd.jl")).read())


JL_C = {"Ptr{Cvoid}": "glrm_handle*", "Int64": "int64_t", "Int32": "int32_t", "Float64": "double", "Ref{Int32}": "int32_t*", "Ref{Int64}": "int64_t*",
        "Ptr{Float64}": "double*", "Cint": "int", "Ref{Float64}": "double*", "Ptr{Int8}": "int8_t*", "Ptr{Int32}": "int32_t*"}


def c_prototypes():
    out = {}
    for header in ("glrm_hip.h", HEADER):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for m in re.finditer(r"\bint\s+(glrm_hip_\w+)\s*\(([^)]*)\)\s*;", txt):
            out[m.group(1)] = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")).replace(" *", "*") for a in m.group(2).split(",")]
    return out


def test_every_ccall_of_the_shim_matches_a_declared_prototype():
    txt, protos = shim(), c_prototypes()
    calls = re.findall(r"ccall\(\s*\(:(glrm_hip_\w+), LIB\)\s*,\s*Cint\s*,\s*\(([^)]*)\)", txt)
    assert len(calls) == len(re.findall(r"\bccall\(", txt)) and calls           # every target is a literal (:symbol, LIB), every result a Cint
    assert {"glrm_hip_cd_solve", "glrm_hip_cd_info"} <= {n for n, _ in calls}
    assert protos["glrm_hip_cd_solve"] == ["glrm_handle*", "int32_t", "int32_t"]
    assert protos["glrm_hip_cd_info"] == ["glrm_handle*", "int32_t", "int64_t*", "int64_t*", "int64_t*", "int8_t*", "int32_t*"]
    for name, jl in calls:
        assert name in protos, name
        jl_args = [a.strip() for a in jl.split(",") if a.strip()]
        assert [JL_C[a] for a in jl_args] == protos[name], (name, jl_args, protos[name])


def test_the_shim_mirrors_the_params_and_the_loop():
    txt = shim()
    assert "module HipGLRMCd" in txt and "export CdParams, hip_cd_solve!, hip_cd_info" in txt
    assert "struct CdParams <: AbstractParams" in txt
    assert "CdParams(; max_iter=100, sweeps=4, abs_tol=0.00001, rel_tol=0.0001, device_id=-1)" in txt
    body = txt[txt.index("function fit!"):]
    assert body.index("hip_cd_solve!(h, 0, p.sweeps)") < body.index("hip_cd_solve!(h, 1, p.sweeps)") < body.index("update_ch!(ch, time() - t, o)")
    assert "i > 10 && (dec < scaled_abs_tol || dec / o < p.rel_tol) && break" in body
    assert "const CD_MAX_K = 64" in txt and "const CD_MAX_SWEEPS = 256" in txt


# ------------------------------------------------------------------ the restatement: two forms

WEIGHTS = (0.5, 1.0, 3.0)
KIND_CASES = ((R.ZERO, 0.0), (R.QUAD, 0.1), (R.ONE, 2.5), (R.NONNEG, 1.0))


def segment(rng, L_, k):
    return rng.standard_normal((L_, k)), rng.standard_normal(L_), rng.choice(WEIGHTS, size=L_)


@pytest.mark.parametrize("k", (1, 5, 20, 64))
def test_the_two_forms_of_the_restatement_agree_bit_for_bit(k):
    """sweeps_vector updates the residual's entries together; sweeps_scalar is the header's loops one scalar at a time.  L = k - 1 makes G
    singular (some ZERO / NONNEG solves then cycle or skip), L = 0 is the empty segment."""
    rng = np.random.default_rng(7300 + k)
    for L_ in (0, max(k - 1, 1), k + 1, 100):
        V, a, w = segment(rng, L_, k)
        if L_ == 100 and k > 2:
            V[:, 2] = 0.0                                                    # G_22 = 0: a skipped coordinate in both forms
        G, b = R.gram(V, a, w)
        x0 = rng.standard_normal(k)
        for kind, gamma in KIND_CASES:
            for sweeps in (1, 3, 40):
                x1, s1, r1 = R.sweeps_vector(G, b, kind, gamma, x0, sweeps)
                x2, s2, r2 = R.sweeps_scalar(G, b, kind, gamma, x0, sweeps)
                assert x1.tobytes() == x2.tobytes() and (s1, r1) == (s2, r2), (k, L_, kind, sweeps)
                assert 1 <= r1 <= sweeps and (r1 == sweeps or s1 & R.CONVERGED)


# ------------------------------------------------------------------ the restatement against the mathematics

def brute_force(G, b, kind, gamma):
    """The minimiser of x'Gx - 2b'x + r(x) by enumeration: every support (NONNEG: x_S > 0 solves G_SS x_S = b_S) or every sign pattern (ONE:
    G_SS x_S = b_S - (gamma / 2) s_S with sign(x_S) = s_S); of the consistent candidates the one of least objective.  -> (x, support)"""
    k = len(b)
    best, best_val, best_S = None, np.inf, None
    patterns = itertools.product((0, 1), repeat=k) if kind == R.NONNEG else itertools.product((-1, 0, 1), repeat=k)
    for pat in patterns:
        s = np.array(pat, dtype=np.float64)
        S = np.flatnonzero(s)
        x = np.zeros(k)
        if len(S):
            rhs = b[S] if kind == R.NONNEG else b[S] - 0.5 * gamma * s[S]
            try:
                x[S] = np.linalg.solve(G[np.ix_(S, S)], rhs)
            except np.linalg.LinAlgError:
                continue
            if not np.all(np.sign(x[S]) == s[S]):
                continue
        val = x @ G @ x - 2.0 * (b @ x) + (gamma * np.sum(np.abs(x)) if kind == R.ONE else 0.0)
        if val < best_val:
            best, best_val, best_S = x, val, S
    return best, best_S


@functools.lru_cache(maxsize=None)
def brute_force_distances():
    """Seeds 0 .. 199, both kinds -> {kind: (worst distance in units, solves that ended by the no-bit-changed rule)}."""
    out = {}
    for kind, gamma in ((R.NONNEG, 1.0), (R.ONE, 2.5)):
        worst, converged = 0.0, 0
        for seed in range(200):
            rng = np.random.default_rng(seed)
            k = int(rng.choice((2, 3, 4, 5)))
            L_ = int(rng.choice((24, 40)))
            V = rng.standard_normal((L_, k))
            a = V @ rng.standard_normal(k) + 0.1 * rng.standard_normal(L_)
            w = rng.choice(WEIGHTS, size=L_)
            x0 = rng.standard_normal(k)
            G, b = R.gram(V, a, w)
            x, status, run = R.sweeps_scalar(G, b, kind, gamma, x0, 512)
            converged += bool(status & R.CONVERGED)
            assert not status & R.SKIPPED and np.all(np.isfinite(x))
            want, S = brute_force(R.full(G), b, kind, gamma)
            assert want is not None
            cond = np.linalg.cond(R.full(G)[np.ix_(S, S)], 2) if len(S) else 1.0
            unit = k * EPS * cond * np.max(np.abs(want))
            dist = np.max(np.abs(x - want))
            worst = max(worst, dist / unit if unit > 0 else (0.0 if dist == 0 else np.inf))
        out[kind] = (worst, converged)
    return out


def test_the_restatement_lands_on_the_brute_force_minimiser():
    """Recipe: seeds 0 .. 199, k from {2, 3, 4, 5}, L from {24, 40}, V standard normal, a = V x* + 0.1 noise, weights from {0.5, 1, 3},
    NonNegConstraint and OneReg(2.5), a standard-normal start, 512 sweeps of the scalar form.  The distance max_a |x_a - brute force| is
    measured in units of k 2^-52 cond_2(G restricted to the brute-force support) max|x|, the first-order bound of the solve the brute
    force itself ran.  Measured here: 2.08 units (NonNegConstraint) and 3.50 units (OneReg: seed 142, rank 2, where rho - h cancels); the cap is 8 units.  Not every solve ends by
    the no-bit-changed rule (here 166 and 138 of 200 did, the rest cycle in the last bit), so the distance is asserted and not the flag."""
    d = brute_force_distances()
    for kind, name in ((R.NONNEG, "NonNegConstraint"), (R.ONE, "OneReg(2.5)")):
        worst, converged = d[kind]
        print(f"{name}: worst distance = {worst:.3g} units; {converged} of 200 solves ended by the no-bit-changed rule")
        assert worst <= 8.0, (name, worst)


# ------------------------------------------------------------------ the rules

def zero_component_segment(k=5, L_=12, seed=3):
    """A segment whose opposing vectors all have component 2 equal to 0.0, so G_22 = 0 and the rest of G is definite.  The values follow a
    positive x* and the start is positive, so that no kind pins another coordinate (NonNegConstraint leaves a coordinate at 0 alone)."""
    rng = np.random.default_rng(seed)
    V, a, w = segment(rng, L_, k)
    V[:, 2] = 0.0
    a = V @ np.array([1.0, 2.0, 0.0, 1.5, 0.5]) + 0.01 * a
    return V, a, w, np.full(k, 0.3)


@pytest.mark.parametrize("kind,gamma", KIND_CASES)
def test_a_zero_denominator_is_skipped_and_the_other_coordinates_move(kind, gamma):
    V, a, w, x0 = zero_component_segment()
    x0[2] = 0.75
    x, status, run = R.solve_segment(V, a, w, kind, gamma, x0, 3, form=R.sweeps_scalar)
    others = [0, 1, 3, 4]
    assert np.all(x[others] != R.start(x0, kind)[others]) and np.all(np.isfinite(x))
    if kind == R.QUAD:                                                       # M_22 = gamma > tol: not skipped, the ridge sends it to 0
        assert not status & R.SKIPPED and x[2] == 0.0
    else:
        assert status & R.SKIPPED
        assert x[2].tobytes() == (np.float64(0.0) if kind == R.ONE else np.float64(0.75)).tobytes()
    # a single opposing vector with component 2 equal to 0.0, hit by every observation: G_22 = 0 and G of rank 1, so coordinate 0 takes up
    # the whole residual and the ones after it may find nothing left to move for
    V1 = np.tile(V[:1], (8, 1))
    x, status, run = R.solve_segment(V1, a[:8], w[:8], kind, gamma, x0, 2, form=R.sweeps_scalar)
    assert bool(status & R.SKIPPED) == (kind != R.QUAD) and x[0] != R.start(x0, kind)[0] and np.all(np.isfinite(x))
    assert kind == R.QUAD or x[2].tobytes() == (np.float64(0.0) if kind == R.ONE else np.float64(0.75)).tobytes()
    # OneReg with scale 0 keeps a skipped coordinate like ZeroReg
    if kind == R.ONE:
        x, status, run = R.solve_segment(V, a, w, R.ONE, 0.0, x0, 3, form=R.sweeps_scalar)
        z = R.solve_segment(V, a, w, R.ZERO, 0.0, x0, 3, form=R.sweeps_scalar)
        assert x.tobytes() == z[0].tobytes() and (status, run) == z[1:] and x[2] == 0.75


@pytest.mark.parametrize("kind,gamma", KIND_CASES)
def test_an_empty_segment_falls_under_the_rules(kind, gamma):
    k = 4
    x0 = np.array([1.5, -2.0, 0.25, -0.0])
    x, status, run = R.solve_segment(np.zeros((0, k)), np.zeros(0), np.zeros(0), kind, gamma, x0, 5, form=R.sweeps_scalar)
    if kind in (R.QUAD, R.ONE):
        assert x.tobytes() == np.zeros(k).tobytes()                          # exactly +0.0
        assert status == (R.CONVERGED if kind == R.QUAD else R.CONVERGED | R.SKIPPED) and run == 2
    else:
        want = x0 if kind == R.ZERO else np.array([1.5, 0.0, 0.25, 0.0])
        assert x.tobytes() == want.tobytes()                                 # the (projected) point, kept
        assert status == R.CONVERGED | R.SKIPPED and run == 1


def test_a_negative_nonneg_start_is_projected_first():
    rng = np.random.default_rng(11)
    V, a, w = segment(rng, 30, 4)
    x0 = np.array([-1.0, 2.0, -0.0, np.nan])
    assert R.start(x0, R.NONNEG).tobytes() == np.array([0.0, 2.0, 0.0, 0.0]).tobytes()
    assert R.start(x0, R.ONE).tobytes() == x0.tobytes()
    G, b = R.gram(V, a, w)
    got = R.sweeps_scalar(G, b, R.NONNEG, 1.0, x0, 2)
    same = R.sweeps_scalar(G, b, R.NONNEG, 1.0, np.array([0.0, 2.0, 0.0, 0.0]), 2)
    assert got[0].tobytes() == same[0].tobytes() and got[1:] == same[1:] and np.all(got[0] >= 0)
    # every coordinate update is the exact minimiser: the objective of the segment never rises, sweep after sweep
    vals = [R.segment_objective(V, a, w, R.NONNEG, 1.0, R.sweeps_scalar(G, b, R.NONNEG, 1.0, x0, s)[0]) for s in range(1, 8)]
    assert all(v1 <= v0 * (1 + 64 * EPS) for v0, v1 in zip(vals, vals[1:])), vals


# ------------------------------------------------------------------ the driver on the host engine

def host():
    return R.HostEngine(O.oracle_api())


def nnmf_model(m=60, n=40, k=4, seed=5, negative_start=False, rx=None, ry=None):
    rng = np.random.default_rng(seed)
    A = rng.random((m, k)) @ rng.random((k, n)) + 0.01 * rng.random((m, n))
    flat = rng.permutation(m * n)[: m * n // 2]                              # half the entries observed
    obs = (np.sort(flat) // n, np.sort(flat) % n)
    X, Y = rng.random((k, m)), rng.random((k, n))
    if negative_start:
        X[1, 3] = -0.5
    g = L.GLRM(A, L.QuadLoss(), L.NonNegConstraint() if rx is None else rx, L.NonNegConstraint() if ry is None else ry, k, obs=obs, X=X, Y=Y)
    return g, len(flat)


def test_fit_with_cdparams_descends_on_an_nnmf():
    g, nobs = nnmf_model()
    api = host()
    X0, Y0 = g.X.copy(order="F"), g.Y.copy(order="F")
    X, Y, ch = L.fit_b(g, L.CdParams(max_iter=8, sweeps=3), engine=api, verbose=False)
    try:
        obj = np.array(ch.objective)
        T = nobs + (g.m + g.n) * g.k
        assert len(obj) == 9 and ch.name == "CdGLRM" and np.all(np.isfinite(obj))
        assert np.all(obj[1:] <= obj[:-1] * (1 + 2 * T * EPS)), obj
        assert obj[-1] < 0.05 * obj[0], (obj[0], obj[-1])
        assert np.all(X >= 0) and np.all(Y >= 0)
        assert len(ch.times) == len(obj) and np.all(np.diff(ch.times) >= 0) and ch.times[0] == 0
        # the iterates are the restatement's, bit for bit, and the kept counts are the last solves'
        pa = g.problem_arrays()
        Xr, Yr = X0, Y0
        for _ in range(8):
            Xr, sx, rx_ = R.solve_side(pa, 0, Xr, Yr, 3)
            Yr, sy, ry_ = R.solve_side(pa, 1, Xr, Yr, 3)
        assert X.tobytes() == np.asfortranarray(Xr).tobytes() and Y.tobytes() == np.asfortranarray(Yr).tobytes()
        assert g._cd_info == {0: R.counts(sx, rx_), 1: R.counts(sy, ry_)}
        assert g._cd_info[0]["sweeps_total"] <= 3 * g.m and g._cd_info[0]["skipped"] == 0
        assert obj[-1] == pytest.approx(api.objective(g._handle_cache[1], np.asfortranarray(X), np.asfortranarray(Y), True), rel=1e-12)
    finally:
        g.close()


def test_a_negative_start_is_infinite_and_the_first_iteration_is_finite():
    g, nobs = nnmf_model(negative_start=True)
    ch = L.fit_b(g, L.CdParams(max_iter=3), engine=host(), verbose=False)[2]
    g.close()
    obj = np.array(ch.objective)
    T = nobs + (g.m + g.n) * g.k
    assert obj[0] == np.inf and np.all(np.isfinite(obj[1:])) and len(obj) == 4
    assert np.all(obj[2:] <= obj[1:-1] * (1 + 2 * T * EPS)), obj
    assert np.all(g.X >= 0)


def test_a_lasso_model_descends_and_zeroes_coordinates():
    g, nobs = nnmf_model(seed=8, rx=L.OneReg(0.5), ry=L.QuadReg(0.1))
    ch = L.fit_b(g, L.CdParams(max_iter=6), engine=host(), verbose=False)[2]
    g.close()
    obj = np.array(ch.objective)
    T = nobs + (g.m + g.n) * g.k
    assert np.all(obj[1:] <= obj[:-1] * (1 + 2 * T * EPS)), obj
    assert np.any(g.X == 0.0) and np.any(g.X != 0.0)


def test_the_stopping_rule_and_its_bookkeeping():
    g, nobs = nnmf_model(seed=6)
    nnz = float(g._rowptr[-1])
    assert nnz == nobs
    p = L.CdParams(max_iter=100, sweeps=2, abs_tol=1e-5, rel_tol=1e-3)
    ch = L.fit_b(g, p, engine=host(), verbose=False)[2]
    g.close()
    obj = ch.objective
    last = len(obj) - 1
    assert 11 <= last < 100                                              # never before iteration 11; this model stops long before 100
    for i in range(1, last):
        assert not _should_stop(i, obj[i - 1], obj[i], p.abs_tol * nnz, p.rel_tol), i
    assert _should_stop(last, obj[last - 1], obj[last], p.abs_tol * nnz, p.rel_tol)
    # max_iter ends a run the rule has not ended; max_iter = 0 records the start alone and solves nothing
    g2, _ = nnmf_model(seed=6)
    assert len(L.fit_b(g2, L.CdParams(max_iter=4), engine=host(), verbose=False)[2].objective) == 5
    g2.close()
    g3, _ = nnmf_model(seed=6)
    X0 = g3.X.copy()
    ch0 = L.fit_b(g3, L.CdParams(max_iter=0), engine=host(), verbose=False)[2]
    g3.close()
    assert len(ch0.objective) == 1 and np.array_equal(g3.X, X0) and not hasattr(g3, "_cd_info")


def refused_before_create(build, words, code=_capi.ERR_UNSUPPORTED):
    api = host()
    with pytest.raises(_capi.GLRMError) as ei:
        build(api)
    assert ei.value.code == code and "glrm_hip_cd_solve" in ei.value.message, ei.value.message
    assert code != _capi.ERR_UNSUPPORTED or "include/glrm_hip_cd.h" in ei.value.message
    for w in words:
        assert w in ei.value.message, (w, ei.value.message)
    assert api.created == 0                                               # before a handle exists


def test_a_model_the_engine_would_refuse_is_refused_on_the_host_before_create():
    rng = np.random.default_rng(9)
    A = rng.standard_normal((8, 6))

    def fit_of(losses, rx, ry, k=2, params=None, **kw):
        return lambda api: L.fit_b(L.GLRM(A, losses, rx, ry, k, rng=np.random.default_rng(1), **kw), params or L.CdParams(max_iter=2), engine=api, verbose=False)
    q, nn = L.QuadReg(0.1), L.NonNegConstraint()
    refused_before_create(fit_of(L.HuberLoss(), nn, nn), ["column 0 has loss kind 2", "needs QuadLoss"])
    refused_before_create(fit_of([L.QuadLoss()] * 5 + [L.L1Loss()], q, nn), ["column 5 has loss kind 1"])
    refused_before_create(fit_of(L.QuadLoss(), L.QuadConstraint(1.0), q), ["rx[0] has regularizer kind 5", "plain ZeroReg (kind 0), QuadReg (kind 1), OneReg (kind 2) or NonNegConstraint (kind 3)"])
    refused_before_create(fit_of(L.QuadLoss(), nn, L.UnitOneSparseConstraint()), ["ry[0] has regularizer kind 4"])
    refused_before_create(fit_of(L.QuadLoss(), q, [L.OneReg(0.1)] * 3 + [L.OneReg(-1.0)] + [L.OneReg(0.1)] * 2), ["ry[3] is OneReg with scale -1"])
    refused_before_create(fit_of(L.QuadLoss(), L.QuadReg(-0.5), nn), ["rx[0] is QuadReg with scale -0.5"])
    refused_before_create(fit_of(L.QuadLoss(), nn, nn, offset=True), ["rx[0]", "wrap 1"])
    refused_before_create(lambda api: L.fit_b(L.GLRM(rng.standard_normal((70, 66)), L.QuadLoss(), nn, nn, 65, rng=np.random.default_rng(1)), L.CdParams(), engine=api, verbose=False),
                          ["rank k = 65 is above GLRM_CD_MAX_K = 64"])
    refused_before_create(fit_of(L.QuadLoss(), nn, nn, params=L.CdParams(sweeps=0)), ["sweeps must be in [1, GLRM_CD_MAX_SWEEPS = 256], got 0"], _capi.ERR_INVALID)
    refused_before_create(fit_of(L.QuadLoss(), nn, nn, params=L.CdParams(sweeps=257)), ["got 257"], _capi.ERR_INVALID)
    # what AlsParams refuses word for word, CdParams takes
    api = host()
    ch = fit_of(L.QuadLoss(), nn, L.OneReg(0.1))(api)[2]
    assert api.created == 1 and len(ch.objective) == 3
