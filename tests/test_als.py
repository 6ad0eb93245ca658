"""The ALS extension (include/glrm_hip_als.h) without a GPU.

  * The built libraries export what the header declares, the boundary header still declares 37 symbols, an engine without the extension is
    refused by name, and the Julia shim (julia/HipGLRMAls.jl, which cannot run here) is held to the C prototypes.
  * The numpy restatement (tests/als_ref.py) -- the reference of tests/test_gpu_als.py -- is held to a DERIVED backward-error bound:
    entrywise |(G + gamma I) x - b| <= (L + 3k + 2) 2^-52 (k (|G|_abs + gamma I) |x| + |b|_abs), the dot-product bound for the L-term sums of
    the Gram matrix and the right-hand side plus Higham's bound for a Cholesky solve (als_ref.residual_ratio), residuals in np.longdouble.
    Measured here over every solved case: at most 0.05 of the bound.  Every status is asserted: a solver that keeps everything cannot pass.
  * The driver (fit_b with AlsParams, transform(exact=True)) runs on the CPU oracle wrapped by als_ref.HostEngine.  Its history is held to
    obj[i] <= obj[i-1] (1 + nnz 2^-52): an exact half-step cannot raise the objective, and the slack is the summation error of the nnz
    non-negative terms of the recorded sum.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import als_ref as R
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.fit import _should_stop
from test_abi import PKG, ROOT, declared, ensure_built

HEADER = "glrm_hip_als.h"


# ------------------------------------------------------------------ the boundary

def test_libraries_export_every_symbol_the_header_declares():
    ensure_built()
    names = declared(HEADER, "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.ALS_SYMBOLS) and len(names) == 2
    assert not set(_capi.ALS_SYMBOLS) & set(_capi.ABI_SYMBOLS)          # outside the 37-symbol boundary
    assert len(declared("glrm_hip.h", "glrm_hip_")) == 37 == len(_capi.ABI_SYMBOLS)
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)


def test_the_header_states_the_limits_and_the_rules():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    assert re.search(r"#define\s+GLRM_ALS_MAX_K\s+64\b", txt) and _capi.ALS_MAX_K == 64
    for name, val in (("GLRM_ALS_SOLVED", _capi.ALS_SOLVED), ("GLRM_ALS_KEPT_SHORT", _capi.ALS_KEPT_SHORT), ("GLRM_ALS_KEPT_PIVOT", _capi.ALS_KEPT_PIVOT)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", txt), name
    assert "tol = (k * 2^-52) * maxd" in txt and "!(s > tol)" in txt              # the pivot rule
    assert "gamma == 0 with L < k is GLRM_ALS_KEPT_SHORT" in txt                   # the short rule
    assert "2 * rx[i].scale * I" in txt                                            # what the streaming file solves instead
    assert not re.findall(r"#define\s+GLRM_HIP_(?!ALS_H\b)\w+", txt)               # no name tests/test_knobs.py would take for a knob


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    assert not api.has_als
    for call in (lambda: api.als_solve(None, 0), lambda: api.als_info(None, 0)):
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "glrm_cpu_als_" in ei.value.message and "include/glrm_hip_als.h" in ei.value.message


def test_the_names_are_part_of_the_package():
    assert "AlsParams" in L.__all__ and issubclass(L.AlsParams, L.AbstractParams)
    p = L.AlsParams()
    assert (p.max_iter, p.abs_tol, p.rel_tol, p.device_id) == (100, 1e-5, 1e-4, -1)
    assert "exact" in L.transform.__code__.co_varnames


# ---- julia/HipGLRMAls.jl

def shim():
    return re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "HipGLRMAls.jl")).read())


JL_C = {"Ptr{Cvoid}": "glrm_handle*", "Int64": "int64_t", "Int32": "int32_t", "Float64": "double", "Ref{Int32}": "int32_t*", "Ref{Int64}": "int64_t*",
        "Ptr{Float64}": "double*", "Cint": "int", "Ref{Float64}": "double*", "Ptr{Int8}": "int8_t*"}


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
    assert {"glrm_hip_als_solve", "glrm_hip_als_info"} <= {n for n, _ in calls}
    for name, jl in calls:
        assert name in protos, name
        jl_args = [a.strip() for a in jl.split(",") if a.strip()]
        assert [JL_C[a] for a in jl_args] == protos[name], (name, jl_args, protos[name])


def test_the_shim_mirrors_the_params_and_the_loop():
    txt = shim()
    assert "module HipGLRMAls" in txt and "export AlsParams, hip_als_solve!, hip_als_info" in txt
    assert "struct AlsParams <: AbstractParams" in txt
    assert "AlsParams(; max_iter=100, abs_tol=0.00001, rel_tol=0.0001, device_id=-1)" in txt
    body = txt[txt.index("function fit!"):]
    assert body.index("hip_als_solve!(h, 0)") < body.index("hip_als_solve!(h, 1)") < body.index("update_ch!(ch, time() - t, o)")
    assert "i > 10 && (dec < scaled_abs_tol || dec / o < p.rel_tol) && break" in body
    assert "const ALS_MAX_K = 64" in txt


# ------------------------------------------------------------------ the restatement

KS = (1, 5, 20, 32, 64)
WEIGHTS = (0.5, 1.0, 3.0)


def lengths(k):
    return sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, 100, 300})


def segment(rng, L_, k):
    return rng.standard_normal((L_, k)), rng.standard_normal(L_), rng.choice(WEIGHTS, size=L_)


@pytest.mark.parametrize("k", KS)
def test_the_restatement_meets_the_backward_error_bound_and_keeps_what_the_rules_name(k):
    rng = np.random.default_rng(7000 + k)
    worst = 0.0
    for L_ in lengths(k):
        V, a, w = segment(rng, L_, k)
        for gamma in (0.1, 0.0):
            st, x = R.solve_segment(V, a, w, gamma)
            want = R.KEPT_SHORT if (gamma == 0.0 and L_ < k) else R.SOLVED
            assert st == want, (k, L_, gamma, st)
            if st == R.SOLVED:
                assert x.shape == (k,) and np.all(np.isfinite(x))
                ratio = R.residual_ratio(V, a, w, gamma, x)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (k, L_, gamma, ratio)
                if L_ == 0:
                    assert x.tobytes() == np.zeros(k).tobytes()         # exactly +0.0, no special case
            else:
                assert x is None
    print(f"k={k}: worst residual / bound = {worst:.3g}")


@pytest.mark.parametrize("k", KS)
def test_the_two_forms_of_the_factorisation_agree_bit_for_bit(k):
    """cholesky_solve deals the header's operations out by rows; cholesky_solve_scalar is the header's loops one scalar at a time."""
    rng = np.random.default_rng(7100 + k)
    for L_ in (k, k + 1, 100):
        V, a, w = segment(rng, L_, k)
        for gamma in (0.1, 0.0):
            G, b = R.gram(V, a, w)
            M = G.copy()
            for d in range(k):
                M[d, d] = G[d, d] + gamma
            s1, x1 = R.cholesky_solve(M, b)
            s2, x2 = R.cholesky_solve_scalar(M, b)
            assert s1 == s2 == R.SOLVED and x1.tobytes() == x2.tobytes(), (k, L_, gamma)


def test_a_rank_deficient_segment_with_enough_observations_fails_a_pivot():
    rng = np.random.default_rng(71)
    three = rng.standard_normal((3, 8))
    V = three[np.arange(12) % 3]
    a, w = rng.standard_normal(12), rng.choice(WEIGHTS, size=12)
    assert R.solve_segment(V, a, w, 0.0) == (R.KEPT_PIVOT, None)
    st, x = R.solve_segment(V, a, w, 0.1)                                # the penalty makes it definite
    assert st == R.SOLVED and R.residual_ratio(V, a, w, 0.1, x) <= 1.0
    assert R.solve_segment(np.zeros((9, 8)), a[:9], w[:9], 0.0)[0] == R.KEPT_PIVOT   # max diagonal 0: everything fails
    bad = V.copy(); bad[5, 2] = np.nan
    assert R.solve_segment(bad, a, w, 0.1)[0] == R.KEPT_PIVOT            # a NaN fails the rule


# ------------------------------------------------------------------ the driver on the host engine

def host():
    return R.HostEngine(O.oracle_api())


def lowrank_model(gamma=1e-9, m=30, n=20, k=3, seed=5, **kw):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k)) @ rng.standard_normal((k, n))
    return L.GLRM(A, L.QuadLoss(), L.QuadReg(gamma), L.QuadReg(gamma), k, rng=rng, **kw), A


def test_fit_with_alsparams_descends_to_the_noiseless_model():
    g, A = lowrank_model()
    api = host()
    X0, Y0 = g.X.copy(order="F"), g.Y.copy(order="F")
    X, Y, ch = L.fit_b(g, L.AlsParams(max_iter=30), engine=api, verbose=False)
    try:
        obj = np.array(ch.objective)
        nnz = g.m * g.n
        assert len(obj) >= 12 and ch.name == "AlsGLRM"
        assert np.all(obj[1:] <= obj[:-1] * (1 + nnz * 2.0 ** -52)), obj
        assert obj[-1] < 1e-6 * obj[0], (obj[0], obj[-1])
        assert g._als_info == {0: dict(solved=g.m, kept_short=0, kept_pivot=0), 1: dict(solved=g.n, kept_short=0, kept_pivot=0)}
        assert len(ch.times) == len(obj) and np.all(np.diff(ch.times) >= 0) and ch.times[0] == 0
        assert np.max(np.abs(X.T @ Y - A)) < 1e-4 * np.max(np.abs(A))
        # the iterates are the restatement's, bit for bit
        pa = g.problem_arrays()
        Xr, Yr = X0, Y0
        for _ in range(len(obj) - 1):
            Xr = R.solve_side(pa, 0, Xr, Yr)[0]
            Yr = R.solve_side(pa, 1, Xr, Yr)[0]
        assert X.tobytes() == np.asfortranarray(Xr).tobytes() and Y.tobytes() == np.asfortranarray(Yr).tobytes()
        # the recorded values are the full objective
        assert obj[-1] == pytest.approx(api.objective(g._handle_cache[1], np.asfortranarray(X), np.asfortranarray(Y), True), rel=1e-12)
    finally:
        g.close()


def test_the_stopping_rule_and_its_bookkeeping():
    g, _ = lowrank_model(gamma=0.5, seed=6)
    nnz = float(g._rowptr[-1])
    p = L.AlsParams(max_iter=100, abs_tol=1e-5, rel_tol=1e-4)
    ch = L.fit_b(g, p, engine=host(), verbose=False)[2]
    g.close()
    obj = ch.objective
    last = len(obj) - 1
    assert 11 <= last < 100                                              # never before iteration 11, and this model converges long before 100
    for i in range(1, last):
        assert not _should_stop(i, obj[i - 1], obj[i], p.abs_tol * nnz, p.rel_tol), i
    assert _should_stop(last, obj[last - 1], obj[last], p.abs_tol * nnz, p.rel_tol)
    # max_iter ends a run the rule has not ended; max_iter = 0 records the start alone and solves nothing
    g2, _ = lowrank_model(gamma=0.5, seed=6)
    assert len(L.fit_b(g2, L.AlsParams(max_iter=4), engine=host(), verbose=False)[2].objective) == 5
    g2.close()
    g3, _ = lowrank_model(gamma=0.5, seed=6)
    X0 = g3.X.copy()
    ch0 = L.fit_b(g3, L.AlsParams(max_iter=0), engine=host(), verbose=False)[2]
    g3.close()
    assert len(ch0.objective) == 1 and np.array_equal(g3.X, X0) and not hasattr(g3, "_als_info")


def test_als_starts_from_a_zero_y():
    g, _ = lowrank_model(gamma=0.1, seed=8)
    g.Y[...] = 0.0
    ch = L.fit_b(g, L.AlsParams(max_iter=5), engine=host(), verbose=False)[2]
    g.close()
    assert ch.objective[1] <= ch.objective[0] and np.all(np.isfinite(ch.objective))
    # X solves to exactly 0 against Y == 0 (ridge), then Y against X == 0: ZeroReg rows would be kept instead
    g2 = L.GLRM(np.ones((6, 5)), L.QuadLoss(), L.ZeroReg(), L.QuadReg(0.1), 2, Y=np.zeros((2, 5)), rng=np.random.default_rng(0))
    L.fit_b(g2, L.AlsParams(max_iter=1), engine=host(), verbose=False)
    g2.close()
    assert g2._als_info[0] == dict(solved=0, kept_short=0, kept_pivot=6)


def refused_before_create(build, words, fit=True):
    api = host()
    with pytest.raises(_capi.GLRMError) as ei:
        build(api)
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_als.h" in ei.value.message, ei.value.message
    for w in words:
        assert w in ei.value.message, (w, ei.value.message)
    assert api.created == 0                                               # before a handle exists


def test_a_model_the_engine_would_refuse_is_refused_on_the_host_before_create():
    rng = np.random.default_rng(9)
    A = rng.standard_normal((8, 6))

    def fit_of(losses, rx, ry, k=2, **kw):
        return lambda api: L.fit_b(L.GLRM(A, losses, rx, ry, k, rng=np.random.default_rng(1), **kw), L.AlsParams(max_iter=2), engine=api, verbose=False)
    q = L.QuadReg(0.1)
    refused_before_create(fit_of(L.HuberLoss(), q, q), ["column 0 has loss kind 2", "needs QuadLoss"])
    refused_before_create(fit_of([L.QuadLoss()] * 5 + [L.L1Loss()], q, q), ["column 5 has loss kind 1"])
    refused_before_create(fit_of(L.QuadLoss(), L.NonNegConstraint(), q), ["rx[0] has regularizer kind 3", "plain QuadReg"])
    refused_before_create(fit_of(L.QuadLoss(), q, L.OneReg(0.1)), ["ry[0] has regularizer kind 2"])
    refused_before_create(fit_of(L.QuadLoss(), q, [L.QuadReg(0.1)] * 3 + [L.QuadReg(-1.0)] + [L.QuadReg(0.1)] * 2), ["ry[3] is QuadReg with scale -1"])
    refused_before_create(fit_of(L.QuadLoss(), q, q, offset=True), ["rx[0]", "wrap 1"])
    refused_before_create(fit_of(L.QuadLoss(), L.QuadConstraint(1.0), q), ["rx[0] has regularizer kind 5"])
    refused_before_create(lambda api: L.fit_b(L.GLRM(rng.standard_normal((70, 66)), L.QuadLoss(), q, q, 65, rng=np.random.default_rng(1)), L.AlsParams(), engine=api, verbose=False),
                          ["rank k = 65 is above GLRM_ALS_MAX_K = 64"])
    # transform(exact=True) looks at the new rows' side only: a OneReg on the columns is not in the system
    fitted = L.GLRM(A, L.QuadLoss(), q, L.OneReg(0.1), 2, rng=np.random.default_rng(1))
    api = host()
    Xn, ch = L.transform(fitted, A[:3], exact=True, api=api)
    assert api.created == 1 and Xn.shape == (2, 3) and len(ch.objective) == 2
    refused_before_create(lambda api: L.transform(fitted, A[:3], exact=True, rx=L.NonNegConstraint(), api=api), ["rx[0] has regularizer kind 3"])
    refused_before_create(lambda api: L.transform(L.GLRM(A, L.HuberLoss(), q, q, 2, rng=np.random.default_rng(1)), A[:3], exact=True, api=api), ["needs QuadLoss"])


def test_alsparams_without_exact_is_not_a_transform_params():
    g, _ = lowrank_model()
    with pytest.raises(TypeError):
        L.transform(g, g.A[:2], L.AlsParams(), api=host())               # without exact=True the driver is the prox-gradient one


def test_transform_exact_is_one_solve_of_the_new_rows():
    g, A = lowrank_model(gamma=1e-9, seed=12)
    api = host()
    L.fit_b(g, L.AlsParams(max_iter=30), engine=api, verbose=False)
    g.close()
    rng = np.random.default_rng(13)
    A_new = rng.standard_normal((7, g.k)) @ g.Y                           # noiseless rows of the fitted model
    X0 = rng.standard_normal((g.k, 7))
    Xn, ch = L.transform(g, A_new, L.AlsParams(), exact=True, X0=X0, api=api)
    new = L.GLRM(A_new, L.QuadLoss(), L.QuadReg(1e-9), L.QuadReg(1e-9), g.k, X=X0, Y=g.Y)
    ref, status = R.solve_side(new.problem_arrays(), 0, np.asfortranarray(X0), np.asfortranarray(g.Y))
    assert np.all(status == R.SOLVED) and Xn.tobytes() == np.asfortranarray(ref).tobytes()
    assert len(ch.objective) == 2 and ch.objective[1] < 1e-6 * ch.objective[0] and ch.name == "AlsGLRM-transform"
    assert np.max(np.abs(L.inverse_transform(g, Xn) - A_new)) < 1e-6 * np.max(np.abs(A_new))
    # the default path is what it was: the prox-gradient driver, same signature
    Xp, chp = L.transform(g, A_new, L.HipProxGradParams(max_iter=3), X0=X0, api=O.oracle_api())
    assert len(chp.objective) == 4 and chp.name == "ProxGradGLRM-transform"
