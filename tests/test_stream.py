"""The streaming extension (include/glrm_hip_stream.h) without a GPU.

  * The built libraries export what the header declares, the boundary header still declares 37 symbols, an engine without the extension is
    refused by name, and the Julia shim (julia/HipGLRMStream.jl, which cannot run here) is held to the C prototypes.
  * glrm_hip_stream_plan is pure host code: it runs here, through ctypes, against the 10-line plan of tests/stream_ref.py, and the plan's
    two properties are asserted on their own (no two rows of a level share a written column; no reader shares a level with a writer).
  * The numpy restatement of a row (stream_ref.stream_rows) -- the reference of tests/test_gpu_stream.py -- is held to als_ref's DERIVED
    backward-error bound with gamma replaced by 2 gamma, and every status is asserted.
  * The restatement against a literal transcription of src/algorithms/quad_streaming.jl (stream_ref.literal): the two differ by LAPACK's
    order of operations and by p = c^d in place of d divisions.  See test_the_restatement_follows_the_literal_loop for the measured
    difference and the factor.
  * The drivers (streaming_fit, streaming_impute_at, streaming_impute) run on the CPU oracle wrapped by stream_ref.HostEngine.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import als_ref as AR
import lowrankmodels.jl_amd as L
import oracle as O
import stream_ref as S
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd import stream as stream_mod
from test_abi import PKG, ROOT, declared, ensure_built

HEADER = "glrm_hip_stream.h"
FIRST = 16
PATTERNS = ((160, 64, 3, 1), (200, 256, 4, 1), (96, 24, 24, 1))     # m, n, observations per row, seed


# ------------------------------------------------------------------ the boundary

def test_libraries_export_every_symbol_the_header_declares():
    ensure_built()
    names = declared(HEADER, "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.STREAM_SYMBOLS) and len(names) == 3
    assert not set(_capi.STREAM_SYMBOLS) & set(_capi.ABI_SYMBOLS)       # outside the 37-symbol boundary
    assert len(declared("glrm_hip.h", "glrm_hip_")) == 37 == len(_capi.ABI_SYMBOLS)
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)


def test_the_header_states_the_rules():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    assert re.search(r"#define\s+GLRM_STREAM_MAX_K\s+64\b", txt) and _capi.STREAM_MAX_K == 64
    for rule in ("L = 1 + max(lastw[j], lastr[j] over the row's observed columns; lastw[j] over its query columns)",
                 "lastw[j] = L for each observed column", "lastr[j] = max(lastr[j], L) for each query column",
                 "With sequential = 1, row first + t has level t + 1",
                 "c = 1 + ((2 * stepsize) * (double)interval) * sy",
                 "D(i) = floor((i1 - 1) / interval) - floor(first / interval)",
                 "p = c, then p = p * c repeated d - 1 times", "c == 1.0 skips all of it",
                 "M_aa = G_aa + 2 * gamma", "NOT written back", "y_a = y_a - (stepsize * r_t) * x_a",
                 "objective = NaN", "floor(m / interval) - floor(first / interval)", "p may overflow to +Inf",
                 "no flags,", "no spinning", "no cooperative launch", "no graph capture"):
        assert rule in txt, rule
    assert not re.findall(r"#define\s+GLRM_HIP_(?!STREAM_H\b)\w+", txt)           # no name tests/test_knobs.py would take for a knob
    als = open(os.path.join(ROOT, "include", "glrm_hip_als.h")).read()
    assert "is not reproduced" not in als and "glrm_hip_stream.h" in als


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    assert not api.has_stream
    calls = (lambda: api.stream_rows(None, 4, 1, 0.1, 1), lambda: api.stream_info(None),
             lambda: api.stream_plan(2, 2, 1, np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    for call in calls:
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "glrm_cpu_stream_" in ei.value.message and "include/glrm_hip_stream.h" in ei.value.message


def test_the_names_are_part_of_the_package():
    for name in ("StreamingParams", "keep_rows", "streaming_fit", "streaming_impute", "streaming_impute_at"):
        assert name in L.__all__, name
    assert issubclass(L.StreamingParams, L.AbstractParams)
    p = L.StreamingParams()
    assert (p.T0, p.stepsize, p.Y_update_interval, p.device_id, p.sequential) == (1000, 1 / 1000, 10, -1, False)
    assert L.StreamingParams(50).stepsize == 1 / 50 and L.StreamingParams(50, stepsize=0.3).stepsize == 0.3
    g = L.GLRM(np.ones((4, 3)), L.QuadLoss(), L.QuadReg(0.1), L.QuadReg(0.1), 2, rng=np.random.default_rng(0))
    with pytest.raises(TypeError):
        L.fit_b(g, L.StreamingParams(2), engine=O.oracle_api(), verbose=False)   # the reference has no fit! method for StreamingParams
    assert "m x n" in L.streaming_impute.__doc__


# ---- julia/HipGLRMStream.jl

def shim():
    return re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "HipGLRMStream.jl")).read())


JL_C = {"Ptr{Cvoid}": "glrm_handle*", "Int64": "int64_t", "Int32": "int32_t", "Float64": "double", "Ref{Int64}": "int64_t*", "Ptr{Int64}": "int64_t*",
        "Ptr{Int32}": "int32_t*", "Ptr{Float64}": "double*", "Ref{Float64}": "double*", "Ptr{Int8}": "int8_t*", "Cint": "int"}


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
    assert {"glrm_hip_stream_plan", "glrm_hip_stream_rows", "glrm_hip_stream_info"} <= {n for n, _ in calls}
    for name, jl in calls:
        assert name in protos, name
        jl_args = [a.strip() for a in jl.split(",") if a.strip()]
        assert [JL_C[a] for a in jl_args] == protos[name], (name, jl_args, protos[name])


def test_the_shim_mirrors_the_loop():
    txt = shim()
    assert "module HipGLRMStream" in txt and "export hip_stream_plan, hip_stream_rows!, hip_stream_info, hip_streaming_fit!, hip_streaming_impute_at" in txt
    body = txt[txt.index("function stream_pass!"):]
    assert body.index("keep_rows(glrm, p.T0)") < body.index("init_svd!(init_glrm)") < body.index("hip_stream_rows!(h, m, p.T0, p.stepsize, p.Y_update_interval")
    assert "append!(ch.objective, objective)" in txt and "const STREAM_MAX_K = 64" in txt
    assert not re.search(r"(?<![\w_])fit!\(", txt)                                # no fit! method, as in the reference


# ------------------------------------------------------------------ the plan

def hip():
    ensure_built()
    return _capi.hip_api()


def same_plan(m, n, first, lists, qlists=None, sequential=False):
    ptr, idx = S.csr(lists)
    qptr, qcol = (None, None) if qlists is None else S.csr(qlists)
    want = S.plan(m, n, first, ptr, idx, qptr, qcol, sequential)
    got = hip().stream_plan(m, n, first, ptr, idx, qptr, qcol, sequential)
    assert np.array_equal(got["level"], want["level"]), (got["level"], want["level"])
    assert {f: got[f] for f in ("nlevels", "nlaunches", "max_width", "dup_rows")} == {f: want[f] for f in ("nlevels", "nlaunches", "max_width", "dup_rows")}
    return want, ptr, idx, qptr, qcol


def check_properties(first, level, lists, qlists=None):
    """no two rows of one level share a written column; no reader shares a level with a writer of its column; and a later row that
    touches a column an earlier row wrote (or writes one an earlier row read) has a higher level"""
    rows = len(level)
    for l in np.unique(level):
        members = np.flatnonzero(level == l)
        written = [set(np.asarray(lists[first + r]).tolist()) for r in members]
        allw = [c for w in written for c in w]
        assert len(allw) == len(set(allw)), ("two writers of a column in level", l)
        if qlists is not None:
            for a, r in enumerate(members):
                for b, w in enumerate(written):
                    if a != b:
                        assert not set(np.asarray(qlists[first + r]).tolist()) & w, ("a reader beside a writer in level", l)
    lastw, lastr = {}, {}
    for r in range(rows):
        w = set(np.asarray(lists[first + r]).tolist())
        q = set() if qlists is None else set(np.asarray(qlists[first + r]).tolist())
        for c in w:
            assert level[r] > max(lastw.get(c, 0), lastr.get(c, 0))
        for c in q:
            assert level[r] > lastw.get(c, 0)
        for c in w:
            lastw[c] = level[r]
        for c in q:
            lastr[c] = max(lastr.get(c, 0), level[r])


@pytest.mark.parametrize("seed", range(4))
def test_the_plan_of_random_lists_with_empty_rows_dup_rows_and_queries(seed):
    rng = np.random.default_rng(300 + seed)
    m, n, first = 90, 40, int(rng.integers(1, 20))
    lists = [rng.choice(n, int(rng.integers(0, 6)), replace=False) for _ in range(m)]
    for i in rng.choice(np.arange(first, m), 6, replace=False):               # dup rows: a column named twice
        if len(lists[i]):
            lists[i] = np.concatenate([lists[i], lists[i][:1]])
    lists[first + 1] = np.zeros(0, dtype=np.int64)                                # an empty row
    want, *_ = same_plan(m, n, first, lists)
    assert want["dup_rows"] >= 1 and want["level"][1] == 1
    check_properties(first, want["level"], lists)
    # queries that name a column the row BEFORE writes, and one the row AFTER writes
    qlists = [np.zeros(0, dtype=np.int64)] * m
    for i in range(first + 1, m - 1):
        qlists[i] = np.unique(np.concatenate([lists[i - 1][:1], lists[i + 1][:1], rng.choice(n, 2)])).astype(np.int64)
    wq, *_ = same_plan(m, n, first, lists, qlists)
    check_properties(first, wq["level"], lists, qlists)
    assert np.all(wq["level"] >= want["level"]) and np.any(wq["level"] > want["level"])
    ws, *_ = same_plan(m, n, first, lists, qlists, sequential=True)
    assert np.array_equal(ws["level"], np.arange(1, m - first + 1)) and ws["nlaunches"] == 1 and ws["max_width"] == 1


def test_a_fully_dense_pattern_is_one_chain_and_first_equal_m_is_empty():
    m, n = 40, 7
    lists = [np.arange(n)] * m
    want, *_ = same_plan(m, n, FIRST, lists)
    assert want["nlevels"] == m - FIRST and want["nlaunches"] == 1 and want["max_width"] == 1
    empty, *_ = same_plan(m, n, m, lists)
    assert (empty["nlevels"], empty["nlaunches"], empty["max_width"], len(empty["level"])) == (0, 0, 0, 0)
    # a chain, a wide level, a chain: three launches
    lists = [np.array([0])] * (FIRST + 3) + [np.array([0, 1, 2, 3])] + [np.array([c]) for c in (1, 2, 3)] + [np.array([1, 2]), np.array([1])]
    mixed, *_ = same_plan(len(lists), n, FIRST, lists)
    assert list(mixed["level"]) == [1, 2, 3, 4, 5, 5, 5, 6, 7] and mixed["nlaunches"] == 3 and mixed["max_width"] == 3, mixed


def test_the_plan_refuses_what_it_cannot_index():
    api = hip()
    ptr, idx = S.csr([np.array([0, 1]), np.array([5])])
    with pytest.raises(_capi.GLRMError) as ei:
        api.stream_plan(2, 3, 0, ptr, idx)
    assert ei.value.code == _capi.ERR_INVALID and "column 5" in ei.value.message
    with pytest.raises(_capi.GLRMError) as ei:
        api.stream_plan(2, 6, 0, ptr, idx, np.array([0, 1, 1]), np.array([9], dtype=np.int32))
    assert ei.value.code == _capi.ERR_INVALID and "column 9" in ei.value.message
    with pytest.raises(_capi.GLRMError) as ei:
        api.stream_plan(2, 6, 3, ptr, idx)
    assert ei.value.code == _capi.ERR_INVALID and "first" in ei.value.message


@pytest.mark.parametrize("case", range(3))
def test_the_three_patterns_of_the_gpu_tests_have_both_launch_shapes(case):
    """The simulation that chose them gave (levels, max width, launches) = (35, 7, 35), (21, 24, 21), (80, 1, 1); what is asserted is the
    restatement's own numbers, and what the GPU tests rely on: wide levels in the first two, one chain in the third."""
    m, n, q, seed = PATTERNS[case]
    lists = S.pattern(m, n, q, seed)
    want, *_ = same_plan(m, n, FIRST, lists)
    check_properties(FIRST, want["level"], lists)
    print(case, want["nlevels"], want["max_width"], want["nlaunches"])
    if case < 2:
        assert want["max_width"] >= 4
    else:
        assert want["nlaunches"] == 1 and want["nlevels"] == m - FIRST


# ------------------------------------------------------------------ the restatement

def ragged_model(k, seed, m=60, n=30):
    rng = np.random.default_rng(400 + seed)
    lens = rng.choice([0, 1, max(k - 1, 0), k, k + 1, 20], size=m)
    lists = [rng.choice(n, l, replace=False) for l in lens]
    lists[FIRST + 3] = np.full(k + 3, 5)                                          # one column k + 3 times: rank 1, a dup row
    return S.model(lists, n, k, seed=seed, rx_scales=(0.0, 0.1, 2.5)), lists


@pytest.mark.parametrize("k", (1, 8, 17))
def test_every_solved_row_meets_the_backward_error_bound_and_every_status_is_what_the_rules_name(k):
    """als_ref.residual_ratio with gamma replaced by 2 gamma, on the columns as the row found them (the restatement's trace).  Measured
    here over every solved row: at most 0.08 of the bound."""
    (g, X0, Y0), lists = ragged_model(k, k)
    pa = g.problem_arrays()
    trace = []
    out = S.stream_rows(pa, X0, Y0, FIRST, 0.05, 3, trace=trace)
    assert [t["i"] for t in trace] == list(range(FIRST, pa.m))
    worst, seen = 0.0, set()
    for t in trace:
        i, V, a, gamma, st = t["i"], t["V"], t["a"], t["gamma"], t["status"]
        rank1 = i == FIRST + 3 and k > 1 and gamma == 0.0
        want = S.KEPT_SHORT if (gamma == 0.0 and len(a) < k) else (S.KEPT_PIVOT if rank1 else S.SOLVED)
        assert st == want == out["status"][i - FIRST], (i, len(a), gamma, st, want)
        seen.add(int(st))
        if st == S.SOLVED:
            x = out["X"][:, i]
            ratio = AR.residual_ratio(V, a, np.ones(len(a)), 2.0 * gamma, x)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (i, ratio)
            assert np.isfinite(out["objective"][i - FIRST]) and out["objective"][i - FIRST] >= 0.0
        else:
            assert out["X"][:, i].tobytes() == X0[:, i].tobytes() and np.isnan(out["objective"][i - FIRST])
    assert {S.SOLVED, S.KEPT_SHORT} <= seen
    assert out["X"][:, :FIRST].tobytes() == np.asfortranarray(X0[:, :FIRST]).tobytes()
    print(f"k={k}: worst residual / bound = {worst:.3g}")


def test_the_decay_is_the_headers_and_a_reader_writes_nothing():
    """interval 1, 3 and 10 with m no multiple: a column nobody touches ends at Y0 / c^total; queries change no bit of X, Y or the
    objective; sy = 0 divides nothing."""
    lists = S.pattern(50, 12, 2, 3)
    lists = [l[l != 11] for l in lists]                                           # column 11 is never observed
    g, X0, Y0 = S.model(lists, 12, 2, seed=3, rx_scales=(0.1, 0.5))
    pa = g.problem_arrays()
    sy = float(AR.gammas(pa.ry, 12)[0])
    for interval in (1, 3, 10):
        out = S.stream_rows(pa, X0, Y0, FIRST, 0.05, interval)
        c = 1.0 + ((2.0 * 0.05) * float(interval)) * sy
        total = 50 // interval - FIRST // interval
        assert out["Y"][:, 11].tobytes() == (Y0[:, 11] / S.power(c, total)).tobytes()
        qptr, qcol = S.csr([np.array([11, 0])] * 50)
        withq = S.stream_rows(pa, X0, Y0, FIRST, 0.05, interval, qptr, qcol)
        assert all(withq[f].tobytes() == out[f].tobytes() for f in ("X", "Y", "objective", "status"))
        i = 40
        D = i // interval - FIRST // interval
        y = Y0[:, 11] / S.power(c, D) if D > 0 else Y0[:, 11]
        assert withq["qout"][qptr[i]] == S.dots(y[None, :], out["X"][:, i])[0]
    g0, X0, Y0 = S.model(lists, 12, 2, seed=3, rx_scales=(0.1, 0.5), sy=0.0)
    assert S.stream_rows(g0.problem_arrays(), X0, Y0, FIRST, 0.05, 1)["Y"][:, 11].tobytes() == Y0[:, 11].tobytes()


# the worst relative difference max|restatement - literal| / max|literal| over X, Y, the objectives and the imputed values of the cases
# below, measured on the CPU this was written on; the assertion allows FACTOR times that for another BLAS build on another machine
MEASURED = 3.07e-15
FACTOR = 64


def test_the_restatement_follows_the_literal_loop():
    """stream_ref.stream_rows against stream_ref.literal (np.linalg.solve, one division of all of Y per interval, a dense Ahat) on
    well-conditioned problems: rx scales >= 0.1, k in {2, 8}, intervals 1 and 10, three seeds each.  The two differ by LAPACK's order of
    operations and by p = c^d in place of d successive divisions.  Measured worst relative difference (max abs difference over max abs
    value, per array): 3.07e-15; asserted at 64 times that, 1.96e-13."""
    worst = 0.0
    for k in (2, 8):
        for interval in (1, 10):
            for seed in range(3):
                m, n = 70, 24
                lists = S.pattern(m, n, 12, 100 * k + 10 * interval + seed)
                g, X0, Y0 = S.model(lists, n, k, seed=seed, rx_scales=(0.1, 0.5, 2.5))
                pa = g.problem_arrays()
                observed = np.zeros((m, n), dtype=bool)
                for i, l in enumerate(lists):
                    observed[i, l] = True
                rows, cols = np.nonzero(~observed[FIRST:])
                rows = rows + FIRST
                qptr = np.zeros(m + 1, dtype=np.int64)
                np.cumsum(np.bincount(rows, minlength=m), out=qptr[1:])
                ours = S.stream_rows(pa, X0, Y0, FIRST, 0.05, interval, qptr, cols.astype(np.int32))
                lit = S.literal(pa, X0, Y0, FIRST, 0.05, interval, A=np.asarray(g.A))
                assert np.all(ours["status"] == S.SOLVED)
                for name, a, b in (("X", ours["X"], lit["X"]), ("Y", ours["Y"], lit["Y"]), ("objective", ours["objective"], lit["objective"]),
                                   ("imputed", ours["qout"], lit["Ahat"][rows, cols])):
                    rel = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
                    worst = max(worst, rel)
                    assert rel <= FACTOR * MEASURED, (k, interval, seed, name, rel)
                assert np.array_equal(lit["Ahat"][observed], np.asarray(g.A)[observed])
    print(f"worst relative difference = {worst:.3g}")


# ------------------------------------------------------------------ the drivers on the host engine

def host():
    return S.HostEngine(O.oracle_api())


def small_model(seed=2, m=40, n=14, k=3):
    lists = S.pattern(m, n, 6, 70 + seed)
    return S.model(lists, n, k, seed=seed, rx_scales=(0.1, 0.5))[0]


def test_streaming_fit_initialises_like_the_reference_and_streams_the_rest():
    T0 = 12
    g = small_model()
    api = host()
    init = L.keep_rows(g, T0)
    assert (init.m, init.n, init.k) == (T0, g.n, g.k) and np.array_equal(init._colidx, g._colidx[: g._rowptr[T0]])
    assert np.array_equal(init._rowvals, g._rowvals[: g._rowptr[T0]]) and [r.scale for r in init.rx] == [r.scale for r in g.rx[:T0]]
    L.init_svd_(init, engine=api)
    init.close()
    p = L.StreamingParams(T0, stepsize=0.05, Y_update_interval=3)
    X, Y, ch = L.streaming_fit(g, p, verbose=False, engine=api)
    try:
        assert X is g.X and Y is g.Y and ch.name == "StreamingGLRM"
        assert g.X[:, :T0].tobytes() == np.asfortranarray(init.X).tobytes()                 # rows < T0: init_svd! of keep_rows
        X0 = g.X.copy(order="F")
        X0[:, :T0] = init.X
        ref = S.stream_rows(g.problem_arrays(), X0, init.Y, T0, 0.05, 3)
        assert g.X[:, :T0].tobytes() == ref["X"][:, :T0].tobytes() and g.Y.tobytes() == ref["Y"].tobytes()
        assert np.array_equal(g.X[:, T0:], ref["X"][:, T0:])
        assert len(ch.objective) == g.m - T0 and np.array_equal(np.array(ch.objective), ref["objective"]) and ch.times == []
        assert g._stream_info["solved"] == g.m - T0 and g._stream_info["nlevels"] >= 1
    finally:
        g.close()


def test_t0_equal_m_streams_nothing_and_t0_above_m_is_refused():
    g = small_model(seed=3)
    api = host()
    init = L.keep_rows(g, g.m)
    L.init_svd_(init, engine=api)
    init.close()
    X, Y, ch = L.streaming_fit(g, L.StreamingParams(g.m), verbose=False, engine=api)
    g.close()
    assert ch.objective == [] and X.tobytes() == np.asfortranarray(init.X).tobytes() and Y.tobytes() == np.asfortranarray(init.Y).tobytes()
    api2 = host()
    for T0 in (g.m + 1, 0):
        with pytest.raises(_capi.GLRMError) as ei:
            L.streaming_fit(small_model(seed=3), _params(T0), verbose=False, engine=api2)
        assert ei.value.code == _capi.ERR_INVALID and "first must be in 1 .. m" in ei.value.message
    assert api2.created == 0


def _params(T0):
    p = L.StreamingParams(5, stepsize=0.1)
    p.T0 = T0
    return p


def test_streaming_impute_equals_streaming_impute_at_entry_for_entry():
    T0 = 12
    p = L.StreamingParams(T0, stepsize=0.05, Y_update_interval=3)
    g = small_model(seed=4)
    Ahat = L.streaming_impute(g, p, engine=host())
    g.close()
    observed = np.zeros((g.m, g.n), dtype=bool)
    observed[np.repeat(np.arange(g.m), np.diff(g._rowptr)), g._colidx] = True
    assert np.array_equal(Ahat[observed], np.asarray(g.A)[observed]) and np.array_equal(Ahat[:T0], np.asarray(g.A)[:T0])
    rows, cols = np.nonzero(~observed[T0:])
    rows = rows + T0
    perm = np.random.default_rng(0).permutation(len(rows))                               # any order; the results come back in the caller's
    g2 = small_model(seed=4)
    vals = L.streaming_impute_at(g2, rows[perm], cols[perm], p, engine=host())
    g2.close()
    assert vals.tobytes() == Ahat[rows[perm], cols[perm]].tobytes()
    assert g2.X.tobytes() == g.X.tobytes() and g2.Y.tobytes() == g.Y.tobytes()
    with pytest.raises(ValueError):
        L.streaming_impute_at(small_model(seed=4), [T0 - 1], [0], p, engine=host())


def test_a_model_the_engine_would_refuse_is_refused_on_the_host_before_create():
    rng = np.random.default_rng(9)
    A = rng.standard_normal((8, 6))
    q = L.QuadReg(0.1)

    def refused(losses, rx, ry, words, k=2, **kw):
        api = host()
        with pytest.raises(_capi.GLRMError) as ei:
            L.streaming_fit(L.GLRM(A, losses, rx, ry, k, rng=np.random.default_rng(1), **kw), L.StreamingParams(4), verbose=False, engine=api)
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_stream.h" in ei.value.message, ei.value.message
        assert ei.value.message.startswith("glrm_hip_stream_rows")
        for w in words:
            assert w in ei.value.message, (w, ei.value.message)
        assert api.created == 0                                           # before a handle exists
    refused(L.HuberLoss(), q, q, ["column 0 has loss kind 2", "needs QuadLoss"])
    refused([L.QuadLoss()] * 5 + [L.L1Loss()], q, q, ["column 5 has loss kind 1"])
    refused(L.QuadLoss(2.0), q, q, ["column 0 is QuadLoss with scale 2", "exactly 1"])
    refused([L.QuadLoss()] * 3 + [L.QuadLoss(0.5)] + [L.QuadLoss()] * 2, q, q, ["column 3 is QuadLoss with scale 0.5"])
    refused(L.QuadLoss(), L.NonNegConstraint(), q, ["rx[0] has regularizer kind 3", "plain QuadReg"])
    refused(L.QuadLoss(), q, L.OneReg(0.1), ["ry[0] has regularizer kind 2"])
    refused(L.QuadLoss(), L.QuadReg(-1.0), q, ["rx[0] is QuadReg with scale -1"])
    refused(L.QuadLoss(), q, [L.QuadReg(0.1)] * 3 + [L.QuadReg(0.2)] + [L.QuadReg(0.1)] * 2, ["ry[3] has scale 0.2 and ry[0] has 0.1", "equal scales"])
    refused(L.QuadLoss(), q, [L.QuadReg(0.1)] * 3 + [L.ZeroReg()] + [L.QuadReg(0.1)] * 2, ["ry[3] has scale 0 and ry[0] has 0.1"])
    refused(L.QuadLoss(), q, q, ["rx[0]", "wrap 1"], offset=True)
    api = host()
    with pytest.raises(_capi.GLRMError) as ei:
        L.streaming_fit(L.GLRM(rng.standard_normal((70, 66)), L.QuadLoss(), q, q, 65, rng=np.random.default_rng(1)), L.StreamingParams(4), verbose=False, engine=api)
    assert "rank k = 65 is above GLRM_STREAM_MAX_K = 64" in ei.value.message and api.created == 0
    with pytest.raises(_capi.GLRMError) as ei:                            # an engine without the extension, by name
        L.streaming_fit(L.GLRM(A, L.QuadLoss(), q, q, 2, rng=np.random.default_rng(1)), L.StreamingParams(4), verbose=False, engine=O.oracle_api())
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "glrm_cpu_stream_rows" in ei.value.message
    assert stream_mod.HEADER == "include/glrm_hip_stream.h"
