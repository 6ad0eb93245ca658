"""The impute_at extension (include/glrm_hip_impute_at.h) without a GPU: the built libraries export what the header declares, the boundary
header still has its 37 symbols, the ctypes argument types and the Julia shim (julia/HipGLRMImputeAt.jl, which cannot run here) are held
to the C prototypes argument by argument, the Python layer validates its arguments and infers the mode, and an engine without the
extension (the CPU oracle) answers by indexing its full impute -- checked on a golden fixture."""
import ctypes
import os
import re

import numpy as np
import pytest

import cases
import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from lowrankmodels.jl_amd.predict import _query
from test_abi import PKG, ROOT, declared, ensure_built
from test_transform_abi import JL_C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = "glrm_hip_impute_at.h"


# ---- the ABI

def c_prototypes():
    """{name: [argument types]} of the header, read the way tests/test_transform_abi.py reads its headers."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(glrm_hip_\w+)\s*\(([^)]*)\)\s*;", txt):
        out[m.group(1)] = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")).replace(" *", "*") for a in m.group(2).split(",")]
    return out


PROTO = {"glrm_hip_impute_at": ["glrm_handle*", "double*", "double*", "glrm_domain*", "int64_t*", "int64_t", "int32_t*", "int64_t", "int32_t",
                                "double*", "int64_t", "double*", "double*", "double*"],
         "glrm_hip_impute_at_info": ["int64_t*", "int64_t*", "int64_t*"]}


def test_libraries_export_every_symbol_the_header_declares():
    ensure_built()
    names = declared(HEADER, "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.IMPUTE_AT_SYMBOLS) and len(names) == 2
    assert not set(_capi.IMPUTE_AT_SYMBOLS) & (set(_capi.ABI_SYMBOLS) | set(_capi.RECOMMEND_SYMBOLS) | set(_capi.TOPK_SYMBOLS))
    assert len(declared("glrm_hip.h", "glrm_hip_")) == 37 == len(_capi.ABI_SYMBOLS)          # the boundary is where it was
    assert len(declared("glrm_hip_recommend.h", "glrm_hip_")) == 2 and len(declared("glrm_hip_topk.h", "glrm_hip_")) == 3
    assert c_prototypes() == PROTO
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)


def test_the_header_states_the_modes_and_the_contract():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    for name, v in (("PAIRS", _capi.IMPUTE_AT_PAIRS), ("ROWS", _capi.IMPUTE_AT_ROWS), ("COLS", _capi.IMPUTE_AT_COLS)):
        assert re.search(r"#define\s+GLRM_IMPUTE_AT_%s\s+%d\b" % (name, v), txt)
    assert "nothing is written" in txt and "not of block_entries" in txt and "r + j * n_rows" in txt and "i + c * m" in txt


CTYPES_C = {ctypes.c_void_p: {"glrm_handle*", "double*", "glrm_domain*", "int64_t*", "int32_t*"}, ctypes.c_int64: {"int64_t"}, ctypes.c_int32: {"int32_t"},
            ctypes.POINTER(ctypes.c_double): {"double*"}, ctypes.POINTER(ctypes.c_int64): {"int64_t*"}}


def test_ctypes_argument_types_match_the_header():
    ensure_built()
    api = _capi.Api(ctypes.CDLL(os.path.join(PKG, "libglrm_hip.so"), mode=ctypes.RTLD_LOCAL), "glrm_hip_", "cuda")
    assert api.has_impute_at
    for name, args in PROTO.items():
        fn = api._f[name[len("glrm_hip_"):]]
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(args), name
        for t, c in zip(fn.argtypes, args):
            assert c in CTYPES_C[t], (name, t, c)


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    assert not api.has_impute_at
    for call in (lambda: api.impute_at(None, None, None, None, 1, 1, [0], [0]), api.impute_at_info):
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_impute_at.h" in ei.value.message


def test_impute_at_is_part_of_the_package():
    assert callable(L.impute_at) and callable(L.error_metric_at)
    assert "impute_at" in L.__all__ and "error_metric_at" in L.__all__
    from lowrankmodels.jl_amd.predict import error_metric_at, impute_at
    assert impute_at is L.impute_at and error_metric_at is L.error_metric_at


# ---- julia/HipGLRMImputeAt.jl

JL_C_MORE = dict(JL_C, **{"Ptr{Int64}": "int64_t*", "Int32": "int32_t", "Ptr{Int32}": "int32_t*", "Ptr{CDomain}": "glrm_domain*"})


def test_every_ccall_of_the_shim_matches_a_declared_prototype():
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "HipGLRMImputeAt.jl")).read())
    protos = c_prototypes()
    calls = re.findall(r"ccall\(\s*\(:(glrm_hip_\w+), LIB\)\s*,\s*Cint\s*,\s*\(([^)]*)\)", txt)
    assert len(calls) == len(re.findall(r"\bccall\(", txt)) == 2                              # one ccall per prototype
    assert sorted(n for n, _ in calls) == sorted(protos)
    for name, jl in calls:
        jl_args = [a.strip() for a in jl.split(",") if a.strip()]
        assert [JL_C_MORE[a] for a in jl_args] == protos[name], (name, jl_args, protos[name])
    assert "module HipGLRMImputeAt" in txt and "export hip_impute_at, hip_error_metric_at, hip_impute_at_info" in txt
    assert "Int64[i - 1 for i in rows]" in txt and "Int32[j - 1 for j in cols]" in txt        # 1-based on the Julia side
    assert "import ..HipGLRMExtras: CDomain, cdomain" in txt                                  # the domain descriptors of hip_impute


# ---- the Python layer

def small_model():
    rng = np.random.default_rng(3)
    return L.GLRM(rng.standard_normal((7, 5)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 2, rng=rng)


def test_mode_inference():
    g = small_model()
    r, c, shape = _query(g, [6, 0, 0], [4, 4, 1])
    assert r.dtype == np.int64 and c.dtype == np.int32 and shape == (3,) and r.tolist() == [6, 0, 0] and c.tolist() == [4, 4, 1]
    r, c, shape = _query(g, [2, 2], None)
    assert c is None and shape == (2, 5)
    r, c, shape = _query(g, None, np.array([4]))
    assert r is None and shape == (7, 1) and c.dtype == np.int32
    assert _query(g, [], [])[2] == (0,) and _query(g, [], None)[2] == (0, 5)
    g.close()


def test_validation():
    g = small_model()
    api = O.oracle_api()
    with pytest.raises(ValueError, match=r"impute\(glrm\)"):
        L.impute_at(g, engine=api)                                                            # neither: points to impute
    with pytest.raises(ValueError, match="as many rows as cols"):
        L.impute_at(g, [0, 1], [0], engine=api)
    for rows, cols in (([7], [0]), ([-1], [0]), ([0], [5]), ([0], [-1]), ([7], None), (None, [5])):
        with pytest.raises(_capi.GLRMError) as ei:
            L.impute_at(g, rows, cols, engine=api)
        assert ei.value.code == _capi.ERR_INVALID
    with pytest.raises(ValueError, match="truth has shape"):
        L.error_metric_at(g, [0, 1], [0, 1], np.zeros(3), engine=api)
    with pytest.raises(ValueError, match="truth has shape"):
        L.error_metric_at(g, [0, 1], None, np.zeros((5, 2)), engine=api)
    with pytest.raises(ValueError, match="domains"):
        L.impute_at(g, [0], [0], domains=[L.RealDomain()] * 4, engine=api)
    g.close()


def test_the_oracle_engine_answers_by_indexing_its_full_impute():
    """tests/golden/mixed.npz: the fitted factors of the mixed-loss fixture on the model its builder makes."""
    kwargs, _ = cases.build_golden_case("mixed")
    z = np.load(os.path.join(GOLDEN, "mixed.npz"))
    g = L.GLRM(**kwargs)
    api = O.oracle_api()
    X, Y = np.asfortranarray(z["X"]), np.asfortranarray(z["Y"])
    Ahat = L.impute(g, X, Y, engine=api)
    rng = np.random.default_rng(8)
    rows, cols = rng.integers(0, g.m, 50), rng.integers(0, g.n, 50)
    got = L.impute_at(g, rows, cols, X=X, Y=Y, engine=api)
    assert got.shape == (50,) and np.array_equal(got, Ahat[rows, cols])
    assert np.array_equal(L.impute_at(g, rows=[g.m - 1, 0, 0], X=X, Y=Y, engine=api), Ahat[[g.m - 1, 0, 0], :])
    slab = L.impute_at(g, cols=[g.n - 1, 0], X=X, Y=Y, engine=api)
    assert slab.flags.f_contiguous and np.array_equal(slab, Ahat[:, [g.n - 1, 0]])
    # errors: the mirror, entry by entry (the fixture's columns are scalar)
    doms = [L.default_domain(l) for l in g.losses]
    assert all(l.embedding_dim == 1 for l in g.losses)
    truth = rng.integers(0, 3, 50).astype(np.float64)
    err, total = L.error_metric_at(g, rows, cols, truth, X=X, Y=Y, engine=api)
    U = X.T @ Y
    want = np.array([L.error_metric_entry(doms[j], g.losses[j], float(U[i, j]), a) for i, j, a in zip(rows, cols, truth)])
    np.testing.assert_allclose(err, want, rtol=1e-9, atol=1e-12)
    assert total == pytest.approx(float(np.sum(want)), rel=1e-9)
    err2, total2 = L.error_metric_at(g, None, [1], Ahat[:, [1]], X=X, Y=Y, engine=api)         # its own prediction: no error
    assert err2.shape == (g.m, 1) and not err2.any() and total2 == 0.0
    g.close()
