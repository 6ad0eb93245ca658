"""The sampling extension (include/glrm_hip_sample.h) without a GPU: the built libraries export exactly what the header declares, the
boundary header still has its 37 symbols, the ctypes argument types and the Julia shim (julia/HipGLRMSample.jl, which cannot run here)
are held to the C prototypes argument by argument, the package exports the four functions, the Python layer validates its arguments, and
an engine without the extension (the CPU oracle) is refused by name."""
import ctypes
import os
import re

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from test_abi import PKG, ROOT, declared, ensure_built
from test_transform_abi import JL_C

HEADER = "glrm_hip_sample.h"


def c_prototypes():
    """{name: [argument types]} of the header, read the way tests/test_transform_abi.py reads its headers."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(glrm_hip_\w+)\s*\(([^)]*)\)\s*;", txt):
        out[m.group(1)] = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")).replace(" *", "*") for a in m.group(2).split(",")]
    return out


PROTO = {"glrm_hip_sample_at": ["glrm_handle*", "double*", "double*", "glrm_domain*", "int64_t*", "int64_t", "int32_t*", "int64_t", "int32_t",
                                "uint64_t", "int32_t", "double*", "int32_t", "int64_t", "double*", "uint8_t*", "double*"],
         "glrm_hip_sample_at_info": ["int64_t*"] * 5}


def test_libraries_export_exactly_the_symbols_the_header_declares():
    ensure_built()
    names = declared(HEADER, "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.SAMPLE_SYMBOLS) and len(names) == 2
    assert not set(_capi.SAMPLE_SYMBOLS) & (set(_capi.ABI_SYMBOLS) | set(_capi.IMPUTE_AT_SYMBOLS) | set(_capi.RECOMMEND_SYMBOLS) | set(_capi.TOPK_SYMBOLS))
    assert len(declared("glrm_hip.h", "glrm_hip_")) == 37 == len(_capi.ABI_SYMBOLS)          # the boundary is where it was
    assert len(declared("glrm_hip_impute_at.h", "glrm_hip_")) == 2
    assert c_prototypes() == PROTO
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)
        assert not hasattr(so, "glrm_hip_sample") and not hasattr(so, "glrm_hip_sample_missing_at")   # ... and nothing else of the kind


def test_the_header_states_the_rules_and_the_contract():
    txt = open(os.path.join(ROOT, "include", HEADER)).read()
    for name, v in _capi.SAMPLE_NOISE.items():
        assert re.search(r"#define\s+GLRM_SAMPLE_NOISE_%s\s+%d\b" % (name.upper(), v), txt)
    for word in ("Philox4x32-10", "S1", "S2", "S3", "S4", "wsample", "Deviations from the reference", "D.min + index", "ROW-VIEW", "nothing is written",
                 "(seed, row, column, X, Y, lists)"):
        assert word in txt, word


CTYPES_C = {ctypes.c_void_p: {"glrm_handle*", "double*", "glrm_domain*", "int64_t*", "int32_t*", "uint8_t*"}, ctypes.c_int64: {"int64_t"},
            ctypes.c_int32: {"int32_t"}, ctypes.c_uint64: {"uint64_t"}, ctypes.POINTER(ctypes.c_int64): {"int64_t*"}}


def test_ctypes_argument_types_match_the_header():
    ensure_built()
    api = _capi.Api(ctypes.CDLL(os.path.join(PKG, "libglrm_hip.so"), mode=ctypes.RTLD_LOCAL), "glrm_hip_", "cuda")
    for name, args in PROTO.items():
        fn = api._f[name[len("glrm_hip_"):]]
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(args), name
        for t, c in zip(fn.argtypes, args):
            assert c in CTYPES_C[t], (name, t, c)


def small_model():
    rng = np.random.default_rng(3)
    return L.GLRM(rng.standard_normal((7, 5)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 2, rng=rng)


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    g = small_model()
    calls = (lambda: api.sample_at(None, None, None, None, 1, 1, [0], [0], seed=1), api.sample_at_info,
             lambda: L.sample_at(g, [0], [0], seed=1, engine=api), lambda: L.sample_missing_at(g, [0], [0], seed=1, engine=api),
             lambda: L.sample(g, seed=1, engine=api), lambda: L.sample_missing(g, rng=np.random.default_rng(1), engine=api))
    for call in calls:
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_sample.h" in ei.value.message
    g.close()


def test_the_package_exports_the_four_functions():
    from lowrankmodels.jl_amd import sample as mod_or_fn                                       # the function shadows the submodule's name
    import sys
    mod = sys.modules["lowrankmodels.jl_amd.sample"]
    assert mod.__all__ == ["sample_at", "sample_missing_at", "sample", "sample_missing"]
    for name in mod.__all__:
        assert callable(getattr(L, name)) and getattr(L, name) is getattr(mod, name) and name in L.__all__
    assert mod_or_fn is mod.sample


class Hip:
    """Stands where the HIP engine would: has the extension, and fails the test if validation lets a call through to it."""
    def _sample(self, name):
        return None

    def __getattr__(self, name):
        raise AssertionError(f"the engine was reached ({name})")


def test_validation_happens_before_the_engine():
    g = small_model()
    with pytest.raises(ValueError, match=r"sample\(glrm\)"):
        L.sample_at(g, seed=1, engine=Hip())                                                  # neither: points to sample
    with pytest.raises(ValueError, match="exactly one of seed"):
        L.sample_at(g, [0], [0], engine=Hip())
    with pytest.raises(ValueError, match="exactly one of seed"):
        L.sample_at(g, [0], [0], seed=1, rng=np.random.default_rng(1), engine=Hip())
    with pytest.raises(ValueError, match="as many rows as cols"):
        L.sample_at(g, [0, 1], [0], seed=1, engine=Hip())
    for rows, cols in (([7], [0]), ([-1], [0]), ([0], [5]), ([7], None), (None, [5])):
        with pytest.raises(_capi.GLRMError) as ei:
            L.sample_at(g, rows, cols, seed=1, engine=Hip())
        assert ei.value.code == _capi.ERR_INVALID
    with pytest.raises(ValueError, match="domains"):
        L.sample_at(g, [0], [0], seed=1, domains=[L.RealDomain()] * 4, engine=Hip())
    with pytest.raises(ValueError, match="noise must be"):
        L.sample_at(g, [0], [0], seed=1, noise="loud", engine=Hip())
    with pytest.raises(ValueError, match="needs noise_sd"):
        L.sample_at(g, [0], [0], seed=1, noise="given", engine=Hip())
    g.close()


def test_one_integer_is_drawn_from_rng():
    from lowrankmodels.jl_amd.sample import _seed
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    s = _seed(None, a)
    assert s == int(b.integers(0, 2 ** 64, dtype=np.uint64)) and a.random() == b.random()      # exactly one draw
    assert _seed(-1, None) == 2 ** 64 - 1 and _seed(2 ** 64 + 5, None) == 5


# ---- julia/HipGLRMSample.jl

JL_C_MORE = dict(JL_C, **{"Ptr{Int64}": "int64_t*", "Int32": "int32_t", "Ptr{Int32}": "int32_t*", "Ptr{CDomain}": "glrm_domain*", "UInt64": "uint64_t",
                          "Ptr{UInt8}": "uint8_t*"})


def test_every_ccall_of_the_shim_matches_a_declared_prototype():
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "HipGLRMSample.jl")).read())
    protos = c_prototypes()
    calls = re.findall(r"ccall\(\s*\(:(glrm_hip_\w+), LIB\)\s*,\s*Cint\s*,\s*\(([^)]*)\)", txt)
    assert len(calls) == len(re.findall(r"\bccall\(", txt)) == 2                              # one ccall per prototype
    assert sorted(n for n, _ in calls) == sorted(protos)
    for name, jl in calls:
        jl_args = [a.strip() for a in jl.split(",") if a.strip()]
        assert [JL_C_MORE[a] for a in jl_args] == protos[name], (name, jl_args, protos[name])
    assert "module HipGLRMSample" in txt and "export hip_sample_at, hip_sample_missing_at, hip_sample_at_info" in txt
    assert "Int64[i - 1 for i in rows]" in txt and "Int32[j - 1 for j in cols]" in txt        # 1-based on the Julia side
    assert "import ..HipGLRMExtras: CDomain, cdomain" in txt                                  # the domain descriptors of hip_impute
    assert re.search(r":residual => 0, :reference => 1, :given => 2", txt)                    # GLRM_SAMPLE_NOISE_*
