"""The transform extension (include/glrm_hip_transform.h) without a GPU: the built libraries export what the header declares, an engine
without the extension is refused by name, the driver is part of the package, and the Julia shim of the extension
(julia/HipGLRMTransform.jl, which cannot run here) is held to the headers the way tests/test_julia_shim.py holds the other shims."""
import ctypes
import os
import re

import pytest

import lowrankmodels.jl_amd as L
import oracle as O
from lowrankmodels.jl_amd import _capi
from test_abi import PKG, ROOT, declared, ensure_built


def test_libraries_export_every_symbol_the_header_declares():
    ensure_built()
    names = declared("glrm_hip_transform.h", "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.TRANSFORM_SYMBOLS) and len(names) == 2
    assert not set(_capi.TRANSFORM_SYMBOLS) & set(_capi.ABI_SYMBOLS)     # outside the 37-symbol boundary
    assert len(declared("glrm_hip.h", "glrm_hip_")) == 37 == len(_capi.ABI_SYMBOLS)
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    assert not api.has_transform
    for call in (lambda: api.solve_x(None, 1, 0.01), lambda: api.solve_x_info(None)):
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_transform.h" in ei.value.message


def test_transform_is_part_of_the_package():
    assert callable(L.transform) and callable(L.inverse_transform)
    assert "transform" in L.__all__ and "inverse_transform" in L.__all__
    from lowrankmodels.jl_amd.transform import inverse_transform, transform
    assert transform is L.transform and inverse_transform is L.inverse_transform


# ---- julia/HipGLRMTransform.jl

def shim():
    return re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "HipGLRMTransform.jl")).read())


JL_C = {"Ptr{Cvoid}": "glrm_handle*", "Int64": "int64_t", "Float64": "double", "Ref{Int32}": "int32_t*", "Ref{Int64}": "int64_t*",
        "Ptr{Float64}": "double*", "Cint": "int", "Ref{Float64}": "double*"}


def c_prototypes():
    out = {}
    for header in ("glrm_hip.h", "glrm_hip_transform.h"):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for m in re.finditer(r"\bint\s+(glrm_hip_\w+)\s*\(([^)]*)\)\s*;", txt):
            args = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")).replace(" *", "*") for a in m.group(2).split(",")]
            out[m.group(1)] = args
    return out


def test_every_ccall_of_the_shim_matches_a_declared_prototype():
    txt, protos = shim(), c_prototypes()
    calls = re.findall(r"ccall\(\s*\(:(glrm_hip_\w+), LIB\)\s*,\s*Cint\s*,\s*\(([^)]*)\)", txt)
    assert len(calls) == len(re.findall(r"\bccall\(", txt)) and calls           # every target is a literal (:symbol, LIB), every result a Cint
    assert {"glrm_hip_solve_x", "glrm_hip_solve_x_info"} <= {n for n, _ in calls}
    for name, jl in calls:
        assert name in protos, name
        jl_args = [a.strip() for a in jl.split(",") if a.strip()]
        assert [JL_C[a] for a in jl_args] == protos[name], (name, jl_args, protos[name])


def test_the_shim_follows_the_reference_loop():
    txt = shim()
    assert "module HipGLRMTransform" in txt and "export transform, inverse_transform" in txt
    assert "transform(glrm::GLRM, A_new, p::HipProxGradParams" in txt
    body = txt[txt.index("function transform"):]
    assert body.index("p.inner_iter_X > 1 &&") < body.index("hip_solve_x!(h, p.inner_iter_X, p.min_stepsize)") < body.index("update_ch!(ch, time() - t, o)")
    assert "i > 10 && (dec < scaled_abs_tol || dec / o < p.rel_tol) && break" in body
    assert "glrm_hip_step_y" not in txt                                          # Y is held fixed
    assert "inverse_transform(glrm::GLRM, X_new) = X_new' * glrm.Y" in txt
