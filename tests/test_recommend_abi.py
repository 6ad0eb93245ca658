"""The recommend extension (include/glrm_hip_recommend.h) without a GPU: the built libraries export what the header declares, the
boundary header still has its 37 symbols, an engine without the extension is refused by name, the driver is part of the package, the
Julia shim (julia/HipGLRMRecommend.jl, which cannot run here) is held to the C prototype argument by argument, and the numpy restatement
the GPU tests compare against (tests/recommend_ref.py) is checked on an example small enough to rank by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
import precision_ref as R
import recommend_ref as RR
from lowrankmodels.jl_amd import _capi
from test_abi import PKG, ROOT, declared, ensure_built
from test_transform_abi import JL_C


def test_libraries_export_every_symbol_the_header_declares():
    ensure_built()
    names = declared("glrm_hip_recommend.h", "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.RECOMMEND_SYMBOLS) and len(names) == 2
    assert not set(_capi.RECOMMEND_SYMBOLS) & (set(_capi.ABI_SYMBOLS) | set(_capi.TOPK_SYMBOLS))
    assert len(declared("glrm_hip.h", "glrm_hip_")) == 37 == len(_capi.ABI_SYMBOLS)          # the boundary is where it was
    assert len(declared("glrm_hip_topk.h", "glrm_hip_")) == 3
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)


def test_the_header_states_the_limit_and_the_order():
    txt = open(os.path.join(ROOT, "include", "glrm_hip_recommend.h")).read()
    assert re.search(r"#define\s+GLRM_ROW_TOPK_MAX\s+128\b", txt) and _capi.ROW_TOPK_MAX == 128
    assert "a NaN score ranks first" in txt and "0x7FF8000000000000" in txt


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    for call in (lambda: api.row_topk(None, None, None, [0], 1), api.row_topk_info):
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_recommend.h" in ei.value.message
    g = L.GLRM(np.ones((3, 4)), L.QuadLoss(), L.ZeroReg(), L.ZeroReg(), 1)
    with pytest.raises(_capi.GLRMError) as ei:
        L.recommend(g, k=2, engine=api)
    g.close()
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_recommend.h" in ei.value.message


def test_recommend_is_part_of_the_package():
    assert callable(L.recommend) and "recommend" in L.__all__
    from lowrankmodels.jl_amd.recommend import recommend
    assert recommend is L.recommend


# ---- julia/HipGLRMRecommend.jl

JL_C_MORE = dict(JL_C, **{"Ptr{Int64}": "int64_t*", "Int32": "int32_t", "Ptr{Int32}": "int32_t*"})


def c_prototypes():
    """{name: [argument types]} of the header, read the way tests/test_transform_abi.py reads its headers."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glrm_hip_recommend.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(glrm_hip_\w+)\s*\(([^)]*)\)\s*;", txt):
        out[m.group(1)] = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")).replace(" *", "*") for a in m.group(2).split(",")]
    return out


def test_the_one_ccall_of_the_shim_matches_the_prototype():
    txt = re.sub(r"#.*", "", open(os.path.join(ROOT, "julia", "HipGLRMRecommend.jl")).read())
    protos = c_prototypes()
    assert protos["glrm_hip_row_topk"] == ["glrm_handle*", "double*", "double*", "int64_t*", "int64_t", "int32_t", "int32_t", "int32_t",
                                           "int32_t*", "double*", "int32_t*"]
    assert protos["glrm_hip_row_topk_info"] == ["int32_t*", "int64_t*", "int64_t*"]
    calls = re.findall(r"ccall\(\s*\(:(glrm_hip_\w+), LIB\)\s*,\s*Cint\s*,\s*\(([^)]*)\)", txt)
    assert len(calls) == len(re.findall(r"\bccall\(", txt)) == 1 and calls[0][0] == "glrm_hip_row_topk"
    jl_args = [a.strip() for a in calls[0][1].split(",") if a.strip()]
    assert [JL_C_MORE[a] for a in jl_args] == protos["glrm_hip_row_topk"], (jl_args, protos["glrm_hip_row_topk"])
    assert "module HipGLRMRecommend" in txt and "export hip_recommend" in txt
    assert "hip_recommend(glrm::GLRM, rows::AbstractVector{<:Integer}; k::Integer=10, exclude_observed::Bool=true, device_id::Int=-1)" in txt
    assert "Int64[i - 1 for i in rows]" in txt and "cols .+ Int32(1)" in txt                   # 1-based on the Julia side, both ways


# ---- tests/recommend_ref.py

def test_the_restatement_on_a_hand_example():
    """3 x 5.  Row 0: a tie between columns 1 and 3 at the top (the lower column first) and a NaN (first of all).  Row 1: its best
    column is in its list.  Row 2: only two columns are left, fewer than kper = 3."""
    nan = np.nan
    XY = np.array([[1.0, 7.0, nan, 7.0, -0.0],
                   [9.0, 2.0, 3.0, 1.0, 0.0],
                   [5.0, 4.0, 3.0, 2.0, 1.0]])
    lists = [[], [0, 0], [4, 0, 2]]
    cols, vals, count = RR.row_topk(XY, None, 3, lists)
    assert cols.dtype == np.int32 and cols.tolist() == [[2, 1, 3], [2, 1, 3], [1, 3, -1]] and count.tolist() == [3, 3, 2]
    assert R.same_bits(vals, np.array([[nan, 7.0, 7.0], [3.0, 2.0, 1.0], [4.0, 2.0, nan]]))
    assert vals.view(np.uint64)[0, 0] == vals.view(np.uint64)[2, 2] == 0x7FF8000000000000
    # no exclusion, a query list with a repeat, kper = 1 and kper above n
    cols, vals, count = RR.row_topk(XY, [1, 1, 0], 1)
    assert cols.tolist() == [[0], [0], [2]] and count.tolist() == [1, 1, 1] and vals[0, 0] == 9.0 and np.isnan(vals[2, 0])
    cols, vals, count = RR.row_topk(XY, [0], 7)
    assert cols.tolist() == [[2, 1, 3, 0, 4, -1, -1]] and count.tolist() == [5]
    assert R.same_bits(vals[0, :5], np.array([nan, 7.0, 7.0, 1.0, -0.0])) and np.isnan(vals[0, 5:]).all()
    # -0.0 is below +0.0; a -NaN is the same value as a NaN (the lower column first)
    z = np.array([[-0.0, 0.0, -nan, nan]])
    assert RR.row_topk(z, None, 4)[0].tolist() == [[2, 3, 1, 0]]
    assert RR.same(RR.row_topk(XY, None, 3, lists), RR.row_topk(XY, [0, 1, 2], 3, lists))
