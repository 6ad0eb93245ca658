"""The scaling extension (include/glrm_hip_scale.h: glrm_hip_scale_columns) is exported by both builds of the engine, stays OUTSIDE
the 37-symbol boundary of include/glrm_hip.h, is bound by name in the Julia file and in _capi, and is refused clearly by an engine
that does not have it (the CPU oracle)."""
import ctypes
import os
import re

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lowrankmodels.jl_amd")


def declared(header, pattern):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(" + pattern + r")\s*\(", txt)))


def test_both_builds_export_the_scaling_entry_points():
    from lowrankmodels.jl_amd import build
    build.build_all(verbose=False)
    names = declared("glrm_hip_scale.h", r"glrm_hip_scale_\w+")
    assert names == ["glrm_hip_scale_columns"]
    for so in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        lib = ctypes.CDLL(os.path.join(PKG, so), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(lib, n), (so, n)


def test_the_boundary_header_is_unchanged():
    assert len(declared("glrm_hip.h", r"glrm_hip_\w+")) == 37 == len(_capi.ABI_SYMBOLS)
    assert not declared("glrm_hip.h", r"glrm_hip_scale_\w+")
    assert _capi.ABI_VERSION == 3


def test_binding_table_lists_the_extension_apart_from_the_boundary():
    assert "scale_columns" in _capi.SCALE_SYMBOLS
    assert not set(_capi.SCALE_SYMBOLS) & set(_capi.ABI_SYMBOLS)
    assert sorted("glrm_hip_" + s for s in _capi.SCALE_SYMBOLS) == declared("glrm_hip_scale.h", r"glrm_hip_scale_\w+")
    assert (_capi.SCALE_EQUILIBRATE, _capi.SCALE_PROB) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "glrm_hip_scale.h")).read()
    assert re.search(r"#define\s+GLRM_SCALE_EQUILIBRATE\s+0\b", hdr) and re.search(r"#define\s+GLRM_SCALE_PROB\s+1\b", hdr)


def test_julia_file_ccalls_declared_symbols_literally():
    src = open(os.path.join(ROOT, "julia", "HipGLRMScale.jl")).read()
    code = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    calls = re.findall(r"ccall\(\s*\(\s*([^,]+?)\s*,", code)
    assert calls, "no ccall found"
    known = set(declared("glrm_hip.h", r"glrm_hip_\w+")) | set(declared("glrm_hip_scale.h", r"glrm_hip_\w+"))
    for c in calls:
        assert re.fullmatch(r":glrm_hip_\w+", c), f"ccall target {c!r} is not a literal symbol"
        assert c[1:] in known, c
    assert ":glrm_hip_scale_columns" in calls
    assert code.count("ccall(") == len(calls)
    for fn in ("hip_equilibrate_variance!", "hip_prob_scale!"):
        assert re.search(r"function\s+" + re.escape(fn) + r"\(", code), fn


def small_model(**kw):
    rng = np.random.default_rng(0)
    A = np.column_stack([rng.standard_normal(12), rng.random(12) < 0.5])
    return L.GLRM(A, [L.QuadLoss(), L.LogisticLoss()], L.QuadReg(), L.QuadReg(), 2, rng=rng, **kw)


def test_an_engine_without_the_extension_refuses_clearly():
    import oracle as O
    api = O.oracle_api()
    g = small_model()
    with pytest.raises(_capi.GLRMError) as ei:
        L.equilibrate_variance_(g, engine=api)
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "scaling extension" in ei.value.message
    with pytest.raises(_capi.GLRMError):
        L.prob_scale_(g, engine=api)
    assert [l.scale for l in g.losses] == [1.0, 1.0]   # nothing was rewritten


def test_scale_true_with_multidimensional_losses_keeps_its_message():
    with pytest.raises(NotImplementedError, match="multi-dimensional"):
        L.GLRM(np.ones((5, 1)), L.MultinomialLoss(3), L.QuadReg(), L.QuadReg(), 2, scale=True)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_scale_true_fails_loudly_without_a_gpu():
    from lowrankmodels.jl_amd import build
    build.build_all(verbose=False)
    with pytest.raises(_capi.GLRMError) as ei:
        small_model(scale=True)
    assert ei.value.code == _capi.ERR_HIP and "no CPU fallback" in ei.value.message
