"""The initialization extension (include/glrm_hip_init.h: glrm_hip_init_kmeanspp) is exported by both builds of the engine, stays
OUTSIDE the 37-symbol boundary of include/glrm_hip.h, is bound by name in the Julia file and in _capi, and is refused clearly where it
cannot run.  The numpy transcription the GPU tests compare against (tests/kmeanspp_ref.py) is pinned by hand on a 3 x 2 case."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import kmeanspp_ref as R
import lowrankmodels.jl_amd as L
from lowrankmodels.jl_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lowrankmodels.jl_amd")


def declared(header, pattern):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(" + pattern + r")\s*\(", txt)))


def test_both_builds_export_the_entry_point():
    from lowrankmodels.jl_amd import build
    build.build_all(verbose=False)
    assert declared("glrm_hip_init.h", r"glrm_hip_\w+") == ["glrm_hip_init_kmeanspp"]
    for so in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        lib = ctypes.CDLL(os.path.join(PKG, so), mode=ctypes.RTLD_LOCAL)
        assert hasattr(lib, "glrm_hip_init_kmeanspp"), so


def test_the_boundary_header_is_unchanged():
    assert len(declared("glrm_hip.h", r"glrm_hip_\w+")) == 37 == len(_capi.ABI_SYMBOLS)
    assert "glrm_hip_init_kmeanspp" not in declared("glrm_hip.h", r"glrm_hip_\w+")
    assert _capi.ABI_VERSION == 3


def test_binding_table_lists_the_extension_apart():
    assert _capi.INIT_SYMBOLS == ("init_kmeanspp",)
    assert not set(_capi.INIT_SYMBOLS) & set(_capi.ABI_SYMBOLS)
    assert not set(_capi.INIT_SYMBOLS) & set(_capi.SCALE_SYMBOLS)
    assert sorted("glrm_hip_" + s for s in _capi.INIT_SYMBOLS) == declared("glrm_hip_init.h", r"glrm_hip_\w+")


def test_julia_file_ccalls_declared_symbols_literally():
    src = open(os.path.join(ROOT, "julia", "HipGLRMInit.jl")).read()
    code = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    calls = re.findall(r"ccall\(\s*\(\s*([^,]+?)\s*,", code)
    assert calls, "no ccall found"
    known = set(declared("glrm_hip.h", r"glrm_hip_\w+")) | set(declared("glrm_hip_init.h", r"glrm_hip_\w+"))
    for c in calls:
        assert re.fullmatch(r":glrm_hip_\w+", c), f"ccall target {c!r} is not a literal symbol"
        assert c[1:] in known, c
    assert calls == [":glrm_hip_init_kmeanspp"]
    assert code.count("ccall(") == len(calls)
    assert len(re.findall(r"\bccall\(\s*\(:glrm_hip_\w+, LIB\)\s*,", code)) == len(calls)
    assert re.search(r"function\s+hip_init_kmeanspp!\(", code)
    # the draws, in the reference's order
    assert code.index("randn(rng, k, n)") < code.index("rand(rng, 1:m)") < code.index("rand(rng, k - 1)")
    assert "kmeanspp" in open(os.path.join(ROOT, "julia", "crosscheck.jl")).read()


def small_model(losses=None, k=3):
    rng = np.random.default_rng(0)
    A = np.column_stack([rng.standard_normal(12), rng.random(12) < 0.5])
    return L.GLRM(A, losses or [L.QuadLoss(), L.LogisticLoss()], L.QuadReg(), L.QuadReg(), k, rng=rng)


def test_an_engine_without_the_extension_refuses_clearly():
    import oracle as O
    g = small_model()
    Y0 = g.Y.copy()
    with pytest.raises(_capi.GLRMError) as ei:
        L.init_kmeanspp_(g, np.random.default_rng(1), engine=O.oracle_api())
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "initialization extension" in ei.value.message
    assert np.array_equal(g.Y, Y0)
    with pytest.raises(_capi.GLRMError) as ei:
        O.oracle_api().init_kmeanspp(None, np.zeros((3, 2), order="F"), 0, [0.5, 0.5])
    assert ei.value.code == _capi.ERR_UNSUPPORTED and "initialization extension" in ei.value.message


def test_multidimensional_losses_are_refused_before_y_is_touched():
    g = L.GLRM(np.ones((5, 1)), L.MultinomialLoss(3), L.QuadReg(), L.QuadReg(), 2)
    Y0 = g.Y.copy()
    with pytest.raises(NotImplementedError, match="multi-dimensional"):
        L.init_kmeanspp_(g, np.random.default_rng(1))
    assert np.array_equal(g.Y, Y0) and not hasattr(g, "_init_kmeanspp_info")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_fails_loudly_without_a_gpu():
    from lowrankmodels.jl_amd import build
    build.build_all(verbose=False)
    g = small_model()
    Y0 = g.Y.copy()
    with pytest.raises(_capi.GLRMError) as ei:
        L.init_kmeanspp_(g, np.random.default_rng(1))
    assert ei.value.code == _capi.ERR_HIP and "no CPU fallback" in ei.value.message
    assert np.array_equal(g.Y, Y0)


# ---- the transcription, by hand.  Rows (0-based): 0 observes columns (0, 1) = (1, 2); 1 observes nothing; 2 lists column 0 TWICE:
# (0, 1, 0) with the values (4, 5, 7).  QuadLoss everywhere.
ROWPTR = np.array([0, 2, 2, 5])
COLIDX = np.array([0, 1, 0, 1, 0], dtype=np.int32)
VALS = np.array([1.0, 2.0, 4.0, 5.0, 7.0])
Y0 = np.array([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0]])
QUAD2 = [L.QuadLoss(), L.QuadLoss()]


def ref(first, u, k=3, rowptr=ROWPTR, colidx=COLIDX, vals=VALS, m=3):
    return R.init_kmeanspp(m, 2, k, rowptr, colidx, vals, QUAD2, Y0[:k], first, u)


def test_transcription_nan_row_sends_every_draw_to_row_zero():
    r = ref(0, [0.9, 0.9])
    # round 1: w = (0 [the first centre], NaN [0 / 0], ((1-4)^2 + (2-5)^2 + (1-7)^2) / 3 = 18); sum NaN -> t NaN -> `cw < t` false -> row 0
    assert r["weights"][0][0] == 0.0 and math.isnan(r["weights"][0][1]) and r["weights"][0][2] == 18.0
    assert r["centers"].tolist() == [0, 0, 0] and np.all(np.isinf(r["margins"]))
    assert np.array_equal(r["Y"], [[1.0, 2.0], [1.0, 2.0], [1.0, 2.0]])


def test_transcription_duplicate_column_last_one_wins_and_unobserved_entries_keep_randn():
    r = ref(2, [], k=1)
    assert np.array_equal(r["Y"], [[7.0, 5.0]]) and r["centers"].tolist() == [2]
    rowptr, colidx, vals = np.array([0, 1, 3]), np.array([1, 0, 0], dtype=np.int32), np.array([2.0, 4.0, 7.0])
    r = R.init_kmeanspp(2, 2, 1, rowptr, colidx, vals, QUAD2, Y0[:1], 0, [])
    assert np.array_equal(r["Y"], [[10.0, 2.0]])           # column 0 is not observed by row 0: the draw stays


def test_transcription_only_the_first_centre_leaves_the_candidates():
    # without the empty row: rows 0 = (1, 2), 1 = (4, 5, 7 on columns 0, 1, 0), 2 = (1.5, 2.5)
    rowptr = np.array([0, 2, 5, 7])
    colidx = np.array([0, 1, 0, 1, 0, 0, 1], dtype=np.int32)
    vals = np.array([1.0, 2.0, 4.0, 5.0, 7.0, 1.5, 2.5])
    r = ref(0, [0.5, 0.999], rowptr=rowptr, colidx=colidx, vals=vals)
    w1 = r["weights"][0]
    assert w1.tolist() == [0.0, 18.0, 0.25]                 # t = 0.5 * 18.25 = 9.125: row 1 (cumulative 0, 18, 18.25)
    assert r["centers"][1] == 1 and r["margins"][0] == pytest.approx(min(9.125 - 0, 18 - 9.125) / 18.25)
    assert np.array_equal(r["Y"][1], [7.0, 5.0])
    # round 2: centre 1 stays a candidate with its COMPUTED weight (its distance to itself: ((7-4)^2 + 0 + 0) / 3 = 3, not 0),
    # the first centre stays at 0; row 2: min(0.25, ((7-1.5)^2 + (5-2.5)^2) / 2 = 18.25) = 0.25
    assert r["weights"][1].tolist() == [0.0, 3.0, 0.25]
    assert r["centers"][2] == 2                              # t = 0.999 * 3.25 = 3.24675 > 3


def test_transcription_a_zero_draw_returns_row_zero():
    rowptr = np.array([0, 2, 5, 7])
    colidx = np.array([0, 1, 0, 1, 0, 0, 1], dtype=np.int32)
    vals = np.array([1.0, 2.0, 4.0, 5.0, 7.0, 1.5, 2.5])
    r = ref(2, [0.0], k=2, rowptr=rowptr, colidx=colidx, vals=vals)
    assert r["weights"][0][0] > 0 and r["centers"].tolist() == [2, 0] and math.isinf(r["margins"][0])
    i, margin = R.wsample(np.array([1.0, 2.0, 1.0]), 0.5)   # t = 2: the first running sum that REACHES t (1, 3) -> row 1
    assert (i, margin) == (1, 0.25)
    assert R.wsample(np.array([1.0, 1.0]), 0.5)[0] == 0     # cw = 1 is not < t = 1
    assert R.wsample(np.array([0.0, 0.0]), 0.7)[0] == 0     # sum 0
