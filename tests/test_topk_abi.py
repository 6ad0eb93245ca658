"""The top-k extension (include/glrm_hip_topk.h) without a GPU: the built libraries export what the header declares, an engine without
the extension is refused by name, the driver is part of the package, and the numpy restatement the GPU tests compare against
(tests/precision_ref.py) orders values like Julia's isless."""
import ctypes
import os

import numpy as np
import pytest

import lowrankmodels.jl_amd as L
import oracle as O
import precision_ref as R
from lowrankmodels.jl_amd import _capi
from test_abi import PKG, declared, ensure_built


def test_libraries_export_every_symbol_the_header_declares():
    ensure_built()
    names = declared("glrm_hip_topk.h", "glrm_hip_")
    assert names == sorted("glrm_hip_" + s for s in _capi.TOPK_SYMBOLS) and len(names) == 3
    assert not set(_capi.TOPK_SYMBOLS) & set(_capi.ABI_SYMBOLS)          # outside the 37-symbol boundary
    for lib in ("libglrm_hip.so", "libglrm_hip_testing.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib), mode=ctypes.RTLD_LOCAL)
        for n in names:
            assert hasattr(so, n), (lib, n)


def test_the_oracle_engine_is_refused_by_name():
    api = O.oracle_api()
    for call in (lambda: api.xy_select(None, None, None, 1), lambda: api.precision_scan(None, None, None, 0.0, [0], [], 1), api.xy_select_info):
        with pytest.raises(_capi.GLRMError) as ei:
            call()
        assert ei.value.code == _capi.ERR_UNSUPPORTED and "include/glrm_hip_topk.h" in ei.value.message


def test_precision_at_k_is_part_of_the_package():
    assert callable(L.precision_at_k) and "precision_at_k" in L.__all__
    from lowrankmodels.jl_amd.crossval import precision_at_k
    assert precision_at_k is L.precision_at_k


def test_restatement_orders_like_isless():
    vals = np.array([np.nan, np.inf, 1.0, 5e-324, 0.0, -0.0, -5e-324, -1.0, -np.inf])
    k = R.keys(vals)
    assert np.all(k[:-1] > k[1:])                                        # NaN > +Inf > .. > +0.0 > -0.0 > .. > -Inf
    assert R.keys(np.array([-np.nan]))[0] == k[0]                        # every NaN is one value
    assert all(R.same_bits(R.unkey(kk), v) for kk, v in zip(k[1:], vals[1:])) and np.isnan(R.unkey(k[0]))
    s = R.Sorted(np.array([[1.0, 2.0, 2.0], [np.nan, -0.0, 0.0]]))
    assert np.isnan(s.select(1)[0]) and s.select(1)[1:] == (0, 1)
    assert s.select(2) == (2.0, 1, 2) and s.select(3) == (2.0, 1, 2) and s.select(4) == (1.0, 3, 1)
    q5, q6 = s.select(5), s.select(6)
    assert R.same_bits(q5[0], 0.0) and q5[1:] == (4, 1) and R.same_bits(q6[0], -0.0) and q6[1:] == (5, 1)
    with pytest.raises(IndexError):
        s.select(7)


def test_restatement_scan_stops_like_the_reference_loop():
    XY = np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.0]])
    train, test = [[0], [], [1]], [[2], [1, 1], []]
    assert R.scan(XY, 1.0, train, test, 0) == (0, 0, [], 0)
    assert R.scan(XY, 1.0, train, test, 1) == (1, 0, [(0, 2, True)], 1)
    assert R.scan(XY, 1.0, train, test, 3) == (2, 1, [(0, 2, True), (1, 0, False), (1, 1, True)], 2)
    assert R.scan(XY, 1.0, train, test, 9) == (2, 2, [(0, 2, True), (1, 0, False), (1, 1, True), (1, 2, False)], 3)
    assert R.scan(XY, np.nan, train, test, 9) == (0, 0, [], 3)
