"""-m gpu: glrm_hip_init_svd and glrm_hip_init_nndsvd reproduce tests/golden/init_bits.npz bit for bit.

The other init tests hold the factors to 1e-5 and the singular values to 1e-8 and cannot see a changed summation order; the engine
promises a fixed one.  The record was made by tests/golden/make_init_bits.py on an MI355X at the commit before the two units were given
one subspace iteration and one column product (tests/init_bits_cases.py lists the cases and what each covers).  Every case also asserts
that a second call on the same handle returns the bits of the first.

To re-record: python tests/golden/make_init_bits.py at the commit whose bits are to be kept.  A mismatch that appears with a new
compiler or runtime and no change to the kernels is settled by re-recording at the parent of the toolchain change, then checking the
change against that record."""
import os

import numpy as np
import pytest

import init_bits_cases as C
from lowrankmodels.jl_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_bits.npz"))


@pytest.mark.parametrize("name", C.CASES)
def test_init_reproduces_the_recorded_bits(name):
    first, second = C.run_twice(name, _capi.hip_api())
    assert first["iters"].tolist() == [C.FIXED_ITERS] * len(first["iters"])
    for key, a in first.items():
        assert a.shape == second[key].shape and C.raw(a) == C.raw(second[key]), f"{name}/{key}: two calls differ"
    kept = C.record(first)
    assert {f"{name}/{key}" for key in kept} == {f for f in GOLDEN.files if f.startswith(name + "/")}
    for key, a in kept.items():
        want = GOLDEN[f"{name}/{key}"]
        assert a.dtype == want.dtype and a.shape == want.shape and C.raw(a) == C.raw(want), f"{name}/{key} differs from the record"
