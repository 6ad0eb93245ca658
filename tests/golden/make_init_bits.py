"""Regenerate tests/golden/init_bits.npz: X, Y, the singular values, the iteration counts and (nndsvd) the split products that the HIP
engine returns for the cases of tests/init_bits_cases.py, bit for bit.  Needs the GPU and the built engine.  The record says what a
given build computes, so it is made at the commit whose bits are to be kept: before a change to the init kernels, or, after a toolchain
change, at the parent of that change.  Run:  python tests/golden/make_init_bits.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import init_bits_cases as C  # noqa: E402
from lowrankmodels.jl_amd import _capi  # noqa: E402

if __name__ == "__main__":
    api = _capi.hip_api()
    fixture = {}
    for name in C.CASES:
        first, second = C.run_twice(name, api)
        assert all(C.raw(first[key]) == C.raw(second[key]) for key in first), f"{name}: two calls differ"
        kept = C.record(first)
        fixture.update({f"{name}/{key}": a for key, a in kept.items()})
        print(f"{name}: X {first['X'].shape} Y {first['Y'].shape} iterations {first['iters'].tolist()} s1..s3 {first['sv'][:3]} "
              f"{'in full' if kept['X'].dtype == np.float64 else 'SHA-256'}", flush=True)
    path = os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "init_bits.npz")
    np.savez(path, **fixture)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} kB")
