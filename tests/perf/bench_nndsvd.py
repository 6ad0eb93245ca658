"""init_nndsvd! at scale (a measurement, not a gate): glrm_hip_init_nndsvd on the synthetic workload of BASELINE config 2 generated in
HBM, with max_iters = 0 (the sparse round alone) and max_iters = 2 (two soft-impute rounds: residual pass per view, rank-k term in
both products).  Prints seconds per round and the subspace iterations of every round.
    python tests/perf/bench_nndsvd.py --m 1000000 --n 10000 --q 500 --k 32"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lowrankmodels.jl_amd import _capi  # noqa: E402
from lowrankmodels.jl_amd.synth import DeviceWorkload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=1000000)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--q", type=int, default=500)
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--tol", type=float, default=1e-6)
ap.add_argument("--variant", default="std")
a = ap.parse_args()
api = _capi.hip_api()
w = DeviceWorkload(a.m, a.n, a.k, a.q)
h = api.create(w.problem())
w.free_sources()
X, Y = np.zeros((a.k, a.m), order="F"), np.zeros((a.k, a.n), order="F")
api.init_nndsvd(h, X, Y, variant=a.variant, max_iters=1, svd_max_iter=1, svd_tol=a.tol)  # warm-up (allocations, first touch)
nnz = a.m * a.q
times = {}
for rounds in (0, 2):
    t = time.time()
    info = api.init_nndsvd(h, X, Y, variant=a.variant, max_iters=rounds, svd_max_iter=100, svd_tol=a.tol)
    times[rounds] = (time.time() - t, info["iterations"].tolist())
    print(f"hip: m={a.m} n={a.n} k={a.k} nnz={nnz:.3g} variant={a.variant} max_iters={rounds}: {times[rounds][0]:.2f} s, subspace "
          f"iterations per round {times[rounds][1]}; s1..s3 = {info['singular_values'][:3]}", flush=True)
(t0, it0), (t2, it2) = times[0], times[2]
soft_its = sum(it2[1:])
print(f"round 0: {t0:.2f} s ({t0 / max(it0[0], 1) * 1e3:.0f} ms per subspace iteration = 2 sparse products + 2 orthonormalizations); "
      f"a soft-impute round: {(t2 - t0) / 2:.2f} s ({(t2 - t0) / max(soft_its, 1) * 1e3:.0f} ms per subspace iteration, the residual pass "
      f"over 2 x {nnz:.3g} entries and the rank-{a.k} terms included)")
api.destroy(h)
