"""glrm_hip_xy_select at the shape of BASELINE config C2 (a measurement, not a gate): the rank-th largest entry of X'Y for
m = 1e6, n = 1e4, k = 32, rank = 5e8, standard normal factors generated from a seed.  The reference cannot run this shape at all
(XY alone is 80 GB), so there is no reference time beside it.

A pass recomputes every u_ij: m n k fma, so its floor is m n k over the fp64 vector rate (78.6 TFLOP/s rating = 39.3e12 fma/s).
  time per pass   one call with GLRM_HIP_TOPK_FINISH=0 (no early finish: exactly eight counting passes) on the handle's resident factors,
                  host clock around the call (it ends in a stream synchronise), divided by 8; median of the repeats after a warm-up.  The
                  eight small reduce kernels and 2 KB copies are inside that figure.
  default call    the same call with the early finish on: its time, its pass count and the keys its last pass sorted
                  (glrm_hip_xy_select_info).
The model's lists are irrelevant to the selection; the handle holds one observation per row.
    python tests/perf/bench_xy_select.py [--m 1000000 --n 10000 --k 32 --rank 500000000] [--repeats 3] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import lowrankmodels.jl_amd as L  # noqa: E402
from lowrankmodels.jl_amd import _capi  # noqa: E402
from lowrankmodels.jl_amd.losses import pack_losses  # noqa: E402
from lowrankmodels.jl_amd.regularizers import pack_regs  # noqa: E402

FP64_VECTOR_FMA_PER_S = 78.6e12 / 2

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=1_000_000)
ap.add_argument("--n", type=int, default=10_000)
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--rank", type=int, default=500_000_000)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()

api = _capi.hip_api()
m, n, k = a.m, a.n, a.k
rng = np.random.default_rng(2)
X = np.asfortranarray(rng.standard_normal((k, m)))
Y = np.asfortranarray(rng.standard_normal((k, n)))

t = np.arange(max(m, n), dtype=np.int64)
I, J = t % m, t % n
pr, pc = np.argsort(I, kind="stable"), np.argsort(J, kind="stable")
rowptr = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=m))]).astype(np.int64)
colptr = np.concatenate([[0], np.cumsum(np.bincount(J, minlength=n))]).astype(np.int64)
vals = np.ones(len(t))
pa = _capi.ProblemArrays(m, n, k, rowptr, np.ascontiguousarray(J[pr].astype(np.int32)), vals, colptr, np.ascontiguousarray(I[pc].astype(np.int32)), vals,
                         pack_losses([L.QuadLoss()]), pack_regs([L.ZeroReg()]), pack_regs([L.ZeroReg()]))


def timed(finish):
    if finish is None:
        os.environ.pop("GLRM_HIP_TOPK_FINISH", None)
    else:
        os.environ["GLRM_HIP_TOPK_FINISH"] = finish
    ts, out = [], None
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        out = api.xy_select(h, None, None, a.rank)
        dt = time.perf_counter() - t0
        if i >= a.warmup:
            ts.append(dt)
    return float(np.median(ts)), float(np.min(ts)), out, api.xy_select_info()


h = api.create(pa, tiled=1)
try:
    api.set_factors(h, X, Y)
    full_s, full_min, full_out, full_info = timed("0")
    dflt_s, dflt_min, dflt_out, dflt_info = timed(None)
finally:
    api.destroy(h)
assert full_info == (8, 0) and full_out == dflt_out, (full_info, full_out, dflt_out)
fma = float(m) * n * k
per_pass = full_s / 8
res = {"shape": {"m": m, "n": n, "k": k, "rank": a.rank}, "q": dflt_out[0], "n_gt": dflt_out[1], "n_eq": dflt_out[2],
       "ms_per_pass": per_pass * 1e3, "ms_per_pass_from_minimum": full_min / 8 * 1e3, "ms_eight_counting_passes": full_s * 1e3,
       "fma_per_pass": fma, "fp64_vector_floor_ms": fma / FP64_VECTOR_FMA_PER_S * 1e3, "fraction_of_fp64_vector_rate": fma / FP64_VECTOR_FMA_PER_S / per_pass,
       "default_call_ms": dflt_s * 1e3, "default_call_ms_minimum": dflt_min * 1e3, "default_passes": dflt_info[0], "default_sorted_keys": dflt_info[1],
       "repeats": a.repeats, "how": "host clock around glrm_hip_xy_select on resident factors; per pass = the eight-pass call / 8"}
print(json.dumps(res), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
