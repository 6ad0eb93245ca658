"""The scaling pass at scale (a measurement, not a gate): glrm_hip_scale_columns with device arrays on
  * the C5-family recipe at the size of tests/golden/jref_C5.json (150 000 x 30 000, 9e7 observations, Quad / Logistic / OrdinalHinge
    columns by f mod 3),
  * a uniform QuadLoss model of the same size, and the same values under one L1Loss descriptor (every column a median column),
next to what a user did before: the host transcription (tests/extras/scaling.py) passed as a callable, timed on a 1/100 sample of the
columns and EXTRAPOLATED (labelled as such).  Warm-up, then the median of the repeats.
    python tests/perf/bench_scale.py [--m 150000 --n 30000 --q 600 --repeats 9] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lowrankmodels.jl_amd as L  # noqa: E402
from lowrankmodels.jl_amd import _capi  # noqa: E402
from lowrankmodels.jl_amd.synth import DeviceWorkload  # noqa: E402

HBM_BYTES_PER_S = 8e12   # the HBM figure of DESIGN.md section 5
# passes over colvals out of memory per kind for a column that fits the LDS staging (csrc/glrm_scale.hip): moments + second moment / loss;
# the selection of a staged column reads LDS only.  A longer median column adds 8 (one per digit) and at most 1 (upper neighbour).
PASSES = {0: 2, 1: 2, 2: 2, 3: 2, 4: 2, 5: 2, 6: 2, 7: 2, 8: 2}
STREAMED_EXTRA = 9

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=150000)
ap.add_argument("--n", type=int, default=30000)
ap.add_argument("--q", type=int, default=600)
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--host-sample", type=int, default=100, help="the host transcription runs on every N-th column")
ap.add_argument("--out", default=None)
a = ap.parse_args()
api = _capi.hip_api()


def timed(prob, mode):
    for _ in range(a.warmup):
        api.scale_columns(prob, mode)
    ts = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        api.scale_columns(prob, mode)
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3


def line(name, w, losses):
    prob = w.problem()
    prob.losses = losses
    lens = np.diff(w.colptr.cpu().numpy())
    kinds = np.broadcast_to(losses["kind"], (w.n,)) if len(losses) == 1 else losses["kind"]
    median_kind = np.isin(kinds, (1, 2, 3, 6))
    passes = np.array([PASSES[int(kd)] for kd in kinds]) + STREAMED_EXTRA * (median_kind & (lens > 4096))
    nbytes = float(np.sum(passes * lens) * 8)
    ms, ms_min = timed(prob, _capi.SCALE_EQUILIBRATE)
    per_kind = {int(kd): {"columns": int(np.sum(kinds == kd)), "passes_over_colvals": float(np.mean(passes[kinds == kd]))} for kd in np.unique(kinds)}
    out = {"model": name, "m": w.m, "n": w.n, "observations": int(w.nnz_cols), "longest_column": int(lens.max()), "ms_median": ms, "ms_min": ms_min,
           "repeats": a.repeats, "per_kind": per_kind, "bytes_read_model": nbytes, "achieved_bytes_per_s": nbytes / (ms * 1e-3),
           "fraction_of_hbm_8e12": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}
    print(json.dumps(out), flush=True)
    return out


def host_transcription(w, losses):
    """What `scale=<callable>` costs today: tests/extras/scaling.py on every host_sample-th column, extrapolated to all of them."""
    import extras as E
    colptr, colvals = w.colptr.cpu().numpy(), w.colvals.cpu().numpy()
    table = {0: L.QuadLoss, 7: L.LogisticLoss, 6: lambda: L.OrdinalHingeLoss(1, 5), 1: L.L1Loss}
    cols = range(0, w.n, a.host_sample)
    t = time.perf_counter()
    for f in cols:
        col = colvals[colptr[f]:colptr[f + 1]]
        l = table[int(losses["kind"][f if len(losses) > 1 else 0])]()
        if len(col):
            E.avgerror(l, col)
            np.var(col, ddof=1) if len(col) > 1 else None
    dt = time.perf_counter() - t
    out = {"host_transcription": {"columns_timed": len(cols), "seconds_on_the_sample": dt, "seconds_extrapolated_to_all_columns": dt * w.n / len(cols),
                                  "note": "EXTRAPOLATED from every %d-th column; one Python call per observation" % a.host_sample}}
    print(json.dumps(out), flush=True)
    return out


res = []
w = DeviceWorkload(a.m, a.n, a.k, a.q, loss_mix=1)
res.append(line("C5 family (Quad / Logistic / OrdinalHinge by f mod 3)", w, w.losses))
res.append(host_transcription(w, w.losses))
w.free_sources()
del w
w = DeviceWorkload(a.m, a.n, a.k, a.q, loss_mix=0)
res.append(line("uniform QuadLoss", w, w.losses))
res.append(line("the same values, one L1Loss descriptor (every column a median column)", w, np.array([(1, 0, 1.0, 0.0, 0.0)], dtype=_capi.LOSS_DTYPE)))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
