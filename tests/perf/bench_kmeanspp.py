"""init_kmeanspp! at scale (a measurement, not a gate): glrm_hip_init_kmeanspp on the synthetic row views of BASELINE configs 2 and 4
(C2: 1e6 x 1e4, 500 observations per row; C4: 1e7 x 1e5, 100 per row), generated in HBM and read in place.

A round streams the row view once (12 B per observation: 4 B column index + 8 B value), so its floor is |Omega| * 12 B over the
device's copy bandwidth.  That bandwidth is measured HERE, in the same run: a device-to-device copy of --copy-mib MiB timed with device
events (read + write bytes over the median time).  The time of a round is the difference of two whole calls, on handles with
k = --k-hi and k = --k-lo over the same borrowed lists, divided by the difference in rounds -- the upload of Y, the first scatter and the
copy-out cancel; what does not cancel is the part of the (pageable) upload and download of Y and of the buffer allocation that grows
with k, so the figure is an UPPER bound on the five kernels of a round.  Warm-up, then the median of the repeats.
    python tests/perf/bench_kmeanspp.py [--configs C2,C4] [--k-lo 2 --k-hi 10] [--repeats 5] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench_legs import CONFIGS  # noqa: E402
from lowrankmodels.jl_amd import _capi  # noqa: E402
from lowrankmodels.jl_amd.synth import DeviceWorkload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="C2,C4")
ap.add_argument("--k-lo", type=int, default=2)
ap.add_argument("--k-hi", type=int, default=10)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--copy-mib", type=int, default=2048)
ap.add_argument("--rows", type=int, default=0, help="override the rows of every config (rehearsals)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
import torch  # noqa: E402

api = _capi.hip_api()
dev = torch.device("cuda", 0)


def copy_bandwidth():
    """bytes per second of a device-to-device copy (read + write), median of 9 after 2 warm-ups."""
    n = a.copy_mib << 20
    src = torch.empty(n, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    ts = []
    for i in range(11):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize(dev)
        if i >= 2:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    del src, dst
    torch.cuda.empty_cache()
    return 2.0 * n / float(np.median(ts))


def call_ms(w, k):
    prob = w.problem(borrow=True)
    prob.k = k
    h = api.create(prob, tiled=1)   # gather families: the cheapest set-up; the call reads the row view, whatever the sweeps would run
    try:
        rng = np.random.default_rng(k)
        Y0, u = np.asfortranarray(rng.standard_normal((k, w.n))), rng.random(k - 1)
        ts, centers = [], None
        for i in range(a.warmup + a.repeats):
            Y = Y0.copy(order="F")
            t = time.perf_counter()
            centers, _ = api.init_kmeanspp(h, Y, 12345 % w.m, u)
            if i >= a.warmup:
                ts.append(time.perf_counter() - t)
    finally:
        api.destroy(h)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, centers.tolist()


bw = copy_bandwidth()
print(json.dumps({"copy_bandwidth_GBps": bw / 1e9, "copy_MiB": a.copy_mib, "how": "device-to-device copy, read + write bytes, device events"}), flush=True)
res = [{"copy_bandwidth_GBps": bw / 1e9}]
for name in a.configs.split(","):
    cfg = CONFIGS[name]
    m = a.rows or cfg["rows"]
    w = DeviceWorkload(m, cfg["cols"], cfg["k"], cfg["q"], value_model=cfg["value_model"], loss_mix=cfg["loss_mix"])
    lo, lo_min, _ = call_ms(w, a.k_lo)
    hi, hi_min, centers = call_ms(w, a.k_hi)
    nnz = w.nnz_rows
    per_round = (hi - lo) / (a.k_hi - a.k_lo)
    floor = nnz * 12.0 / bw * 1e3
    out = {"config": name, "m": m, "n": cfg["cols"], "observations": nnz, "ms_call_k_lo": lo, "ms_call_k_hi": hi, "k_lo": a.k_lo, "k_hi": a.k_hi,
           "ms_per_round": per_round, "ms_per_round_from_minima": (hi_min - lo_min) / (a.k_hi - a.k_lo), "stream_floor_ms": floor,
           "floor_over_round": floor / per_round, "achieved_stream_GBps": nnz * 12.0 / (per_round * 1e-3) / 1e9, "repeats": a.repeats,
           "centers_k_hi": centers}
    print(json.dumps(out), flush=True)
    res.append(out)
    w.free_sources()
    del w
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
