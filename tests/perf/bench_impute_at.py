"""glrm_hip_impute_at on 1e8 uniformly random pairs (measurements, not gates).

  c4        BASELINE config C4's geometry: m = 1e7, n = 1e5, k = 64, QuadLoss, standard normal resident factors (generated on the device
            and bound, so no 5 GB host copy of X exists).  The model's lists are the device generator's, 4 observations per row: the
            call never reads them.  No route to these entries exists without the extension: glrm_hip_impute would need 8 TB.
  versus    m = 1e5, n = 1e4, k = 32: the same 1e8 pairs count against glrm_hip_impute of the whole 1e9-entry matrix (8 GB on the device
            and on the host), the only route the engine had.
Reported per line: the whole call (host clock around the library call, which ends in a stream synchronise, into preallocated host
buffers; warm-up discarded; median of the repeats), the plain copies of the same bytes through pageable memory (12 B of indices per
pair up, 8 B of output per pair down) timed separately, and -- with --kernel-csv, the `*_kernel_stats.csv` of a
`rocprofv3 --kernel-trace --stats` run of this script with the same --warmup / --repeats -- the kernel time per call and the gather rate
it implies (2 x kp x 8 B per pair over the kernel time; the measured gather ceiling of bench_legs.py is 8.2 TB/s, Infinity-Cache resident).
    python tests/perf/bench_impute_at.py [--pairs 100000000] [--repeats 3] [--only c4|versus] [--kernel-csv FILE] [--out profiles/impute_at_c4.json]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=100_000_000)
ap.add_argument("--m", type=int, default=10_000_000)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--only", choices=["c4", "versus"], default=None)
ap.add_argument("--kernel-csv", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impute_at_c4.json"))
a = ap.parse_args()

import torch  # noqa: E402
from lowrankmodels.jl_amd import _capi, synth  # noqa: E402
from lowrankmodels.jl_amd.domains import RealDomain, pack_domains  # noqa: E402

api = _capi.hip_api()
dev = torch.device("cuda", 0)
KERNEL = "impute_at_fast_kernel"


def median_ms(fn):
    ts = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3


def kernel_ms_per_call(calls):
    """Total time of the fast kernel in the rocprofv3 stats over the library calls of that run (same --warmup / --repeats, one line only)."""
    if not a.kernel_csv:
        return None
    with open(a.kernel_csv) as f:
        rows = [r for r in csv.DictReader(f) if KERNEL in r["Name"]]
    assert len(rows) == 1, [r["Name"] for r in rows]
    return float(rows[0]["TotalDurationNs"]) / calls / 1e6, int(rows[0]["Calls"])


def line(m, n, k, P, seed, versus_full):
    w = synth.DeviceWorkload(m, n, k, 4, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0), device=dev)
    h = api.create(w.problem(), profile=0)
    w.free_sources()
    try:
        kp = api.factor_ld(h)
        dX, dY = w.init_factors(kp)
        objc, objr = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64, device=dev)
        api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), objc.data_ptr(), objr.data_ptr())
        rng = np.random.default_rng(seed)
        rows, cols = rng.integers(0, m, P, dtype=np.int64), rng.integers(0, n, P, dtype=np.int64).astype(np.int32)
        doms = pack_domains([RealDomain()] * n)
        out = np.empty(P)
        fn = api._f["impute_at"]

        def call():
            rc = fn(h, None, None, doms.ctypes.data, rows.ctypes.data, P, cols.ctypes.data, P, 0, None, 0, out.ctypes.data, None, None)
            assert rc == 0, api.last_error()
        ms, ms_min = median_ms(call)
        res = {"shape": {"m": m, "n": n, "k": k, "kp": kp, "pairs": P, "loss": "QuadLoss", "factors": "standard normal, resident"},
               "impute_at_ms": ms, "impute_at_ms_minimum": ms_min, "info": api.impute_at_info(), "pairs_per_s_whole_call": P / (ms * 1e-3)}
        # a few entries against the chain, on the host
        Xs = dX.view(m, kp)[torch.from_numpy(rows[:64]).to(dev)].cpu().numpy()
        Ys = dY.view(n, kp)[torch.from_numpy(cols[:64].astype(np.int64)).to(dev)].cpu().numpy()
        u = np.zeros(64)
        for c in range(k):
            u = Xs[:, c] * Ys[:, c] + u
        res["max_abs_diff_first_64_vs_unfused_host_chain"] = float(np.abs(u - out[:64]).max())
        # the plain copies of the same bytes through pageable memory
        d_rows, d_cols, d_out = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        t_rows, t_cols, t_out = torch.from_numpy(rows), torch.from_numpy(cols), torch.from_numpy(np.empty(P))   # (a host buffer of its own: `out` is compared below)
        res["h2d_12B_per_pair_ms"], _ = median_ms(lambda: (d_rows.copy_(t_rows), d_cols.copy_(t_cols)))
        res["d2h_8B_per_pair_ms"], _ = median_ms(lambda: t_out.copy_(d_out))
        res["copies_ms"] = res["h2d_12B_per_pair_ms"] + res["d2h_8B_per_pair_ms"]
        del d_rows, d_cols, d_out, t_out
        km = kernel_ms_per_call(a.warmup + a.repeats)
        if km:
            res["kernel_ms_per_call"], res["kernel_launches_in_profile"] = km
            res["gather_bytes_per_pair"] = 2 * kp * 8
            res["gather_TB_per_s"] = P * 2.0 * kp * 8 / (km[0] * 1e-3) / 1e12
            res["gather_ceiling_TB_per_s_bench_legs"] = 8.2
        if versus_full:
            X, Y = np.zeros((k, m), order="F"), np.zeros((k, n), order="F")
            api.get_factors(h, X, Y)
            Ahat = np.empty((m, n), order="F")
            imp = api._f["impute"]

            def full():
                rc = imp(h, X.ctypes.data, Y.ctypes.data, doms.ctypes.data, Ahat.ctypes.data)
                assert rc == 0, api.last_error()
            res["full_impute_ms"], res["full_impute_ms_minimum"] = median_ms(full)
            res["full_impute_entries"] = m * n
            res["same_bits_as_full_impute"] = bool(np.array_equal(Ahat[rows, cols].view(np.uint64), out.view(np.uint64)))
            res["ratio_full_impute_to_impute_at"] = res["full_impute_ms"] / ms
        return res
    finally:
        api.destroy(h)


res = {"how": "host clock around the library call on resident factors into preallocated host buffers; warm-up discarded; median of the repeats; "
              "kernel time from a separate rocprofv3 --kernel-trace --stats run where given",
       "repeats": a.repeats, "device": torch.cuda.get_device_name()}
if os.path.exists(a.out):                                               # a second run (the other line, or the profiled one) adds to the file
    with open(a.out) as f:
        res.update({k_: v for k_, v in json.load(f).items() if k_ in ("c4", "versus_full_impute")})
if a.only in (None, "c4"):
    res["c4"] = line(a.m, 100_000, 64, a.pairs, 5, False)
    print(json.dumps(res["c4"]), flush=True)
    torch.cuda.empty_cache()
if a.only in (None, "versus"):
    res["versus_full_impute"] = line(100_000, 10_000, 32, a.pairs, 6, True)
    print(json.dumps(res["versus_full_impute"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
