"""glrm_hip_sample_at beside glrm_hip_impute_at on the same 1e8 uniformly random pairs (measurements, not gates: no draw had a path before).

  c4        BASELINE config C4's geometry, as tests/perf/bench_impute_at.py builds it: m = 1e7, n = 1e5, k = 64, QuadLoss / RealDomain (every
            entry is S1), standard normal resident factors, 4 observations per row.  In one run: impute_at, sample_at under the "given"
            noise rule (sd = 1), and the variance pass alone (a call with no entries that asks for noise_sd_out under the "residual" rule).
  keep      m = 1e6, n = 1e5, k = 64 with 100 observations per row: sample_at with keep_observed = 0 and 1 on the same pairs.
Reported per line: the whole call (host clock around the library call, which ends in a stream synchronise, into preallocated host
buffers; warm-up discarded; median and minimum of the repeats) and -- with --kernel-csv, the `*_kernel_stats.csv` of a
`rocprofv3 --kernel-trace --stats` run of this script with --only LINE, merged afterwards by `--merge-kernels --only LINE` so that the
whole-call figures stay those of the unprofiled run -- the kernel times per call.
    python tests/perf/bench_sample_at.py [--pairs 100000000] [--repeats 3] [--only c4|keep] [--out profiles/sample_at_c4.json]
    python tests/perf/bench_sample_at.py --merge-kernels --only c4|keep --kernel-csv FILE [--out profiles/sample_at_c4.json]"""
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
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--only", choices=["c4", "keep"], default=None)
ap.add_argument("--kernel-csv", default=None)
ap.add_argument("--merge-kernels", action="store_true", help="run nothing: add the kernel times of --kernel-csv to the --only line of --out")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_at_c4.json"))
a = ap.parse_args()

if not a.merge_kernels:
    import torch  # noqa: E402
    from lowrankmodels.jl_amd import _capi, synth  # noqa: E402
    from lowrankmodels.jl_amd.domains import RealDomain, pack_domains  # noqa: E402

    api = _capi.hip_api()
    dev = torch.device("cuda", 0)
SEED = 0x9E3779B97F4A7C15


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


def kernel_ms(*words):
    """(ms per launch, launches) of the one kernel of the rocprofv3 stats whose name holds every word."""
    if not a.kernel_csv:
        return None
    with open(a.kernel_csv) as f:
        rows = [r for r in csv.DictReader(f) if all(w in r["Name"] for w in words)]
    assert len(rows) == 1, (words, [r["Name"] for r in rows])
    return float(rows[0]["TotalDurationNs"]) / int(rows[0]["Calls"]) / 1e6, int(rows[0]["Calls"])


def add_kernels(res, which):
    """The kernel times of a profiled run of the same line (--only c4 / --only keep), merged into the line's figures: per call = the mean
    launch x the blocks of a call (a block is one launch of each kernel; the variance pass is one launch)."""
    if which == "c4":
        ki, ks, kv = kernel_ms("impute_at_fast_kernel"), kernel_ms("sample_at_fast_kernel"), kernel_ms("sa_variance_kernel")
        blocks = res["sample_info"]["blocks"]
        res["impute_at_kernel_ms_per_call"], res["sample_at_kernel_ms_per_call"], res["variance_kernel_ms"] = ki[0] * blocks, ks[0] * blocks, kv[0]
        res["blocks_per_call"] = blocks
        res["kernel_launches_in_profile"] = {"impute": ki[1], "sample": ks[1], "variance": kv[1]}
        res["ratio_kernel_sample_to_impute"] = ks[0] / ki[0]
        res["sample_gather_TB_per_s"] = res["shape"]["pairs"] * 2.0 * res["shape"]["kp"] * 8 / (ks[0] * blocks * 1e-3) / 1e12
    else:
        kf, kk = kernel_ms("sample_at_fast_kernel"), kernel_ms("sa_keep_kernel")
        blocks = res["info"]["blocks"]
        res["sample_at_kernel_ms_per_call"], res["keep_kernel_ms_per_call"] = kf[0] * blocks, kk[0] * blocks
        res["blocks_per_call"] = blocks
        res["kernel_launches_in_profile"] = {"sample": kf[1], "keep": kk[1]}


def workload(m, n, k, per_row):
    w = synth.DeviceWorkload(m, n, k, per_row, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0), device=dev)
    h = api.create(w.problem(), profile=0)
    w.free_sources()
    kp = api.factor_ld(h)
    dX, dY = w.init_factors(kp)
    objc, objr = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64, device=dev)
    api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), objc.data_ptr(), objr.data_ptr())
    return h, kp, (w, dX, dY, objc, objr)


def sample_call(h, doms, rows, cols, P, rule, sd_in, keep, out, kept, sd_out):
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    rc = api._f["sample_at"](h, None, None, doms.ctypes.data, p(rows), P, p(cols), P, 0, SEED, rule, p(sd_in), keep, 0, out.ctypes.data, p(kept), p(sd_out))
    assert rc == 0, api.last_error()


def line_c4(P):
    m, n, k = 10_000_000, 100_000, 64
    h, kp, keepalive = workload(m, n, k, 4)
    try:
        rng = np.random.default_rng(5)
        rows, cols = rng.integers(0, m, P, dtype=np.int64), rng.integers(0, n, P, dtype=np.int64).astype(np.int32)
        doms, out, out_s, ones, sd = pack_domains([RealDomain()] * n), np.empty(P), np.empty(P), np.ones(n), np.empty(n)

        def impute():
            rc = api._f["impute_at"](h, None, None, doms.ctypes.data, rows.ctypes.data, P, cols.ctypes.data, P, 0, None, 0, out.ctypes.data, None, None)
            assert rc == 0, api.last_error()
        res = {"shape": {"m": m, "n": n, "k": k, "kp": kp, "pairs": P, "loss": "QuadLoss", "domain": "RealDomain", "observations_per_row": 4}}
        res["impute_at_ms"], res["impute_at_ms_minimum"] = median_ms(impute)
        res["sample_at_given_ms"], res["sample_at_given_ms_minimum"] = median_ms(lambda: sample_call(h, doms, rows, cols, P, 2, ones, 0, out_s, None, None))
        res["sample_info"] = api.sample_at_info()
        res["ratio_whole_call_sample_to_impute"] = res["sample_at_given_ms"] / res["impute_at_ms"]
        z = out_s - out                                                # sd = 1: the draw minus the score is z
        res["z_mean"], res["z_var"], res["z_abs_max"] = float(z.mean()), float(z.var()), float(np.abs(z).max())
        res["variance_pass_call_ms"], res["variance_pass_call_ms_minimum"] = median_ms(lambda: sample_call(h, doms, None, None, 0, 0, None, 0, out_s, None, sd))
        res["variance_columns"] = api.sample_at_info()["variance_columns"]
        res["noise_sd_median"] = float(np.median(sd))
        return res
    finally:
        api.destroy(h)


def line_keep(P):
    m, n, k = 1_000_000, 100_000, 64
    h, kp, keepalive = workload(m, n, k, 100)
    try:
        rng = np.random.default_rng(6)
        rows, cols = rng.integers(0, m, P, dtype=np.int64), rng.integers(0, n, P, dtype=np.int64).astype(np.int32)
        doms, out, ones, kept = pack_domains([RealDomain()] * n), np.empty(P), np.ones(n), np.zeros(P, dtype=np.uint8)
        res = {"shape": {"m": m, "n": n, "k": k, "kp": kp, "pairs": P, "observations_per_row": 100}}
        res["sample_at_ms"], res["sample_at_ms_minimum"] = median_ms(lambda: sample_call(h, doms, rows, cols, P, 2, ones, 0, out, None, None))
        res["sample_at_keep_observed_ms"], res["sample_at_keep_observed_ms_minimum"] = median_ms(lambda: sample_call(h, doms, rows, cols, P, 2, ones, 1, out, kept, None))
        res["info"] = api.sample_at_info()
        return res
    finally:
        api.destroy(h)


res = {"how": "host clock around the library call on resident factors into preallocated host buffers; warm-up discarded; median of the repeats; "
              "kernel time from a separate rocprofv3 --kernel-trace --stats run where given",
       "repeats": a.repeats}
if os.path.exists(a.out):                                               # a second run (the other line, or the merge) adds to the file
    with open(a.out) as f:
        res.update({k_: v for k_, v in json.load(f).items() if k_ in ("c4", "keep", "device")})
if not a.merge_kernels:
    res["device"] = torch.cuda.get_device_name()
if a.merge_kernels:
    add_kernels(res[a.only], a.only)
    print(json.dumps(res[a.only]), flush=True)
elif a.only in (None, "c4"):
    res["c4"] = line_c4(a.pairs)
    print(json.dumps(res["c4"]), flush=True)
    torch.cuda.empty_cache()
if not a.merge_kernels and a.only in (None, "keep"):
    res["keep"] = line_keep(a.pairs)
    print(json.dumps(res["keep"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
