"""glrm_hip_row_topk at the shape of BASELINE config C2 and in the few-rows regime (measurements, not gates).

  line 1  C2 of DESIGN.md section 4.15: m = 1e6, n = 1e4, k = 32, standard normal factors, the lists of the C2 recipe (500 observations per
          row from the device generator): every row, kper = 10, exclude = 1, the handle's resident factors.
  line 2  1 024 random query rows at the C4 column geometry (n = 1e5, k = 64; m = 1e6 rows, 100 observations per row): the regime
          where the column spans fill the device.  Also timed with col_splits = 1 (one workgroup per band of 128 rows).
Against
  (a) one counting pass of glrm_hip_xy_select at the shape of line 1, same run, same library: eight passes with the early finish
      off, divided by 8 (tests/perf/bench_xy_select.py);
  (b) what a user does today: fp64 Xq' Y in row blocks on the device with torch, a mask from the lists, torch.topk.  It uses the matrix
      cores and another summation order: context, not a parity reference.
Timing: host clock around the library call (it ends in a stream synchronise) into preallocated host buffers, a warm-up discarded, the
median of the repeats.  `d2h_same_bytes_ms` is a plain device-to-host copy of the bytes the call returns, for scale.
    python tests/perf/bench_recommend.py [--repeats 3] [--out profiles/recommend_c2.json] [--m 1000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=1_000_000)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_c2.json"))
a = ap.parse_args()

import torch  # noqa: E402
from lowrankmodels.jl_amd import _capi, synth  # noqa: E402

api = _capi.hip_api()
dev = torch.device("cuda", 0)


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


def torch_topk(Xd, Yd, rowptr, colidx, rows, kper, block):
    """(b): row blocks of fp64 Xq' Y, -inf at the listed columns, torch.topk; the results go to the host like the library's."""
    out_c, out_v = [], []
    for b0 in range(0, len(rows), block):
        r = rows[b0:b0 + block]
        S = Xd[r] @ Yd.T
        lo, hi = rowptr[r], rowptr[r + 1]
        cnt = hi - lo
        local = torch.repeat_interleave(torch.arange(len(r), device=dev), cnt)
        pos = torch.arange(int(cnt.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt) + torch.repeat_interleave(lo, cnt)
        S[local, colidx[pos].long()] = -float("inf")
        v, c = torch.topk(S, kper, dim=1)
        out_c.append(c.to(torch.int32).cpu()); out_v.append(v.cpu())
    return torch.cat(out_c), torch.cat(out_v)


def setup(m, n, k, q, seed):
    w = synth.DeviceWorkload(m, n, k, q, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0), device=dev)
    h = api.create(w.problem(), profile=0)
    rng = np.random.default_rng(seed)
    X, Y = np.asfortranarray(rng.standard_normal((k, m))), np.asfortranarray(rng.standard_normal((k, n)))
    api.set_factors(h, X, Y)
    Xd, Yd = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev), torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    return w, h, Xd, Yd


def library_call(h, rows, n_rows, kper, col_splits):
    cols, vals, count = np.empty((n_rows, kper), dtype=np.int32), np.empty((n_rows, kper)), np.empty(n_rows, dtype=np.int32)
    fn = api._f["row_topk"]
    rptr = None if rows is None else rows.ctypes.data

    def call():
        rc = fn(h, None, None, rptr, n_rows, kper, 1, col_splits, cols.ctypes.data, vals.ctypes.data, count.ctypes.data)
        assert rc == 0, api.last_error()
    return call, (cols, vals, count)


res = {"how": "host clock around glrm_hip_row_topk on resident factors into preallocated host buffers; warm-up discarded; median of the repeats",
       "repeats": a.repeats, "device": torch.cuda.get_device_name()}

# ---- line 1: C2, every row
m, n, k, q, kper = a.m, 10_000, 32, 500, 10
w, h, Xd, Yd = setup(m, n, k, q, seed=2)
try:
    call, out = library_call(h, None, m, kper, 0)
    ms, ms_min = median_ms(call)
    info = api.row_topk_info()
    os.environ["GLRM_HIP_TOPK_FINISH"] = "0"                        # (a): exactly eight counting passes
    sel_ms, _ = median_ms(lambda: api.xy_select(h, None, None, m * n // 2))
    assert api.xy_select_info() == (8, 0)
    os.environ.pop("GLRM_HIP_TOPK_FINISH", None)
    dbuf = torch.empty(m * kper * 12 + m * 4, dtype=torch.uint8, device=dev)
    d2h_ms, _ = median_ms(lambda: dbuf.cpu())
    rows_all = torch.arange(m, device=dev)
    tt_ms, _ = median_ms(lambda: torch_topk(Xd, Yd, w.rowptr, w.colidx, rows_all, kper, 16384))
    tc, tv = torch_topk(Xd, Yd, w.rowptr, w.colidx, rows_all[:4096], kper, 4096)
    agree = float((tc.numpy() == out[0][:4096]).mean())            # other summation order: near-ties may swap, so a fraction, not a check
    res["c2_all_rows"] = {"shape": {"m": m, "n": n, "k": k, "obs_per_row": q, "kper": kper, "exclude": 1, "rows": "all"},
                          "row_topk_ms": ms, "row_topk_ms_minimum": ms_min, "info": info,
                          "xy_select_counting_pass_ms": sel_ms / 8, "ratio_to_counting_pass": ms / (sel_ms / 8),
                          "d2h_same_bytes_ms": d2h_ms, "torch_gemm_mask_topk_ms": tt_ms, "torch_columns_equal_fraction_first_4096_rows": agree,
                          "count_min": int(out[2].min()), "fma": float(m) * n * k}
    print(json.dumps(res["c2_all_rows"]), flush=True)
finally:
    api.destroy(h)
del w, Xd, Yd, dbuf, rows_all
torch.cuda.empty_cache()

# ---- line 2: 1 024 query rows, C4 column geometry
m, n, k, q, nq = a.m, 100_000, 64, 100, 1024
w, h, Xd, Yd = setup(m, n, k, q, seed=3)
try:
    rows = np.ascontiguousarray(np.random.default_rng(4).choice(m, nq, replace=False).astype(np.int64))
    call, out = library_call(h, rows, nq, kper, 0)
    ms, ms_min = median_ms(call)
    info = api.row_topk_info()
    call1, out1 = library_call(h, rows, nq, kper, 1)
    ms1, _ = median_ms(call1)
    assert all(np.array_equal(x, y) for x, y in zip(out[:1] + out[2:], out1[:1] + out1[2:])) and np.array_equal(out[1].view(np.uint64), out1[1].view(np.uint64))
    rows_d = torch.from_numpy(rows).to(dev)
    tt_ms, _ = median_ms(lambda: torch_topk(Xd, Yd, w.rowptr, w.colidx, rows_d, kper, 1024))
    res["c4_columns_1024_rows"] = {"shape": {"m": m, "n": n, "k": k, "obs_per_row": q, "kper": kper, "exclude": 1, "rows": nq},
                                   "row_topk_ms": ms, "row_topk_ms_minimum": ms_min, "info": info, "row_topk_one_span_ms": ms1,
                                   "torch_gemm_mask_topk_ms": tt_ms, "fma": float(nq) * n * k}
    print(json.dumps(res["c4_columns_1024_rows"]), flush=True)
finally:
    api.destroy(h)

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
