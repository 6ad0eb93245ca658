"""glrm_hip_stream_rows measured on two recipes.  A side benchmark, not bench.py, and a measurement, not a target.

    python tests/perf/bench_stream.py [--recipe c2|sparse|both] [--rows N] [--first 1000] [--interval 10] [--rounds 3] [--out-dir profiles]

  c2      the C2 recipe (bench_legs.CONFIGS["C2"]): 10k columns, 500 observations per row, rank 32, QuadReg(1.0) on X and Y.  Every row
          shares a column with the row before it: the plan is ONE chain, one workgroup walks it.
  sparse  100k columns, 20 observations per row, rank 32: levels about a hundred rows wide.
``--rows`` is the number of rows the handle holds (default 1M for both, the recipes' own size); rows first .. rows-1 are streamed.  A
smaller ``--rows`` measures a prefix: the time per row of a chain does not depend on how long the chain is.

One process, one handle with the default options, X and Y bound as device buffers and restored before every pass.  Per recipe:
  plan_ms (the host's pass over the row view, from glrm_hip_stream_info), levels, launches, widest level, mean width;
  a pass level by level and a pass with sequential = 1: wall ms of the call, ms between two device events recorded around the call (they
  enclose the plan, which the host builds while the stream is idle), that minus plan_ms, and the latter per streamed row in microseconds;
  medians over ``rounds`` after one untimed pass of each kind;
  als_solve(h, 0) + als_solve(h, 1) on the same handle, between device events: the on-device yardstick (every row and every column solved
  once, all in parallel).
Results go to <out-dir>/stream_<recipe>.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RECIPES = {"c2": dict(n=10_000, q=500, k=32), "sparse": dict(n=100_000, q=20, k=32)}


def run(name, args):
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    api = _capi.hip_api()
    r = RECIPES[name]
    m, n, q, k = args.rows, r["n"], r["q"], r["k"]
    first, interval, step = args.first, args.interval, 1.0 / args.first
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)
    w = synth.DeviceWorkload(m, n, k, q, value_model=0, rx=(1, 0, 1.0), ry=(1, 0, 1.0))
    h = api.create(w.problem(), stream=stream)
    ld = api.factor_ld(h)
    X0, Y0 = w.init_factors(ld)
    w.free_sources()
    dX, dY = X0.clone(), Y0.clone()
    oc, orow = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64, device=dev)
    sync()
    api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), oc.data_ptr(), orow.data_ptr())

    def restore():
        dX.copy_(X0)
        dY.copy_(Y0)
        sync()

    def one_pass(sequential):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        obj, _ = api.stream_rows(h, m, first, step, interval, sequential=sequential)
        b.record()
        sync()
        wall = (time.perf_counter() - t0) * 1e3
        info = api.stream_info(h)
        return dict(wall_ms=wall, events_ms=a.elapsed_time(b), plan_ms=info["plan_ms"]), info, obj

    out = dict(recipe=name, m=m, n=n, k=k, obs_per_row=q, first=first, interval=interval, stepsize=step, rows_streamed=m - first,
               device=torch.cuda.get_device_name(), rounds=args.rounds)
    for label, sequential in (("by_level", False), ("sequential", True)):
        one_pass(sequential)                                              # untimed
        runs = [one_pass(sequential) for _ in range(args.rounds)]
        info, obj = runs[-1][1], runs[-1][2]
        med = {f: float(np.median([t[0][f] for t in runs])) for f in ("wall_ms", "events_ms", "plan_ms")}
        med["events_minus_plan_ms"] = med["events_ms"] - med["plan_ms"]
        med["us_per_row"] = med["events_minus_plan_ms"] * 1e3 / max(m - first, 1)
        out[label] = dict(med, by_round=[t[0] for t in runs], levels=info["nlevels"], launches=info["nlaunches"], max_width=info["max_width"],
                          mean_width=(m - first) / max(info["nlevels"], 1), solved=info["solved"], kept_short=info["kept_short"],
                          kept_pivot=info["kept_pivot"], objective_finite=bool(np.all(np.isfinite(obj[np.isfinite(obj)]))),
                          objective_mean_last_1000=float(np.nanmean(obj[-1000:])))
    # the yardstick: every row and every column solved once
    restore()
    ms = []
    for i in range(args.rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        api.als_solve(h, 0)
        api.als_solve(h, 1)
        b.record()
        sync()
        if i:
            ms.append(a.elapsed_time(b))
    out["als_solve_rows_then_cols_ms"] = float(np.median(ms))
    api.destroy(h)
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"stream_{name}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    del dX, dY, X0, Y0, oc, orow
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recipe", choices=("c2", "sparse", "both"), default="both")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--first", type=int, default=1000)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    for name in (("c2", "sparse") if args.recipe == "both" else (args.recipe,)):
        run(name, args)


if __name__ == "__main__":
    main()
