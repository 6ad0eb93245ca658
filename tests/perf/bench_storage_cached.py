"""fp32 storage: the cached row sweep against the gather sweeps, on the C4 recipe of bench.py: QuadLoss, rank 64,
100 observations per row, 100 000 columns, NonNegConstraint on both factors; 1e9 observations.  The measurement that decides whether a
float handle takes the family by the fp64 auto rule (csrc/glrm_engine.hpp: GLRM_CACHED_F32_AUTO).

    python tests/perf/bench_storage_cached.py [--obs 1e9] [--iters 10] [--rounds 3] [--out profiles/storage_f32_cached_c4.json]

Method of tests/perf/bench_storage.py: one process, the handles alive together on the same device data, 2 warm-up iterations, then
`rounds` rounds of `iters` outer iterations with the legs taking turns, device events around every half-step, medians over the rounds.
    (c) storage = f32, tiled = 1: the float gather sweeps, rows on one wave (what the mode ran before the family had a float form)
    (d) storage = f32 with the family on (GLRM_HIP_CACHED=1 at create): rows of <= 104 observations on the float cached row sweep
Both legs start from the same factors and run the same number of iterations; their final objectives are recorded side by side.  The rule:
the family is adopted when the median X half-step of (d) is below that of (c) by more than the largest difference between two rounds of
one leg.  The fp64 production figures are quoted from profiles/r12_c4_ab.txt, not re-run.  These are measurements, not targets.

    GLRM_HIP_LIB_PATH=.../libglrm_hip_<tag>.so python tests/perf/bench_storage_cached.py --grid-sweep 50,75,100

adds "resident_grid_sweep" to the file: the X half-step of leg (d) with the persistent kernel launched on that percentage of its resident
grid (is the float kernel latency bound, as the fp64 one is?).  The product library has no switch for this (tools/README.md): the sweep
needs a variant build whose launch_reg_inst scales the grid it computed by the environment variable GLRM_HIP_CACHED_GRID_PCT, one line
added for the measurement; on the product library the three figures come out equal."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1e9")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "storage_f32_cached_c4.json"))
    ap.add_argument("--grid-sweep", default="", help="percentages of the resident grid, e.g. 50,75,100 (variant build only; see above)")
    args = ap.parse_args()
    if args.grid_sweep:
        return grid_sweep(args)
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    api = _capi.hip_api()
    n, k, q = 100_000, 64, 100
    m = int(float(args.obs)) // q
    legs_spec = [("c_f32_gather", dict(tiled=1, storage=1), None), ("d_f32_cached", dict(tiled=1, storage=1), "1")]
    stream = torch.cuda.current_stream().cuda_stream
    w = synth.DeviceWorkload(m, n, k, q, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0))
    legs = []
    keep = os.environ.pop("GLRM_HIP_CACHED", None)
    for name, o, cached in legs_spec:
        if cached is not None:
            os.environ["GLRM_HIP_CACHED"] = cached      # read at create
        h = api.create(w.problem(), stream=stream, profile=0, **o)
        os.environ.pop("GLRM_HIP_CACHED", None)
        legs.append(dict(name=name, h=h, opts=o, cached=cached))
        print(f"created {name}", flush=True)
    if keep is not None:
        os.environ["GLRM_HIP_CACHED"] = keep
    ld = api.factor_ld(legs[0]["h"])
    X0, Y0 = w.init_factors(ld)
    X0.abs_().mul_(1.0 / k ** 0.5)
    Y0.abs_().mul_(1.0 / k ** 0.5)
    w.free_sources()
    for leg in legs:
        leg["dX"], leg["dY"] = X0.float(), Y0.float()
        leg["objcol"] = torch.zeros(n, dtype=torch.float64, device=X0.device)
        leg["objrow"] = torch.zeros(m, dtype=torch.float64, device=X0.device)
        api.bind_buffers(leg["h"], leg["dX"].data_ptr(), leg["dY"].data_ptr(), leg["objcol"].data_ptr(), leg["objrow"].data_ptr())
        api.reset_stepsizes(leg["h"], 1.0)
        leg["rounds"] = []
    del X0, Y0

    def run(leg, iters, timed):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)] if timed else None
        for i in range(iters):
            if timed:
                ev[i][0].record()
            api.step_x(leg["h"], 0.01)
            if timed:
                ev[i][1].record()
            api.step_y(leg["h"], 0.01)
            if timed:
                ev[i][2].record()
        torch.cuda.synchronize()
        if timed:
            return sum(e[0].elapsed_time(e[1]) for e in ev) / iters, sum(e[1].elapsed_time(e[2]) for e in ev) / iters

    for leg in legs:
        run(leg, args.warmup, False)
        api.kernel_stats(leg["h"], reset=True)
    for _ in range(args.rounds):
        for leg in legs:                      # the legs take turns
            leg["rounds"].append(run(leg, args.iters, True))
            print(leg["name"], "ms X / Y per iteration: %.2f / %.2f" % leg["rounds"][-1], flush=True)
    total_iters = args.rounds * args.iters
    out = dict(recipe="C4", m=m, n=n, k=k, obs_per_row=q, observations=m * q, iters_per_round=args.iters, rounds=args.rounds,
               warmup=args.warmup, device=torch.cuda.get_device_name(), legs={})
    for leg in legs:
        st = api.kernel_stats(leg["h"])
        o = api.sum_order(leg["h"], 0).asdict()
        ms_x = [r[0] for r in leg["rounds"]]
        ms_y = [r[1] for r in leg["rounds"]]
        ms_it = [x + y for x, y in leg["rounds"]]
        out["legs"][leg["name"]] = dict(
            options=leg["opts"], GLRM_HIP_CACHED=leg["cached"], families=st["tiled"], waves_row=st["waves_row"], waves_col=st["waves_col"],
            cached_maxlen=o["cached_maxlen"], cached_waves=o["cached_waves"],
            ms_per_iteration_by_round=ms_it, ms_x_by_round=ms_x, ms_y_by_round=ms_y,
            ms_per_iteration=float(np.median(ms_it)), ms_x=float(np.median(ms_x)), ms_y=float(np.median(ms_y)),
            ms_x_spread=max(ms_x) - min(ms_x), updates_per_s=2.0 * m * q / (float(np.median(ms_it)) * 1e-3),
            bytes_per_observation_per_pass=4 + 4 + ld * 4,
            passes_x=1.0 + st["trials_x"] / (m * total_iters), passes_y=1.0 + st["trials_y"] / (n * total_iters),
            iterations=args.warmup + total_iters, final_objective=api.sum(leg["h"], leg["objcol"].data_ptr(), n))
    c, d = out["legs"]["c_f32_gather"], out["legs"]["d_f32_cached"]
    spread = max(c["ms_x_spread"], d["ms_x_spread"])
    out["ms_x_c_minus_d"] = c["ms_x"] - d["ms_x"]
    out["largest_round_to_round_difference_ms_x"] = spread
    out["auto_rule_adopted"] = bool(c["ms_x"] - d["ms_x"] > spread)
    out["final_objective_c_d"] = [c["final_objective"], d["final_objective"]]
    # context, quoted and not re-run: the fp64 production pair (cached rows + phase-aligned columns) since the row-chain work
    out["fp64_production_context"] = dict(source="profiles/r12_c4_ab.txt", ms_x=67.5, ms_y=114.2)
    for leg in legs:
        api.destroy(leg["h"])
    if os.path.exists(args.out):                 # a resident-grid sweep recorded by an earlier run of a variant build stays in the file
        try:
            old = json.load(open(args.out))
            if "resident_grid_sweep" in old:
                out["resident_grid_sweep"] = old["resident_grid_sweep"]
        except ValueError:
            pass
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def grid_sweep(args):
    """Leg (d) alone, one handle per percentage (the grid is computed at a handle's first sweep): median X half-step of `rounds` rounds."""
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    api = _capi.hip_api()
    n, k, q = 100_000, 64, 100
    m = int(float(args.obs)) // q
    stream = torch.cuda.current_stream().cuda_stream
    w = synth.DeviceWorkload(m, n, k, q, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0))
    X0 = Y0 = None
    res = {}
    for pct in [int(p) for p in args.grid_sweep.split(",")]:
        os.environ["GLRM_HIP_CACHED"] = "1"
        os.environ["GLRM_HIP_CACHED_GRID_PCT"] = str(pct)
        h = api.create(w.problem(), stream=stream, profile=0, tiled=1, storage=1)
        del os.environ["GLRM_HIP_CACHED"]
        if X0 is None:
            X0, Y0 = w.init_factors(api.factor_ld(h))
            X0.abs_().mul_(1.0 / k ** 0.5)
            Y0.abs_().mul_(1.0 / k ** 0.5)
        dX, dY = X0.float(), Y0.float()
        objcol = torch.zeros(n, dtype=torch.float64, device=dX.device)
        objrow = torch.zeros(m, dtype=torch.float64, device=dX.device)
        api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), objcol.data_ptr(), objrow.data_ptr())
        api.reset_stepsizes(h, 1.0)
        assert api.kernel_stats(h)["tiled"] & 64
        ms = []
        for r in range(args.rounds + 1):       # (the first round is the warm-up; only step_x is timed, step_y keeps the trajectory the bench's)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.iters)]
            for i in range(args.iters):
                ev[i][0].record()
                api.step_x(h, 0.01)
                ev[i][1].record()
                api.step_y(h, 0.01)
            torch.cuda.synchronize()
            if r:
                ms.append(sum(e[0].elapsed_time(e[1]) for e in ev) / args.iters)
                print(f"resident grid {pct} %: ms X per iteration {ms[-1]:.2f}", flush=True)
        res[str(pct)] = dict(ms_x=float(np.median(ms)), ms_x_by_round=ms)
        api.destroy(h)
        del dX, dY, objcol, objrow
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["resident_grid_sweep"] = dict(percent_of_resident_grid=res, iters_per_round=args.iters, rounds=args.rounds,
                                      library=os.path.basename(_capi.HIP_LIB_PATH))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["resident_grid_sweep"]))


if __name__ == "__main__":
    main()
