"""fp32 storage on the gather sweeps against the fp64 production kernels, on the C4 recipe of bench.py:
QuadLoss, rank 64, 100 observations per row, 100 000 columns, NonNegConstraint on both factors; 1e9 observations (1e8 when the three
handles do not fit together).

    python tests/perf/bench_storage.py [--obs 1e9] [--iters 10] [--rounds 3] [--out profiles/storage_f32_c4.json]

One process, three handles on the same device data:  (a) fp64, the engine's own choice of kernel families (cached rows + phase-aligned
columns at this shape);  (b) fp64, gather sweeps only (tiled = 1);  (c) storage = f32 (gather sweeps).  Every leg is warmed up, then the
legs take turns: `rounds` rounds of `iters` outer iterations each, timed with device events around every half-step, so that the spread
between rounds is known.  All legs start from the same factors and run the same number of iterations; the final objectives of (b) and
(c) are printed side by side.  These are measurements, not targets."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="auto", help="1e9, 1e8 or auto (1e9, falling back to 1e8 when a handle cannot be created)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "storage_f32_c4.json"))
    args = ap.parse_args()
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    api = _capi.hip_api()
    n, k, q = 100_000, 64, 100
    sizes = [1e9, 1e8] if args.obs == "auto" else [float(args.obs)]
    legs_spec = [("a_f64_auto", dict(tiled=0, storage=0)), ("b_f64_gather", dict(tiled=1, storage=0)), ("c_f32_gather", dict(tiled=0, storage=1))]
    stream = torch.cuda.current_stream().cuda_stream
    for obs in sizes:
        m = int(obs) // q
        w = synth.DeviceWorkload(m, n, k, q, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0))
        legs = []
        try:
            for name, o in legs_spec:
                h = api.create(w.problem(), stream=stream, profile=0, **o)
                legs.append(dict(name=name, h=h, opts=o))
            break
        except (_capi.GLRMError, RuntimeError) as e:
            for leg in legs:
                api.destroy(leg["h"])
            if obs == sizes[-1]:
                raise
            print(f"{obs:.0e} observations: {e}; falling back", flush=True)
            del w
            torch.cuda.empty_cache()
    ld = api.factor_ld(legs[0]["h"])
    X0, Y0 = w.init_factors(ld)
    X0.abs_().mul_(1.0 / k ** 0.5)
    Y0.abs_().mul_(1.0 / k ** 0.5)
    w.free_sources()
    for leg in legs:
        f32 = leg["opts"]["storage"] == 1
        leg["dX"] = X0.float() if f32 else X0.clone()
        leg["dY"] = Y0.float() if f32 else Y0.clone()
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
    total_iters = args.rounds * args.iters
    out = dict(recipe="C4", m=m, n=n, k=k, obs_per_row=q, observations=m * q, iters_per_round=args.iters, rounds=args.rounds,
               warmup=args.warmup, device=torch.cuda.get_device_name(), legs={})
    for leg in legs:
        st = api.kernel_stats(leg["h"])
        f32 = leg["opts"]["storage"] == 1
        s = 4 if f32 else 8
        ms_x = [r[0] for r in leg["rounds"]]
        ms_y = [r[1] for r in leg["rounds"]]
        ms_it = [x + y for x, y in leg["rounds"]]
        best = min(ms_it)
        out["legs"][leg["name"]] = dict(
            options=leg["opts"], families=st["tiled"], waves_row=st["waves_row"], waves_col=st["waves_col"],
            ms_per_iteration_by_round=ms_it, ms_x_by_round=ms_x, ms_y_by_round=ms_y,
            ms_per_iteration=float(np.median(ms_it)), ms_x=float(np.median(ms_x)), ms_y=float(np.median(ms_y)),
            updates_per_s=2.0 * m * q / (float(np.median(ms_it)) * 1e-3), best_round_ms=best,
            # one pass over a view reads, per observation, its index, its value and the opposing k-vector (computed from the shapes)
            bytes_per_observation_per_pass=4 + s + ld * s,
            passes_x=1.0 + st["trials_x"] / (m * total_iters), passes_y=1.0 + st["trials_y"] / (n * total_iters),
            final_objective=api.sum(leg["h"], leg["objcol"].data_ptr(), n))
    L_ = out["legs"]
    out["ratio_c_over_b"] = L_["c_f32_gather"]["ms_per_iteration"] / L_["b_f64_gather"]["ms_per_iteration"]
    out["ratio_c_over_a"] = L_["c_f32_gather"]["ms_per_iteration"] / L_["a_f64_auto"]["ms_per_iteration"]
    out["final_objective_b_c"] = [L_["b_f64_gather"]["final_objective"], L_["c_f32_gather"]["final_objective"]]
    for leg in legs:
        api.destroy(leg["h"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
