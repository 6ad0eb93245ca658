"""fp32 storage on the phase-aligned gather passes, on the C4 recipe of bench.py with bench_storage.py's method:
QuadLoss, rank 64, 100 observations per row, 100 000 columns, NonNegConstraint on both factors, 1e9 observations; one process, the
handles alive together on the same device data, 2 warm-up iterations, then `rounds` rounds of `iters` outer iterations with the legs
taking turns, device events around every half-step, medians over the rounds.

    python tests/perf/bench_storage_blocked.py [--obs 1e9] [--iters 10] [--rounds 3] [--out profiles/storage_f32_blocked_c4.json]
    python tests/perf/bench_storage_blocked.py --gates                                             # leg (e) alone: the phase gate, added to the same file
    GLRM_HIP_LIB_PATH=<variant build> python tests/perf/bench_storage_blocked.py --bound NAME      # leg (e) alone, added to the same file

Legs:  (a) fp64, the engine's choice;  (c) storage = f32 on the gather sweeps (what an f32 handle runs by default: the baseline);
(e) f32 with GLRM_HIP_BLOCKED=2, the Y half-step on the float phase-aligned passes;  (f) (e) plus GLRM_HIP_CACHED=1, the f32 form of the
production pair.  --gates: one handle of leg (e) under GLRM_HIP_BLOCKED_GATE = 5 120 ... 65 536 rows (the gate is read at
every pass and changes no sum); every timing starts again from the initial factors and step sizes, so that all settings time the same
iterations -- the number of trial rounds of a Y half-step changes along a fit.  --bound: the same leg (e) on another build of the library (build.py --variant with
GLRM_BLOCKED_F32_GRAD_WAVES=<waves per SIMD the float QuadLoss gradient pass is built for>), stored under "waves_per_simd".
Reported: (e) / (c) on the Y half-step, (f) / (a) and (f) / (c) on the iteration, each beside the largest round-to-round difference of
one leg.  These are measurements, not targets."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GATES = (5120, 8192, 10240, 16384, 24576, 32768, 65536)
LEGS = [("a_f64_auto", dict(tiled=0, storage=0), {}),
        ("c_f32_gather", dict(tiled=0, storage=1), {}),
        ("e_f32_blocked_cols", dict(tiled=0, storage=1), {"GLRM_HIP_BLOCKED": "2"}),
        ("f_f32_blocked_cols_cached_rows", dict(tiled=0, storage=1), {"GLRM_HIP_BLOCKED": "2", "GLRM_HIP_CACHED": "1"})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="1e9")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gates", action="store_true", help="run leg (e) alone under the phase-gate settings and add them to the file")
    ap.add_argument("--bound", default=None, help="run leg (e) alone on the library GLRM_HIP_LIB_PATH names and file it under this name")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "storage_f32_blocked_c4.json"))
    args = ap.parse_args()
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    api = _capi.hip_api()
    n, k, q = 100_000, 64, 100
    m = int(float(args.obs)) // q
    spec = [s for s in LEGS if s[0].startswith("e_")] if (args.bound or args.gates) else LEGS
    stream = torch.cuda.current_stream().cuda_stream
    w = synth.DeviceWorkload(m, n, k, q, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0))
    legs = []
    for name, o, env in spec:
        for key in ("GLRM_HIP_BLOCKED", "GLRM_HIP_CACHED", "GLRM_HIP_BLOCKED_GATE"):
            os.environ.pop(key, None)
        os.environ.update(env)         # the family switches are read when the handle is created
        legs.append(dict(name=name, h=api.create(w.problem(), stream=stream, profile=0, **o), opts=o, env=env))
        print(f"created {name}: families {api.kernel_stats(legs[-1]['h'])['tiled']}", flush=True)
    for key in ("GLRM_HIP_BLOCKED", "GLRM_HIP_CACHED"):
        os.environ.pop(key, None)
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
    X0f, Y0f = X0.float(), Y0.float()
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

    if args.gates:
        # every (round, setting) runs iterations warmup + 1 .. warmup + iters of the same fit: the same sums, the same trial rounds
        e = legs[0]
        gate = {str(g): [] for g in GATES}
        for r in range(args.rounds):
            for g in GATES:                   # the settings take turns
                os.environ["GLRM_HIP_BLOCKED_GATE"] = str(g)
                e["dX"].copy_(X0f)
                e["dY"].copy_(Y0f)
                api.reset_stepsizes(e["h"], 1.0)
                run(e, args.warmup, False)
                gate[str(g)].append(run(e, args.iters, True)[1])
            print(f"round {r}: " + ", ".join(f"gate {g}: y {v[-1]:.1f} ms" for g, v in gate.items()), flush=True)
        os.environ.pop("GLRM_HIP_BLOCKED_GATE", None)
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        out["gate_rows_ms_y_by_round"] = gate
        out["gate_rows_ms_y"] = {g: float(np.median(v)) for g, v in gate.items()}
        api.destroy(e["h"])
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
        print(json.dumps({k: out[k] for k in ("gate_rows_ms_y_by_round", "gate_rows_ms_y")}))
        return
    for leg in legs:
        run(leg, args.warmup, False)
        api.kernel_stats(leg["h"], reset=True)
    for r in range(args.rounds):
        for leg in legs:                      # the legs take turns
            leg["rounds"].append(run(leg, args.iters, True))
        print(f"round {r}: " + ", ".join(f"{leg['name']} x {leg['rounds'][-1][0]:.1f} y {leg['rounds'][-1][1]:.1f} ms" for leg in legs), flush=True)
    total_iters = args.rounds * args.iters
    res = {}
    for leg in legs:
        st = api.kernel_stats(leg["h"])
        ms_x, ms_y = [r[0] for r in leg["rounds"]], [r[1] for r in leg["rounds"]]
        ms_it = [x + y for x, y in leg["rounds"]]
        res[leg["name"]] = dict(
            options=leg["opts"], environment=leg["env"], families=st["tiled"], waves_row=st["waves_row"], waves_col=st["waves_col"],
            ms_per_iteration_by_round=ms_it, ms_x_by_round=ms_x, ms_y_by_round=ms_y,
            ms_per_iteration=float(np.median(ms_it)), ms_x=float(np.median(ms_x)), ms_y=float(np.median(ms_y)),
            spread_iteration=max(ms_it) - min(ms_it), spread_y=max(ms_y) - min(ms_y),
            launches_x=st["launches_x"], launches_y=st["launches_y"],
            passes_x=1.0 + st["trials_x"] / (m * total_iters), passes_y=1.0 + st["trials_y"] / (n * total_iters),
            iterations=args.warmup + total_iters, final_objective=api.sum(leg["h"], leg["objcol"].data_ptr(), n))
    if args.bound:
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        out.setdefault("waves_per_simd", {})[args.bound] = dict(library=os.path.basename(os.environ.get("GLRM_HIP_LIB_PATH", "libglrm_hip.so")), **res["e_f32_blocked_cols"])
    else:
        out = dict(recipe="C4", m=m, n=n, k=k, obs_per_row=q, observations=m * q, iters_per_round=args.iters, rounds=args.rounds,
                   warmup=args.warmup, device=torch.cuda.get_device_name(), legs=res,
                   phase_gate_rows=os.environ.get("GLRM_HIP_BLOCKED_GATE") or "the engine's defaults: 5120 (fp64), 16384 (f32)")
        if os.path.exists(args.out):      # what --gates filed earlier stays
            prev = json.load(open(args.out))
            out.update({key: v for key, v in prev.items() if key.startswith("gate_rows")})
        spread = max(v["spread_iteration"] for v in res.values())
        spread_y = max(v["spread_y"] for v in res.values())
        a, c, e_, f = (res[s[0]] for s in LEGS)
        out["y_e_over_c"] = e_["ms_y"] / c["ms_y"]
        out["iteration_f_over_a"] = f["ms_per_iteration"] / a["ms_per_iteration"]
        out["iteration_f_over_c"] = f["ms_per_iteration"] / c["ms_per_iteration"]
        out["largest_round_to_round_difference_ms"] = dict(iteration=spread, y=spread_y)
    for leg in legs:
        api.destroy(leg["h"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
