"""glrm_hip_solve_x against loops of glrm_hip_step_x, on the C4 recipe's geometry cut to what a transform sees:
QuadLoss, rank 64, 100 000 columns (Y = 51 MB, beyond L2), about 100 observations per row, m = 1e6 new rows, NonNegConstraint on both
factors; T = 10 X half-steps against the fixed Y.

    python tests/perf/bench_transform.py [--rows 1000000] [--inner 10] [--rounds 3] [--out profiles/transform_solve_x.json]

One process, on bench_storage.py's method: six handles on the same device data --
    (a) T step_x calls on a gather handle (GLRM_HIP_CACHED=0 at create),
    (b) T step_x calls on a GLRM_HIP_CACHED=1 handle (the persistent register kernel),
    (c) solve_x(T) on a handle created without the variable (tiled = 1: its own step_x runs the gather sweep),
each in fp64 and with storage = 1 -- every leg is warmed up, then the legs take turns: `rounds` rounds, each from the same X0 and step
sizes, timed with device events around the T half-steps; medians over the rounds.  The legs' final X are compared ((b) and (c) must be
equal bit for bit: the contract of include/glrm_hip_transform.h).  These are measurements, not targets."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_solve_x.json"))
    args = ap.parse_args()
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    api = _capi.hip_api()
    m, n, k, q, T = args.rows, 100_000, 64, 100, args.inner
    w = synth.DeviceWorkload(m, n, k, q, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0))
    stream = torch.cuda.current_stream().cuda_stream
    spec = [("a_step_x_gather", "0", False), ("b_step_x_cached", "1", False), ("c_solve_x", None, True)]
    legs = []
    for storage in (0, 1):
        for name, env, solve in spec:
            os.environ.pop("GLRM_HIP_CACHED", None)
            if env is not None:
                os.environ["GLRM_HIP_CACHED"] = env                    # read at create
            h = api.create(w.problem(), stream=stream, profile=0, tiled=1, storage=storage)
            legs.append(dict(name=name + ("_f32" if storage else "_f64"), h=h, storage=storage, solve=solve, env=env))
    os.environ.pop("GLRM_HIP_CACHED", None)
    ld = api.factor_ld(legs[0]["h"])
    X0, Y0 = w.init_factors(ld)
    X0.abs_().mul_(1.0 / k ** 0.5)
    Y0.abs_().mul_(1.0 / k ** 0.5)
    w.free_sources()
    X0f = X0.float()
    for leg in legs:
        f32 = leg["storage"] == 1
        leg["dX"] = X0f.clone() if f32 else X0.clone()
        leg["dY"] = Y0.float() if f32 else Y0.clone()
        leg["objcol"] = torch.zeros(n, dtype=torch.float64, device=X0.device)
        leg["objrow"] = torch.zeros(m, dtype=torch.float64, device=X0.device)
        api.bind_buffers(leg["h"], leg["dX"].data_ptr(), leg["dY"].data_ptr(), leg["objcol"].data_ptr(), leg["objrow"].data_ptr())
        leg["ms"] = []

    def run(leg, timed):
        leg["dX"].copy_(X0f if leg["storage"] else X0)                 # every round from the same start
        api.reset_stepsizes(leg["h"], 1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if leg["solve"]:
            api.solve_x(leg["h"], T, 0.01)
        else:
            for _ in range(T):
                api.step_x(leg["h"], 0.01)
        b.record()
        torch.cuda.synchronize()
        if timed:
            leg["ms"].append(a.elapsed_time(b))

    for leg in legs:
        for _ in range(args.warmup):
            run(leg, False)
        api.kernel_stats(leg["h"], reset=True)
    for _ in range(args.rounds):
        for leg in legs:                                               # the legs take turns
            run(leg, True)
    out = dict(recipe="C4 geometry, X half-steps against a fixed Y", m=m, n=n, k=k, obs_per_row=q, observations=m * q, inner_iter=T,
               rounds=args.rounds, warmup=args.warmup, device=torch.cuda.get_device_name(), legs={})
    for leg in legs:
        st = api.kernel_stats(leg["h"])
        info = api.solve_x_info(leg["h"]) if leg["solve"] else None
        out["legs"][leg["name"]] = dict(
            GLRM_HIP_CACHED=leg["env"], storage=leg["storage"], families=st["tiled"], solve_x_info=info,
            ms_by_round=leg["ms"], ms=float(np.median(leg["ms"])), ms_per_half_step=float(np.median(leg["ms"])) / T,
            launches_x=st["launches_x"], trials_per_row_per_step=st["trials_x"] / (m * T * args.rounds),
            accepts_per_row_per_step=st["accepts_x"] / (m * T * args.rounds))
    by = {leg["name"]: leg for leg in legs}
    for s in ("_f64", "_f32"):
        g = out["legs"]
        out["ratio_c_over_a" + s] = g["c_solve_x" + s]["ms"] / g["a_step_x_gather" + s]["ms"]
        out["ratio_c_over_b" + s] = g["c_solve_x" + s]["ms"] / g["b_step_x_cached" + s]["ms"]
        out["X_equal_b_c" + s] = bool(torch.equal(by["b_step_x_cached" + s]["dX"], by["c_solve_x" + s]["dX"]))
    for leg in legs:
        api.destroy(leg["h"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
