"""glrm_hip_cd_solve measured on the C4 recipe (bench_legs.CONFIGS["C4"]: 10M x 100k, rank 64, QuadLoss, 100 observations per row,
NonNegConstraint on X and Y -- the NNMF of the north star).  A side benchmark, not bench.py.

    python tests/perf/bench_cd.py [--rows 10000000] [--rounds 3] [--warmup 1] [--sweeps 1 4 16] [--race-sweeps 4] [--out profiles/cd_c4.json]

One process, one handle created with the default options (what production runs), the start of bench.py (|N(0,1)| / sqrt(k)), device
events around every timed call:
  (a) ms per cd_solve(h, 0, s) and per cd_solve(h, 1, s) for every s of --sweeps, and beside them step_x / step_y of the handle's own
      family.  Every leg is warmed up `warmup` times, then the legs take turns for `rounds` rounds; medians.  The factors are put back to the
      start before every timed solve, so every round does the same work (a solve from its own result would leave early).  Next to them the
      operation-count estimate of the Gram stage: observations x k(k+1)/2 triangle entries x (mul + add), and of a sweep: segments x k^2 x
      (mul + add).
  (b) from that start: the prox-gradient loop of bench.py's convergence run (step_x, step_y, objective; ProxGradParams defaults, stop rule
      of src/algorithms/proxgrad.jl:210-213) on its own wall clock, the FULL objective it ends at, and for every s of --race-sweeps the
      CdParams iteration (solve rows, solve columns, full objective) at which that objective is first reached, with the wall time to
      there -- or that it is not reached in --cd-max-iter iterations.
These are measurements, not targets."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sweeps", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--race-sweeps", type=int, nargs="*", default=[4])
    ap.add_argument("--cd-max-iter", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cd_c4.json"))
    args = ap.parse_args()
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    from lowrankmodels.jl_amd.fit import _should_stop
    from lowrankmodels.jl_amd.params import ProxGradParams
    api = _capi.hip_api()
    m, n, k, q = args.rows, args.cols, 64, 100
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)

    t0 = time.perf_counter()
    w = synth.DeviceWorkload(m, n, k, q, value_model=1, rx=(3, 0, 1.0), ry=(3, 0, 1.0), device=dev)
    nnz = w.nnz_rows
    h = api.create(w.problem(), stream=stream)
    w.free_sources()
    ld = api.factor_ld(h)
    z = lambda c: torch.zeros(c, dtype=torch.float64, device=dev)
    dX, dY, oc, orow = z(ld * m), z(ld * n), z(n), z(m)
    X0, Y0 = w.init_factors(ld)
    X0.abs_().mul_(1.0 / k ** 0.5); Y0.abs_().mul_(1.0 / k ** 0.5)      # bench.py's NNMF start
    sync()
    api.bind_buffers(h, dX.data_ptr(), dY.data_ptr(), oc.data_ptr(), orow.data_ptr())
    setup_s = time.perf_counter() - t0

    def load_start():
        dX.copy_(X0); dY.copy_(Y0)
        sync()
        api.reset_stepsizes(h, 1.0)

    def full_objective():
        api.col_losses(h)
        loss = api.sum(h, oc.data_ptr(), n)
        api.row_penalties(h)
        px = api.sum(h, orow.data_ptr(), m)
        api.col_penalties(h)
        return loss + (px + api.sum(h, oc.data_ptr(), n))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        sync()
        return a.elapsed_time(b)

    out = dict(recipe="C4", m=m, n=n, k=k, obs_per_row=q, observations=nnz, regularizer="NonNegConstraint", device=torch.cuda.get_device_name(),
               library=os.path.basename(_capi.HIP_LIB_PATH), rounds=args.rounds, warmup=args.warmup, families=api.kernel_stats(h)["tiled"],
               setup_s=setup_s, start="X0, Y0 = |N(0,1)| / sqrt(k)")
    gram_ops = nnz * (k * (k + 1) // 2) * 2
    out["estimate"] = dict(gram_fp64_operations_per_half_step=gram_ops, sweep_fp64_operations_rows=m * k * k * 2, sweep_fp64_operations_cols=n * k * k * 2,
                           note="Gram: observations x k(k+1)/2 triangle entries x (mul + add); a sweep: segments x k^2 x (mul + add); the "
                                "right-hand side, u = w v and the divisions come on top")

    # ---- (a) a half-step of each kind from the same start, taking turns
    legs = {}
    for s in args.sweeps:
        legs[f"cd_solve_rows_sweeps_{s}"] = lambda s=s: api.cd_solve(h, 0, s)
        legs[f"cd_solve_cols_sweeps_{s}"] = lambda s=s: api.cd_solve(h, 1, s)
    legs["step_x"] = lambda: api.step_x(h, 0.01)
    legs["step_y"] = lambda: api.step_y(h, 0.01)
    ms = {name: [] for name in legs}
    for name, fn in legs.items():
        for _ in range(args.warmup):
            load_start()
            timed(fn)
    info = {}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            load_start()
            ms[name].append(timed(fn))
            if name.startswith("cd_solve"):
                info[name] = api.cd_info(h, 0 if "rows" in name else 1)
    out["half_steps"] = {name: dict(ms=float(np.median(v)), ms_by_round=v, **({"cd_info": info[name]} if name in info else {})) for name, v in ms.items()}
    for name, v in out["half_steps"].items():
        if name.startswith("cd_solve"):
            v["gram_fp64_tflops_of_the_estimate"] = gram_ops / (v["ms"] * 1e-3) / 1e12

    # ---- (b) time to the objective the prox-gradient fit stops at, from the same start
    if args.race_sweeps:
        p = ProxGradParams()
        load_start()
        t0 = time.perf_counter()
        hist = [full_objective()]
        for i in range(1, p.max_iter + 1):
            api.step_x(h, p.min_stepsize)
            api.step_y(h, p.min_stepsize)
            hist.append(full_objective())
            if _should_stop(i, hist[-2], hist[-1], p.abs_tol * nnz, p.rel_tol):
                break
        wall_pg = time.perf_counter() - t0
        target = hist[-1]
        out["proxgrad"] = dict(iterations=len(hist) - 1, wall_s=wall_pg, objective_start=hist[0], full_objective_end=target, objective=hist,
                               stop_rule="ProxGradParams defaults: abs_tol = 1e-5 |Omega|, rel_tol = 1e-4, max_iter = 100; the full objective is evaluated after every "
                                         "iteration in both loops")
        out["cd"] = {}
        for s in args.race_sweeps:
            load_start()
            hist, t_solve, t_all, reached = [full_objective()], [0.0], [0.0], None
            for i in range(1, args.cd_max_iter + 1):
                t0 = time.perf_counter()
                api.cd_solve(h, 0, s)
                api.cd_solve(h, 1, s)
                api.synchronize(h)
                t1 = time.perf_counter()
                hist.append(full_objective())
                t2 = time.perf_counter()
                t_solve.append(t_solve[-1] + (t1 - t0))
                t_all.append(t_all[-1] + (t2 - t0))
                if hist[-1] <= target:
                    reached = i
                    break
            out["cd"][f"sweeps_{s}"] = dict(objective=hist, seconds_solves_only=t_solve, seconds_with_objective=t_all, max_iter=args.cd_max_iter,
                                            reached_proxgrad_objective_at_iteration=reached, seconds_to_there=None if reached is None else t_all[reached],
                                            cd_info={0: api.cd_info(h, 0), 1: api.cd_info(h, 1)})
    api.destroy(h)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
