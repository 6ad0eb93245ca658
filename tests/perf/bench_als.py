"""glrm_hip_als_solve measured on the C2 recipe (bench_legs.CONFIGS["C2"]: 1M x 10k, rank 32, QuadLoss, 500 observations per row,
QuadReg(1.0) on X and Y).  A side benchmark, not bench.py.

    python tests/perf/bench_als.py [--rows 1000000] [--rounds 5] [--warmup 2] [--new-rows 100000] [--out profiles/als_c2.json]

One process, one handle created with the default options (what production runs), device events around every timed call:
  (a) ms per als_solve(h, 0) and per als_solve(h, 1), and beside them step_x / step_y of the handle's own family, taking turns for
      `rounds` rounds after `warmup` untimed ones; medians.  Next to them the operation-count estimate: observations x k(k+1)/2 triangle
      entries x (mul + add) per half-step.
  (b) from one init_svd start: glrm_hip_fit with HipProxGradParams(max_iter=72) (72 as in the C2 parity fixture; the iterations it ran and
      its own clock are recorded), the FULL objective it ends at, and the ALS iteration (solve rows, solve columns, full objective) at which
      that objective is first reached, with the wall time to there.
  (c) the embedding of `new-rows` rows of the same generator against the Y of (b)'s ALS run: one als_solve(h, 0) against the default
      transform path (solve_x per outer iteration, objective, stopping rule) run to its stopping rule.  The generator is index-hashed, so
      these rows coincide with the first rows of the training problem; the cost does not depend on that.
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
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--new-rows", type=int, default=100_000)
    ap.add_argument("--als-max-iter", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_c2.json"))
    args = ap.parse_args()
    import torch
    from lowrankmodels.jl_amd import _capi, synth
    from lowrankmodels.jl_amd.fit import _should_stop
    from lowrankmodels.jl_amd.params import HipProxGradParams
    api = _capi.hip_api()
    m, n, k, q = args.rows, args.cols, 32, 500
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)

    class Model:
        """A handle of the recipe with `rows` rows and its bound buffers."""

        def __init__(self, rows):
            w = synth.DeviceWorkload(rows, n, k, q, value_model=0, rx=(1, 0, 1.0), ry=(1, 0, 1.0))
            self.m, self.nnz = rows, w.nnz_rows
            self.h = api.create(w.problem(), stream=stream)
            w.free_sources()
            self.ld = api.factor_ld(self.h)
            z = lambda c: torch.zeros(c, dtype=torch.float64, device=dev)
            self.dX, self.dY, self.oc, self.orow = z(self.ld * rows), z(self.ld * n), z(n), z(rows)
            sync()
            api.bind_buffers(self.h, self.dX.data_ptr(), self.dY.data_ptr(), self.oc.data_ptr(), self.orow.data_ptr())

        def full_objective(self):
            h = self.h
            api.col_losses(h)
            loss = api.sum(h, self.oc.data_ptr(), n)
            api.row_penalties(h)
            px = api.sum(h, self.orow.data_ptr(), self.m)
            api.col_penalties(h)
            return loss + (px + api.sum(h, self.oc.data_ptr(), n))

        def fit_objective(self):
            """What fit! records after an iteration: column losses + column penalties."""
            h = self.h
            api.col_losses(h)
            loss = api.sum(h, self.oc.data_ptr(), n)
            api.col_penalties(h)
            return loss + api.sum(h, self.oc.data_ptr(), n)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        sync()
        return a.elapsed_time(b)

    M = Model(m)
    h = M.h
    X0, Y0 = np.zeros((k, m), order="F"), np.zeros((k, n), order="F")
    t0 = time.perf_counter()
    api.init_svd(h, X0, Y0)
    init_s = time.perf_counter() - t0
    out = dict(recipe="C2", m=m, n=n, k=k, obs_per_row=q, observations=M.nnz, device=torch.cuda.get_device_name(), rounds=args.rounds,
               warmup=args.warmup, families=api.kernel_stats(h)["tiled"], init_svd_s=init_s)
    ops = M.nnz * (k * (k + 1) // 2) * 2
    out["estimate"] = dict(fp64_operations_per_half_step=ops, note="observations x k(k+1)/2 triangle entries x (mul + add); the right-hand side, "
                           "u = w v and the factorisations come on top")

    # ---- (a) a half-step of each kind, taking turns
    api.set_factors(h, X0, Y0)
    api.reset_stepsizes(h, 1.0)
    legs = dict(als_solve_rows=lambda: api.als_solve(h, 0), als_solve_cols=lambda: api.als_solve(h, 1),
                step_x=lambda: api.step_x(h, 0.01), step_y=lambda: api.step_y(h, 0.01))
    ms = {name: [] for name in legs}
    for name, fn in legs.items():
        for _ in range(args.warmup):
            timed(fn)
    for _ in range(args.rounds):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    out["half_steps"] = {name: dict(ms=float(np.median(v)), ms_by_round=v) for name, v in ms.items()}
    for name in ("als_solve_rows", "als_solve_cols"):
        out["half_steps"][name]["fp64_tflops_of_the_estimate"] = ops / (out["half_steps"][name]["ms"] * 1e-3) / 1e12
    out["als_info"] = {0: api.als_info(h, 0), 1: api.als_info(h, 1)}

    # ---- (b) time to the objective of 72 prox-gradient iterations, from the same start
    Xp, Yp = X0.copy(order="F"), Y0.copy(order="F")
    p = HipProxGradParams(max_iter=72)
    t0 = time.perf_counter()
    obj_pg, sec_pg = api.fit(h, p, Xp, Yp)
    wall_pg = time.perf_counter() - t0
    api.bind_buffers(h, M.dX.data_ptr(), M.dY.data_ptr(), M.oc.data_ptr(), M.orow.data_ptr())
    api.set_factors(h, Xp, Yp)
    target = M.full_objective()
    out["proxgrad"] = dict(max_iter=72, iterations=len(obj_pg) - 1, seconds_by_its_own_clock=float(sec_pg[-1]), wall_s_with_transfers=wall_pg,
                           objective_start=float(obj_pg[0]), recorded_last=float(obj_pg[-1]), full_objective_end=target)
    api.set_factors(h, X0, Y0)
    sync()
    hist, t_solve, t_all, reached = [M.full_objective()], [0.0], [0.0], None
    for i in range(1, args.als_max_iter + 1):
        t0 = time.perf_counter()
        api.als_solve(h, 0)
        api.als_solve(h, 1)
        api.synchronize(h)
        t1 = time.perf_counter()
        hist.append(M.full_objective())
        t2 = time.perf_counter()
        t_solve.append(t_solve[-1] + (t1 - t0))
        t_all.append(t_all[-1] + (t2 - t0))
        if reached is None and hist[-1] <= target:
            reached = i
            break
    out["als"] = dict(objective=hist, seconds_solves_only=t_solve, seconds_with_objective=t_all, reached_proxgrad_objective_at_iteration=reached,
                      seconds_to_there=None if reached is None else t_all[reached], als_info={0: api.als_info(h, 0), 1: api.als_info(h, 1)})
    Yfit = np.zeros((k, n), order="F")
    api.get_factors(h, X0, Yfit)
    api.destroy(h)
    del M
    torch.cuda.empty_cache()

    # ---- (c) embedding new rows against the fitted Y
    mt = args.new_rows
    T = Model(mt)
    Xs = np.asfortranarray(np.random.default_rng(1).standard_normal((k, mt)))
    tp = HipProxGradParams()
    res = {}
    for name in ("warmup", "exact", "default"):
        api.set_factors(T.h, Xs, Yfit)
        api.reset_stepsizes(T.h, tp.stepsize)
        sync()
        t0 = time.perf_counter()
        start = T.full_objective()
        if name != "default":
            api.als_solve(T.h, 0)
            objs = [start, T.full_objective()]
        else:
            objs = [start]
            for i in range(1, tp.max_iter + 1):
                api.solve_x(T.h, tp.inner_iter_X, tp.min_stepsize)
                objs.append(T.fit_objective())
                if _should_stop(i, objs[-2], objs[-1], tp.abs_tol * T.nnz, tp.rel_tol):
                    break
        api.synchronize(T.h)
        res[name] = dict(wall_s=time.perf_counter() - t0, iterations=len(objs) - 1, objective_start=objs[0], objective_end_as_recorded=objs[-1],
                         full_objective_end=T.full_objective())
        if name == "exact":
            res[name]["als_info"] = api.als_info(T.h, 0)
    res.pop("warmup")
    out["transform"] = dict(new_rows=mt, observations=T.nnz, **res)
    api.destroy(T.h)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
