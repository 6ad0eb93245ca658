"""Host reference of the storage = f32 phase-aligned gather passes (csrc/glrm_blocked_f32.hip; test infrastructure).

tests/storage_f32_ref.Simulation with the pass of every segment swapped for `lane_orders.windowed_pass(..., L2=True)` -- the lane-by-lane
walk of tiled_pass<..., L2 = true> over one super-tile after the other, partial sums added in super-tile order -- at the engine's geometry:
TILE = glrm_tile_rows(kp) rows, `tiles_per_sup` tiles per super-tile, the whole batch of G observations per step (`four`) for every model
but the uniform QuadLoss one at G = 4 or 8.  The rounding after the prox is storage_f32_ref's.  Columns of at least `long_from`
observations leave the passes for the 8-wave gather sweep (`strided_pass`), as the engine diverts them.  With `rounding=False` this is the
fp64 family, which tests/test_storage_f32_blocked.py holds against the CPU oracle in the windowed order bit for bit.
"""
import lane_orders as LO
import shapes
import storage_f32_ref as S

KIND_QUAD, KIND_L1, KIND_HUBER, KIND_WHINGE = 0, 1, 2, 8   # include/glrm_hip.h: GLRM_LOSS_*


def tile_rows(kp):
    return shapes.tile_rows(kp)


def tiles_per_sup(kp, forced=0):
    """glrm_setup_blocked: ~128 MB of the opposing factor per super-tile, counted in 8-byte elements in both storages; GLRM_HIP_BLOCKED_TPS
    (`forced`) overrides."""
    if forced:
        return int(forced)
    return max(1, (128 * 1024 * 1024) // (tile_rows(kp) * kp * 8))


def _sign(d):
    return 1.0 if d > 0 else (-1.0 if d < 0 else d)


def loss_fn(desc):
    """(u, a) -> (L, dL) of one descriptor (kind, dim, scale, p0, p1), operation for operation as loss_both (csrc/glrm_device.hpp) writes
    the kinds without a transcendental: QuadLoss, L1Loss, HuberLoss, (Weighted)HingeLoss."""
    kind, s, p0 = int(desc[0]), float(desc[2]), float(desc[3])
    if kind == KIND_QUAD:
        return lambda u, a: LO.quad_loss(s, u, a)
    if kind == KIND_L1:
        def l1(u, a):
            d = u - a
            return s * abs(d), _sign(d) * s
        return l1
    if kind == KIND_HUBER:
        def huber(u, a):
            c, d = p0, u - a
            ad = abs(d)
            return ((ad - c + c * c) * s, _sign(d) * s) if ad > c else ((d * d) * s, d * s)
        return huber
    if kind == KIND_WHINGE:
        def whinge(u, a):
            r, aa = p0, 2 * a - 1
            loss = s * max(1 - aa * u, 0.0)
            g = 0.0 if aa * u >= 1 else -aa * s
            if r != 1.0 and a == 1.0:
                loss *= r
                g *= r
            return loss, g
        return whinge
    raise ValueError(f"loss kind {kind} is not modelled")


class Simulation(S.Simulation):
    """step_x / step_y of a handle whose two views run the phase-aligned passes.  tps: (row view, column view) tiles per super-tile.
    losses: None (one QuadLoss of scale `loss_scale`, the two-observation step) or the model's descriptor array -- one descriptor for
    the whole model or one per column -- which run the whole-batch step where G is 4 or 8."""

    def __init__(self, pa, X0, Y0, G, R, reg, tps, long_from=0, losses=None, **kw):
        super().__init__(pa, X0, Y0, G, R, reg, **kw)
        self.tile, self.tps, self.long_from = tile_rows(G * R), tuple(tps), int(long_from)
        self.lossfns = None if losses is None else [loss_fn(d) for d in losses]
        self.four = losses is not None and G in (4, 8)

    def _lossfn(self, rows, s):
        if self.lossfns is None:
            return None
        if len(self.lossfns) == 1:
            f = self.lossfns[0]
            return lambda c, u, a: f(u, a)
        if rows:   # a descriptor per observation: the column's
            return lambda c, u, a: self.lossfns[c](u, a)
        f = self.lossfns[s]
        return lambda c, u, a: f(u, a)

    def _half_step(self, rows):
        pa, k, G, R = self.pa, self.pa.k, self.G, self.R
        ptr, idx, vals = (pa.rowptr, pa.colidx, pa.rowvals) if rows else (pa.colptr, pa.rowidx, pa.colvals)
        own, fac = (self.X, self.Y) if rows else (self.Y, self.X)
        n_other = fac.shape[1]
        facl = [list(fac[:, i]) for i in range(n_other)]
        regfn, proxfn = S.reg_fns(self.reg, k, G, R, self.rounding)
        side = 0 if rows else 1
        tps = self.tps[side]
        with S.fast_fma():
            for s in range(len(ptr) - 1):
                b, e = int(ptr[s]), int(ptr[s + 1])
                ix, vv = [int(v) for v in idx[b:e]], [float(v) for v in vals[b:e]]
                if not rows and self.long_from > 0 and e - b >= self.long_from:
                    assert self.lossfns is None, "the diverted columns are modelled for the uniform QuadLoss model"
                    passfn = lambda x, grad: LO.strided_pass(ix, vv, x, facl, k, G, R, 8, self.scale, grad)  # noqa: E731
                else:
                    lf = self._lossfn(rows, s)
                    passfn = lambda x, grad: LO.windowed_pass(ix, vv, x, facl, k, G, R, self.tile, tps, n_other, self.scale, grad,  # noqa: E731
                                                              four=self.four, L2=True, lossfn=lf)
                xn, a, J, t = LO.half_step(passfn, regfn, proxfn, [float(v) for v in own[:, s]], float(self.alpha[side][s]), e - b,
                                           self.min_stepsize)
                own[:, s] = xn
                self.alpha[side][s] = a
                self.obj[side][s] = J
                self.trials[side] += t


def nine_kinds_problem(seed, per_row=6, k=8):
    """tests/test_gpu_storage_f32.py's mixed_problem, enlarged: the nine scalar loss kinds by column (a descriptor per column), values each
    kind accepts, A, X0 and Y0 float-representable, QuadReg(0.2) on both sides, and T + 8 rows and columns (T = the rank-8 tile), so that
    the opposing dimension of each view spans two one-tile super-tiles.  `per_row` sorted observations per row; row 3 and column 4 empty.
    Returns (pa, X0, Y0, loss objects by column)."""
    import numpy as np

    import lowrankmodels.jl_amd as L
    from lowrankmodels.jl_amd import _capi
    rng = np.random.default_rng(seed)
    m = n = tile_rows(8) + 8
    kinds = [L.QuadLoss(0.8), L.L1Loss(0.6), L.HuberLoss(1.1, crossover=0.7), L.QuantileLoss(0.9, quantile=0.3), L.PeriodicLoss(2.5, 0.8),
             L.PoissonLoss(20), L.OrdinalHingeLoss(1, 5, 0.9), L.LogisticLoss(0.7), L.WeightedHingeLoss(1.2, case_weight_ratio=2.0)]
    objs = [kinds[f % 9] for f in range(n)]
    free = np.array([f for f in range(n) if f != 4])
    rows = [np.sort(rng.choice(free, per_row, replace=False)) if e != 3 else free[:0] for e in range(m)]
    I = np.repeat(np.arange(m), [len(r) for r in rows])
    J = np.concatenate(rows)
    z = rng.standard_normal(len(I)).astype(np.float32).astype(np.float64)
    vals = z.copy()
    kind = J % 9
    vals[kind == 5] = rng.integers(0, 6, int((kind == 5).sum()))
    vals[kind == 6] = rng.integers(1, 6, int((kind == 6).sum()))
    vals[kind >= 7] = rng.random(int((kind >= 7).sum())) < 0.5
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    order = np.lexsort((I, J))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(J, minlength=n))]).astype(np.int64)
    losses = np.array([lo.descriptor() for lo in objs], dtype=_capi.LOSS_DTYPE)
    r = np.array([(S.REG_QUAD, 0, 0.2)], dtype=_capi.REG_DTYPE)
    pa = _capi.ProblemArrays(m, n, k, rowptr, J.astype(np.int32), vals, colptr, I[order].astype(np.int32), vals[order], losses, r, r)
    f32 = lambda a: np.asfortranarray(a.astype(np.float32).astype(np.float64))  # noqa: E731
    return pa, f32(0.3 * rng.standard_normal((k, m))), f32(0.3 * rng.standard_normal((k, n))), objs


def least_decision_margin(pa, X0, Y0, objs, stepsize=1.0, min_stepsize=0.01, reg_scale=0.2):
    """One step_x and one step_y from (X0, Y0), in plain fp64 numpy: the least |J_trial - J_old| / max(|J_old|, 1e-300) over every evaluated
    trial of every segment.  Which order the sums are formed in moves J by ~1e-15 relative; a margin of 1e-4 leaves no accept / reject
    decision within reach of it or of the rounding of a trial point to float (~6e-8 per component)."""
    import numpy as np
    least = float("inf")
    for rows in (True, False):
        ptr, idx, vals = (pa.rowptr, pa.colidx, pa.rowvals) if rows else (pa.colptr, pa.rowidx, pa.colvals)
        own, fac = (X0, Y0) if rows else (Y0, X0)
        for s in range(len(ptr) - 1):
            b, e = int(ptr[s]), int(ptr[s + 1])
            ix, av = idx[b:e], vals[b:e]
            los = [objs[c] for c in ix] if rows else [objs[s]] * (e - b)
            Yv = fac[:, ix]

            def J_of(x):
                u = x @ Yv
                return sum(lo.evaluate(float(ui), float(ai)) for lo, ui, ai in zip(los, u, av)) + reg_scale * float(x @ x)
            x = own[:, s]
            u = x @ Yv
            g = Yv @ np.array([lo.grad(float(ui), float(ai)) for lo, ui, ai in zip(los, u, av)]) if e > b else np.zeros_like(x)
            Jold, alpha, l = J_of(x), stepsize, (e - b) + 1.0
            while alpha > min_stepsize:
                st = alpha / l
                Jn = J_of((x - st * g) / (1 + 2 * st * reg_scale))
                least = min(least, abs(Jn - Jold) / max(abs(Jold), 1e-300))
                if Jn < Jold:
                    break
                alpha *= 0.7
    return least


def trajectory(pa, X0, Y0, G, R, reg, iters, tps, **kw):
    """storage_f32_ref.trajectory on the phase-aligned passes: (X after step_x, Y after step_y, objcol, trials_x, trials_y, objrow) per
    outer iteration, trial counts cumulative."""
    sim = Simulation(pa, X0, Y0, G, R, reg, tps, **kw)
    out = []
    for _ in range(iters):
        sim.step_x()
        X1 = sim.X.copy(order="F")
        sim.step_y()
        out.append((X1, sim.Y.copy(order="F"), sim.obj[1].copy(), sim.trials[0], sim.trials[1], sim.obj[0].copy()))
    return out
