"""Host reference of a storage = f32 handle whose short rows run on the cached row sweep (csrc/glrm_cached.hpp; test infrastructure).

tests/storage_f32_ref.Simulation with the wave count of a ROW chosen as the engine chooses it: the cached sweep sums a row of at most
`cached_maxlen` observations on two waves (wave w holds the observations (t * 2 + w) * NG + group: lane_orders.strided_pass with
waves = 2, reg_pass + row_combine), a longer row goes to the gather sweep with the waves its own length asks for.  Columns are unchanged.
With `rounding=False` this is the order an fp64 handle on the family reports (cached_waves = 2), which tests/test_storage_f32_cached.py
holds against the CPU oracle bit for bit.
"""
import lane_orders as LO
import storage_f32_ref as S

CACHED_WAVES = 2


def cached_maxlen(G):
    """Longest row the register variant takes: 13 trips of the lane layout, 64 / G observations each (104 at G = 8, 208 at G = 4)."""
    return 13 * (64 // G)


class Simulation(S.Simulation):
    def __init__(self, pa, X0, Y0, G, R, reg, maxlen=None, **kw):
        super().__init__(pa, X0, Y0, G, R, reg, **kw)
        self.maxlen = cached_maxlen(G) if maxlen is None else maxlen

    def row_waves(self, n):
        return CACHED_WAVES if n <= self.maxlen else S.wave_count(n, self.waves)

    def _half_step(self, rows):
        if not rows:
            return super()._half_step(False)
        pa, k, G, R = self.pa, self.pa.k, self.G, self.R
        facl = [list(self.Y[:, i]) for i in range(self.Y.shape[1])]
        regfn, proxfn = S.reg_fns(self.reg, k, G, R, self.rounding)
        with S.fast_fma():
            for s in range(pa.m):
                b, e = int(pa.rowptr[s]), int(pa.rowptr[s + 1])
                ix, vv = [int(v) for v in pa.colidx[b:e]], [float(v) for v in pa.rowvals[b:e]]
                w = self.row_waves(e - b)
                passfn = lambda x, grad: LO.strided_pass(ix, vv, x, facl, k, G, R, w, self.scale, grad)  # noqa: E731
                xn, a, J, t = LO.half_step(passfn, regfn, proxfn, [float(v) for v in self.X[:, s]], float(self.alpha[0][s]), e - b,
                                           self.min_stepsize)
                self.X[:, s] = xn
                self.alpha[0][s] = a
                self.obj[0][s] = J
                self.trials[0] += t


def trajectory(pa, X0, Y0, G, R, reg, iters, **kw):
    """storage_f32_ref.trajectory on this simulation: (X after step_x, Y after step_y, objcol, trials_x, trials_y, objrow) per iteration."""
    sim = Simulation(pa, X0, Y0, G, R, reg, **kw)
    out = []
    for _ in range(iters):
        sim.step_x()
        X1 = sim.X.copy(order="F")
        sim.step_y()
        out.append((X1, sim.Y.copy(order="F"), sim.obj[1].copy(), sim.trials[0], sim.trials[1], sim.obj[0].copy()))
    return out


# ---- the problems of tests/test_gpu_storage_f32_cached.py (n = 131, QuadLoss scale 0.75; built by test_sum_order.small_problem) ----------

#: rank 64, QuadReg(0.1): every trip count of the MAXT = 7 kernel, rows beyond 104 bring the listed form, the 300 repeats columns
LENS_K64 = [0, 1, 7, 8, 9, 16, 17, 63, 64, 65, 100, 104, 105, 208, 300]
#: rank 64, NonNegConstraint: no cached row beyond 64 observations (the MAXT = 4 kernel), two long rows
LENS_K64_SHORT = [0, 1, 7, 8, 9, 16, 17, 63, 64] * 7 + [105, 300]
#: rank 20 (kp = 32, G = 4): trips of 32 observations, rows beyond 208 on the gather sweep
LENS_K20 = [0, 1, 15, 16, 17, 32, 33, 128, 129, 208, 209, 300]
