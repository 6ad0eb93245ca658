"""Host reference of the storage = f32 gather sweeps (include/glrm_hip_storage.h; test infrastructure).

The half-step of every segment through tests/lane_orders.py -- `strided_pass` adds in the order of sweep_pass / block_combine,
`half_step` is the line search -- with the one thing the f32 kernels add: after the regularizer's prox every component of the trial point
goes through numpy.float32 (C's (float) conversion, round to nearest even), before the trial pass and before the regularizer is evaluated.
Step sizes are kept per segment across iterations, as the engine keeps alpharow / alphacol.  With `rounding=False` this is the fp64 gather
sweep, which tests/test_storage_f32.py holds against the CPU oracle in the strided order bit for bit.

lane_orders.fma is exact rational arithmetic, ~5 us a call; a k = 100 case needs millions.  `fast_fma` swaps it for the C library's fma
(IEEE: the exact product and sum, rounded once -- the same function on finite operands) while a simulation runs.
"""
import contextlib
import ctypes
import ctypes.util

import numpy as np

import lane_orders as LO

REG_ZERO, REG_QUAD, REG_NONNEG = 0, 1, 3   # include/glrm_hip.h: GLRM_REG_*

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
libm_fma = _libm.fma


@contextlib.contextmanager
def fast_fma():
    keep = LO.fma
    LO.fma = libm_fma
    try:
        yield
    finally:
        LO.fma = keep


def round_f32(x):
    return [float(np.float32(v)) for v in x]


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def reg_fns(reg, k, G, R, rounding):
    """(regfn, proxfn) of the descriptor (kind, wrap, scale): QuadReg, ZeroReg, NonNegConstraint."""
    kind, _, scale = reg
    if kind == REG_QUAD:
        regfn = lambda x: LO.reg_quad(scale, x, k, G, R)  # noqa: E731
        prox = lambda x, a: [1 / (1 + 2 * a * scale) * v for v in x]  # noqa: E731
    elif kind == REG_NONNEG:
        regfn = lambda x: float("inf") if any(v < 0 for v in x) else 0.0  # noqa: E731
        prox = lambda x, a: [v if v > 0 else 0.0 for v in x]  # noqa: E731
    elif kind == REG_ZERO:
        regfn = lambda x: 0.0  # noqa: E731
        prox = lambda x, a: list(x)  # noqa: E731
    else:
        raise ValueError(f"regularizer kind {kind} is not modelled")
    proxfn = (lambda x, a: round_f32(prox(x, a))) if rounding else prox
    return regfn, proxfn


def wave_count(n, forced):
    return forced or (1 if n < 1536 else (4 if n < 98304 else 8))


class Simulation:
    """The factors, per-segment step sizes and counters of one model on the gather sweeps; step_x / step_y are the engine's half-steps."""

    def __init__(self, pa, X0, Y0, G, R, reg, waves=0, loss_scale=0.75, alpha0=1.0, min_stepsize=0.01, rounding=True):
        self.pa, self.G, self.R, self.reg, self.waves, self.scale = pa, G, R, tuple(reg), waves, loss_scale
        self.min_stepsize, self.rounding = min_stepsize, rounding
        self.X, self.Y = np.array(X0, order="F", dtype=np.float64), np.array(Y0, order="F", dtype=np.float64)
        self.alpha = [np.full(pa.m, float(alpha0)), np.full(pa.n, float(alpha0))]
        self.obj = [np.zeros(pa.m), np.zeros(pa.n)]      # per-segment objective of the last half-step (objrow is not kept by the engine)
        self.trials = [0, 0]

    def _half_step(self, rows):
        pa, k, G, R = self.pa, self.pa.k, self.G, self.R
        ptr, idx, vals = (pa.rowptr, pa.colidx, pa.rowvals) if rows else (pa.colptr, pa.rowidx, pa.colvals)
        own, fac = (self.X, self.Y) if rows else (self.Y, self.X)
        facl = [list(fac[:, i]) for i in range(fac.shape[1])]
        regfn, proxfn = reg_fns(self.reg, k, G, R, self.rounding)
        side = 0 if rows else 1
        with fast_fma():
            for s in range(len(ptr) - 1):
                b, e = int(ptr[s]), int(ptr[s + 1])
                ix, vv = [int(v) for v in idx[b:e]], [float(v) for v in vals[b:e]]
                w = wave_count(e - b, self.waves)
                passfn = lambda x, grad: LO.strided_pass(ix, vv, x, facl, k, G, R, w, self.scale, grad)  # noqa: E731
                xn, a, J, t = LO.half_step(passfn, regfn, proxfn, [float(v) for v in own[:, s]], float(self.alpha[side][s]), e - b,
                                           self.min_stepsize)
                own[:, s] = xn
                self.alpha[side][s] = a
                self.obj[side][s] = J
                self.trials[side] += t

    def step_x(self):
        self._half_step(True)

    def step_y(self):
        self._half_step(False)


def trajectory(pa, X0, Y0, G, R, reg, iters, **kw):
    """`iters` outer iterations (step_x, step_y): a list of (X after step_x, Y after step_y, objcol, trials_x, trials_y, objrow) per iteration,
    trial counts cumulative."""
    sim = Simulation(pa, X0, Y0, G, R, reg, **kw)
    out = []
    for _ in range(iters):
        sim.step_x()
        X1 = sim.X.copy(order="F")
        sim.step_y()
        out.append((X1, sim.Y.copy(order="F"), sim.obj[1].copy(), sim.trials[0], sim.trials[1], sim.obj[0].copy()))
    return out
