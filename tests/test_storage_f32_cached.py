"""glrm_options.storage = 1 on the cached row sweep, the CPU side: the host reference the GPU test holds the float kernels to
(tests/storage_f32_cached_ref.py) is pinned to the CPU oracle before the GPU is involved.  The GPU part is
tests/test_gpu_storage_f32_cached.py."""
import numpy as np

import oracle as O
import storage_f32_cached_ref as SC
import storage_f32_ref as S
from test_storage_f32 import oracle_iterations
from test_sum_order import small_problem


def test_without_rounding_the_reference_is_the_oracle_in_the_cached_order():
    """The small rank-64 shape of the GPU test, two outer iterations (the step sizes carried over are part of what is compared).  The
    oracle adds in the order an fp64 handle on the family reports: strided, (G, R) = (8, 8), cached_waves = 2, cached_maxlen = 104."""
    lens = SC.LENS_K64
    pa, X0, Y0 = small_problem(2 * len(lens), 131, 64, lens, seed=64, reg=(S.REG_QUAD, 0, 0.1))
    order = O.make_sum_order("strided", 8, 8, cached_maxlen=104, cached_waves=2)
    want = oracle_iterations(pa, X0, Y0, order, 2)
    got = SC.trajectory(pa, X0, Y0, 8, 8, (S.REG_QUAD, 0, 0.1), 2, rounding=False)
    for (X1, Y2, tx, ty), (Xs, Ys, _, sx, sy, _) in zip(want, got):
        assert np.array_equal(Xs, X1) and np.array_equal(Ys, Y2)
        assert (sx, sy) == (tx, ty)
    # the wave count is what is being pinned: with one wave on the short rows the same simulation lands elsewhere
    one = S.trajectory(pa, X0, Y0, 8, 8, (S.REG_QUAD, 0, 0.1), 1, rounding=False)
    assert not np.array_equal(one[0][0], want[0][0])


def test_row_wave_counts():
    sim = SC.Simulation(*small_problem(2, 8, 64, [1], seed=1), 8, 8, (S.REG_ZERO, 0, 1.0))
    assert [sim.row_waves(n) for n in (0, 1, 104, 105, 1535, 1536, 98304)] == [2, 2, 2, 1, 1, 4, 8]
    sim4 = SC.Simulation(*small_problem(2, 8, 20, [1], seed=1), 4, 8, (S.REG_ZERO, 0, 1.0))
    assert [sim4.row_waves(n) for n in (208, 209)] == [2, 1] and SC.cached_maxlen(4) == 208 and SC.cached_maxlen(8) == 104
