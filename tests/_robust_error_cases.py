"""Shapes and states for the robust film's noise estimate (rl_robust_unit_estimate), shared by tests/test_robust_error.py,
tests/test_robust_error_abi.py and tests/test_gpu_robust_error.py: _robust_cases' shapes, bucket counts, parameters, schedules and
edge_state, and two shapes of more than one tile.  Test-only."""
import numpy as np

import _robust_cases as RC

NO_LIMIT = RC.NO_LIMIT
BUCKETS = RC.BUCKETS
PARAMS = RC.PARAMS
SCHEDULES = RC.SCHEDULES
edge_state = RC.edge_state
schedule = RC.schedule
noisy = RC.noisy
# the estimate kernel's edges on top of the resolve's: 33 x 17 is 3 x 2 tiles, partial in both directions (one pixel wide and one
# pixel high at the far edges); 100 x 50 is 7 x 4 tiles
SHAPES = RC.SHAPES + [(33, 17), (100, 50)]
POISON_SHAPES = [(17, 5), (33, 17), (64, 36)]


def firefly_state(m, pixels=2000, seed=0):
    """poisson(20) * exponential(1) + 1 bucket means over `pixels` pixels (one row), bucket 0 times 1000 in every pixel; equal n."""
    rng = np.random.default_rng(seed)
    n = 64
    means = rng.poisson(20.0, size=(m, 1, pixels)) * rng.exponential(1.0, size=(m, 3, pixels)) + 1.0
    means[0] *= 1000.0
    return (means * n).reshape(m, 3, 1, pixels), [n] * m, m


def iid_state(m, draw, pixels=20000, seed=0):
    """`pixels` i.i.d. pixels (one row) whose M bucket means of Y are draw(rng, (m, pixels)); n[j] = 1, so a key is its sum."""
    rng = np.random.default_rng(seed)
    sums = np.zeros((m, 3, 1, pixels), np.float64)
    sums[:, 1, 0, :] = draw(rng, (m, pixels))
    return sums, [1] * m, m


DRAWS = {"normal": lambda rng, size: rng.normal(10.0, 1.0, size=size),
         "poisson_exponential": lambda rng, size: rng.poisson(3.0, size=size) * rng.exponential(1.0, size=size)}
# (M, c): gain infinity and max_trim = c fix the trim
CALIBRATION = [(15, 0), (15, 2), (15, 6), (32, 0), (32, 8), (32, 15)]
