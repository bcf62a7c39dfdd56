"""CPU: the delta-log records derived from the NumPy oracle (``helpers.run_oracle_delta_log``, used by the GPU tests
for the environments the C oracle does not have) equal the C oracle's own records bit for bit on the hash environment,
for both update semantics, on tables small enough that cells repeat inside a step."""

import numpy as np
import pytest

from helpers import make_oracle_env, run_oracle_delta_log, shares_a_cell_within_a_step
from oracle import c_oracle


@pytest.mark.parametrize(("n", "S", "A", "masked", "mode", "steps"), [
    (64, 20, 4, False, "iter", 40),
    (64, 20, 4, False, "vec", 40),
    (96, 30, 9, True, "iter", 25),
    (96, 30, 9, True, "vec", 25),
])
def test_numpy_oracle_records_equal_the_c_oracle(n, S, A, masked, mode, steps):
    got = run_oracle_delta_log(make_oracle_env(("hash", n, S, A, masked)), steps, "f4", "bench", mode)
    run = c_oracle.CHashRollout(n, S, A, masked=masked, dtype=np.float32, mode=mode)
    eps, _ = c_oracle.exp_schedule(1.0, 0.01, 0.995, n, steps)
    lr, _ = c_oracle.exp_schedule(0.1, 1e-5, 0.995, n, steps)
    want = run.run(eps, lr, trace=True, delta_log=True)
    assert shares_a_cell_within_a_step(want["cells"], n)
    assert np.array_equal(got["actions"], want["actions"])
    assert np.array_equal(got["cells"], want["cells"])
    assert np.array_equal(got["deltas"].view(np.uint32), want["deltas"].view(np.uint32))
    assert np.array_equal(got["q"], run.q)
