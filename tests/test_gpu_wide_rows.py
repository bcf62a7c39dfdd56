"""GPU: rows of more than 64 actions -- the generic-width build of the selection, learn and rollout kernels (32 or 64
lanes per row, some of them beyond the row) and the one-wavefront-per-row kernels above 256 -- bit for bit against the
NumPy oracle on the cases of tests/wide_row_cases.py, and against the real reference's record of them
(tests/golden/wide_rows.npz) at ``GOLDEN_WIDTHS``.  Actions, tables (NaN included), episode history, final observations,
running returns and the exception type are compared; no tolerance anywhere.  tests/test_wide_row_cases.py asserts on the
oracle alone that these inputs tie, reach the last lane and the last sweep, share rows and raise where they are meant to.

One engine per (width, dtype); its cases run inside one test."""

import numpy as np
import pytest

import wide_row_cases as W
from helpers import GOLDEN
from test_gpu_nan_regime import _compare, _run_product_chunks
from test_gpu_parity import _product, _run_product_trace
from test_oracle_wide_rows_golden import golden_learn, golden_select

pytestmark = pytest.mark.gpu


def _engine(A, dt, gamma=0.9):
    from dist_classicrl_amd import _lib

    algo = _product()[0](W.S_ROWS, A, gamma, seed=7 + W.WIDTHS.index(A), dtype=np.dtype(dt))
    assert int(_lib.load().qe_table_row_stride(algo.handle)) == W.row_stride(A)
    if A <= 256:
        assert algo.lanes_per_row == W.lanes_per_row(A)
    return algo


@pytest.mark.parametrize("dt", W.DTYPES)
@pytest.mark.parametrize("A", W.WIDTHS)
def test_selection_matches_the_oracle(A, dt):
    """k_select with 32 / 64 lanes per row (A <= 256), k_select_large beyond."""
    from dist_classicrl_amd import _lib

    g = np.load(GOLDEN / "wide_rows.npz") if A in W.GOLDEN_WIDTHS else None
    algo = _engine(A, dt)
    algo.q_table = W.wide_table(A, dt)
    ran = 0
    for k, c in enumerate(W.select_cases(A)):
        if c["dt"] != dt:
            continue
        assert c["seed"] == algo.seed
        _q, states, masks = W.select_inputs(c)
        _lib.check(_lib.load().qe_set_agent_offset(algo.handle, c["offset"]))
        got = W.call_select(algo, c, states, masks, lambda step, _n: setattr(algo, "step_counter", step))
        want = W.run_select_oracle(A, k)
        assert got[0] == want[0], c  # IndexError exactly where the oracle raises it
        if want[0] == "ok":
            assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), c
            assert algo.step_counter == c["step"] + (c["n"] if c["entry"] == "single" else 1)
        ref = None if g is None else golden_select(g, A, k)
        if ref is not None:
            assert got[0] == ref[0] and (ref[1] is None or np.array_equal(got[1], ref[1])), c
        ran += 1
    assert ran >= 5


@pytest.mark.parametrize("dt", W.DTYPES)
@pytest.mark.parametrize("A", W.WIDTHS)
def test_learning_matches_the_oracle(A, dt):
    """qe_learn: the ordered path (slow_body) on both sides of its mode switch and k_vec_inc at 32 / 64 lanes per row,
    k_learn_large beyond 256 columns."""
    g = np.load(GOLDEN / "wide_rows.npz") if A in W.GOLDEN_WIDTHS else None
    algo = _engine(A, dt, W.LEARN_GAMMA)
    ran = 0
    for k, c in enumerate(W.learn_cases(A)):
        if c["dt"] != dt:
            continue
        q0, batch = W.learn_inputs(c)
        algo.q_table = q0
        W.call_learn(algo, c, batch)
        got = np.asarray(algo.q_table)
        assert got.dtype == q0.dtype
        assert np.array_equal(got, W.run_learn_oracle(A, k), equal_nan=True), c
        if g is not None:
            assert np.array_equal(got, golden_learn(g, A, k, q0), equal_nan=True), c
        ran += 1
    assert ran >= 4


# ------------------------------------------------------------------------------- closed loop
def _device_env(spec):
    _, _, envs, _ = _product()
    if spec[0] == "table":
        return envs.TabularMDPEnv(spec[1], W.table_mdp(*spec[2:]), seed=1)
    return None  # test_gpu_parity.make_device_env builds the hash environments


def _reached(path):
    """The path a rollout comes out on: forcing "turnstile" asks for the automatic choice, and every workgroup of every
    shape here is resident at once (2100 agents at 64 lanes per row are 525 workgroups), so that is the turnstile; the
    wide rounds run only where they are forced."""
    return {"stepwise": "stepwise", "wide": "wide", "wide_listed": "wide"}.get(path, "turnstile")


CLEAN = [name for name, case in W.ROLLOUTS.items() if not case[4]]
ROLLOUT_RUNS = [(name, path) for name in CLEAN for path in ("stepwise", "wide", "wide_listed", "turnstile", "turnstile_reread", "auto")
                if path != "turnstile_reread" or W.ROLLOUTS[name][2:4] == ("f4", "iter")]  # forwarding: float32 learn_iter only


@pytest.mark.parametrize(("name", "path"), ROLLOUT_RUNS)
def test_rollout_matches_the_oracle(name, path):
    from dist_classicrl_amd import _lib

    spec, chunks, dt, mode, _ = W.ROLLOUTS[name]
    want = W.run_rollout_oracle(name)[-1]
    got = _run_product_trace(spec, chunks[0], dt, "const", mode, path=path, q0=W.rollout_q0(name), env=_device_env(spec))
    for key in ("actions", "q", "history", "final_obs", "agent_rewards"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    stats = got["stats"]
    assert _lib.decode_variant(stats["kernel_variant"])["path"] == _reached(path)
    assert stats["involved"] > 0  # the ordered path ran
    assert len(want["history"]) > 0


NAN_RUNS = [(name, path) for name, case in W.ROLLOUTS.items() if case[4] for path in ("stepwise", "wide", "turnstile", "auto")]


@pytest.mark.parametrize(("name", "path"), NAN_RUNS)
def test_rollout_from_a_nan_table_matches_the_oracle(name, path):
    """Fewer than 100 unmasked agents: the list variants step over NaN; 150 of them: IndexError in the oracle's call."""
    spec, chunks, dt, mode, _ = W.ROLLOUTS[name]
    want = W.run_rollout_oracle(name)
    got = _run_product_chunks(spec, chunks, dt, "const", mode, path, q0=W.rollout_q0(name))
    _compare(got, want)


def test_the_persistent_kernel_refuses_rows_wider_than_64():
    Algo, Runtime, envs, sch = _product()
    algo = Algo(30, 65, 0.99, seed=0)
    algo.set_rollout_path("persistent")
    rt = Runtime(algo, sch.ConstantSchedule(0.1), sch.ConstantSchedule(0.1))
    with pytest.raises(NotImplementedError, match="persistent rollout needs num_agents <= 512 and action_size <= 64") as info:
        rt.run_steps(3, envs.HashTabularEnv(40, 30, 65, seed=1), None)
    assert "65 actions" in str(info.value)
    assert not np.asarray(algo.q_table).any()  # refused, not run
