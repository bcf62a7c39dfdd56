"""CPU: the NumPy model of the population's double estimator (tests/double_q_model.py), which the GPU parity tests of
``QLearningPopulation(double_q=True)`` compare against.

* In every step at most one cell of the two tables changes, and it lies in the table the coin names.
* The coin is ``x3 >> 31`` of the policy Philox block of that step: the block whose ``x0, x1, x2`` the oracle's draw
  protocol hands to the selection.
* ``a*`` follows ``np.argmax`` over the valid columns, ties and NaN included; a step worked out by hand.
* Two calls of K steps equal one call of 2K steps.
* With ``lr == 0`` both tables stay zero and the run acts exactly like the oracle-pinned Q-learning model with
  ``lr == 0`` (the same draws on all-tie rows); greedy evaluation with B == 0 is that of the single table A.
"""
import copy

import numpy as np
import pytest

from double_q_model import DoubleRun, bootstrap, coin
from oracle import envs as oenvs
from oracle.draws import STREAM_POLICY, philox4x32, policy_draws
from oracle.qlearn_oracle import OracleSchedule
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import TdRun


def _env(kind, offset):
    if kind == "hash":
        return oenvs.HashTabularEnv(1, 60, 8, seed=3, agent_offset=offset)
    if kind == "hash_masked":  # 16 masked actions: the NumPy selection variants
        return oenvs.HashTabularEnv(1, 60, 16, seed=3, masked=True, agent_offset=offset)
    if kind == "grid":
        return oenvs.GridLakeEnv(1, side=4, seed=2)
    if kind == "bandit":
        return oenvs.RiggedBanditVecEnv(1, episode_len=7)
    if kind == "tictactoe":
        return oenvs.TicTacToeVecEnv(1, seed=5, agent_offset=offset)
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    arrays, isd, masks = random_mdp(12, 5, 3, seed=4, masked=True)
    return TableMDPVecEnv(1, encode_table_mdp(*arrays, isd, masks), seed=3, agent_offset=offset)


KINDS = ["hash", "hash_masked", "grid", "bandit", "tictactoe", "table"]


def _schedules():
    return OracleSchedule("exponential", 0.9, 0.05, 0.99), OracleSchedule("linear", 0.4, None, -1e-3)


def _run(kind, dt, mode, offset=5, seed=9, **kw):
    eps, lr = _schedules()
    return DoubleRun(_env(kind, offset), 0.93, eps, lr, seed=seed, dtype=dt, mode=mode, agent_id=offset, **kw)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_a_step_changes_at_most_one_cell_in_the_table_the_coin_names(kind, dt, mode):
    offset, seed, K = 5, 9, 200
    run = _run(kind, dt, mode, offset, seed)
    run.reset()
    changed = [0, 0]
    for k in range(K):
        before = (run.qa.copy(), run.qb.copy())
        run.run(1)
        diff = [np.argwhere(before[i].view(np.uint8) != (run.qa, run.qb)[i].view(np.uint8)) for i in (0, 1)]
        cells = [{tuple(d[:2] // [1, np.dtype(dt).itemsize]) for d in diff[i]} for i in (0, 1)]
        # the coin, straight from the generator: word 3 of the block whose words 0..2 are the step's policy draws
        x = philox4x32(offset, k, 0, STREAM_POLICY, seed, seed >> 32)
        assert [int(w) for w in x[:3]] == [int(w[0]) for w in policy_draws(seed, np.array([offset], dtype=np.uint32), k)]
        c = int(x[3]) >> 31
        assert run.rt.coins[k] == (k, c) and coin(seed, offset, k) == c
        assert not cells[1 - c], (k, c, cells)
        assert len(cells[c]) <= 1, (k, c, cells)
        changed[c] += len(cells[c])
    assert changed[0] and changed[1], changed  # both tables learn (GridLake rewards are sparse: a few cells)
    assert not np.array_equal(run.qa, run.qb)


def test_bootstrap_follows_argmax_with_ties_and_nan():
    nan, inf = np.nan, np.inf
    f = np.dtype(np.float64)
    y = np.array([10.0, 20.0, 30.0, 40.0])
    assert bootstrap(np.array([1.0, 3.0, 3.0, 2.0]), y, f) == 20.0           # first of the tied maxima
    assert bootstrap(np.array([1.0, nan, 5.0, nan]), y, f) == 20.0          # a NaN is the maximum, the first one wins
    assert bootstrap(np.array([inf, nan, inf, 0.0]), y, f) == 20.0
    assert bootstrap(np.array([-inf, -inf, -inf, -inf]), y, f) == 10.0      # all -inf: index 0, not "none"
    assert bootstrap(np.array([-0.0, 0.0, -1.0, 0.0]), y, f) == 10.0        # signed zeros tie
    assert bootstrap(np.array([2.0, inf, inf, 1.0]), y, f) == 20.0
    got = bootstrap(np.array([]), np.array([]), np.dtype(np.float32))
    assert got == -inf and got.dtype == np.float32                           # the empty maximum of the Q-learning path
    assert np.isnan(bootstrap(np.array([0.0, 1.0]), np.array([5.0, nan]), f))  # Y's value is taken as it is


@pytest.mark.parametrize("special", ["tie", "nan"])
def test_a_bandit_step_worked_out_by_hand(special):
    """One state, two actions, s' == s: the update of step k bootstraps from Y[0, argmax X[0]] with the rows as they stood
    before the store."""
    seed, lr, gamma = 4, 0.5, 0.9
    qa0 = np.array([[1.0, 1.0]]) if special == "tie" else np.array([[1.0, np.nan]])
    qb0 = np.array([[5.0, 7.0]])
    run = DoubleRun(oenvs.RiggedBanditVecEnv(1, episode_len=50), gamma, OracleSchedule("constant", 1.0),
                    OracleSchedule("constant", lr), seed=seed, dtype=np.float64, agent_id=0, qa0=qa0, qb0=qb0)
    run.reset()
    env = copy.deepcopy(run.env)
    want = [qa0.copy(), qb0.copy()]
    for k in range(6):
        trace = run.rt.trace = []
        run.run(1)
        a = int(trace[0][0][0])
        _, rewards, *_ = env.step(np.array([a], dtype=np.int32))
        c = coin(seed, 0, k)
        X, Y = want[c], want[1 - c]
        star = 0
        for j in (0, 1):  # np.argmax, spelled out
            if not np.isnan(X[0, star]) and (np.isnan(X[0, j]) or X[0, j] > X[0, star]):
                star = j
        if k == 0 and c == 0:
            assert star == (0 if special == "tie" else 1)
        X[0, a] = X[0, a] + lr * ((np.float64(rewards[0]) + gamma * Y[0, star]) - X[0, a])
        assert np.array_equal(run.qa, want[0], equal_nan=True) and np.array_equal(run.qb, want[1], equal_nan=True), k


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_equal_one_call(kind, dt, mode):
    K = 120
    whole, halves = _run(kind, dt, mode), _run(kind, dt, mode)
    h, at = whole.run(2 * K)
    h1, at1 = halves.run(K)
    h2, at2 = halves.run(K)
    assert np.array_equal(np.concatenate([h1, h2]), h) and np.array_equal(np.concatenate([at1, at2 + K]), at)
    for a, b in ((whole.qa, halves.qa), (whole.qb, halves.qb)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and a.any()
    assert (whole.obs, whole.acc[0], whole.eps, whole.lr, whole.rt.step_counter) == \
        (halves.obs, halves.acc[0], halves.eps, halves.lr, halves.rt.step_counter)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_without_learning_the_run_is_the_q_learning_model_without_learning(kind, dt):
    K, offset, seed = 150, 3, 2
    eps = OracleSchedule("exponential", 0.9, 0.05, 0.99)
    zero = OracleSchedule("constant", 0.0)
    double = DoubleRun(_env(kind, offset), 0.9, eps, zero, seed=seed, dtype=dt, agent_id=offset)
    single = TdRun(_env(kind, offset), "q_learning", 0.9, eps, zero, seed=seed, dtype=dt, agent_id=offset)
    (h, at), (h1, at1) = double.run(K), single.run(K)
    assert np.array_equal(h, h1) and np.array_equal(at, at1) and len(h)
    assert (double.obs, double.acc[0], double.eps) == (single.obs, single.acc[0], single.eps)
    assert not double.qa.any() and not double.qb.any() and not single.q.any()


@pytest.mark.parametrize("kind", ["hash", "hash_masked", "table"])
def test_greedy_evaluation_with_an_empty_second_table_is_that_of_the_first(kind):
    offset, seed = 3, 2
    env = _env(kind, offset)
    rng = np.random.default_rng(0)
    qa0 = rng.standard_normal((env.state_size, env.action_size)).round(1)  # (rounded: ties)
    eps, lr = _schedules()
    double = DoubleRun(env, 0.9, eps, lr, seed=seed, dtype=np.float64, agent_id=offset, qa0=qa0)
    single = TdRun(_env(kind, offset), "q_learning", 0.9, eps, lr, seed=seed, dtype=np.float64, agent_id=offset, q0=qa0)
    # (a greedy policy need not end an episode: the episode form only where the step form has seen it end some)
    for ev in ("evaluate_steps", "evaluate_episodes") if kind == "hash_masked" else ("evaluate_steps",):
        n = 600 if ev == "evaluate_steps" else 3
        got = getattr(double, ev)(_env(kind, offset), n)
        val = _env(kind, offset)
        if hasattr(val, "step_index"):
            val.step_index = single.rt.step_counter
        want = getattr(single.rt, ev)(val, n)
        assert got[0] == want[0] and got[1] == want[1] and (len(got[1]) or kind != "hash_masked")
        assert double.rt.step_counter == single.rt.step_counter
