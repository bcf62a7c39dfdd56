"""CPU: the NumPy model of the population's update rules (tests/td_rules_model.py), which the GPU parity tests of
``QLearningPopulation(update_rule=...)`` compare against.

* With rule ``q_learning`` the model's loop is, bit for bit, the reference-pinned ``OracleRuntime`` on one agent: this
  anchors its step order, draws, schedules and update arithmetic (with the bootstrap scalar handed in) to the oracle.
* Expected SARSA at epsilon == 0 bootstraps from the maximum: bit for bit Q-learning.
* SARSA on the rigged bandit (every step has s' == s) and on a three-state episodic MDP gives the tables worked out by
  hand below.
* Two model calls chained through the pending action equal one call.  (A run that loses it re-picks with the same draws
  and epsilon from the row of the same state: another action only where the last update wrote into that row, s' == s --
  step 1 of the bandit case.)
"""
import copy

import numpy as np
import pytest

from oracle import envs as oenvs
from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning, OracleRuntime, OracleSchedule
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import TdRun, expected_value


def _env(kind, offset):
    if kind == "hash":
        return oenvs.HashTabularEnv(1, 60, 8, seed=3, agent_offset=offset)
    if kind == "hash_masked":  # 16 masked actions: the NumPy selection variants
        return oenvs.HashTabularEnv(1, 60, 16, seed=3, masked=True, agent_offset=offset)
    if kind == "grid":
        return oenvs.GridLakeEnv(1, side=4, seed=2)
    if kind == "tictactoe":
        return oenvs.TicTacToeVecEnv(1, seed=5, agent_offset=offset)
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    arrays, isd, masks = random_mdp(12, 5, 3, seed=4, masked=True)
    return TableMDPVecEnv(1, encode_table_mdp(*arrays, isd, masks), seed=3, agent_offset=offset)


def _schedules():
    return OracleSchedule("exponential", 0.9, 0.05, 0.99), OracleSchedule("linear", 0.4, None, -1e-3)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["hash", "hash_masked", "grid", "tictactoe", "table"])
def test_q_learning_rule_is_the_oracle_runtime_on_one_agent(kind, dt, mode):
    K, offset, seed = 150, 5, 9
    eps, lr = _schedules()
    run = TdRun(_env(kind, offset), "q_learning", 0.93, eps, lr, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    history, _ = run.run(K)

    env = _env(kind, offset)
    algo = OracleQLearning(env.state_size, env.action_size, 0.93, seed=seed, dtype=np.dtype(dt))
    algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=getattr(env, "agent_ids", np.array([offset], dtype=np.uint32)))
    eps, lr = _schedules()
    rt = OracleRuntime(algo, lr, eps, learn_mode=mode)
    try:
        _, want, _, sd = rt.run_steps(K, env)
    except ZeroDivisionError:
        pytest.fail("the case must end an episode")
    assert np.array_equal(run.q.view(np.uint8), algo.q_table.view(np.uint8))
    assert np.array_equal(history, np.array(want, dtype=np.float32))
    obs = sd["states"]["observation"] if isinstance(sd["states"], dict) else sd["states"]
    assert run.obs == obs[0] and run.acc[0] == sd["rewards"][0]
    assert (run.eps, run.lr) == (eps.get_value(), lr.get_value())
    assert run.q.any()


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["hash", "hash_masked", "table"])
def test_expected_sarsa_without_exploration_is_q_learning(kind, dt, mode):
    lr = OracleSchedule("linear", 0.4, None, -1e-3)
    runs = [TdRun(_env(kind, 2), rule, 0.9, OracleSchedule("constant", 0.0), copy.copy(lr), seed=1, dtype=dt, mode=mode,
                  agent_id=2) for rule in ("q_learning", "expected_sarsa")]
    results = [r.run(200) for r in runs]
    assert np.array_equal(runs[0].q.view(np.uint8), runs[1].q.view(np.uint8)) and runs[0].q.any()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])


def test_expected_value_by_hand():
    row = np.array([1.0, 3.0, -2.0, 0.5], dtype=np.float32)  # max 3, mean 2.5 / 4 = 0.625
    assert expected_value(row, 0.2, row.dtype) == np.float32(0.8 * 3.0 + 0.2 * 0.625)
    assert expected_value(row, -0.3, row.dtype) == np.float32(3.0)      # epsilon below 0 acts as 0
    assert expected_value(row, 1.7, row.dtype) == np.float32(0.625)     # ... above 1 as 1
    assert expected_value(row, 0.5, row.dtype).dtype == np.float32
    assert np.isnan(expected_value(np.array([1.0, np.nan]), 0.0, np.dtype(np.float64)))
    assert np.isnan(expected_value(np.array([1.0, np.inf]), 0.0, np.dtype(np.float64)))  # 0 * inf


def test_sarsa_on_the_bandit_by_hand():
    """One state, reward = action, epsilon 0, lr = gamma = 0.5, Q0 = [0.25, 0.2] (no ties: the draws do not matter).

    step 0: a = 0 (greedy), a' = 0 from [0.25, 0.2], v = 0.25:  Q[0] = 0.25 + 0.5 (0 + 0.125 - 0.25)   = 0.1875
    step 1: a = 0 (PENDING, though the row now prefers 1); its prediction is the UPDATED cell 0.1875;
            a' = 1 from [0.1875, 0.2], v = 0.2:                 Q[0] = 0.1875 + 0.5 (0 + 0.1 - 0.1875) = 0.14375
    step 2: a = 1, r = 1, a' = 1, v = 0.2:                      Q[1] = 0.2 + 0.5 (1 + 0.1 - 0.2)       = 0.65
    step 3: a = 1, r = 1, a' = 1, v = 0.65 (updated cell):      Q[1] = 0.65 + 0.5 (1 + 0.325 - 0.65)   = 0.9875
    """
    def make(rule):
        return TdRun(oenvs.RiggedBanditVecEnv(1, episode_len=10), rule, 0.5, OracleSchedule("constant", 0.0),
                     OracleSchedule("constant", 0.5), seed=0, dtype=np.float64, q0=[[0.25, 0.2]])

    run = make("sarsa")
    run.rt.trace = []
    want = [(0.1875, 0.2), (0.1875 + 0.5 * (0.0 + 0.5 * 0.2 - 0.1875), 0.2), None, None]
    want[2] = (want[1][0], 0.2 + 0.5 * (1.0 + 0.5 * 0.2 - 0.2))
    want[3] = (want[1][0], want[2][1] + 0.5 * (1.0 + 0.5 * want[2][1] - want[2][1]))
    for t in range(4):
        run.run(1)
        assert tuple(run.q[0]) == want[t], t
    assert np.allclose(run.q[0], [0.14375, 0.9875], rtol=0, atol=1e-15)
    assert [int(a[0][0]) for a in run.rt.trace] == [0, 0, 1, 1] and run.pending == 1
    # Q-learning on the same start takes action 1 already at step 1
    ql = make("q_learning")
    ql.rt.trace = []
    ql.run(2)
    assert [int(a[0][0]) for a in ql.rt.trace] == [0, 1]


def test_sarsa_on_a_three_state_episodic_mdp_by_hand():
    """States 0 (start), 1, 2; action a of state 0 leads to state 1 + a with reward 0; every action of state 1 ends the
    episode with reward 1, of state 2 with reward -1.  epsilon 0, lr = gamma = 0.5, Q0 = [[.3, .1], [.5, .2], [0, -.4]].

    step 0: s = 0, a = 0, s' = 1, a' = 0, v = 0.5:          Q[0,0] = 0.3 + 0.5 (0 + 0.25 - 0.3)      = 0.275
    step 1: s = 1, a = 0 (pending), r = 1, terminated; s' = 0 (reset), a' = 0 chosen from the new episode's first row
            and NOT bootstrapped from:                      Q[1,0] = 0.5 + 0.5 (1 - 0.5)             = 0.75
    step 2: s = 0, a = 0 (pending), s' = 1, a' = 0, v = 0.75: Q[0,0] = 0.275 + 0.5 (0 + 0.375 - 0.275) = 0.325
    step 3: s = 1, a = 0, r = 1, terminated:                Q[1,0] = 0.75 + 0.5 (1 - 0.75)           = 0.875
    """
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    nxt = np.array([[[1], [2]], [[0], [0]], [[0], [0]]])
    rew = np.array([[[0.0], [0.0]], [[1.0], [1.0]], [[-1.0], [-1.0]]])
    term = np.array([[[False], [False]], [[True], [True]], [[True], [True]]])
    mdp = encode_table_mdp(np.ones((3, 2, 1)), nxt, rew, term, np.array([1.0, 0.0, 0.0]))
    q0 = np.array([[0.3, 0.1], [0.5, 0.2], [0.0, -0.4]])
    run = TdRun(TableMDPVecEnv(1, mdp, seed=1), "sarsa", 0.5, OracleSchedule("constant", 0.0),
                OracleSchedule("constant", 0.5), seed=0, dtype=np.float64, q0=q0)
    returns, at = run.run(4)
    want = q0.copy()
    want[0, 0] = 0.3 + 0.5 * (0.0 + 0.5 * 0.5 - 0.3)
    want[1, 0] = 0.5 + 0.5 * (1.0 + 0.5 * 0 - 0.5)
    want[0, 0] = want[0, 0] + 0.5 * (0.0 + 0.5 * want[1, 0] - want[0, 0])
    want[1, 0] = want[1, 0] + 0.5 * (1.0 + 0.5 * 0 - want[1, 0])
    assert np.array_equal(run.q, want)
    assert np.allclose(run.q, [[0.325, 0.1], [0.875, 0.2], [0.0, -0.4]], rtol=0, atol=1e-15)
    assert returns.tolist() == [1.0, 1.0] and at.tolist() == [1, 3]
    assert run.obs == 0 and run.pending == 0


@pytest.mark.parametrize("kind", ["hash", "hash_masked", "tictactoe"])
def test_two_sarsa_calls_chained_through_the_pending_action_equal_one(kind):
    K = 120

    def make():
        return TdRun(_env(kind, 4), "sarsa", 0.9, OracleSchedule("constant", 0.5), OracleSchedule("exponential", 0.5, 0.01, 0.99),
                     seed=6, dtype=np.float32, agent_id=4)

    whole = make()
    ret, at = whole.run(2 * K)
    first = make()
    r1, a1 = first.run(K)
    assert first.pending >= 0

    def resume(pending):
        second = make()  # "a fresh process": table, env state, counter, schedules and the pending action carried over
        second.q[:] = first.q
        second.env, second.states, second.acc = copy.deepcopy(first.env), copy.deepcopy(first.states), first.acc.copy()
        second.rt.step_counter = first.rt.step_counter
        second.rt.lr_schedule.value, second.rt.exploration_rate_schedule.value = first.lr, first.eps
        second.rt.pending = pending
        r2, a2 = second.run(K)
        return second, np.concatenate([r1, r2]), np.concatenate([a1, a2 + K])

    second, r12, a12 = resume(first.pending)
    assert np.array_equal(second.q.view(np.uint8), whole.q.view(np.uint8))
    assert np.array_equal(r12, ret) and np.array_equal(a12, at)
    assert (second.obs, second.pending, second.lr) == (whole.obs, whole.pending, whole.lr)
