"""CPU: the NumPy model of the population's n-step rules (tests/n_step_model.py), which the GPU parity tests of
``QLearningPopulation(update_rule=..., n_step=n)`` compare against.

* With ``n = 1`` the model is, bit for bit, ``TdRun`` (tests/td_rules_model.py) for both rules: this anchors its step
  order, draws, schedules and update arithmetic to the merged model, which is anchored to the oracle.
* 2-step SARSA on the rigged bandit gives the tables worked out by hand below.
* Two model calls chained through the window equal one call, and a lost window does not.
* The NaN / infinity case of tests/test_gpu_n_step.py meets its two conditions in the model alone: some run has no
  selectable action, and some other run ends with a non-finite cell.
"""
import copy

import numpy as np
import pytest

from n_step_model import NStepRun
from oracle import envs as oenvs
from oracle.qlearn_oracle import OracleSchedule
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import TdRun

RULES = ["sarsa", "expected_sarsa"]


def _env(kind, offset):
    if kind == "hash":
        return oenvs.HashTabularEnv(1, 60, 8, seed=3, agent_offset=offset)
    if kind == "hash_masked":  # 16 masked actions: the NumPy selection variants
        return oenvs.HashTabularEnv(1, 60, 16, seed=3, masked=True, agent_offset=offset)
    if kind == "bandit":
        return oenvs.RiggedBanditVecEnv(1, episode_len=7)
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    arrays, isd, masks = random_mdp(12, 5, 3, seed=4, masked=True)
    return TableMDPVecEnv(1, encode_table_mdp(*arrays, isd, masks), seed=3, agent_offset=offset)


def _schedules():
    return OracleSchedule("exponential", 0.9, 0.05, 0.99), OracleSchedule("linear", 0.4, None, -1e-3)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["hash", "hash_masked", "bandit", "table"])
@pytest.mark.parametrize("rule", RULES)
def test_one_step_is_the_merged_model(rule, kind, dt, mode):
    K, offset, seed = 150, 5, 9
    eps, lr = _schedules()
    got = NStepRun(_env(kind, offset), rule, 0.93, eps, lr, n=1, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    eps, lr = _schedules()
    want = TdRun(_env(kind, offset), rule, 0.93, eps, lr, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    for _ in range(2):  # two chained calls
        (h1, a1), (h2, a2) = got.run(K), want.run(K)
        assert np.array_equal(got.q.view(np.uint8), want.q.view(np.uint8))
        assert np.array_equal(h1, h2) and np.array_equal(a1, a2)
        assert (got.obs, got.acc[0], got.pending, got.eps, got.lr) == (want.obs, want.acc[0], want.pending, want.eps, want.lr)
        assert got.rt.step_counter == want.rt.step_counter
        assert got.window[0] == 0 and got.rt.window == []
    assert got.q.any()


def test_two_step_sarsa_on_the_bandit_by_hand():
    """One state, reward = action, episodes of 3 steps, n = 2, epsilon 0, lr = gamma = 0.5, Q0 = [0.25, 0.125] (no
    ties: the draws do not matter; every number below is a dyadic fraction, so the arithmetic is exact).

    step 0: a = 0 (greedy), r = 0, W = [(0,0)]; a' = 0, v = 0.25; one entry: no update.
    step 1: a = 0 (pending), r = 0, W = [(0,0), (0,0)]; a' = 0, v = 0.25; L == n: entry 0 with
            g_1 = 0 + 0.5 * 0.25 = 0.125:              Q[0] = 0.25 + 0.5 (0 + 0.0625 - 0.25)              = 0.15625
    step 2: a = 0 (pending), r = 0, terminated, W = [(0,0), (0,0)]; a' = 0 from [0.15625, 0.125] (before the stores).
            Flush, oldest first: entry 0 with g_1 = 0 + 0 (entry 1 ends the episode):
                                                       Q[0] = 0.15625 + 0.5 (0 + 0 - 0.15625)             = 0.078125
            entry 1, the same cell, sees that update:  Q[0] = 0.078125 + 0.5 (0 - 0.078125)               = 0.0390625
    step 3: a = 0 (PENDING, though the row now prefers 1), r = 0, W = [(0,0)]; a' = 1, v = 0.125; no update.
    step 4: a = 1, r = 1, W = [(0,0), (1,1)]; a' = 1, v = 0.125; entry 0 -- action 0 -- is credited with the reward of
            the step after it, g_1 = 1 + 0.5 * 0.125 = 1.0625:
                                                       Q[0] = 0.0390625 + 0.5 (0 + 0.53125 - 0.0390625)   = 0.28515625
    step 5: a = 1 (pending), r = 1, terminated, W = [(1,1), (1,1)]; a' = 0 from [0.28515625, 0.125].
            entry 0 with g_1 = 1 + 0:                  Q[1] = 0.125 + 0.5 (1 + 0.5 - 0.125)               = 0.8125
            entry 1:                                   Q[1] = 0.8125 + 0.5 (1 - 0.8125)                   = 0.90625
    """
    for dt, mode in ((np.float64, "iter"), (np.float32, "iter"), (np.float64, "vec"), (np.float32, "vec")):
        run = NStepRun(oenvs.RiggedBanditVecEnv(1, episode_len=3), "sarsa", 0.5, OracleSchedule("constant", 0.0),
                       OracleSchedule("constant", 0.5), n=2, seed=0, dtype=dt, mode=mode, q0=[[0.25, 0.125]])
        run.rt.trace = []
        want = [(0.25, 0.125), (0.15625, 0.125), (0.0390625, 0.125), (0.0390625, 0.125), (0.28515625, 0.125),
                (0.28515625, 0.90625)]
        lengths, returns, ends = [1, 1, 0, 1, 1, 0], [], []
        for t in range(6):
            history, at = run.run(1)
            returns += history.tolist()
            ends += (at + t).tolist()
            assert tuple(run.q[0]) == want[t], (t, dt, mode)
            assert run.window[0] == lengths[t], t
        assert [int(a[0][0]) for a in run.rt.trace] == [0, 0, 0, 0, 1, 1]
        assert run.pending == 0 and returns == [0.0, 2.0] and ends == [2, 5]
        assert run.rt.step_counter == 6


def test_expected_sarsa_window_by_hand():
    """The same bandit under 2-step Expected SARSA at epsilon 0 (v = the maximum of the row before the stores); the pick
    of a step reads the row after the stores of the step before.

    step 0: a = 0, r = 0; v = 0.25; no update.
    step 1: a = 0, r = 0; v = 0.25, g_1 = 0.125:       Q[0] = 0.25 + 0.5 (0.0625 - 0.25)                  = 0.15625
    step 2: a = 0, r = 0, terminated: as SARSA's:      Q[0] = 0.0390625
    step 3: a = 1 (the row is [0.0390625, 0.125]), r = 1; no update.
    step 4: a = 1, r = 1; v = 0.125, g_1 = 1.0625:     Q[1] = 0.125 + 0.5 (1 + 0.53125 - 0.125)           = 0.828125
    step 5: a = 1, r = 1, terminated: entry 0, g_1 = 1: Q[1] = 0.828125 + 0.5 (1 + 0.5 - 0.828125)        = 1.1640625
            entry 1:                                   Q[1] = 1.1640625 + 0.5 (1 - 1.1640625)             = 1.08203125
    """
    run = NStepRun(oenvs.RiggedBanditVecEnv(1, episode_len=3), "expected_sarsa", 0.5, OracleSchedule("constant", 0.0),
                   OracleSchedule("constant", 0.5), n=2, seed=0, dtype=np.float64, q0=[[0.25, 0.125]])
    run.rt.trace = []
    want = [(0.25, 0.125), (0.15625, 0.125), (0.0390625, 0.125), (0.0390625, 0.125), (0.0390625, 0.828125),
            (0.0390625, 1.08203125)]
    for t in range(6):
        run.run(1)
        assert tuple(run.q[0]) == want[t], t
    assert [int(a[0][0]) for a in run.rt.trace] == [0, 0, 0, 1, 1, 1] and run.pending == -1


@pytest.mark.parametrize("kind", ["hash", "hash_masked", "bandit"])
@pytest.mark.parametrize("rule", RULES)
def test_two_calls_chained_through_the_window_equal_one(rule, kind):
    K, n = 61, 4

    def make():
        return NStepRun(_env(kind, 4), rule, 0.9, OracleSchedule("constant", 0.5), OracleSchedule("exponential", 0.5, 0.01, 0.99),
                        n=n, seed=6, dtype=np.float32, agent_id=4)

    whole = make()
    ret, at = whole.run(2 * K)
    first = make()
    r1, a1 = first.run(K)
    assert first.window[0] > 0

    def resume(window):
        second = make()  # "a fresh process": table, env state, counter, schedules, pending action and window carried over
        second.q[:] = first.q
        second.env, second.states, second.acc = copy.deepcopy(first.env), copy.deepcopy(first.states), first.acc.copy()
        second.rt.step_counter = first.rt.step_counter
        second.rt.lr_schedule.value, second.rt.exploration_rate_schedule.value = first.lr, first.eps
        second.rt.pending = first.rt.pending
        second.rt.window = list(window)
        r2, a2 = second.run(K)
        return second, np.concatenate([r1, r2]), np.concatenate([a1, a2 + K])

    second, r12, a12 = resume(first.rt.window)
    assert np.array_equal(second.q.view(np.uint8), whole.q.view(np.uint8))
    assert np.array_equal(r12, ret) and np.array_equal(a12, at)
    assert (second.obs, second.pending, second.lr, second.rt.window) == (whole.obs, whole.pending, whole.lr, whole.rt.window)
    lost, _, _ = resume([])  # the dropped entries are never updated
    assert not np.array_equal(lost.q, whole.q)


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [
    (8, False, np.float32, "iter"),
    (8, True, np.float64, "vec"),
    (16, True, np.float32, "vec"),
])
@pytest.mark.parametrize("rule", RULES)
def test_the_special_value_case_meets_its_conditions_in_the_model_alone(rule, A, masked, dt, mode):
    """What test_gpu_n_step.py's NaN test asserts about its inputs holds without a device."""
    from test_gpu_n_step import NAN_CASE, nan_case_model

    raised, special_kept = nan_case_model(rule, A, masked, dt, mode)
    assert raised, "no run met a row without a selectable action"
    assert special_kept, "no run finished with a NaN or an infinity in its table"
    assert len(raised) < NAN_CASE["M"]
