"""CPU: the NumPy model of the population's n-step Tree Backup (tests/tree_backup_model.py), which the GPU parity tests
of ``QLearningPopulation(tree_backup=n)`` compare against.

* With ``n = 1`` the model is, bit for bit, ``TdRun``'s Q-learning (tests/td_rules_model.py), which is anchored to the oracle.
* With epsilon 0 on a NaN-free table every action is greedy and the model is, bit for bit, n-step Expected SARSA at
  epsilon 0 (tests/n_step_model.py): the fold without a cut.
* Two three-step examples on the one-state bandit worked out by hand: a cut at ``i = j + 1`` and a cut deeper in the
  window, each continued through the steps after it (and one through a flush).
* Two model calls chained through the window equal one call.
"""
import copy

import numpy as np
import pytest

from n_step_model import NStepRun
from oracle import envs as oenvs
from oracle.qlearn_oracle import OracleSchedule
from td_rules_model import TdRun
from test_n_step_model import _env, _schedules
from tree_backup_model import TreeBackupRun


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["hash", "hash_masked", "bandit", "table"])
def test_one_step_is_the_merged_q_learning_model(kind, dt, mode):
    K, offset, seed = 150, 5, 9
    eps, lr = _schedules()
    got = TreeBackupRun(_env(kind, offset), 0.93, eps, lr, n=1, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    eps, lr = _schedules()
    want = TdRun(_env(kind, offset), "q_learning", 0.93, eps, lr, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    for _ in range(2):  # two chained calls
        (h1, a1), (h2, a2) = got.run(K), want.run(K)
        assert np.array_equal(got.q.view(np.uint8), want.q.view(np.uint8))
        assert np.array_equal(h1, h2) and np.array_equal(a1, a2)
        assert (got.obs, got.acc[0], got.eps, got.lr) == (want.obs, want.acc[0], want.eps, want.lr)
        assert got.rt.step_counter == want.rt.step_counter
        assert got.window[0] == 0 and got.rt.window == []
    assert got.q.any()


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2, 5, 16])
@pytest.mark.parametrize("kind", ["hash", "hash_masked", "bandit", "table"])
def test_without_exploration_it_is_n_step_expected_sarsa(kind, n, dt, mode):
    K, offset, seed = 150, 3, 9

    def schedules():
        return OracleSchedule("constant", 0.0), OracleSchedule("linear", 0.4, None, -1e-3)

    got = TreeBackupRun(_env(kind, offset), 0.93, *schedules(), n=n, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    want = NStepRun(_env(kind, offset), "expected_sarsa", 0.93, *schedules(), n=n, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    for _ in range(2):
        (h1, a1), (h2, a2) = got.run(K), want.run(K)
        assert np.isfinite(want.q).all()
        assert np.array_equal(got.q.view(np.uint8), want.q.view(np.uint8))
        assert np.array_equal(h1, h2) and np.array_equal(a1, a2)
        length, states, actions, rewards, greedy = got.window
        assert (length, *map(bytes, (states, actions, rewards))) == (want.window[0], *map(bytes, want.window[1:]))
        assert greedy[:length].all() and not greedy[length:].any()
    assert got.q.any()
    assert got.counts["steady_cut_next"] == got.counts["steady_cut_deep"] == got.counts["flush_cut"] == 0


def _scripted(actions, episode_len, dt, mode):
    """The bandit (one state, reward = action) at lr = gamma = 0.5 from Q0 = [0.25, 0.125], n = 3, with the picks given:
    every number of the examples is a dyadic fraction, so the arithmetic is exact in either dtype and learn mode."""
    run = TreeBackupRun(oenvs.RiggedBanditVecEnv(1, episode_len=episode_len), 0.5, OracleSchedule("constant", 0.0),
                        OracleSchedule("constant", 0.5), n=3, seed=0, dtype=dt, mode=mode, q0=[[0.25, 0.125]])
    script = list(actions)
    run.rt._pick = lambda states: np.array([script.pop(0)], dtype=np.int32)
    return run


MODES = ((np.float64, "iter"), (np.float32, "iter"), (np.float64, "vec"), (np.float32, "vec"))


def test_a_cut_at_the_next_entry_by_hand():
    """Entries are (a, r, f); f = (Q[a] == max Q) when the action was taken.

    step 0: a = 0, f = 1 (0.25 is the maximum), r = 0; W = [(0,0,1)]; no update.
    step 1: a = 1, f = 0 (0.125 is not), r = 1;        W = [(0,0,1), (1,1,0)]; no update.
    step 2: a = 0, f = 1, r = 0; L == n: entry 0.  Its nearest cut is entry 1 = j + 1: g_1 = max Q = 0.25, nothing to fold:
                                                       Q[0] = 0.25 + 0.5 (0 + 0.5 * 0.25 - 0.25)            = 0.1875
            (the uncut fold would have credited it with entry 1's reward: target 0.53125)
    step 3: a = 0, f = 1 (row [0.1875, 0.125]), r = 0; W = [(1,1,0), (0,0,1), (0,0,1)]; entry 0 -- its own flag is not
            read -- has no cut after it: v = 0.1875, g_2 = 0.09375, g_1 = 0.046875:
                                                       Q[1] = 0.125 + 0.5 (1 + 0.0234375 - 0.125)           = 0.57421875
    step 4: a = 0, f = 0 (row [0.1875, 0.57421875]), r = 0, terminated; W = [(0,0,1), (0,0,1), (0,0,0)]; flush:
            entry 0: nearest cut entry 2: g_2 = max Q = 0.57421875, g_1 = 0 + 0.5 g_2 = 0.287109375:
                                                       Q[0] = 0.1875 + 0.5 (0.1435546875 - 0.1875)          = 0.16552734375
            entry 1: cut at entry 2 = j + 1, the row read after that store: g_2 = 0.57421875:
                                                       Q[0] = 0.16552734375 + 0.5 (0.287109375 - 0.16552734375) = 0.226318359375
            entry 2 ends the episode:                  Q[0] = 0.226318359375 + 0.5 (0 - 0.226318359375)     = 0.1131591796875
    """
    want = [(0.25, 0.125), (0.25, 0.125), (0.1875, 0.125), (0.1875, 0.57421875), (0.1131591796875, 0.57421875)]
    for dt, mode in MODES:
        run = _scripted([0, 1, 0, 0, 0], 5, dt, mode)
        lengths, flags = [1, 2, 2, 2, 0], [[1, 0], [1, 0], [0, 1], [1, 1], [0, 0]]
        for t in range(5):
            run.run(1)
            assert tuple(run.q[0]) == want[t], (t, dt, mode)
            assert run.window[0] == lengths[t] and run.window[4].tolist() == flags[t], t
        c = run.counts
        assert (c["steady_cut_next"], c["steady_no_cut"], c["steady_cut_deep"], c["flush_cut"], c["flush_no_cut"]) == (1, 1, 0, 2, 0)
        assert c["cut_own_state"] == 3  # one state: every cut state is s'


def test_a_cut_deeper_in_the_window_by_hand():
    """step 0: a = 0, f = 1, r = 0.   step 1: a = 0, f = 1, r = 0.   No update.
    step 2: a = 1, f = 0, r = 1; W = [(0,0,1), (0,0,1), (1,1,0)]; entry 0: the nearest cut is entry 2 > j + 1 (this step's
            own entry): g_2 = max Q = 0.25, g_1 = 0 + 0.5 * 0.25 = 0.125:
                                                       Q[0] = 0.25 + 0.5 (0.0625 - 0.25)                    = 0.15625
    step 3: a = 0, f = 1 (row [0.15625, 0.125]), r = 0; W = [(0,0,1), (1,1,0), (0,0,1)]; entry 0: cut at entry 1:
            g_1 = 0.15625:                             Q[0] = 0.15625 + 0.5 (0.078125 - 0.15625)            = 0.1171875
    step 4: a = 1, f = 1 (row [0.1171875, 0.125]), r = 1; W = [(1,1,0), (0,0,1), (1,1,1)]; entry 0, no cut after it:
            v = 0.125, g_2 = 1.0625, g_1 = 0.53125:    Q[1] = 0.125 + 0.5 (1 + 0.265625 - 0.125)            = 0.6953125
    """
    want = [(0.25, 0.125), (0.25, 0.125), (0.15625, 0.125), (0.1171875, 0.125), (0.1171875, 0.6953125)]
    for dt, mode in MODES:
        run = _scripted([0, 0, 1, 0, 1], 10, dt, mode)
        for t in range(5):
            run.run(1)
            assert tuple(run.q[0]) == want[t], (t, dt, mode)
        c = run.counts
        assert (c["steady_cut_deep"], c["steady_cut_next"], c["steady_no_cut"]) == (1, 1, 1)
        length, states, actions, rewards, greedy = run.window
        assert (length, actions.tolist(), rewards.tolist(), greedy.tolist()) == (2, [0, 1], [0.0, 1.0], [1, 1])


@pytest.mark.parametrize("kind", ["hash", "hash_masked", "bandit"])
def test_two_calls_chained_through_the_window_equal_one(kind):
    K, n = 61, 4

    def make():
        return TreeBackupRun(_env(kind, 4), 0.9, OracleSchedule("constant", 0.5), OracleSchedule("exponential", 0.5, 0.01, 0.99),
                             n=n, seed=6, dtype=np.float32, agent_id=4)

    whole = make()
    ret, at = whole.run(2 * K)
    first = make()
    r1, a1 = first.run(K)
    assert first.window[0] > 0

    def resume(window):
        second = make()
        second.q[:] = first.q
        second.env, second.states, second.acc = copy.deepcopy(first.env), copy.deepcopy(first.states), first.acc.copy()
        second.rt.step_counter = first.rt.step_counter
        second.rt.lr_schedule.value, second.rt.exploration_rate_schedule.value = first.lr, first.eps
        second.rt.window = list(window)
        r2, a2 = second.run(K)
        return second, np.concatenate([r1, r2]), np.concatenate([a1, a2 + K])

    second, r12, a12 = resume(first.rt.window)
    assert np.array_equal(second.q.view(np.uint8), whole.q.view(np.uint8))
    assert np.array_equal(r12, ret) and np.array_equal(a12, at)
    assert (second.obs, second.lr) == (whole.obs, whole.lr)
    assert [np.asarray(x).tolist() for x in second.window] == [np.asarray(x).tolist() for x in whole.window]
    lost, _, _ = resume([])  # the dropped entries are never updated
    assert not np.array_equal(lost.q, whole.q)
