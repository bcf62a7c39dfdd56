"""CPU: the NumPy model of the population's visit counts (tests/visit_model.py), which the GPU parity tests of
``QLearningPopulation(exploration_bonus=..., visit_lr=...)`` compare against.

* With beta = 0 and no ``visit_lr`` the model is, bit for bit, ``TdRun("q_learning")`` (tests/td_rules_model.py): this
  anchors its step order, draws, schedules and update arithmetic to the merged model, which is anchored to the oracle --
  and the counts are a by-product.
* With beta > 0 and epsilon = 0 every valid action of a state is taken once before any is repeated.
* ``visit_lr`` with a constant rate of 1 and gamma = 0 on the bandit makes Q[0, a] the sequential running mean of the
  rewards of arm a.
* The counts saturate at 2^32 - 1.
* Two model calls equal one call.
"""
import copy

import numpy as np
import pytest

from dyna_model import _Recording
from oracle import envs as oenvs
from oracle.qlearn_oracle import OracleSchedule
from td_rules_model import TdRun
from test_trace_model import _same_run, _same_table, _special_table
from visit_model import VISIT_MAX, VisitRun, bonus


def _schedules():
    return OracleSchedule("exponential", 0.9, 0.05, 0.99), OracleSchedule("linear", 0.4, None, -1e-3)


def _env(kind, offset):
    if kind == "hash":
        return oenvs.HashTabularEnv(1, 60, 8, seed=3, agent_offset=offset)
    if kind == "hash_masked":  # 16 masked actions: the NumPy selection variants
        return oenvs.HashTabularEnv(1, 60, 16, seed=3, masked=True, agent_offset=offset)
    if kind == "grid":
        return oenvs.GridLakeEnv(1, side=6, seed=2)
    return oenvs.RiggedBanditVecEnv(1, episode_len=7)


def _walk(run, K):
    """K single steps; returns the (state, action) of each, read off the counts."""
    taken = []
    for _ in range(K):
        before = run.counts.copy()
        run.run(1)
        (s,), (a,) = np.nonzero(run.counts != before)
        assert run.counts[s, a] == before[s, a] + 1
        taken.append((int(s), int(a)))
    return taken


# ---- 1. beta = 0 without visit_lr is Q-learning --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("env_kind", ["hash", "grid"])
def test_without_bonus_and_rate_the_model_is_the_merged_model(env_kind, dt, mode):
    K, offset, seed = 150, 5, 9
    got = VisitRun(_env(env_kind, offset), 0.93, *_schedules(), beta=0.0, visit_lr=False, seed=seed, dtype=dt, mode=mode,
                   agent_id=offset)
    want = TdRun(_env(env_kind, offset), "q_learning", 0.93, *_schedules(), seed=seed, dtype=dt, mode=mode, agent_id=offset)
    assert _same_run(got, want, K)
    assert got.q.any() and got.counts.sum() == 2 * K and not got.bonus.any()
    if env_kind == "grid":  # (sparse reward: too few updates to tell the runs apart)
        return
    # ... and either option changes the run
    for kw in ({"beta": 0.5, "visit_lr": False}, {"beta": 0.0, "visit_lr": True}):
        other = VisitRun(_env(env_kind, offset), 0.93, *_schedules(), seed=seed, dtype=dt, mode=mode, agent_id=offset, **kw)
        other.run(2 * K)
        assert not _same_table(other.q, want.q), kw


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_without_bonus_and_rate_on_a_table_of_special_values(dt, mode):
    reached = 0
    for offset, masked, A in ((1, False, 8), (2, True, 8), (3, True, 16), (4, False, 8)):
        q0 = _special_table(30, A, dt, seed=offset, nan_row=offset == 4)
        env = oenvs.HashTabularEnv(1, 30, A, seed=1, masked=masked, agent_offset=offset)
        got = VisitRun(copy.deepcopy(env), 0.93, *_schedules(), beta=0.0, visit_lr=False, seed=2, dtype=dt, mode=mode,
                       agent_id=offset, q0=q0)
        want = TdRun(copy.deepcopy(env), "q_learning", 0.93, *_schedules(), seed=2, dtype=dt, mode=mode, agent_id=offset, q0=q0)
        _same_run(got, want, 150)
        reached = max(reached, got.rt.step_counter)
    assert reached > 30


# ---- 2. optimism: untried actions go first ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("env_kind", ["hash", "hash_masked", "grid"])
def test_every_valid_action_is_taken_once_before_any_is_repeated(env_kind, dt):
    env = _env(env_kind, 2)
    greedy = OracleSchedule("constant", 0.0)
    run = VisitRun(env, 0.9, greedy, OracleSchedule("constant", 0.3), beta=0.5, visit_lr=False, seed=4, dtype=dt, agent_id=2)
    taken = _walk(run, 400)
    by_state = {}
    for s, a in taken:
        by_state.setdefault(s, []).append(a)
    repeated = 0
    for s, acts in by_state.items():
        valid = np.flatnonzero(env.action_masks(np.array([s]))[0]) if env.masked else np.arange(env.action_size)
        first = acts[:len(valid)]
        assert len(set(first)) == len(first) and set(first) <= set(valid.tolist()), (s, acts)
        repeated += len(acts) > len(valid)
    assert repeated, "no state was visited often enough to repeat an action"
    assert np.isinf(run.bonus[run.counts == 0]).all() and np.isfinite(run.bonus[run.counts > 0]).all()


# ---- 3. the sample-average rate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_visit_lr_on_the_bandit_is_the_running_mean_of_each_arm(dt, mode):
    env = _Recording(_env("bandit", 0))
    run = VisitRun(env, 0.0, OracleSchedule("constant", 0.3), OracleSchedule("constant", 1.0), beta=0.0, visit_lr=True, seed=6,
                   dtype=dt, mode=mode)
    T = np.dtype(dt).type
    mean, n = [T(0), T(0)], [0, 0]
    for _ in range(120):
        before = run.counts.copy()
        run.run(1)
        a = int(np.flatnonzero((run.counts != before)[0])[0])
        n[a] += 1
        rate = 1.0 / n[a] if dt is np.float64 else np.float32(1.0 / n[a])  # alpha = lr_k / float64(N), rounded as lr_k is
        mean[a] = T(mean[a] + T(rate) * (T(env.last_reward) - mean[a]))
        assert run.q[0].tolist() == [float(mean[0]), float(mean[1])]
    assert min(n) > 5 and run.counts[0].tolist() == n
    assert abs(float(run.q[0, 0]) - float(run.q[0, 1])) > 0  # the rigged arms differ


# ---- 4. saturation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("visit_lr", [False, True])
def test_the_counts_saturate(visit_lr):
    n0 = np.full((1, 2), VISIT_MAX - 1, dtype=np.uint32)
    run = VisitRun(_env("bandit", 0), 0.9, OracleSchedule("constant", 0.5), OracleSchedule("constant", 0.5), beta=3.0,
                   visit_lr=visit_lr, seed=1, dtype=np.float32, n0=n0)
    run.run(5)
    assert run.counts.dtype == np.uint32 and run.counts.max() == VISIT_MAX and run.counts.min() >= VISIT_MAX - 1
    run.run(20)
    assert run.counts.tolist() == [[VISIT_MAX, VISIT_MAX]]
    assert np.array_equal(run.bonus, bonus(3.0, [[VISIT_MAX, VISIT_MAX]], np.float32)) and (run.bonus > 0).all()


def test_the_bonus_function():
    counts = np.array([0, 1, 2, 3, 4, 2 ** 24 + 1, VISIT_MAX], dtype=np.uint32)
    for dt in (np.float32, np.float64):
        assert not bonus(0.0, counts, dt).any() and bonus(0.0, counts, dt).dtype == dt
        b = bonus(0.5, counts, dt)
        assert b.dtype == dt and b[0] == np.inf and b[1] == 0.5 and b[4] == 0.25
        assert b[2] == dt(0.5 / np.sqrt(np.float64(2.0)))
        assert (np.diff(b) <= 0).all()


# ---- 5. chaining -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_kind", ["hash_masked", "bandit"])
def test_two_model_calls_equal_one(env_kind):
    offset = 3
    kw = {"beta": 0.5, "visit_lr": True, "seed": 4, "dtype": np.float32, "mode": "vec", "agent_id": offset}
    one = VisitRun(_env(env_kind, offset), 0.9, *_schedules(), **kw)
    two = VisitRun(_env(env_kind, offset), 0.9, *_schedules(), **kw)
    h1, a1 = one.run(120)
    h2a, a2a = two.run(60)
    h2b, a2b = two.run(60)
    assert _same_table(one.q, two.q) and np.array_equal(one.counts, two.counts)
    assert np.array_equal(h1, np.concatenate([h2a, h2b])) and np.array_equal(a1, np.concatenate([a2a, a2b + 60]))
