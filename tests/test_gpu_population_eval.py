"""GPU: greedy evaluation of every run of a ``QLearningPopulation`` (k_evaluate_runs), per-run draw counters and ``train``.

Run r of the population must be, bit for bit, the standalone one-agent ``GpuRolloutQLearning`` with agent_offset = r,
the same schedules and discount: its ``evaluate_steps`` / ``evaluate_episodes`` (returns, their float32 sum, draw
counter, final environment state) and its ``train`` (reward and validation histories, tables).  M = 67 is one full and
one partial wavefront; the standalone side runs for a subset of the runs.  Every evaluation asserts that path 7 ran.
"""
import copy
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M_ODD = 67
CHECK = (0, 1, 33, 63, 64, 66)


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms import QLearningPopulation
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return _lib, environments, schedules, QLearningPopulation, OptimalQLearningBase, GpuRolloutQLearning


def _schedules(M):
    """Different constant / linear / exponential epsilon and learning-rate schedules and discounts per run."""
    _, _, sch, *_ = _product()
    eps, lr, gamma = [], [], []
    for r in range(M):
        k = r % 3
        if k == 0:
            eps.append(sch.ConstantSchedule(0.05 + 0.01 * (r % 7)))
            lr.append(sch.ExponentialSchedule(0.5, 0.01 + 0.001 * r, 0.97))
        elif k == 1:
            eps.append(sch.LinearSchedule(0.9, -0.002 - 1e-5 * r))
            lr.append(sch.ConstantSchedule(0.1 + 0.002 * r))
        else:
            eps.append(sch.ExponentialSchedule(1.0, 0.02, 0.99 - 0.0005 * r))
            lr.append(sch.LinearSchedule(0.3, -1e-4))
        gamma.append(0.9 + 0.001 * r)
    return eps, lr, gamma


def _slippery_mdp(envs, seed=7, S=16, A=4, masked=False):
    """Every (state, action) has three outcomes, one of them terminal: episodes end under any policy, after a number
    of steps that differs from run to run."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    rng = np.random.default_rng(seed)
    probs = rng.random((S, A, 3)) + 0.05
    probs[..., 2] = 0.12 + 0.1 * rng.random((S, A))
    nxt = rng.integers(0, S, (S, A, 3))
    rew = rng.normal(size=(S, A, 3)).round(3)
    term = np.zeros((S, A, 3), dtype=bool)
    term[..., 2] = True
    masks = None
    if masked:
        masks = rng.random((S, A)) < 0.7
        masks[np.arange(S), rng.integers(0, A, S)] = True
    return encode_table_mdp(probs, nxt, rew, term, rng.dirichlet(np.ones(S)), masks)


def _env_factory(kind, envs):
    """(S, A, make_env(num_agents, agent_offset, seed))."""
    if kind in ("hash", "hash_masked"):
        S, A, masked = (300, 8, False) if kind == "hash" else (300, 16, True)
        return S, A, lambda n, off, seed: envs.HashTabularEnv(n, S, A, seed=seed, masked=masked, agent_offset=off)
    if kind == "grid":
        def grid(n, off, seed):
            env = envs.GridLakeEnv(n, side=6, seed=seed)
            env._params.agent_offset = off
            return env
        return 36, 4, grid
    if kind == "bandit":
        def bandit(n, off, seed):  # noqa: ARG001
            env = envs.RiggedTwoArmedBanditVecEnv(n, episode_len=7)
            env._params.agent_offset = off
            return env
        return 1, 2, bandit
    if kind == "tictactoe":
        return 19683, 9, lambda n, off, seed: envs.TicTacToeEnv(n, seed=seed, agent_offset=off)
    mdp = _slippery_mdp(envs, masked=True)
    return mdp.state_size, mdp.action_size, lambda n, off, seed: envs.TabularMDPEnv(n, mdp, seed=seed, agent_offset=off)


def _population(QLearningPopulation, M, S, A, sched, seed, dt, mode="iter"):
    eps_s, lr_s, gamma = sched
    return QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt,
                               learn_mode=mode)


def _standalone(r, S, A, sched, seed, dt, mode="iter"):
    _lib, _, _, _, OptimalQLearningBase, GpuRolloutQLearning = _product()
    eps_s, lr_s, gamma = sched
    algo = OptimalQLearningBase(S, A, gamma[r], seed=seed, dtype=dt)
    _lib.check(_lib.load().qe_set_agent_offset(algo.handle, r))
    return GpuRolloutQLearning(algo, copy.deepcopy(lr_s[r]), copy.deepcopy(eps_s[r]), learn_mode=mode)


def _train(rt, K, env, sd=None):
    """Standalone run_steps that tolerates a call without a finished episode (its mean divides by zero)."""
    try:
        return rt.run_steps(K, env, sd)[3]
    except ZeroDivisionError:
        return None


def _eval_variant(pop):
    d = pop.last_stats
    from dist_classicrl_amd import _lib

    assert _lib.decode_variant(d["kernel_variant"])["path"] == "population_eval", d


def _device_schedules(pop):
    from dist_classicrl_amd import _lib
    import ctypes as C

    eps = np.empty(pop.runs)
    lr = np.empty(pop.runs)
    _lib.check(pop._lib.qe_population_schedules(pop.handle, _lib.ptr(eps, C.c_double), _lib.ptr(lr, C.c_double)))
    return eps, lr


def _env_state(env):
    states, acc = env.observe()
    obs = states["observation"] if isinstance(states, dict) else states
    return obs, acc, env.aux()


# ---------------------------------------------------------------------------------------------------- 1. step mode
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["hash", "hash_masked", "grid", "bandit", "tictactoe", "table"])
def test_step_evaluation_after_training_matches_standalone(kind, dt):
    _lib, envs, *_ = _product()
    QLearningPopulation = _product()[3]
    K, V = 200, 150
    S, A, make_env = _env_factory(kind, envs)
    sched = _schedules(M_ODD)
    pop = _population(QLearningPopulation, M_ODD, S, A, sched, 11, dt)
    pop.run_steps(K, make_env(M_ODD, 0, 2))
    tables = pop.q_tables
    eps_before, lr_before = _device_schedules(pop)
    val = make_env(M_ODD, 0, 5)
    res = pop.evaluate_steps(val, V)
    _eval_variant(pop)
    assert pop.last_stats["dominant_env_steps"] == V * M_ODD
    # tables and schedule values bitwise untouched
    after = pop.q_tables
    assert np.array_equal(after.view(np.uint8), tables.view(np.uint8))
    eps_after, lr_after = _device_schedules(pop)
    assert np.array_equal(eps_after.view(np.uint64), eps_before.view(np.uint64))
    assert np.array_equal(lr_after.view(np.uint64), lr_before.view(np.uint64))
    assert np.array_equal(res.steps_used, np.full(M_ODD, V)) and res.finished.all()
    assert np.array_equal(pop.step_counters, np.full(M_ODD, K + V))
    assert pop.step_counter == K + V
    obs, acc, aux = _env_state(val)
    for r in CHECK:
        rt = _standalone(r, S, A, sched, 11, dt)
        _train(rt, K, make_env(1, r, 2))
        assert np.array_equal(tables[r], np.asarray(rt.algorithm.q_table)), f"{kind} run {r}: table"
        v1 = make_env(1, r, 5)
        total, history = rt.evaluate_steps(v1, V)
        want = np.array(history, dtype=np.float32)
        assert np.array_equal(res.run_returns(r), want), f"{kind} run {r}: returns"
        assert res.episode_counts[r] == len(history)
        assert res.totals[r] == total and res.totals.dtype == np.float32, (r, res.totals[r], total)
        assert pop.step_counters[r] == rt.algorithm.step_counter
        o1, a1, x1 = _env_state(v1)
        assert (obs[r], acc[r], aux[r]) == (o1[0], a1[0], x1[0]), f"{kind} run {r}: final state"


def test_step_evaluation_steps_over_nan_like_the_standalone():
    """Unmasked rows of 16 actions with NaN cells: the standalone's deterministic selection takes the NumPy variant
    above 10 actions (a NaN maximum: no selectable action), the list variant at or below (NaN cells skipped)."""
    _lib, envs, sch, QLearningPopulation, *_ = _product()
    for A in (8, 16):
        S, V = 50, 60
        rng = np.random.default_rng(A)
        init = rng.normal(size=(M_ODD, S, A)).astype(np.float32)
        init[rng.random(init.shape) < 0.02] = np.nan
        sched = ([sch.ConstantSchedule(0.1)] * M_ODD, [sch.ConstantSchedule(0.1)] * M_ODD, [0.9] * M_ODD)
        pop = _population(QLearningPopulation, M_ODD, S, A, sched, 3, np.float32)
        pop.set_q_tables(init)
        try:
            res = pop.evaluate_steps(envs.HashTabularEnv(M_ODD, S, A, seed=4), V)
            bad = []
        except IndexError as err:
            res, bad = err.result, err.runs
        _eval_variant(pop)
        for r in CHECK:
            rt = _standalone(r, S, A, sched, 3, np.float32)
            rt.algorithm.q_table = init[r]
            try:
                _, history = rt.evaluate_steps(envs.HashTabularEnv(1, S, A, seed=4, agent_offset=r), V)
                raised = False
            except IndexError:
                raised = True
            assert raised == (r in bad), (A, r)
            if not raised:
                assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), (A, r)


# ---------------------------------------------------------------------------------------------------- 2. episode mode
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_episode_evaluation_then_more_training_matches_standalone(dt):
    _lib, envs, _, QLearningPopulation, *_ = _product()
    K, E, K2 = 120, 4, 90
    mdp = _slippery_mdp(envs)
    S, A = mdp.state_size, mdp.action_size

    def make_env(n, off, seed):
        return envs.TabularMDPEnv(n, mdp, seed=seed, agent_offset=off)

    sched = _schedules(M_ODD)
    pop = _population(QLearningPopulation, M_ODD, S, A, sched, 5, dt)
    env = make_env(M_ODD, 0, 2)
    first = pop.run_steps(K, env)
    assert isinstance(first.state_dict["rng_step"], int) and first.state_dict["rng_step"] == K
    res = pop.evaluate_episodes(make_env(M_ODD, 0, 9), E)
    _eval_variant(pop)
    assert res.finished.all() and np.array_equal(res.episode_counts, np.full(M_ODD, E))
    assert len(set(res.steps_used.tolist())) > 1, "the runs should need different step counts"
    assert np.array_equal(pop.step_counters, K + res.steps_used)
    with pytest.raises(ValueError):
        pop.step_counter  # noqa: B018  (the runs no longer agree)
    second = pop.run_steps(K2, env, first.state_dict)
    assert np.array_equal(second.state_dict["rng_step"], K + res.steps_used + K2)
    tables = pop.q_tables
    for r in CHECK:
        rt = _standalone(r, S, A, sched, 5, dt)
        env1 = make_env(1, r, 2)
        sd1 = _train(rt, K, env1)
        total, history = rt.evaluate_episodes(make_env(1, r, 9), E)
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), r
        assert res.totals[r] == total, r
        assert res.steps_used[r] == rt.algorithm.step_counter - K, r
        history2 = []
        try:
            _, history2, _, sd2 = rt.run_steps(K2, env1, sd1)
        except ZeroDivisionError:
            sd2 = env1.state_dict()
            sd2["rng_step"] = rt.algorithm.step_counter
        assert np.array_equal(tables[r], np.asarray(rt.algorithm.q_table)), f"run {r}: table"
        assert np.array_equal(second.run_returns(r), np.array(history2, dtype=np.float32)), r
        sd = second.state_dict
        assert sd["states"][r] == sd2["states"][0] and sd["rewards"][r] == sd2["rewards"][0] and sd["aux"][r] == sd2["aux"][0]
        assert sd["rng_step"][r] == sd2["rng_step"], r


# ---------------------------------------------------------------------------------------------------- 3. train
@pytest.mark.parametrize("val", ["steps", "episodes"])
def test_train_matches_standalone_train(val):
    _lib, envs, _, QLearningPopulation, *_ = _product()
    steps, every = 250, 70  # segments of 70, 70, 70 and 40 steps
    mdp = _slippery_mdp(envs, seed=11, masked=True)
    S, A = mdp.state_size, mdp.action_size

    def make_env(n, off, seed):
        return envs.TabularMDPEnv(n, mdp, seed=seed, agent_offset=off)

    kw = {"val_steps": 60} if val == "steps" else {"val_episodes": 3}
    sched = _schedules(M_ODD)
    pop = _population(QLearningPopulation, M_ODD, S, A, sched, 8, np.float32)
    out = pop.train(make_env(M_ODD, 0, 2), steps, make_env(M_ODD, 0, 3), every, **kw)
    _eval_variant(pop)
    assert out.val_totals.shape == (4, M_ODD) and out.val_totals.dtype == np.float32
    assert out.val_finished.all() and len(out.segments) == 4
    tables = pop.q_tables
    for r in CHECK:
        rt = _standalone(r, S, A, sched, 8, np.float32)
        history, val_history, _, _ = rt.train(make_env(1, r, 2), steps, make_env(1, r, 3), every, **kw)
        assert np.array_equal(out.run_reward_history(r), np.array(history, dtype=np.float32)), r
        assert np.array_equal(out.val_totals[:, r], np.array(val_history, dtype=np.float32)), r
        assert np.array_equal(tables[r], np.asarray(rt.algorithm.q_table)), r
        assert pop.step_counters[r] == rt.algorithm.step_counter, r


def test_train_rejects_bad_arguments_before_the_device():
    _lib, envs, _, QLearningPopulation, *_ = _product()
    pop = QLearningPopulation(8, 50, 4)
    env = envs.HashTabularEnv(8, 50, 4)
    counter = pop.step_counter
    with pytest.raises(ValueError):
        pop.train(env, 10, env, 5)
    with pytest.raises(ValueError):
        pop.train(env, 10, env, 5, val_steps=3, val_episodes=3)
    with pytest.raises(ValueError):
        pop.train(env, 10, envs.HashTabularEnv(9, 50, 4), 5, val_steps=3)
    with pytest.raises(TypeError):
        pop.train(env, 10, object(), 5, val_steps=3)
    with pytest.raises(ValueError):
        pop.evaluate_steps(envs.HashTabularEnv(7, 50, 4), 3)
    assert pop.step_counter == counter


# ---------------------------------------------------------------------------------------------------- 4. resume
def test_resume_with_differing_counters_equals_the_uninterrupted_population(tmp_path):
    _lib, envs, _, QLearningPopulation, *_ = _product()
    mdp = _slippery_mdp(envs, seed=3)
    S, A = mdp.state_size, mdp.action_size
    sched = _schedules(M_ODD)

    def make_env(n, seed):
        return envs.TabularMDPEnv(n, mdp, seed=seed)

    whole = _population(QLearningPopulation, M_ODD, S, A, sched, 6, np.float64)
    env = make_env(M_ODD, 2)
    first = whole.run_steps(80, env)
    ev = whole.evaluate_episodes(make_env(M_ODD, 4), 3)
    assert len(set(ev.steps_used.tolist())) > 1
    second = whole.run_steps(50, env, first.state_dict)
    assert isinstance(second.state_dict["rng_step"], np.ndarray)
    whole.save(tmp_path / "tables.npy")
    saved = pickle.loads(pickle.dumps(second.state_dict))
    third = whole.run_steps(60, env, second.state_dict)

    fresh = _population(QLearningPopulation, M_ODD, S, A, sched, 6, np.float64)
    fresh.load(tmp_path / "tables.npy")
    fresh.restore_training_state(saved)
    assert np.array_equal(fresh.step_counters, second.state_dict["rng_step"])
    again = fresh.run_steps(60, make_env(M_ODD, 2), saved)
    assert np.array_equal(fresh.q_tables, whole.q_tables)
    assert np.array_equal(again.returns, third.returns) and np.array_equal(again.offsets, third.offsets)
    for key in ("states", "aux", "rewards", "lr", "exploration_rate", "rng_step"):
        assert np.array_equal(again.state_dict[key], third.state_dict[key]), key
    # an old-style dict (one int) puts every run back on one counter
    fresh.restore_training_state(first.state_dict)
    assert fresh.step_counter == 80 and np.array_equal(fresh.step_counters, np.full(M_ODD, 80))


# ---------------------------------------------------------------------------------------------------- 5. split launches
@pytest.mark.parametrize("mode", ["steps", "episodes"])
def test_an_evaluation_split_over_launches_matches_standalone(mode):
    _lib, envs, sch, QLearningPopulation, *_ = _product()
    M = 4096
    mdp = _slippery_mdp(envs, seed=21, S=24, A=8)
    S, A = mdp.state_size, mdp.action_size
    rng = np.random.default_rng(0)
    init = rng.normal(size=(M, S, A)).astype(np.float32)
    sched = ([sch.ConstantSchedule(0.1)] * M, [sch.ConstantSchedule(0.1)] * M, [0.9] * M)
    pop = _population(QLearningPopulation, M, S, A, sched, 1, np.float32)
    pop.set_q_tables(init)
    make = lambda n, off: envs.TabularMDPEnv(n, mdp, seed=6, agent_offset=off)  # noqa: E731
    if mode == "steps":
        V = 9000  # > 2048 steps per logged launch at 4096 runs, > 8192 per unlogged one
        res = pop.evaluate_steps(make(M, 0), V)
        assert pop.last_stats["launches"] == 3 * 5  # five launches, each with its log scan and pack
        pop.step_counter = 0  # the same evaluation again, without the log
        plain = pop.evaluate_steps(make(M, 0), V, log=False)
        assert pop.last_stats["launches"] == 2
    else:
        E = 500  # about 3000 steps per run: two or more logged launches
        res = pop.evaluate_episodes(make(M, 0), E)
        assert res.finished.all() and res.steps_used.max() > 2048
        assert pop.last_stats["launches"] >= 6
        pop.step_counter = 0
        plain = pop.evaluate_episodes(make(M, 0), E, log=False)
    _eval_variant(pop)
    assert np.array_equal(plain.totals, res.totals) and np.array_equal(plain.steps_used, res.steps_used)
    assert np.array_equal(np.diff(res.offsets), res.episode_counts)
    for r in (0, 1, 2047, 2048, M - 1):
        rt = _standalone(r, S, A, sched, 1, np.float32)
        rt.algorithm.q_table = init[r]
        start = rt.algorithm.step_counter
        if mode == "steps":
            total, history = rt.evaluate_steps(make(1, r), V)
        else:
            total, history = rt.evaluate_episodes(make(1, r), E)
            assert res.steps_used[r] == rt.algorithm.step_counter - start, r
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), r
        assert res.totals[r] == total, r


# ---------------------------------------------------------------------------------------------------- 6. bounded / empty
def test_episode_mode_is_bounded_and_reports_unfinished_runs():
    _lib, envs, sch, QLearningPopulation, *_ = _product()
    # state 0: action 0 stays in state 0 (not terminal), action 1 ends the episode; state 1 is never reached
    env = envs.TabularMDPEnv.from_arrays(M_ODD, [[0, 0], [1, 1]], [[0.5, 1.0], [0.0, 0.0]], [[False, True], [False, True]])
    init = np.zeros((M_ODD, 2, 2), dtype=np.float32)
    looping = np.arange(M_ODD) % 3 == 1
    init[looping, 0, 0] = 1.0   # greedy: stay forever
    init[~looping, 0, 1] = 1.0  # greedy: end the episode every step
    sched = ([sch.ConstantSchedule(0.1)] * M_ODD, [sch.ConstantSchedule(0.1)] * M_ODD, [0.9] * M_ODD)
    pop = _population(QLearningPopulation, M_ODD, 2, 2, sched, 0, np.float32)
    pop.set_q_tables(init)
    res = pop.evaluate_episodes(env, 2, max_steps=50)
    _eval_variant(pop)
    assert np.array_equal(res.finished, ~looping)
    assert np.array_equal(res.steps_used, np.where(looping, 50, 2))
    assert np.array_equal(res.episode_counts, np.where(looping, 0, 2))
    assert np.array_equal(res.totals, np.where(looping, 0.0, 2.0).astype(np.float32))
    assert np.array_equal(pop.step_counters, res.steps_used)
    assert np.array_equal(pop.q_tables, init)
    # the default bound: 1000 steps per requested episode
    res = pop.evaluate_episodes(env, 3)
    assert np.array_equal(res.steps_used, np.where(looping, 3000, 3))


def test_an_empty_masked_row_raises_naming_the_runs():
    _lib, envs, sch, QLearningPopulation, *_ = _product()
    # state 0: action 0 leads to state 1, whose row has no valid action; action 1 ends the episode
    masks = np.array([[True, True], [False, False]])
    env = envs.TabularMDPEnv.from_arrays(M_ODD, [[1, 0], [1, 1]], 1.0, [[False, True], [False, False]], action_masks=masks)
    init = np.zeros((M_ODD, 2, 2), dtype=np.float32)
    bad = [r for r in range(M_ODD) if r % 20 == 7]
    init[:, 0, 1] = 1.0
    init[bad, 0, 0] = 2.0
    sched = ([sch.ConstantSchedule(0.1)] * M_ODD, [sch.ConstantSchedule(0.1)] * M_ODD, [0.9] * M_ODD)
    pop = _population(QLearningPopulation, M_ODD, 2, 2, sched, 0, np.float32)
    pop.set_q_tables(init)
    with pytest.raises(IndexError) as info:
        pop.evaluate_steps(env, 10)
    _eval_variant(pop)
    assert info.value.runs == bad
    assert str(info.value).endswith("(runs " + ", ".join(map(str, bad)) + ")")
    good = np.setdiff1d(np.arange(M_ODD), bad)
    assert np.array_equal(info.value.result.episode_counts[good], np.full(good.size, 10))
    with pytest.raises(IndexError) as info:
        pop.evaluate_episodes(env, 4)
    assert info.value.runs == bad
