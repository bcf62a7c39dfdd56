"""GPU: ``QLearningPopulation`` -- M independent single-agent runs in one launch (k_rollout_runs).

Run r of a population must be, bit for bit, the standalone one-agent run with its own schedules and discount on the
same environment with agent_offset = r: against the C oracle (HashEnv) and against one-agent ``GpuRolloutQLearning``
runs (Grid, Bandit, TicTacToe, TabularMDP).  Every case also asserts that the population kernel ran (path 6).
"""
import copy

import numpy as np
import pytest

from oracle import c_oracle

pytestmark = pytest.mark.gpu

S_HASH, K_STEPS, M_ODD = 1000, 300, 67  # 67 runs: a full and a partial wavefront


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
            lr.append(sch.ExponentialSchedule(0.5, 0.01 + 0.001 * r, 0.97))  # reaches its floor inside the call
        elif k == 1:
            eps.append(sch.LinearSchedule(0.9, -0.002 - 1e-5 * r))
            lr.append(sch.ConstantSchedule(0.1 + 0.002 * r))
        else:
            eps.append(sch.ExponentialSchedule(1.0, 0.02, 0.99 - 0.0005 * r))
            lr.append(sch.LinearSchedule(0.3, -1e-4))
        gamma.append(0.9 + 0.001 * r)
    return eps, lr, gamma


def _variant_ok(pop):
    assert pop.last_stats["kernel_variant"] & 0xF == 6, pop.last_stats


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [8, 16])
def test_runs_match_the_c_oracle(A, masked, dt, mode):
    _lib, envs, _, QLearningPopulation, *_ = _product()
    eps_s, lr_s, gamma = _schedules(M_ODD)
    pop = QLearningPopulation(M_ODD, S_HASH, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=dt,
                              learn_mode=mode)
    res = pop.run_steps(K_STEPS, envs.HashTabularEnv(M_ODD, S_HASH, A, seed=1, masked=masked))
    _variant_ok(pop)
    d = _lib.decode_variant(pop.last_stats["kernel_variant"])
    assert d["masked"] == masked and d["nv"] == {8: 2, 16: 4}[A], d
    tables = pop.q_tables
    sd = res.state_dict
    for r in range(M_ODD):
        ref = c_oracle.CHashRollout(1, S_HASH, A, masked=masked, agent_offset=r, gamma=gamma[r], dtype=dt, mode=mode)
        want = ref.run(copy.deepcopy(eps_s[r]).advance_values(1, K_STEPS), copy.deepcopy(lr_s[r]).advance_values(1, K_STEPS))
        assert np.array_equal(tables[r], ref.q), f"run {r}: table"
        assert np.array_equal(res.run_returns(r), want["history"]), f"run {r}: returns"
        assert np.array_equal(res.run_steps(r), want["ep_step"]), f"run {r}: episode steps"
        assert res.episode_counts[r] == want["episodes"]
        assert sd["states"][r] == ref.obs[0] and sd["aux"][r] == ref.episode[0] and sd["rewards"][r] == ref.acc[0], r
        if want["episodes"]:
            assert res.mean_returns[r] == np.cumsum(want["history"], dtype=np.float32)[-1] / np.float32(want["episodes"])
        else:
            assert np.isnan(res.mean_returns[r])
    # schedules are left advanced like the standalone runtime leaves them
    for r in (0, 1, 2, M_ODD - 1):
        want = copy.deepcopy(eps_s[r])
        want.advance_values(1, K_STEPS)
        assert pop.exploration_rate_schedules[r].get_value() == want.get_value()
    assert pop.step_counter == K_STEPS


def _table_env_factory(envs):
    """A stochastic (3 outcomes), masked 20 x 5 MDP with a spread start distribution."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    rng = np.random.default_rng(7)
    S, A, K = 20, 5, 3
    probs = rng.random((S, A, K))
    probs[..., 2] *= rng.random((S, A)) < 0.5
    nxt = rng.integers(0, S, (S, A, K))
    rew = rng.normal(size=(S, A, K)).round(3)
    term = rng.random((S, A, K)) < 0.08
    masks = rng.random((S, A)) < 0.7
    masks[np.arange(S), rng.integers(0, A, S)] = True
    mdp = encode_table_mdp(probs, nxt, rew, term, rng.dirichlet(np.ones(S)), masks)
    return S, A, lambda n, off: envs.TabularMDPEnv(n, mdp, seed=3, agent_offset=off)


def _env_factory(kind, envs):
    if kind == "grid":
        def grid(n, off):
            env = envs.GridLakeEnv(n, side=6, seed=2)
            env._params.agent_offset = off
            return env
        return 36, 4, grid
    if kind == "bandit":
        def bandit(n, off):
            env = envs.RiggedTwoArmedBanditVecEnv(n, episode_len=7)
            env._params.agent_offset = off
            return env
        return 1, 2, bandit
    if kind == "tictactoe":
        return 19683, 9, lambda n, off: envs.TicTacToeEnv(n, seed=5, agent_offset=off)
    return _table_env_factory(envs)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["grid", "bandit", "tictactoe", "table"])
def test_runs_match_standalone_one_agent_runs(kind, dt, mode):
    _lib, envs, _, QLearningPopulation, OptimalQLearningBase, GpuRolloutQLearning = _product()
    M, K = 100, 250
    S, A, make_env = _env_factory(kind, envs)
    eps_s, lr_s, gamma = _schedules(M)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=11, dtype=dt, learn_mode=mode)
    res = pop.run_steps(K, make_env(M, 0))
    _variant_ok(pop)
    tables = pop.q_tables
    sd = res.state_dict
    for r in (0, 1, 63, 64, M - 1):
        algo = OptimalQLearningBase(S, A, gamma[r], seed=11, dtype=dt)
        _lib.check(_lib.load().qe_set_agent_offset(algo.handle, r))
        rt = GpuRolloutQLearning(algo, copy.deepcopy(lr_s[r]), copy.deepcopy(eps_s[r]), learn_mode=mode)
        env = make_env(1, r)
        try:
            mean, history, _, sd1 = rt.run_steps(K, env)
        except ZeroDivisionError:
            mean, history = None, []
            sd1 = env.state_dict()
        assert np.array_equal(tables[r], np.asarray(algo.q_table)), f"{kind} run {r}: table"
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), f"{kind} run {r}: returns"
        obs = sd1["states"]["observation"] if isinstance(sd1["states"], dict) else sd1["states"]
        assert sd["states"][r] == obs[0] and sd["aux"][r] == sd1["aux"][0] and sd["rewards"][r] == sd1["rewards"][0], r
        if mean is not None:
            assert res.mean_returns[r] == mean
        assert pop.lr_schedules[r].get_value() == rt.lr_schedule.get_value()


def test_two_calls_and_a_restored_population_equal_one_call(tmp_path):
    _lib, envs, _, QLearningPopulation, *_ = _product()
    M, S, A, K = 67, 500, 16, 150
    eps_s, lr_s, gamma = _schedules(M)

    def make():
        return QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=4, dtype=np.float32)

    whole = make()
    one = whole.run_steps(2 * K, envs.HashTabularEnv(M, S, A, seed=9, masked=True))
    halves = make()
    env = envs.HashTabularEnv(M, S, A, seed=9, masked=True)
    first = halves.run_steps(K, env)
    halves.save(tmp_path / "tables.npy")
    second = halves.run_steps(K, env, first.state_dict)
    restored = make()
    restored.load(tmp_path / "tables.npy")
    restored.restore_training_state(first.state_dict)
    third = restored.run_steps(K, envs.HashTabularEnv(M, S, A, seed=9, masked=True), first.state_dict)
    for pop in (whole, halves, restored):
        _variant_ok(pop)
    assert np.array_equal(halves.q_tables, whole.q_tables)
    assert np.array_equal(restored.q_tables, whole.q_tables)
    for r in range(M):
        want_ret, want_at = one.run_returns(r), one.run_steps(r)
        for tail in (second, third):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), want_ret), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + K]), want_at), r
    for key in ("states", "aux", "rewards", "lr", "exploration_rate"):
        assert np.array_equal(second.state_dict[key], one.state_dict[key]), key
        assert np.array_equal(third.state_dict[key], one.state_dict[key]), key
    assert halves.step_counter == restored.step_counter == whole.step_counter == 2 * K


def test_uploaded_tables_give_each_run_its_own_start():
    _lib, envs, sch, QLearningPopulation, *_ = _product()
    M, S, A, K = 70, 300, 8, 200
    rng = np.random.default_rng(3)
    init = rng.normal(size=(M, S, A))
    pop = QLearningPopulation(M, S, A, 0.95, sch.ConstantSchedule(0.2), sch.ConstantSchedule(0.3), seed=0, dtype=np.float64)
    pop.set_q_tables(init)
    assert np.array_equal(pop.q_tables, init)
    assert np.array_equal(pop.q_table(5), init[5])
    res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1))
    _variant_ok(pop)
    for r in (0, 5, 63, 64, M - 1):
        ref = c_oracle.CHashRollout(1, S, A, agent_offset=r, gamma=0.95, dtype=np.float64)
        ref.q[:] = init[r]
        want = ref.run(np.full(K, 0.3), np.full(K, 0.2))
        assert np.array_equal(pop.q_table(r), ref.q), r
        assert np.array_equal(res.run_returns(r), want["history"]), r
    pop.set_q_tables(init[0])  # (S, A): every run starts from it
    assert np.array_equal(pop.q_tables, np.broadcast_to(init[0], (M, S, A)))


def test_a_run_without_a_selectable_action_raises_and_the_others_are_unaffected():
    _lib, envs, sch, QLearningPopulation, *_ = _product()
    M, S, A, K = 16, 200, 8, 100  # one agent, unmasked: the list variant, which steps over NaN columns
    init = np.zeros((M, S, A), dtype=np.float32)
    init[5] = np.nan
    pop = QLearningPopulation(M, S, A, 0.9, sch.ConstantSchedule(0.1), sch.ConstantSchedule(0.0), seed=0, dtype=np.float32)
    pop.set_q_tables(init)
    with pytest.raises(IndexError) as info:
        pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1))
    _variant_ok(pop)
    assert info.value.runs == [5]
    assert str(info.value).endswith("(runs 5)")
    res = info.value.result
    tables = pop.q_tables
    for r in range(M):
        if r == 5:
            continue
        ref = c_oracle.CHashRollout(1, S, A, agent_offset=r, gamma=0.9, dtype=np.float32)
        want = ref.run(np.zeros(K), np.full(K, 0.1))
        assert np.array_equal(tables[r], ref.q), r
        assert np.array_equal(res.run_returns(r), want["history"]), r
        assert res.state_dict["states"][r] == ref.obs[0]


def test_errors():
    _lib, envs, _, QLearningPopulation, *_ = _product()
    import ctypes as C

    with pytest.raises(NotImplementedError):
        QLearningPopulation(4, 10, 65)
    pop = QLearningPopulation(8, 50, 4)
    with pytest.raises(ValueError):
        pop.run_steps(10, envs.HashTabularEnv(9, 50, 4))
    with pytest.raises(ValueError):
        pop.set_q_tables(np.zeros((7, 50, 4)))
    lib, h = _lib.load(), pop.handle
    env = envs.HashTabularEnv(8, 50, 4)
    env.bind(pop)
    assert lib.qe_population_runs(h) == 8
    s = np.zeros(8, dtype=np.int32)
    eps = np.full(4, 0.1)
    out = np.empty(8, dtype=np.int32)
    unsupported = _lib.ERR_UNSUPPORTED
    assert lib.qe_choose_actions(h, _lib.ptr(s, C.c_int32), 8, None, 0.1, 0, _lib.ptr(out, C.c_int32)) == unsupported
    r = np.zeros(8, dtype=np.float32)
    t = np.zeros(8, dtype=np.uint8)
    assert lib.qe_learn(h, _lib.ptr(s, C.c_int32), _lib.ptr(s, C.c_int32), _lib.ptr(r, C.c_float), _lib.ptr(s, C.c_int32),
                        _lib.ptr(t, C.c_uint8), 8, 0.1, None, 0) == unsupported
    f64 = _lib.ptr(eps, C.c_double)
    assert lib.qe_rollout(h, env.handle, 4, f64, f64, 0, None, None) == unsupported
    assert lib.qe_rollout_begin(h, env.handle, 4, f64, f64, 0, 0) == unsupported
    assert lib.qe_evaluate(h, env.handle, 4, None) == unsupported
    assert lib.qe_schedule_plan(h, f64, f64, 4) == unsupported
    assert lib.qe_rollout_chunk_limit(h, env.handle, 1) == unsupported
    assert lib.qe_delta_log_attach(h, None, 0) == unsupported
    rb = C.c_void_p()
    _lib.check(lib.qe_replay_create(C.byref(rb), 0, 16))
    try:
        assert lib.qe_replay_attach(h, rb) == unsupported
    finally:
        lib.qe_replay_destroy(rb)
    # ... while the population itself still runs on that environment
    res = pop.run_steps(20, env)
    _variant_ok(pop)
    assert res.episode_counts.shape == (8,)


def test_an_environment_that_outlives_its_population_is_released_cleanly():
    """Garbage collection may finalise the population before an environment bound to it (a reference cycle through a
    raised exception's traceback does): releasing the environment afterwards must not touch the destroyed engine, nor
    leave a HIP error behind for the next engine."""
    _lib, envs, _, QLearningPopulation, OptimalQLearningBase, _ = _product()
    pop = QLearningPopulation(8, 50, 4, dtype=np.float32)
    env = envs.HashTabularEnv(8, 50, 4)
    pop.run_steps(5, env)
    pop.__del__()  # the engine first ...
    env.close()    # ... then its environment
    algo = OptimalQLearningBase(3, 3, 0.9, seed=0, dtype=np.float32)  # (padded rows: qe_create checks its launch)
    assert np.array_equal(np.asarray(algo.q_table), np.zeros((3, 3), dtype=np.float32))


# ---- host bookkeeping around the launches: refused calls, zero-step calls, a method switched off and on again -----------------
TINY = (3, 4, 2)  # runs, states, actions
METHODS = [({"update_rule": "sarsa"}, 6), ({"update_rule": "expected_sarsa", "n_step": 3}, 6),
           ({"update_rule": "sarsa", "trace_decay": 0.5, "trace_length": 4}, 6), ({"planning_steps": 2}, 6), ({"double_q": True}, 9)]


def _tiny(**kw):
    _, envs, sch, QLearningPopulation, *_ = _product()
    pop = QLearningPopulation(*TINY, 0.9, sch.ExponentialSchedule(0.5, 0.01, 0.99), sch.LinearSchedule(0.9, -0.001), seed=3,
                              dtype=np.float32, **kw)
    return pop, envs.HashTabularEnv(*TINY, seed=1, p_term_256=64)


def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for key, value in b.items():
        if isinstance(value, dict):
            _same_dict(a[key], value)
        else:
            assert np.array_equal(a[key], value), key


def _same_call(pop, res, want_pop, want):
    """Two populations after a call each: tables, model, result and state dict are equal."""
    assert np.array_equal(pop.q_tables, want_pop.q_tables)
    if pop.double_q:
        assert np.array_equal(pop.q_tables_b, want_pop.q_tables_b)
    if pop.planning_steps:
        _same_dict(pop.planning_model, want_pop.planning_model)
    for field in ("mean_returns", "episode_counts", "returns", "offsets", "steps"):
        assert np.array_equal(getattr(res, field), getattr(want, field), equal_nan=True), field
    _same_dict(res.state_dict, want.state_dict)
    assert pop.last_stats["kernel_variant"] == want_pop.last_stats["kernel_variant"]


def test_a_refused_call_leaves_the_population_as_it_was():
    import ctypes as C

    _lib, envs, _, QLearningPopulation, *_ = _product()
    lib = _lib.load()
    M = TINY[0]
    pop, env = _tiny()
    res = pop.run_steps(60, env)
    assert res.episode_counts.sum() > 0 and res.returns.size == res.episode_counts.sum()
    other = QLearningPopulation(*TINY, dtype=np.float32)
    foreign = envs.HashTabularEnv(*TINY)
    foreign.bind(other)

    def state():
        eps, lr = np.empty(M), np.empty(M)
        _lib.check(lib.qe_population_schedules(pop.handle, _lib.ptr(eps, C.c_double), _lib.ptr(lr, C.c_double)))
        return [pop.step_counters, eps, lr, pop.q_tables]

    before = state()
    st = _lib.RolloutStats()
    h, ev = pop.handle, env.handle
    for call, text in (
            (lambda: lib.qe_population_rollout(h, ev, -1, _lib.LEARN_ITER, 1, C.byref(st), *[None] * 6), "steps must be >= 0"),
            (lambda: lib.qe_population_rollout(h, ev, 5, 2, 1, C.byref(st), *[None] * 6), "bad learn mode"),
            (lambda: lib.qe_population_rollout(h, foreign.handle, 5, _lib.LEARN_ITER, 1, C.byref(st), *[None] * 6), "engine/env mismatch"),
            (lambda: lib.qe_population_evaluate(h, ev, 5, -1, 1, C.byref(st), *[None] * 4), "episodes must be >= 0")):
        assert lib.qe_population_log(h, 0, None, None) == res.returns.size  # the log of the latest accepted call
        st.kernel_ms, st.launches, st.kernel_variant = 1.0, 1, 1
        assert call() == _lib.ERR_INVALID
        assert lib.qe_last_error().decode() == text
        assert not any(getattr(st, f) for f, _ in st._fields_), text
        assert lib.qe_population_log(h, 0, None, None) == 0, text
        for got, want in zip(state(), before):
            assert np.array_equal(got, want), text
        res = pop.run_steps(60, env, res.state_dict)  # ... and the population runs on
        before = state()
        assert res.returns.size > 0


@pytest.mark.parametrize(("kw", "variant"), METHODS)
def test_a_zero_step_call_moves_nothing_under_every_method(kw, variant):
    pop, env = _tiny(**kw)
    pop.step_counter = 11
    res = pop.run_steps(0, env)
    assert pop.last_stats["launches"] == 0 and pop.last_stats["kernel_variant"] == variant
    assert pop.step_counter == 11 and res.state_dict["rng_step"] == 11
    assert not res.episode_counts.any() and res.returns.size == 0
    sd = res.state_dict
    assert ("pending_actions" in sd) == (kw.get("update_rule") == "sarsa")
    assert ("n_step_window" in sd) == ("n_step" in kw) and ("eligibility_traces" in sd) == ("trace_decay" in kw)
    if "pending_actions" in sd:
        assert (sd["pending_actions"] == -1).all()
    if "n_step_window" in sd:
        assert not any(v.any() for v in sd["n_step_window"].values())
    if "eligibility_traces" in sd:
        assert not any(v.any() for v in sd["eligibility_traces"].values())
    if pop.planning_steps:
        model = pop.planning_model
        assert not model["count"].any() and (model["next_states"] == -1).all() and (model["visited"] == -1).all()
    after = pop.run_steps(20, env, sd)
    fresh, fresh_env = _tiny(**kw)
    fresh.step_counter = 11
    _same_call(pop, after, fresh, fresh.run_steps(20, fresh_env))
    assert pop.last_stats["launches"] > 0 and pop.step_counter == 31


@pytest.mark.parametrize("method", ["n_step", "traces", "planning"])
def test_a_method_switched_off_and_on_again_starts_from_nothing(method):
    import ctypes as C

    _lib, *_ = _product()
    lib = _lib.load()
    M = TINY[0]
    kw = {"n_step": {"update_rule": "sarsa", "n_step": 3}, "traces": {"update_rule": "sarsa", "trace_decay": 0.5, "trace_length": 4},
          "planning": {"planning_steps": 2}}[method]
    pop, env = _tiny(**kw)
    first = pop.run_steps(5, env)
    tables, h = pop.q_tables, pop.handle
    if method == "n_step":
        assert first.state_dict["n_step_window"]["length"].any()
        assert lib.qe_population_set_n_step(h, 1) == 0 and lib.qe_population_n_step(h) == 1
        assert lib.qe_population_set_n_step(h, 3) == 0 and lib.qe_population_n_step(h) == 3
        assert not any(v.any() for v in pop.n_step_window.values())
    elif method == "traces":
        assert first.state_dict["eligibility_traces"]["values"].any()
        assert lib.qe_population_set_traces(h, 0, 0, None) == 0 and lib.qe_population_trace_config(h, None, None, None) == 0
        assert lib.qe_population_set_traces(h, 4, 0, _lib.ptr(np.full(M, 0.5), C.c_double)) == 0
        assert lib.qe_population_trace_config(h, None, None, None) == 1
        assert not any(v.any() for v in pop.eligibility_traces.values())
    else:
        assert pop.planning_model["count"].all()
        assert lib.qe_population_set_planning(h, 0) == 0 and lib.qe_population_planning(h) == 0
        assert lib.qe_population_set_planning(h, 2) == 0 and lib.qe_population_planning(h) == 2
        model = pop.planning_model
        assert not model["count"].any() and (model["next_states"] == -1).all() and (model["visited"] == -1).all()
    # the environment, the schedules, the counters and SARSA's pending action go on; the method's own state does not
    sd = {k: v for k, v in first.state_dict.items() if k not in ("n_step_window", "eligibility_traces")}
    second = pop.run_steps(5, env, dict(sd))
    fresh, fresh_env = _tiny(**kw)
    fresh.set_q_tables(tables)
    fresh.restore_training_state(sd)
    _same_call(pop, second, fresh, fresh.run_steps(5, fresh_env, dict(sd)))
    assert pop.step_counter == 10 and not np.array_equal(pop.q_tables, tables)
