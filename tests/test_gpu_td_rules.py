"""GPU: ``QLearningPopulation(update_rule="sarsa" | "expected_sarsa")`` (k_rollout_runs_td) against the NumPy model of
the rules (tests/td_rules_model.py), bit for bit: per run the table, the episode returns and their steps, the counts,
the final observation / env word / running return, the pending action, the schedule values and the draw counter.  No
tolerance anywhere.  Every case asserts the kernel build it means to cover (path 8, rule, NV and masked bits).
"""
import copy
import pickle

import numpy as np
import pytest

from oracle import envs as oenvs
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import TdRun, env_word
from test_gpu_population import _schedules

pytestmark = pytest.mark.gpu

RULES = ["sarsa", "expected_sarsa"]
M_ODD = 67  # a full and a partial wavefront


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms import QLearningPopulation

    return _lib, environments, schedules, QLearningPopulation


def _nv(A):
    return max(4, 1 << (A - 1).bit_length()) // 4


def _reached(pop, rule, nv=None, masked=None):
    d = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert pop.last_stats["kernel_variant"] & 15 == 8 and d["path"] == "population_td" and d["rule"] == rule, d
    assert pop.update_rule == rule
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _check(pop, res, r, run, history, at, tables, counter):
    """Run r of a population call against its model run (after the same call)."""
    assert np.array_equal(tables[r], run.q, equal_nan=True), f"run {r}: table"
    assert np.array_equal(res.run_returns(r), history), f"run {r}: returns"
    assert np.array_equal(res.run_steps(r), at), f"run {r}: episode steps"
    assert res.episode_counts[r] == len(history), f"run {r}: episode count"
    if len(history):
        mean = np.cumsum(history, dtype=np.float32)[-1] / np.float32(len(history))
        assert res.mean_returns[r] == mean, f"run {r}: mean"
    else:
        assert np.isnan(res.mean_returns[r]), r
    sd = res.state_dict
    assert (sd["states"][r], sd["aux"][r], sd["rewards"][r]) == (run.obs, env_word(run.env), run.acc[0]), f"run {r}: state"
    if pop.update_rule == "sarsa":
        assert sd["pending_actions"][r] == run.pending, f"run {r}: pending action"
    else:
        assert "pending_actions" not in sd
    assert sd["exploration_rate"][r] == run.eps == pop.exploration_rate_schedules[r].get_value(), f"run {r}: epsilon"
    assert sd["lr"][r] == run.lr == pop.lr_schedules[r].get_value(), f"run {r}: learning rate"
    assert pop.step_counters[r] == counter == run.rt.step_counter, f"run {r}: draw counter"


def _model_env(kind, r, p):
    if kind == "hash":
        return oenvs.HashTabularEnv(1, p["S"], p["A"], seed=p["seed"], masked=p["masked"], agent_offset=r)
    if kind == "grid":
        return oenvs.GridLakeEnv(1, side=p["side"], seed=p["seed"])
    if kind == "bandit":
        return oenvs.RiggedBanditVecEnv(1, episode_len=p["episode_len"])
    if kind == "tictactoe":
        return oenvs.TicTacToeVecEnv(1, seed=p["seed"], agent_offset=r)
    return TableMDPVecEnv(1, p["mdp"], seed=p["seed"], agent_offset=r)


def _device_env(kind, M, p):
    envs = _product()[1]
    if kind == "hash":
        return envs.HashTabularEnv(M, p["S"], p["A"], seed=p["seed"], masked=p["masked"])
    if kind == "grid":
        return envs.GridLakeEnv(M, side=p["side"], seed=p["seed"])
    if kind == "bandit":
        return envs.RiggedTwoArmedBanditVecEnv(M, episode_len=p["episode_len"])
    if kind == "tictactoe":
        return envs.TicTacToeEnv(M, seed=p["seed"])
    return envs.TabularMDPEnv(M, p["mdp"], seed=p["seed"])


def _model_runs(kind, p, runs, rule, sched, seed, dt, mode, q0=None):
    eps_s, lr_s, gamma = sched
    return {r: TdRun(_model_env(kind, r, p), rule, gamma[r], eps_s[r], lr_s[r], seed=seed, dtype=dt, mode=mode, agent_id=r,
                     q0=None if q0 is None else q0[r]) for r in runs}


def _population(M, S, A, sched, seed, dt, mode, rule):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode,
                         update_rule=rule)


def _run_and_check(kind, p, S, A, M, K, rule, dt, mode, sched, seed=0, runs=None, nv=None, masked=None):
    pop = _population(M, S, A, sched, seed, dt, mode, rule)
    res = pop.run_steps(K, _device_env(kind, M, p))
    _reached(pop, rule, nv=nv, masked=masked)
    tables = pop.q_tables
    for r, run in _model_runs(kind, p, range(M) if runs is None else runs, rule, sched, seed, dt, mode).items():
        history, at = run.run(K)
        _check(pop, res, r, run, history, at, tables, K)
    return pop, res


# ---- 1. every row width, both dtypes, both learn modes --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [4, 8, 16, 64])
@pytest.mark.parametrize("rule", RULES)
def test_hash_runs_match_the_model(rule, A, masked, dt, mode):
    p = {"S": 300, "A": A, "seed": 1, "masked": masked}
    _run_and_check("hash", p, 300, A, M_ODD, 150, rule, dt, mode, _schedules(M_ODD), nv=_nv(A), masked=masked)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("rule", RULES)
def test_the_32_column_build_matches_the_model(rule, dt):
    p = {"S": 200, "A": 20, "seed": 1, "masked": True}
    _run_and_check("hash", p, 200, 20, M_ODD, 150, rule, dt, "iter", _schedules(M_ODD), nv=8, masked=True)


# ---- 2. the other environments: s' == s on walls and always on the bandit, TicTacToe, a stochastic masked MDP ---------
def _other(kind):
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    if kind == "grid":
        return 36, 4, {"side": 6, "seed": 2}, 1, False
    if kind == "bandit":
        return 1, 2, {"episode_len": 7}, 1, False
    if kind == "tictactoe":
        return 19683, 9, {"seed": 5}, 4, True
    arrays, isd, masks = random_mdp(20, 5, 3, seed=7, masked=True)
    return 20, 5, {"mdp": encode_table_mdp(*arrays, isd, masks), "seed": 3}, 2, True


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["grid", "bandit", "tictactoe", "table"])
@pytest.mark.parametrize("rule", RULES)
def test_other_environments_match_the_model(rule, kind, dt, mode):
    S, A, p, nv, masked = _other(kind)
    _run_and_check(kind, p, S, A, M_ODD, 150, rule, dt, mode, _schedules(M_ODD), seed=11, nv=nv, masked=masked)


# ---- 3. epsilon leaving [0, 1] in both directions (the clamp of Expected SARSA's e, the threshold of the picks) --------
@pytest.mark.parametrize("rule", RULES)
def test_linear_epsilon_that_leaves_the_unit_interval(rule):
    sch = _product()[2]
    M, K = M_ODD, 120
    eps = [sch.LinearSchedule(0.03, -0.001) if r % 2 else sch.LinearSchedule(0.96, 0.001 + 1e-5 * r) for r in range(M)]
    lr = [sch.ConstantSchedule(0.2 + 0.001 * r) for r in range(M)]
    p = {"S": 40, "A": 8, "seed": 1, "masked": False}
    pop, _ = _run_and_check("hash", p, 40, 8, M, K, rule, np.float64, "iter", (eps, lr, [0.95] * M), nv=2, masked=False)
    values = np.array([s.get_value() for s in pop.exploration_rate_schedules])
    assert values.min() < 0 and values.max() > 1


# ---- 4. Expected SARSA without exploration is Q-learning ---------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_expected_sarsa_at_epsilon_zero_equals_the_q_learning_population(dt):
    _lib, envs, sch, _ = _product()
    M, S, A, K = M_ODD, 200, 16, 300
    _, lr_s, gamma = _schedules(M)
    sched = ([sch.ConstantSchedule(0.0)] * M, lr_s, gamma)
    rng = np.random.default_rng(1)
    q0 = rng.standard_normal((M, S, A)).astype(dt)
    got = {}
    for rule in ("q_learning", "expected_sarsa"):
        pop = _population(M, S, A, sched, 3, dt, "iter", rule)
        pop.set_q_tables(q0)
        res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=True))
        got[rule] = (pop.q_tables, res)
        d = _lib.decode_variant(pop.last_stats["kernel_variant"])
        assert (d["path"], d["rule"]) == (("population", "q_learning") if rule == "q_learning" else ("population_td", rule)), d
    (qa, a), (qb, b) = got["q_learning"], got["expected_sarsa"]
    assert np.array_equal(qa, qb) and not np.array_equal(qa, q0)
    assert np.array_equal(a.returns, b.returns) and np.array_equal(a.steps, b.steps) and np.array_equal(a.offsets, b.offsets)
    for key in ("states", "aux", "rewards", "lr"):
        assert np.array_equal(a.state_dict[key], b.state_dict[key]), key


# ---- 5. chaining: calls, a fresh process, launches ---------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 400])  # four states: s' == s at many call boundaries
@pytest.mark.parametrize("rule", RULES)
def test_two_calls_and_a_restored_population_equal_one_call(rule, S, tmp_path):
    envs = _product()[1]
    M, A, K = M_ODD, 8, 90
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter", rule)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * K, env())
    halves = make()
    e = env()
    first = halves.run_steps(K, e)
    halves.save(tmp_path / "tables.npy")
    blob = pickle.dumps(first.state_dict)
    second = halves.run_steps(K, e, first.state_dict)
    restored = make()  # what a fresh process does: tables from the file, everything else from the pickled dict
    sd = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.restore_training_state(sd)
    if rule == "sarsa":
        assert np.array_equal(restored.pending_actions, first.state_dict["pending_actions"])
        assert (first.state_dict["pending_actions"] >= 0).all()
    third = restored.run_steps(K, env(), sd)
    for pop in (whole, halves, restored):
        _reached(pop, rule, nv=2, masked=True)
        assert np.array_equal(pop.q_tables, whole.q_tables)
        assert np.array_equal(pop.step_counters, np.full(M, 2 * K))
    for tail in (second, third):
        for r in range(M):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), one.run_returns(r)), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + K]), one.run_steps(r)), r
        assert sorted(tail.state_dict) == sorted(one.state_dict)
        for key in one.state_dict:
            if isinstance(one.state_dict[key], np.ndarray):
                assert np.array_equal(tail.state_dict[key], one.state_dict[key]), key
    # a dict without the key: every run picks at its first step with the draws and epsilon of that step (the model, told so)
    if rule == "sarsa":
        lost = make()
        lost.load(tmp_path / "tables.npy")
        stripped = {k: v for k, v in sd.items() if k != "pending_actions"}
        lost.restore_training_state(stripped)
        assert (lost.pending_actions == -1).all()
        res = lost.run_steps(K, env(), stripped)
        tables = lost.q_tables
        p = {"S": S, "A": A, "seed": 9, "masked": True}
        for r, run in _model_runs("hash", p, range(M), rule, sched, 4, np.float32, "iter").items():
            run.run(K)
            run.rt.pending = None
            history, at = run.run(K)
            _check(lost, res, r, run, history, at, tables, 2 * K)


@pytest.mark.parametrize("rule", RULES)
def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_and_the_model(rule):
    envs = _product()[1]
    M, K, S, A = 40_000, 2000, 100, 8
    eps0, lr0, gamma0 = _schedules(97)
    sched = [[x[r % 97] for r in range(M)] for x in (eps0, lr0, gamma0)]
    logged = _population(M, S, A, sched, 21, np.float32, "vec", rule)
    res = logged.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1))
    _reached(logged, rule, nv=2, masked=False)
    assert logged.last_stats["launches"] > 9, "the logged call must be cut into more than three launches"
    tables = logged.q_tables
    quiet = _population(M, S, A, sched, 21, np.float32, "vec", rule)
    res_q = quiet.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1), log=False)
    assert 1 < quiet.last_stats["launches"] < logged.last_stats["launches"] // 3, "the unlogged call is cut differently"
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    assert sorted(res_q.state_dict) == sorted(res.state_dict)
    for key, value in res.state_dict.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(res_q.state_dict[key], value), key
    del quiet
    p = {"S": S, "A": A, "seed": 1, "masked": False}
    picked = [0, 1, 63, 64, 20_000, M - 1]
    for r, run in _model_runs("hash", p, picked, rule, sched, 21, np.float32, "vec").items():
        history, at = run.run(K)
        _check(logged, res, r, run, history, at, {r: tables[r]}, K)


# ---- 6. train(): validation by episodes lets the draw counters drift apart --------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_train_with_episode_validation_matches_the_model_driven_the_same_way(rule):
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)  # every move may end the episode: greedy validation episodes end too
    M, S, A, seg, n_seg, val_episodes = M_ODD, mdp.state_size, mdp.action_size, 60, 3, 2
    sched = _schedules(M)
    pop = _population(M, S, A, sched, 8, np.float64, "iter", rule)
    out = pop.train(envs.TabularMDPEnv(M, mdp, seed=1), seg * n_seg, envs.TabularMDPEnv(M, mdp, seed=5), seg,
                    val_episodes=val_episodes)
    _reached_eval = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert _reached_eval["path"] == "population_eval", _reached_eval
    assert out.val_finished.all()
    tables = pop.q_tables
    counters = pop.step_counters
    assert len(set(counters.tolist())) > 1, "the validations must leave the runs at different counters"
    pt = {"mdp": mdp, "seed": 1}
    for r, run in _model_runs("table", pt, range(M), rule, sched, 8, np.float64, "iter").items():
        for k in range(n_seg):
            history, at = run.run(seg, reset=True)  # (train passes curr_state_dict=None: every segment resets)
            assert np.array_equal(out.segments[k].run_returns(r), history), (r, k)
            assert np.array_equal(out.segments[k].run_steps(r), at), (r, k)
            val = TableMDPVecEnv(1, mdp, seed=5, agent_offset=r)
            val.step_index = run.rt.step_counter  # the validation steps draw at the run's own counter
            total, _ = run.rt.evaluate_episodes(val, val_episodes)
            assert out.val_totals[k, r] == np.float32(total), (r, k)
        assert np.array_equal(tables[r], run.q), r
        assert counters[r] == run.rt.step_counter, r
        if rule == "sarsa":
            assert out.state_dict["pending_actions"][r] == run.pending == pop.pending_actions[r], r


def test_greedy_evaluation_neither_reads_nor_clears_the_pending_actions():
    envs = _product()[1]
    M, S, A = M_ODD, 50, 8
    pop = _population(M, S, A, _schedules(M), 0, np.float32, "iter", "sarsa")
    assert (pop.pending_actions == -1).all()
    pop.run_steps(40, envs.HashTabularEnv(M, S, A, seed=1))
    pending = pop.pending_actions
    assert (pending >= 0).all() and (pending < A).all()
    pop.evaluate_steps(envs.HashTabularEnv(M, S, A, seed=5), 30)
    pop.evaluate_episodes(envs.HashTabularEnv(M, S, A, seed=5), 1)
    assert np.array_equal(pop.pending_actions, pending)


# ---- 7. NaN and infinities in the tables; runs without a selectable action ---------------------------------------------
def _special_tables(M, S, A, dt, seed):
    """Random tables; run r gets r % 5 NaN cells, r % 3 cells of +inf and r % 4 of -inf and, for r % 13 == 12, a whole
    NaN row (the list selection has no candidate only on a row without a number)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((M, S, A)).astype(dt)
    for r in range(M):
        for count, value in ((r % 5, np.nan), (r % 3, np.inf), (r % 4, -np.inf)):
            q[r].ravel()[rng.choice(S * A, size=count, replace=False)] = value
        if r % 13 == 12:
            q[r, rng.integers(0, S)] = np.nan
    return q


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [
    (8, False, np.float32, "iter"),   # list selection: steps over NaN
    (8, True, np.float64, "vec"),     # list selection, masked
    (16, True, np.float32, "vec"),    # NumPy-style selection: a NaN in a valid column raises
])
@pytest.mark.parametrize("rule", RULES)
def test_nan_and_infinite_cells_match_the_model_and_stuck_runs_are_named(rule, A, masked, dt, mode):
    envs = _product()[1]
    M, S, K = M_ODD, 30, 150
    sched = _schedules(M)
    q0 = _special_tables(M, S, A, dt, seed=A)
    pop = _population(M, S, A, sched, 0, dt, mode, rule)
    pop.set_q_tables(q0)
    try:
        res, raised = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=masked)), []
    except IndexError as err:
        assert str(err).startswith("Cannot choose from an empty sequence (runs ")
        res, raised = err.result, err.runs
    _reached(pop, rule, nv=_nv(A), masked=masked)
    tables = pop.q_tables
    p = {"S": S, "A": A, "seed": 1, "masked": masked}
    want_raised, special_kept = [], 0
    for r, run in _model_runs("hash", p, range(M), rule, sched, 0, dt, mode, q0=q0).items():
        try:
            history, at = run.run(K)
        except IndexError:  # some pick of the run (its a or, SARSA, its a') had no candidate
            want_raised.append(r)
            continue
        special_kept += not np.isfinite(run.q).all()
        _check(pop, res, r, run, history, at, tables, K)
    assert raised == want_raised
    assert want_raised, "no run met a row without a selectable action"
    assert special_kept, "no run finished with a NaN or an infinity in its table"


# ---- 8. the default rule is untouched; arguments -----------------------------------------------------------------------
def test_q_learning_spelled_out_is_the_default_path():
    _lib, envs, _, QLearningPopulation = _product()
    variants = []
    for kw in ({}, {"update_rule": "q_learning"}):
        pop = QLearningPopulation(M_ODD, 100, 16, seed=2, dtype=np.float32, **kw)
        res = pop.run_steps(50, envs.HashTabularEnv(M_ODD, 100, 16, seed=1, masked=True))
        variants.append((pop.last_stats["kernel_variant"], pop.q_tables, pop.update_rule))
        assert "pending_actions" not in res.state_dict and (pop.pending_actions == -1).all()
    assert variants[0][0] == variants[1][0] == 6 | (4 << 12) | (1 << 20)
    assert np.array_equal(variants[0][1], variants[1][1]) and variants[0][2] == variants[1][2] == "q_learning"


def test_no_build_is_refused():
    """Every (dtype, width, masked) build of both rules compiles without scratch (tests/test_td_rules_host.py), so none
    answers QE_ERR_UNSUPPORTED: the widest one, fp64 with 64 masked actions, runs."""
    for rule in RULES:
        p = {"S": 50, "A": 64, "seed": 1, "masked": True}
        _run_and_check("hash", p, 50, 64, 8, 40, rule, np.float64, "iter", _schedules(8), nv=16, masked=True)


def test_arguments():
    import ctypes as C

    _lib, envs, _, QLearningPopulation = _product()
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase

    lib = _lib.load()
    algo = OptimalQLearningBase(10, 4, 0.9, seed=0)
    assert lib.qe_population_set_update_rule(algo.handle, _lib.RULE_SARSA) == _lib.ERR_INVALID
    assert "not a population engine" in lib.qe_last_error().decode()
    pop = QLearningPopulation(8, 50, 4, update_rule="sarsa")
    assert lib.qe_population_update_rule(pop.handle) == _lib.RULE_SARSA
    assert lib.qe_population_set_update_rule(pop.handle, 3) == _lib.ERR_INVALID
    assert "unknown update rule" in lib.qe_last_error().decode()
    assert lib.qe_population_update_rule(pop.handle) == _lib.RULE_SARSA
    with pytest.raises(ValueError):
        pop.pending_actions = np.zeros(7, dtype=np.int32)
    for bad in (4, -2):
        with pytest.raises(ValueError, match="outside"):
            pop.pending_actions = np.full(8, bad)
    pop.pending_actions = np.array([0, 1, 2, 3, -1, 0, 1, 2])
    assert pop.pending_actions.tolist() == [0, 1, 2, 3, -1, 0, 1, 2]
    pop.pending_actions = None
    assert (pop.pending_actions == -1).all()
    out = np.empty(8, dtype=np.int32)
    assert lib.qe_population_pending_actions(pop.handle, None) == _lib.ERR_INVALID
    assert lib.qe_population_pending_actions(algo.handle, _lib.ptr(out, C.c_int32)) == _lib.ERR_INVALID
    res = pop.run_steps(10, envs.HashTabularEnv(8, 50, 4))
    assert res.state_dict["pending_actions"].dtype == np.int32
