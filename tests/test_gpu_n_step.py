"""GPU: ``QLearningPopulation(update_rule="sarsa" | "expected_sarsa", n_step=n)`` (k_nstep_rollout) against the NumPy
model of the n-step rules (tests/n_step_model.py), bit for bit: per run the table, the episode returns and their steps,
the counts, the final observation / env word / running return, the pending action, the schedule values, the draw counter
and the window.  No tolerance anywhere.  Every case asserts the kernel build it means to cover (path 11, rule, NV, masked
and n).
"""
import copy
import pickle

import numpy as np
import pytest

from n_step_model import NStepRun
from test_gpu_population import _schedules
from test_gpu_td_rules import _check as _check_td
from test_gpu_td_rules import _device_env, _model_env, _nv, _product, _special_tables

pytestmark = pytest.mark.gpu

RULES = ["sarsa", "expected_sarsa"]
M_ODD = 67  # a full and a partial wavefront
NAN_CASE = {"M": M_ODD, "S": 30, "K": 150, "n": 3, "seed": 0, "env_seed": 1}


def _reached(pop, rule, n, nv=None, masked=None):
    d = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert pop.last_stats["kernel_variant"] & 15 == 11 and d["path"] == "population_nstep", d
    assert d["rule"] == rule == pop.update_rule and d["n_step"] == n == pop.n_step, d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _check(pop, res, r, run, history, at, tables, counter):
    """Run r of a population call against its model run (after the same call): the 1-step rules' list, and the window."""
    _check_td(pop, res, r, run, history, at, tables, counter)
    length, states, actions, rewards = run.window
    win = res.state_dict["n_step_window"]
    assert win["length"][r] == length, f"run {r}: window length"
    assert np.array_equal(win["states"][r], states), f"run {r}: window states"
    assert np.array_equal(win["actions"][r], actions), f"run {r}: window actions"
    assert np.array_equal(win["rewards"][r].view(np.uint32), rewards.view(np.uint32)), f"run {r}: window rewards"


def _model_runs(kind, p, runs, rule, n, sched, seed, dt, mode, q0=None):
    eps_s, lr_s, gamma = sched
    return {r: NStepRun(_model_env(kind, r, p), rule, gamma[r], eps_s[r], lr_s[r], n=n, seed=seed, dtype=dt, mode=mode,
                        agent_id=r, q0=None if q0 is None else q0[r]) for r in runs}


def _population(M, S, A, sched, seed, dt, mode, rule, n):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode,
                         update_rule=rule, n_step=n)


def _run_and_check(kind, p, S, A, M, K, rule, n, dt, mode, sched, seed=0, nv=None, masked=None):
    pop = _population(M, S, A, sched, seed, dt, mode, rule, n)
    res = pop.run_steps(K, _device_env(kind, M, p))
    _reached(pop, rule, n, nv=nv, masked=masked)
    tables = pop.q_tables
    for r, run in _model_runs(kind, p, range(M), rule, n, sched, seed, dt, mode).items():
        history, at = run.run(K)
        _check(pop, res, r, run, history, at, tables, K)
    win = res.state_dict["n_step_window"]
    assert win["length"].dtype == win["states"].dtype == win["actions"].dtype == np.int32 and win["rewards"].dtype == np.float32
    assert win["length"].shape == (M,) and win["states"].shape == win["actions"].shape == win["rewards"].shape == (M, n - 1)
    return pop, res


# ---- 1. every row width, both dtypes, both learn modes; the horizons -----------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [4, 8, 16, 64])
@pytest.mark.parametrize("rule", RULES)
def test_hash_runs_match_the_model(rule, A, masked, dt, mode):
    p = {"S": 300, "A": A, "seed": 1, "masked": masked}
    _run_and_check("hash", p, 300, A, M_ODD, 150, rule, 3, dt, mode, _schedules(M_ODD), nv=_nv(A), masked=masked)


@pytest.mark.parametrize(("n", "dt", "mode"), [(2, np.float32, "iter"), (2, np.float64, "vec"), (5, np.float32, "vec"),
                                               (5, np.float64, "iter"), (16, np.float32, "iter"), (16, np.float64, "vec")])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rule", RULES)
def test_the_horizons_match_the_model(rule, masked, n, dt, mode):
    p = {"S": 300, "A": 8, "seed": 1, "masked": masked}
    _, res = _run_and_check("hash", p, 300, 8, M_ODD, 150, rule, n, dt, mode, _schedules(M_ODD), nv=2, masked=masked)
    assert res.state_dict["n_step_window"]["length"].max() == n - 1


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("rule", RULES)
def test_the_32_column_build_matches_the_model(rule, dt):
    p = {"S": 200, "A": 20, "seed": 1, "masked": True}
    _run_and_check("hash", p, 200, 20, M_ODD, 150, rule, 3, dt, "iter", _schedules(M_ODD), nv=8, masked=True)


# ---- 2. the other environments ---------------------------------------------------------------------------------------
def _other(kind):
    """(S, A, parameters, NV, masked, n)"""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp
    from table_mdp_model import random_mdp

    if kind == "grid":
        return 36, 4, {"side": 6, "seed": 2}, 1, False, 3
    if kind == "bandit":  # steady updates and flushes, one state: every window repeats cells, every store lands in the held row
        return 1, 2, {"episode_len": 7}, 1, False, 3
    if kind == "bandit_mc":  # episodes shorter than the horizon: flush only, Monte Carlo
        return 1, 2, {"episode_len": 3}, 1, False, 5
    if kind == "tictactoe":
        return 19683, 9, {"seed": 5}, 4, True, 3
    arrays, isd, masks = random_mdp(20, 5, 3, seed=7, masked=True)
    return 20, 5, {"mdp": encode_table_mdp(*arrays, isd, masks), "seed": 3}, 2, True, 3


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["grid", "bandit", "bandit_mc", "tictactoe", "table"])
@pytest.mark.parametrize("rule", RULES)
def test_other_environments_match_the_model(rule, kind, dt, mode):
    S, A, p, nv, masked, n = _other(kind)
    _, res = _run_and_check(kind.split("_")[0], p, S, A, M_ODD, 150, rule, n, dt, mode, _schedules(M_ODD), seed=11, nv=nv,
                            masked=masked)
    if kind == "bandit_mc":
        assert res.state_dict["n_step_window"]["length"].max() == 0  # 150 steps = 50 whole episodes


# ---- 3. chaining: calls, a fresh process, calls shorter than the horizon --------------------------------------------
@pytest.mark.parametrize("S", [4, 400])  # four states: windows that repeat cells, s' == s_j at many call boundaries
@pytest.mark.parametrize("rule", RULES)
def test_calls_and_a_restored_population_equal_one_call(rule, S, tmp_path):
    envs = _product()[1]
    M, A, K, n = M_ODD, 8, 90, 4
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter", rule, n)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * K, env())
    halves = make()
    e = env()
    first = halves.run_steps(K, e)
    assert first.state_dict["n_step_window"]["length"].max() == n - 1, "the window must be non-empty at the cut"
    halves.save(tmp_path / "tables.npy")
    blob = pickle.dumps(first.state_dict)
    second = halves.run_steps(K, e, first.state_dict)
    restored = make()  # what a fresh process does: tables from the file, everything else from the pickled dict
    sd = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.restore_training_state(sd)
    for key, value in restored.n_step_window.items():
        assert np.array_equal(value, first.state_dict["n_step_window"][key]), key
    third = restored.run_steps(K, env(), sd)
    short = make()  # 60 calls of 3 steps: every call is shorter than the horizon
    e3, sd3, pieces = env(), None, []
    for _ in range(2 * K // 3):
        res3 = short.run_steps(3, e3, sd3) if sd3 is not None else short.run_steps(3, e3)
        sd3 = res3.state_dict
        pieces.append(res3)
    for pop in (whole, halves, restored, short):
        _reached(pop, rule, n, nv=2, masked=True)
        assert np.array_equal(pop.q_tables, whole.q_tables)
        assert np.array_equal(pop.step_counters, np.full(M, 2 * K))

    def same_state(a, b):
        assert sorted(a) == sorted(b)
        for key in b:
            if isinstance(b[key], np.ndarray):
                assert np.array_equal(a[key], b[key]), key
            elif isinstance(b[key], dict):
                for k2 in b[key]:
                    assert np.array_equal(a[key][k2], b[key][k2]), (key, k2)

    for tail in (second, third):
        for r in range(M):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), one.run_returns(r)), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + K]), one.run_steps(r)), r
        same_state(tail.state_dict, one.state_dict)
    same_state(sd3, one.state_dict)
    for r in range(M):
        assert np.array_equal(np.concatenate([x.run_returns(r) for x in pieces]), one.run_returns(r)), r
        assert np.array_equal(np.concatenate([x.run_steps(r) + 3 * i for i, x in enumerate(pieces)]), one.run_steps(r)), r
    # a dict without the key: every window starts empty, its entries are never updated (the model, told so)
    lost = make()
    lost.load(tmp_path / "tables.npy")
    stripped = {k: v for k, v in sd.items() if k != "n_step_window"}
    lost.restore_training_state(stripped)
    assert (lost.n_step_window["length"] == 0).all()
    res = lost.run_steps(K, env(), stripped)
    tables = lost.q_tables
    assert not np.array_equal(tables, whole.q_tables)
    p = {"S": S, "A": A, "seed": 9, "masked": True}
    for r, run in _model_runs("hash", p, range(M), rule, n, sched, 4, np.float32, "iter").items():
        run.run(K)
        run.rt.window.clear()
        history, at = run.run(K)
        _check(lost, res, r, run, history, at, tables, 2 * K)


# ---- 4. launch chopping ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_and_the_model(rule):
    envs = _product()[1]
    M, K, S, A, n = 40_000, 2000, 100, 8, 3
    eps0, lr0, gamma0 = _schedules(97)
    sched = [[x[r % 97] for r in range(M)] for x in (eps0, lr0, gamma0)]
    logged = _population(M, S, A, sched, 21, np.float32, "vec", rule, n)
    res = logged.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1))
    _reached(logged, rule, n, nv=2, masked=False)
    assert logged.last_stats["launches"] > 9, "the logged call must be cut into more than three launches"
    tables = logged.q_tables
    quiet = _population(M, S, A, sched, 21, np.float32, "vec", rule, n)
    res_q = quiet.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1), log=False)
    assert 1 < quiet.last_stats["launches"] < logged.last_stats["launches"] // 3, "the unlogged call is cut differently"
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    assert sorted(res_q.state_dict) == sorted(res.state_dict)
    for key, value in res.state_dict.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(res_q.state_dict[key], value), key
    for key, value in res.state_dict["n_step_window"].items():
        assert np.array_equal(res_q.state_dict["n_step_window"][key], value), key
    del quiet
    p = {"S": S, "A": A, "seed": 1, "masked": False}
    picked = [0, 1, 63, 64, 20_000, M - 1]
    for r, run in _model_runs("hash", p, picked, rule, n, sched, 21, np.float32, "vec").items():
        history, at = run.run(K)
        _check(logged, res, r, run, history, at, {r: tables[r]}, K)


# ---- 5. train(): every segment resets and drops its window; validation by episodes lets the counters drift apart -------
@pytest.mark.parametrize("rule", RULES)
def test_train_with_episode_validation_matches_the_model_driven_the_same_way(rule):
    from table_mdp_model import TableMDPVecEnv
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)  # every move may end the episode: greedy validation episodes end too
    M, S, A, seg, n_seg, val_episodes, n = M_ODD, mdp.state_size, mdp.action_size, 60, 3, 2, 3
    sched = _schedules(M)
    pop = _population(M, S, A, sched, 8, np.float64, "iter", rule, n)
    out = pop.train(envs.TabularMDPEnv(M, mdp, seed=1), seg * n_seg, envs.TabularMDPEnv(M, mdp, seed=5), seg,
                    val_episodes=val_episodes)
    assert _product()[0].decode_variant(pop.last_stats["kernel_variant"])["path"] == "population_eval"
    assert out.val_finished.all()
    tables = pop.q_tables
    counters = pop.step_counters
    assert len(set(counters.tolist())) > 1, "the validations must leave the runs at different counters"
    pt = {"mdp": mdp, "seed": 1}
    dropped = 0
    window = pop.n_step_window  # greedy evaluation neither reads nor clears it
    for r, run in _model_runs("table", pt, range(M), rule, n, sched, 8, np.float64, "iter").items():
        for k in range(n_seg):
            dropped += k > 0 and len(run.rt.window) > 0
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
        length, states, actions, rewards = run.window
        for win in (window, out.state_dict["n_step_window"]):
            assert win["length"][r] == length and np.array_equal(win["states"][r], states), r
            assert np.array_equal(win["actions"][r], actions) and np.array_equal(win["rewards"][r], rewards), r
    assert dropped, "no segment started over a non-empty window"


# ---- 6. NaN and infinities in the tables; runs without a selectable action ---------------------------------------------
def nan_case_model(rule, A, masked, dt, mode, check=None):
    """The model's side of the case below: the runs whose pick finds no candidate, and how many of the others end with a
    non-finite cell.  ``check(r, run, history, at)`` is called for every run that is compared."""
    c = NAN_CASE
    sched = _schedules(c["M"])
    q0 = _special_tables(c["M"], c["S"], A, dt, seed=A)
    p = {"S": c["S"], "A": A, "seed": c["env_seed"], "masked": masked}
    raised, special_kept = [], 0
    for r, run in _model_runs("hash", p, range(c["M"]), rule, c["n"], sched, c["seed"], dt, mode, q0=q0).items():
        try:
            history, at = run.run(c["K"])
        except IndexError:  # some pick of the run (its a or, SARSA, its a') had no candidate
            raised.append(r)
            continue
        special_kept += not np.isfinite(run.q).all()
        if check is not None:
            check(r, run, history, at)
    return raised, special_kept


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [
    (8, False, np.float32, "iter"),   # list selection: steps over NaN
    (8, True, np.float64, "vec"),     # list selection, masked
    (16, True, np.float32, "vec"),    # NumPy-style selection: a NaN in a valid column raises
])
@pytest.mark.parametrize("rule", RULES)
def test_nan_and_infinite_cells_match_the_model_and_stuck_runs_are_named(rule, A, masked, dt, mode):
    envs = _product()[1]
    c = NAN_CASE
    M, S, K, n = c["M"], c["S"], c["K"], c["n"]
    q0 = _special_tables(M, S, A, dt, seed=A)
    pop = _population(M, S, A, _schedules(M), c["seed"], dt, mode, rule, n)
    pop.set_q_tables(q0)
    try:
        res, raised = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=c["env_seed"], masked=masked)), []
    except IndexError as err:
        assert str(err).startswith("Cannot choose from an empty sequence (runs ")
        res, raised = err.result, err.runs
    _reached(pop, rule, n, nv=_nv(A), masked=masked)
    tables = pop.q_tables
    want_raised, special_kept = nan_case_model(
        rule, A, masked, dt, mode, check=lambda r, run, history, at: _check(pop, res, r, run, history, at, tables, K))
    assert raised == want_raised
    assert want_raised, "no run met a row without a selectable action"
    assert special_kept, "no run finished with a NaN or an infinity in its table"


# ---- 7. the widest build -----------------------------------------------------------------------------------------------
def test_no_build_is_refused():
    """Every (dtype, width, masked) build of both rules compiles without scratch (tests/test_n_step_host.py), so none
    answers QE_ERR_UNSUPPORTED: the widest one, fp64 with 64 masked actions, runs at the longest horizon."""
    for rule in RULES:
        p = {"S": 50, "A": 64, "seed": 1, "masked": True}
        _run_and_check("hash", p, 50, 64, 8, 40, rule, 16, np.float64, "iter", _schedules(8), nv=16, masked=True)


# ---- 8. n_step = 1 is untouched; refusals ------------------------------------------------------------------------------
@pytest.mark.parametrize(("rule", "variant"), [("q_learning", 6), ("sarsa", 8 | (1 << 4)), ("expected_sarsa", 8 | (2 << 4))])
def test_one_step_spelled_out_is_the_default_path(rule, variant):
    _, envs, _, QLearningPopulation = _product()
    got = []
    for kw in ({}, {"n_step": 1}):
        pop = QLearningPopulation(M_ODD, 100, 16, seed=2, dtype=np.float32, update_rule=rule, **kw)
        res = pop.run_steps(50, envs.HashTabularEnv(M_ODD, 100, 16, seed=1, masked=True))
        got.append((pop.last_stats["kernel_variant"], pop.q_tables, sorted(res.state_dict)))
        assert "n_step_window" not in res.state_dict and pop.n_step_window is None and pop.n_step == 1
    assert got[0][0] == got[1][0] == variant | (4 << 12) | (1 << 20)
    assert np.array_equal(got[0][1], got[1][1]) and got[0][1].any() and got[0][2] == got[1][2]


def test_refusals_and_arguments():
    import ctypes as C

    _lib, envs, _, QLearningPopulation = _product()
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase

    lib = _lib.load()
    i32 = lambda a: _lib.ptr(a, C.c_int32)  # noqa: E731
    algo = OptimalQLearningBase(10, 4, 0.9, seed=0)
    assert lib.qe_population_set_n_step(algo.handle, 2) == _lib.ERR_INVALID
    assert "not a population engine" in lib.qe_last_error().decode()
    assert lib.qe_population_n_step(algo.handle) == _lib.ERR_INVALID
    # Python: before anything is allocated
    for kw, text in (({"update_rule": "q_learning"}, "not an off-policy method"), ({}, "not an off-policy method"),
                     ({"double_q": True}, "double estimator is a one-step method")):
        with pytest.raises(ValueError, match=f"n_step=2 .*{text}"):
            QLearningPopulation(8, 50, 4, n_step=2, **kw)
    # C: n > 1 on Q-learning, on the double estimator; either of those while n > 1
    ql = QLearningPopulation(8, 50, 4)
    assert lib.qe_population_n_step(ql.handle) == 1
    assert lib.qe_population_set_n_step(ql.handle, 2) == _lib.ERR_UNSUPPORTED
    assert "uncorrected n-step Q-learning is not an off-policy method" in lib.qe_last_error().decode()
    assert lib.qe_population_set_n_step(ql.handle, 1) == 0 and lib.qe_population_n_step(ql.handle) == 1
    for bad in (0, -1, 17):
        assert lib.qe_population_set_n_step(ql.handle, bad) == _lib.ERR_INVALID
        assert "n_step must be in 1 .. 16" in lib.qe_last_error().decode()
    dq = QLearningPopulation(8, 50, 4, double_q=True)
    assert lib.qe_population_set_n_step(dq.handle, 3) == _lib.ERR_UNSUPPORTED
    pop = QLearningPopulation(8, 50, 4, update_rule="sarsa", n_step=3)
    assert lib.qe_population_n_step(pop.handle) == 3
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_Q_LEARNING) == _lib.ERR_UNSUPPORTED
    assert "uncorrected n-step Q-learning is not an off-policy method" in lib.qe_last_error().decode()
    assert lib.qe_population_set_double(pop.handle, 1) == _lib.ERR_UNSUPPORTED
    assert "the double estimator is a one-step method" in lib.qe_last_error().decode()
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_EXPECTED_SARSA) == 0
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_SARSA) == 0
    assert lib.qe_population_update_rule(pop.handle) == _lib.RULE_SARSA and lib.qe_population_n_step(pop.handle) == 3
    # the window's setter: shapes, lengths, states and actions
    win = pop.n_step_window
    assert (win["length"] == 0).all() and win["states"].shape == (8, 2)
    good = {"length": np.array([0, 1, 2, 0, 1, 2, 0, 1]), "states": np.arange(16).reshape(8, 2) % 50,
            "actions": np.arange(16).reshape(8, 2) % 4, "rewards": np.linspace(-1, 1, 16).reshape(8, 2)}
    pop.n_step_window = good
    back = pop.n_step_window
    used = np.arange(2)[None, :] < good["length"][:, None]
    assert np.array_equal(back["length"], good["length"])
    for key in ("states", "actions", "rewards"):
        assert np.array_equal(back[key], np.where(used, good[key], 0).astype(back[key].dtype)), key
    for key, value, text in (("length", np.full(8, 3), "length 3 is outside"), ("length", np.full(8, -1), "length -1"),
                             ("states", np.full((8, 2), 50), "state 50 is outside"),
                             ("actions", np.full((8, 2), 4), "action 4 is outside"),
                             ("actions", np.full((8, 2), -1), "action -1 is outside")):
        bad = dict(good, **{key: value})
        if key != "length":
            bad["length"] = np.full(8, 2)
        with pytest.raises(ValueError, match=text):
            pop.n_step_window = bad
    for bad in (dict(good, states=np.zeros((8, 3), dtype=np.int32)), dict(good, length=np.zeros(7, dtype=np.int32)),
                dict(good, rewards=np.zeros((8, 2), dtype=complex)), {"length": good["length"]}, [1, 2]):
        with pytest.raises(ValueError, match="n_step_window"):
            pop.n_step_window = bad
    assert np.array_equal(pop.n_step_window["length"], good["length"])  # a refused window changes nothing
    length = np.zeros(8, dtype=np.int32)
    assert lib.qe_population_window(pop.handle, None, None, None, None) == _lib.ERR_INVALID
    assert lib.qe_population_window(pop.handle, i32(length), None, None, None) == 0 and np.array_equal(length, good["length"])
    assert lib.qe_population_set_window(pop.handle, i32(length), None, None, None) == _lib.ERR_INVALID
    pop.n_step_window = None
    assert (pop.n_step_window["length"] == 0).all()
    res = pop.run_steps(10, envs.HashTabularEnv(8, 50, 4))
    assert res.state_dict["n_step_window"]["length"].max() == 2
    # greedy evaluation neither reads nor clears the window
    before = pop.n_step_window
    pop.evaluate_steps(envs.HashTabularEnv(8, 50, 4, seed=5), 30)
    pop.evaluate_episodes(envs.HashTabularEnv(8, 50, 4, seed=5), 1)
    for key, value in pop.n_step_window.items():
        assert np.array_equal(value, before[key]), key
    # setting the horizon empties the windows
    assert lib.qe_population_set_n_step(pop.handle, 5) == 0 and lib.qe_population_n_step(pop.handle) == 5
    assert lib.qe_population_window(pop.handle, i32(length), None, None, None) == 0 and (length == 0).all()


def test_the_window_calls_at_horizon_one():
    """n_step = 1 has no window: the getter writes nothing, the setter takes only "every window empty"."""
    import ctypes as C

    _lib, _, _, QLearningPopulation = _product()
    lib = _lib.load()
    i32 = lambda a: _lib.ptr(a, C.c_int32)  # noqa: E731
    pop = QLearningPopulation(8, 50, 4, update_rule="sarsa", n_step=1)
    length = np.full(8, 7, dtype=np.int32)
    assert lib.qe_population_window(pop.handle, i32(length), None, None, None) == 0 and (length == 7).all()
    assert lib.qe_population_window(pop.handle, None, None, None, None) == 0
    assert lib.qe_population_set_window(pop.handle, None, None, None, None) == 0
    assert lib.qe_population_set_window(pop.handle, i32(np.zeros(8, dtype=np.int32)), None, None, None) == 0
    one = np.array([0, 1, 0, 0, 0, 0, 0, 0], dtype=np.int32)
    assert lib.qe_population_set_window(pop.handle, i32(one), None, None, None) == _lib.ERR_INVALID
    assert "window of run 1: length 1 with n_step = 1" in lib.qe_last_error().decode()
    assert lib.qe_population_n_step(pop.handle) == 1 and pop.n_step_window is None
