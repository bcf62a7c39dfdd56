"""GPU: ``QLearningPopulation(planning_steps=n)`` (k_dyna_rollout) against the NumPy model of Dyna-Q
(tests/dyna_model.py), bit for bit.

Per run: the table, the episode returns and their steps, the counts, the final observation / env word / running return,
the schedule values, the draw counter and the whole ``planning_model`` (next states, rewards, flags, the visited list and
its count).  No tolerance anywhere.  Every case asserts the kernel build it means to cover (path 13, NV, masked and n).
"""
import copy
import pickle

import numpy as np
import pytest

from dyna_model import DynaRun
from test_gpu_population import _schedules
from test_gpu_td_rules import _check as _check_td
from test_gpu_td_rules import _device_env, _model_env, _nv, _product, _special_tables

pytestmark = pytest.mark.gpu

M_ODD = 67  # a full and a partial wavefront


def _reached(pop, n, nv=None, masked=None):
    d = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert pop.last_stats["kernel_variant"] & 15 == 13 and d["path"] == "population_dyna", d
    assert d["planning_steps"] == n == pop.planning_steps and d["rule"] == "q_learning" == pop.update_rule, d
    assert d["n_step"] == 1 and d["trace_length"] == 0, d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _check_model(model, r, run):
    nxt, rew, term, visited, count = run.planning_model
    assert model["count"][r] == count, f"run {r}: count"
    assert np.array_equal(model["visited"][r], visited), f"run {r}: visited list"
    assert np.array_equal(model["next_states"][r], nxt), f"run {r}: next states"
    assert np.array_equal(model["rewards"][r].view(np.uint32), rew.view(np.uint32)), f"run {r}: rewards"
    assert np.array_equal(model["terminated"][r], term), f"run {r}: terminated"


def _check(pop, res, r, run, history, at, tables, counter, model):
    """Run r of a population call against its model run (after the same call): Q-learning's list, and the model."""
    _check_td(pop, res, r, run, history, at, tables, counter)
    _check_model(model, r, run)


def _model_runs(kind, p, runs, n, sched, seed, dt, mode, q0=None, offset=0):
    eps_s, lr_s, gamma = sched
    return {r: DynaRun(_model_env(kind, r + offset, p), gamma[r], eps_s[r], lr_s[r], n=n, seed=seed, dtype=dt, mode=mode,
                       agent_id=r + offset, q0=None if q0 is None else q0[r]) for r in runs}


def _population(M, S, A, sched, seed, dt, mode, **kw):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode, **kw)


def _model_shapes(pop, model):
    M, S, A = pop.runs, pop.state_size, pop.action_size
    assert sorted(model) == ["count", "next_states", "rewards", "terminated", "visited"]
    assert model["next_states"].dtype == model["visited"].dtype == model["count"].dtype == np.int32
    assert model["rewards"].dtype == np.float32 and model["terminated"].dtype == bool
    assert model["next_states"].shape == model["rewards"].shape == model["terminated"].shape == (M, S, A)
    assert model["visited"].shape == (M, S * A) and model["count"].shape == (M,)
    unseen = model["next_states"] < 0
    assert (model["next_states"][unseen] == -1).all() and not model["rewards"][unseen].any() and not model["terminated"][unseen].any()
    assert np.array_equal((~unseen).sum(axis=(1, 2)), model["count"])
    assert np.array_equal((model["visited"] >= 0).sum(axis=1), model["count"])


def _run_and_check(kind, p, S, A, M, steps, n, dt, mode, sched, seed=0, nv=None, masked=None):
    pop = _population(M, S, A, sched, seed, dt, mode, planning_steps=n)
    res = pop.run_steps(steps, _device_env(kind, M, p))
    _reached(pop, n, nv=nv, masked=masked)
    assert "planning_model" not in res.state_dict
    tables, model = pop.q_tables, pop.planning_model
    _model_shapes(pop, model)
    for r, run in _model_runs(kind, p, range(M), n, sched, seed, dt, mode).items():
        history, at = run.run(steps)
        _check(pop, res, r, run, history, at, tables, steps, model)
    return pop, res, model


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for key in b:
        if isinstance(b[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


def _same_model(a, b):
    for key in b:
        assert np.array_equal(a[key], b[key]), key


# ---- 1. every row width, masked and not, both dtypes, both learn modes ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [4, 8, 16, 32, 64])
def test_hash_runs_match_the_model(A, masked, dt, mode):
    p = {"S": 100, "A": A, "seed": 1, "masked": masked}
    _run_and_check("hash", p, 100, A, M_ODD, 150, 4, dt, mode, _schedules(M_ODD), nv=_nv(A), masked=masked)


# ---- 2. planning counts: one word, a full block, a second block, the maximum ---------------------------------------------------
@pytest.mark.parametrize(("n", "steps", "dt", "mode"), [(1, 150, np.float32, "iter"), (4, 150, np.float64, "vec"),
                                                        (5, 150, np.float32, "vec"), (5, 150, np.float64, "iter"),
                                                        (64, 20, np.float32, "iter"), (64, 20, np.float64, "vec")])
def test_planning_counts_match_the_model(n, steps, dt, mode):
    """(n = 64: 20 steps, 1 300 table updates per run -- the model is what takes the time.)"""
    p = {"S": 100, "A": 8, "seed": 1, "masked": True}
    _run_and_check("hash", p, 100, 8, M_ODD, steps, n, dt, mode, _schedules(M_ODD), nv=2, masked=True)


# ---- 3. planning stores into the row held in registers --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize(("A", "masked"), [(4, False), (16, True)])
def test_four_states_collide_with_the_held_row(A, masked, dt, mode):
    p = {"S": 4, "A": A, "seed": 1, "masked": masked}
    _, _, model = _run_and_check("hash", p, 4, A, M_ODD, 150, 5, dt, mode, _schedules(M_ODD), nv=_nv(A), masked=masked)
    assert (model["count"] > 4).all()


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_on_the_bandit_every_planning_store_lands_in_the_held_row(dt, mode):
    p = {"episode_len": 50}
    _, _, model = _run_and_check("bandit", p, 1, 2, M_ODD, 140, 3, dt, mode, _schedules(M_ODD), seed=11, nv=1, masked=False)
    assert (model["count"] == 2).any() and (model["next_states"][model["next_states"] >= 0] == 0).all()


# ---- 4. other environments ----------------------------------------------------------------------------------------------------
def _other(kind):
    """(S, A, parameters, NV, masked)"""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp
    from table_mdp_model import random_mdp

    if kind == "grid":
        return 36, 4, {"side": 6, "seed": 2}, 1, False
    if kind == "tictactoe":  # the masks of remembered next states
        return 19683, 9, {"seed": 5}, 4, True
    arrays, isd, masks = random_mdp(20, 5, 3, seed=7, masked=True)  # three outcomes per cell: outcomes are overwritten
    return 20, 5, {"mdp": encode_table_mdp(*arrays, isd, masks), "seed": 3}, 2, True


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["grid", "tictactoe", "table"])
def test_other_environments_match_the_model(kind, dt, mode):
    S, A, p, nv, masked = _other(kind)
    steps = 60 if kind == "tictactoe" else 150  # (the model copes slowly with 19 683 x 9 cells per run)
    _, res, model = _run_and_check(kind, p, S, A, M_ODD, steps, 4, dt, mode, _schedules(M_ODD), seed=11, nv=nv, masked=masked)
    assert res.episode_counts.sum() > 0
    if kind == "table":
        assert (model["count"] < steps).all(), "no cell was observed twice: nothing was overwritten"


# ---- 5. NaN and infinities in the tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [(8, False, np.float32, "iter"), (8, True, np.float64, "vec"),
                                                         (16, True, np.float32, "vec")])
def test_nan_and_infinite_cells_match_the_model(A, masked, dt, mode):
    envs = _product()[1]
    M, S, K, n = M_ODD, 30, 100, 4
    sched = _schedules(M)
    q0 = _special_tables(M, S, A, dt, seed=A)
    pop = _population(M, S, A, sched, 0, dt, mode, planning_steps=n)
    pop.set_q_tables(q0)
    try:
        res, raised = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=masked)), []
    except IndexError as err:
        res, raised = err.result, err.runs
    _reached(pop, n, nv=_nv(A), masked=masked)
    tables, model = pop.q_tables, pop.planning_model
    p = {"S": S, "A": A, "seed": 1, "masked": masked}
    want_raised, special_kept = [], 0
    for r, run in _model_runs("hash", p, range(M), n, sched, 0, dt, mode, q0=q0).items():
        try:
            history, at = run.run(K)
        except IndexError:  # (a run without a selectable action is on its own from there on)
            want_raised.append(r)
            continue
        special_kept += not np.isfinite(run.q).all()
        _check(pop, res, r, run, history, at, tables, K, model)
    assert raised == want_raised
    assert len(want_raised) < M and special_kept, "no compared run finished with a NaN or an infinity in its table"


# ---- 6. a non-zero agent offset --------------------------------------------------------------------------------------------------
def test_a_population_at_an_agent_offset_matches_the_model():
    envs = _product()[1]
    M, S, A, steps, n, off = M_ODD, 50, 8, 100, 4, 1000
    sched = _schedules(M)
    pop = _population(M, S, A, sched, 3, np.float32, "iter", planning_steps=n)
    res = pop.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1, masked=True, agent_offset=off))
    _reached(pop, n, nv=2, masked=True)
    tables, model = pop.q_tables, pop.planning_model
    p = {"S": S, "A": A, "seed": 1, "masked": True}
    for r, run in _model_runs("hash", p, range(M), n, sched, 3, np.float32, "iter", offset=off).items():
        history, at = run.run(steps)
        _check(pop, res, r, run, history, at, tables, steps, model)


# ---- 7. chaining and resume ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 400])
def test_calls_and_a_restored_population_equal_one_call(S, tmp_path):
    envs = _product()[1]
    M, A, steps, n = M_ODD, 8, 90, 5
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter", planning_steps=n)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * steps, env())
    halves = make()
    e = env()
    first = halves.run_steps(steps, e)
    assert "planning_model" not in first.state_dict
    at_cut = halves.planning_model
    assert (at_cut["count"] > 0).all()
    halves.save(tmp_path / "tables.npy")
    halves.save_model(tmp_path / "model.npz")
    blob = pickle.dumps(first.state_dict)
    second = halves.run_steps(steps, e, first.state_dict)
    restored = make()  # what a fresh process does: tables and model from their files, the rest from the pickled dict
    sd = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.load_model(tmp_path / "model.npz")
    restored.restore_training_state(sd)
    _same_model(restored.planning_model, at_cut)
    third = restored.run_steps(steps, env(), sd)
    for pop in (whole, halves, restored):
        _reached(pop, n, nv=2, masked=True)
        assert np.array_equal(pop.q_tables, whole.q_tables)
        assert np.array_equal(pop.step_counters, np.full(M, 2 * steps))
        _same_model(pop.planning_model, whole.planning_model)
    for tail in (second, third):
        for r in range(M):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), one.run_returns(r)), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + steps]), one.run_steps(r)), r
        _same_state(tail.state_dict, one.state_dict)
    # the model survives a reset of the environment (curr_state_dict=None): a second call from the start state
    again = make()
    again.run_steps(steps, env())
    kept = again.planning_model
    res = again.run_steps(0, env())
    _same_model(again.planning_model, kept)
    assert res.state_dict["rng_step"] == steps


def test_forgetting_the_model_midway_equals_a_model_run_cleared_at_the_same_point():
    envs = _product()[1]
    M, S, A, steps, n = M_ODD, 30, 8, 70, 4
    sched = _schedules(M)
    pop = _population(M, S, A, sched, 6, np.float64, "vec", planning_steps=n)
    e = envs.HashTabularEnv(M, S, A, seed=2, masked=False)
    first = pop.run_steps(steps, e)
    assert pop.planning_model["count"].all()
    pop.planning_model = None
    empty = pop.planning_model
    assert not empty["count"].any() and (empty["next_states"] == -1).all() and (empty["visited"] == -1).all()
    res = pop.run_steps(steps, e, first.state_dict)
    _reached(pop, n, nv=2, masked=False)
    tables, model = pop.q_tables, pop.planning_model
    p = {"S": S, "A": A, "seed": 2, "masked": False}
    for r, run in _model_runs("hash", p, range(M), n, sched, 6, np.float64, "vec").items():
        run.run(steps)
        run.rt.forget()
        history, at = run.run(steps)
        _check(pop, res, r, run, history, at, tables, 2 * steps, model)


def test_the_model_setter_and_the_refusals_on_a_live_engine():
    _lib, envs, _, QLearningPopulation = _product()
    lib = _lib.load()
    M, S, A = 8, 20, 4
    plain = QLearningPopulation(M, S, A)
    assert plain.planning_model is None and plain.planning_steps == 0 and lib.qe_population_planning(plain.handle) == 0
    assert lib.qe_population_model(plain.handle, None, None, None, None, None) == _lib.ERR_INVALID
    assert "planning is off" in lib.qe_last_error().decode()
    assert lib.qe_population_set_model(plain.handle, None, None, None, None, None) == _lib.ERR_INVALID
    with pytest.raises(ValueError, match="has no planning model"):
        plain.planning_model = {}
    with pytest.raises(ValueError, match="has no planning model"):
        plain.save_model("unused.npz")
    for bad in (-1, 65):
        assert lib.qe_population_set_planning(plain.handle, bad) == _lib.ERR_INVALID
    for kw in ({"update_rule": "sarsa"}, {"update_rule": "expected_sarsa"}, {"double_q": True}, {"update_rule": "sarsa", "n_step": 3},
               {"trace_decay": 0.5}):
        other = QLearningPopulation(M, S, A, **kw)
        assert lib.qe_population_set_planning(other.handle, 4) == _lib.ERR_UNSUPPORTED, kw
        assert lib.qe_population_planning(other.handle) == 0
    pop = QLearningPopulation(M, S, A, planning_steps=3, dtype=np.float32)
    assert lib.qe_population_planning(pop.handle) == 3
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_SARSA) == _lib.ERR_UNSUPPORTED
    assert "planning is on" in lib.qe_last_error().decode()
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_EXPECTED_SARSA) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_double(pop.handle, 1) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_n_step(pop.handle, 2) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_traces(pop.handle, 4, 0, _lib.ptr(np.full(M, 0.5), __import__("ctypes").c_double)) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_Q_LEARNING) == 0 and lib.qe_population_n_step(pop.handle) == 1
    pop.run_steps(40, envs.HashTabularEnv(M, S, A))
    good = pop.planning_model
    assert good["count"].all()
    pop.planning_model = None
    pop.planning_model = good
    _same_model(pop.planning_model, good)
    r, c0 = 5, int(good["visited"][5, 0])
    unseen = int(np.flatnonzero(good["next_states"][r].ravel() < 0)[0])

    def changed(key, index, value):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][index] = value
        return bad

    for bad, text in ((changed("visited", (r, 0), unseen), "is unseen in the model"),
                      (changed("visited", (r, 1), c0), "is listed twice"),
                      (changed("visited", (r, 0), S * A), "is outside"), (changed("visited", (r, 0), -1), "is outside"),
                      (changed("count", r, good["count"][r] - 1), "count is"), (changed("count", r, good["count"][r] + 1), "count is"),
                      (changed("next_states", (r, c0 // A, c0 % A), S), "next state 20 is outside"),
                      (changed("next_states", (r, c0 // A, c0 % A), -2), "next state -2"),
                      (changed("next_states", (r, unseen // A, unseen % A), 0), "count is")):
        with pytest.raises(ValueError, match=text):
            pop.planning_model = bad
    _same_model(pop.planning_model, good)  # a refused model changes nothing
    # planning_steps changed on a live engine keeps the model; 0 forgets it and gives the one-step kernel back
    assert lib.qe_population_set_planning(pop.handle, 7) == 0 and lib.qe_population_planning(pop.handle) == 7
    _same_model(pop.planning_model, good)
    assert lib.qe_population_set_planning(pop.handle, 0) == 0
    assert lib.qe_population_model(pop.handle, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.qe_population_set_n_step(pop.handle, 1) == 0 and lib.qe_population_set_double(pop.handle, 1) == 0


# ---- 8. launch cutting --------------------------------------------------------------------------------------------------------
def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_and_the_model():
    envs = _product()[1]
    M, steps, S, A, n = 20_000, 2000, 50, 8, 1
    eps0, lr0, gamma0 = _schedules(97)
    sched = [[x[r % 97] for r in range(M)] for x in (eps0, lr0, gamma0)]
    logged = _population(M, S, A, sched, 21, np.float32, "vec", planning_steps=n)
    res = logged.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1))
    _reached(logged, n, nv=2, masked=False)
    # 2^23 log entries / 20 000 runs = 419 steps per launch: 5 launches, each with its scan and its pack
    assert logged.last_stats["launches"] == 15
    tables, model = logged.q_tables, logged.planning_model
    quiet = _population(M, S, A, sched, 21, np.float32, "vec", planning_steps=n)
    res_q = quiet.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1), log=False)
    # 2^25 table updates / 20 000 runs / (1 + n) = 838 steps per launch; without planning the call would take 2 launches
    assert quiet.last_stats["launches"] == 3
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    _same_state(res_q.state_dict, res.state_dict)
    _same_model(quiet.planning_model, model)
    del quiet
    p = {"S": S, "A": A, "seed": 1, "masked": False}
    picked = [0, 1, 63, 64, 10_000, M - 1]
    for r, run in _model_runs("hash", p, picked, n, sched, 21, np.float32, "vec").items():
        history, at = run.run(steps)
        _check(logged, res, r, run, history, at, {r: tables[r]}, steps, model)


# ---- 9. evaluation and train() ---------------------------------------------------------------------------------------------------
def test_evaluation_between_training_calls_leaves_the_model_and_the_training_alone():
    envs = _product()[1]
    M, S, A, n = M_ODD, 50, 8, 4
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 6, np.float64, "iter", planning_steps=n)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=2, masked=True)

    straight, e1 = make(), env()
    a1 = straight.run_steps(70, e1)
    a2 = straight.run_steps(70, e1, a1.state_dict)
    paused, e2 = make(), env()
    b1 = paused.run_steps(70, e2)
    before = paused.planning_model
    paused.evaluate_steps(envs.HashTabularEnv(M, S, A, seed=5, masked=True), 40)
    assert _product()[0].decode_variant(paused.last_stats["kernel_variant"])["path"] == "population_eval"
    paused.evaluate_episodes(envs.HashTabularEnv(M, S, A, seed=5, masked=True), 1)
    _same_model(paused.planning_model, before)
    paused.step_counter = 70  # (the evaluations drew steps of their own: back to where training stood)
    b2 = paused.run_steps(70, e2, b1.state_dict)
    assert np.array_equal(paused.q_tables, straight.q_tables)
    _same_state(b2.state_dict, a2.state_dict)
    _same_model(paused.planning_model, straight.planning_model)
    for r in range(M):
        assert np.array_equal(b2.run_returns(r), a2.run_returns(r)), r


def test_train_with_episode_validation_matches_the_model_driven_the_same_way():
    from table_mdp_model import TableMDPVecEnv
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)  # every move may end the episode: greedy validation episodes end too
    M, S, A, seg, n_seg, val_episodes, n = M_ODD, mdp.state_size, mdp.action_size, 60, 3, 2, 4
    sched = _schedules(M)
    pop = _population(M, S, A, sched, 8, np.float64, "iter", planning_steps=n)
    out = pop.train(envs.TabularMDPEnv(M, mdp, seed=1), seg * n_seg, envs.TabularMDPEnv(M, mdp, seed=5), seg,
                    val_episodes=val_episodes)
    assert _product()[0].decode_variant(pop.last_stats["kernel_variant"])["path"] == "population_eval"
    assert out.val_finished.all()
    tables, model, counters = pop.q_tables, pop.planning_model, pop.step_counters
    assert len(set(counters.tolist())) > 1, "the validations must leave the runs at different counters"
    assert "planning_model" not in out.state_dict
    pt = {"mdp": mdp, "seed": 1}
    for r, run in _model_runs("table", pt, range(M), n, sched, 8, np.float64, "iter").items():
        for k in range(n_seg):
            history, at = run.run(seg, reset=True)  # (train passes curr_state_dict=None: every segment resets; the model stays)
            assert np.array_equal(out.segments[k].run_returns(r), history), (r, k)
            assert np.array_equal(out.segments[k].run_steps(r), at), (r, k)
            val = TableMDPVecEnv(1, mdp, seed=5, agent_offset=r)
            val.step_index = run.rt.step_counter  # the validation steps draw at the run's own counter
            total, _ = run.rt.evaluate_episodes(val, val_episodes)
            assert out.val_totals[k, r] == np.float32(total), (r, k)
        assert np.array_equal(tables[r], run.q), r
        assert counters[r] == run.rt.step_counter, r
        _check_model(model, r, run)


# ---- 10. planning off is untouched -------------------------------------------------------------------------------------------------
def test_planning_steps_zero_is_the_default_path():
    _, envs, _, QLearningPopulation = _product()
    got = []
    for kw in ({}, {"planning_steps": 0}):
        pop = QLearningPopulation(M_ODD, 100, 16, seed=2, dtype=np.float32, **kw)
        res = pop.run_steps(50, envs.HashTabularEnv(M_ODD, 100, 16, seed=1, masked=True))
        got.append((pop.last_stats["kernel_variant"], pop.q_tables, sorted(res.state_dict)))
        assert pop.planning_model is None and pop.planning_steps == 0
        pop.planning_model = None  # nothing to forget
    assert got[0][0] == got[1][0] == 6 | (4 << 12) | (1 << 20)
    assert np.array_equal(got[0][1], got[1][1]) and got[0][1].any() and got[0][2] == got[1][2]
