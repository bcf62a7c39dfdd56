"""GPU: ``QLearningPopulation(tree_backup=n)`` (k_tree_rollout) against the NumPy model of n-step Tree Backup
(tests/tree_backup_model.py), bit for bit: per run the table, the episode returns and their steps, the counts, the final
observation / env word / running return, the schedule values, the draw counter and the window with its flags.  No
tolerance anywhere.  Every case asserts the kernel build it means to cover (path 15, NV, masked and n).  The training
cases and their model runs come from tests/tree_backup_cases.py, which builds them without a device.
"""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest

import tree_backup_cases as tc
from test_gpu_population import _schedules
from test_gpu_td_rules import _check as _check_td
from test_gpu_td_rules import _device_env, _product

pytestmark = pytest.mark.gpu

M_ODD = tc.M_ODD
WINDOW_KEYS = ("length", "states", "actions", "rewards", "greedy")


def _reached(pop, n, nv=None, masked=None):
    d = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert pop.last_stats["kernel_variant"] & 15 == 15 and d["path"] == "population_tree", d
    assert d["rule"] == "q_learning" == pop.update_rule and d["tree_backup"] == n == pop.tree_backup and d["n_step"] == 1, d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _check(pop, res, r, run, history, at, tables, counter):
    """Run r of a population call against its model run (after the same call): the 1-step rules' list, and the window."""
    _check_td(pop, res, r, run, history, at, tables, counter)
    length, states, actions, rewards, greedy = run.window
    win = res.state_dict["tree_backup_window"]
    assert win["length"][r] == length, f"run {r}: window length"
    assert np.array_equal(win["states"][r], states), f"run {r}: window states"
    assert np.array_equal(win["actions"][r], actions), f"run {r}: window actions"
    assert np.array_equal(win["rewards"][r].view(np.uint32), rewards.view(np.uint32)), f"run {r}: window rewards"
    assert np.array_equal(win["greedy"][r], greedy), f"run {r}: window flags"


def _population(M, S, A, sched, seed, dt, mode, n, **kw):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode,
                         tree_backup=n, **kw)


def _same_window(a, b):
    assert sorted(a) == sorted(WINDOW_KEYS) == sorted(b)
    for key in WINDOW_KEYS:
        assert np.array_equal(a[key], b[key]), key


# ---- 1. the training cases: every row width, both dtypes and learn modes, the horizons, every environment ----------------
@pytest.mark.parametrize("case_id", [c["id"] for c in tc.CASES])
def test_runs_match_the_model(case_id):
    c = tc.BY_ID[case_id]
    M, K, n, dt = c["M"], c["K"], c["n"], np.dtype(c["dt"])
    pop = _population(M, c["S"], c["A"], _schedules(M), c["seed"], dt, c["mode"], n)
    q0 = tc.initial_tables(c)
    if q0 is not None:
        pop.set_q_tables(q0)
    res = pop.run_steps(K, _device_env(c["kind"].split("_")[0], M, tc.env_params(c)))
    _reached(pop, n, nv=c["nv"], masked=c["masked"])
    tables = pop.q_tables
    for r, (run, history, at) in tc.model(case_id).items():
        _check(pop, res, r, run, history, at, tables, K)
    win = res.state_dict["tree_backup_window"]
    assert win["length"].dtype == win["states"].dtype == win["actions"].dtype == np.int32
    assert win["rewards"].dtype == np.float32 and win["greedy"].dtype == np.uint8
    assert win["length"].shape == (M,)
    assert win["states"].shape == win["actions"].shape == win["rewards"].shape == win["greedy"].shape == (M, n - 1)
    assert win["length"].max() == (0 if c["kind"] == "bandit_mc" else n - 1)
    _same_window(pop.tree_backup_window, win)


# ---- 2. chaining: calls, a fresh process, calls shorter than the horizon; a reset drops the window; log=False ------------
@pytest.mark.parametrize("S", [4, 400])  # four states: windows that repeat cells, cut states equal to s' at many call boundaries
def test_calls_and_a_restored_population_equal_one_call(S, tmp_path):
    envs = _product()[1]
    M, A, K, n = M_ODD, 8, 90, 4
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter", n)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * K, env())
    quiet = make()
    one_q = quiet.run_steps(2 * K, env(), log=False)
    assert one_q.returns.size == 0 and np.array_equal(one_q.episode_counts, one.episode_counts)
    assert np.array_equal(one_q.mean_returns, one.mean_returns, equal_nan=True)
    halves = make()
    e = env()
    first = halves.run_steps(K, e)
    assert first.state_dict["tree_backup_window"]["length"].max() == n - 1, "the window must be non-empty at the cut"
    assert not first.state_dict["tree_backup_window"]["greedy"].all() and first.state_dict["tree_backup_window"]["greedy"].any()
    halves.save(tmp_path / "tables.npy")
    blob = pickle.dumps(first.state_dict)
    second = halves.run_steps(K, e, first.state_dict)
    restored = make()  # what a fresh process does: tables from the file, everything else from the pickled dict
    sd = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.restore_training_state(sd)
    _same_window(restored.tree_backup_window, first.state_dict["tree_backup_window"])
    third = restored.run_steps(K, env(), sd)
    short = make()  # 60 calls of 3 steps: every call is shorter than the horizon
    e3, sd3, pieces = env(), None, []
    for _ in range(2 * K // 3):
        res3 = short.run_steps(3, e3, sd3) if sd3 is not None else short.run_steps(3, e3)
        sd3 = res3.state_dict
        pieces.append(res3)
    for pop in (whole, quiet, halves, restored, short):
        _reached(pop, n, nv=2, masked=True)
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
    same_state(one_q.state_dict, one.state_dict)
    for r in range(M):
        assert np.array_equal(np.concatenate([x.run_returns(r) for x in pieces]), one.run_returns(r)), r
        assert np.array_equal(np.concatenate([x.run_steps(r) + 3 * i for i, x in enumerate(pieces)]), one.run_steps(r)), r
    # a dict without the key: every window starts empty, its entries are never updated (the model, told so)
    lost = make()
    lost.load(tmp_path / "tables.npy")
    stripped = {k: v for k, v in sd.items() if k != "tree_backup_window"}
    lost.restore_training_state(stripped)
    assert (lost.tree_backup_window["length"] == 0).all()
    res = lost.run_steps(K, env(), stripped)
    tables = lost.q_tables
    assert not np.array_equal(tables, whole.q_tables)
    p = {"S": S, "A": A, "seed": 9, "masked": True}
    for r, run in tc.model_runs("hash", p, range(M), n, sched, 4, np.float32, "iter").items():
        run.run(K)
        run.rt.window.clear()
        history, at = run.run(K)
        _check(lost, res, r, run, history, at, tables, 2 * K)


def test_a_reset_drops_the_window_and_evaluation_and_train_leave_it_alone():
    from table_mdp_model import TableMDPVecEnv
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)  # every move may end the episode: greedy validation episodes end too
    M, S, A, seg, n_seg, val_episodes, n = M_ODD, mdp.state_size, mdp.action_size, 60, 3, 2, 3
    sched = _schedules(M)
    pop = _population(M, S, A, sched, 8, np.float64, "iter", n)
    out = pop.train(envs.TabularMDPEnv(M, mdp, seed=1), seg * n_seg, envs.TabularMDPEnv(M, mdp, seed=5), seg,
                    val_episodes=val_episodes)
    assert _product()[0].decode_variant(pop.last_stats["kernel_variant"])["path"] == "population_eval"
    assert out.val_finished.all()
    tables = pop.q_tables
    counters = pop.step_counters
    assert len(set(counters.tolist())) > 1, "the validations must leave the runs at different counters"
    window = pop.tree_backup_window  # greedy evaluation neither reads nor clears it
    _same_window(window, out.state_dict["tree_backup_window"])
    pop.evaluate_steps(envs.TabularMDPEnv(M, mdp, seed=5), 30)
    _same_window(pop.tree_backup_window, window)
    pop.policy_values(envs.TabularMDPEnv(M, mdp, seed=5), tol=1e-6, max_sweeps=50)
    _same_window(pop.tree_backup_window, window)
    dropped = 0
    for r, run in tc.model_runs("table", {"mdp": mdp, "seed": 1}, range(M), n, sched, 8, np.float64, "iter").items():
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
        length, states, actions, rewards, greedy = run.window
        assert window["length"][r] == length and np.array_equal(window["states"][r], states), r
        assert np.array_equal(window["actions"][r], actions) and np.array_equal(window["rewards"][r], rewards), r
        assert np.array_equal(window["greedy"][r], greedy), r
    assert dropped, "no segment started over a non-empty window"


# ---- 2b. launch chopping ---------------------------------------------------------------------------------------------------
def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for key, value in b.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(a[key], value), key
    _same_window(a["tree_backup_window"], b["tree_backup_window"])


def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_and_the_model():
    """Every launch loads the window from the per-run arrays and stores it there, compacted to ``base = 0``."""
    from test_gpu_population_limits import _cycled_schedules

    envs = _product()[1]
    M, K, S, A, n = 20_000, 2000, 40, 8, 4
    sched = _cycled_schedules(M)

    def make():
        return _population(M, S, A, sched, 21, np.float32, "iter", n)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=1, masked=True)

    logged = make()
    res = logged.run_steps(K, env())
    _reached(logged, n, nv=2, masked=True)
    # 2^23 log entries / 20 000 runs = 419 steps per launch: 5 launches, each with its scan and its pack
    assert logged.last_stats["launches"] == 15
    tables = logged.q_tables
    quiet = make()
    res_q = quiet.run_steps(K, env(), log=False)
    assert 1 < quiet.last_stats["launches"] < 5, "the unlogged call is cut differently"
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    _same_state(res_q.state_dict, res.state_dict)
    _same_window(quiet.tree_backup_window, res.state_dict["tree_backup_window"])
    del quiet
    halves = make()
    e = env()
    first = halves.run_steps(K // 2, e)
    second = halves.run_steps(K // 2, e, first.state_dict)
    assert first.state_dict["tree_backup_window"]["length"].max() == n - 1
    assert np.array_equal(halves.q_tables, tables)
    assert np.array_equal(first.episode_counts + second.episode_counts, res.episode_counts)
    # the mean of a call is the float32 sequential sum of its logged returns over their count: the two calls' logs,
    # joined run by run, are the one call's log, and with it its means
    at1, at2 = first.offsets, second.offsets
    for r in range(M):
        joined = np.concatenate([first.returns[at1[r]:at1[r + 1]], second.returns[at2[r]:at2[r + 1]]])
        assert np.array_equal(joined, res.returns[res.offsets[r]:res.offsets[r + 1]]), r
        if joined.size:
            assert np.cumsum(joined, dtype=np.float32)[-1] / np.float32(joined.size) == res.mean_returns[r], r
    _same_state(second.state_dict, res.state_dict)
    _same_window(halves.tree_backup_window, res.state_dict["tree_backup_window"])
    del halves
    p = {"S": S, "A": A, "seed": 1, "masked": True}
    picked = [0, 1, 63, 64, 65, 1023, 1024, 1025, 10_000, M - 1]
    for r, run in tc.model_runs("hash", p, picked, n, sched, 21, np.float32, "iter").items():
        history, at = run.run(K)
        _check(logged, res, r, run, history, at, {r: tables[r]}, K)


# ---- 3. NaN, infinities and ties in the tables; runs without a selectable action -----------------------------------------
@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [
    (8, False, np.float32, "iter"),   # list selection: steps over NaN
    (8, True, np.float64, "vec"),     # list selection, masked
    (16, True, np.float32, "vec"),    # NumPy-style selection: a NaN in a valid column raises
])
def test_special_cells_match_the_model_and_stuck_runs_are_named(A, masked, dt, mode):
    envs = _product()[1]
    c = tc.NAN_CASE
    M, S, K, n = c["M"], c["S"], c["K"], c["n"]
    q0 = tc.special_tables(M, S, A, dt, seed=A)
    pop = _population(M, S, A, _schedules(M), c["seed"], dt, mode, n)
    pop.set_q_tables(q0)
    try:
        res, raised = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=c["env_seed"], masked=masked)), []
    except IndexError as err:
        assert str(err).startswith("Cannot choose from an empty sequence (runs ")
        res, raised = err.result, err.runs
    _reached(pop, n, nv=tc.nv_of(A), masked=masked)
    tables = pop.q_tables
    want_raised, special_kept = tc.nan_case_model(
        A, masked, dt, mode, check=lambda r, run, history, at: _check(pop, res, r, run, history, at, tables, K))
    assert raised == want_raised
    assert want_raised, "no run met a row without a selectable action"
    assert special_kept, "no run finished with a NaN or an infinity in its table"


# ---- 4. anchors ---------------------------------------------------------------------------------------------------------
def test_tree_backup_one_is_the_plain_population():
    _, envs, _, QLearningPopulation = _product()
    got = []
    for kw in ({}, {"tree_backup": 1}):
        pop = QLearningPopulation(M_ODD, 100, 16, seed=2, dtype=np.float32, **kw)
        res = pop.run_steps(50, envs.HashTabularEnv(M_ODD, 100, 16, seed=1, masked=True))
        got.append((pop.last_stats["kernel_variant"], pop.q_tables, sorted(res.state_dict)))
        assert "tree_backup_window" not in res.state_dict and pop.tree_backup_window is None and pop.tree_backup == 1
        pop.tree_backup_window = None
        with pytest.raises(ValueError, match="has no window"):
            pop.tree_backup_window = {}
    assert got[0][0] == got[1][0] == 6 | (4 << 12) | (1 << 20)
    assert np.array_equal(got[0][1], got[1][1]) and got[0][1].any() and got[0][2] == got[1][2]


@pytest.mark.parametrize(("n", "dt", "mode", "masked"), [(2, np.float32, "vec", False), (5, np.float64, "iter", True),
                                                        (16, np.float32, "iter", True)])
def test_without_exploration_it_is_n_step_expected_sarsa_on_the_device(n, dt, mode, masked):
    _, envs, sch, QLearningPopulation = _product()
    M, S, A, K = M_ODD, 40, 8, 150
    lr = [sch.ConstantSchedule(0.1 + 0.002 * r) for r in range(M)]
    gamma = [0.9 + 0.001 * r for r in range(M)]
    out = []
    for kw in ({"tree_backup": n}, {"update_rule": "expected_sarsa", "n_step": n}):
        pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr), sch.ConstantSchedule(0.0), seed=3, dtype=dt,
                                  learn_mode=mode, **kw)
        res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=2, masked=masked))
        out.append((pop, res))
    (tree, a), (nstep, b) = out
    _reached(tree, n, nv=2, masked=masked)
    assert nstep.last_stats["kernel_variant"] & 15 == 11
    assert np.array_equal(tree.q_tables, nstep.q_tables) and tree.q_tables.any() and np.isfinite(tree.q_tables).all()
    assert np.array_equal(a.returns, b.returns) and np.array_equal(a.steps, b.steps) and np.array_equal(a.offsets, b.offsets)
    wa, wb = a.state_dict["tree_backup_window"], b.state_dict["n_step_window"]
    for key in ("length", "states", "actions", "rewards"):
        assert np.array_equal(wa[key], wb[key]), key
    assert np.array_equal(wa["greedy"], np.arange(n - 1)[None, :] < wa["length"][:, None])  # every action was greedy


def test_run_r_is_the_one_run_population_at_its_agent_offset():
    _, envs, _, QLearningPopulation = _product()
    M, S, A, K, n, off = M_ODD, 40, 8, 120, 4, 5
    eps_s, lr_s, gamma = _schedules(M)
    pop = _population(M, S, A, (eps_s, lr_s, gamma), 6, np.float64, "vec", n)
    res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=2, masked=True, agent_offset=off))
    _reached(pop, n, nv=2, masked=True)
    tables = pop.q_tables
    for r in (0, 1, 63, 64, M - 1):
        solo = QLearningPopulation(1, S, A, gamma[r], copy.deepcopy(lr_s[r]), copy.deepcopy(eps_s[r]), seed=6, dtype=np.float64,
                                   learn_mode="vec", tree_backup=n)
        one = solo.run_steps(K, envs.HashTabularEnv(1, S, A, seed=2, masked=True, agent_offset=off + r))
        _reached(solo, n, nv=2, masked=True)
        assert np.array_equal(solo.q_tables[0], tables[r]), r
        assert np.array_equal(one.returns, res.run_returns(r)) and np.array_equal(one.steps, res.run_steps(r)), r
        for key in ("states", "aux", "rewards", "lr", "exploration_rate"):
            assert one.state_dict[key][0] == res.state_dict[key][r], (r, key)
        for key in WINDOW_KEYS:
            assert np.array_equal(one.state_dict["tree_backup_window"][key][0], res.state_dict["tree_backup_window"][key][r]), (r, key)


# ---- 5. refusals, both directions; the window's setter -------------------------------------------------------------------
def test_refusals_and_arguments():
    _lib, envs, _, QLearningPopulation = _product()
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase

    lib = _lib.load()
    i32 = lambda a: _lib.ptr(a, C.c_int32)  # noqa: E731
    algo = OptimalQLearningBase(10, 4, 0.9, seed=0)
    assert lib.qe_population_set_tree_backup(algo.handle, 2) == _lib.ERR_INVALID
    assert "not a population engine" in lib.qe_last_error().decode()
    assert lib.qe_population_tree_backup(algo.handle) == _lib.ERR_INVALID
    # Python: before anything is allocated (tests/test_tree_backup_host.py has the whole list)
    with pytest.raises(ValueError, match="tree_backup=2 .*needs update_rule='q_learning'"):
        QLearningPopulation(8, 50, 4, update_rule="sarsa", tree_backup=2)
    # C: the switch on a population that is in another mode
    lam = np.full(8, 0.5)
    beta = np.full(8, 0.5)
    others = (({"update_rule": "sarsa"}, "update rule 1"), ({"update_rule": "expected_sarsa"}, "update rule 2"),
              ({"double_q": True}, "double estimator"), ({"update_rule": "sarsa", "n_step": 3}, "update rule 1"),
              ({"trace_decay": 0.5}, "eligibility traces are on"), ({"planning_steps": 2}, "planning is on"),
              ({"exploration_bonus": 0.5}, "visit counts are on"), ({"visit_lr": True}, "visit counts are on"))
    for kw, text in others:
        other = QLearningPopulation(8, 50, 4, **kw)
        assert lib.qe_population_set_tree_backup(other.handle, 3) == _lib.ERR_UNSUPPORTED, kw
        assert text in lib.qe_last_error().decode(), (kw, lib.qe_last_error().decode())
        assert lib.qe_population_tree_backup(other.handle) == 1
        assert lib.qe_population_set_tree_backup(other.handle, 1) == 0  # 1 is what they have
    # ... and every other mode on a population with the switch on
    pop = QLearningPopulation(8, 50, 4, tree_backup=3)
    assert lib.qe_population_tree_backup(pop.handle) == 3
    for bad in (0, -1, 17):
        assert lib.qe_population_set_tree_backup(pop.handle, bad) == _lib.ERR_INVALID
        assert "tree_backup must be in 1 .. 16" in lib.qe_last_error().decode()
    f64 = lambda a: _lib.ptr(a, C.c_double)  # noqa: E731
    for call in (lambda: lib.qe_population_set_update_rule(pop.handle, _lib.RULE_SARSA),
                 lambda: lib.qe_population_set_update_rule(pop.handle, _lib.RULE_EXPECTED_SARSA),
                 lambda: lib.qe_population_set_double(pop.handle, 1),
                 lambda: lib.qe_population_set_n_step(pop.handle, 2),
                 lambda: lib.qe_population_set_traces(pop.handle, 4, _lib.TRACE_REPLACING, f64(lam)),
                 lambda: lib.qe_population_set_planning(pop.handle, 2),
                 lambda: lib.qe_population_set_visits(pop.handle, f64(beta), 0),
                 lambda: lib.qe_population_set_visits(pop.handle, None, 1)):
        assert call() == _lib.ERR_UNSUPPORTED
        assert "tree_backup = 3 is on" in lib.qe_last_error().decode(), lib.qe_last_error().decode()
    # the switches' own "off" and Q-learning stay accepted
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_Q_LEARNING) == 0 and lib.qe_population_set_double(pop.handle, 0) == 0
    assert lib.qe_population_set_n_step(pop.handle, 1) == 0 and lib.qe_population_set_planning(pop.handle, 0) == 0
    assert lib.qe_population_set_traces(pop.handle, 0, 0, None) == 0 and lib.qe_population_set_visits(pop.handle, None, 0) == 0
    assert lib.qe_population_tree_backup(pop.handle) == 3
    # n_step = 2 with Q-learning keeps its refusal
    ql = QLearningPopulation(8, 50, 4)
    assert lib.qe_population_set_n_step(ql.handle, 2) == _lib.ERR_UNSUPPORTED
    assert "uncorrected n-step Q-learning is not an off-policy method" in lib.qe_last_error().decode()
    # the window's setter: shapes, lengths, states, actions and flags
    win = pop.tree_backup_window
    assert (win["length"] == 0).all() and win["states"].shape == (8, 2) and win["greedy"].dtype == np.uint8
    good = {"length": np.array([0, 1, 2, 0, 1, 2, 0, 1]), "states": np.arange(16).reshape(8, 2) % 50,
            "actions": np.arange(16).reshape(8, 2) % 4, "rewards": np.linspace(-1, 1, 16).reshape(8, 2),
            "greedy": (np.arange(16).reshape(8, 2) % 3 == 0)}
    pop.tree_backup_window = good
    back = pop.tree_backup_window
    used = np.arange(2)[None, :] < good["length"][:, None]
    assert np.array_equal(back["length"], good["length"])
    for key in ("states", "actions", "rewards", "greedy"):
        assert np.array_equal(back[key], np.where(used, good[key], 0).astype(back[key].dtype)), key
    for key, value, text in (("length", np.full(8, 3), "length 3 is outside"), ("length", np.full(8, -1), "length -1"),
                             ("states", np.full((8, 2), 50), "state 50 is outside"),
                             ("actions", np.full((8, 2), 4), "action 4 is outside"),
                             ("actions", np.full((8, 2), -1), "action -1 is outside"),
                             ("greedy", np.full((8, 2), 2), "flags 0 or 1")):
        bad = dict(good, **{key: value})
        if key != "length":
            bad["length"] = np.full(8, 2)
        with pytest.raises(ValueError, match=text):
            pop.tree_backup_window = bad
    for bad in (dict(good, states=np.zeros((8, 3), dtype=np.int32)), dict(good, length=np.zeros(7, dtype=np.int32)),
                dict(good, rewards=np.zeros((8, 2), dtype=complex)), {"length": good["length"]}, [1, 2]):
        with pytest.raises(ValueError, match="tree_backup_window"):
            pop.tree_backup_window = bad
    _same_window(pop.tree_backup_window, back)  # a refused window changes nothing
    # the C setter's own checks: a flag other than 0 or 1, NULL arrays
    length = np.ascontiguousarray(good["length"], dtype=np.int32)
    states, actions = (np.ascontiguousarray(good[k], dtype=np.int32) for k in ("states", "actions"))
    rewards = np.ascontiguousarray(good["rewards"], dtype=np.float32)
    flags = np.full((8, 2), 2, dtype=np.uint8)
    args = (i32(length), i32(states), i32(actions), _lib.ptr(rewards, C.c_float))
    assert lib.qe_population_set_tree_window(pop.handle, *args, _lib.ptr(flags, C.c_uint8)) == _lib.ERR_INVALID
    assert "greedy flag 2 is neither 0 nor 1" in lib.qe_last_error().decode()
    assert lib.qe_population_set_tree_window(pop.handle, *args, None) == _lib.ERR_INVALID
    _same_window(pop.tree_backup_window, back)
    out = np.zeros(8, dtype=np.int32)
    assert lib.qe_population_tree_window(pop.handle, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.qe_population_tree_window(pop.handle, i32(out), None, None, None, None) == 0 and np.array_equal(out, good["length"])
    pop.tree_backup_window = None
    assert (pop.tree_backup_window["length"] == 0).all()
    res = pop.run_steps(10, envs.HashTabularEnv(8, 50, 4))
    assert res.state_dict["tree_backup_window"]["length"].max() == 2
    # run_steps(curr_state_dict=None) empties the window: the dropped entries are never updated
    pop.run_steps(0, envs.HashTabularEnv(8, 50, 4))
    assert (pop.tree_backup_window["length"] == 0).all()
    # setting the horizon empties the windows
    pop.run_steps(10, envs.HashTabularEnv(8, 50, 4))
    assert lib.qe_population_set_tree_backup(pop.handle, 5) == 0 and lib.qe_population_tree_backup(pop.handle) == 5
    assert lib.qe_population_tree_window(pop.handle, i32(out), None, None, None, None) == 0 and (out == 0).all()


def test_the_window_calls_at_horizon_one():
    """tree_backup = 1 has no window: the getter writes nothing, the setter takes only "every window empty"."""
    _lib, _, _, QLearningPopulation = _product()
    lib = _lib.load()
    i32 = lambda a: _lib.ptr(a, C.c_int32)  # noqa: E731
    pop = QLearningPopulation(8, 50, 4, tree_backup=1)
    length = np.full(8, 7, dtype=np.int32)
    assert lib.qe_population_tree_window(pop.handle, i32(length), None, None, None, None) == 0 and (length == 7).all()
    assert lib.qe_population_tree_window(pop.handle, None, None, None, None, None) == 0
    assert lib.qe_population_set_tree_window(pop.handle, None, None, None, None, None) == 0
    assert lib.qe_population_set_tree_window(pop.handle, i32(np.zeros(8, dtype=np.int32)), None, None, None, None) == 0
    one = np.array([0, 1, 0, 0, 0, 0, 0, 0], dtype=np.int32)
    assert lib.qe_population_set_tree_window(pop.handle, i32(one), None, None, None, None) == _lib.ERR_INVALID
    assert "window of run 1: length 1 with tree_backup = 1" in lib.qe_last_error().decode()
    assert lib.qe_population_tree_backup(pop.handle) == 1 and pop.tree_backup_window is None
