"""GPU: ``QLearningPopulation(double_q=True)`` (k_double_rollout / k_double_evaluate) against the NumPy model of Double
Q-learning (tests/double_q_model.py), bit for bit: per run both tables, the episode returns and their steps, the counts,
the float32 sums, the final observation / env word / running return, the schedule values and the draw counter.  No
tolerance anywhere.  Every case asserts the kernel build it means to cover (paths 9 and 10, NV and masked bits).

Two anchors do not rest on that model: greedy evaluation with B == 0 is the single-table population's, and a double
population that does not learn (lr == 0) acts exactly like the single-table one that does not learn.
"""
import copy
import pickle

import numpy as np
import pytest

from double_q_model import DoubleRun
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import env_word
from test_gpu_population import _schedules
from test_gpu_td_rules import _device_env, _model_env, _nv, _other, _product

pytestmark = pytest.mark.gpu

M_ODD = 67  # a full and a partial wavefront


def _reached(pop, path="population_double", nv=None, masked=None):
    d = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert pop.last_stats["kernel_variant"] & 15 == {"population_double": 9, "population_double_eval": 10}[path], d
    assert d["path"] == path and pop.double_q and pop.update_rule == "q_learning", d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _population(M, S, A, sched, seed, dt, mode, double_q=True):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode,
                         double_q=double_q)


def _model_runs(kind, p, runs, sched, seed, dt, mode, qa0=None, qb0=None):
    eps_s, lr_s, gamma = sched
    return {r: DoubleRun(_model_env(kind, r, p), gamma[r], eps_s[r], lr_s[r], seed=seed, dtype=dt, mode=mode, agent_id=r,
                         qa0=None if qa0 is None else qa0[r], qb0=None if qb0 is None else qb0[r]) for r in runs}


def _check(pop, res, r, run, history, at, ta, tb, counter):
    """Run r of a population call against its model run (after the same call)."""
    assert np.array_equal(ta[r], run.qa, equal_nan=True), f"run {r}: table A"
    assert np.array_equal(tb[r], run.qb, equal_nan=True), f"run {r}: table B"
    assert np.array_equal(res.run_returns(r), history), f"run {r}: returns"
    assert np.array_equal(res.run_steps(r), at), f"run {r}: episode steps"
    assert res.episode_counts[r] == len(history), f"run {r}: episode count"
    if len(history):
        mean = np.cumsum(history, dtype=np.float32)[-1] / np.float32(len(history))  # the float32 sequential sum / count
        assert res.mean_returns[r] == mean, f"run {r}: mean"
    else:
        assert np.isnan(res.mean_returns[r]), r
    sd = res.state_dict
    assert "pending_actions" not in sd and not [k for k in sd if "double" in k or k.endswith("_b")], sorted(sd)  # unchanged
    assert (sd["states"][r], sd["aux"][r], sd["rewards"][r]) == (run.obs, env_word(run.env), run.acc[0]), f"run {r}: state"
    assert sd["exploration_rate"][r] == run.eps == pop.exploration_rate_schedules[r].get_value(), f"run {r}: epsilon"
    assert sd["lr"][r] == run.lr == pop.lr_schedules[r].get_value(), f"run {r}: learning rate"
    assert pop.step_counters[r] == counter == run.rt.step_counter, f"run {r}: draw counter"


def _run_and_check(kind, p, S, A, M, K, dt, mode, sched, seed=0, nv=None, masked=None):
    pop = _population(M, S, A, sched, seed, dt, mode)
    res = pop.run_steps(K, _device_env(kind, M, p))
    _reached(pop, nv=nv, masked=masked)
    ta, tb = pop.q_tables, pop.q_tables_b
    learned = [0, 0]
    for r, run in _model_runs(kind, p, range(M), sched, seed, dt, mode).items():
        history, at = run.run(K)
        _check(pop, res, r, run, history, at, ta, tb, K)
        learned[0] += bool(run.qa.any())
        learned[1] += bool(run.qb.any())
    assert learned[0] and learned[1], "the case must write into both tables"
    return pop, res


# ---- 1. every row width, both dtypes, both learn modes --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [4, 8, 16, 32, 64])
def test_hash_runs_match_the_model(A, masked, dt, mode):
    p = {"S": 300, "A": A, "seed": 1, "masked": masked}
    pop, _ = _run_and_check("hash", p, 300, A, M_ODD, 150, dt, mode, _schedules(M_ODD), nv=_nv(A), masked=masked)
    assert np.array_equal(pop.q_table(5), pop.q_tables[5]) and np.array_equal(pop.q_table_b(5), pop.q_tables_b[5])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_padded_row_matches_the_model(dt):
    p = {"S": 200, "A": 20, "seed": 1, "masked": True}  # 20 actions in rows of 32
    _run_and_check("hash", p, 200, 20, M_ODD, 150, dt, "iter", _schedules(M_ODD), nv=8, masked=True)
    p = {"S": 200, "A": 5, "seed": 1, "masked": False}  # 5 actions in rows of 8, unmasked: padding is never the arg-max
    _run_and_check("hash", p, 200, 5, 130, 150, dt, "vec", _schedules(130), nv=2, masked=False)


# ---- 2. the other environments: s' == s on walls and always on the bandit, TicTacToe, a stochastic masked MDP ---------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["grid", "bandit", "tictactoe", "table"])
def test_other_environments_match_the_model(kind, dt, mode):
    S, A, p, nv, masked = _other(kind)
    K = 400 if kind == "grid" else 150  # (GridLake's rewards are sparse)
    _run_and_check(kind, p, S, A, M_ODD, K, dt, mode, _schedules(M_ODD), seed=11, nv=nv, masked=masked)


# ---- 3. chaining: calls, a fresh population, launches ----------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 400])  # four states: s' == s at many call boundaries
def test_two_calls_and_a_restored_population_equal_one_call(S, tmp_path):
    envs = _product()[1]
    M, A, K = M_ODD, 8, 90
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter")

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * K, env())
    halves = make()
    e = env()
    first = halves.run_steps(K, e)
    halves.save(tmp_path / "tables.npy")
    assert np.load(tmp_path / "tables.npy").shape == (2, M, S, A)
    blob = pickle.dumps(first.state_dict)
    second = halves.run_steps(K, e, first.state_dict)
    restored = make()  # what a fresh process does: tables from the file, everything else from the pickled dict
    sd = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.restore_training_state(sd)
    third = restored.run_steps(K, env(), sd)
    for pop in (whole, halves, restored):
        _reached(pop, nv=2, masked=True)
        assert np.array_equal(pop.q_tables, whole.q_tables) and np.array_equal(pop.q_tables_b, whole.q_tables_b)
        assert np.array_equal(pop.step_counters, np.full(M, 2 * K))
    assert whole.q_tables.any() and whole.q_tables_b.any()
    for tail in (second, third):
        for r in range(M):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), one.run_returns(r)), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + K]), one.run_steps(r)), r
        assert sorted(tail.state_dict) == sorted(one.state_dict)
        for key in one.state_dict:
            if isinstance(one.state_dict[key], np.ndarray):
                assert np.array_equal(tail.state_dict[key], one.state_dict[key]), key
    # ... and the whole call is the model's
    p = {"S": S, "A": A, "seed": 9, "masked": True}
    ta, tb = whole.q_tables, whole.q_tables_b
    for r, run in _model_runs("hash", p, range(M), sched, 4, np.float32, "iter").items():
        history, at = run.run(2 * K)
        _check(whole, one, r, run, history, at, ta, tb, 2 * K)


def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_and_the_model():
    envs = _product()[1]
    M, K, S, A = 40_000, 2000, 100, 8
    eps0, lr0, gamma0 = _schedules(97)
    sched = [[x[r % 97] for r in range(M)] for x in (eps0, lr0, gamma0)]
    logged = _population(M, S, A, sched, 21, np.float32, "vec")
    res = logged.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1))
    _reached(logged, nv=2, masked=False)
    assert logged.last_stats["launches"] > 9, "the logged call must be cut into more than three launches"
    picked = [0, 1, 63, 64, 20_000, M - 1]
    ta, tb = ({r: t[r] for r in picked} for t in (logged.q_tables, logged.q_tables_b))
    quiet = _population(M, S, A, sched, 21, np.float32, "vec")
    res_q = quiet.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1), log=False)
    assert 1 < quiet.last_stats["launches"] < logged.last_stats["launches"] // 3, "the unlogged call is cut differently"
    assert np.array_equal(quiet.q_tables, logged.q_tables) and np.array_equal(quiet.q_tables_b, logged.q_tables_b)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    for key, value in res.state_dict.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(res_q.state_dict[key], value), key
    del quiet
    p = {"S": S, "A": A, "seed": 1, "masked": False}
    for r, run in _model_runs("hash", p, picked, sched, 21, np.float32, "vec").items():
        history, at = run.run(K)
        _check(logged, res, r, run, history, at, ta, tb, K)


# ---- 4. NaN and infinities in the tables; runs without a selectable action ---------------------------------------------
def special_tables(M, S, A, dt, seed):
    """Random tables.  Every third run gets special cells -- with k = r // 3: k % 3 NaN cells, 1 + k % 2 cells of +inf and
    k % 4 of -inf -- and the runs with r % 13 == 12 a whole NaN row (the list selection has no candidate only on a row
    without a number).  The other runs stay finite, so that no case can lose half its runs."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((M, S, A)).astype(dt)
    for r in range(M):
        k = r // 3
        for count, value in ((k % 3, np.nan), (1 + k % 2, np.inf), (k % 4, -np.inf)) if r % 3 == 0 else ():
            q[r].ravel()[rng.choice(S * A, size=count, replace=False)] = value
        if r % 13 == 12:
            q[r, rng.integers(0, S)] = np.nan
    return q


SPECIAL = [
    (8, False, np.float32, "iter"),   # list selection: steps over NaN
    (8, True, np.float64, "vec"),     # list selection, masked
    (16, True, np.float32, "vec"),    # NumPy-style selection: a NaN in a valid column of the sum row raises
]


def special_case(where, A, dt, M=M_ODD, S=30):
    qa0 = special_tables(M, S, A, dt, seed=A) if where in ("a", "both") else np.zeros((M, S, A), dtype=dt)
    qb0 = special_tables(M, S, A, dt, seed=A + 100) if where in ("b", "both") else np.zeros((M, S, A), dtype=dt)
    return qa0, qb0


def model_outcomes(kind, p, M, K, sched, seed, dt, mode, qa0=None, qb0=None):
    """{run: (model run, history, steps)} of the runs the model completes, and the runs it flags."""
    done, flagged = {}, []
    for r, run in _model_runs(kind, p, range(M), sched, seed, dt, mode, qa0=qa0, qb0=qb0).items():
        try:
            history, at = run.run(K)
        except IndexError:  # some pick of the run had no candidate
            flagged.append(r)
            continue
        done[r] = (run, history, at)
    return done, flagged


def _run_flagged(pop, K, env):
    try:
        return pop.run_steps(K, env), []
    except IndexError as err:
        assert str(err).startswith("Cannot choose from an empty sequence (runs ")
        return err.result, err.runs


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), SPECIAL)
@pytest.mark.parametrize("where", ["a", "b", "both"])
def test_nan_and_infinite_cells_match_the_model_and_stuck_runs_are_named(where, A, masked, dt, mode):
    envs = _product()[1]
    M, S, K = M_ODD, 30, 150
    sched = _schedules(M)
    qa0, qb0 = special_case(where, A, dt)
    pop = _population(M, S, A, sched, 0, dt, mode)
    pop.set_q_tables(qa0, qb0)
    assert np.array_equal(pop.q_tables, qa0, equal_nan=True) and np.array_equal(pop.q_tables_b, qb0, equal_nan=True)
    res, raised = _run_flagged(pop, K, envs.HashTabularEnv(M, S, A, seed=1, masked=masked))
    _reached(pop, nv=_nv(A), masked=masked)
    ta, tb = pop.q_tables, pop.q_tables_b
    p = {"S": S, "A": A, "seed": 1, "masked": masked}
    done, want_raised = model_outcomes("hash", p, M, K, sched, 0, dt, mode, qa0, qb0)
    special_kept = 0
    for r, (run, history, at) in done.items():
        special_kept += not (np.isfinite(run.qa).all() and np.isfinite(run.qb).all())
        _check(pop, res, r, run, history, at, ta, tb, K)
    assert raised == want_raised  # no run is left out that the model does not flag itself
    assert want_raised, "no run met a row without a selectable action"
    assert len(done) >= (M + 1) // 2, "the case must keep at least half its runs"
    assert special_kept, "no run finished with a NaN or an infinity in its tables"


def dead_row_mdp():
    """The stochastic masked 20 x 5 MDP of the other cases with one state whose mask row is all invalid."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    arrays, isd, masks = random_mdp(20, 5, 3, seed=7, masked=True)
    masks = np.array(masks, dtype=bool)
    masks[13] = False
    return encode_table_mdp(*arrays, isd, masks)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_runs_that_meet_an_all_invalid_mask_row_are_named_and_the_others_unaffected(dt):
    M, K = M_ODD, 12
    sched = _schedules(M)
    p = {"mdp": dead_row_mdp(), "seed": 3}
    pop = _population(M, 20, 5, sched, 6, dt, "iter")
    res, raised = _run_flagged(pop, K, _device_env("table", M, p))
    _reached(pop, nv=2, masked=True)
    ta, tb = pop.q_tables, pop.q_tables_b
    done, want_raised = model_outcomes("table", p, M, K, sched, 6, dt, "iter")
    for r, (run, history, at) in done.items():
        _check(pop, res, r, run, history, at, ta, tb, K)
    assert raised == want_raised and want_raised
    assert len(done) >= (M + 1) // 2, "the case must keep at least half its runs"


# ---- 5. greedy evaluation and train() ------------------------------------------------------------------------------------
def _trained(mdp, M, dt, seed=8, K=200):
    envs = _product()[1]
    sched = _schedules(M)
    pop = _population(M, mdp.state_size, mdp.action_size, sched, seed, dt, "iter")
    pop.run_steps(K, envs.TabularMDPEnv(M, mdp, seed=1))
    runs = _model_runs("table", {"mdp": mdp, "seed": 1}, range(M), sched, seed, dt, "iter")
    for run in runs.values():
        run.run(K)
    return pop, runs


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_step_and_episode_evaluation_match_the_model(dt):
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    M, K, V, E = M_ODD, 200, 120, 3
    mdp = _slippery_mdp(envs, masked=True)  # every move may end the episode: greedy episodes end under any policy
    pop, runs = _trained(mdp, M, dt, K=K)
    ta, tb = pop.q_tables, pop.q_tables_b
    res = pop.evaluate_steps(envs.TabularMDPEnv(M, mdp, seed=5), V)
    _reached(pop, "population_double_eval", nv=1, masked=True)
    assert np.array_equal(pop.q_tables, ta) and np.array_equal(pop.q_tables_b, tb)  # no store
    assert (res.steps_used == V).all() and res.finished.all()
    for r, run in runs.items():
        total, history = run.evaluate_steps(TableMDPVecEnv(1, mdp, seed=5, agent_offset=r), V)
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), r
        assert res.totals[r] == np.float32(total) and res.episode_counts[r] == len(history), r
        assert pop.step_counters[r] == run.rt.step_counter == K + V, r
    res = pop.evaluate_episodes(envs.TabularMDPEnv(M, mdp, seed=5), E)
    _reached(pop, "population_double_eval", nv=1, masked=True)
    assert res.finished.all() and (res.episode_counts == E).all()
    for r, run in runs.items():
        before = run.rt.step_counter
        total, history = run.evaluate_episodes(TableMDPVecEnv(1, mdp, seed=5, agent_offset=r), E)
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), r
        assert res.totals[r] == np.float32(total), r
        assert res.steps_used[r] == run.rt.step_counter - before, r
        assert pop.step_counters[r] == run.rt.step_counter, r
    assert len(set(pop.step_counters.tolist())) > 1, "the episode evaluation must leave the runs at different counters"
    # a bound that stops some runs early: finished says which
    bound = int(np.median(res.steps_used))
    short = pop.evaluate_episodes(envs.TabularMDPEnv(M, mdp, seed=5), E, max_steps=bound)
    assert np.array_equal(short.finished, short.episode_counts == E) and (short.steps_used <= bound).all()
    assert (short.steps_used[~short.finished] == bound).all()
    # training goes on from the differing counters, still the model's
    more = pop.run_steps(60, envs.TabularMDPEnv(M, mdp, seed=1))
    ta, tb = pop.q_tables, pop.q_tables_b
    for r, run in runs.items():
        run.rt.step_counter += int(short.steps_used[r])
        history, at = run.run(60, reset=True)
        _check(pop, more, r, run, history, at, ta, tb, run.rt.step_counter)


def _flag_empty_picks(rt):
    """The oracle's greedy evaluation hands the list selection's -1 (no selectable action) on to the environment; every
    engine path raises IndexError for such a run, as the model's training steps do.  The same for the evaluation's picks."""
    greedy = rt._greedy

    def pick(states):
        actions = greedy(states)
        if actions[0] < 0:
            msg = "Cannot choose from an empty sequence"
            raise IndexError(msg)
        return actions

    rt._greedy = pick


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_an_evaluation_that_meets_an_all_invalid_mask_row_names_its_runs_and_the_others_match(dt):
    """k_double_evaluate's empty pick: the runs whose greedy walk reaches the dead state are named, exactly the model's,
    and every other run's returns are the model's."""
    M, V = M_ODD, 12
    sched = _schedules(M)
    p = {"mdp": dead_row_mdp(), "seed": 3}
    rng = np.random.default_rng(5)
    qa0, qb0 = (rng.standard_normal((M, 20, 5)).astype(dt) for _ in range(2))
    pop = _population(M, 20, 5, sched, 6, dt, "iter")
    pop.set_q_tables(qa0, qb0)
    try:
        res, raised = pop.evaluate_steps(_device_env("table", M, p), V), []
    except IndexError as err:
        assert str(err).startswith("Cannot choose from an empty sequence (runs ")
        res, raised = err.result, err.runs
    _reached(pop, "population_double_eval", nv=2, masked=True)
    done, flagged = {}, []
    for r, run in _model_runs("table", p, range(M), sched, 6, dt, "iter", qa0, qb0).items():
        _flag_empty_picks(run.rt)
        try:
            done[r] = run.evaluate_steps(_model_env("table", r, p), V)
        except IndexError:
            flagged.append(r)
    assert raised == flagged and flagged, "no run met the row without a selectable action"
    assert len(done) >= (M + 1) // 2, "the case must keep at least half its runs"
    for r, (total, history) in done.items():
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), f"run {r}: returns"
        assert res.totals[r] == np.float32(total) and res.episode_counts[r] == len(history), r


@pytest.mark.parametrize("mode", ["steps", "episodes"])
def test_a_logged_evaluation_cut_into_launches_equals_the_unlogged_one_and_the_model(mode):
    """k_double_evaluate over several launches with the log: 20 000 runs leave a logged launch 2**23 // 20 000 = 419
    steps, and on this MDP (one outcome in three of every move is terminal) every run ends episodes in each of them."""
    from test_gpu_population_eval import _slippery_mdp

    envs, sch = _product()[1:3]
    M = 20_000
    mdp = _slippery_mdp(envs, seed=21, S=24, A=8)
    S, A = mdp.state_size, mdp.action_size
    rng = np.random.default_rng(0)
    qa0, qb0 = (rng.normal(size=(M, S, A)).astype(np.float32) for _ in range(2))
    sched = ([sch.ConstantSchedule(0.1)] * M, [sch.ConstantSchedule(0.1)] * M, [0.9] * M)
    pop = _population(M, S, A, sched, 1, np.float32, "iter")
    pop.set_q_tables(qa0, qb0)
    if mode == "steps":
        V = 900  # two launches of 419 steps and one of 62
        res = pop.evaluate_steps(envs.TabularMDPEnv(M, mdp, seed=6), V)
        assert pop.last_stats["launches"] == 3 * 3  # each launch with its log scan and pack
        pop.step_counter = 0  # the same evaluation again, without the log
        plain = pop.evaluate_steps(envs.TabularMDPEnv(M, mdp, seed=6), V, log=False)
        assert pop.last_stats["launches"] == 1
    else:
        E = 150  # about 900 steps per run
        res = pop.evaluate_episodes(envs.TabularMDPEnv(M, mdp, seed=6), E)
        assert res.finished.all() and res.steps_used.min() > 419
        assert pop.last_stats["launches"] >= 3 * 3
        pop.step_counter = 0
        plain = pop.evaluate_episodes(envs.TabularMDPEnv(M, mdp, seed=6), E, log=False)
    _reached(pop, "population_double_eval", nv=2, masked=False)
    assert np.array_equal(plain.totals, res.totals) and np.array_equal(plain.steps_used, res.steps_used)
    assert np.array_equal(plain.episode_counts, res.episode_counts)
    assert np.array_equal(np.diff(res.offsets), res.episode_counts)
    picked = [0, 1, 63, 64, 10_000, M - 1]
    for r, run in _model_runs("table", {"mdp": mdp, "seed": 6}, picked, sched, 1, np.float32, "iter", qa0, qb0).items():
        env = TableMDPVecEnv(1, mdp, seed=6, agent_offset=r)
        if mode == "steps":
            total, history = run.evaluate_steps(env, V)
        else:
            total, history = run.evaluate_episodes(env, E)
            assert res.steps_used[r] == run.rt.step_counter, r
        assert len(history) > 2 and np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), r
        assert res.totals[r] == np.float32(total) and res.episode_counts[r] == len(history), r


def test_train_with_episode_validation_matches_the_model_driven_the_same_way():
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)
    M, S, A, seg, n_seg, val_episodes = M_ODD, mdp.state_size, mdp.action_size, 60, 3, 2
    sched = _schedules(M)
    pop = _population(M, S, A, sched, 8, np.float64, "iter")
    out = pop.train(envs.TabularMDPEnv(M, mdp, seed=1), seg * n_seg, envs.TabularMDPEnv(M, mdp, seed=5), seg,
                    val_episodes=val_episodes)
    _reached(pop, "population_double_eval")
    assert out.val_finished.all()
    ta, tb = pop.q_tables, pop.q_tables_b
    counters = pop.step_counters
    assert len(set(counters.tolist())) > 1, "the validations must leave the runs at different counters"
    for r, run in _model_runs("table", {"mdp": mdp, "seed": 1}, range(M), sched, 8, np.float64, "iter").items():
        for k in range(n_seg):
            history, at = run.run(seg, reset=True)  # (train passes curr_state_dict=None: every segment resets)
            assert np.array_equal(out.segments[k].run_returns(r), history), (r, k)
            assert np.array_equal(out.segments[k].run_steps(r), at), (r, k)
            total, _ = run.evaluate_episodes(TableMDPVecEnv(1, mdp, seed=5, agent_offset=r), val_episodes)
            assert out.val_totals[k, r] == np.float32(total), (r, k)
        assert np.array_equal(ta[r], run.qa) and np.array_equal(tb[r], run.qb), r
        assert counters[r] == run.rt.step_counter, r


# ---- 6. exact anchors to the single-table path ---------------------------------------------------------------------------
ANCHOR_KINDS = ["hash", "hash_masked", "hash_wide", "grid", "bandit", "tictactoe", "table"]


def _anchor_case(kind):
    """(S, A, parameters of _device_env, its kind)."""
    if kind.startswith("hash"):
        A, masked = {"hash": (8, False), "hash_masked": (16, True), "hash_wide": (64, True)}[kind]
        return 120, A, {"S": 120, "A": A, "seed": 1, "masked": masked}, "hash"
    if kind == "table":
        from test_gpu_population_eval import _slippery_mdp

        mdp = _slippery_mdp(_product()[1], masked=True)
        return mdp.state_size, mdp.action_size, {"mdp": mdp, "seed": 3}, "table"
    S, A, p, _, _ = _other(kind)
    return S, A, p, kind


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ANCHOR_KINDS)
def test_anchor_evaluation_with_an_empty_second_table_is_the_single_table_evaluation(kind, dt):
    """A + 0 is A (signed zeros do not change ties): evaluate_steps / evaluate_episodes of the double population holding
    (A, 0) equal those of a single-table population holding A, bit for bit."""
    S, A, p, env_kind = _anchor_case(kind)
    M = M_ODD
    sched = _schedules(M)
    rng = np.random.default_rng(3)
    qa = rng.standard_normal((M, S, A)).round(1).astype(dt)  # (rounded: ties, and -0.0 among them)
    qa[qa == 0] *= -1
    episodes = kind in ("bandit", "tictactoe", "table")  # (where every greedy policy ends its episodes)
    got = []
    for double_q in (True, False):
        pop = _population(M, S, A, sched, 2, dt, "iter", double_q=double_q)
        pop.set_q_tables(qa)
        out = [pop.evaluate_steps(_device_env(env_kind, M, p), 150)]
        if double_q:
            _reached(pop, "population_double_eval")
            assert not pop.q_tables_b.any()
        else:
            assert pop.last_stats["kernel_variant"] & 15 == 7
        if episodes:
            out.append(pop.evaluate_episodes(_device_env(env_kind, M, p), 3, max_steps=400))
        got.append((out, pop.step_counters, pop.q_tables))
    (a, ca, ta), (b, cb, tb) = got
    for x, y in zip(a, b):
        for field in x._fields:
            assert np.array_equal(getattr(x, field), getattr(y, field)), (kind, field)
    assert a[0].episode_counts.any() or kind in ("hash", "hash_masked", "hash_wide", "grid")
    assert np.array_equal(ca, cb) and np.array_equal(ta, tb) and np.array_equal(ta, qa)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ANCHOR_KINDS)
def test_anchor_without_learning_the_double_population_acts_like_the_single_table_one(kind, dt, mode):
    """lr == 0 from zero tables: both tables stay zero; same draws, same all-tie picks as the single-table Q-learning
    population with lr == 0, so returns, their steps, observations and counters are equal."""
    sch = _product()[2]
    S, A, p, env_kind = _anchor_case(kind)
    M, K = M_ODD, 300
    eps_s, _, gamma = _schedules(M)
    sched = (eps_s, [sch.ConstantSchedule(0.0)] * M, gamma)
    got = []
    for double_q in (True, False):
        pop = _population(M, S, A, sched, 5, dt, mode, double_q=double_q)
        res = pop.run_steps(K, _device_env(env_kind, M, p))
        if double_q:
            _reached(pop)
            assert not pop.q_tables_b.any()
        else:
            assert pop.last_stats["kernel_variant"] & 15 == 6
        assert not pop.q_tables.any()
        got.append((res, pop.step_counters))
    (a, ca), (b, cb) = got
    for field in ("mean_returns", "episode_counts", "returns", "offsets", "steps"):
        assert np.array_equal(getattr(a, field), getattr(b, field), equal_nan=field == "mean_returns"), (kind, field)
    assert sorted(a.state_dict) == sorted(b.state_dict)
    for key in a.state_dict:
        if key != "infos":
            assert np.array_equal(a.state_dict[key], b.state_dict[key]), key
    assert a.episode_counts.any() and np.array_equal(ca, cb)


# ---- 7. variant, arguments and errors ------------------------------------------------------------------------------------
def test_the_single_table_population_is_untouched():
    _lib, envs, _, QLearningPopulation = _product()
    variants = []
    for kw in ({}, {"double_q": False}):
        pop = QLearningPopulation(M_ODD, 100, 16, seed=2, dtype=np.float32, **kw)
        pop.run_steps(50, envs.HashTabularEnv(M_ODD, 100, 16, seed=1, masked=True))
        variants.append((pop.last_stats["kernel_variant"], pop.q_tables))
        assert _lib.load().qe_population_double(pop.handle) == 0 and not pop.double_q
        with pytest.raises(ValueError, match="second table"):
            pop.q_tables_b
        with pytest.raises(ValueError, match="second table"):
            pop.q_table_b(0)
        with pytest.raises(ValueError, match="second table"):
            pop.set_q_tables(np.zeros((100, 16)), np.zeros((100, 16)))
    assert variants[0][0] == variants[1][0] == 6 | (4 << 12) | (1 << 20)
    assert np.array_equal(variants[0][1], variants[1][1])


def test_no_build_is_refused():
    """Every (dtype, width, masked) build compiles without scratch (tests/test_double_q_host.py), so none answers
    QE_ERR_UNSUPPORTED: the widest one, fp64 with 64 masked actions, trains and evaluates."""
    envs = _product()[1]
    p = {"S": 50, "A": 64, "seed": 1, "masked": True}
    pop, _ = _run_and_check("hash", p, 50, 64, 8, 40, np.float64, "iter", _schedules(8), nv=16, masked=True)
    pop.evaluate_steps(envs.HashTabularEnv(8, 50, 64, seed=1, masked=True), 20)
    _reached(pop, "population_double_eval", nv=16, masked=True)


def test_tables_save_and_load(tmp_path):
    M, S, A = 5, 7, 3
    pop = _population(M, S, A, _schedules(M), 0, np.float64, "iter")
    assert not pop.q_tables.any() and not pop.q_tables_b.any()  # both zero at creation
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((M, S, A)), rng.standard_normal((S, A))
    pop.set_q_tables(a, b)  # one table for every run broadcasts, as for A
    assert np.array_equal(pop.q_tables, a) and np.array_equal(pop.q_tables_b, np.broadcast_to(b, (M, S, A)))
    pop.set_q_tables(2 * a)  # None leaves B as it is
    assert np.array_equal(pop.q_tables, 2 * a) and np.array_equal(pop.q_tables_b, np.broadcast_to(b, (M, S, A)))
    assert np.array_equal(pop.q_table_b(3), b) and np.array_equal(pop.q_table(3), 2 * a[3])
    with pytest.raises(IndexError):
        pop.q_table_b(M)
    with pytest.raises(ValueError, match="shape"):
        pop.set_q_tables(a, np.zeros((M, S)))
    assert np.array_equal(pop.q_tables, 2 * a)  # (both shapes are checked before either table is sent)
    pop.set_q_tables(a.astype(np.float32), b.astype(np.float32))  # the other host dtype converts, as for A
    assert np.array_equal(pop.q_tables_b[0], b.astype(np.float32).astype(np.float64))
    pop.save(tmp_path / "t.npy")
    other = _population(M, S, A, _schedules(M), 0, np.float64, "iter")
    other.load(tmp_path / "t.npy")
    assert np.array_equal(other.q_tables, pop.q_tables) and np.array_equal(other.q_tables_b, pop.q_tables_b)
    np.save(tmp_path / "single.npy", a)
    with pytest.raises(ValueError, match="shape"):
        other.load(tmp_path / "single.npy")
    single = _population(M, S, A, _schedules(M), 0, np.float64, "iter", double_q=False)
    single.load(tmp_path / "single.npy")  # a single-table population behaves as before
    assert np.array_equal(single.q_tables, a)
    single.save(tmp_path / "single2.npy")
    assert np.load(tmp_path / "single2.npy").shape == (M, S, A)


def test_entry_point_errors():
    import ctypes as C

    _lib, envs, _, QLearningPopulation = _product()
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase

    lib = _lib.load()
    buf = np.zeros((8, 50, 4), dtype=np.float64)
    algo = OptimalQLearningBase(10, 4, 0.9, seed=0)  # not a population engine
    for rc in (lib.qe_population_set_double(algo.handle, 1), lib.qe_population_double(algo.handle),
               lib.qe_population_table_b_upload(algo.handle, buf.ctypes.data, _lib.QE_F64),
               lib.qe_population_table_b_download(algo.handle, buf.ctypes.data, _lib.QE_F64),
               lib.qe_population_table_b_download_rows(algo.handle, buf.ctypes.data, 0, 1)):
        assert rc == _lib.ERR_INVALID
        assert "not a population engine" in lib.qe_last_error().decode()
    sarsa = QLearningPopulation(8, 50, 4, update_rule="sarsa")
    for rc in (lib.qe_population_set_double(sarsa.handle, 1), lib.qe_population_set_double(sarsa.handle, 0),
               lib.qe_population_double(sarsa.handle)):
        assert rc == _lib.ERR_UNSUPPORTED
        assert "Q-learning only" in lib.qe_last_error().decode()
    with pytest.raises(ValueError, match="double_q"):
        QLearningPopulation(8, 50, 4, update_rule="expected_sarsa", double_q=True)
    pop = QLearningPopulation(8, 50, 4, dtype=np.float64)
    assert lib.qe_population_double(pop.handle) == 0
    for rc in (lib.qe_population_table_b_upload(pop.handle, buf.ctypes.data, _lib.QE_F64),  # double is off
               lib.qe_population_table_b_download(pop.handle, buf.ctypes.data, _lib.QE_F64),
               lib.qe_population_table_b_download_rows(pop.handle, buf.ctypes.data, 0, 1)):
        assert rc == _lib.ERR_INVALID
        assert "double estimator is off" in lib.qe_last_error().decode()
    assert lib.qe_population_set_double(pop.handle, 1) == 0 and lib.qe_population_double(pop.handle) == 1
    assert lib.qe_population_set_double(pop.handle, 1) == 0  # again: B is kept
    for rule in (_lib.RULE_SARSA, _lib.RULE_EXPECTED_SARSA):
        assert lib.qe_population_set_update_rule(pop.handle, rule) == _lib.ERR_UNSUPPORTED
        assert "Q-learning only" in lib.qe_last_error().decode()
    assert lib.qe_population_set_update_rule(pop.handle, 3) == _lib.ERR_INVALID  # still no fourth rule
    assert "unknown update rule" in lib.qe_last_error().decode()
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_Q_LEARNING) == 0
    assert lib.qe_population_update_rule(pop.handle) == _lib.RULE_Q_LEARNING
    # table B transfers: the checks of their qe_table_* counterparts
    assert lib.qe_population_table_b_upload(pop.handle, None, _lib.QE_F64) == _lib.ERR_INVALID
    assert lib.qe_population_table_b_upload(pop.handle, buf.ctypes.data, 7) == _lib.ERR_INVALID
    assert lib.qe_population_table_b_download(pop.handle, None, _lib.QE_F64) == _lib.ERR_INVALID
    assert lib.qe_population_table_b_download_rows(pop.handle, buf.ctypes.data, 8 * 50 - 1, 2) == _lib.ERR_INVALID
    assert lib.qe_population_table_b_download_rows(pop.handle, buf.ctypes.data, -1, 1) == _lib.ERR_INVALID
    buf[:] = np.arange(buf.size).reshape(buf.shape)
    assert lib.qe_population_table_b_upload(pop.handle, buf.ctypes.data, _lib.QE_F64) == 0
    row = np.zeros(4)
    assert lib.qe_population_table_b_download_rows(pop.handle, row.ctypes.data, 3 * 50 + 2, 1) == 0
    assert np.array_equal(row, buf[3, 2])
    host = np.ones_like(buf)
    assert lib.qe_table_download(pop.handle, host.ctypes.data, _lib.QE_F64) == 0 and not host.any()  # A is untouched
    # off frees B; on again starts from zeros
    assert lib.qe_population_set_double(pop.handle, 0) == 0 and lib.qe_population_double(pop.handle) == 0
    assert lib.qe_population_table_b_download(pop.handle, host.ctypes.data, _lib.QE_F64) == _lib.ERR_INVALID
    res = pop.run_steps(10, envs.HashTabularEnv(8, 50, 4))  # ... and the engine is a single-table population again
    assert pop.last_stats["kernel_variant"] & 15 == 6 and res.episode_counts.shape == (8,)
    assert lib.qe_population_set_double(pop.handle, 1) == 0
    assert lib.qe_population_table_b_download(pop.handle, host.ctypes.data, _lib.QE_F64) == 0 and not host.any()
    stats = _lib.RolloutStats()
    assert C.sizeof(stats) == 104 and lib.qe_abi_version() == 2
