"""GPU: ``QLearningPopulation(planning_steps=n, planning_order="prioritized")`` (k_sweep_rollout) against the NumPy model of
prioritized sweeping (tests/sweep_model.py), bit for bit.

Per run: the table, the episode returns and their steps, the counts, the final observation / env word / running return,
the schedule values, the draw counter, the whole 7-key ``planning_model`` (next states, rewards, flags, the visited list
and its count, the predecessor lists) and the queue.  No tolerance anywhere.  Every case asserts the kernel build it
means to cover (path 13, bit 4, K, NV, masked and n).  ``_case`` names the cases; tests/test_sweep_cases.py counts, on the
model alone, that they reach every branch of the rule.
"""
import copy
import functools
import pickle

import numpy as np
import pytest

from sweep_model import SweepRun, canonical_lists
from test_gpu_dyna import _check_model, _model_shapes, _same_model, _same_state
from test_gpu_population import _schedules
from test_gpu_td_rules import _check as _check_td
from test_gpu_td_rules import _device_env, _model_env, _nv, _product, _special_tables

pytestmark = pytest.mark.gpu

M_ODD = 67  # a full and a partial wavefront
THETAS = (0.0, 1e-4, 1e-2)


def _thetas(M):
    return [THETAS[r % 3] for r in range(M)]


def _frozen_mdp():
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp, outcome_arrays
    from table_mdp_model import FROZEN_4x4, frozen_lake_isd, frozen_lake_P

    return encode_table_mdp(*outcome_arrays(frozen_lake_P(FROZEN_4x4, True)), frozen_lake_isd(FROZEN_4x4))


def _case(name):
    """kind, environment parameters, S, A, steps, n, K, seed, NV, masked of the named case."""
    if name.startswith("hash"):  # hash-<A>-<masked>
        _, A, masked = name.split("-")
        A, masked = int(A), masked == "masked"
        return "hash", {"S": 100, "A": A, "seed": 1, "masked": masked}, 100, A, 150, 5, 4, 0, _nv(A), masked
    p8 = {"S": 100, "A": 8, "seed": 1, "masked": True}
    if name in ("K1", "K32", "n1"):
        return "hash", p8, 100, 8, 150, 1 if name == "n1" else 5, {"K1": 1, "K32": 32}.get(name, 4), 0, 2, True
    if name == "n64":
        return "hash", p8, 100, 8, 20, 64, 32, 0, 2, True
    if name.startswith("four"):  # four-<A>-<masked>: the held row is hit constantly
        _, A, masked = name.split("-")
        A, masked = int(A), masked == "masked"
        return "hash", {"S": 4, "A": A, "seed": 1, "masked": masked}, 4, A, 150, 5, 4, 0, _nv(A), masked
    if name == "bandit":  # one state: every cell is its predecessor, the flag flips at the episode end
        return "bandit", {"episode_len": 7}, 1, 2, 140, 3, 4, 11, 1, False
    if name == "frozen":  # slippery: next states change and cells unlink
        return "table", {"mdp": _frozen_mdp(), "seed": 3}, 16, 4, 150, 5, 4, 11, 1, False
    if name == "grid":  # at 150 steps this one learns nothing: the goal of the 6 x 6 grid is all but never reached, the
        # tables of its first 12 runs stay zero and every step finds its queue empty -- it checks the walk and the model
        return "grid", {"side": 6, "seed": 2}, 36, 4, 150, 5, 4, 11, 1, False
    if name == "grid-small":  # 4 x 4: the goal is reached, its reward is swept back two moves and further
        return "grid", {"side": 4, "seed": 2}, 16, 4, 150, 5, 4, 11, 1, False
    if name == "tictactoe":  # (with five pops per step no call ends with anything queued)
        return "tictactoe", {"seed": 5}, 19683, 9, 60, 5, 4, 11, 4, True
    if name == "tictactoe-n1":  # one pop per step: some runs end the call with entries in their queue
        return "tictactoe", {"seed": 5}, 19683, 9, 60, 1, 4, 11, 4, True
    raise KeyError(name)


def model_runs(name, runs, dt, mode, thetas=None, q0=None, offset=0, sched=None):
    """The model runs of the named case (tests/test_sweep_cases.py runs them without a device)."""
    kind, p, _, _, _, n, K, seed, _, _ = _case(name)
    eps_s, lr_s, gamma = _schedules(M_ODD) if sched is None else sched
    thetas = _thetas(M_ODD) if thetas is None else thetas
    return {r: SweepRun(_model_env(kind, r + offset, p), gamma[r], eps_s[r], lr_s[r], n=n, K=K, theta=thetas[r], seed=seed, dtype=dt,
                        mode=mode, agent_id=r + offset, q0=None if q0 is None else q0[r]) for r in runs}


def _reached(pop, n, K, nv=None, masked=None):
    v = pop.last_stats["kernel_variant"]
    d = _product()[0].decode_variant(v)
    assert v & 15 == 13 and (v >> 4) & 1 and d["path"] == "population_dyna" and d["prioritized"] is True, d
    assert d["planning_steps"] == n == pop.planning_steps and d["queue_length"] == K == pop.queue_length, d
    assert d["rule"] == "q_learning" == pop.update_rule and d["n_step"] == 1 and d["trace_length"] == 0, d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _check_sweep(model, queue, r, run):
    _check_model(model, r, run)
    head, nxt = run.predecessors
    assert np.array_equal(model["pred_head"][r], head), f"run {r}: heads of the predecessor lists"
    assert np.array_equal(model["pred_next"][r], nxt), f"run {r}: links of the predecessor lists"
    cells, priorities = run.sweep_queue
    assert np.array_equal(queue["cells"][r], cells), f"run {r}: queue cells"
    assert np.array_equal(queue["priorities"][r].view(np.uint64), priorities.view(np.uint64)), f"run {r}: queue priorities"


def _check(pop, res, r, run, history, at, tables, counter, model):
    """Run r of a population call against its model run (after the same call)."""
    _check_td(pop, res, r, run, history, at, tables, counter)
    _check_sweep(model, res.state_dict["sweep_queue"], r, run)


def _population(M, S, A, sched, seed, dt, mode, n, K, thetas, **kw):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode,
                         planning_steps=n, planning_order="prioritized", sweep_threshold=thetas, queue_length=K, **kw)


def _shapes(pop, model, queue):
    M, S, A, K = pop.runs, pop.state_size, pop.action_size, pop.queue_length
    assert sorted(model) == ["count", "next_states", "pred_head", "pred_next", "rewards", "terminated", "visited"]
    _model_shapes(pop, {k: v for k, v in model.items() if not k.startswith("pred_")})
    assert model["pred_head"].dtype == model["pred_next"].dtype == np.int32
    assert model["pred_head"].shape == (M, S) and model["pred_next"].shape == (M, S, A)
    assert sorted(queue) == ["cells", "priorities"]
    assert queue["cells"].dtype == np.int32 and queue["priorities"].dtype == np.float64
    assert queue["cells"].shape == queue["priorities"].shape == (M, K)
    free = queue["cells"] < 0
    assert (queue["cells"][free] == -1).all() and not queue["priorities"][free].any()


def _run_and_check(name, dt, mode):
    kind, p, S, A, steps, n, K, seed, nv, masked = _case(name)
    sched = _schedules(M_ODD)
    pop = _population(M_ODD, S, A, sched, seed, dt, mode, n, K, _thetas(M_ODD))
    res = pop.run_steps(steps, _device_env(kind, M_ODD, p))
    _reached(pop, n, K, nv=nv, masked=masked)
    assert "planning_model" not in res.state_dict
    tables, model = pop.q_tables, pop.planning_model
    _shapes(pop, model, res.state_dict["sweep_queue"])
    runs = model_runs(name, range(M_ODD), dt, mode)
    for r, run in runs.items():
        history, at = run.run(steps)
        _check(pop, res, r, run, history, at, tables, steps, model)
    return pop, res, model, runs


# ---- 1. every row width, masked and not, both dtypes, both learn modes ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [4, 8, 16, 32, 64])
def test_hash_runs_match_the_model(A, masked, dt, mode):
    _lib = _product()[0]
    name = f"hash-{A}-{'masked' if masked else 'plain'}"
    if not _lib.sweep_build_shipped(dt, A):  # a width whose build is refused: the constructor says so
        with pytest.raises(ValueError, match="prioritized sweeping: the kernel for .* is not built"):
            _population(M_ODD, 100, A, _schedules(M_ODD), 0, dt, mode, 5, 4, _thetas(M_ODD))
        return
    _run_and_check(name, dt, mode)


# ---- 2. queue lengths and planning counts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "dt", "mode"), [("K1", np.float32, "iter"), ("K1", np.float64, "vec"), ("K32", np.float32, "vec"),
                                                  ("K32", np.float64, "iter"), ("n1", np.float32, "vec"), ("n1", np.float64, "iter"),
                                                  ("n64", np.float32, "iter"), ("n64", np.float64, "vec")])
def test_queue_lengths_and_planning_counts_match_the_model(name, dt, mode):
    _run_and_check(name, dt, mode)


# ---- 3. the held row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["four-4-plain", "four-16-masked"])
def test_four_states_collide_with_the_held_row(name, dt, mode):
    _, _, model, _ = _run_and_check(name, dt, mode)
    assert (model["count"] > 4).all()


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_on_the_bandit_every_cell_is_a_predecessor_of_the_one_state(dt, mode):
    _, _, model, _ = _run_and_check("bandit", dt, mode)
    assert (model["count"] == 2).any() and (model["next_states"][model["next_states"] >= 0] == 0).all()


# ---- 4. other environments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "dt", "mode"), [("frozen", np.float32, "iter"), ("frozen", np.float64, "vec"),
                                                  ("grid", np.float32, "vec"), ("tictactoe", np.float64, "iter"),
                                                  ("grid-small", np.float32, "iter"), ("grid-small", np.float64, "iter"),
                                                  ("grid-small", np.float64, "vec"), ("tictactoe-n1", np.float32, "vec")])
def test_other_environments_match_the_model(name, dt, mode):
    _, res, model, runs = _run_and_check(name, dt, mode)
    assert res.episode_counts.sum() > 0
    if name == "frozen":
        assert (model["count"] < 150).all(), "no cell was observed twice: nothing was overwritten"
    if name == "grid-small":  # (tests/test_sweep_cases.py: in most runs value reaches a state two moves from the goal)
        assert 2 * sum(bool(run.q.any()) for run in runs.values()) >= M_ODD
    if name == "tictactoe-n1":
        assert (res.state_dict["sweep_queue"]["cells"] >= 0).any(), "every queue is empty at the end of the call"


# ---- 5. NaN and infinities in the tables ---------------------------------------------------------------------------------------
SPECIAL = [(8, False, np.float32, "iter"), (8, True, np.float64, "vec"), (16, True, np.float32, "vec")]


def special_runs(A, masked, dt, mode, runs=range(M_ODD)):
    """(model runs, q0) of a special-table case: Hash 30 x A, n = 4, K = 4."""
    q0 = _special_tables(M_ODD, 30, A, dt, seed=A)
    eps_s, lr_s, gamma = _schedules(M_ODD)
    thetas = _thetas(M_ODD)
    p = {"S": 30, "A": A, "seed": 1, "masked": masked}
    return {r: SweepRun(_model_env("hash", r, p), gamma[r], eps_s[r], lr_s[r], n=4, K=4, theta=thetas[r], seed=0, dtype=dt, mode=mode,
                        agent_id=r, q0=q0[r]) for r in runs}, q0


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), SPECIAL)
def test_nan_and_infinite_cells_match_the_model(A, masked, dt, mode):
    envs = _product()[1]
    M, S, K, n = M_ODD, 30, 100, 4
    runs, q0 = special_runs(A, masked, dt, mode)
    pop = _population(M, S, A, _schedules(M), 0, dt, mode, n, 4, _thetas(M))
    pop.set_q_tables(q0)
    try:
        res, raised = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=masked)), []
    except IndexError as err:
        res, raised = err.result, err.runs
    _reached(pop, n, 4, nv=_nv(A), masked=masked)
    tables, model = pop.q_tables, pop.planning_model
    want_raised, special_kept = [], 0
    for r, run in runs.items():
        try:
            history, at = run.run(K)
        except IndexError:  # (a run without a selectable action is on its own from there on)
            want_raised.append(r)
            continue
        special_kept += not np.isfinite(run.q).all()
        _check(pop, res, r, run, history, at, tables, K, model)
    assert raised == want_raised
    assert len(want_raised) < M and special_kept, "no compared run finished with a NaN or an infinity in its table"


# ---- 6. a threshold nothing passes: the plain Q-learning population ----------------------------------------------------------------
@pytest.mark.parametrize(("dt", "mode"), [(np.float32, "vec"), (np.float64, "iter")])
def test_a_threshold_above_every_increment_equals_the_population_without_planning(dt, mode):
    envs = _product()[1]
    M, S, A, steps = M_ODD, 100, 8, 150
    sched = _schedules(M)
    eps_s, lr_s, gamma = sched
    pop = _population(M, S, A, sched, 2, dt, mode, 5, 4, 1e300)
    res = pop.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1, masked=True))
    _reached(pop, 5, 4, nv=2, masked=True)
    plain = _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=2, dtype=dt, learn_mode=mode, planning_steps=0)
    want = plain.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1, masked=True))
    assert plain.last_stats["kernel_variant"] & 15 == 6
    assert np.array_equal(pop.q_tables, plain.q_tables) and pop.q_tables.any()
    assert np.array_equal(res.returns, want.returns) and np.array_equal(res.offsets, want.offsets)
    assert np.array_equal(res.steps, want.steps)
    assert (res.state_dict["sweep_queue"]["cells"] == -1).all()
    assert pop.planning_model["count"].all()


# ---- 7. a non-zero agent offset: run r is a one-run population at agent_offset + r -------------------------------------------------
def test_run_r_equals_a_one_run_population_at_its_agent_offset():
    envs = _product()[1]
    M, S, A, steps, n, K, off = M_ODD, 50, 8, 100, 4, 4, 1000
    sched = _schedules(M)
    thetas = _thetas(M)
    pop = _population(M, S, A, sched, 3, np.float32, "iter", n, K, thetas)
    res = pop.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1, masked=True, agent_offset=off))
    _reached(pop, n, K, nv=2, masked=True)
    tables, model = pop.q_tables, pop.planning_model
    queue = res.state_dict["sweep_queue"]
    for r in (0, 1, 38, 63, 64, 66):
        one = _population(1, S, A, [[x[r]] for x in sched], 3, np.float32, "iter", n, K, [thetas[r]])
        got = one.run_steps(steps, envs.HashTabularEnv(1, S, A, seed=1, masked=True, agent_offset=off + r))
        assert np.array_equal(one.q_tables[0], tables[r]), r
        assert np.array_equal(got.returns, res.run_returns(r)) and np.array_equal(got.run_steps(0), res.run_steps(r)), r
        for key, value in one.planning_model.items():
            assert np.array_equal(value[0], model[key][r]), (r, key)
        for key, value in got.state_dict["sweep_queue"].items():
            assert np.array_equal(value[0], queue[key][r]), (r, key)
    # ... and the model agrees about them
    p = {"S": S, "A": A, "seed": 1, "masked": True}
    eps_s, lr_s, gamma = sched
    for r in (0, 64, 66):
        run = SweepRun(_model_env("hash", r + off, p), gamma[r], eps_s[r], lr_s[r], n=n, K=K, theta=thetas[r], seed=3, dtype=np.float32,
                       mode="iter", agent_id=r + off)
        history, at = run.run(steps)
        _check(pop, res, r, run, history, at, tables, steps, model)


# ---- 8. chaining and resume ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 400])
def test_calls_and_a_restored_population_equal_one_call(S, tmp_path):
    envs = _product()[1]
    M, A, steps, n, K = M_ODD, 8, 75, 5, 4
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter", n, K, _thetas(M))

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * steps, env())
    halves = make()
    e = env()
    first = halves.run_steps(steps, e)
    assert "planning_model" not in first.state_dict
    assert (first.state_dict["sweep_queue"]["cells"] >= 0).any(), "no queue holds anything at the cut: nothing is carried"
    at_cut = halves.planning_model
    assert (at_cut["count"] > 0).all() and (at_cut["pred_head"] >= 0).any()
    halves.save(tmp_path / "tables.npy")
    halves.save_model(tmp_path / "model.npz")
    blob = pickle.dumps(first.state_dict)
    second = halves.run_steps(steps, e, first.state_dict)
    restored = make()  # a fresh process: tables and model from their files, then the rest from the pickled dict
    sd = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.load_model(tmp_path / "model.npz")
    restored.restore_training_state(sd)
    _same_model(restored.planning_model, at_cut)
    _same_model(restored.sweep_queue, first.state_dict["sweep_queue"])
    third = restored.run_steps(steps, env(), sd)
    for pop in (whole, halves, restored):
        _reached(pop, n, K, nv=2, masked=True)
        assert np.array_equal(pop.q_tables, whole.q_tables)
        assert np.array_equal(pop.step_counters, np.full(M, 2 * steps))
        _same_model(pop.planning_model, whole.planning_model)
        _same_model(pop.sweep_queue, whole.sweep_queue)
    for tail in (second, third):
        for r in range(M):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), one.run_returns(r)), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + steps]), one.run_steps(r)), r
        sq = tail.state_dict.pop("sweep_queue")
        _same_model(sq, one.state_dict["sweep_queue"])
        _same_state(tail.state_dict, {k: v for k, v in one.state_dict.items() if k != "sweep_queue"})


def test_a_reset_empties_the_queue_and_keeps_the_model_and_the_lists():
    envs = _product()[1]
    M, S, A, steps, n, K = M_ODD, 30, 8, 70, 4, 8
    sched = _schedules(M)
    thetas = _thetas(M)
    pop = _population(M, S, A, sched, 6, np.float64, "vec", n, K, thetas)
    first = pop.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=2, masked=False))
    assert (first.state_dict["sweep_queue"]["cells"] >= 0).any()
    kept = pop.planning_model
    res = pop.run_steps(0, envs.HashTabularEnv(M, S, A, seed=2, masked=False))  # curr_state_dict=None: a reset
    _same_model(pop.planning_model, kept)
    assert (res.state_dict["sweep_queue"]["cells"] == -1).all() and not res.state_dict["sweep_queue"]["priorities"].any()
    assert res.state_dict["rng_step"] == steps
    # a dict without the key starts every queue empty as well; the model run does the same
    pop2 = _population(M, S, A, sched, 6, np.float64, "vec", n, K, thetas)
    e2 = envs.HashTabularEnv(M, S, A, seed=2, masked=False)
    a = pop2.run_steps(steps, e2)
    b = pop2.run_steps(steps, e2, {k: v for k, v in a.state_dict.items() if k != "sweep_queue"})
    _reached(pop2, n, K, nv=2, masked=False)
    tables, model = pop2.q_tables, pop2.planning_model
    p = {"S": S, "A": A, "seed": 2, "masked": False}
    eps_s, lr_s, gamma = sched
    for r in range(0, M, 6):
        run = SweepRun(_model_env("hash", r, p), gamma[r], eps_s[r], lr_s[r], n=n, K=K, theta=thetas[r], seed=6, dtype=np.float64,
                       mode="vec", agent_id=r)
        run.run(steps)
        run.rt.empty_queue()
        history, at = run.run(steps)
        _check(pop2, b, r, run, history, at, tables, 2 * steps, model)


def test_forgetting_the_model_empties_the_lists_and_the_queue():
    envs = _product()[1]
    M, S, A, n, K = 8, 20, 4, 3, 4
    pop = _product()[3](M, S, A, planning_steps=n, planning_order="prioritized", queue_length=K, dtype=np.float32)
    pop.run_steps(60, envs.HashTabularEnv(M, S, A))
    assert (pop.sweep_queue["cells"] >= 0).any() and (pop.planning_model["pred_head"] >= 0).any()
    pop.planning_model = None
    empty = pop.planning_model
    assert not empty["count"].any() and (empty["pred_head"] == -1).all() and (empty["pred_next"] == -1).all()
    assert (pop.sweep_queue["cells"] == -1).all() and not pop.sweep_queue["priorities"].any()


# ---- 9. the model setter ---------------------------------------------------------------------------------------------------------
def test_the_model_setter_the_queue_setter_and_the_refusals_on_a_live_engine():
    import ctypes

    from dist_classicrl_amd.environments.device_envs import encode_table_mdp
    from table_mdp_model import random_mdp

    _lib, envs, _, QLearningPopulation = _product()
    lib = _lib.load()
    M, S, A, K = 8, 20, 5, 4
    f64 = ctypes.c_double
    arrays, isd, masks = random_mdp(S, A, 3, seed=7, masked=True)  # three outcomes per cell: cells unlink, the lists reorder
    mdp = encode_table_mdp(*arrays, isd, masks)
    plain = QLearningPopulation(M, S, A, planning_steps=3)
    assert plain.sweep_queue is None and lib.qe_population_sweeping(plain.handle) == 0
    assert sorted(plain.planning_model) == ["count", "next_states", "rewards", "terminated", "visited"]
    for rc in (lib.qe_population_predecessors(plain.handle, None, None), lib.qe_population_set_predecessors(plain.handle, None, None),
               lib.qe_population_queue(plain.handle, None, None), lib.qe_population_set_queue(plain.handle, None, None)):
        assert rc == _lib.ERR_INVALID and "prioritized sweeping is off" in lib.qe_last_error().decode()
    with pytest.raises(ValueError, match="has no sweep queue"):
        plain.sweep_queue = {}
    theta = np.zeros(M)
    for bad in (-1, 33):
        assert lib.qe_population_set_sweeping(plain.handle, bad, _lib.ptr(theta, f64)) == _lib.ERR_INVALID
    for bad in (-1.0, np.inf, np.nan):
        assert lib.qe_population_set_sweeping(plain.handle, 4, _lib.ptr(np.full(M, bad), f64)) == _lib.ERR_INVALID
    assert lib.qe_population_set_sweeping(plain.handle, 4, None) == _lib.ERR_INVALID
    none = QLearningPopulation(M, S, A)
    assert lib.qe_population_set_sweeping(none.handle, 4, _lib.ptr(theta, f64)) == _lib.ERR_INVALID
    assert "planning is off" in lib.qe_last_error().decode()

    pop = QLearningPopulation(M, S, A, planning_steps=3, planning_order="prioritized", queue_length=K, dtype=np.float32)
    assert lib.qe_population_sweeping(pop.handle) == K and lib.qe_population_planning(pop.handle) == 3
    # the other setters refuse to switch rules, as they do for planning
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_SARSA) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_double(pop.handle, 1) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_n_step(pop.handle, 2) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_visits(pop.handle, None, 1) == _lib.ERR_UNSUPPORTED
    res = pop.run_steps(150, envs.TabularMDPEnv(M, mdp, seed=3))
    good, queue = pop.planning_model, res.state_dict["sweep_queue"]
    assert good["count"].all() and (queue["cells"] >= 0).any()
    five = {k: v for k, v in good.items() if not k.startswith("pred_")}

    # a 7-key upload round-trips and empties the queue; the queue goes back in after it
    pop.planning_model = None
    pop.planning_model = good
    _same_model(pop.planning_model, good)
    assert (pop.sweep_queue["cells"] == -1).all()
    pop.sweep_queue = queue
    _same_model(pop.sweep_queue, queue)
    # a 5-key upload rebuilds the lists in the canonical order
    pop.planning_model = five
    got = pop.planning_model
    _same_model({k: got[k] for k in five}, five)
    differs = False
    for r in range(M):
        head, nxt = canonical_lists(five["next_states"][r], five["terminated"][r], five["visited"][r], five["count"][r])
        assert np.array_equal(got["pred_head"][r], head) and np.array_equal(got["pred_next"][r], nxt), r
        differs |= not np.array_equal(good["pred_next"][r], nxt)
    assert differs, "every run's lists were canonical already: the rebuild shows nothing"
    pop.planning_model = good

    # bad lists are refused and change nothing; no kernel is launched on them
    r = 5
    linked = good["pred_next"][r].ravel() >= 0
    x = int(np.flatnonzero([len(_walk(good, r, s)) >= 2 for s in range(S)])[0])  # a state with two predecessors or more
    lst = _walk(good, r, x)
    other = int(np.flatnonzero([s != x and len(_walk(good, r, s)) >= 1 for s in range(S)])[0])
    other_head = int(good["pred_head"][r, other])
    term = np.flatnonzero((good["next_states"][r].ravel() >= 0) & good["terminated"][r].ravel())
    unseen = int(np.flatnonzero(good["next_states"][r].ravel() < 0)[0])
    assert linked.any()

    def changed(*edits):
        bad = {k: v.copy() for k, v in good.items()}
        for key, index, value in edits:
            bad[key][index] = value
        return bad

    def nx(c):
        return (r, c // A, c % A)

    cases = [
        (changed(("pred_next", nx(lst[-1]), lst[0])), "is reached twice"),                       # a cycle
        (changed(("pred_next", nx(lst[-1]), other_head)), "next state of cell"),                  # a tail shared with another list
        (changed(("pred_head", (r, other), lst[0])), "next state of cell"),                       # a node of another state
        (changed(("pred_head", (r, x), lst[1])), "they reach"),                                   # a missing node
        (changed(("pred_next", nx(lst[-1]), unseen)), "is unseen in the model"),
        (changed(("pred_next", nx(lst[-1]), S * A)), "is outside"),
        (changed(("pred_next", nx(lst[-1]), -2)), "is outside"),
        (changed(("pred_next", nx(unseen), lst[0])), "is not linked"),
    ]
    if term.size:
        cases.append((changed(("pred_next", nx(lst[-1]), int(term[0]))), "is terminated in the model"))
    pop.sweep_queue = queue
    for bad, text in cases:
        with pytest.raises(ValueError, match=text):
            pop.planning_model = bad
        _same_model(pop.planning_model, good)
    assert lib.qe_population_set_predecessors(pop.handle, _lib.ptr(np.ascontiguousarray(good["pred_head"]), ctypes.c_int32), None) == _lib.ERR_INVALID
    # bad queues
    pop.sweep_queue = queue
    seen = np.flatnonzero(good["next_states"][r].ravel() >= 0)

    def queue_with(cells, priorities):
        bad = {k: v.copy() for k, v in queue.items()}
        bad["cells"][r], bad["priorities"][r] = cells, priorities
        return bad

    for bad, text in ((queue_with([unseen, -1, -1, -1], [1.0, 0, 0, 0]), "is unseen in the model"),
                      (queue_with([seen[0], seen[0], -1, -1], [1.0, 2.0, 0, 0]), "name the same cell"),
                      (queue_with([S * A, -1, -1, -1], [1.0, 0, 0, 0]), "is outside"),
                      (queue_with([-2, -1, -1, -1], [1.0, 0, 0, 0]), "is outside"),
                      (queue_with([seen[0], -1, -1, -1], [np.nan, 0, 0, 0]), "NaN or negative"),
                      (queue_with([seen[0], -1, -1, -1], [-1.0, 0, 0, 0]), "NaN or negative"),
                      (queue_with([-1, -1, -1, -1], [0, 0.5, 0, 0]), "a free slot holds priority 0")):
        with pytest.raises(ValueError, match=text):
            pop.sweep_queue = bad
        _same_model(pop.sweep_queue, queue)
    pop.sweep_queue = queue_with([seen[0], -1, seen[1], -1], [0.0, 0, np.inf, 0])  # a zero and an infinite priority are priorities
    assert np.array_equal(pop.sweep_queue["cells"][r], [seen[0], -1, seen[1], -1])
    # queue_length changed on a live engine keeps the model and empties the queues; 0 gives uniform Dyna-Q back
    assert lib.qe_population_set_sweeping(pop.handle, 7, _lib.ptr(theta, f64)) == 0 and lib.qe_population_sweeping(pop.handle) == 7
    assert lib.qe_population_set_sweeping(pop.handle, K, _lib.ptr(theta, f64)) == 0
    assert (pop.sweep_queue["cells"] == -1).all()
    assert lib.qe_population_set_sweeping(pop.handle, 0, None) == 0 and lib.qe_population_sweeping(pop.handle) == 0
    assert lib.qe_population_planning(pop.handle) == 3
    assert lib.qe_population_queue(pop.handle, None, None) == _lib.ERR_INVALID


def _walk(model, r, x):
    """The predecessor list of state x of run r, head to tail."""
    out, c = [], int(model["pred_head"][r, x])
    nxt = model["pred_next"][r].ravel()
    while c >= 0:
        out.append(c)
        c = int(nxt[c])
    return out


# ---- 10. a priority equal to the threshold: ``P > theta`` is strict at all three sites ---------------------------------------------
THETA_EQUAL = [(np.float32, "iter"), (np.float64, "vec"), (np.float32, "vec")]  # (the last: the unrounded float64 increment)
THETA_PROBE = 40


@functools.lru_cache(maxsize=None)
def equal_threshold_runs(dt, mode):
    """``(thresholds, {run: (model run, history, steps)})`` of ``four-16-masked`` at 150 steps, where run r's threshold is
    the smallest non-zero priority its model run at threshold 0 compares within 40 steps.  Every comparison before the
    first with that priority is of 0 or of something greater, so it falls as at threshold 0, the history up to it is the
    probe's, and the comparison ``P == theta`` takes place (tests/test_sweep_cases.py counts at which site)."""
    name = "four-16-masked"
    thetas = []
    for run in model_runs(name, range(M_ODD), dt, mode, thetas=[0.0] * M_ODD).values():
        run.run(THETA_PROBE)
        thetas.append(run.rt.smallest_compared)
    runs = model_runs(name, range(M_ODD), dt, mode, thetas=thetas)
    return thetas, {r: (run, *run.run(_case(name)[4])) for r, run in runs.items()}


@pytest.mark.parametrize(("dt", "mode"), THETA_EQUAL)
def test_a_priority_equal_to_the_threshold_does_not_pass(dt, mode):
    kind, p, S, A, steps, n, K, seed, nv, masked = _case("four-16-masked")
    thetas, done = equal_threshold_runs(dt, mode)
    assert all(0 < t < np.inf for t in thetas)
    pop = _population(M_ODD, S, A, _schedules(M_ODD), seed, dt, mode, n, K, thetas)
    res = pop.run_steps(steps, _device_env(kind, M_ODD, p))
    _reached(pop, n, K, nv=nv, masked=masked)
    tables, model = pop.q_tables, pop.planning_model
    for r, (run, history, at) in done.items():
        assert sum(run.rt.events[f"threshold_equal_{site}"] for site in ("step", "plan", "propagate")), r
        _check(pop, res, r, run, history, at, tables, steps, model)


# ---- 11. a call cut into launches: the queue goes LDS -> [slot][runs] -> LDS, and ``hi`` is rebuilt over holes ---------------------
# 2^25 / runs / (1 + n) steps per launch, and at most 2^23 / runs in a logged call: from n = 3 on the first bound is the
# smaller one and both calls are cut at the same steps, so n = 2.  40 000 runs: 209 steps per logged launch, 279 per
# unlogged one
CUT = {"M": 40_000, "K": 500, "S": 40, "A": 8, "n": 2, "queue": 4, "seed": 21}


def _holes_below_a_live_slot(cells):
    """Per run: some free slot lies below a live one."""
    live = cells >= 0
    above = np.flip(np.logical_or.accumulate(np.flip(live, axis=1), axis=1), axis=1)  # slot i or a later one is live
    return (~live & above).any(axis=1)


def _same_call_state(a, b):
    a, b = dict(a), dict(b)
    _same_model(a.pop("sweep_queue"), b.pop("sweep_queue"))
    _same_state(a, b)


def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_the_halves_and_the_model():
    from test_gpu_population_limits import _cycled_schedules

    envs = _product()[1]
    M, K, S, A, n, Q, seed = (CUT[k] for k in ("M", "K", "S", "A", "n", "queue", "seed"))
    sched = _cycled_schedules(M)
    thetas = _thetas(M)

    def make():
        return _population(M, S, A, sched, seed, np.float32, "iter", n, Q, thetas)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=1, masked=True)

    logged = make()
    res = logged.run_steps(K, env())
    _reached(logged, n, Q, nv=2, masked=True)
    assert logged.last_stats["launches"] == 9  # 209 + 209 + 82 steps, each launch with its scan and its pack
    tables, model = logged.q_tables, logged.planning_model
    quiet = make()
    res_q = quiet.run_steps(K, env(), log=False)
    assert quiet.last_stats["launches"] == 2, "the unlogged call is cut differently: 279 + 221 steps"
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    _same_call_state(res_q.state_dict, res.state_dict)
    _same_model(quiet.planning_model, model)
    _same_model(quiet.sweep_queue, res.state_dict["sweep_queue"])
    del quiet
    halves = make()
    e = env()
    first = halves.run_steps(K // 2, e)
    assert halves.last_stats["launches"] == 6  # 209 + 41 steps
    at_cut = first.state_dict["sweep_queue"]["cells"]
    assert _holes_below_a_live_slot(at_cut).any(), "no queue crosses the call boundary with a hole below a live slot"
    second = halves.run_steps(K // 2, e, first.state_dict)
    assert np.array_equal(halves.q_tables, tables)
    assert np.array_equal(first.episode_counts + second.episode_counts, res.episode_counts)
    at1, at2 = first.offsets, second.offsets
    for r in range(M):  # the two calls' logs, joined run by run, are the one call's log
        joined = np.concatenate([first.returns[at1[r]:at1[r + 1]], second.returns[at2[r]:at2[r + 1]]])
        assert np.array_equal(joined, res.returns[res.offsets[r]:res.offsets[r + 1]]), r
    _same_call_state(second.state_dict, res.state_dict)
    _same_model(halves.planning_model, model)
    _same_model(halves.sweep_queue, res.state_dict["sweep_queue"])
    del halves
    p = {"S": S, "A": A, "seed": 1, "masked": True}
    eps_s, lr_s, gamma = sched
    for r in (0, 1, 63, 64, 65, 1023, 1024, 1025, M // 2, M - 1):
        run = SweepRun(_model_env("hash", r, p), gamma[r], eps_s[r], lr_s[r], n=n, K=Q, theta=thetas[r], seed=seed, dtype=np.float32,
                       mode="iter", agent_id=r)
        history, at = run.run(K)
        _check(logged, res, r, run, history, at, tables, K, model)


# ---- 12. a call that starts from an uploaded queue: a hole, a live zero and an infinity --------------------------------------------
@pytest.mark.parametrize(("dt", "mode"), [(np.float32, "vec"), (np.float64, "iter")])
def test_a_call_from_an_uploaded_queue_with_a_hole_a_zero_and_an_infinity_matches_the_model(dt, mode):
    envs = _product()[1]
    M, S, A, steps, n, K = M_ODD, 20, 5, 60, 3, 4  # rows of 8: the cell s * A + a lies at s * 8 + a on the device
    sched = _schedules(M)
    thetas = _thetas(M)
    pop = _population(M, S, A, sched, 7, dt, mode, n, K, thetas)
    e = envs.HashTabularEnv(M, S, A, seed=1, masked=True)
    first = pop.run_steps(steps, e)
    _reached(pop, n, K, nv=2, masked=True)
    tables1, model1 = pop.q_tables, pop.planning_model
    visited, count = model1["visited"], model1["count"]
    assert (count >= 2).all()
    queue = {"cells": np.full((M, K), -1, dtype=np.int32), "priorities": np.zeros((M, K))}
    queue["cells"][:, 0], queue["cells"][:, 2] = visited[:, 0], visited[:, 1]
    queue["priorities"][:, 2] = np.inf
    assert (queue["cells"][:, [0, 2]] >= A).any(), "no uploaded cell has another offset on the device than on the host"
    pop.sweep_queue = queue
    _same_model(pop.sweep_queue, queue)
    second = pop.run_steps(steps, e, {**first.state_dict, "sweep_queue": queue})
    tables, model = pop.q_tables, pop.planning_model
    p = {"S": S, "A": A, "seed": 1, "masked": True}
    eps_s, lr_s, gamma = sched
    popped_inf = 0
    for r in range(M):
        run = SweepRun(_model_env("hash", r, p), gamma[r], eps_s[r], lr_s[r], n=n, K=K, theta=thetas[r], seed=7, dtype=dt, mode=mode,
                       agent_id=r)
        history, at = run.run(steps)
        assert np.array_equal(tables1[r], run.q), f"run {r}: table before the upload"
        _check_sweep(model1, first.state_dict["sweep_queue"], r, run)
        run.rt.cells = [int(c) for c in queue["cells"][r]]
        run.rt.priorities = [float(x) for x in queue["priorities"][r]]
        history, at = run.run(steps)
        popped_inf += bool(run.rt.events["pop_inf"])
        _check(pop, second, r, run, history, at, tables, 2 * steps, model)
    assert popped_inf == M


# ---- 12b. a planning store that puts the first NaN into the row held in registers ----------------------------------------------------
NAN_UPLOAD = [(8, np.float32, "iter"), (16, np.float64, "vec")]  # list selection / NumPy-style selection
NAN_UPLOAD_STEPS = (60, 4)


@functools.lru_cache(maxsize=None)
def nan_upload_case(A, dt, mode):
    """Four states, masked, n = 5, K = 4.  After 60 steps run r gets a NaN in column 0 (always valid) of row ``x = r % 4``
    and a queue of up to four seen, linked cells of other rows whose model entry leads to ``x``, all at priority inf.
    The next step pops them: each stores a NaN, and where its row is the next observation's the row the kernel holds
    turns NaN under it (``held_row_turns_nan``).  Returns the tables and queues to upload and, per run, the model run
    with the outcome of the 4 steps after the upload (None for a run the model flags)."""
    name = f"four-{A}-masked"
    _, _, S, _, _, n, K, _, _, _ = _case(name)
    runs = model_runs(name, range(M_ODD), dt, mode)
    tables = np.zeros((M_ODD, S, A), dtype=dt)
    queue = {"cells": np.full((M_ODD, K), -1, dtype=np.int32), "priorities": np.zeros((M_ODD, K))}
    out = {}
    for r, run in runs.items():
        before = run.run(NAN_UPLOAD_STEPS[0])
        x = r % S
        run.q[x, 0] = np.nan
        tables[r] = run.q
        into_x = [c for c, (nxt, _, term) in sorted(run.rt.model.items()) if nxt == x and not term and c // A != x][:K]
        queue["cells"][r, :len(into_x)] = into_x
        queue["priorities"][r, :len(into_x)] = np.inf
        run.rt.cells, run.rt.priorities = [int(c) for c in queue["cells"][r]], [float(p) for p in queue["priorities"][r]]
        try:
            out[r] = (run, before, run.run(NAN_UPLOAD_STEPS[1]))
        except IndexError:
            out[r] = (run, before, None)
    return tables, queue, out


@pytest.mark.parametrize(("A", "dt", "mode"), NAN_UPLOAD)
def test_a_planning_store_that_turns_the_held_row_nan_matches_the_model(A, dt, mode):
    kind, p, S, _, _, n, K, seed, nv, masked = _case(f"four-{A}-masked")
    tables0, queue, out = nan_upload_case(A, dt, mode)
    k1, k2 = NAN_UPLOAD_STEPS
    pop = _population(M_ODD, S, A, _schedules(M_ODD), seed, dt, mode, n, K, _thetas(M_ODD))
    e = _device_env(kind, M_ODD, p)
    first = pop.run_steps(k1, e)
    pop.set_q_tables(tables0)
    pop.sweep_queue = queue
    try:
        second, raised = pop.run_steps(k2, e, {**first.state_dict, "sweep_queue": queue}), []
    except IndexError as err:
        second, raised = err.result, err.runs
    _reached(pop, n, K, nv=nv, masked=masked)
    tables, model = pop.q_tables, pop.planning_model
    assert raised == [r for r, (_, _, after) in out.items() if after is None]
    turned = 0
    for r, (run, (history, at), after) in out.items():
        assert np.array_equal(first.run_returns(r), history) and np.array_equal(first.run_steps(r), at), r
        if after is not None:
            turned += bool(run.rt.events["held_row_turns_nan"])
            _check(pop, second, r, run, *after, tables, k1 + k2, model)
    assert turned >= 5, "too few compared runs turn the held row NaN"


# ---- 13. the uniform order is untouched -----------------------------------------------------------------------------------------
def test_the_uniform_order_is_the_default_and_keeps_its_five_keys():
    _, envs, _, QLearningPopulation = _product()
    got = []
    for kw in ({}, {"planning_order": "uniform"}):
        pop = QLearningPopulation(M_ODD, 100, 16, seed=2, dtype=np.float32, planning_steps=4, **kw)
        res = pop.run_steps(50, envs.HashTabularEnv(M_ODD, 100, 16, seed=1, masked=True))
        got.append((pop.last_stats["kernel_variant"], pop.q_tables, sorted(res.state_dict), sorted(pop.planning_model)))
        assert pop.sweep_queue is None and pop.planning_order == "uniform"
    assert got[0][0] == got[1][0] == 13 | (4 << 12) | (1 << 20) | (4 << 24)
    assert np.array_equal(got[0][1], got[1][1]) and got[0][1].any() and got[0][2] == got[1][2]
    assert "sweep_queue" not in got[0][2] and got[0][3] == ["count", "next_states", "rewards", "terminated", "visited"]
