"""GPU: ``QLearningPopulation(update_rule="sarsa" | "q_learning", trace_decay=lam)`` (k_trace_rollout), bit for bit:

* against the EXISTING one-step kernels where the definition says the step is theirs (lambda = 0; one replacing slot at
  any lambda) -- an anchor the trace model has no part in;
* against the NumPy model of the traces (tests/trace_model.py) everywhere else.

Per run: the table, the episode returns and their steps, the counts, the final observation / env word / running return,
the pending action, the schedule values, the draw counter and the trace slots.  No tolerance anywhere.  Every case
asserts the kernel build it means to cover (path 12, rule, NV, masked, K and the trace kind).
"""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest

from test_gpu_population import _schedules
from test_gpu_td_rules import _check as _check_td
from test_gpu_td_rules import _device_env, _model_env, _nv, _product, _special_tables
from trace_model import TraceRun

pytestmark = pytest.mark.gpu

RULES = ["sarsa", "q_learning"]
KINDS = ["replacing", "accumulating"]
M_ODD = 67  # a full and a partial wavefront


def _lambdas(M):
    """A lambda grid over the runs, 0 and 1 included."""
    return [(0.0, 1.0, 0.9, 0.5, 0.97)[r % 5] for r in range(M)]


def _reached(pop, rule, K, kind="replacing", nv=None, masked=None):
    d = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert pop.last_stats["kernel_variant"] & 15 == 12 and d["path"] == "population_trace", d
    assert d["rule"] == rule == pop.update_rule and d["trace_length"] == K == pop.trace_length, d
    assert d["trace_kind"] == kind == pop.trace_kind and d["n_step"] == 1, d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _check(pop, res, r, run, history, at, tables, counter):
    """Run r of a population call against its model run (after the same call): the 1-step rules' list, and the slots."""
    _check_td(pop, res, r, run, history, at, tables, counter)
    states, actions, values = run.slots
    tr = res.state_dict["eligibility_traces"]
    assert np.array_equal(tr["values"][r].view(np.uint64), values.view(np.uint64)), f"run {r}: trace values"
    assert np.array_equal(tr["states"][r], states), f"run {r}: trace states"
    assert np.array_equal(tr["actions"][r], actions), f"run {r}: trace actions"


def _model_runs(kind, p, runs, rule, lam, K, tkind, sched, seed, dt, mode, q0=None):
    eps_s, lr_s, gamma = sched
    return {r: TraceRun(_model_env(kind, r, p), rule, gamma[r], eps_s[r], lr_s[r], lam=lam[r], K=K, kind=tkind, seed=seed,
                        dtype=dt, mode=mode, agent_id=r, q0=None if q0 is None else q0[r]) for r in runs}


def _population(M, S, A, sched, seed, dt, mode, rule, **kw):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode,
                         update_rule=rule, **kw)


def _run_and_check(kind, p, S, A, M, steps, rule, dt, mode, sched, K=8, tkind="replacing", lam=None, seed=0, nv=None, masked=None):
    lam = _lambdas(M) if lam is None else lam
    pop = _population(M, S, A, sched, seed, dt, mode, rule, trace_decay=lam, trace_length=K, trace_kind=tkind)
    res = pop.run_steps(steps, _device_env(kind, M, p))
    _reached(pop, rule, K, tkind, nv=nv, masked=masked)
    tables = pop.q_tables
    for r, run in _model_runs(kind, p, range(M), rule, lam, K, tkind, sched, seed, dt, mode).items():
        history, at = run.run(steps)
        _check(pop, res, r, run, history, at, tables, steps)
    tr = res.state_dict["eligibility_traces"]
    assert tr["states"].dtype == tr["actions"].dtype == np.int32 and tr["values"].dtype == np.float64
    assert tr["states"].shape == tr["actions"].shape == tr["values"].shape == (M, K)
    free = tr["values"] == 0
    assert not tr["states"][free].any() and not tr["actions"][free].any()
    return pop, res


def _same_state(a, b, but=()):
    assert sorted(a) == sorted(b)
    for key in b:
        if key in but:
            continue
        if isinstance(b[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        elif isinstance(b[key], dict):
            for k2 in b[key]:
                assert np.array_equal(a[key][k2], b[key][k2]), (key, k2)
        else:
            assert a[key] == b[key], key


# ---- 1. against the existing kernels: lambda = 0, and one replacing slot ------------------------------------------------------
def _against_the_one_step_kernel(rule, dt, mode, A, masked, S=100, steps=150, q0=None, **trace_kw):
    envs = _product()[1]
    sched = _schedules(M_ODD)
    out = []
    for kw in ({}, trace_kw):
        pop = _population(M_ODD, S, A, sched, 3, dt, mode, rule, **kw)
        if q0 is not None:
            pop.set_q_tables(q0)
        try:
            res, raised = pop.run_steps(steps, envs.HashTabularEnv(M_ODD, S, A, seed=1, masked=masked)), []
        except IndexError as err:
            res, raised = err.result, err.runs
        out.append((pop, res, raised))
    (plain, want, stuck), (pop, got, stuck_t) = out
    one_step = {"q_learning": 6, "sarsa": 8 | (1 << 4)}[rule]
    assert plain.last_stats["kernel_variant"] == one_step | (_nv(A) << 12) | (int(masked) << 20)
    _reached(pop, rule, trace_kw["trace_length"], trace_kw.get("trace_kind", "replacing"), nv=_nv(A), masked=masked)
    assert stuck == stuck_t
    keep = np.setdiff1d(np.arange(M_ODD), stuck)  # (a run without a selectable action is on its own from there on)
    assert len(keep), "every run met a row without a selectable action: nothing is compared"
    a, b = pop.q_tables[keep], plain.q_tables[keep]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint8), b[~np.isnan(b)].view(np.uint8))
    assert a[~np.isnan(a)].any()
    for r in keep:
        assert np.array_equal(got.run_returns(r), want.run_returns(r)) and np.array_equal(got.run_steps(r), want.run_steps(r)), r
    assert np.array_equal(got.episode_counts[keep], want.episode_counts[keep])
    assert np.array_equal(got.mean_returns[keep], want.mean_returns[keep], equal_nan=True)
    assert sorted(got.state_dict) == sorted([*want.state_dict, "eligibility_traces"])
    for key, value in want.state_dict.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(got.state_dict[key][keep], value[keep]), key
        else:
            assert got.state_dict[key] == value, key
    assert np.array_equal(pop.step_counters, plain.step_counters)
    for s_a, s_b in zip(pop.exploration_rate_schedules + pop.lr_schedules, plain.exploration_rate_schedules + plain.lr_schedules):
        assert s_a.get_value() == s_b.get_value()
    return got.state_dict["eligibility_traces"], keep


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rule", RULES)
def test_lambda_zero_is_the_one_step_kernel(rule, kind, dt, mode):
    tr, _ = _against_the_one_step_kernel(rule, dt, mode, 8, True, trace_decay=0.0, trace_length=4, trace_kind=kind)
    assert not tr["values"].any() and not tr["states"].any() and not tr["actions"].any()


@pytest.mark.parametrize(("A", "masked"), [(4, False), (64, True)])
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("rule", RULES)
def test_one_replacing_slot_is_the_one_step_kernel(rule, dt, mode, A, masked):
    tr, _ = _against_the_one_step_kernel(rule, dt, mode, A, masked, S=5, trace_decay=0.9, trace_length=1)
    assert tr["values"].any()


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [(8, False, np.float32, "iter"), (8, True, np.float64, "vec"),
                                                         (16, True, np.float32, "vec")])
@pytest.mark.parametrize(("kw", "live"), [({"trace_decay": 0.0, "trace_length": 8, "trace_kind": "accumulating"}, False),
                                          ({"trace_decay": 0.9, "trace_length": 1}, True)])
@pytest.mark.parametrize("rule", RULES)
def test_nan_and_infinite_tables_equal_the_one_step_kernel(rule, kw, live, A, masked, dt, mode):
    q0 = _special_tables(M_ODD, 30, A, dt, seed=A)
    tr, keep = _against_the_one_step_kernel(rule, dt, mode, A, masked, S=30, steps=60, q0=q0, **kw)
    assert tr["values"][keep].any() == live
    # the conditions of the siblings' NaN cases: some run is stuck, and some run that is compared starts from special cells
    assert len(keep) < M_ODD, "no run met a row without a selectable action"
    assert not np.isfinite(q0[keep]).all(), "no compared run has a NaN or an infinity in its table"


# ---- 2. against the model: every row width, both dtypes, both learn modes; kinds and slot counts ---------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [4, 8, 16, 64])
@pytest.mark.parametrize("rule", RULES)
def test_hash_runs_match_the_model(rule, A, masked, dt, mode):
    p = {"S": 300, "A": A, "seed": 1, "masked": masked}
    _run_and_check("hash", p, 300, A, M_ODD, 150, rule, dt, mode, _schedules(M_ODD), nv=_nv(A), masked=masked)


@pytest.mark.parametrize(("K", "tkind", "dt", "mode"), [
    (8, "accumulating", np.float32, "iter"), (8, "accumulating", np.float64, "vec"), (8, "accumulating", np.float32, "vec"),
    (2, "replacing", np.float32, "vec"), (2, "accumulating", np.float64, "iter"),
    (32, "replacing", np.float64, "iter"), (32, "accumulating", np.float32, "iter"), (32, "replacing", np.float64, "vec")])
@pytest.mark.parametrize("rule", RULES)
def test_kinds_and_slot_counts_match_the_model(rule, K, tkind, dt, mode):
    p = {"S": 300, "A": 8, "seed": 1, "masked": True}
    _, res = _run_and_check("hash", p, 300, 8, M_ODD, 150, rule, dt, mode, _schedules(M_ODD), K=K, tkind=tkind, nv=2, masked=True)
    live = (res.state_dict["eligibility_traces"]["values"] != 0).sum(axis=1)
    if rule == "sarsa":
        assert live.max() == K and live.min() <= 1  # lambda = 1 keeps every slot busy, lambda = 0 none
    else:
        assert live.max() > 1


# ---- 3. eviction and recurrence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("tkind", KINDS)
@pytest.mark.parametrize("rule", RULES)
def test_six_cells_for_four_slots(rule, tkind, dt, mode):
    """S = 3, A = 2: every step finds its cell, evicts one or patches a store into the row it holds."""
    p = {"S": 3, "A": 2, "seed": 1, "masked": False}
    _, res = _run_and_check("hash", p, 3, 2, M_ODD, 150, rule, dt, mode, _schedules(M_ODD), K=4, tkind=tkind, nv=1, masked=False)
    if rule == "sarsa":
        assert ((res.state_dict["eligibility_traces"]["values"] != 0).sum(axis=1) == 4).any()


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("rule", RULES)
def test_accumulating_traces_on_the_bandit_grow_past_one(rule, dt, mode):
    p = {"episode_len": 50}
    _, res = _run_and_check("bandit", p, 1, 2, M_ODD, 140, rule, dt, mode, _schedules(M_ODD), K=2, tkind="accumulating", seed=11,
                            nv=1, masked=False)
    assert res.state_dict["eligibility_traces"]["values"].max() > 1


# ---- 4. episodes: a terminated step frees every slot ------------------------------------------------------------------------
def _other(kind):
    """(S, A, parameters, NV, masked)"""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp
    from table_mdp_model import random_mdp

    if kind == "grid":
        return 36, 4, {"side": 6, "seed": 2}, 1, False
    if kind == "bandit":  # 150 steps = 50 whole episodes: the call ends on a terminated step
        return 1, 2, {"episode_len": 3}, 1, False
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
    _, res = _run_and_check(kind, p, S, A, M_ODD, 150, rule, dt, mode, _schedules(M_ODD), K=6, seed=11, nv=nv, masked=masked)
    assert res.episode_counts.sum() > 0
    if kind == "bandit":
        assert not res.state_dict["eligibility_traces"]["values"].any()  # after a terminated final step


# ---- 5. underflow: traces pass through the denormal range and free their slots ---------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_traces_underflow_through_denormals_to_free_slots(rule):
    """gamma * lambda = 2^-20 on a float32 table: 1, 2^-20, ... 2^-140 (a denormal), then 0 -- a slot is free again
    after 8 steps, so at most 8 of the 16 are ever live."""
    M = M_ODD
    eps_s, lr_s, _ = _schedules(M)
    sched = (eps_s, lr_s, [2.0 ** -10] * M)
    p = {"S": 300, "A": 8, "seed": 1, "masked": False}
    _, res = _run_and_check("hash", p, 300, 8, M, 150, rule, np.float32, "iter", sched, K=16, lam=[2.0 ** -10] * M, nv=2, masked=False)
    values = res.state_dict["eligibility_traces"]["values"]
    assert ((values != 0).sum(axis=1) <= 8).all()
    assert ((values > 0) & (values < 2.0 ** -126)).any(), "no trace is a denormal at the end of the call"


# ---- 6. chaining: calls, a fresh process, calls shorter than the slots; launch chopping ------------------------------------
@pytest.mark.parametrize("S", [4, 400])  # four states: s' == s_i at many call boundaries
@pytest.mark.parametrize("rule", RULES)
def test_calls_and_a_restored_population_equal_one_call(rule, S, tmp_path):
    envs = _product()[1]
    M, A, steps, K = M_ODD, 8, 90, 8
    sched = _schedules(M)
    lam = _lambdas(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter", rule, trace_decay=lam, trace_length=K, trace_kind="accumulating")

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * steps, env())
    halves = make()
    e = env()
    first = halves.run_steps(steps, e)
    assert (first.state_dict["eligibility_traces"]["values"] != 0).any(), "the slots must be non-empty at the cut"
    halves.save(tmp_path / "tables.npy")
    blob = pickle.dumps(first.state_dict)
    second = halves.run_steps(steps, e, first.state_dict)
    restored = make()  # what a fresh process does: tables from the file, everything else from the pickled dict
    sd = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.restore_training_state(sd)
    for key, value in restored.eligibility_traces.items():
        assert np.array_equal(value, first.state_dict["eligibility_traces"][key]), key
    third = restored.run_steps(steps, env(), sd)
    short = make()  # 60 calls of 3 steps: every call is shorter than the slot count
    e3, sd3, pieces = env(), None, []
    for _ in range(2 * steps // 3):
        res3 = short.run_steps(3, e3, sd3) if sd3 is not None else short.run_steps(3, e3)
        sd3 = res3.state_dict
        pieces.append(res3)
    for pop in (whole, halves, restored, short):
        _reached(pop, rule, K, "accumulating", nv=2, masked=True)
        assert np.array_equal(pop.q_tables, whole.q_tables)
        assert np.array_equal(pop.step_counters, np.full(M, 2 * steps))
    for tail in (second, third):
        for r in range(M):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), one.run_returns(r)), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + steps]), one.run_steps(r)), r
        _same_state(tail.state_dict, one.state_dict)
    _same_state(sd3, one.state_dict)
    for r in range(M):
        assert np.array_equal(np.concatenate([x.run_returns(r) for x in pieces]), one.run_returns(r)), r
        assert np.array_equal(np.concatenate([x.run_steps(r) + 3 * i for i, x in enumerate(pieces)]), one.run_steps(r)), r
    # a dict without the key: every slot starts free (the model, told so)
    lost = make()
    lost.load(tmp_path / "tables.npy")
    stripped = {k: v for k, v in sd.items() if k != "eligibility_traces"}
    lost.restore_training_state(stripped)
    assert not lost.eligibility_traces["values"].any()
    res = lost.run_steps(steps, env(), stripped)
    tables = lost.q_tables
    assert not np.array_equal(tables, whole.q_tables)
    p = {"S": S, "A": A, "seed": 9, "masked": True}
    for r, run in _model_runs("hash", p, range(M), rule, lam, K, "accumulating", sched, 4, np.float32, "iter").items():
        run.run(steps)
        run.rt.clear()
        history, at = run.run(steps)
        _check(lost, res, r, run, history, at, tables, 2 * steps)


@pytest.mark.parametrize("rule", RULES)
def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_and_the_model(rule):
    envs = _product()[1]
    M, steps, S, A, K = 40_000, 2000, 100, 8, 4
    eps0, lr0, gamma0 = _schedules(97)
    sched = [[x[r % 97] for r in range(M)] for x in (eps0, lr0, gamma0)]
    lam = _lambdas(M)
    kw = {"trace_decay": lam, "trace_length": K}
    logged = _population(M, S, A, sched, 21, np.float32, "vec", rule, **kw)
    res = logged.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1))
    _reached(logged, rule, K, nv=2, masked=False)
    assert logged.last_stats["launches"] > 9, "the logged call must be cut into more than three launches"
    tables = logged.q_tables
    quiet = _population(M, S, A, sched, 21, np.float32, "vec", rule, **kw)
    res_q = quiet.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1), log=False)
    assert 1 < quiet.last_stats["launches"] < logged.last_stats["launches"] // 3, "the unlogged call is cut differently"
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    _same_state(res_q.state_dict, res.state_dict)
    del quiet
    p = {"S": S, "A": A, "seed": 1, "masked": False}
    picked = [0, 1, 63, 64, 20_000, M - 1]
    for r, run in _model_runs("hash", p, picked, rule, lam, K, "replacing", sched, 21, np.float32, "vec").items():
        history, at = run.run(steps)
        _check(logged, res, r, run, history, at, {r: tables[r]}, steps)


# ---- 7. evaluation and train() ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_evaluation_between_training_calls_leaves_the_slots_and_the_training_alone(rule):
    envs = _product()[1]
    M, S, A, K = M_ODD, 50, 8, 8
    sched = _schedules(M)
    lam = _lambdas(M)

    def make():
        return _population(M, S, A, sched, 6, np.float64, "iter", rule, trace_decay=lam, trace_length=K)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=2, masked=True)

    straight, e1 = make(), env()
    a1 = straight.run_steps(70, e1)
    a2 = straight.run_steps(70, e1, a1.state_dict)
    paused, e2 = make(), env()
    b1 = paused.run_steps(70, e2)
    before = paused.eligibility_traces
    assert before["values"].any()
    paused.evaluate_steps(envs.HashTabularEnv(M, S, A, seed=5, masked=True), 40)
    assert _product()[0].decode_variant(paused.last_stats["kernel_variant"])["path"] == "population_eval"
    for key, value in paused.eligibility_traces.items():
        assert np.array_equal(value, before[key]), key
    paused.step_counter = 70  # (the evaluation drew 40 steps: back to where training stood)
    b2 = paused.run_steps(70, e2, b1.state_dict)
    assert np.array_equal(paused.q_tables, straight.q_tables)
    _same_state(b2.state_dict, a2.state_dict)
    for r in range(M):
        assert np.array_equal(b2.run_returns(r), a2.run_returns(r)), r


@pytest.mark.parametrize("rule", RULES)
def test_train_with_episode_validation_matches_the_model_driven_the_same_way(rule):
    from table_mdp_model import TableMDPVecEnv
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)  # every move may end the episode: greedy validation episodes end too
    M, S, A, seg, n_seg, val_episodes, K = M_ODD, mdp.state_size, mdp.action_size, 60, 3, 2, 6
    sched = _schedules(M)
    lam = _lambdas(M)
    pop = _population(M, S, A, sched, 8, np.float64, "iter", rule, trace_decay=lam, trace_length=K)
    out = pop.train(envs.TabularMDPEnv(M, mdp, seed=1), seg * n_seg, envs.TabularMDPEnv(M, mdp, seed=5), seg,
                    val_episodes=val_episodes)
    assert _product()[0].decode_variant(pop.last_stats["kernel_variant"])["path"] == "population_eval"
    assert out.val_finished.all()
    tables = pop.q_tables
    counters = pop.step_counters
    assert len(set(counters.tolist())) > 1, "the validations must leave the runs at different counters"
    pt = {"mdp": mdp, "seed": 1}
    slots = pop.eligibility_traces  # greedy evaluation neither reads nor clears them
    for r, run in _model_runs("table", pt, range(M), rule, lam, K, "replacing", sched, 8, np.float64, "iter").items():
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
        states, actions, values = run.slots
        for tr in (slots, out.state_dict["eligibility_traces"]):
            assert np.array_equal(tr["states"][r], states) and np.array_equal(tr["actions"][r], actions), r
            assert np.array_equal(tr["values"][r], values), r


# ---- 8. traces off is untouched; the setter; refusals on a live engine ------------------------------------------------------
@pytest.mark.parametrize(("rule", "variant"), [("q_learning", 6), ("sarsa", 8 | (1 << 4))])
def test_no_trace_decay_is_the_default_path(rule, variant):
    _, envs, _, QLearningPopulation = _product()
    got = []
    for kw in ({}, {"trace_decay": None, "trace_length": 4, "trace_kind": "accumulating"}):
        pop = QLearningPopulation(M_ODD, 100, 16, seed=2, dtype=np.float32, update_rule=rule, **kw)
        res = pop.run_steps(50, envs.HashTabularEnv(M_ODD, 100, 16, seed=1, masked=True))
        got.append((pop.last_stats["kernel_variant"], pop.q_tables, sorted(res.state_dict)))
        assert "eligibility_traces" not in res.state_dict and pop.eligibility_traces is None and pop.trace_decay is None
    assert got[0][0] == got[1][0] == variant | (4 << 12) | (1 << 20)
    assert np.array_equal(got[0][1], got[1][1]) and got[0][1].any() and got[0][2] == got[1][2]


def test_the_setter_and_the_refusals():
    _lib, envs, _, QLearningPopulation = _product()
    lib = _lib.load()
    i32 = lambda a: _lib.ptr(a, C.c_int32)  # noqa: E731
    f64 = lambda a: _lib.ptr(a, C.c_double)  # noqa: E731
    M, S, A, K = 8, 50, 4, 3
    lam = np.full(M, 0.5)
    # C: on a population without traces; refusals while another multi-step method or rule is on, and the converse
    plain = QLearningPopulation(M, S, A)
    assert lib.qe_population_trace_config(plain.handle, None, None, None) == 0
    assert lib.qe_population_traces(plain.handle, None, None, None) == _lib.ERR_INVALID
    assert "traces are off" in lib.qe_last_error().decode()
    assert lib.qe_population_set_trace_state(plain.handle, None, None, None) == _lib.ERR_INVALID
    for k, kind in ((0, 0), (33, 0), (4, 2), (4, -1)):
        assert lib.qe_population_set_traces(plain.handle, k, kind, f64(lam)) == _lib.ERR_INVALID
    for bad in (-0.1, 1.5, np.nan, np.inf):
        assert lib.qe_population_set_traces(plain.handle, 4, 0, f64(np.array([0.5] * 7 + [bad]))) == _lib.ERR_UNSUPPORTED
        assert "lambda" in lib.qe_last_error().decode()
    big = QLearningPopulation(M, S, A, discount_factor=1.5)
    assert lib.qe_population_set_traces(big.handle, 4, 0, f64(np.full(M, 0.9))) == _lib.ERR_UNSUPPORTED
    assert "outside [0, 1]" in lib.qe_last_error().decode()
    assert lib.qe_population_set_traces(big.handle, 4, 0, f64(lam)) == 0  # 0.75
    for kw in ({"update_rule": "expected_sarsa"}, {"double_q": True}, {"update_rule": "sarsa", "n_step": 3}):
        other = QLearningPopulation(M, S, A, **kw)
        assert lib.qe_population_set_traces(other.handle, 4, 0, f64(lam)) == _lib.ERR_UNSUPPORTED
        assert lib.qe_population_trace_config(other.handle, None, None, None) == 0
    pop = QLearningPopulation(M, S, A, update_rule="sarsa", trace_decay=0.5, trace_length=K, dtype=np.float32)
    k_out, kind_out, lam_out = C.c_int32(), C.c_int32(), np.zeros(M)
    assert lib.qe_population_trace_config(pop.handle, C.byref(k_out), C.byref(kind_out), f64(lam_out)) == 1
    assert (k_out.value, kind_out.value) == (K, 0) and np.array_equal(lam_out, lam)
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_EXPECTED_SARSA) == _lib.ERR_UNSUPPORTED
    assert "policy-probability weighting" in lib.qe_last_error().decode()
    assert lib.qe_population_set_double(pop.handle, 1) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_n_step(pop.handle, 2) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_Q_LEARNING) == 0
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_SARSA) == 0
    assert lib.qe_population_n_step(pop.handle) == 1 and lib.qe_population_update_rule(pop.handle) == _lib.RULE_SARSA
    # the setter
    tr = pop.eligibility_traces
    assert not tr["values"].any() and tr["states"].shape == (M, K)
    good = {"states": np.arange(M * K).reshape(M, K) % S, "actions": np.arange(M * K).reshape(M, K) % A,
            "values": np.tile([1.0, 0.0, 2.0 ** -140], (M, 1))}
    pop.eligibility_traces = good
    back = pop.eligibility_traces
    live = good["values"] != 0
    assert np.array_equal(back["values"], good["values"])
    assert np.array_equal(back["states"], np.where(live, good["states"], 0)) and np.array_equal(back["actions"], np.where(live, good["actions"], 0))
    twice = good["states"].copy(), good["actions"].copy()
    twice[0][5, 2], twice[1][5, 2] = twice[0][5, 0], twice[1][5, 0]
    for key, value, text in (("states", np.full((M, K), S), "state 50 is outside"), ("states", np.full((M, K), -1), "state -1"),
                             ("actions", np.full((M, K), A), "action 4 is outside"),
                             ("values", np.full((M, K), -1.0), "negative"), ("values", np.full((M, K), np.nan), "not finite"),
                             ("values", np.full((M, K), np.inf), "not finite"), ("values", np.full((M, K), 0.1), "not a float32"),
                             ("values", np.full((M, K), 1e-60), "not a float32"), ("states", twice[0], "name the same cell")):
        bad = dict(good, **{key: value})
        if key == "states" and value is twice[0]:
            bad["actions"] = twice[1]
        with pytest.raises(ValueError, match=text):
            pop.eligibility_traces = bad
        assert lib.qe_population_set_trace_state(pop.handle, i32(np.ascontiguousarray(bad["states"], dtype=np.int32)),
                                                 i32(np.ascontiguousarray(bad["actions"], dtype=np.int32)),
                                                 f64(np.ascontiguousarray(bad["values"], dtype=np.float64))) == _lib.ERR_INVALID
    free_twice = dict(good, states=np.zeros((M, K), dtype=np.int32), actions=np.zeros((M, K), dtype=np.int32),
                      values=np.tile([0.0, 0.0, 1.0], (M, 1)))
    pop.eligibility_traces = free_twice  # free slots name no cell: nothing collides
    pop.eligibility_traces = good
    for bad in (dict(good, states=np.zeros((M, K + 1), dtype=np.int32)), dict(good, values=np.zeros((M, K), dtype=complex)),
                {"states": good["states"]}, [1, 2]):
        with pytest.raises(ValueError, match="eligibility_traces"):
            pop.eligibility_traces = bad
    assert np.array_equal(pop.eligibility_traces["values"], good["values"])  # a refused state changes nothing
    z = np.zeros((M, K), dtype=np.int32)
    assert lib.qe_population_set_trace_state(pop.handle, i32(z), None, None) == _lib.ERR_INVALID
    pop.eligibility_traces = None
    assert not pop.eligibility_traces["values"].any()
    res = pop.run_steps(10, envs.HashTabularEnv(M, S, A))
    assert res.state_dict["eligibility_traces"]["values"].any()
    # greedy evaluation neither reads nor clears the slots; setting traces frees them; off gives the one-step kernel back
    before = pop.eligibility_traces
    pop.evaluate_steps(envs.HashTabularEnv(M, S, A, seed=5), 30)
    pop.evaluate_episodes(envs.HashTabularEnv(M, S, A, seed=5), 1)
    for key, value in pop.eligibility_traces.items():
        assert np.array_equal(value, before[key]), key
    assert lib.qe_population_set_traces(pop.handle, 5, 1, f64(lam)) == 0
    out = np.ones((M, 5))
    assert lib.qe_population_traces(pop.handle, None, None, f64(out)) == 0 and not out.any()
    assert lib.qe_population_set_traces(pop.handle, 0, 0, None) == 0 and lib.qe_population_trace_config(pop.handle, None, None, None) == 0
    assert lib.qe_population_set_n_step(pop.handle, 2) == 0
