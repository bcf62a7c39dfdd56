"""GPU: ``QLearningPopulation(exploration_bonus=..., visit_lr=...)`` (k_visit_rollout) against the NumPy model of the
visit counts (tests/visit_model.py), bit for bit.

Per run: the table, the counts, the ``visit_bonus`` plane (also against the NumPy formula applied to the counts), the
episode returns and their steps, the episode counts and means, the final observation / env word / running return, the
schedule values and the draw counter.  No tolerance anywhere.  Every case asserts the kernel build it means to cover (path
14, NV, masked and the two flag bits).
"""
import copy
import pickle

import numpy as np
import pytest

from test_gpu_population import _schedules
from test_gpu_td_rules import _check as _check_td
from test_gpu_td_rules import _device_env, _model_env, _nv, _product, _special_tables
from visit_model import VISIT_MAX, VisitRun, bonus

pytestmark = pytest.mark.gpu

M_ODD = 67  # a full and a partial wavefront
BETAS = (0.0, 0.05, 0.5, 4.0)


def _betas(M):
    return [BETAS[r % 4] for r in range(M)]


def _reached(pop, nv=None, masked=None):
    v = pop.last_stats["kernel_variant"]
    d = _product()[0].decode_variant(v)
    assert v & 15 == 14 and d["path"] == "population_visit" and d["rule"] == "q_learning" == pop.update_rule, d
    assert d["visit_lr"] == pop.visit_lr == bool((v >> 4) & 1), d
    assert d["bonus"] == bool((pop.exploration_bonus > 0).any()) == bool((v >> 5) & 1), d
    assert d["n_step"] == 1 and d["trace_length"] == 0 and "planning_steps" not in d, d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d


def _same_bits(a, b):
    """Bit for bit, except that a NaN equals any NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) | np.isnan(a), np.signbit(b) | np.isnan(b))


def _check_planes(pop, counts, plane):
    """The invariant B == bonus(beta, N) in every cell, by the NumPy formula."""
    assert counts.dtype == np.uint32 and counts.shape == (pop.runs, pop.state_size, pop.action_size)
    assert plane.dtype == pop.dtype and plane.shape == counts.shape
    for r in range(pop.runs):
        assert _same_bits(plane[r], bonus(pop.exploration_bonus[r], counts[r], pop.dtype)), f"run {r}: bonus plane vs formula"


def _check(pop, res, r, run, history, at, tables, counter, counts, plane):
    """Run r of a population call against its model run (after the same call)."""
    _check_td(pop, res, r, run, history, at, tables, counter)
    assert np.array_equal(counts[r], run.counts), f"run {r}: counts"
    assert _same_bits(plane[r], run.bonus), f"run {r}: bonus plane"


def _model_runs(kind, p, runs, sched, seed, dt, mode, betas, visit_lr, q0=None, n0=None):
    eps_s, lr_s, gamma = sched
    return {r: VisitRun(_model_env(kind, r, p), gamma[r], eps_s[r], lr_s[r], beta=betas[r], visit_lr=visit_lr, seed=seed, dtype=dt,
                        mode=mode, agent_id=r, q0=None if q0 is None else q0[r], n0=None if n0 is None else n0[r]) for r in runs}


def _population(M, S, A, sched, seed, dt, mode, **kw):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode, **kw)


def _run_flagged(pop, K, env, state=None):
    try:
        return pop.run_steps(K, env, state), []
    except IndexError as err:
        return err.result, err.runs


def _run_and_check(kind, p, S, A, M, K, dt, mode, sched, visit_lr, seed=0, nv=None, masked=None, q0=None, flagged_cap=0):
    """One call against the model.  ``flagged_cap``: how many runs the MODEL may flag (no selectable action); the device
    must flag exactly those, and every other run is compared."""
    betas = _betas(M)
    if not _product()[0].visit_build_shipped(np.dtype(dt), A):  # a shape DESIGN lists as refused: the refusal instead
        with pytest.raises(ValueError, match="is not built"):
            _population(M, S, A, sched, seed, dt, mode, exploration_bonus=betas, visit_lr=visit_lr)
        return None
    pop = _population(M, S, A, sched, seed, dt, mode, exploration_bonus=betas, visit_lr=visit_lr)
    if q0 is not None:
        pop.set_q_tables(q0)
    res, raised = _run_flagged(pop, K, _device_env(kind, M, p))
    _reached(pop, nv=nv, masked=masked)
    assert "visit_counts" not in res.state_dict and "visit_bonus" not in res.state_dict
    tables, counts, plane = pop.q_tables, pop.visit_counts, pop.visit_bonus
    _check_planes(pop, counts, plane)
    assert np.array_equal(counts.sum(axis=(1, 2), dtype=np.uint64), np.full(M, K))
    want_raised = []
    for r, run in _model_runs(kind, p, range(M), sched, seed, dt, mode, betas, visit_lr, q0=q0).items():
        try:
            history, at = run.run(K)
        except IndexError:  # (a run without a selectable action is on its own from there on)
            want_raised.append(r)
            continue
        _check(pop, res, r, run, history, at, tables, K, counts, plane)
    assert raised == want_raised, "the device flags exactly the runs the model flags"
    assert len(want_raised) <= flagged_cap, f"the model flags {len(want_raised)} runs: the case hides too much"
    return pop, res, want_raised


# ---- 1. every row width, masked and not, both dtypes, both learn modes ---------------------------------------------------------
_WIDTHS = [(A, masked, dt, mode) for A in (4, 8, 16, 64) for masked in (False, True) for dt in (np.float32, np.float64)
           for mode in ("iter", "vec")]


@pytest.mark.parametrize(("case", "A", "masked", "dt", "mode"), [(i, *c) for i, c in enumerate(_WIDTHS)])
def test_hash_runs_match_the_model(case, A, masked, dt, mode):
    """(In the masked hash environment action 0 is always valid: no run may be flagged.)"""
    p = {"S": 300, "A": A, "seed": 1, "masked": masked}
    _run_and_check("hash", p, 300, A, M_ODD, 150, dt, mode, _schedules(M_ODD), visit_lr=(case + case // 2) % 2 == 1, nv=_nv(A),
                   masked=masked)


@pytest.mark.parametrize(("dt", "visit_lr"), [(np.float32, True), (np.float64, False)])
def test_the_32_column_build_matches_the_model(dt, visit_lr):
    p = {"S": 300, "A": 20, "seed": 1, "masked": True}
    _run_and_check("hash", p, 300, 20, M_ODD, 150, dt, "iter", _schedules(M_ODD), visit_lr=visit_lr, nv=8, masked=True)


# ---- 2. the other environments --------------------------------------------------------------------------------------------------
TABLE_STATES, TABLE_SEED, DEAD_STATE, TABLE_STEPS = 60, 8, 9, 100


def dead_row_mdp():
    """A stochastic masked 60 x 5 MDP with one state whose mask row is all invalid.  Seed and state were chosen on the CPU
    so that the model alone flags 10 of 67 runs within 100 steps, in each of the four cases below."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp
    from table_mdp_model import random_mdp

    arrays, isd, masks = random_mdp(TABLE_STATES, 5, 3, seed=TABLE_SEED, masked=True)
    masks = np.array(masks, dtype=bool)
    masks[DEAD_STATE] = False
    return encode_table_mdp(*arrays, isd, masks)


def _other(kind):
    """(S, A, parameters, NV, masked, steps)"""
    if kind == "grid":  # s' == s on the walls: the held-B patch fires
        return 36, 4, {"side": 6, "seed": 2}, 1, False, 150
    if kind == "bandit":  # every step is s' == s
        return 1, 2, {"episode_len": 7}, 1, False, 150
    if kind == "tictactoe":  # (the model copes slowly with 19 683 x 9 cells per run)
        return 19683, 9, {"seed": 5}, 4, True, 60
    return TABLE_STATES, 5, {"mdp": dead_row_mdp(), "seed": 3}, 2, True, TABLE_STEPS


@pytest.mark.parametrize("visit_lr", [False, True])
@pytest.mark.parametrize(("dt", "mode"), [(np.float32, "iter"), (np.float64, "vec")])
@pytest.mark.parametrize("kind", ["grid", "bandit", "tictactoe"])
def test_other_environments_match_the_model(kind, dt, mode, visit_lr):
    S, A, p, nv, masked, steps = _other(kind)
    _, res, _ = _run_and_check(kind, p, S, A, M_ODD, steps, dt, mode, _schedules(M_ODD), visit_lr, seed=11, nv=nv, masked=masked)
    assert res.episode_counts.sum() > 0


@pytest.mark.parametrize(("dt", "mode", "visit_lr"), [(np.float32, "iter", False), (np.float64, "vec", True),
                                                      (np.float32, "vec", True), (np.float64, "iter", False)])
def test_a_table_mdp_with_an_empty_mask_row_names_its_runs_and_the_others_match(dt, mode, visit_lr):
    """The model alone flags at most a quarter of the runs (checked on the CPU when the MDP, the dead state and the step
    count were chosen: 10 of 67 in each of the four cases)."""
    S, A, p, nv, masked, steps = _other("table")
    _, res, flagged = _run_and_check("table", p, S, A, M_ODD, steps, dt, mode, _schedules(M_ODD), visit_lr, seed=11, nv=nv,
                                     masked=masked, flagged_cap=M_ODD // 4)
    assert flagged, "no run met the row without a valid action"
    assert res.episode_counts.sum() > 0


# ---- 3. identity against the merged kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize(("A", "masked"), [(8, False), (16, True)])
def test_zero_bonus_without_the_rate_is_the_plain_population(A, masked, dt, mode):
    envs = _product()[1]
    M, S, K = M_ODD, 30, 100
    sched = _schedules(M)
    q0 = _special_tables(M, S, A, dt, seed=A)  # NaN and +-inf cells
    got = []
    for kw in ({}, {"exploration_bonus": 0.0, "visit_lr": False}):
        pop = _population(M, S, A, sched, 5, dt, mode, **kw)
        pop.set_q_tables(q0)
        res, raised = _run_flagged(pop, K, envs.HashTabularEnv(M, S, A, seed=1, masked=masked))
        got.append((pop, res, raised, pop.q_tables))
    (plain, a, raised_a, qa), (counting, b, raised_b, qb) = got
    assert plain.last_stats["kernel_variant"] == 6 | (_nv(A) << 12) | (int(masked) << 20)
    assert plain.visit_counts is None and plain.visit_bonus is None and not plain.counting
    _reached(counting, nv=_nv(A), masked=masked)
    assert counting.last_stats["kernel_variant"] == 14 | (_nv(A) << 12) | (int(masked) << 20)
    assert raised_a == raised_b
    # (a flagged run continues at action 0 on both kernels, so every run is compared, flagged or not)
    assert len(raised_a) < M
    assert np.array_equal(qa, qb, equal_nan=True) and not np.array_equal(qa, q0, equal_nan=True)
    assert np.array_equal(a.returns, b.returns) and np.array_equal(a.steps, b.steps) and np.array_equal(a.offsets, b.offsets)
    assert np.array_equal(a.episode_counts, b.episode_counts) and np.array_equal(a.mean_returns, b.mean_returns, equal_nan=True)
    assert sorted(a.state_dict) == sorted(b.state_dict)
    for key in a.state_dict:
        assert np.array_equal(a.state_dict[key], b.state_dict[key]), key
    assert np.array_equal(plain.step_counters, counting.step_counters)
    assert np.array_equal(counting.visit_counts.sum(axis=(1, 2)), np.full(M, K))
    assert not counting.visit_bonus.any()


# ---- 4. the bonus function on the device ------------------------------------------------------------------------------------------
COUNTS = (0, 1, 2, 3, 5, 7, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_bonus_plane_is_the_numpy_formula_and_the_counts_saturate(dt):
    envs = _product()[1]
    betas = [0.0, 1e-3, 0.5, 3.0]
    M, S, A = len(betas), 1, 2
    pop = _population(M, S, A, ([_product()[2].ConstantSchedule(0.2)] * M, [_product()[2].ConstantSchedule(0.5)] * M, [0.9] * M), 3, dt,
                      "iter", exploration_bonus=betas, visit_lr=True)
    for first in range(0, len(COUNTS), 2):
        n = np.empty((M, S, A), dtype=np.uint64)
        n[:, 0, 0], n[:, 0, 1] = COUNTS[first], COUNTS[first + 1]
        pop.visit_counts = n
        assert np.array_equal(pop.visit_counts, n.astype(np.uint32))
        plane = pop.visit_bonus
        _check_planes(pop, pop.visit_counts, plane)
        for r, beta in enumerate(betas):
            with np.errstate(all="ignore"):
                want = [dt(0) if beta == 0 else dt(np.float64(beta) / np.sqrt(np.float64(c))) for c in COUNTS[first:first + 2]]
            assert plane[r, 0].tolist() == [float(w) for w in want], (r, first)
    # five steps on the bandit from 2^32 - 2: the counts stop at 2^32 - 1
    n0 = np.full((M, S, A), VISIT_MAX - 1, dtype=np.uint32)
    pop.visit_counts = n0
    res = pop.run_steps(5, envs.RiggedTwoArmedBanditVecEnv(M, episode_len=7))
    _reached(pop, nv=1, masked=False)
    tables, counts, plane = pop.q_tables, pop.visit_counts, pop.visit_bonus
    _check_planes(pop, counts, plane)
    assert counts.max() == VISIT_MAX and counts.min() >= VISIT_MAX - 1
    sched = ([_product()[2].ConstantSchedule(0.2)] * M, [_product()[2].ConstantSchedule(0.5)] * M, [0.9] * M)
    for r, run in _model_runs("bandit", {"episode_len": 7}, range(M), sched, 3, dt, "iter", betas, True, n0=n0).items():
        history, at = run.run(5)
        _check(pop, res, r, run, history, at, tables, 5, counts, plane)


# ---- 5. scores that go NaN ------------------------------------------------------------------------------------------------------------
def _nan_score_tables(M, S, A, dt, seed):
    """Random tables with -inf cells (score -inf + inf = NaN while the cell is untried) and NaN cells in every run."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((M, S, A)).astype(dt)
    for r in range(M):
        for count, value in ((2 + r % 5, -np.inf), (r % 4, np.nan), (r % 3, np.inf)):
            q[r].ravel()[rng.choice(S * A, size=count, replace=False)] = value
    return q


@pytest.mark.parametrize(("A", "masked", "S", "dt", "mode", "visit_lr"), [
    (8, False, 30, np.float32, "iter", False),   # list selection: steps over NaN
    (8, True, 30, np.float64, "vec", True),      # list selection, masked: 7 runs meet a row without a candidate
    (16, False, 30, np.float64, "iter", True),   # unmasked, one agent: the list selection at every width
    # NumPy-style selection: a NaN in a valid column of the score row leaves no candidate.  300 states, so that most
    # runs never meet such a row (the model flags 19 of 67; with 30 states it flags 54)
    (16, True, 300, np.float32, "vec", False),
])
def test_scores_that_go_nan_match_the_model(A, masked, S, dt, mode, visit_lr):
    M, K = M_ODD, 100
    q0 = _nan_score_tables(M, S, A, dt, seed=A)
    p = {"S": S, "A": A, "seed": 1, "masked": masked}
    # (a run whose score row offers no candidate is flagged by model and device alike; two thirds must remain: the model flags at most 19 of 67)
    pop, _, flagged = _run_and_check("hash", p, S, A, M, K, dt, mode, _schedules(M), visit_lr, nv=_nv(A), masked=masked, q0=q0,
                                     flagged_cap=M // 3)
    assert not np.isfinite(pop.q_tables).all()
    assert bool(flagged) == masked


# ---- 6. chaining and resume --------------------------------------------------------------------------------------------------------
def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for key in b:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize(("S", "visit_lr"), [(4, True), (400, False)])
def test_calls_and_a_restored_population_equal_one_call(S, visit_lr, tmp_path):
    envs = _product()[1]
    M, A, K = M_ODD, 8, 60
    sched = _schedules(M)

    def make():
        return _population(M, S, A, sched, 4, np.float32, "iter", exploration_bonus=_betas(M), visit_lr=visit_lr)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=9, masked=True)

    whole = make()
    one = whole.run_steps(2 * K, env())
    halves = make()
    e = env()
    first = halves.run_steps(K, e)
    at_cut = halves.visit_counts
    assert np.array_equal(at_cut.sum(axis=(1, 2)), np.full(M, K))
    halves.save(tmp_path / "tables.npy")
    blob = pickle.dumps((first.state_dict, at_cut))
    second = halves.run_steps(K, e, first.state_dict)
    restored = make()  # what a fresh process does: tables from their file, counts and the rest from the pickle
    sd, counts = pickle.loads(blob)
    restored.load(tmp_path / "tables.npy")
    restored.visit_counts = counts
    restored.restore_training_state(sd)
    assert np.array_equal(restored.visit_counts, at_cut)
    _check_planes(restored, restored.visit_counts, restored.visit_bonus)
    third = restored.run_steps(K, env(), sd)
    for pop in (whole, halves, restored):
        _reached(pop, nv=2, masked=True)
        assert np.array_equal(pop.q_tables, whole.q_tables)
        assert np.array_equal(pop.step_counters, np.full(M, 2 * K))
        assert np.array_equal(pop.visit_counts, whole.visit_counts)
        assert _same_bits(pop.visit_bonus, whole.visit_bonus)
    for tail in (second, third):
        for r in range(M):
            assert np.array_equal(np.concatenate([first.run_returns(r), tail.run_returns(r)]), one.run_returns(r)), r
            assert np.array_equal(np.concatenate([first.run_steps(r), tail.run_steps(r) + K]), one.run_steps(r)), r
        _same_state(tail.state_dict, one.state_dict)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_reset_keeps_the_counts_and_the_none_setter_forgets_them(dt):
    M, S, A, K = M_ODD, 30, 8, 60
    sched = _schedules(M)
    betas = _betas(M)
    p = {"S": S, "A": A, "seed": 2, "masked": False}
    pop = _population(M, S, A, sched, 6, dt, "vec", exploration_bonus=betas, visit_lr=True)
    e = _device_env("hash", M, p)
    pop.run_steps(K, e)
    kept = pop.visit_counts
    res = pop.run_steps(K, e)  # curr_state_dict=None: the environment is reset, the counts stay
    _reached(pop, nv=2, masked=False)
    tables, counts, plane = pop.q_tables, pop.visit_counts, pop.visit_bonus
    assert np.array_equal(counts.sum(axis=(1, 2)), np.full(M, 2 * K)) and (counts >= kept).all()
    runs = _model_runs("hash", p, range(M), sched, 6, dt, "vec", betas, True)
    for r, run in runs.items():
        run.run(K)
        history, at = run.run(K, reset=True)
        _check(pop, res, r, run, history, at, tables, 2 * K, counts, plane)
    pop.visit_counts = None
    assert not pop.visit_counts.any()
    _check_planes(pop, pop.visit_counts, pop.visit_bonus)
    assert np.isinf(pop.visit_bonus[1]).all() and not pop.visit_bonus[0].any()  # beta 0.05 and beta 0
    res = pop.run_steps(K, e, res.state_dict)
    tables, counts, plane = pop.q_tables, pop.visit_counts, pop.visit_bonus
    for r, run in runs.items():
        run.rt.counts[:] = 0
        history, at = run.run(K)
        _check(pop, res, r, run, history, at, tables, 3 * K, counts, plane)


def test_the_setters_and_the_refusals_on_a_live_engine():
    import ctypes

    _lib, envs, _, QLearningPopulation = _product()
    lib = _lib.load()
    M, S, A = 8, 20, 4
    f64 = lambda x: _lib.ptr(np.ascontiguousarray(x, dtype=np.float64), ctypes.c_double)  # noqa: E731
    plain = QLearningPopulation(M, S, A)
    on, lr = ctypes.c_int32(7), ctypes.c_int32(7)
    assert lib.qe_population_visits(plain.handle, ctypes.byref(on), ctypes.byref(lr), None) == 0 and (on.value, lr.value) == (0, 0)
    out = np.zeros((M, S, A), dtype=np.uint32)
    assert lib.qe_population_visit_counts(plain.handle, _lib.ptr(out, ctypes.c_uint32)) == _lib.ERR_INVALID
    assert "visit counts are off" in lib.qe_last_error().decode()
    assert lib.qe_population_set_visit_counts(plain.handle, None) == _lib.ERR_INVALID
    assert lib.qe_population_visit_bonus(plain.handle, out.ctypes.data, _lib.QE_F32) == _lib.ERR_INVALID
    with pytest.raises(ValueError, match="has no visit counts"):
        plain.visit_counts = np.zeros((M, S, A), dtype=np.uint32)
    plain.visit_counts = None  # nothing to forget
    for bad in ([-1.0] + [0.0] * (M - 1), [np.nan] * M, [np.inf] * M):
        assert lib.qe_population_set_visits(plain.handle, f64(bad), 0) == _lib.ERR_UNSUPPORTED, bad
    for kw in ({"update_rule": "sarsa"}, {"update_rule": "expected_sarsa"}, {"double_q": True}, {"update_rule": "sarsa", "n_step": 3},
               {"trace_decay": 0.5}, {"planning_steps": 2}):
        other = QLearningPopulation(M, S, A, **kw)
        assert lib.qe_population_set_visits(other.handle, f64([0.5] * M), 1) == _lib.ERR_UNSUPPORTED, kw
        assert lib.qe_population_visits(other.handle, ctypes.byref(on), None, None) == 0 and on.value == 0
    pop = QLearningPopulation(M, S, A, exploration_bonus=[0.25 * r for r in range(M)], visit_lr=True, dtype=np.float32)
    beta = np.zeros(M)
    assert lib.qe_population_visits(pop.handle, ctypes.byref(on), ctypes.byref(lr), _lib.ptr(beta, ctypes.c_double)) == 0
    assert (on.value, lr.value) == (1, 1) and beta.tolist() == [0.25 * r for r in range(M)]
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_SARSA) == _lib.ERR_UNSUPPORTED
    assert "visit counts are on" in lib.qe_last_error().decode()
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_EXPECTED_SARSA) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_double(pop.handle, 1) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_n_step(pop.handle, 2) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_traces(pop.handle, 4, 0, f64(np.full(M, 0.5))) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_planning(pop.handle, 2) == _lib.ERR_UNSUPPORTED
    assert lib.qe_population_set_update_rule(pop.handle, _lib.RULE_Q_LEARNING) == 0 and lib.qe_population_set_n_step(pop.handle, 1) == 0
    assert lib.qe_population_set_double(pop.handle, 0) == 0 and lib.qe_population_set_planning(pop.handle, 0) == 0
    pop.run_steps(40, envs.HashTabularEnv(M, S, A))
    good = pop.visit_counts
    assert np.array_equal(good.sum(axis=(1, 2)), np.full(M, 40))
    for bad in (good.astype(np.float64), good[:, :, :3], np.full((M, S, A), -1), np.full((M, S, A), 2 ** 32)):
        with pytest.raises(ValueError, match="visit_counts"):
            pop.visit_counts = bad
    assert np.array_equal(pop.visit_counts, good)  # a refused array changes nothing
    # the 64-bit download of a float32 plane is exact
    wide = np.empty((M, S, A), dtype=np.float64)
    assert lib.qe_population_visit_bonus(pop.handle, wide.ctypes.data, _lib.QE_F64) == 0
    assert np.array_equal(wide, pop.visit_bonus.astype(np.float64))
    # new betas on a live engine keep the counts and rewrite the plane; off forgets and gives the plain kernel back
    assert lib.qe_population_set_visits(pop.handle, f64(np.full(M, 2.0)), 0) == 0
    pop.exploration_bonus, pop.visit_lr = np.full(M, 2.0), False
    assert np.array_equal(pop.visit_counts, good)
    _check_planes(pop, good, pop.visit_bonus)
    assert lib.qe_population_set_visits(pop.handle, None, 0) == 0
    assert lib.qe_population_visit_counts(pop.handle, _lib.ptr(out, ctypes.c_uint32)) == _lib.ERR_INVALID
    assert lib.qe_population_set_double(pop.handle, 1) == 0


# ---- 7. launch cutting ------------------------------------------------------------------------------------------------------------
def test_a_logged_call_cut_into_launches_equals_the_unlogged_call_and_the_model():
    envs = _product()[1]
    M, steps, S, A = 20_000, 2000, 50, 8
    eps0, lr0, gamma0 = _schedules(97)
    sched = [[x[r % 97] for r in range(M)] for x in (eps0, lr0, gamma0)]
    betas = _betas(M)
    logged = _population(M, S, A, sched, 21, np.float32, "vec", exploration_bonus=betas, visit_lr=True)
    res = logged.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1))
    _reached(logged, nv=2, masked=False)
    # 2^23 log entries / 20 000 runs = 419 steps per launch: 5 launches, each with its scan and its pack
    assert logged.last_stats["launches"] == 15 > 1
    tables, counts, plane = logged.q_tables, logged.visit_counts, logged.visit_bonus
    quiet = _population(M, S, A, sched, 21, np.float32, "vec", exploration_bonus=betas, visit_lr=True)
    res_q = quiet.run_steps(steps, envs.HashTabularEnv(M, S, A, seed=1), log=False)
    assert quiet.last_stats["launches"] == 2 > 1  # 2^25 env-steps / 20 000 runs = 1 677 steps per launch
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(quiet.visit_counts, counts) and _same_bits(quiet.visit_bonus, plane)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    _same_state(res_q.state_dict, res.state_dict)
    del quiet
    _check_planes(logged, counts, plane)
    p = {"S": S, "A": A, "seed": 1, "masked": False}
    picked = [0, 1, 63, 64, 10_000, M - 1]
    for r, run in _model_runs("hash", p, picked, sched, 21, np.float32, "vec", betas, True).items():
        history, at = run.run(steps)
        _check(logged, res, r, run, history, at, {r: tables[r]}, steps, counts, plane)


# ---- 8. evaluation and train() ---------------------------------------------------------------------------------------------------
def test_evaluation_and_policy_values_leave_the_counts_alone_and_equal_the_plain_population():
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)
    M, S, A = M_ODD, mdp.state_size, mdp.action_size
    sched = _schedules(M)
    counting = _population(M, S, A, sched, 6, np.float64, "iter", exploration_bonus=_betas(M), visit_lr=True)
    counting.run_steps(120, envs.TabularMDPEnv(M, mdp, seed=1))
    _reached(counting, nv=1, masked=True)
    before, plane = counting.visit_counts, counting.visit_bonus
    plain = _population(M, S, A, sched, 6, np.float64, "iter")
    plain.set_q_tables(counting.q_tables)
    plain.step_counter = counting.step_counter
    for call in (lambda pop: pop.evaluate_steps(envs.TabularMDPEnv(M, mdp, seed=5), 40),
                 lambda pop: pop.evaluate_episodes(envs.TabularMDPEnv(M, mdp, seed=5), 2),
                 lambda pop: pop.policy_values(envs.TabularMDPEnv(M, mdp, seed=5))):
        a, b = call(counting), call(plain)
        if hasattr(a, "totals"):
            assert _product()[0].decode_variant(counting.last_stats["kernel_variant"])["path"] == "population_eval"
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
        assert np.array_equal(counting.step_counters, plain.step_counters)
    assert np.array_equal(counting.visit_counts, before) and _same_bits(counting.visit_bonus, plane)
    assert np.array_equal(counting.q_tables, plain.q_tables)


def test_train_with_two_segments_matches_the_model_driven_the_same_way():
    from table_mdp_model import TableMDPVecEnv
    from test_gpu_population_eval import _slippery_mdp

    envs = _product()[1]
    mdp = _slippery_mdp(envs, masked=True)  # every move may end the episode: greedy validation episodes end too
    M, S, A, seg, n_seg, val_episodes = M_ODD, mdp.state_size, mdp.action_size, 60, 2, 2
    sched = _schedules(M)
    betas = _betas(M)
    pop = _population(M, S, A, sched, 8, np.float64, "iter", exploration_bonus=betas, visit_lr=True)
    out = pop.train(envs.TabularMDPEnv(M, mdp, seed=1), seg * n_seg, envs.TabularMDPEnv(M, mdp, seed=5), seg, val_episodes=val_episodes)
    assert out.val_finished.all() and "visit_counts" not in out.state_dict
    tables, counters, counts, plane = pop.q_tables, pop.step_counters, pop.visit_counts, pop.visit_bonus
    assert np.array_equal(counts.sum(axis=(1, 2)), np.full(M, seg * n_seg))
    pt = {"mdp": mdp, "seed": 1}
    for r, run in _model_runs("table", pt, range(M), sched, 8, np.float64, "iter", betas, True).items():
        for k in range(n_seg):
            history, at = run.run(seg, reset=True)  # (train passes curr_state_dict=None: every segment resets; the counts stay)
            assert np.array_equal(out.segments[k].run_returns(r), history), (r, k)
            assert np.array_equal(out.segments[k].run_steps(r), at), (r, k)
            val = TableMDPVecEnv(1, mdp, seed=5, agent_offset=r)
            val.step_index = run.rt.step_counter  # the validation steps draw at the run's own counter
            total, _ = run.rt.evaluate_episodes(val, val_episodes)
            assert out.val_totals[k, r] == np.float32(total), (r, k)
        assert np.array_equal(tables[r], run.q), r
        assert counters[r] == run.rt.step_counter, r
        assert np.array_equal(counts[r], run.counts) and _same_bits(plane[r], run.bonus), r
