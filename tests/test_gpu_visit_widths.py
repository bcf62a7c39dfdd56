"""GPU: the population's visit counts (``QLearningPopulation(exploration_bonus=..., visit_lr=...)``, k_visit_rollout,
k_visit_fill and the count getter and setter) at the places the other update rules were already taken to
(tests/test_gpu_population_rule_widths.py): padded and degenerate row widths, the selection threshold at 10 / 11 actions
on tables with NaN and infinite cells, real columns that tie with the padding, draw counters and agent ids that wrap at
2^32, saturating counts next to the held-row patch, and the count planes through the host at a padded width.

The family keeps two more planes per run than the others, N and B, both at ``s * ld + a``; the pick sees ``Q + B``; the
padding of B is 0 where the table's is -inf; an untried real cell at -inf scores ``-inf + inf = NaN`` and a tried one
-inf, like the padding.  A wrong column or stride in any of that shows only where ``ld != A``.

Every comparison is bit for bit against the NumPy model run of the same run (visit_model.py) through the ``_check`` of
tests/test_gpu_visits.py: the table, the counts, the bonus plane (also against ``bonus()`` of the counts), episode returns
and their steps, counts and means, final observation / env word / running return, schedule values and the draw counter.
No tolerance anywhere.  Every case asserts the build it reaches (path 14, NV, masked and the two flag bits).

The inputs with NaN or infinite cells are built here by functions without a device in them;
tests/test_visit_width_cases.py asserts on the models alone that they keep enough runs to test something.  Model
outcomes are computed once per case (``functools.lru_cache``) and shared by both modules.
"""
import functools
import pickle

import numpy as np
import pytest

import test_gpu_visits as tv
from table_mdp_model import TableMDPVecEnv, random_mdp
from test_gpu_double_q import special_tables
from test_gpu_population import _schedules
from test_gpu_population_rule_widths import COMBOS, EVAL_WIDTHS, M_ODD, NAN_S, NAN_SHAPES, OFFSET, STEP0, WIDTHS, _sample, hash_model_env
from test_gpu_td_rules import _nv, _product
from visit_model import VISIT_MAX, VisitRun, bonus

pytestmark = pytest.mark.gpu

K_STEPS = 150
BETAS = tv._betas(M_ODD)  # (0, 0.05, 0.5, 4.0)[r % 4]


def _name(A, masked):
    return f"A{A}-{'masked' if masked else 'plain'}"


# ---- the model side (no device) -------------------------------------------------------------------------------------------
def visit_models(make_env, runs, K, sched, seed, dt, mode, visit_lr, *, q0=None, n0=None, step0=0):
    """{run: (model run, history, steps)} of the runs the model completes, and the runs it flags (IndexError)."""
    eps_s, lr_s, gamma = sched
    done, flagged = {}, []
    for r in runs:
        run = VisitRun(make_env(r), gamma[r], eps_s[r], lr_s[r], beta=BETAS[r], visit_lr=visit_lr, seed=seed, dtype=dt,
                       mode=mode, agent_id=r, q0=None if q0 is None else q0[r], n0=None if n0 is None else n0[r])
        run.rt.step_counter = step0
        try:
            history, at = run.run(K)
        except IndexError:  # some pick of the run had no candidate
            flagged.append(r)
            continue
        done[r] = (run, history, at)
    return done, flagged


# ---- the device side ------------------------------------------------------------------------------------------------------
def population(S, A, sched, seed, dt, mode, visit_lr):
    return tv._population(M_ODD, S, A, sched, seed, dt, mode, exploration_bonus=BETAS, visit_lr=visit_lr)


def snapshot(pop):
    """What the comparison reads from the device after a call, downloaded once; the plane against the formula."""
    tables, counts, plane = pop.q_tables, pop.visit_counts, pop.visit_bonus
    tv._check_planes(pop, counts, plane)
    return tables, counts, plane


def check_runs(pop, res, done, snap, counter):
    for r, (run, history, at) in done.items():
        tv._check(pop, res, r, run, history, at, snap[0], counter, snap[1], snap[2])


def hash_case(S, A, masked, dt, mode, visit_lr, runs, *, K=K_STEPS, seed=0, env_seed=1, offset=0, step0=0):
    """One call on the hash environment against the model runs ``runs``; no run may be flagged."""
    envs = _product()[1]
    sched = _schedules(M_ODD)
    pop = population(S, A, sched, seed, dt, mode, visit_lr)
    if step0:
        pop.step_counter = step0
    res = pop.run_steps(K, envs.HashTabularEnv(M_ODD, S, A, seed=env_seed, masked=masked, agent_offset=offset))
    tv._reached(pop, nv=_nv(A), masked=masked)
    assert "visit_counts" not in res.state_dict and "visit_bonus" not in res.state_dict
    snap = snapshot(pop)
    assert np.array_equal(snap[1].sum(axis=(1, 2), dtype=np.uint64), np.full(M_ODD, K))
    done, flagged = visit_models(lambda r: hash_model_env(r, S, A, masked, env_seed, offset), runs, K, sched, seed, dt, mode,
                                 visit_lr, step0=step0)
    assert not flagged
    check_runs(pop, res, done, snap, step0 + K)
    return pop, res, done


# ---- 1. every padded and degenerate row width -------------------------------------------------------------------------------
def width_combo(wi, masked):
    """Width index and mask to (dtype, learn mode, visit_lr): over the eight widths every (dtype, mode, visit_lr) triple
    meets a plain and a masked case (tests/test_visit_width_cases.py asserts it)."""
    return (*COMBOS[(wi + 2 * int(masked)) % 4], (wi // 4 + int(masked)) % 2 == 1)


WIDTH_CASES = [pytest.param(A, masked, *width_combo(wi, masked), id=_name(A, masked)) for wi, A in enumerate(WIDTHS)
               for masked in (False, True)]


@pytest.mark.parametrize(("A", "masked", "dt", "mode", "visit_lr"), WIDTH_CASES)
def test_every_padded_width_matches_the_model(A, masked, dt, mode, visit_lr):
    """(In the masked hash environment action 0 is always valid: no run may be flagged.)"""
    _, _, done = hash_case(300, A, masked, dt, mode, visit_lr, range(M_ODD))
    if A > 1:  # (at A = 1 explore and greedy coincide and every row has one candidate: the walk is a fixed cycle)
        assert any(np.any(run.q) for run, _, _ in done.values()), "no compared run learned anything"


# ---- 2. the selection threshold at 10 / 11 actions, on tables with NaN and infinite cells --------------------------------------
NAN_CASES = [pytest.param(A, masked, id=_name(A, masked)) for A, masked in NAN_SHAPES]


@functools.lru_cache(maxsize=None)
def nan_case(A, masked):
    """The inputs and the model's side of one case: a dict of dt, mode, visit_lr, sched, q0, n0, done and flagged.  The
    score row is ``Q + B``: an untried cell scores +inf (beta > 0), or NaN where the table holds -inf."""
    i = NAN_SHAPES.index((A, masked))
    dt, mode = COMBOS[i]
    visit_lr = i % 2 == 1
    sched = _schedules(M_ODD)
    q0 = special_tables(M_ODD, NAN_S, A, dt, seed=A)
    done, flagged = visit_models(lambda r: hash_model_env(r, NAN_S, A, masked), range(M_ODD), K_STEPS, sched, 0, dt, mode,
                                 visit_lr, q0=q0)
    return {"dt": dt, "mode": mode, "visit_lr": visit_lr, "sched": sched, "q0": q0, "n0": None, "done": done, "flagged": flagged}


def compare_with_flagged_runs(c, S, A, masked, K, seed=0, env_seed=1):
    """The call of case ``c`` on the device: the runs it names are the model's, every other run is the model's run."""
    envs = _product()[1]
    pop = population(S, A, c["sched"], seed, c["dt"], c["mode"], c["visit_lr"])
    pop.set_q_tables(c["q0"])
    if c["n0"] is not None:
        pop.visit_counts = c["n0"]
        assert np.array_equal(pop.visit_counts, c["n0"]), "the getter returns what the setter took"
        tv._check_planes(pop, c["n0"], pop.visit_bonus)
    res, raised = tv._run_flagged(pop, K, envs.HashTabularEnv(M_ODD, S, A, seed=env_seed, masked=masked))
    tv._reached(pop, nv=_nv(A), masked=masked)
    snap = snapshot(pop)
    assert raised == c["flagged"]  # in order; no run is left out that the model does not flag itself
    check_runs(pop, res, c["done"], snap, K)
    return pop, res, snap


@pytest.mark.parametrize(("A", "masked"), NAN_CASES)
def test_the_selection_threshold_on_special_tables_matches_the_model(A, masked):
    c = nan_case(A, masked)
    assert c["flagged"] and len(c["done"]) >= (M_ODD + 1) // 2  # (tests/test_visit_width_cases.py, in full)
    assert any(not np.isfinite(run.q).all() for run, _, _ in c["done"].values())
    compare_with_flagged_runs(c, NAN_S, A, masked, K_STEPS)


# ---- 3. real columns that tie with the padding, through the count setter -------------------------------------------------------
TIE_COMBOS = {3: (np.float32, "iter", False), 5: (np.float64, "vec", True)}  # A -> dtype, learn mode, visit_lr
TIE_CASES = [pytest.param(A, tried, id=f"A{A}-{'tried' if tried else 'untried'}") for tried in (True, False) for A in (3, 5)]


def tie_inputs(A, tried):
    """Unmasked rows of A in 4 or 8 columns: every third run starts with one whole row of -inf (``rows``: run -> row) in
    an otherwise finite table, and the runs alternate between epsilon 0 and 0.3.  ``tried``: starting counts of 0..3
    everywhere and 1..4 on the -inf row, whose cells then score -inf exactly, like the padding; else no starting counts,
    and an untried -inf cell scores ``-inf + inf = NaN`` wherever beta > 0."""
    sch = _product()[2]
    dt, mode, visit_lr = TIE_COMBOS[A]
    rng = np.random.default_rng(100 + A)
    q0 = rng.standard_normal((M_ODD, NAN_S, A)).astype(dt)
    rows = {r: int(rng.integers(0, NAN_S)) for r in range(0, M_ODD, 3)}
    n0 = rng.integers(0, 4, (M_ODD, NAN_S, A)).astype(np.uint32)
    for r, s in rows.items():
        q0[r, s] = -np.inf
        n0[r, s] = rng.integers(1, 5, A)
    _, lr_s, gamma = _schedules(M_ODD)
    eps_s = [sch.ConstantSchedule(0.3 if r % 2 else 0.0) for r in range(M_ODD)]
    return dt, mode, visit_lr, (eps_s, lr_s, gamma), q0, n0 if tried else None, rows


@functools.lru_cache(maxsize=None)
def tie_case(A, tried):
    dt, mode, visit_lr, sched, q0, n0, rows = tie_inputs(A, tried)
    done, flagged = visit_models(lambda r: hash_model_env(r, NAN_S, A, False), range(M_ODD), K_STEPS, sched, 0, dt, mode,
                                 visit_lr, q0=q0, n0=n0)
    return {"dt": dt, "mode": mode, "visit_lr": visit_lr, "sched": sched, "q0": q0, "n0": n0, "done": done, "flagged": flagged,
            "rows": rows}


def wrote_into_its_row(c, r):
    """Run r (completed) has changed a cell of the row that started as -inf."""
    q = c["done"][r][0].q[c["rows"][r]]
    return not np.array_equal(q, np.full_like(q, -np.inf))


@pytest.mark.parametrize(("A", "tried"), TIE_CASES)
def test_real_columns_that_tie_with_the_padding_keep_the_pick_inside_the_row(A, tried):
    c = tie_case(A, tried)
    assert len(c["done"]) >= (M_ODD + 1) // 2
    if tried:
        assert any(wrote_into_its_row(c, r) for r in c["rows"] if r in c["done"])
    # (the setter at S > 1 with ld != A: the getter and the plane are asserted before the call, in compare_with_flagged_runs)
    pop, _, (tables, counts, _) = compare_with_flagged_runs(c, NAN_S, A, False, K_STEPS)
    # a pick at or above A would count and store in a padding column and leave the real cells as they were: the real
    # columns of every compared run equal the model's (above), every step of theirs is counted in a real column, and
    # the runs differ from their start
    start = np.zeros(M_ODD, dtype=np.uint64) if c["n0"] is None else c["n0"].sum(axis=(1, 2), dtype=np.uint64)
    kept = list(c["done"])
    assert np.array_equal(counts.sum(axis=(1, 2), dtype=np.uint64)[kept], start[kept] + np.uint64(K_STEPS))
    assert not np.array_equal(tables, c["q0"], equal_nan=True)


# ---- 4. counters and agent ids at 2^32 -----------------------------------------------------------------------------------------
WRAP_SHAPES = [(9, True, True), (5, False, False)]  # A, masked, visit_lr
WRAP_CASES = [pytest.param(A, masked, visit_lr, id=_name(A, masked)) for A, masked, visit_lr in WRAP_SHAPES]


def wrap_combo(A, shift):
    """(dtype, learn mode) of a wrap case: the tests of one shape take different ones."""
    return COMBOS[(A // 8 + shift) % 4]


@pytest.mark.parametrize(("A", "masked", "visit_lr"), WRAP_CASES)
def test_a_step_counter_crossing_2_pow_32_matches_the_model(A, masked, visit_lr):
    _, res, _ = hash_case(200, A, masked, *wrap_combo(A, 0), visit_lr, _sample(A), step0=STEP0)
    assert res.state_dict["rng_step"] == STEP0 + K_STEPS > 2**32


@pytest.mark.parametrize(("A", "masked", "visit_lr"), WRAP_CASES)
def test_a_counter_wrap_next_to_a_saved_and_restored_call_boundary_matches_the_model(A, masked, visit_lr, tmp_path):
    """Two calls of 75 steps; the second by a fresh population from the saved tables, the pickled counts and the pickled
    state dict.  The wrap is step 69 of the first call.  One model run is driven through both calls."""
    envs = _product()[1]
    dt, mode = wrap_combo(A, 1)
    S, K, seed = 200, 75, 4
    sched = _schedules(M_ODD)

    def env():
        return envs.HashTabularEnv(M_ODD, S, A, seed=9, masked=masked)

    pop = population(S, A, sched, seed, dt, mode, visit_lr)
    pop.step_counter = STEP0
    first = pop.run_steps(K, env())
    snap1 = snapshot(pop)
    assert np.array_equal(snap1[1].sum(axis=(1, 2), dtype=np.uint64), np.full(M_ODD, K))
    pop.save(tmp_path / "tables.npy")
    blob = pickle.dumps((first.state_dict, snap1[1]))
    fresh = population(S, A, sched, seed, dt, mode, visit_lr)
    sd, counts = pickle.loads(blob)
    fresh.load(tmp_path / "tables.npy")
    fresh.visit_counts = counts
    fresh.restore_training_state(sd)
    assert np.array_equal(fresh.visit_counts, snap1[1]) and tv._same_bits(fresh.visit_bonus, snap1[2])
    second = fresh.run_steps(K, env(), sd)
    snap2 = snapshot(fresh)
    assert np.array_equal(snap2[1].sum(axis=(1, 2), dtype=np.uint64), np.full(M_ODD, 2 * K))
    for p in (pop, fresh):
        tv._reached(p, nv=_nv(A), masked=masked)
    assert first.state_dict["rng_step"] == STEP0 + K > 2**32
    eps_s, lr_s, gamma = sched
    for r in _sample(10 + A):
        run = VisitRun(hash_model_env(r, S, A, masked, 9), gamma[r], eps_s[r], lr_s[r], beta=BETAS[r], visit_lr=visit_lr, seed=seed,
                       dtype=dt, mode=mode, agent_id=r)
        run.rt.step_counter = STEP0
        history, at = run.run(K)
        tv._check(pop, first, r, run, history, at, snap1[0], STEP0 + K, snap1[1], snap1[2])
        history, at = run.run(K)
        tv._check(fresh, second, r, run, history, at, snap2[0], STEP0 + 2 * K, snap2[1], snap2[2])


@pytest.mark.parametrize(("A", "masked", "visit_lr"), WRAP_CASES)
def test_agent_ids_that_wrap_past_2_pow_32_match_the_model(A, masked, visit_lr):
    runs = sorted(set(_sample(30 + A)) | {28, 29, 30, 31})  # ids 2^32 - 2, 2^32 - 1, 0 and 1
    hash_case(200, A, masked, *wrap_combo(A, 2), not visit_lr, runs, offset=OFFSET)


@pytest.mark.parametrize(("A", "visit_lr", "dt", "mode"), [(9, True, *wrap_combo(9, 3)), (5, False, *wrap_combo(5, 3))])
def test_a_step_counter_crossing_2_pow_32_on_a_table_env_matches_the_model(A, visit_lr, dt, mode):
    """The table environment hashes the step too (``step >> 32`` in its word), unlike the hash environment."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    envs = _product()[1]
    S, K, seed = 300, K_STEPS, 2
    arrays, isd, masks = random_mdp(S, A, 3, seed=6, masked=True)
    mdp = encode_table_mdp(*arrays, isd, masks)
    sched = _schedules(M_ODD)
    pop = population(S, A, sched, seed, dt, mode, visit_lr)
    pop.step_counter = STEP0
    res, raised = tv._run_flagged(pop, K, envs.TabularMDPEnv(M_ODD, mdp, seed=3))
    tv._reached(pop, nv=_nv(A), masked=True)
    snap = snapshot(pop)
    done, flagged = visit_models(lambda r: TableMDPVecEnv(1, mdp, seed=3, agent_offset=r), _sample(20), K, sched, seed, dt, mode,
                                 visit_lr, step0=STEP0)
    assert not flagged and not raised
    check_runs(pop, res, done, snap, STEP0 + K)
    assert np.array_equal(snap[1].sum(axis=(1, 2), dtype=np.uint64), np.full(M_ODD, K))
    assert res.episode_counts.sum() > 0


# ---- 5. saturation next to the held-row patch at a padded width ------------------------------------------------------------------
def run_counting_stays(run, K):
    """``run.run(K)``, and how many of the K steps ended in the state they began in (the kernel then patches the rows it
    holds in registers instead of loading them)."""
    run.reset()
    history, at, stays = [], [], 0
    for t in range(K):
        before = run.obs
        h, _ = run.run(1)
        history += h.tolist()
        at += [t] * len(h)
        stays += run.obs == before
    return np.array(history, dtype=np.float32), np.array(at, dtype=np.int32), stays


@pytest.mark.parametrize(("masked", "dt", "mode"), [(False, *COMBOS[0]), (True, *COMBOS[1])])
def test_counts_saturate_next_to_the_held_row_patch_at_three_actions(masked, dt, mode):
    envs = _product()[1]
    S, A, K, seed = 2, 3, 20, 3
    sched = _schedules(M_ODD)
    n0 = np.full((M_ODD, S, A), VISIT_MAX - 1, dtype=np.uint32)
    pop = population(S, A, sched, seed, dt, mode, True)
    pop.visit_counts = n0
    assert np.array_equal(pop.visit_counts, n0)
    tv._check_planes(pop, n0, pop.visit_bonus)
    res = pop.run_steps(K, envs.HashTabularEnv(M_ODD, S, A, seed=1, masked=masked))
    tv._reached(pop, nv=1, masked=masked)
    tables, counts, plane = snapshot(pop)
    assert counts.max() == VISIT_MAX and counts.min() >= VISIT_MAX - 1
    assert (counts.reshape(M_ODD, -1).max(axis=1) == VISIT_MAX).all()  # every run took a step, and stopped there
    eps_s, lr_s, gamma = sched
    stayed = 0
    for r in range(M_ODD):
        run = VisitRun(hash_model_env(r, S, A, masked), gamma[r], eps_s[r], lr_s[r], beta=BETAS[r], visit_lr=True, seed=seed, dtype=dt,
                       mode=mode, agent_id=r, n0=n0[r])
        history, at, stays = run_counting_stays(run, K)
        stayed += stays
        tv._check(pop, res, r, run, history, at, tables, K, counts, plane)
    assert stayed > 0, "no compared run met s' == s"


# ---- 6. the count getter and setter at every padded width ------------------------------------------------------------------------
COUNT_VALUES = (0, 1, 2**24 + 1, 2**32 - 1)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("A", EVAL_WIDTHS)
def test_counts_go_through_the_setter_and_the_getter_at_every_padded_width(A, dt):
    """Random 32-bit counts, so that a cell read or written at ``s * A + a`` where the device keeps ``s * ld + a`` shows.
    One step follows, for the build: it changes at most one count per run, by one."""
    envs = _product()[1]
    S = 7
    rng = np.random.default_rng(A)
    n = rng.integers(0, 2**32, (M_ODD, S, A), dtype=np.uint64)
    where = rng.permutation(n.size)[:4 * len(COUNT_VALUES)]
    n.ravel()[where] = np.repeat(np.array(COUNT_VALUES, dtype=np.uint64), 4)
    n = n.astype(np.uint32)
    assert all((n == v).any() for v in COUNT_VALUES)
    pop = population(S, A, _schedules(M_ODD), 1, dt, "iter", A % 2 == 1)
    assert not pop.visit_counts.any()
    pop.visit_counts = n
    got = pop.visit_counts
    assert got.dtype == np.uint32 and np.array_equal(got, n)
    plane = pop.visit_bonus
    tv._check_planes(pop, n, plane)
    for r in range(M_ODD):
        assert tv._same_bits(plane[r], bonus(BETAS[r], n[r], dt)), r
    pop.visit_counts = None  # ... and forgotten in every cell, the ones of the last rows included
    assert not pop.visit_counts.any()
    tv._check_planes(pop, pop.visit_counts, pop.visit_bonus)
    pop.visit_counts = n
    pop.run_steps(1, envs.HashTabularEnv(M_ODD, S, A, seed=1))
    tv._reached(pop, nv=_nv(A), masked=False)
    after = pop.visit_counts
    moved = after != n
    assert (moved.reshape(M_ODD, -1).sum(axis=1) <= 1).all() and np.array_equal(after[moved], n[moved] + np.uint32(1))
    tv._check_planes(pop, after, pop.visit_bonus)
