"""GPU: the population's later update rules -- SARSA and Expected SARSA (k_rollout_runs_td), n-step (k_nstep_rollout),
eligibility traces (k_trace_rollout), Dyna-Q (k_dyna_rollout), Double Q (k_double_rollout), n-step Tree Backup
(k_tree_rollout), prioritized sweeping (k_sweep_rollout) and the two greedy-evaluation kernels -- at the places the Q-learning kernel was already taken to
(tests/test_gpu_population_limits.py): padded and degenerate row widths, the selection threshold at 10 / 11 actions on
NaN tables, real columns that tie with the padding, draw counters and agent ids that wrap at 2^32, and carried state
that goes through the host at a padded width.

Every comparison is bit for bit against the NumPy model run of the same run (td_rules_model.py, n_step_model.py,
trace_model.py, dyna_model.py, double_q_model.py, tree_backup_model.py, sweep_model.py), through the ``_check`` of the family's own test
module: tables, episode returns and their steps, counts, final observation / env word / running return, schedule
values, draw counter and the family's carried state.  The single-table evaluation is compared with the standalone
one-agent evaluation, as in test_gpu_population_eval.py.  No tolerance anywhere.  Every case asserts the build it
reaches (path, rule, NV, masked).

The inputs of the NaN and infinity cases are built here by functions without a device in them;
tests/test_population_rule_width_cases.py asserts on the models alone that they keep enough runs to test something.
Model outcomes are computed once per case (``functools.lru_cache``) and shared by both modules.
"""
import copy
import functools
import pickle

import numpy as np
import pytest

import test_gpu_double_q as dq
import test_gpu_dyna as dy
import test_gpu_n_step as ns
import test_gpu_sweep as sw
import test_gpu_td_rules as td
import test_gpu_traces as tr
import test_gpu_tree_backup as tb
import tree_backup_cases as tbc
from double_q_model import DoubleRun
from dyna_model import DynaRun
from n_step_model import NStepRun
from oracle import envs as oenvs
from sweep_model import SweepRun
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import TdRun
from test_gpu_double_q import _run_flagged, special_tables
from test_gpu_population import _schedules
from test_gpu_population_limits import _nv
from trace_model import TraceRun
from tree_backup_model import TreeBackupRun

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
M_ODD = 67  # a full and a partial wavefront
FIXED = (0, 1, 62, 63, 64, 65, 66)
N_STEP, TRACE_K, PLANNING = 3, 4, 4
COMBOS = [(np.float32, "iter"), (np.float64, "vec"), (np.float32, "vec"), (np.float64, "iter")]

# a family: "<kernel>[-<rule>[-<trace kind>]]"; Tree Backup: "tree-<horizon>"
FAMILIES = (["sarsa", "expected_sarsa"] + [f"nstep-{rule}" for rule in ns.RULES]
            + [f"trace-{rule}-{kind}" for rule in tr.RULES for kind in tr.KINDS] + ["dyna", "double"])
SIX = ["sarsa", "expected_sarsa", "nstep", "trace", "dyna", "double"]
SEVEN = [*SIX, "tree"]  # appended: the six keep their indices, and with them their dtypes, learn modes and seeds
EIGHT = [*SEVEN, "sweep"]  # appended likewise: prioritized sweeping, n = 4 updates per step from a queue of 4 slots
TREE_FAMILIES = [f"tree-{n}" for n in tbc.HORIZONS]
SWEEP_K = 4


def _product():
    return td._product()


def _rotated(family, i):
    """The i-th member of one of the eight families: n-step and the traces rotate their rules and kinds, Tree Backup
    its horizon."""
    if family == "nstep":
        return f"nstep-{ns.RULES[i % 2]}"
    if family == "trace":
        return f"trace-{tr.RULES[i % 2]}-{tr.KINDS[(i // 2) % 2]}"
    if family == "tree":  # (from the second horizon on: the first special-table shape then has a horizon above 2)
        return f"tree-{tbc.HORIZONS[(i + 1) % 3]}"
    return family


def group_of(fam):
    """The family a width case counts for: the Tree Backup horizons are one family."""
    return "tree" if fam.startswith("tree-") else fam


def _sample(seed, extra=3):
    rng = np.random.default_rng(seed)
    return sorted(set(FIXED) | set(rng.integers(2, 62, extra).tolist()))


def _lambdas(M):
    """A lambda grid over the runs, every one above 0, 1 included."""
    return [(1.0, 0.9, 0.5, 0.97, 0.3)[r % 5] for r in range(M)]


def family_kw(fam, M):
    """The keyword arguments of ``QLearningPopulation`` that turn the family on."""
    kind, *rest = fam.split("-")
    if kind == "q_learning":
        return {}
    if kind in td.RULES:
        return {"update_rule": kind}
    if kind == "nstep":
        return {"update_rule": rest[0], "n_step": N_STEP}
    if kind == "trace":
        return {"update_rule": rest[0], "trace_decay": _lambdas(M), "trace_length": TRACE_K, "trace_kind": rest[1]}
    if kind == "dyna":
        return {"planning_steps": PLANNING}
    if kind == "tree":
        return {"tree_backup": int(rest[0])}
    if kind == "sweep":  # (the thresholds cycle over 0, 1e-4 and 1e-2 by run, as in tests/test_gpu_sweep.py)
        return {"planning_steps": PLANNING, "planning_order": "prioritized", "queue_length": SWEEP_K,
                "sweep_threshold": sw._thetas(M)}
    return {"double_q": True}


def model_run(fam, env, r, sched, seed, dt, mode, q0=None, qb0=None):
    """The model of run r (schedules and discount of index r) on the one-agent oracle environment ``env``."""
    eps_s, lr_s, gamma = sched
    kind, *rest = fam.split("-")
    ids = getattr(env, "agent_ids", None)
    kw = {"seed": seed, "dtype": dt, "mode": mode, "agent_id": r if ids is None else int(ids[0])}
    if kind in td.RULES:
        return TdRun(env, kind, gamma[r], eps_s[r], lr_s[r], q0=q0, **kw)
    if kind == "nstep":
        return NStepRun(env, rest[0], gamma[r], eps_s[r], lr_s[r], n=N_STEP, q0=q0, **kw)
    if kind == "trace":
        return TraceRun(env, rest[0], gamma[r], eps_s[r], lr_s[r], lam=_lambdas(len(gamma))[r], K=TRACE_K, kind=rest[1],
                        q0=q0, **kw)
    if kind == "dyna":
        return DynaRun(env, gamma[r], eps_s[r], lr_s[r], n=PLANNING, q0=q0, **kw)
    if kind == "tree":  # (with the census of its branches and of the cut rows it reads: tests/tree_backup_cases.py)
        return tbc.with_census(TreeBackupRun(env, gamma[r], eps_s[r], lr_s[r], n=int(rest[0]), q0=q0, **kw))
    if kind == "sweep":  # (its census is the model's own ``events``: tests/sweep_model.py)
        return SweepRun(env, gamma[r], eps_s[r], lr_s[r], n=PLANNING, K=SWEEP_K, theta=sw.THETAS[r % 3], q0=q0, **kw)
    return DoubleRun(env, gamma[r], eps_s[r], lr_s[r], qa0=q0, qb0=qb0, **kw)


def hash_model_env(r, S, A, masked, seed=1, offset=0):
    return oenvs.HashTabularEnv(1, S, A, seed=seed, masked=masked, agent_offset=(offset + r) & U32)


def run_models(fam, make_env, runs, K, sched, seed, dt, mode, q0=None, qb0=None, step0=0):
    """{run: (model run, history, steps)} of the runs the model completes, and the runs it flags (IndexError)."""
    done, flagged = {}, []
    for r in runs:
        run = model_run(fam, make_env(r), r, sched, seed, dt, mode, None if q0 is None else q0[r],
                        None if qb0 is None else qb0[r])
        run.rt.step_counter = step0
        try:
            history, at = run.run(K)
        except IndexError:  # some pick of the run had no candidate
            flagged.append(r)
            continue
        done[r] = (run, history, at)
    return done, flagged


def tables_of(run):
    return (run.qa, run.qb) if isinstance(run, DoubleRun) else (run.q,)


# ---- the device side ------------------------------------------------------------------------------------------------------
def population(fam, M, S, A, sched, seed, dt, mode):
    eps_s, lr_s, gamma = sched
    return _product()[3](M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=seed, dtype=dt, learn_mode=mode,
                         **family_kw(fam, M))


def reached(fam, pop, A, masked):
    kind, *rest = fam.split("-")
    nv = _nv(A)
    if kind in td.RULES:
        td._reached(pop, kind, nv=nv, masked=masked)
    elif kind == "nstep":
        ns._reached(pop, rest[0], N_STEP, nv=nv, masked=masked)
    elif kind == "trace":
        tr._reached(pop, rest[0], TRACE_K, rest[1], nv=nv, masked=masked)
    elif kind == "dyna":
        dy._reached(pop, PLANNING, nv=nv, masked=masked)
    elif kind == "tree":
        tb._reached(pop, int(rest[0]), nv=nv, masked=masked)
    elif kind == "sweep":
        sw._reached(pop, PLANNING, SWEEP_K, nv=nv, masked=masked)
    else:
        dq._reached(pop, nv=nv, masked=masked)


def snapshot(fam, pop):
    """What the comparison reads from the device after a call, downloaded once."""
    return {"a": pop.q_tables, "b": pop.q_tables_b if fam == "double" else None,
            "model": pop.planning_model if fam in ("dyna", "sweep") else None}


def check(fam, pop, res, r, run, history, at, snap, counter):
    kind = fam.split("-")[0]
    if kind in td.RULES:
        td._check(pop, res, r, run, history, at, snap["a"], counter)
    elif kind == "tree":
        tb._check(pop, res, r, run, history, at, snap["a"], counter)
    elif kind == "nstep":
        ns._check(pop, res, r, run, history, at, snap["a"], counter)
    elif kind == "trace":
        tr._check(pop, res, r, run, history, at, snap["a"], counter)
    elif kind == "dyna":
        dy._check(pop, res, r, run, history, at, snap["a"], counter, snap["model"])
    elif kind == "sweep":  # (the queue is read from ``res.state_dict["sweep_queue"]``)
        sw._check(pop, res, r, run, history, at, snap["a"], counter, snap["model"])
    else:
        dq._check(pop, res, r, run, history, at, snap["a"], snap["b"], counter)


def hash_models(fam, S, A, masked, dt, mode, runs, *, K=150, seed=0, env_seed=1, offset=0, step0=0):
    """The model's side of ``hash_case``: ``run_models`` of the runs ``runs``."""
    return run_models(fam, lambda r: hash_model_env(r, S, A, masked, env_seed, offset), runs, K, _schedules(M_ODD), seed, dt,
                      mode, step0=step0)


def hash_case(fam, S, A, masked, dt, mode, runs, *, K=150, seed=0, env_seed=1, offset=0, step0=0, models=None):
    """One call on the hash environment against the model runs ``runs`` (``models``: their ``hash_models``, if the
    caller has them already)."""
    envs = _product()[1]
    sched = _schedules(M_ODD)
    pop = population(fam, M_ODD, S, A, sched, seed, dt, mode)
    if step0:
        pop.step_counter = step0
    res = pop.run_steps(K, envs.HashTabularEnv(M_ODD, S, A, seed=env_seed, masked=masked, agent_offset=offset))
    reached(fam, pop, A, masked)
    snap = snapshot(fam, pop)
    done, flagged = models or hash_models(fam, S, A, masked, dt, mode, runs, K=K, seed=seed, env_seed=env_seed,
                                          offset=offset, step0=step0)
    assert not flagged and sorted(done) == sorted(runs)
    for r, (run, history, at) in done.items():
        check(fam, pop, res, r, run, history, at, snap, step0 + K)
    return pop, res, done


# ---- 1. padded and degenerate row widths, all eight training families -------------------------------------------------------
WIDTHS = [1, 2, 3, 5, 9, 17, 33, 63]
WIDTH_CASES = [pytest.param(fam, A, masked, *COMBOS[(wi + 2 * int(masked) + fi) % 4],
                            id=f"{fam}-A{A}-{'masked' if masked else 'plain'}")
               for fi, fam in enumerate(FAMILIES) for wi, A in enumerate(WIDTHS) for masked in (False, True)]
# Tree Backup, appended: the horizon rotates with the width and the mask, and S = 40 -- at S = 300 stores into the held
# row and cut states equal to s' are 10 to 20 times rarer
TREE_S = 40
WIDTH_CASES += [pytest.param(fam, A, masked, *COMBOS[(wi + 2 * int(masked) + len(FAMILIES)) % 4],
                             id=f"{fam}-A{A}-{'masked' if masked else 'plain'}")
                for wi, A in enumerate(WIDTHS) for masked in (False, True)
                for fam in [TREE_FAMILIES[(wi + int(masked)) % 3]]]
TREE_WIDTH_CASES = [p.values for p in WIDTH_CASES if group_of(p.values[0]) == "tree"]
# prioritized sweeping, appended after it: S = 40 as well -- at S = 100 a planning store or a propagate meets the held
# row too rarely
SWEEP_S = 40
WIDTH_CASES += [pytest.param("sweep", A, masked, *COMBOS[(wi + 2 * int(masked) + len(FAMILIES) + 1) % 4],
                             id=f"sweep-A{A}-{'masked' if masked else 'plain'}")
                for wi, A in enumerate(WIDTHS) for masked in (False, True)]
SWEEP_WIDTH_CASES = [p.values for p in WIDTH_CASES if p.values[0] == "sweep"]


@functools.lru_cache(maxsize=None)
def tree_width_models(fam, A, masked, dt, mode):
    """The model's side of a Tree Backup width case, computed once for this module and for
    tests/test_population_rule_width_cases.py."""
    return hash_models(fam, TREE_S, A, masked, dt, mode, _sample(A))


@functools.lru_cache(maxsize=None)
def sweep_width_mdp(A, masked):
    """The environment of a prioritized-sweeping width case: a random table MDP of three outcomes per cell.  On the hash
    environment the next state of a cell never changes, so no cell is ever unlinked from a predecessor list."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    arrays, isd, masks = random_mdp(SWEEP_S, A, 3, seed=70 + A, masked=masked)
    return encode_table_mdp(*arrays, isd, masks)


@functools.lru_cache(maxsize=None)
def sweep_width_models(fam, A, masked, dt, mode):
    """The same for a prioritized-sweeping width case."""
    mdp = sweep_width_mdp(A, masked)
    return run_models(fam, lambda r: TableMDPVecEnv(1, mdp, seed=3, agent_offset=r), _sample(A), 150, _schedules(M_ODD), 0,
                      dt, mode)


def table_case(fam, mdp, A, masked, dt, mode, models, *, K=150, seed=0, env_seed=3):
    """``hash_case`` on a table environment, against the model runs ``models``."""
    envs = _product()[1]
    pop = population(fam, M_ODD, mdp.thr.shape[0], A, _schedules(M_ODD), seed, dt, mode)
    res = pop.run_steps(K, envs.TabularMDPEnv(M_ODD, mdp, seed=env_seed))
    reached(fam, pop, A, masked)
    snap = snapshot(fam, pop)
    done, flagged = models
    assert not flagged and done
    for r, (run, history, at) in done.items():
        check(fam, pop, res, r, run, history, at, snap, K)
    return pop, res, done


@pytest.mark.parametrize(("fam", "A", "masked", "dt", "mode"), WIDTH_CASES)
def test_every_padded_width_matches_the_model(fam, A, masked, dt, mode):
    tree = group_of(fam) == "tree"
    if fam == "sweep":
        _, _, done = table_case(fam, sweep_width_mdp(A, masked), A, masked, dt, mode, sweep_width_models(fam, A, masked, dt, mode))
    else:
        S = 100 if fam == "dyna" else TREE_S if tree else 300
        _, _, done = hash_case(fam, S, A, masked, dt, mode, _sample(A),
                               models=tree_width_models(fam, A, masked, dt, mode) if tree else None)
    if A > 1:  # (at A = 1 explore and greedy coincide and every row has one candidate: the walk is a fixed cycle)
        assert any(np.any(t) for run, _, _ in done.values() for t in tables_of(run)), "no compared run learned anything"


# ---- 2. the selection threshold at 10 / 11 actions, on tables with NaN and infinite cells ------------------------------------
NAN_SHAPES = [(10, True), (11, True), (11, False), (5, False)]  # list selection / NumPy-style / list (unmasked) / padded list
NAN_S = 30


def _steps(fam):
    """Steps of a case that needs every model run (Dyna-Q's model takes 1 + 4 table updates per step)."""
    return 100 if fam == "dyna" else 150


NAN_CASES = [pytest.param(family, A, masked, id=f"{family}-A{A}-{'masked' if masked else 'plain'}")
             for family in EIGHT for A, masked in NAN_SHAPES]


@functools.lru_cache(maxsize=None)
def nan_case(family, A, masked):
    """The inputs and the model's side of one case: a dict of fam, dt, mode, sched, q0, qb0, done and flagged."""
    i = NAN_SHAPES.index((A, masked))
    fam = _rotated(family, i)
    dt, mode = COMBOS[(i + EIGHT.index(family)) % 4]
    sched = _schedules(M_ODD)
    q0, qb0 = dq.special_case("both", A, dt, S=NAN_S) if fam == "double" else (special_tables(M_ODD, NAN_S, A, dt, seed=A), None)
    done, flagged = run_models(fam, lambda r: hash_model_env(r, NAN_S, A, masked), range(M_ODD), _steps(fam), sched, 0, dt,
                               mode, q0, qb0)
    return {"fam": fam, "dt": dt, "mode": mode, "sched": sched, "q0": q0, "qb0": qb0, "done": done, "flagged": flagged}


def compare_with_flagged_runs(c, S, A, masked, K, seed=0, env_seed=1):
    """The call of case ``c`` on the device: the runs it names are the model's, every other run is the model's run."""
    envs = _product()[1]
    fam = c["fam"]
    pop = population(fam, M_ODD, S, A, c["sched"], seed, c["dt"], c["mode"])
    pop.set_q_tables(c["q0"], *(() if c["qb0"] is None else (c["qb0"],)))
    res, raised = _run_flagged(pop, K, envs.HashTabularEnv(M_ODD, S, A, seed=env_seed, masked=masked))
    reached(fam, pop, A, masked)
    snap = snapshot(fam, pop)
    assert raised == c["flagged"]  # in order; no run is left out that the model does not flag itself
    for r, (run, history, at) in c["done"].items():
        check(fam, pop, res, r, run, history, at, snap, K)
    return pop, res


@pytest.mark.parametrize(("family", "A", "masked"), NAN_CASES)
def test_the_selection_threshold_on_special_tables_matches_the_model(family, A, masked):
    c = nan_case(family, A, masked)
    assert c["flagged"] and len(c["done"]) >= (M_ODD + 1) // 2  # (tests/test_population_rule_width_cases.py, in full)
    compare_with_flagged_runs(c, NAN_S, A, masked, _steps(c["fam"]))


# ---- 3. real columns that tie with the padding ---------------------------------------------------------------------------------
TIE_FAMILIES = ["sarsa", "expected_sarsa", "dyna", "double", "tree-3", "sweep"]
TIE_CASES = [pytest.param(fam, A, id=f"{fam}-A{A}") for fam in TIE_FAMILIES for A in (3, 5)]


def tie_inputs(fam, A):
    """Unmasked rows of A in 4 or 8 columns: every third run starts with one whole row of -inf (``rows``: run -> row) in
    an otherwise finite table (Double Q: in both tables), and the runs alternate between epsilon 0 and 0.3."""
    sch = _product()[2]
    dt, mode = COMBOS[(TIE_FAMILIES.index(fam) + A // 4) % 4]
    rng = np.random.default_rng(100 + A)
    q0 = rng.standard_normal((M_ODD, NAN_S, A)).astype(dt)
    qb0 = rng.standard_normal((M_ODD, NAN_S, A)).astype(dt) if fam == "double" else None
    rows = {r: int(rng.integers(0, NAN_S)) for r in range(0, M_ODD, 3)}
    for r, s in rows.items():
        q0[r, s] = -np.inf
        if qb0 is not None:
            qb0[r, s] = -np.inf
    _, lr_s, gamma = _schedules(M_ODD)
    eps_s = [sch.ConstantSchedule(0.3 if r % 2 else 0.0) for r in range(M_ODD)]
    return dt, mode, (eps_s, lr_s, gamma), q0, qb0, rows


@functools.lru_cache(maxsize=None)
def tie_case(fam, A):
    dt, mode, sched, q0, qb0, rows = tie_inputs(fam, A)
    done, flagged = run_models(fam, lambda r: hash_model_env(r, NAN_S, A, False), range(M_ODD), _steps(fam), sched, 0, dt,
                               mode, q0, qb0)
    return {"fam": fam, "dt": dt, "mode": mode, "sched": sched, "q0": q0, "qb0": qb0, "done": done, "flagged": flagged,
            "rows": rows}


def wrote_into_its_row(c, r):
    """Run r (completed) has changed a cell of the row that started as -inf."""
    s = c["rows"][r]
    return any(not np.array_equal(t[s], np.full_like(t[s], -np.inf)) for t in tables_of(c["done"][r][0]))


@pytest.mark.parametrize(("fam", "A"), TIE_CASES)
def test_real_columns_that_tie_with_the_padding_keep_the_pick_inside_the_row(fam, A):
    c = tie_case(fam, A)
    assert len(c["done"]) >= (M_ODD + 1) // 2 and any(wrote_into_its_row(c, r) for r in c["rows"] if r in c["done"])
    pop, res = compare_with_flagged_runs(c, NAN_S, A, False, _steps(fam))
    if fam == "sarsa":  # the pick made last, for the next step, lies inside the row (a flagged run may hold none: -1)
        pending = res.state_dict["pending_actions"]
        assert (pending < A).all() and (pending[list(c["done"])] >= 0).all()
    if group_of(fam) == "tree":  # ... and so does every action a completed run holds in its window
        assert (res.state_dict["tree_backup_window"]["actions"][list(c["done"])] < A).all()
    if fam == "sweep":  # ... and every queue cell and every list link comes back in the host numbering s * A + a
        cells, links = res.state_dict["sweep_queue"]["cells"], pop.planning_model["pred_next"]
        assert (cells >= 0).any() and (links >= 0).any()
        assert (cells < NAN_S * A).all() and (links < NAN_S * A).all() and (pop.planning_model["pred_head"] < NAN_S * A).all()
    # a pick at or above A would store into a padding column and leave the real cell as it was: the real columns of
    # every compared run equal the model's (above), and the runs differ from their start
    assert not np.array_equal(pop.q_tables, c["q0"], equal_nan=True)


# ---- 4. counters and agent ids at 2^32, per family -----------------------------------------------------------------------------
STEP0 = 2**32 - 70   # a 150-step call: the step whose successor counter is exactly 2^32 is step 69 of the call
OFFSET = 2**32 - 30  # run r has agent id (OFFSET + r) mod 2^32: 2^32 - 30 .. 36
WRAP_SHAPE = {"sarsa": (9, True), "expected_sarsa": (5, False), "nstep": (17, True), "trace": (3, False), "dyna": (5, True),
              "double": (9, False), "tree": (33, True),  # Tree Backup: a 64-bit lane mask
              "sweep": (33, False)}  # ... and sweeping the same unmasked: NV = 16, which no other sweep case reaches


@pytest.mark.parametrize("family", EIGHT)
def test_a_step_counter_crossing_2_pow_32_matches_the_model(family):
    i = EIGHT.index(family)
    A, masked = WRAP_SHAPE[family]
    _, res, done = hash_case(_rotated(family, i), 200, A, masked, *COMBOS[i % 4], _sample(i), step0=STEP0)
    assert res.state_dict["rng_step"] == STEP0 + 150 > 2**32


@pytest.mark.parametrize("family", EIGHT)
def test_a_counter_wrap_next_to_a_saved_and_restored_call_boundary_matches_the_model(family, tmp_path):
    """Two calls of 75 steps; the second by a fresh population from the saved tables (Dyna-Q and sweeping: and model)
    and the pickled state dict.  The wrap is step 69 of the first call: the pending action, window, slots, model or
    queue cross the boundary five steps after it."""
    envs = _product()[1]
    i = EIGHT.index(family)
    fam = _rotated(family, i + 1)
    A, masked = WRAP_SHAPE[family]
    dt, mode = COMBOS[(i + 1) % 4]
    S, K, seed = 200, 75, 4
    sched = _schedules(M_ODD)

    def env():
        return envs.HashTabularEnv(M_ODD, S, A, seed=9, masked=masked)

    pop = population(fam, M_ODD, S, A, sched, seed, dt, mode)
    pop.step_counter = STEP0
    first = pop.run_steps(K, env())
    snap1 = snapshot(fam, pop)
    pop.save(tmp_path / "tables.npy")
    if fam in ("dyna", "sweep"):
        pop.save_model(tmp_path / "model.npz")
    blob = pickle.dumps(first.state_dict)
    fresh = population(fam, M_ODD, S, A, sched, seed, dt, mode)
    sd = pickle.loads(blob)
    fresh.load(tmp_path / "tables.npy")
    if fam in ("dyna", "sweep"):
        fresh.load_model(tmp_path / "model.npz")
    fresh.restore_training_state(sd)
    if fam == "sweep":  # the 7-key model and the queue are the saved ones, and some compared queue carries an entry
        dy._same_model(fresh.planning_model, snap1["model"])
        dy._same_model(fresh.sweep_queue, first.state_dict["sweep_queue"])
        assert (first.state_dict["sweep_queue"]["cells"][_sample(10 + i)] >= 0).any(), "every compared queue is empty at the cut"
    if family == "tree":  # the window carries entries from before the wrap through the pickle
        window = first.state_dict["tree_backup_window"]
        assert window["length"].max() == pop.tree_backup - 1, "the window must be non-empty at the cut"
        tb._same_window(fresh.tree_backup_window, window)
    second = fresh.run_steps(K, env(), sd)
    snap2 = snapshot(fam, fresh)
    for p in (pop, fresh):
        reached(fam, p, A, masked)
    assert first.state_dict["rng_step"] == STEP0 + K > 2**32
    for r in _sample(10 + i):
        run = model_run(fam, hash_model_env(r, S, A, masked, 9), r, sched, seed, dt, mode)
        run.rt.step_counter = STEP0
        history, at = run.run(K)
        check(fam, pop, first, r, run, history, at, snap1, STEP0 + K)
        history, at = run.run(K)
        check(fam, fresh, second, r, run, history, at, snap2, STEP0 + 2 * K)


@pytest.mark.parametrize("family", ["trace", "dyna", "tree", "sweep"])
def test_a_step_counter_crossing_2_pow_32_on_a_table_env_matches_the_model(family):
    """The table environment hashes the step too (``step >> 32`` in its word), unlike the hash environment."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    envs = _product()[1]
    arrays, isd, masks = random_mdp(300, 9, 3, seed=6, masked=True)
    mdp = encode_table_mdp(*arrays, isd, masks)
    fam = _rotated(family, 0)  # (Tree Backup: n = 5)
    dt, mode = COMBOS[{"trace": 1, "dyna": 2, "tree": 3, "sweep": 0}[family]]
    S, A, K, seed = 300, 9, 150, 2
    sched = _schedules(M_ODD)
    pop = population(fam, M_ODD, S, A, sched, seed, dt, mode)
    pop.step_counter = STEP0
    res = pop.run_steps(K, envs.TabularMDPEnv(M_ODD, mdp, seed=3))
    reached(fam, pop, A, True)
    snap = snapshot(fam, pop)
    done, flagged = run_models(fam, lambda r: TableMDPVecEnv(1, mdp, seed=3, agent_offset=r), _sample(20), K, sched, seed,
                               dt, mode, step0=STEP0)
    assert not flagged
    for r, (run, history, at) in done.items():
        check(fam, pop, res, r, run, history, at, snap, STEP0 + K)
    assert res.episode_counts.sum() > 0


@pytest.mark.parametrize("family", EIGHT)
def test_agent_ids_that_wrap_past_2_pow_32_match_the_model(family):
    i = EIGHT.index(family)
    A, masked = WRAP_SHAPE[family if family in ("tree", "sweep") else SIX[(i + 3) % 6]]  # (the six trade shapes among themselves)
    runs = sorted(set(_sample(30 + i)) | {28, 29, 30, 31})  # ids 2^32 - 2, 2^32 - 1, 0 and 1
    hash_case(_rotated(family, i + 2), 200, A, masked, *COMBOS[(i + 2) % 4], runs, offset=OFFSET)


# ---- 5. carried state through the host at a padded width ------------------------------------------------------------------------
def _same_result(a, b):
    """Two calls' results are equal, state dicts with their nested dicts included."""
    for field in ("mean_returns", "episode_counts", "returns", "offsets", "steps"):
        assert np.array_equal(getattr(a, field), getattr(b, field), equal_nan=True), field
    assert sorted(a.state_dict) == sorted(b.state_dict)
    for key, value in b.state_dict.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(a.state_dict[key], value), key
        elif isinstance(value, dict):
            for k2 in value:
                assert np.array_equal(a.state_dict[key][k2], value[k2]), (key, k2)


DYNA_HOST = {"M": M_ODD, "K1": 300, "K2": 75, "seed": 3, "env_seed": 3, "mdp_seed": 2, "dt": np.float32, "mode": "vec"}


def dyna_host_inputs(S, A):
    """A small unmasked stochastic table MDP in which every cell can be reached (the hash environment's walks leave cells
    out at these sizes), and schedules that explore in at least half the steps, so that most runs see every cell."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    sch = _product()[2]
    arrays, isd, _ = random_mdp(S, A, 3, seed=DYNA_HOST["mdp_seed"], start_support=3)
    _, lr_s, gamma = _schedules(M_ODD)
    eps_s = [sch.ConstantSchedule(0.5 + 0.005 * r) for r in range(M_ODD)]
    return encode_table_mdp(*arrays, isd), (eps_s, lr_s, gamma)


def dyna_host_models(S, A):
    """The model runs of the Dyna-Q case below after its first call, for the sample of runs that is compared with the
    model: {run: (model run, history, steps)}."""
    c = DYNA_HOST
    mdp, sched = dyna_host_inputs(S, A)
    done, flagged = run_models("dyna", lambda r: TableMDPVecEnv(1, mdp, seed=c["env_seed"], agent_offset=r), _sample(60),
                               c["K1"], sched, c["seed"], c["dt"], c["mode"])
    assert not flagged
    return done


@pytest.mark.parametrize(("S", "A"), [(4, 3), (6, 5)])  # rows of 4 and of 8: the cell s * A + a lies at s * ld + a
def test_a_full_dyna_model_through_the_getter_and_the_setter_at_a_padded_width(S, A):
    envs = _product()[1]
    c = DYNA_HOST
    M, K1, K2, dt, mode = c["M"], c["K1"], c["K2"], c["dt"], c["mode"]
    mdp, sched = dyna_host_inputs(S, A)

    def env():
        return envs.TabularMDPEnv(M, mdp, seed=c["env_seed"])

    whole = population("dyna", M, S, A, sched, c["seed"], dt, mode)
    one = whole.run_steps(K1 + K2, env())
    pop = population("dyna", M, S, A, sched, c["seed"], dt, mode)
    first = pop.run_steps(K1, env())
    reached("dyna", pop, A, False)
    snap = snapshot("dyna", pop)
    model = snap["model"]
    dy._model_shapes(pop, model)
    done = dyna_host_models(S, A)
    full = [r for r, (run, _, _) in done.items() if run.planning_model[4] == S * A]
    assert 2 * len(full) >= len(done), "most compared runs must have seen every cell"
    for r, (run, history, at) in done.items():
        check("dyna", pop, first, r, run, history, at, snap, K1)  # arrays and list in the host numbering s * A + a
    assert (model["count"][full] == S * A).all()
    assert all(sorted(model["visited"][r]) == list(range(S * A)) for r in full)
    fresh = population("dyna", M, S, A, sched, c["seed"], dt, mode)
    fresh.set_q_tables(snap["a"])
    fresh.planning_model = model
    fresh.restore_training_state(first.state_dict)
    dy._same_model(fresh.planning_model, model)
    second = fresh.run_steps(K2, env(), first.state_dict)
    snap2 = snapshot("dyna", fresh)
    assert np.array_equal(snap2["a"], whole.q_tables)
    dy._same_model(snap2["model"], whole.planning_model)
    for key, value in one.state_dict.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(second.state_dict[key], value), key
    for r, (run, _, _) in done.items():
        history, at = run.run(K2)
        check("dyna", fresh, second, r, run, history, at, snap2, K1 + K2)
    assert one.episode_counts.sum() > 0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("family", ["trace", "nstep", "tree"])
def test_slots_and_windows_through_the_getter_and_the_setter_at_five_actions(family, masked):
    envs = _product()[1]
    key = attr = {"trace": "eligibility_traces", "nstep": "n_step_window", "tree": "tree_backup_window"}[family]
    i = 1 - int(masked) if family == "tree" else int(masked) + 2 * (family == "nstep")
    fam = "tree-5" if family == "tree" else _rotated(family, i)
    dt, mode = COMBOS[i]
    M, S, A, K1, K2, seed = M_ODD, 12, 5, 80, 70, 6
    sched = _schedules(M)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=2, masked=masked)

    whole = population(fam, M, S, A, sched, seed, dt, mode)
    one = whole.run_steps(K1 + K2, env())
    pop = population(fam, M, S, A, sched, seed, dt, mode)
    first = pop.run_steps(K1, env())
    reached(fam, pop, A, masked)
    carried = getattr(pop, attr)
    busy = carried["values"] != 0 if family == "trace" else carried["length"] > 0
    assert busy.any(), "nothing is carried at the cut"
    if family == "tree":
        assert sorted(carried) == sorted(tb.WINDOW_KEYS)
        held = np.arange(carried["greedy"].shape[1])[None, :] < carried["length"][:, None]
        assert ((carried["greedy"].astype(bool) & held).any(axis=1) & (~carried["greedy"].astype(bool) & held).any(axis=1)).any(), \
            "no window holds both a set and a cleared flag at the cut"
    for k2, value in first.state_dict[key].items():
        assert np.array_equal(carried[k2], value), k2
    fresh = population(fam, M, S, A, sched, seed, dt, mode)
    fresh.set_q_tables(pop.q_tables)
    fresh.restore_training_state(first.state_dict)
    setattr(fresh, attr, carried)
    for k2, value in getattr(fresh, attr).items():
        assert np.array_equal(value, carried[k2]), k2
    second = fresh.run_steps(K2, env(), first.state_dict)
    snap1, snap2 = snapshot(fam, pop), snapshot(fam, fresh)
    assert np.array_equal(snap2["a"], whole.q_tables)
    for k, value in one.state_dict.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(second.state_dict[k], value), k
    for k2, value in one.state_dict[key].items():
        assert np.array_equal(second.state_dict[key][k2], value), k2
    for r in _sample(40 + i):
        run = model_run(fam, hash_model_env(r, S, A, masked, 2), r, sched, seed, dt, mode)
        history, at = run.run(K1)
        check(fam, pop, first, r, run, history, at, snap1, K1)
        history, at = run.run(K2)
        check(fam, fresh, second, r, run, history, at, snap2, K1 + K2)


# ---- 6. greedy evaluation at the same widths --------------------------------------------------------------------------------------
EVAL_WIDTHS = [1, 3, 5, 9, 17, 33, 63]
EVAL_S, EVAL_K, EVAL_V, EVAL_E = 16, 120, 100, 2
CHECK = (0, 1, 33, 63, 64, 66)
EVAL_CASES = [pytest.param(A, masked, id=f"A{A}-{'masked' if masked else 'plain'}") for A in EVAL_WIDTHS for masked in (False, True)]


def _eval_reached(pop, double, A, masked):
    d = _product()[0].decode_variant(pop.last_stats["kernel_variant"])
    assert d["path"] == ("population_double_eval" if double else "population_eval"), d
    assert d["nv"] == _nv(A) and d["masked"] == masked, d


def _slippery(A, masked):
    """Episodes end under any policy (test_gpu_population_eval.py): the hash environment's greedy walks may never end."""
    from test_gpu_population_eval import _slippery_mdp

    return _slippery_mdp(_product()[1], S=EVAL_S, A=A, masked=masked)


@pytest.mark.parametrize(("A", "masked"), EVAL_CASES)
def test_single_table_evaluation_at_every_width_matches_the_standalone(A, masked):
    from test_gpu_population_eval import _env_state, _standalone, _train

    envs = _product()[1]
    wi = EVAL_WIDTHS.index(A)
    dt = COMBOS[(wi + int(masked)) % 4][0]
    M, S, K, V, E = M_ODD, EVAL_S, EVAL_K, EVAL_V, EVAL_E
    mdp = _slippery(A, masked)
    sched = _schedules(M)

    def hash_env(n, off, seed):
        return envs.HashTabularEnv(n, S, A, seed=seed, masked=masked, agent_offset=off)

    pop = population("q_learning", M, S, A, sched, 11, dt, "iter")
    pop.run_steps(K, hash_env(M, 0, 2))
    tables = pop.q_tables
    val = hash_env(M, 0, 5)
    by_steps = pop.evaluate_steps(val, V)
    _eval_reached(pop, False, A, masked)
    obs, acc, aux = _env_state(val)
    by_episodes = pop.evaluate_episodes(envs.TabularMDPEnv(M, mdp, seed=9), E)
    _eval_reached(pop, False, A, masked)
    assert by_episodes.finished.all() and (by_episodes.episode_counts == E).all()
    assert np.array_equal(pop.q_tables.view(np.uint8), tables.view(np.uint8))
    for r in CHECK:
        rt = _standalone(r, S, A, sched, 11, dt)
        _train(rt, K, hash_env(1, r, 2))
        assert np.array_equal(tables[r], np.asarray(rt.algorithm.q_table)), f"run {r}: table"
        v1 = hash_env(1, r, 5)
        total, history = rt.evaluate_steps(v1, V)
        assert np.array_equal(by_steps.run_returns(r), np.array(history, dtype=np.float32)), f"run {r}: returns"
        assert by_steps.totals[r] == total and by_steps.episode_counts[r] == len(history), r
        o1, a1, x1 = _env_state(v1)
        assert (obs[r], acc[r], aux[r]) == (o1[0], a1[0], x1[0]), f"run {r}: final state"
        total, history = rt.evaluate_episodes(envs.TabularMDPEnv(1, mdp, seed=9, agent_offset=r), E)
        assert np.array_equal(by_episodes.run_returns(r), np.array(history, dtype=np.float32)), f"run {r}: episode returns"
        assert by_episodes.totals[r] == total, r
        assert by_episodes.steps_used[r] == rt.algorithm.step_counter - K - V, r
        assert pop.step_counters[r] == rt.algorithm.step_counter, r


@pytest.mark.parametrize(("A", "masked"), EVAL_CASES)
def test_double_q_evaluation_at_every_width_matches_the_model(A, masked):
    envs = _product()[1]
    wi = EVAL_WIDTHS.index(A)
    dt, mode = COMBOS[(wi + int(masked) + 1) % 4]
    M, S, K, V, E = M_ODD, EVAL_S, EVAL_K, EVAL_V, EVAL_E
    mdp = _slippery(A, masked)
    sched = _schedules(M)
    pop = population("double", M, S, A, sched, 8, dt, mode)
    pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=2, masked=masked))
    ta, tb = pop.q_tables, pop.q_tables_b
    by_steps = pop.evaluate_steps(envs.HashTabularEnv(M, S, A, seed=5, masked=masked), V)
    _eval_reached(pop, True, A, masked)
    by_episodes = pop.evaluate_episodes(envs.TabularMDPEnv(M, mdp, seed=9), E)
    _eval_reached(pop, True, A, masked)
    assert by_episodes.finished.all() and (by_episodes.episode_counts == E).all()
    assert np.array_equal(pop.q_tables, ta) and np.array_equal(pop.q_tables_b, tb)  # no store
    done, flagged = run_models("double", lambda r: hash_model_env(r, S, A, masked, 2), _sample(50 + wi), K, sched, 8, dt, mode)
    assert not flagged
    for r, (run, _, _) in done.items():
        assert np.array_equal(ta[r], run.qa) and np.array_equal(tb[r], run.qb), f"run {r}: tables"
        total, history = run.evaluate_steps(hash_model_env(r, S, A, masked, 5), V)
        assert np.array_equal(by_steps.run_returns(r), np.array(history, dtype=np.float32)), f"run {r}: returns"
        assert by_steps.totals[r] == np.float32(total) and by_steps.episode_counts[r] == len(history), r
        before = run.rt.step_counter
        assert before == K + V
        total, history = run.evaluate_episodes(TableMDPVecEnv(1, mdp, seed=9, agent_offset=r), E)
        assert np.array_equal(by_episodes.run_returns(r), np.array(history, dtype=np.float32)), f"run {r}: episode returns"
        assert by_episodes.totals[r] == np.float32(total), r
        assert by_episodes.steps_used[r] == run.rt.step_counter - before, r
        assert pop.step_counters[r] == run.rt.step_counter, r


EVAL_NAN_SHAPES = [(10, False), (10, True), (11, False), (11, True)]  # evaluation takes the NumPy-style selection above 10
EVAL_NAN_S, EVAL_NAN_V = 30, 60
EVAL_NAN_CASES = [pytest.param(A, masked, id=f"A{A}-{'masked' if masked else 'plain'}") for A, masked in EVAL_NAN_SHAPES]


def eval_nan_tables(A, masked, double):
    i = EVAL_NAN_SHAPES.index((A, masked))
    dt = COMBOS[(i + int(double)) % 4][0]
    if double:
        return dq.special_case("both", A, dt, S=EVAL_NAN_S)
    return special_tables(M_ODD, EVAL_NAN_S, A, dt, seed=A + 7), None


def _flag_empty_picks(rt):
    """The oracle's greedy evaluation hands the list selection's -1 (a row without a number) on to the environment; every
    engine path raises IndexError for such a run (tests/test_gpu_population_limits.py, ``_run_catching``), as
    ``TdRuntime._pick`` does for the training steps.  The same for the evaluation's picks of ``rt``."""
    greedy = rt._greedy

    def pick(states):
        actions = greedy(states)
        if actions[0] < 0:
            msg = "Cannot choose from an empty sequence"
            raise IndexError(msg)
        return actions

    rt._greedy = pick


@functools.lru_cache(maxsize=None)
def eval_nan_case(A, masked, double):
    """The model's side of a greedy evaluation of the seeded tables: {run: (total, history)} and the runs it flags.  The
    single-table population is the Q-learning model's oracle runtime here (the device test compares with the standalone)."""
    q0, qb0 = eval_nan_tables(A, masked, double)
    sched = _schedules(M_ODD)
    done, flagged = {}, []
    for r in range(M_ODD):
        env = hash_model_env(r, EVAL_NAN_S, A, masked, 5)
        if double:
            run = model_run("double", env, r, sched, 3, q0.dtype, "iter", q0[r], qb0[r])
            evaluate = run.evaluate_steps
        else:
            run = TdRun(env, "q_learning", sched[2][r], sched[0][r], sched[1][r], seed=3, dtype=q0.dtype, q0=q0[r])
            evaluate = run.rt.evaluate_steps
        _flag_empty_picks(run.rt)
        try:
            done[r] = evaluate(env, EVAL_NAN_V)
        except IndexError:
            flagged.append(r)
    return {"q0": q0, "qb0": qb0, "done": done, "flagged": flagged}


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
@pytest.mark.parametrize(("A", "masked"), EVAL_NAN_CASES)
def test_evaluation_of_seeded_nan_tables_at_the_threshold(A, masked, double):
    from test_gpu_population_eval import _standalone

    envs = _product()[1]
    c = eval_nan_case(A, masked, double)
    q0, qb0 = c["q0"], c["qb0"]
    S, V = EVAL_NAN_S, EVAL_NAN_V
    sched = _schedules(M_ODD)
    pop = population("double" if double else "q_learning", M_ODD, S, A, sched, 3, q0.dtype, "iter")
    pop.set_q_tables(q0, *((qb0,) if double else ()))
    try:
        res, bad = pop.evaluate_steps(envs.HashTabularEnv(M_ODD, S, A, seed=5, masked=masked), V), []
    except IndexError as err:
        assert str(err).startswith("Cannot choose from an empty sequence (runs ")
        res, bad = err.result, err.runs
    _eval_reached(pop, double, A, masked)
    assert bad == c["flagged"]
    assert len(c["done"]) >= (M_ODD + 1) // 2
    for r, (total, history) in c["done"].items():
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), f"run {r}: returns"
        assert res.totals[r] == np.float32(total) and res.episode_counts[r] == len(history), r
    if not double:  # ... and the standalone one-agent evaluation says the same
        for r in sorted(set(CHECK) | set(bad)):
            rt = _standalone(r, S, A, sched, 3, q0.dtype)
            rt.algorithm.q_table = q0[r]
            try:
                total, history = rt.evaluate_steps(envs.HashTabularEnv(1, S, A, seed=5, masked=masked, agent_offset=r), V)
            except IndexError:
                assert r in bad, r
                continue
            assert r not in bad, r
            assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)) and res.totals[r] == total, r
