"""The training cases of tests/test_gpu_tree_backup.py, built without a device, and their model runs.

Every case is a population of ``M`` runs for ``K`` steps; ``model(case)`` runs the NumPy model of every run once (cached:
the coverage test and the GPU tests of one session share it) and is never changed afterwards.

Coverage (tests/test_tree_backup_cases.py): the model runs of every case together perform each kind of update in
``required(case)`` at least once -- all of ``tree_backup_model.KINDS``, less what the case's structure rules out:

* ``n = 2``: the window of a steady update holds entries 0 and 1, so its nearest cut can only be ``i = j + 1``: no
  ``steady_cut_deep``;
* episodes shorter than ``n`` (``bandit_mc``): the window never fills, every update belongs to a flush: no steady kind;
* TicTacToe: a window holds entries of one episode only (a terminated step empties it) and every move adds a mark, so the
  states of a window are distinct, and s' has either one mark more than all of them or is a start position with fewer
  than any entry after the first: no ``cut_own_state``.

The grid world pays only at the goal, so from a zero table every action ties and no cut would ever occur: its runs start
from ``initial_tables`` -- multiples of 0.25, which keep ties as well.

A case that misses a kind gets another seed, epsilon, K or initial table -- the condition is not weakened.
"""
from functools import lru_cache

import numpy as np

from tree_backup_model import KINDS, TreeBackupRun

M_ODD = 67  # a full and a partial wavefront
K_STEPS = 150
HORIZONS = (2, 5, 16)
WIDTHS = (4, 8, 16, 20, 64)
NAN_CASE = {"M": M_ODD, "S": 30, "K": 150, "n": 3, "seed": 0, "env_seed": 1}


def nv_of(A):
    return max(4, 1 << (A - 1).bit_length()) // 4


def _hash_cases():
    out = []
    k = 0
    for A in WIDTHS:
        for masked in (False, True):
            for dt in ("float32", "float64"):
                for mode in ("iter", "vec"):
                    n = HORIZONS[k % 3]
                    k += 1
                    if (A, masked, dt) == (64, True, "float64"):
                        n = 16  # the widest build at the longest horizon
                    out.append({"id": f"hash-A{A}-{'masked' if masked else 'plain'}-{dt}-{mode}-n{n}", "kind": "hash",
                                "S": 40, "A": A, "p": {"S": 40, "A": A, "seed": 1, "masked": masked}, "n": n, "dt": dt,
                                "mode": mode, "seed": 0, "nv": nv_of(A), "masked": masked})
    return out


def _other_cases():
    out = []
    specs = (("grid", 36, 4, {"side": 6, "seed": 2}, 1, False, 3),
             # one state: every window repeats cells, every store lands in the held row, every cut state is s'
             ("bandit", 1, 2, {"episode_len": 7}, 1, False, 3),
             ("bandit_mc", 1, 2, {"episode_len": 3}, 1, False, 5),  # episodes shorter than the horizon: flush only
             ("tictactoe", 19683, 9, {"seed": 5}, 4, True, 3),
             ("table", 20, 5, {"mdp_seed": 7, "seed": 3}, 2, True, 3))
    for kind, S, A, p, nv, masked, n in specs:
        for dt, mode in (("float32", "iter"), ("float64", "vec")):
            out.append({"id": f"{kind}-{dt}-{mode}-n{n}", "kind": kind, "S": S, "A": A, "p": p, "n": n, "dt": dt, "mode": mode,
                        "seed": 11, "nv": nv, "masked": masked, "q0_seed": 5 if kind == "grid" else None})
    return out


CASES = _hash_cases() + _other_cases()
for _c in CASES:
    _c.setdefault("M", M_ODD)
    _c.setdefault("K", K_STEPS)
BY_ID = {c["id"]: c for c in CASES}


def required(case):
    kinds = set(KINDS)
    if case["n"] == 2:
        kinds.discard("steady_cut_deep")
    if case["kind"] == "bandit_mc":
        kinds -= {"steady_no_cut", "steady_cut_next", "steady_cut_deep"}
    if case["kind"] == "tictactoe":
        kinds.discard("cut_own_state")
    return kinds


def initial_tables(case):
    """None (zeros), or the case's ``[M, S, A]`` start tables: 0, 0.25 or 0.5 in every cell."""
    if case.get("q0_seed") is None:
        return None
    cells = np.random.default_rng(case["q0_seed"]).integers(0, 3, size=(case["M"], case["S"], case["A"]))
    return (cells * 0.25).astype(case["dt"])


def env_params(case):
    """The parameters as tests/test_gpu_td_rules.py's ``_model_env`` / ``_device_env`` take them."""
    p = dict(case["p"])
    if case["kind"] == "table":
        from dist_classicrl_amd.environments.device_envs import encode_table_mdp
        from table_mdp_model import random_mdp

        arrays, isd, masks = random_mdp(case["S"], case["A"], 3, seed=p.pop("mdp_seed"), masked=True)
        p["mdp"] = encode_table_mdp(*arrays, isd, masks)
    return p


def model_runs(kind, p, runs, n, sched, seed, dt, mode, q0=None):
    from test_gpu_td_rules import _model_env

    eps_s, lr_s, gamma = sched
    return {r: TreeBackupRun(_model_env(kind.split("_")[0], r, p), gamma[r], eps_s[r], lr_s[r], n=n, seed=seed, dtype=dt,
                             mode=mode, agent_id=r, q0=None if q0 is None else q0[r]) for r in runs}


@lru_cache(maxsize=None)
def model(case_id):
    """``{r: (run, history, episode steps)}`` of the case's model runs after its K steps."""
    from test_gpu_population import _schedules

    c = BY_ID[case_id]
    runs = model_runs(c["kind"], env_params(c), range(c["M"]), c["n"], _schedules(c["M"]), c["seed"], np.dtype(c["dt"]), c["mode"],
                      q0=initial_tables(c))
    return {r: (run, *run.run(c["K"])) for r, run in runs.items()}


def performed(case_id):
    total = dict.fromkeys(KINDS, 0)
    for run, _, _ in model(case_id).values():
        for kind, count in run.counts.items():
            total[kind] += int(count)
    return total


BRANCHES = ("steady_cut_old", "steady_cut_own", "flush_first_full", "flush_first_short")
CUT_ROWS = ("nan_hidden", "nan_valid", "gathered_nan_hidden", "gathered_nan_valid")


def with_census(run):
    """``run`` with two counters of its own, filled as it runs, read from the model's windows (``KINDS`` stay as they are).

    ``run.branches``: the sources the kernel's step has for the value at the cut, which ``KINDS`` do not tell apart --
    ``steady_cut_old``: a steady update whose nearest cut lies among the entries the step started with (the row gathered
    at the top of the step); ``steady_cut_own``: one whose cut is the step's own entry, ``cut == L - 1`` (the held row's
    maximum); ``flush_first_full`` / ``flush_first_short``: the first update of a terminated step with ``L == n`` (the
    early path inside a flush) / ``L < n`` (the per-entry path for entry 0).

    ``run.cut_rows``: the reads of a cut row (every ``_row_max`` of a step after its first, which is the flag's) with a
    NaN in masked-out columns only (``nan_hidden``: the maximum stays a number) and with one in a valid column
    (``nan_valid``: the fold carries NaN); ``gathered_...``: those of them that the kernel reads from the table
    (``row_np_max_at``), which is every cut but the one at the step's own entry seen from entry 0 of a full window, whose
    row is the held row.  With ``n = 2`` no cut row is ever gathered."""
    rt = run.rt
    run.branches = dict.fromkeys(BRANCHES, 0)
    run.cut_rows = dict.fromkeys(CUT_ROWS, 0)
    count, row_max, step = rt._count, rt._row_max, rt.run_single_step
    calls, last = [0], [None]

    def counted(j, L, cut, start, terminated, s_j, n_obs):
        if last[0] is not None and not (j == 0 and L == rt.n and cut == L - 1):
            run.cut_rows["gathered_" + last[0]] += 1
        last[0] = None
        if terminated:
            if j == 0:
                run.branches["flush_first_full" if L == rt.n else "flush_first_short"] += 1
        elif cut is not None:
            run.branches["steady_cut_own" if cut == L - 1 else "steady_cut_old"] += 1
        return count(j, L, cut, start, terminated, s_j, n_obs)

    def read(s, mask):
        calls[0] += 1
        if calls[0] > 1 and mask is not None:
            nan = np.isnan(rt.algorithm.q_table[s])
            last[0] = "nan_valid" if nan[np.where(mask)].any() else "nan_hidden" if nan.any() else None
            if last[0] is not None:
                run.cut_rows[last[0]] += 1
        return row_max(s, mask)

    def one_step(*args):
        calls[0] = 0
        return step(*args)

    rt._count, rt._row_max, rt.run_single_step = counted, read, one_step
    return run


def special_tables(M, S, A, dt, seed):
    """The NaN / infinity tables of tests/test_gpu_td_rules.py, and in every run r two TIE rows: row ``r % S`` all equal,
    row ``(r + 1) % S`` with its first two columns equal and above the rest."""
    from test_gpu_td_rules import _special_tables

    q = _special_tables(M, S, A, dt, seed)
    for r in range(M):
        q[r, r % S] = 0.5
        q[r, (r + 1) % S] = -1.0
        q[r, (r + 1) % S, :2] = 2.0
    return q


def nan_case_model(A, masked, dt, mode, check=None):
    """The model's side of the special-table case: the runs whose pick finds no candidate, and how many of the others
    end with a non-finite cell.  ``check(r, run, history, at)`` is called for every run that is compared."""
    from test_gpu_population import _schedules

    c = NAN_CASE
    q0 = special_tables(c["M"], c["S"], A, dt, seed=A)
    p = {"S": c["S"], "A": A, "seed": c["env_seed"], "masked": masked}
    raised, special_kept = [], 0
    for r, run in model_runs("hash", p, range(c["M"]), c["n"], _schedules(c["M"]), c["seed"], dt, mode, q0=q0).items():
        try:
            history, at = run.run(c["K"])
        except IndexError:
            raised.append(r)
            continue
        special_kept += not np.isfinite(run.q).all()
        if check is not None:
            check(r, run, history, at)
    return raised, special_kept
