"""The inputs of tests/test_gpu_population_rule_widths.py keep enough runs to test something: properties of the NumPy
models alone, checked without a device.

A case on tables with NaN, +inf and -inf cells that loses most of its runs to ``IndexError`` compares nothing.  Each such
case is built here by the very functions the GPU module calls (``nan_case``, ``tie_case``, ``eval_nan_case``,
``dyna_host_models``) and must satisfy:

* the model completes at least half of its runs;
* at least one run is flagged (the cases at the 10 / 11 threshold);
* at least one completed run ends with a non-finite cell;
* the -inf-row cases: at least one completed run has written into its -inf row.

Tree Backup (``tree_backup_model.py``) has conditions of its own, counted by ``tree_backup_cases.with_census``:

* the width cases of one horizon together perform every kind of update in ``tree_backup_cases.required``, and every
  case with more than one action performs an update with a cut and one without;
* the width cases of horizons 5 and 16 together reach all four sources of the value at the cut
  (``tree_backup_cases.BRANCHES``), those of horizon 2 all but the cut among the old entries, which it cannot have;
* over the masked threshold cases, some update reads a cut row whose NaN sits in masked-out columns only and some
  update reads one with a NaN in a valid column -- and some of either through the kernel's own walk of a row
  (``row_np_max_at``), which a horizon of 2 never takes.

Prioritized sweeping (``sweep_model.py``) is counted by the model's own ``events``: the 16 width cases together reach the
queue's, the lists' and the held row's branches, every one with more than one action inserts, uses all its pops and
unlinks; the special-table cases take row maxima over hidden and over valid NaNs and pop infinite priorities; the wrap
case crosses its call boundary with a queued entry.

Every test prints the figures it asserts on (``pytest -s``).
"""
import numpy as np
import pytest

import test_gpu_population_rule_widths as cases
import tree_backup_cases as tbc

HALF = (cases.M_ODD + 1) // 2


def _non_finite(done):
    return sum(not all(np.isfinite(t).all() for t in cases.tables_of(run)) for run, _, _ in done.values())


@pytest.mark.parametrize(("family", "A", "masked"), cases.NAN_CASES)
def test_the_threshold_cases_keep_half_their_runs_flag_some_and_keep_special_cells(family, A, masked):
    c = cases.nan_case(family, A, masked)
    kept = _non_finite(c["done"])
    print(f"{c['fam']} A={A} masked={masked}: completed {len(c['done'])} of {cases.M_ODD}, flagged {len(c['flagged'])}, "
          f"completed with a non-finite cell {kept}")
    assert len(c["done"]) + len(c["flagged"]) == cases.M_ODD
    assert len(c["done"]) >= HALF
    assert c["flagged"]
    assert kept >= 1


@pytest.mark.parametrize(("fam", "A"), cases.TIE_CASES)
def test_the_minus_infinity_row_cases_keep_half_their_runs_and_write_into_the_row(fam, A):
    c = cases.tie_case(fam, A)
    wrote = [r for r in c["rows"] if r in c["done"] and cases.wrote_into_its_row(c, r)]
    kept = _non_finite(c["done"])
    print(f"{fam} A={A}: completed {len(c['done'])} of {cases.M_ODD}, flagged {len(c['flagged'])}, completed with a "
          f"non-finite cell {kept}, completed and wrote into the -inf row {len(wrote)} of {len(c['rows'])}")
    assert sorted(c["rows"]) == list(range(0, cases.M_ODD, 3))
    for r, s in c["rows"].items():  # one whole row of -inf in an otherwise finite table
        for t in (c["q0"], c["qb0"]) if c["qb0"] is not None else (c["q0"],):
            assert np.isneginf(t[r, s]).all() and np.isfinite(np.delete(t[r], s, axis=0)).all()
    eps = [s.get_value() for s in c["sched"][0]]
    assert eps[0::2] == [0.0] * len(eps[0::2]) and eps[1::2] == [0.3] * len(eps[1::2])
    assert len(c["done"]) >= HALF
    assert kept >= 1
    assert wrote


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
@pytest.mark.parametrize(("A", "masked"), cases.EVAL_NAN_CASES)
def test_the_evaluation_cases_keep_half_their_runs(A, masked, double):
    c = cases.eval_nan_case(A, masked, double)
    tables = (c["q0"],) if c["qb0"] is None else (c["q0"], c["qb0"])
    kept = sum(not all(np.isfinite(t[r]).all() for t in tables) for r in c["done"])
    print(f"evaluation A={A} masked={masked} double={double}: completed {len(c['done'])} of {cases.M_ODD}, "
          f"flagged {len(c['flagged'])}, completed on a table with a non-finite cell {kept}")
    assert len(c["done"]) >= HALF
    assert kept >= 1
    if A > 10:  # the NumPy-style selection: a NaN maximum has no candidate
        assert c["flagged"]


@pytest.mark.parametrize(("S", "A"), [(4, 3), (6, 5)])
def test_most_dyna_runs_see_every_cell_before_the_model_goes_through_the_host(S, A):
    done = cases.dyna_host_models(S, A)
    full = sum(run.planning_model[4] == S * A for run, _, _ in done.values())
    print(f"Dyna-Q S={S} A={A}: {full} of {len(done)} runs have seen all {S * A} cells")
    assert len(done) >= 10 and 2 * full >= len(done)


def test_every_family_meets_every_dtype_and_learn_mode_in_the_width_sweep():
    met = {}
    for p in cases.WIDTH_CASES:
        fam, _, _, dt, mode = p.values
        met.setdefault(cases.group_of(fam), set()).add((dt, mode))
    assert sorted(met) == sorted([*cases.FAMILIES, "tree", "sweep"])
    assert all(len(v) == 4 for v in met.values()), met
    tree = cases.TREE_WIDTH_CASES
    assert [(A, masked) for _, A, masked, _, _ in tree] == [(A, masked) for A in cases.WIDTHS for masked in (False, True)]
    for fam, A, masked, _, _ in tree:
        assert fam == f"tree-{tbc.HORIZONS[(cases.WIDTHS.index(A) + int(masked)) % 3]}", (fam, A, masked)
    # the ids, dtypes and learn modes of the other families' cases are those they had before Tree Backup and
    # prioritized sweeping were appended
    assert [p.id for p in cases.WIDTH_CASES[:3]] == ["sarsa-A1-plain", "sarsa-A1-masked", "sarsa-A2-plain"]
    assert cases.WIDTH_CASES[len(cases.FAMILIES) * 16 - 1].id == "double-A63-masked"
    assert cases.WIDTH_CASES[(len(cases.FAMILIES) + 1) * 16 - 1].id == "tree-16-A63-masked"
    assert len(cases.WIDTH_CASES) == (len(cases.FAMILIES) + 2) * 16
    assert [(A, masked) for _, A, masked, _, _ in cases.SWEEP_WIDTH_CASES] == [(A, masked) for A in cases.WIDTHS for masked in (False, True)]
    assert cases.SEVEN == [*cases.SIX, "tree"] and cases.EIGHT == [*cases.SEVEN, "sweep"]


def _tree_totals(which, cases_of_horizon):
    """The sum over the compared runs of the given Tree Backup width cases of the counter ``which`` of every run."""
    total = {}
    for case in cases_of_horizon:
        done, flagged = cases.tree_width_models(*case)
        assert not flagged
        for run, _, _ in done.values():
            for kind, count in getattr(run, which).items():
                total[kind] = total.get(kind, 0) + int(count)
    return total


@pytest.mark.parametrize("n", tbc.HORIZONS)
def test_the_tree_backup_width_cases_of_a_horizon_perform_every_kind_of_update(n):
    of_n = [c for c in cases.TREE_WIDTH_CASES if c[0] == f"tree-{n}"]
    assert len(of_n) >= 5 and {c[2] for c in of_n} == {False, True}
    got = _tree_totals("counts", of_n)
    print(f"tree-{n}: {len(of_n)} width cases perform {got}")
    missing = sorted(kind for kind in tbc.required({"n": n, "kind": "hash"}) if not got[kind])
    assert not missing, (missing, got)
    for case in of_n:
        one = _tree_totals("counts", [case])
        cut = one["steady_cut_next"] + one["steady_cut_deep"] + one["flush_cut"]
        plain = one["steady_no_cut"] + one["flush_no_cut"]
        print(f"  A={case[1]} masked={case[2]}: updates with a cut {cut}, without {plain}, {one}")
        if case[1] == 1:  # one action: every pick is greedy, and the walk is a fixed cycle
            assert cut == 0 and plain > 0
        else:
            assert cut > 0 and plain > 0, case


def test_the_tree_backup_width_cases_reach_every_source_of_the_value_at_the_cut():
    long = _tree_totals("branches", [c for c in cases.TREE_WIDTH_CASES if c[0] != "tree-2"])
    short = _tree_totals("branches", [c for c in cases.TREE_WIDTH_CASES if c[0] == "tree-2"])
    print(f"horizons 5 and 16: {long}\nhorizon 2: {short}")
    assert sorted(long) == sorted(short) == sorted(tbc.BRANCHES)
    assert all(long.values()), long
    assert short["steady_cut_old"] == 0  # a window of one old entry has none after entry 0
    assert all(count for kind, count in short.items() if kind != "steady_cut_old"), short


def _sweep_events(done):
    """The sum of the model's event counters over the completed runs ``done``."""
    total = {}
    for run, _, _ in done.values():
        for kind, count in run.rt.events.items():
            total[kind] = total.get(kind, 0) + int(count)
    return total


def test_the_sweep_width_cases_reach_the_branches_of_the_queue_the_lists_and_the_held_row():
    together = {}
    for case in cases.SWEEP_WIDTH_CASES:
        _, A, masked, dt, mode = case
        done, flagged = cases.sweep_width_models(*case)
        assert not flagged and sorted(done) == cases._sample(A)
        got = _sweep_events(done)
        print(f"sweep A={A} masked={masked} {np.dtype(dt).name} {mode}: {dict(sorted(got.items()))}")
        for kind, count in got.items():
            together[kind] = together.get(kind, 0) + count
        if A > 1:
            assert got.get("insert_free") and got.get("all_pops_used") and got.get("unlinked"), case
    print(f"the 16 sweep width cases together: {dict(sorted(together.items()))}")
    for kind in ("evicted", "dropped", "insert_raises", "insert_hole", "unlink_inner", "patched_held_row", "propagate_held",
                 "propagate_other", "queue_ran_empty"):
        assert together.get(kind), kind


def test_the_sweep_threshold_cases_take_row_maxima_over_hidden_and_over_valid_nans():
    total = {}
    for A, masked in cases.NAN_SHAPES:
        c = cases.nan_case("sweep", A, masked)
        got = _sweep_events(c["done"])
        print(f"sweep A={A} masked={masked}: " + ", ".join(f"{k} {got.get(k, 0)}" for k in
                                                           ("rowmax_hidden_nan", "rowmax_valid_nan", "nan_not_queued", "pop_inf")))
        if masked:
            assert got.get("rowmax_hidden_nan"), (A, masked)  # the masked cases gather rows whose NaN is hidden
        else:
            assert not got.get("rowmax_hidden_nan")
        for kind, count in got.items():
            total[kind] = total.get(kind, 0) + count
    for kind in ("rowmax_hidden_nan", "rowmax_valid_nan", "nan_not_queued", "pop_inf"):
        assert total.get(kind), kind


def test_the_sweep_wrap_case_crosses_its_call_boundary_with_a_queued_entry_in_a_compared_run():
    i = cases.EIGHT.index("sweep")
    A, masked = cases.WRAP_SHAPE["sweep"]
    assert cases._nv(A) == 16 and not masked
    dt, mode = cases.COMBOS[(i + 1) % 4]
    queued = 0
    for r in cases._sample(10 + i):
        run = cases.model_run("sweep", cases.hash_model_env(r, 200, A, masked, 9), r, cases._schedules(cases.M_ODD), 4, dt, mode)
        run.rt.step_counter = cases.STEP0
        run.run(75)
        queued += max(run.rt.cells) >= 0
    print(f"sweep, two calls of 75 steps around 2^32: {queued} of {len(cases._sample(10 + i))} compared queues hold an entry at the cut")
    assert queued >= 1


def test_the_masked_tree_backup_threshold_cases_read_cut_rows_with_hidden_and_with_valid_nans():
    total = dict.fromkeys(tbc.CUT_ROWS, 0)
    for A, masked in cases.NAN_SHAPES:
        c = cases.nan_case("tree", A, masked)
        got = dict.fromkeys(tbc.CUT_ROWS, 0)
        for run, _, _ in c["done"].values():
            for kind, count in run.cut_rows.items():
                got[kind] += count
        print(f"{c['fam']} A={A} masked={masked}: cut rows read by completed runs {got}")
        if masked:
            for kind, count in got.items():
                total[kind] += count
        else:
            assert not any(got.values())  # (no column is masked out, and the census counts masked rows only)
    assert all(total.values()), total
