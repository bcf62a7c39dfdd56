"""CPU, no device: the GPU cases of tests/test_gpu_sweep.py reach every branch of prioritized sweeping.

A bit-for-bit comparison shows only what its inputs exercise.  Here the NumPy model (tests/sweep_model.py) runs the very
cases the GPU tests run -- the same environments, schedules, thresholds, queue lengths and seeds, a dozen of their 67 runs
each -- and its event counters say which branches of the rule those runs took.  Every branch below is met by at least one
run of the case named beside it.  These are conditions on the cases, not measurements of the kernel.
"""
from collections import Counter

import numpy as np
import pytest

import test_gpu_sweep as cases

RUNS = range(12)


def _events(runs, steps):
    """Per event: in how many of the runs it happened; and in how many one cell's flag turned both on and off."""
    seen, both = Counter(), 0
    for run in runs.values():
        try:
            run.run(steps)
        except IndexError:  # (a run without a selectable action: the GPU test leaves it out as well)
            continue
        for key, count in run.rt.events.items():
            seen[key] += bool(count)
        flips = run.rt.flag_flips
        both += any((c, True) in flips and (c, False) in flips for c, _ in flips)
    return seen, both


@pytest.fixture(scope="module")
def reached():
    out = {}
    for name in ("hash-8-masked", "K1", "K32", "n64", "four-4-plain", "bandit", "frozen"):
        out[name] = _events(cases.model_runs(name, RUNS, np.float32, "iter"), cases._case(name)[4])
    A, masked, dt, mode = cases.SPECIAL[0]
    out["special"] = _events(cases.special_runs(A, masked, dt, mode, RUNS)[0], 100)
    return out


@pytest.mark.parametrize(("event", "name"), [
    ("insert_free", "hash-8-masked"),       # an insert into a free slot
    ("insert_raises", "K32"),               # an insert that raises a live entry
    ("insert_keeps", "K32"),                # an insert that leaves a live entry because its priority is higher
    ("evicted", "K1"),                      # eviction of the smallest
    ("dropped", "K1"),                      # a newcomer dropped
    ("queue_ran_empty", "n64"),             # a pop from a queue that then runs empty before n
    ("all_pops_used", "hash-8-masked"),     # all n pops used
    ("unlink_inner", "frozen"),             # an unlink from a list of >= 3 nodes that is not the head
    ("self_loop", "bandit"),                # a self-loop predecessor
    ("patched_held_row", "four-4-plain"),   # a planning store patched into the held row
    ("propagate_none", "hash-8-masked"),    # a propagate that inserts nothing
    ("nan_not_queued", "special"),          # a NaN increment that is not queued
    # the tie rules, pinned: a reshuffled seed must not lose them silently
    ("pop_tie", "four-4-plain"),            # a pop among equal maxima: the lowest index
    ("pop_tie", "frozen"),
    ("evict_tie", "four-4-plain"),          # an eviction among equal smallest: the lowest index
    ("evict_tie", "frozen"),
    ("dropped_equal", "four-4-plain"),      # a newcomer equal to the smallest is dropped
    ("dropped_equal", "frozen"),
    ("insert_equal", "four-4-plain"),       # an insert equal to the live entry's priority
    ("insert_equal", "frozen"),
    ("insert_hole", "hash-8-masked"),       # an insert into a hole below a live slot
    ("unlink_head", "frozen"),              # an unlink of the head
    ("unlink_tail", "frozen"),              # ... and of the last node
])
def test_a_gpu_case_reaches_the_branch(reached, event, name):
    seen, _ = reached[name]
    assert seen[event] >= 1, (name, dict(seen))


def test_a_terminated_flag_turns_on_and_off_for_one_cell(reached):
    for name in ("bandit", "frozen"):
        seen, both = reached[name]
        assert both >= 1 and seen["flag_on"] and seen["flag_off"], (name, dict(seen))


def test_the_grid_case_sweeps_nothing_and_the_small_grid_does():
    """``grid`` at 150 steps: empty tables and empty queues.  ``grid-small``: in at least half of the runs the goal is
    reached, a propagate inserts something, all n pops of a step are used, and a state two moves from the goal holds a
    non-zero value."""
    seen, _ = _events(cases.model_runs("grid", RUNS, np.float32, "vec"), cases._case("grid")[4])
    assert not {"insert_free", "propagate_some", "all_pops_used", "queue_ran_empty"} & set(+seen) and seen["queue_was_empty"] == len(RUNS)
    _, p, _, _, steps, *_ = cases._case("grid-small")
    side = p["side"]
    goal = side * side - 1
    two_moves = [goal - 2, goal - side - 1, goal - 2 * side]
    for dt, mode in ((np.float32, "iter"), (np.float64, "iter"), (np.float64, "vec")):  # the pairs the device test runs
        good = 0
        for run in cases.model_runs("grid-small", RUNS, dt, mode).values():
            history, _ = run.run(steps)
            ev = run.rt.events
            good += bool((np.asarray(history) > 0).any() and ev["propagate_some"] and ev["all_pops_used"]
                         and run.q[two_moves].any())
        print(f"grid-small {np.dtype(dt).name} {mode}: {good} of {len(RUNS)} runs sweep the goal's reward two moves back")
        assert 2 * good >= len(RUNS)


def test_a_tictactoe_call_ends_with_entries_queued_only_with_one_pop_per_step():
    for name, dt, mode, want in (("tictactoe", np.float64, "iter", False), ("tictactoe-n1", np.float32, "vec", True)):
        runs = cases.model_runs(name, RUNS, dt, mode)
        for run in runs.values():
            run.run(cases._case(name)[4])
        queued = [r for r, run in runs.items() if max(run.rt.cells) >= 0]
        print(f"{name}: runs that end with a non-empty queue {queued}")
        assert bool(queued) == want


@pytest.mark.parametrize(("dt", "mode"), cases.THETA_EQUAL)
def test_the_equal_threshold_case_meets_the_comparison_at_all_three_sites(dt, mode):
    thetas, done = cases.equal_threshold_runs(dt, mode)
    at = {site: sum(bool(run.rt.events[f"threshold_equal_{site}"]) for run, _, _ in done.values())
          for site in ("step", "plan", "propagate")}
    every = sum(any(run.rt.events[f"threshold_equal_{site}"] for site in at) for run, _, _ in done.values())
    print(f"{np.dtype(dt).name} {mode}: P == theta in {every} of {len(done)} runs; runs per site {at}")
    assert len(done) == cases.M_ODD == every and all(0 < t < np.inf for t in thetas)
    assert at["propagate"] >= (cases.M_ODD + 1) // 2 and at["step"] >= 1 and at["plan"] >= 1


@pytest.mark.parametrize(("A", "dt", "mode"), cases.NAN_UPLOAD)
def test_the_nan_upload_case_turns_the_held_row_nan_in_compared_runs(A, dt, mode):
    """No other sweep case does: over the special-table cases the model never stores the first NaN of the held row by a
    planning update (``held_row_turns_nan`` is 0 there), and a kernel that keeps its old NaN flag passes them."""
    tables, queue, out = cases.nan_upload_case(A, dt, mode)
    done = [r for r, (_, _, after) in out.items() if after is not None]
    turned = [r for r in done if out[r][0].rt.events["held_row_turns_nan"]]
    print(f"A={A} {np.dtype(dt).name} {mode}: {len(done)} of {cases.M_ODD} runs complete, {len(turned)} of them turn the held row NaN; "
          f"{int((queue['cells'] >= 0).any(axis=1).sum())} queues uploaded with an entry")
    assert len(turned) >= 5 and all(np.isnan(tables[r, r % 4, 0]) for r in range(cases.M_ODD))
    assert np.isinf(queue["priorities"][queue["cells"] >= 0]).all() and not queue["priorities"][queue["cells"] < 0].any()
    special, _ = _events(cases.special_runs(*cases.SPECIAL[0], RUNS)[0], 100)
    assert not special["held_row_turns_nan"]


def test_the_cut_call_has_three_launches_logged_and_two_unlogged():
    """``launch_len`` of the library (csrc/qe_population.hip), restated: the conditions on the shape of the cut call."""
    M, K, n = cases.CUT["M"], cases.CUT["K"], cases.CUT["n"]
    unlogged = 2**25 // M // (1 + n)
    logged = min(unlogged, 2**23 // M)
    assert (unlogged, logged) == (279, 209)
    assert -(-K // logged) == 3 and -(-K // unlogged) == 2 and -(-(K // 2) // logged) == 2
    assert K // 2 % logged and K // 2 % unlogged and (K // 2) not in (logged, 2 * logged, unlogged)


def test_the_thresholds_cycle_and_every_one_is_met():
    thetas = cases._thetas(cases.M_ODD)
    assert [thetas[r] for r in RUNS][:3] == [0.0, 1e-4, 1e-2] and set(thetas) == {0.0, 1e-4, 1e-2}
