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
])
def test_a_gpu_case_reaches_the_branch(reached, event, name):
    seen, _ = reached[name]
    assert seen[event] >= 1, (name, dict(seen))


def test_a_terminated_flag_turns_on_and_off_for_one_cell(reached):
    for name in ("bandit", "frozen"):
        seen, both = reached[name]
        assert both >= 1 and seen["flag_on"] and seen["flag_off"], (name, dict(seen))


def test_the_thresholds_cycle_and_every_one_is_met():
    thetas = cases._thetas(cases.M_ODD)
    assert [thetas[r] for r in RUNS][:3] == [0.0, 1e-4, 1e-2] and set(thetas) == {0.0, 1e-4, 1e-2}
