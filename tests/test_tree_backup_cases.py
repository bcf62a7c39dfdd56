"""CPU: the case list of tests/test_gpu_tree_backup.py is built without a device, and the model runs of every training
case together perform every kind of update the case's structure allows (tests/tree_backup_cases.py says which and why).
"""
import numpy as np
import pytest

import tree_backup_cases as tc
from tree_backup_model import KINDS


def test_the_case_list_covers_what_the_gpu_tests_mean_to_cover():
    cases = tc.CASES
    assert len({c["id"] for c in cases}) == len(cases)
    hashed = [c for c in cases if c["kind"] == "hash"]
    for A in tc.WIDTHS:
        for masked in (False, True):
            for dt in ("float32", "float64"):
                for mode in ("iter", "vec"):
                    assert [c for c in hashed if (c["A"], c["masked"], c["dt"], c["mode"]) == (A, masked, dt, mode)], (A, masked, dt, mode)
    assert {c["nv"] for c in hashed} == {1, 2, 4, 8, 16}
    for n in tc.HORIZONS:
        assert {(c["dt"], c["mode"]) for c in hashed if c["n"] == n} >= {("float32", "iter"), ("float64", "vec")}, n
        assert {c["masked"] for c in hashed if c["n"] == n} == {False, True}, n
    assert [c for c in hashed if (c["A"], c["masked"], c["dt"], c["n"]) == (64, True, "float64", 16)]
    assert {c["kind"] for c in cases} == {"hash", "grid", "bandit", "bandit_mc", "tictactoe", "table"}
    for c in cases:
        assert c["M"] == 67 and 2 <= c["n"] <= 16
        if c["kind"] == "bandit":
            assert c["p"]["episode_len"] > c["n"]
        if c["kind"] == "bandit_mc":
            assert c["p"]["episode_len"] < c["n"]
        assert tc.required(c) <= set(KINDS) and {"flush_cut", "flush_no_cut", "tie_pass"} <= tc.required(c)


@pytest.mark.parametrize("case_id", [c["id"] for c in tc.CASES])
def test_every_case_performs_every_kind_of_update(case_id):
    case = tc.BY_ID[case_id]
    got = tc.performed(case_id)
    missing = sorted(kind for kind in tc.required(case) if not got[kind])
    assert not missing, (missing, got)
    runs = tc.model(case_id)
    assert len(runs) == case["M"]
    assert max(run.window[0] for run, _, _ in runs.values()) == (0 if case["kind"] == "bandit_mc" else case["n"] - 1)


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [
    (8, False, np.float32, "iter"),
    (8, True, np.float64, "vec"),
    (16, True, np.float32, "vec"),
])
def test_the_special_value_case_meets_its_conditions_in_the_model_alone(A, masked, dt, mode):
    raised, special_kept = tc.nan_case_model(A, masked, dt, mode)
    assert raised, "no run met a row without a selectable action"
    assert special_kept, "no run finished with a NaN or an infinity in its table"
    assert len(raised) < tc.NAN_CASE["M"]
