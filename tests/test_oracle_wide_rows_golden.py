"""CPU: the oracle against the REAL reference on rows of more than 64 actions (tests/golden/wide_rows.npz, written by
tests/golden/make_wide_rows.py from the reference's own ``OptimalQLearningBase``): every selection case and every learn
case of ``wide_row_cases.GOLDEN_WIDTHS``.  Bit for bit; what the reference raised is part of the record.  The tables are
rebuilt from the case and must have the fingerprint the generator saw."""

import numpy as np
import pytest

import wide_row_cases as W
from helpers import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "wide_rows.npz")


def golden_select(g, A, k):
    """("ok", actions) / ("IndexError", None) as the reference did it, or None where the fixture has no record."""
    status = int(g[f"s{A}_{k}_status"])
    assert status in (0, 1, 2), str(g[f"s{A}_{k}_exception"])  # (the reference raised nothing else on these cases)
    if status == 2:
        return None
    return ("ok", g[f"s{A}_{k}_actions"].astype(np.int32)) if status == 0 else ("IndexError", None)


def golden_learn(g, A, k, q0):
    q = q0.copy()
    q.ravel()[g[f"l{A}_{k}_idx"]] = g[f"l{A}_{k}_val"]
    return q


@pytest.mark.parametrize("A", W.GOLDEN_WIDTHS)
def test_tables_have_the_fingerprint_the_generator_saw(golden, A):
    for dt in W.DTYPES:
        assert W.table_fingerprint(W.wide_table(A, dt)) == int(golden[f"fp_{A}_{dt}"])


@pytest.mark.parametrize("A", W.GOLDEN_WIDTHS)
def test_oracle_selection_equals_the_reference(golden, A):
    seen = {"ok": 0, "IndexError": 0, None: 0}
    for k, c in enumerate(W.select_cases(A)):
        want = golden_select(golden, A, k)
        assert (want is None) == W.shim_cannot_observe(c), c
        if want is None:
            seen[None] += 1
            continue
        status, actions = W.run_select_oracle(A, k)
        assert status == want[0], c
        if status == "ok":
            assert np.array_equal(actions, want[1]), c
        seen[status] += 1
    assert seen["ok"] >= 6 and seen["IndexError"] >= 1 and seen[None] <= len(W.select_cases(A)) // 4


def test_the_golden_subset_holds_what_it_is_meant_to(golden):
    recorded = [c for A in W.GOLDEN_WIDTHS for k, c in enumerate(W.select_cases(A)) if golden_select(golden, A, k) is not None]
    for group in (W.MID, W.LARGE):
        sub = [c for c in recorded if c["A"] in group]
        assert {c["entry"] for c in sub} == set(W.ENTRIES)
        assert any(c["det"] for c in sub) and any(c["mask"] == "half+empty" for c in sub)
        assert any(c["rows"] == "all" for c in sub)  # the NaN rows
    assert {W.lanes_per_row(A) for A in W.GOLDEN_WIDTHS if A <= 256} == {32, 64}


@pytest.mark.parametrize("A", W.GOLDEN_WIDTHS)
def test_oracle_learning_equals_the_reference(golden, A):
    for k, c in enumerate(W.learn_cases(A)):
        q0, _ = W.learn_inputs(c)
        want = golden_learn(golden, A, k, q0)
        got = W.run_learn_oracle(A, k)
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), c
        assert np.array_equal(np.isnan(want), W.declared_nan_cells(c)), c  # the reference leaves the NaN where declared
