"""CPU: the inputs of the wide-row tests (tests/wide_row_cases.py) test something -- asserted on the NumPy oracle alone.

tests/test_gpu_wide_rows.py compares the product with the oracle on these cases bit for bit; a comparison on inputs whose
picks never tie, never land in the last lane or never share a row would pass with a wrong lane mask, scan guard or chunk
count.  Every condition below is an assertion on what the oracle does with the inputs, never on the product."""

import numpy as np
import pytest

import wide_row_cases as W


# ------------------------------------------------------------------------------- unfused selection
def _greedy_agents(A):
    """(case, agent, action, candidate set) of every greedy pick of the width's non-raising cases."""
    for k, c in enumerate(W.select_cases(A)):
        status, actions = W.run_select_oracle(A, k)
        if status != "ok":
            continue
        an = W.select_analysis(c)
        for i, cand in enumerate(an["candidates"]):
            if cand is not None:
                yield c, i, int(actions[i]), cand


@pytest.mark.parametrize("A", W.WIDTHS)
def test_every_select_case_declares_whether_it_raises(A):
    cases = W.select_cases(A)
    raised = 0
    for k, c in enumerate(cases):
        status, actions = W.run_select_oracle(A, k)
        assert (status == "IndexError") == W.select_analysis(c)["raises"], c
        raised += status == "IndexError"
        if status == "ok":
            assert actions.shape == (c["n"],) and actions.max() < A and actions.min() >= -1
    assert 1 <= raised <= len(cases) // 3  # the IndexError is met, and most cases compare actions


@pytest.mark.parametrize("A", W.WIDTHS)
def test_select_cases_rotate_every_axis_over_every_width(A):
    cases = W.select_cases(A)
    assert {c["entry"] for c in cases} == set(W.ENTRIES)
    for entry in W.ENTRIES:
        assert {c["dt"] for c in cases if c["entry"] == entry} == set(W.DTYPES), entry
    assert {c["mask"] is None for c in cases} == {True, False}
    assert any(c["det"] for c in cases) and any(not c["det"] for c in cases)
    assert any(c["offset"] for c in cases)
    nan_rows = empty = 0
    for c in cases:
        _q, states, masks = W.select_inputs(c)
        nan_rows += int(np.isin(states, (W.ROW_ONE_NAN, W.ROW_ALL_NAN)).sum())
        empty += 0 if masks is None else int((masks.sum(axis=1) == 0).sum())
    assert nan_rows > 0 and empty > 0
    # the list variants' -1 and the NumPy variants' pick over all columns are both met on an empty mask
    assert any(c["mask"] == "half+empty" and not W.numpy_variant(c["entry"], c["n"], c["det"], True, A) for c in cases)
    assert any(c["mask"] == "half+empty" and W.numpy_variant(c["entry"], c["n"], c["det"], True, A) for c in cases)


def test_select_axes_are_all_used_somewhere():
    cases = [c for A in W.WIDTHS for c in W.select_cases(A)]
    assert {c["eps"] for c in cases} == set(W.EPS)
    assert {c["n"] for c in cases if c["entry"] != "single"} >= set(W.AGENTS)
    assert {c["step"] for c in cases} == set(W.STEP_COUNTERS)
    assert {c["mask"] for c in cases} == set(W.MASK_KINDS) | {None}
    for group in (W.MID, W.LARGE):  # each mask kind, each batch size at both kernel families
        sub = [c for c in cases if c["A"] in group]
        assert {c["mask"] for c in sub} == set(W.MASK_KINDS) | {None}
        assert {c["n"] for c in sub if c["entry"] != "single"} >= set(W.AGENTS)


@pytest.mark.parametrize("A", W.WIDTHS)
def test_greedy_picks_are_where_the_oracle_says_and_a_quarter_come_from_ties(A):
    picks = list(_greedy_agents(A))
    assert len(picks) >= 30
    for c, i, act, cand in picks:
        assert (act in cand) if len(cand) else act == -1, (c, i)
    assert sum(len(cand) >= 2 for *_, cand in picks) * 4 >= len(picks)


@pytest.mark.parametrize("A", W.MID)
def test_mid_width_picks_reach_the_last_lane_and_the_last_column(A):
    acts = [act for _c, _i, act, _cand in _greedy_agents(A)]
    assert any(act >= W.last_lane_start(A) for act in acts)
    assert any(act == A - 1 for act in acts)
    assert W.lanes_per_row(A) == (32 if A <= 128 else 64)


@pytest.mark.parametrize("A", W.LARGE)
def test_large_width_picks_fall_in_the_first_a_later_and_the_last_sweep(A):
    picks = [(act, cand) for _c, _i, act, cand in _greedy_agents(A) if act >= 0]
    last = (A - 1) // 64
    assert any(act // 64 == 0 for act, _ in picks)
    assert any(act // 64 == last for act, _ in picks)
    assert any(act // 64 > cand[0] // 64 for act, cand in picks)  # the ballot walk carries k across sweeps
    assert any(0 < act // 64 < last and act // 64 > cand[0] // 64 for act, cand in picks)  # ... and stops in a middle one


def test_the_table_builder_makes_the_rows_it_names():
    for A in W.WIDTHS:
        q = W.wide_table(A, "f8")
        assert np.flatnonzero(q[W.ROW_MAX_LAST] == q[W.ROW_MAX_LAST].max()).tolist() == [A - 1]
        assert np.flatnonzero(q[W.ROW_TIE_ENDS] == q[W.ROW_TIE_ENDS].max()).tolist() == [0, A - 1]
        per_sweep = np.bincount(np.flatnonzero(q[W.ROW_ONE_PER_SWEEP] == 2) // 64, minlength=(A + 63) // 64)
        assert (per_sweep == 1).all()
        assert (q[W.ROW_NEG_INF] == -np.inf).all() and np.isnan(q[W.ROW_ALL_NAN]).all()
        assert np.flatnonzero(np.isnan(q[W.ROW_ONE_NAN])).tolist() == [W.nan_col(A)]
        assert np.isfinite(q[list(W.FINITE_ROWS)]).all()
        assert np.array_equal(W.wide_table(A, "f4").astype("f8"), q, equal_nan=True)  # exact in both dtypes
        assert W.table_fingerprint(q) == W.table_fingerprint(W.wide_table(A, "f8"))


# ------------------------------------------------------------------------------- unfused learning
@pytest.mark.parametrize("A", W.WIDTHS)
def test_learn_cases_change_cells_and_leave_nan_exactly_where_declared(A):
    cases = W.learn_cases(A)
    new_nan = {"learn": 0, "learn_vec": 0}
    for k, c in enumerate(cases):
        q0, (s, a, _r, s2, term, masks) = W.learn_inputs(c)
        q = W.run_learn_oracle(A, k)
        assert not np.array_equal(q, q0, equal_nan=True), c
        declared = W.declared_nan_cells(c)
        assert np.array_equal(np.isnan(q), declared), c
        new_nan[c["fn"]] += int((declared & ~np.isnan(q0)).sum())
        assert len(set(np.unique(s).tolist())) <= 4 and np.isfinite(q0[np.unique(s)]).all()
        untouched = np.ones_like(declared)
        untouched[s, a] = False
        assert np.array_equal(q[untouched], q0[untouched], equal_nan=True)
        if c["kind"] == "nan_off":  # the NaN sits in a masked-out column of a live next row: it must not reach a target
            live = np.flatnonzero((s2 == W.ROW_ONE_NAN) & ~term)
            assert live.size and not masks[live, W.nan_col(A)].any()
            by_terminal = np.zeros_like(declared)  # (learn_vec: inf * 0 of a terminated transition may share the cell)
            by_terminal[s[term], a[term]] = c["fn"] == "learn_vec"
            assert not (declared & ~np.isnan(q0) & ~by_terminal).any()
        if c["kind"] == "nan_valid":
            live = np.flatnonzero((s2 == W.ROW_ONE_NAN) & ~term)
            assert live.size and declared[s[live], a[live]].all()
        if c["kind"] == "last":
            assert (masks.sum(axis=1) == 1).all() and masks[:, A - 1].all()
        if c["fn"] == "learn_vec" and c["n"] >= 31:  # np.add.at order matters only where a cell repeats
            assert np.bincount(s.astype(np.int64) * A + a).max() >= 3, c
        if c["n"] >= 31:  # terminated transitions onto the infinite and the NaN rows
            assert set(s2[term].tolist()) >= {W.ROW_NEG_INF, W.ROW_ALL_NAN}, c
    assert new_nan["learn"] > 0 and new_nan["learn_vec"] > new_nan["learn"]  # (learn_vec: inf * 0 on top)
    for fn in ("learn", "learn_vec"):
        for masked in (False, True):
            sub = [c for c in cases if c["fn"] == fn and c["masked"] == masked]
            assert {c["dt"] for c in sub} == set(W.DTYPES)
            assert [c["n"] for c in sub] == list(W.learn_batch_sizes(A))
    assert {c["kind"] for c in cases} == {"plain", "nan_valid", "nan_off", "last"}


def test_learn_batch_sizes_straddle_the_ordered_paths_mode_switch():
    assert W.learn_batch_sizes(65) == (1, 63, 64, 65, 300) and W.learn_batch_sizes(128) == (1, 63, 64, 65, 300)
    assert W.learn_batch_sizes(129) == (1, 31, 32, 33, 300) and W.learn_batch_sizes(256) == (1, 31, 32, 33, 300)
    assert W.learn_batch_sizes(257) == (1, 65, 300)
    rewards = W.learn_inputs(W.learn_cases(100 if 100 in W.WIDTHS else 96)[4])[1][2]
    assert rewards.dtype == np.float32 and (rewards.astype(np.float64) * 2.0**20 % 1 != 0).any()  # not short binary fractions


# ------------------------------------------------------------------------------- closed loop
CLEAN = [name for name, case in W.ROLLOUTS.items() if not case[4]]


@pytest.mark.parametrize("name", CLEAN)
def test_rollout_cases_use_the_wide_columns_end_episodes_and_contest_rows(name):
    spec, chunks, _dt, _mode, _ = W.ROLLOUTS[name]
    A = spec[3]
    want = W.run_rollout_oracle(name)
    assert len(want) == len(chunks) and not want[-1]["raised"]
    facts = W.rollout_facts(name)
    assert facts["episodes"] >= 1
    if A == 65:
        assert facts["col64"]  # the only column beyond the first 64
    else:
        assert facts["share_ge64"] >= 0.25
    # more than 2 * ngrp transitions of one step touch a row another agent writes: the ordered path's second mode
    assert facts["most_involved"] >= 2 * W.groups_per_block(A) + 1
    q0 = W.rollout_q0(name)
    assert np.isfinite(q0).all() and not np.array_equal(want[-1]["q"], q0)


def test_rollout_cases_cover_the_widths_dtypes_modes_and_agent_counts():
    hashed = [c for c in W.ROLLOUTS.values() if c[0][0] == "hash" and not c[4]]
    assert {c[0][3] for c in hashed} == {65, 100, 129, 255, 256}
    for A in (65, 100, 129, 255, 256):
        sub = [c for c in hashed if c[0][3] == A]
        assert {c[2] for c in sub} == set(W.DTYPES) and {c[0][4] for c in sub} == {True, False}
    assert {c[3] for c in hashed} == {"iter", "vec"}
    assert {c[0][1] for c in hashed} == {40, 150, 600, 2100}
    assert all(30 <= c[0][2] <= 500 for c in W.ROLLOUTS.values())
    tables = [c for c in W.ROLLOUTS.values() if c[0][0] == "table"]
    assert sorted(c[0][3] for c in tables) == [72, 130]
    for c in tables:  # masked, and the last state's mask words end the allocation
        assert W.table_mdp(*c[0][2:]).masks is not None


def test_nan_start_tables_do_what_their_names_say():
    # fewer than 100 unmasked agents: the list variants step over NaN, no error, and the NaN is met
    want = W.run_rollout_oracle("nan_a100_n60_list")
    assert [w["raised"] for w in want] == [False, False, False]
    assert np.isnan(W.rollout_q0("nan_a100_n60_list")).sum() == 60 and (want[-1]["actions"] >= 0).all()
    q0 = W.rollout_q0("nan_a100_n60_list")
    obs_rows = np.unique(want[-1]["final_obs"])
    assert np.isnan(want[-1]["q"]).sum() >= 60 and np.isnan(q0).any(axis=1).sum() >= 20 and obs_rows.size > 1
    assert not np.array_equal(np.isnan(want[-1]["q"]), np.isnan(q0))  # a NaN row was a next row: the NaN spread
    # 150 unmasked agents on 100 actions: choose_actions_vec, IndexError -- in a later call than the first
    want = W.run_rollout_oracle("nan_a100_n150_numpy")
    assert [w["raised"] for w in want] == [False, False, False, True]
