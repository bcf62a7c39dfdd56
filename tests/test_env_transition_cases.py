"""CPU: the environment transition cases (tests/env_cases.py) -- the conditions on the inputs that the GPU tests rely on,
asserted from the oracle's draws alone, and the oracle's TicTacToe pinned to the reference's own environment over the
whole game through the golden table (tests/golden/ttt_transitions.npz, tests/golden/make_ttt_transitions.py)."""

import numpy as np
import pytest

import env_cases as ec
from oracle.envs import TicTacToeVecEnv, ttt_encode


@pytest.fixture(scope="module")
def ttt_steps():
    return [ec.ttt_case(step) for step in ec.TTT_STEPS]


# ------------------------------------------------------------------------------- the golden table itself
def test_golden_table_has_the_counted_rows():
    t = ec.ttt_table()
    c = t.cols
    got = {"positions": len(t.pos_row), "pairs": len(t.pair_row), "agent_ends": int((c["reply"] == 9).sum()),
           "reply_rows": int((c["reply"] < 9).sum()), "rows": len(c["reply"])}
    assert got == ec.TTT_COUNTS
    # positions: the agent's turn by the mark counts, nothing occupied twice, board not full
    pop = lambda m: np.array([bin(int(x)).count("1") for x in m])  # noqa: E731
    assert not (c["m1"] & c["m2"]).any() and ((c["m1"] | c["m2"]) != 0x1FF).all()
    assert np.array_equal(pop(c["m1"]), pop(c["m2"]) + (c["mark"] == 2))
    # actions and replies are empty cells, the reply differs from the action, every reply of a pair occurs once
    occupied = c["m1"] | c["m2"]
    assert not ((occupied >> c["action"]) & 1).any()
    r = c["reply"] < 9
    assert not (((occupied | (1 << c["action"])) >> c["reply"])[r] & 1).any()
    assert np.array_equal(np.sort(t.row_of[t.row_of >= 0]), np.arange(len(c["reply"])))
    assert np.array_equal((t.row_of[:, :9] >= 0).sum(axis=1), np.where(t.row_of[:, 9] >= 0, 0, t.n_empty))
    assert set(np.unique(c["reward"])) == {-1, 0, 1} and ((c["reward"] != 0) <= (c["terminated"] == 1)).all()


def test_oracle_encoder_equals_the_reference_ids_on_every_position():
    t = ec.ttt_table()
    c = t.cols
    pos = t.pos_row
    want = c["obs"][pos]
    assert len(np.unique(want[c["mark"][pos] == 1])) == (c["mark"][pos] == 1).sum()  # ids name boards
    got = np.array([ttt_encode(int(a), int(b)) for a, b in zip(c["m1"][pos], c["m2"][pos])])
    assert np.array_equal(got, want)
    assert np.array_equal(ec.ttt_encode_vec(c["m1"][pos], c["m2"][pos]), want)
    assert np.array_equal(ec.ttt_encode_vec(c["m1"], c["m2"]), c["obs"])


def test_oracle_action_masks_are_the_empty_cells_of_every_id():
    ids = np.arange(19683)
    digits = (ids[:, None] // 3 ** np.arange(8, -1, -1)) % 3
    assert np.array_equal(TicTacToeVecEnv(1).action_masks(ids), (digits == 0).astype(np.int8))


# ------------------------------------------------------------------------------- coverage of the committed parameters
def test_the_two_steps_hit_every_reply_row_and_every_opening(ttt_steps):
    t = ec.ttt_table()
    assert [c.n for c in ttt_steps] == [517344, 517344]
    rows = np.unique(np.concatenate([c.info["row"] for c in ttt_steps]))
    assert np.array_equal(rows, np.arange(ec.TTT_COUNTS["rows"]))  # all 43 644 replies (and the 2 862 agent-ended pairs)
    assert ((t.cols["reply"] < 9).sum(), (t.cols["reply"] == 9).sum()) == (43644, 2862)
    openings = np.unique(np.concatenate([c.info["opening"][c.terminated] for c in ttt_steps]))
    assert np.array_equal(openings, np.arange(10))  # the agent starts, or the machine opens on each of the 9 cells


def test_oracle_step_equals_the_reference_table_on_every_row(ttt_steps):
    """One agent per golden row -- the first replica that realises it, at step 0 if one does, else at 2^32 + 5 -- through
    ``TicTacToeVecEnv.step`` with its state set directly: board and marks (``env_aux``), observation, masks, reward and
    ``terminated`` must be what the reference's table and the draw protocol give."""
    t = ec.ttt_table()
    c = t.cols
    done = np.zeros(ec.TTT_COUNTS["rows"], dtype=bool)
    agents = 0
    for case in ttt_steps:
        rows, first = np.unique(case.info["row"], return_index=True)
        first = first[~done[rows]]
        done[case.info["row"][first]] = True
        row = case.info["row"][first]
        env = TicTacToeVecEnv(len(first), seed=ec.TTT_SEED)
        env.agent_ids = case.info["ids"][first]
        env.m1[:], env.m2[:], env.agent_mark[:] = c["m1"][row], c["m2"][row], c["mark"][row]
        env.step_index = case.step
        obs, reward, terminated, truncated, _ = env.step(c["action"][row])
        agents += len(first)
        assert np.array_equal(reward, c["reward"][row].astype(np.float32))
        assert np.array_equal(terminated, c["terminated"][row] == 1) and not truncated.any()
        go_on = ~terminated  # the reference leaves the final board, the vector environment has reopened already
        assert np.array_equal(env.m1[go_on], c["out_m1"][row][go_on]) and np.array_equal(env.m2[go_on], c["out_m2"][row][go_on])
        assert np.array_equal(env.agent_mark[go_on], c["mark"][row][go_on])
        assert np.array_equal(ec.env_aux(env), case.next_aux[first])
        assert np.array_equal(obs["observation"], case.next_obs[first])
        assert np.array_equal(obs["action_mask"].astype(bool), case.masks[first])
        assert np.array_equal(case.reward[first], reward) and np.array_equal(case.terminated[first], terminated)
    assert done.all() and agents == ec.TTT_COUNTS["rows"]


def test_reset_word_and_occupied_cell_cases_are_what_they_mean_to_be():
    t = ec.ttt_table()
    c = t.cols
    case = ec.ttt_occupied_cell_case()
    assert case.n == int(sum(bin(int(x)).count("1") for x in (c["m1"] | c["m2"])[t.pos_row]))
    m1, m2 = case.aux & 0x1FF, (case.aux >> 9) & 0x1FF
    assert (((m1 | m2) >> case.actions.astype(np.uint32)) & 1).all()
    mine = np.where((case.aux >> 18) & 1, m2, m1)
    assert ((mine >> case.actions.astype(np.uint32)) & 1).any() and (~(mine >> case.actions.astype(np.uint32)) & 1).any()
    # the vectorised builder and the per-agent oracle agree at the reset word too (one replica of every pair)
    fast = ec.ttt_case(ec.RESET_STEP, replicas=1)
    first = t.pair_row
    slow = ec.ttt_oracle_case(c["m1"][first], c["m2"][first], c["mark"][first], c["action"][first], ec.RESET_STEP)
    for name in ("obs", "aux", "actions", "next_obs", "next_aux", "reward", "terminated", "start_masks", "masks"):
        assert np.array_equal(getattr(fast, name), getattr(slow, name)), name
    assert fast.terminated.any() and not fast.terminated.all()


# ------------------------------------------------------------------------------- the other environments' builders
def test_hash_cases_meet_their_conditions():
    both = {13: [0, 0], 128: [0, 0]}
    wrapped = 0
    for S, A, masked in ec.HASH_SHAPES:
        for p in ec.HASH_P_TERM:
            case = ec.hash_case(S, A, masked, p)
            assert case.n == S * A and set(np.unique(case.aux)) <= {0, 1, 0xFFFFFFFF}
            if p == 0:
                assert not case.terminated.any()
            elif p == 256:
                assert case.terminated.all()
            else:
                both[p][0] += int(case.terminated.sum())
                both[p][1] += int((~case.terminated).sum())
                if S >= 20:  # (termination is a function of the successor: a shape needs more than a few states for both)
                    assert case.terminated.any() and not case.terminated.all()
            wrap = case.terminated & (case.aux == 0xFFFFFFFF)
            wrapped += int(wrap.sum())
            assert (case.next_aux[wrap] == 0).all()
            assert np.array_equal(case.next_aux, case.aux + case.terminated.astype(np.uint32))
            if S * A >= 3:
                assert len(np.unique(case.aux)) == 3
        if masked:
            # a state whose last column -- the highest bit read from the last mask word -- is valid, and one where it is not
            # (column 0 is forced valid, so with A <= 32 "no valid bit in the last word" cannot occur: the last column
            # stands for the word's far end)
            last = case.start_masks[:, A - 1]
            assert last.any() and not last.all()
            assert case.start_masks[:, 0].all()
    assert all(min(v) > 0 for v in both.values()) and wrapped > 0
    crossing = ec.agent_ids(ec.crossing_offset(257), 257)
    assert crossing[127] == 0xFFFFFFFF and crossing[128] == 0 and ec.agent_ids(ec.crossing_offset(1), 1)[0] == 0xFFFFFFFF


def test_grid_cases_meet_their_conditions():
    for side in ec.GRID_SIDES:
        holes = [ec.grid_case(side, seed).info["holes"] for seed in ec.GRID_SEEDS]
        assert ec.grid_case(side, 1).n == 4 * side * side
        if side >= 3:
            assert holes[0].any() and holes[1].any() and not np.array_equal(holes[0], holes[1])
        for h in holes:
            assert not h[0] and not h[-1]


def test_bandit_cases_meet_their_conditions():
    for length in ec.BANDIT_LENGTHS:
        case = ec.bandit_case(length)
        assert np.array_equal(np.unique(case.aux), np.arange(length)) and set(case.actions[case.aux == 0]) == {0, 1}
        assert np.array_equal(case.terminated, case.aux == length - 1) and np.array_equal(case.reward, case.actions)


@pytest.mark.parametrize("name", list(ec.TABLE_SHAPES))
def test_table_cases_draw_every_positive_slot_and_every_start_state(name):
    S, A, K, n_start, masked = ec.TABLE_SHAPES[name]
    for step in ec.TABLE_STEPS:
        case = ec.table_case(name, step)
        mdp = case.info["mdp"]
        assert mdp.thr.shape == (S, A, K) and len(mdp.start_state) == n_start and (mdp.masks is not None) == masked
        weights = mdp.outcome_weights()
        assert (weights % (1 << 29) == 0).all() and (mdp.start_weights() % (1 << 29) == 0).all()
        assert (mdp.start_weights() > 0).all()
        if K > 1:
            assert (weights == 0).any()  # zero-weight slots are part of the case
        # every slot has a reward of its own: the rewards seen are the slots drawn
        assert np.array_equal(np.isin(mdp.reward, case.reward), weights > 0)
        assert set(case.next_obs[case.terminated].tolist()) == set(mdp.start_state.tolist())
        assert case.terminated.any() and not case.terminated.all()
        if masked:
            assert case.start_masks.any(axis=1).all() and not case.start_masks.all()


def test_the_two_environment_curriculum_tells_the_environments_apart():
    stages = ec.two_env_curriculum("A")
    assert [s["env"] for s in stages] == ["A", "B", "A"] and [s["step_counter"] for s in stages] == [40, 80, 110]
    a, b = stages[0], stages[1]
    n = min(len(a["obs"]), len(b["obs"]))
    # what a stale mirror would hand out for A is B's state: it has to differ in every array the test compares
    assert not np.array_equal(a["obs"][:n], b["obs"][:n]) and not np.array_equal(a["aux"][:n], b["aux"][:n])
    assert not np.array_equal(a["acc"][:n], b["acc"][:n])
    assert all(len(s["history"]) > 0 for s in stages)
