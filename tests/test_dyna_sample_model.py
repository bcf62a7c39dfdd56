"""CPU: the NumPy model of Dyna-Q over a sample model (tests/dyna_sample_model.py).

* Where every cell has one (reward, flag, successor) signature -- the hash environment, the grid -- the model equals
  ``DynaRun`` at the same ``n``: every ``t`` falls in slot 0 and the outcome draws come from a stream of their own.
* The inputs tests/test_gpu_dyna_sample.py compares on really reach every branch of the learn step and of the slot
  walk: the model counts them.
"""
import numpy as np
import pytest

from dyna_model import DynaRun
from dyna_sample_model import COUNT_MAX, DynaSampleRun, DynaSampleRuntime, table_case
from test_gpu_population import _schedules
from test_gpu_td_rules import _model_env

M_ODD = 67
RUNS = range(0, M_ODD, 6)  # 12 of the 67 runs the device test compares


def _runs(kind, p, K, n, steps, runs=RUNS, seed=11, dt=np.float32, mode="iter"):
    eps_s, lr_s, gamma = _schedules(M_ODD)
    out = {}
    for r in runs:
        run = DynaSampleRun(_model_env(kind, r, p), gamma[r], eps_s[r], lr_s[r], n=n, K=K, seed=seed, dtype=dt, mode=mode, agent_id=r)
        out[r] = (run, *run.run(steps))
    return out


def _events(runs):
    return {key: sum(int(run.events[key]) for run, *_ in runs.values()) for key in next(iter(runs.values()))[0].events}


@pytest.mark.parametrize(("kind", "p", "dt", "mode"), [
    ("hash", {"S": 100, "A": 8, "seed": 1, "masked": True}, np.float32, "iter"),
    ("hash", {"S": 100, "A": 8, "seed": 1, "masked": True}, np.float64, "vec"),
    ("grid", {"side": 6, "seed": 2}, np.float32, "vec"), ("grid", {"side": 6, "seed": 2}, np.float64, "iter")])
def test_one_signature_per_cell_equals_dyna_q(kind, p, dt, mode):
    eps_s, lr_s, gamma = _schedules(M_ODD)
    n, steps = 4, 150
    got = _runs(kind, p, 4, n, steps, dt=dt, mode=mode)
    ev = _events(got)
    assert ev["second_slots"] == ev["high_picks"] == ev["evictions"] == 0 and ev["matches"] > 0 and ev["picks"] == len(got) * steps * n
    for r, (run, history, at) in got.items():
        ref = DynaRun(_model_env(kind, r, p), gamma[r], eps_s[r], lr_s[r], n=n, seed=11, dtype=dt, mode=mode, agent_id=r)
        want_history, want_at = ref.run(steps)
        assert np.array_equal(run.q, ref.q, equal_nan=True), r
        assert np.array_equal(history, want_history) and np.array_equal(at, want_at), r
        nxt, rew, term, cnt, visited, count = run.planning_model
        wn, wr, wt, wv, wc = ref.planning_model
        assert np.array_equal(nxt[..., 0], wn) and np.array_equal(rew[..., 0].view(np.uint32), wr.view(np.uint32)), r
        assert np.array_equal(term[..., 0], wt) and np.array_equal(visited, wv) and count == wc, r
        assert (nxt[..., 1:] == -1).all() and not cnt[..., 1:].any() and cnt[..., 0].sum() == steps, r


def test_the_compared_inputs_reach_every_branch():
    S, A, p3, _, _ = table_case("three")
    two = _events(_runs("table", p3, 2, 4, 150))
    assert two["second_slots"] > 0 and two["high_picks"] > 0 and two["evictions"] > two["tie_evictions"] > 0
    assert two["terminated_rematches"] > 0 and two["picks"] == len(RUNS) * 150 * 4
    for K in (4, 8):  # three outcomes per cell: nothing is evicted
        ev = _events(_runs("table", p3, K, 4, 150))
        assert ev["evictions"] == 0 and ev["second_slots"] > 0 and ev["high_picks"] > 0
    _, _, p8, _, _ = table_case("eight")
    four = _events(_runs("table", p8, 4, 4, 150))
    assert four["evictions"] > four["tie_evictions"] > 0 and four["high_picks"] > 0
    eight = _events(_runs("table", p8, 8, 4, 150))
    assert eight["evictions"] == 0 and eight["full_cells"] > 0, "no cell filled all eight slots"
    bandit = _events(_runs("bandit", {"episode_len": 50}, 2, 3, 140))
    assert bandit["second_slots"] > 0 and bandit["high_picks"] > 0 and bandit["evictions"] == 0
    ttt = _events(_runs("tictactoe", {"seed": 5}, 2, 4, 60, runs=range(3)))
    assert ttt["evictions"] > 0 and ttt["tie_evictions"] > 0


def _bare(K):
    rt = DynaSampleRuntime.__new__(DynaSampleRuntime)
    rt.K = K
    rt.slots, rt.visited = {}, []
    rt.events = dict.fromkeys(("second_slots", "high_picks", "picks", "evictions", "tie_evictions", "terminated_rematches", "matches",
                               "full_cells", "saturated_matches", "saturated_inserts", "top_picks"), 0)
    return rt


def test_the_learn_step_by_hand():
    rt = _bare(3)
    rt.learn(7, 2, 1.0, False)
    rt.learn(7, 2, 1.0, False)
    rt.learn(7, 3, 1.0, False)          # another successor: a slot of its own
    rt.learn(7, 5, -0.0, True)
    rt.learn(7, 9, -0.0, True)          # a terminated outcome is one outcome whatever the reset returned; the newest is kept
    assert rt.slots[7] == [[2, np.float32(1), False, 2], [3, np.float32(1), False, 1], [9, np.float32(-0.0), True, 2]]
    rt.learn(7, 9, 0.0, True)           # 0.0 is not -0.0: no match, no free slot, slot 1 is the rarest
    assert rt.slots[7][1][:1] + rt.slots[7][1][2:] == [9, True, 1] and np.signbit(rt.slots[7][2][1]) and not np.signbit(rt.slots[7][1][1])
    nan = np.uint32(0x7FC00001).view(np.float32)
    rt.learn(7, 4, nan, False)          # slots count 2, 1, 2: slot 1 goes again
    rt.learn(7, 4, nan, False)          # a NaN matches its own bit pattern
    assert rt.slots[7][1][0] == 4 and rt.slots[7][1][3] == 2
    rt.learn(7, 0, 3.0, False)          # all counts 2: the lowest index goes
    assert rt.slots[7][0] == [0, np.float32(3), False, 1] and rt.events["tie_evictions"] == 1 and rt.events["evictions"] == 3
    # saturation: the total never passes 2^32 - 1
    rt.slots[8] = [[1, np.float32(0), False, COUNT_MAX - 2], [2, np.float32(0), False, 1]]
    rt.learn(8, 2, 0.0, False)
    assert [x[3] for x in rt.slots[8]] == [COUNT_MAX - 2, 2]
    rt.learn(8, 2, 0.0, False)
    rt.learn(8, 1, 0.0, False)
    assert [x[3] for x in rt.slots[8]] == [COUNT_MAX - 2, 2] and rt.events["saturated_matches"] == 2
    # ... nor does a new outcome: at 2^32 - 1 no slot is opened, the rarest occupied one goes
    rt.slots[8][0][3] += 1
    rt.learn(8, 3, 0.0, False)
    assert rt.slots[8] == [[1, np.float32(0), False, COUNT_MAX - 1], [3, np.float32(0), False, 1]] and rt.events["saturated_inserts"] == 1
    rt.slots[8] = [[1, np.float32(0), False, COUNT_MAX - 2], [2, np.float32(0), False, 2]]
    # the slot walk at the top of the range
    assert rt.choose(8, 0xFFFFFFFF)[0] == 2 and rt.choose(8, 0)[0] == 1 and rt.choose(8, 0xFFFFFFFD)[0] == 1
