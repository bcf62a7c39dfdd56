"""CPU: the NumPy model of the population's prioritized sweeping (tests/sweep_model.py), which the GPU parity tests of
``QLearningPopulation(planning_order="prioritized")`` compare against.

* With planning skipped, and with a threshold above every increment, the model is, bit for bit, ``TdRun("q_learning")``
  (tests/td_rules_model.py): this anchors its step order, draws, schedules and update arithmetic -- and ``_increment``,
  which must be the very amount ``_update`` adds -- to the merged model.  It still learns its model and its lists.
* The book's property (Sutton & Barto, section 8.4) on a deterministic corridor: the step that first earns the reward
  carries value back to every cell on the way, where uniform Dyna-Q with the same number of updates does not.
* The lists are the canonical ones while no cell changes its outcome; the queue obeys its definition on a hand-made case.
* Two model calls equal one call.
"""
import numpy as np
import pytest

from dist_classicrl_amd.environments.device_envs import encode_table_mdp
from dyna_model import DynaRun
from oracle.qlearn_oracle import OracleSchedule
from sweep_model import SweepRun, SweepRuntime, canonical_lists
from table_mdp_model import TableMDPVecEnv
from td_rules_model import TdRun
from test_dyna_model import _env, _schedules
from test_trace_model import _same_run, _same_table


# ---- 1. without planning the step is Q-learning's ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("env_kind", ["hash", "hash_masked", "bandit", "tictactoe", "table"])
@pytest.mark.parametrize("how", ["skip_planning", "threshold"])
def test_without_planning_the_model_is_the_merged_model(how, env_kind, dt, mode):
    K, offset, seed = 150, 5, 9
    theta = 1e300 if how == "threshold" else 0.0
    got = SweepRun(_env(env_kind, offset), 0.93, *_schedules(), n=4, K=8, theta=theta, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    got.rt.skip_planning = how == "skip_planning"
    want = TdRun(_env(env_kind, offset), "q_learning", 0.93, *_schedules(), seed=seed, dtype=dt, mode=mode, agent_id=offset)
    assert _same_run(got, want, K)
    assert got.q.any() and got.sweep_queue[0].max() == -1
    nxt, rew, term, visited, count = got.planning_model
    assert count == (nxt >= 0).sum() > 1
    head, link = got.predecessors
    assert (head >= 0).any() and ((link >= 0).sum() + (head >= 0).sum()) == ((nxt >= 0) & ~term).sum()
    # ... and with it, planning changes the table
    planned = SweepRun(_env(env_kind, offset), 0.93, *_schedules(), n=4, K=8, theta=0.0, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    planned.run(K)
    assert not _same_table(planned.q, want.q)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_increment_is_what_the_update_adds(dt, mode):
    run = SweepRun(_env("hash", 2), 0.93, *_schedules(), n=4, K=8, theta=0.0, seed=3, dtype=dt, mode=mode, agent_id=2)
    run.run(60)
    rt, q = run.rt, run.q
    for c in run.planning_model[3][:10]:
        s, a = divmod(int(c), q.shape[1])
        before = q[s, a]
        u = rt._increment(s, a, np.float32(0.25), q[3].max(), False, 0.3)
        assert u.dtype == (np.float64 if mode == "vec" else dt)
        rt._update(s, a, np.float32(0.25), q[3].max(), False, 0.3)
        assert q[s, a] == dt(np.float64(before) + np.float64(u)) if mode == "vec" else q[s, a] == before + u
        assert rt.last_priority == abs(float(u))


# ---- 2. the book's property on a corridor ----------------------------------------------------------------------------------------
L = 12
RIGHT, STAY = 0, 1


def _corridor():
    nxt = np.zeros((L, 2, 1), dtype=np.int64)
    nxt[:, RIGHT, 0] = np.minimum(np.arange(L) + 1, L - 1)
    nxt[:, STAY, 0] = np.arange(L)
    rew = np.zeros((L, 2, 1), dtype=np.float32)
    rew[L - 2, RIGHT, 0] = 1.0  # on entering the last state
    term = np.zeros((L, 2, 1), dtype=bool)
    term[L - 2, RIGHT, 0] = True
    term[L - 1] = True
    isd = np.zeros(L)
    isd[0] = 1.0
    return encode_table_mdp(np.ones((L, 2, 1)), nxt, rew, term, isd)


def _until_the_first_reward(run):
    moved_right = set()
    for _ in range(5000):
        s = 0 if run.states is None else run.obs
        before = run.rt.step_counter
        history, _ = run.run(1)
        assert run.rt.step_counter == before + 1
        if run.rt.last_action == RIGHT:
            moved_right.add(s)
        if len(history):
            assert history[0] == 1.0
            return moved_right
    pytest.fail("the run never reached the end of the corridor")


def test_the_first_reward_reaches_every_cell_on_the_way_and_uniform_planning_does_not():
    seed, eps, lr = 5, OracleSchedule("constant", 0.3), OracleSchedule("constant", 0.5)
    mdp = _corridor()
    sweep = SweepRun(TableMDPVecEnv(1, mdp, seed=1), 0.9, eps, lr, n=64, K=32, theta=0.0, seed=seed, dtype=np.float64)
    moved = _until_the_first_reward(sweep)
    assert moved == set(range(L - 1))  # (the only way to the end)
    assert (sweep.q[sorted(moved), RIGHT] > 0).all(), sweep.q[:, RIGHT]
    assert sweep.rt.events["queue_was_empty"] == sweep.rt.step_counter - 1, "before the reward nothing is worth an update"
    dyna = DynaRun(TableMDPVecEnv(1, mdp, seed=1), 0.9, eps, lr, n=64, seed=seed, dtype=np.float64)
    moved = _until_the_first_reward(dyna)
    assert dyna.rt.step_counter == sweep.rt.step_counter, "up to the first reward every table is zero: the same walk"
    assert (dyna.q[sorted(moved), RIGHT] == 0).any(), dyna.q[:, RIGHT]


# ---- 3. lists and queue ------------------------------------------------------------------------------------------------------------
def test_on_a_deterministic_environment_the_lists_are_the_canonical_ones():
    run = SweepRun(_env("table_deterministic", 1), 0.93, *_schedules(), n=3, K=4, theta=1e-3, seed=2, dtype=np.float32, agent_id=1)
    run.run(200)
    nxt, _, term, visited, count = run.planning_model
    head, link = run.predecessors
    want_head, want_link = canonical_lists(nxt, term, visited, count)
    assert np.array_equal(head, want_head) and np.array_equal(link, want_link) and (link >= 0).any()
    assert not run.rt.events["unlinked"]


def test_the_queue_by_hand():
    rt = SweepRuntime.__new__(SweepRuntime)
    rt.K, rt.events = 3, __import__("collections").Counter()
    rt.empty_queue()
    assert rt.pop() == -1
    rt.insert(7, 0.5)
    rt.insert(8, 0.25)
    rt.insert(7, 0.125)                      # a live entry keeps the larger priority
    assert (rt.cells, rt.priorities) == ([7, 8, -1], [0.5, 0.25, 0.0])
    rt.insert(8, 1.0)                        # ... and takes a larger one
    rt.insert(9, 0.25)
    assert (rt.cells, rt.priorities) == ([7, 8, 9], [0.5, 1.0, 0.25])
    rt.insert(10, 0.25)                      # full: not strictly greater than the smallest, dropped
    assert rt.cells == [7, 8, 9]
    rt.insert(10, 0.5)                       # strictly greater: the smallest gives way
    assert (rt.cells, rt.priorities) == ([7, 8, 10], [0.5, 1.0, 0.5])
    assert rt.pop() == 8 and (rt.cells, rt.priorities) == ([7, -1, 10], [0.5, 0.0, 0.5])
    rt.insert(11, 0.125)                     # the lowest free slot
    assert rt.cells == [7, 11, 10]
    assert rt.pop() == 7                     # the lowest index among equals
    assert rt.pop() == 10 and rt.pop() == 11 and rt.pop() == -1
    assert rt.events == {"insert_free": 4, "insert_keeps": 1, "insert_raises": 1, "dropped": 1, "evicted": 1,
                         "dropped_equal": 1, "insert_hole": 1, "pop_tie": 1}  # (10 at 0.25; 11 below 10; 7 before 10)
    rt.insert(3, 2.0)
    rt.insert(4, 2.0)
    rt.insert(5, 2.0)
    rt.insert(6, 3.0)                        # the lowest index among the equal smallest
    assert rt.cells == [6, 4, 5]


def _queue(cells, priorities):
    rt = SweepRuntime.__new__(SweepRuntime)
    rt.K, rt.events = len(cells), __import__("collections").Counter()
    rt.cells, rt.priorities = list(cells), list(priorities)
    return rt


def test_the_census_of_the_tie_events_by_hand():
    """Each queue is written out; the counter named beside it moves, and only where it should."""
    # pop_tie: two live slots share the maximum -> the lower index; a hole and a smaller entry do not count
    rt = _queue([5, -1, 6, 7], [2.0, 0.0, 2.0, 1.0])
    assert rt.pop() == 5 and rt.events == {"pop_tie": 1}
    assert rt.pop() == 6 and rt.pop() == 7 and rt.pop() == -1 and rt.events == {"pop_tie": 1}
    # a free slot's 0.0 is not an entry: a single live zero is no tie
    rt = _queue([-1, 9, -1], [0.0, 0.0, 0.0])
    assert rt.pop() == 9 and not rt.events
    # pop_inf
    rt = _queue([3, 4], [1.0, np.inf])
    assert rt.pop() == 4 and rt.events == {"pop_inf": 1}
    rt = _queue([3, 4], [np.inf, np.inf])
    assert rt.pop() == 3 and rt.events == {"pop_inf": 1, "pop_tie": 1}
    # evict_tie: full, two slots at the smallest, the newcomer is greater -> the lower of them gives way
    rt = _queue([1, 2, 3], [4.0, 0.5, 0.5])
    rt.insert(8, 1.0)
    assert rt.cells == [1, 8, 3] and rt.events == {"evicted": 1, "evict_tie": 1}
    rt.insert(9, 2.0)                        # one smallest now: an eviction without a tie
    assert rt.cells == [1, 8, 9] and rt.events == {"evicted": 2, "evict_tie": 1}
    # dropped_equal: the newcomer equals the smallest; a smaller one is dropped without the count
    rt.insert(10, 1.0)
    assert rt.cells == [1, 8, 9] and rt.events == {"evicted": 2, "evict_tie": 1, "dropped": 1, "dropped_equal": 1}
    rt.insert(10, 0.25)
    assert rt.events["dropped"] == 2 and rt.events["dropped_equal"] == 1
    # insert_equal: a live entry meets its own priority again
    rt.insert(8, 1.0)
    assert rt.priorities == [4.0, 1.0, 2.0] and rt.events["insert_equal"] == 1
    # insert_hole: the lowest free slot lies below a live one; a free slot above every live one is no hole
    rt = _queue([1, -1, 3, -1], [1.0, 0.0, 1.0, 0.0])
    rt.insert(4, 0.5)
    assert rt.cells == [1, 4, 3, -1] and rt.events == {"insert_free": 1, "insert_hole": 1}
    rt.insert(5, 0.5)
    assert rt.cells == [1, 4, 3, 5] and rt.events == {"insert_free": 2, "insert_hole": 1}


def test_the_census_of_unlinks_thresholds_and_the_held_row_by_hand():
    """A stochastic table MDP, whose cells change their outcome: the lists before and after each step say where the
    unlinked cell stood, and the counters must say the same; the held state is the observation after the step."""
    run = SweepRun(_env("table", 2), 0.93, *_schedules(), n=2, K=4, theta=0.0, seed=5, dtype=np.float64, agent_id=2)
    rt = run.rt
    A = run.q.shape[1]
    run.run(1)
    for _ in range(300):
        before = {x: list(lst) for x, lst in rt.lists.items()}
        ev0 = dict(rt.events)
        s = run.obs
        run.run(1)
        cell = s * A + rt.last_action
        moved = {k: rt.events[k] - ev0.get(k, 0) for k in ("unlinked", "unlink_head", "unlink_tail", "unlink_inner")}
        was = [lst for lst in before.values() if cell in lst]
        assert len(was) <= 1
        if moved["unlinked"]:
            lst = was[0]
            assert moved["unlink_head"] == (lst[0] == cell)
            assert moved["unlink_tail"] == (lst[-1] == cell and lst[0] != cell)
            assert moved["unlink_inner"] == (len(lst) >= 3 and lst[0] != cell)
        else:  # the cell was not linked, or it keeps its place in a list that no step 2 has touched
            assert not any(moved.values())
            assert not was or before[rt.model[cell][0]] == rt.lists[rt.model[cell][0]] == was[0]
        assert rt.held == run.obs
    ev = rt.events
    assert ev["unlink_head"] and ev["unlink_tail"] and ev["unlinked"] >= ev["unlink_head"] + ev["unlink_tail"]
    assert ev["propagate_held"] and ev["propagate_other"]
    assert ev["propagate_held"] + ev["propagate_other"] == ev["propagate_some"] + ev["propagate_none"]
    assert 0 < rt.smallest_compared < np.inf and not any(k.startswith("threshold_equal") for k in ev)
    # ... and a threshold equal to a priority is counted at its site, and does not pass
    rt.theta = 0.5
    assert not rt._passes(0.5, "plan") and rt._passes(0.75, "plan") and not rt._passes(0.25, "step") and not rt._passes(np.nan, "step")
    assert {k: v for k, v in ev.items() if k.startswith("threshold_equal")} == {"threshold_equal_plan": 1}
    assert rt.smallest_compared <= 0.25
    rt.theta = 0.0
    assert not rt._passes(0.0, "propagate") and "threshold_equal_propagate" not in ev  # P == theta == 0 is not the event


def test_the_census_of_rows_with_hidden_and_with_valid_nans_by_hand():
    run = SweepRun(_env("hash_masked", 1), 0.93, *_schedules(), n=1, K=4, theta=0.0, seed=5, dtype=np.float32, agent_id=1)
    rt, q = run.rt, run.q
    q[:] = np.arange(q.size, dtype=np.float32).reshape(q.shape)
    x = next(s for s in range(q.shape[0]) if len(rt.mask_of(s)) < q.shape[1])  # a state with a masked-out column
    cols = rt.mask_of(x)
    hidden, valid = int(np.setdiff1d(np.arange(q.shape[1]), cols)[0]), int(cols[0])
    assert rt._rowmax(x) == q[x][cols].max() and not rt.events
    q[x, hidden] = np.nan
    assert rt._rowmax(x) == q[x][cols].max() and rt.events == {"rowmax_hidden_nan": 1}
    q[x, valid] = np.nan
    assert np.isnan(rt._rowmax(x)) and rt.events == {"rowmax_hidden_nan": 1, "rowmax_valid_nan": 1}


# ---- 4. chaining ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_kind", ["hash_small", "table"])
def test_two_calls_equal_one_call(env_kind):
    def make():
        return SweepRun(_env(env_kind, 3), 0.93, *_schedules(), n=5, K=4, theta=1e-4, seed=4, dtype=np.float32, mode="vec", agent_id=3)

    whole, halves = make(), make()
    h, at = whole.run(120)
    h1, at1 = halves.run(60)
    h2, at2 = halves.run(60)
    assert np.array_equal(np.concatenate([h1, h2]), h) and np.array_equal(np.concatenate([at1, at2 + 60]), at)
    assert _same_table(whole.q, halves.q)
    for a, b in zip(whole.planning_model + whole.predecessors + whole.sweep_queue,
                    halves.planning_model + halves.predecessors + halves.sweep_queue):
        assert np.array_equal(a, b)
