"""CPU: the NumPy model of the population's Dyna-Q (tests/dyna_model.py), which the GPU parity tests of
``QLearningPopulation(planning_steps=n)`` compare against.

* With the planning loop skipped (a hook of the model, not a product path) the model is, bit for bit,
  ``TdRun("q_learning")`` (tests/td_rules_model.py): this anchors its step order, draws, schedules and update arithmetic
  to the merged model, which is anchored to the oracle -- and it still learns its model and its list.
* A dense Dyna-Q loop written here, straight from the book (Sutton & Barto, 2nd ed., section 8.2: arrays ``Model[S, A]``,
  a list of the observed pairs), gives the same tables from the same draws.
* Two cases worked out by hand.
* The book's maze: planning finishes more episodes.
* Two model calls equal one call.
"""
import copy

import numpy as np
import pytest

from dist_classicrl_amd.environments.device_envs import encode_table_mdp
from dyna_model import STREAM_PLAN, DynaRun
from oracle import envs as oenvs
from oracle.draws import InjectedDraws, mulhi32, philox4x32
from oracle.qlearn_oracle import OracleQLearning, OracleSchedule
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import U64, TdRun, TdRuntime, oracle_schedule
from test_trace_model import _same_run, _same_table, _special_table


def _deterministic_mdp(S, A, seed, masked):
    """One outcome per (s, a): what the model remembers is what happens again."""
    arrays, isd, masks = random_mdp(S, A, 1, seed=seed, masked=masked)
    return encode_table_mdp(*arrays, isd, masks)


def _env(kind, offset):
    if kind == "hash":
        return oenvs.HashTabularEnv(1, 60, 8, seed=3, agent_offset=offset)
    if kind == "hash_masked":  # 16 masked actions: the NumPy selection variants
        return oenvs.HashTabularEnv(1, 60, 16, seed=3, masked=True, agent_offset=offset)
    if kind == "hash_small":  # 16 cells: every one of them is replayed many times
        return oenvs.HashTabularEnv(1, 4, 4, seed=3, agent_offset=offset)
    if kind == "bandit":
        return oenvs.RiggedBanditVecEnv(1, episode_len=7)
    if kind == "tictactoe":
        return oenvs.TicTacToeVecEnv(1, seed=5, agent_offset=offset)
    if kind == "table_deterministic":
        return TableMDPVecEnv(1, _deterministic_mdp(12, 5, 4, True), seed=3, agent_offset=offset)
    arrays, isd, masks = random_mdp(12, 5, 3, seed=4, masked=True)  # stochastic: outcomes are overwritten
    return TableMDPVecEnv(1, encode_table_mdp(*arrays, isd, masks), seed=3, agent_offset=offset)


def _schedules():
    return OracleSchedule("exponential", 0.9, 0.05, 0.99), OracleSchedule("linear", 0.4, None, -1e-3)


# ---- 1. without the planning loop the step is Q-learning's -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("env_kind", ["hash", "hash_masked", "bandit", "tictactoe", "table"])
def test_with_the_planning_loop_skipped_the_model_is_the_merged_model(env_kind, dt, mode):
    K, offset, seed = 150, 5, 9
    got = DynaRun(_env(env_kind, offset), 0.93, *_schedules(), n=4, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    got.rt.skip_planning = True
    want = TdRun(_env(env_kind, offset), "q_learning", 0.93, *_schedules(), seed=seed, dtype=dt, mode=mode, agent_id=offset)
    assert _same_run(got, want, K)
    assert got.q.any()
    nxt, rew, term, visited, count = got.planning_model
    assert count == (nxt >= 0).sum() > 1 and sorted(visited[:count]) == np.flatnonzero(nxt.ravel() >= 0).tolist()
    # ... and with it, planning changes the table
    planned = DynaRun(_env(env_kind, offset), 0.93, *_schedules(), n=4, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    planned.run(K)
    assert not _same_table(planned.q, want.q)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_skipped_planning_on_a_table_of_special_values(dt, mode):
    reached = 0
    for offset, masked, A in ((1, False, 8), (2, True, 8), (3, True, 16), (4, False, 8)):
        q0 = _special_table(30, A, dt, seed=offset, nan_row=offset == 4)
        env = oenvs.HashTabularEnv(1, 30, A, seed=1, masked=masked, agent_offset=offset)
        got = DynaRun(copy.deepcopy(env), 0.93, *_schedules(), n=2, seed=2, dtype=dt, mode=mode, agent_id=offset, q0=q0)
        got.rt.skip_planning = True
        want = TdRun(copy.deepcopy(env), "q_learning", 0.93, *_schedules(), seed=2, dtype=dt, mode=mode, agent_id=offset, q0=q0)
        _same_run(got, want, 150)
        reached = max(reached, got.rt.step_counter)
    assert reached > 30


# ---- 2. the dense algorithm of the book --------------------------------------------------------------------------------------
class PlanDraws:
    """The adapter that hands the dense loop the protocol's planning draws: ``index(k, i, count)`` is the position in the
    list of observed pairs that planning update ``i`` of the step with draw counter ``k`` replays."""

    def __init__(self, seed, agent_id):
        self.seed, self.agent_id = int(seed), int(agent_id)

    def index(self, k, i, count):
        words = philox4x32(self.agent_id, k & 0xFFFFFFFF, k >> 32, STREAM_PLAN | ((i >> 2) << 8), self.seed, self.seed >> 32)
        return int(mulhi32(words[i & 3], count))


class DenseDyna(TdRuntime):
    """Tabular Dyna-Q (Sutton & Barto, 2nd ed., section 8.2, the boxed algorithm): (a) S, (b) A epsilon-greedy, (c) take A,
    observe R, S', (d) the Q-learning update, (e) Model(S, A) <- R, S', (f) n times: a previously observed pair at random,
    its modelled outcome, the Q-learning update.  The model is three dense arrays and a list of the observed pairs; the
    selection and the draws are the oracle's."""

    def __init__(self, *args, n, draws, valid, **kw):
        super().__init__(*args, **kw)
        S, A = self.algorithm.q_table.shape
        self.n, self.draws, self.valid = n, draws, valid
        self.m_next = np.zeros((S, A), dtype=np.int64)
        self.m_reward = np.zeros((S, A), dtype=np.float32)
        self.m_term = np.zeros((S, A), dtype=bool)
        self.observed = np.zeros((S, A), dtype=bool)
        self.pairs = []

    def _q_update(self, s, a, r, s_next, term, lr):
        algo, q = self.algorithm, self.algorithm.q_table
        row = q[s_next] if self.valid is None else q[s_next][np.flatnonzero(self.valid(s_next))]
        v = np.max(row) if row.size else q.dtype.type(-np.inf)
        if self.learn_mode == "iter":
            q[s, a] += lr * (r + algo.discount_factor * (0 if term else v) - q[s, a])
        else:
            targets = np.array([r]) + algo.discount_factor * np.array([v], dtype=q.dtype) * (1 - np.array([term]))
            np.add.at(q, ([s], [a]), lr * (targets - q[[s], [a]]))

    def run_single_step(self, env, states, agent_rewards, reward_history):
        k = self.step_counter
        actions = self._pick(states)
        if hasattr(env, "step_index"):
            env.step_index = k
        s, a = int((states["observation"] if isinstance(states, dict) else states)[0]), int(actions[0])
        next_states, rewards, terminateds, truncateds, infos = env.step(actions)
        agent_rewards += rewards
        lr = self.lr_schedule.get_value()
        self.lr_schedule.update(1)
        self.exploration_rate_schedule.update(1)
        self.step_counter = (k + 1) & U64
        s_next = int((next_states["observation"] if isinstance(next_states, dict) else next_states)[0])
        with np.errstate(all="ignore"):
            self._q_update(s, a, rewards[0], s_next, bool(terminateds[0]), lr)
            if not self.observed[s, a]:
                self.observed[s, a] = True
                self.pairs.append((s, a))
            self.m_next[s, a], self.m_reward[s, a], self.m_term[s, a] = s_next, rewards[0], terminateds[0]
            for i in range(self.n):
                ps, pa = self.pairs[self.draws.index(k, i, len(self.pairs))]
                self._q_update(ps, pa, self.m_reward[ps, pa], int(self.m_next[ps, pa]), bool(self.m_term[ps, pa]), lr)
        if terminateds[0] or truncateds[0]:
            reward_history.append(agent_rewards[0])
            agent_rewards[0] = 0
        return next_states, infos


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("env_kind", ["hash", "hash_small", "hash_masked", "table_deterministic"])
def test_the_model_is_the_dense_algorithm_of_the_book(env_kind, n, dt, mode):
    offset, seed, gamma = 2, 5, 0.9
    env = _env(env_kind, offset)
    got = DynaRun(copy.deepcopy(env), gamma, *_schedules(), n=n, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    want = TdRun(copy.deepcopy(env), "q_learning", gamma, *_schedules(), seed=seed, dtype=dt, mode=mode, agent_id=offset)
    algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dt))
    algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=env.agent_ids)
    eps, lr = _schedules()
    valid = (lambda obs: want.env.action_masks(np.array([obs]))[0]) if env.masked else None
    want.rt = DenseDyna(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, rule="q_learning", n=n,
                        draws=PlanDraws(seed, offset), valid=valid)
    for _ in range(3):
        assert _same_run(got, want, 100, calls=1)
        nxt, rew, term, visited, count = got.planning_model
        dense = want.rt
        assert np.array_equal(nxt >= 0, dense.observed) and count == len(dense.pairs)
        assert [divmod(int(c), env.action_size) for c in visited[:count]] == dense.pairs
        seen = dense.observed
        assert np.array_equal(nxt[seen], dense.m_next[seen]) and np.array_equal(rew[seen], dense.m_reward[seen])
        assert np.array_equal(term[seen], dense.m_term[seen])
    assert got.q.any() and count > 3


# ---- 3. by hand ----------------------------------------------------------------------------------------------------------------
def _chain(next_states, rewards, terminated):
    """A deterministic one-action MDP from per-state outcomes, started in state 0."""
    S = len(next_states)
    shape = (S, 1, 1)
    isd = np.zeros(S)
    isd[0] = 1
    return encode_table_mdp(np.ones(shape), np.array(next_states).reshape(shape), np.array(rewards, dtype=np.float64).reshape(shape),
                            np.array(terminated).reshape(shape), isd)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_three_state_chain_by_hand(dt, mode):
    """0 -(r=1)-> 1 -(r=0)-> 2 -(r=0, terminated)-> start; one action, lr = gamma = 0.5, n = 2, Q = 0.

    Step 0: Q[0,0] = 0 + .5 (1 + .5 * 0 - 0) = .5.  One cell is seen, so both planning updates replay it, whatever the
    draws: p = 1, max Q[1] = 0: Q[0,0] = .5 + .5 (1 - .5) = .75, then .75 + .5 (1 - .75) = .875.
    Step 1: Q[1,0] = 0 + .5 (0 + .5 * 0 - 0) = 0.  Two cells are seen; each replay of cell 0 halves the distance of Q[0,0]
    to 1 (max Q[1] is still 0), each replay of cell 1 leaves Q[1,0] = 0: Q[0,0] = 1 - .125 * .5^z, z the number of draws
    with mulhi32(x, 2) == 0."""
    mdp = _chain([1, 2, 0], [1.0, 0.0, 0.0], [False, False, True])
    const = OracleSchedule("constant", 0.5)
    run = DynaRun(TableMDPVecEnv(1, mdp, seed=1), 0.5, OracleSchedule("constant", 0.0), const, n=2, seed=7, dtype=dt, mode=mode)
    run.run(1)
    assert run.q.tolist() == [[0.875], [0.0], [0.0]]
    nxt, rew, term, visited, count = run.planning_model
    assert (nxt.tolist(), rew.tolist(), term.tolist()) == ([[1], [-1], [-1]], [[1.0], [0.0], [0.0]], [[False]] * 3)
    assert (visited.tolist(), count) == ([0, -1, -1], 1)
    z = sum(int(mulhi32(x, 2)) == 0 for x in run.rt.plan_draws(1))
    run.run(1)
    assert run.q.tolist() == [[1 - 0.125 * 0.5 ** z], [0.0], [0.0]]
    assert run.planning_model[3].tolist() == [0, 1, -1]
    run.run(1)  # the terminated step: the model remembers the observation after the reset, and the flag
    nxt, rew, term, visited, count = run.planning_model
    assert (nxt.tolist(), term.tolist(), visited.tolist(), count) == ([[1], [2], [0]], [[False], [False], [True]], [0, 1, 2], 3)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_replaying_the_cell_just_updated_by_hand(dt, mode):
    """0 -(r=1)-> 0, one action, lr = gamma = 0.5, n = 2, Q = 0: the replayed cell is the one just stored, and p == s.

    Step 0: m is taken before the store: Q[0,0] = 0 + .5 (1 + .5 * 0 - 0) = .5.  Planning reads the row as it stands:
    m_0 = .5: Q[0,0] = .5 + .5 (1 + .25 - .5) = .875; m_1 = .875: Q[0,0] = .875 + .5 (1 + .4375 - .875) = 1.15625."""
    mdp = _chain([0, 0], [1.0, 0.0], [False, False])
    const = OracleSchedule("constant", 0.5)
    run = DynaRun(TableMDPVecEnv(1, mdp, seed=1), 0.5, OracleSchedule("constant", 0.0), const, n=2, seed=7, dtype=dt, mode=mode)
    run.run(1)
    assert run.q.tolist() == [[1.15625], [0.0]]
    assert run.planning_model[4] == 1


# ---- 4. the book's maze ------------------------------------------------------------------------------------------------------------
MAZE = [
    ".......WG",
    "..W....W.",
    "S.W....W.",
    "..W......",
    ".....W...",
    ".........",
]


def dyna_maze():
    """The 6 x 9 maze of Sutton & Barto figure 8.2 as a finite MDP: up, down, right, left; a move into a wall or off the
    grid stays; reaching G pays 1 and ends the episode; every episode starts at S."""
    rows, cols = len(MAZE), len(MAZE[0])
    S = rows * cols
    nxt = np.zeros((S, 4, 1), dtype=np.int64)
    rew = np.zeros((S, 4, 1))
    term = np.zeros((S, 4, 1), dtype=bool)
    isd = np.zeros(S)
    for r in range(rows):
        for c in range(cols):
            s = r * cols + c
            if MAZE[r][c] == "S":
                isd[s] = 1
            for a, (dr, dc) in enumerate(((-1, 0), (1, 0), (0, 1), (0, -1))):
                r2, c2 = r + dr, c + dc
                if not (0 <= r2 < rows and 0 <= c2 < cols) or MAZE[r2][c2] == "W":
                    r2, c2 = r, c
                nxt[s, a, 0] = r2 * cols + c2
                if MAZE[r2][c2] == "G" and MAZE[r][c] != "G":
                    rew[s, a, 0], term[s, a, 0] = 1.0, True
    return encode_table_mdp(np.ones((S, 4, 1)), nxt, rew, term, isd)


def test_planning_finishes_more_episodes_in_the_books_maze():
    """8 runs (agent ids 0 .. 7, one seed) of 3 000 steps with alpha = 0.1, epsilon = 0.1, gamma = 0.95, float64, iter.

    Episodes finished per run, measured on this model before the assertion was written:
        n = 0  : [4, 6, 11, 5, 47, 1, 8, 4], total 86
        n = 16 : [131, 143, 110, 60, 148, 21, 138, 85], total 836
    n = 16 finishes strictly more episodes in total, and in at least 7 of the 8 runs."""
    mdp = dyna_maze()
    plain, planned = [], []
    for r in range(8):
        sched = OracleSchedule("constant", 0.1), OracleSchedule("constant", 0.1)
        a = TdRun(TableMDPVecEnv(1, mdp, seed=1, agent_offset=r), "q_learning", 0.95, *sched, seed=3, dtype=np.float64, agent_id=r)
        b = DynaRun(TableMDPVecEnv(1, mdp, seed=1, agent_offset=r), 0.95, *sched, n=16, seed=3, dtype=np.float64, agent_id=r)
        plain.append(len(a.run(3000)[0]))
        planned.append(len(b.run(3000)[0]))
    print("episodes, n = 0:", plain, sum(plain), "n = 16:", planned, sum(planned))
    assert sum(planned) > sum(plain)
    assert sum(p > q for p, q in zip(planned, plain)) >= 7


# ---- 5. chaining -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_kind", ["hash_small", "table"])
def test_two_model_calls_equal_one(env_kind):
    offset = 3
    one = DynaRun(_env(env_kind, offset), 0.9, *_schedules(), n=5, seed=4, dtype=np.float32, mode="vec", agent_id=offset)
    two = DynaRun(_env(env_kind, offset), 0.9, *_schedules(), n=5, seed=4, dtype=np.float32, mode="vec", agent_id=offset)
    h1, a1 = one.run(120)
    h2a, a2a = two.run(60)
    h2b, a2b = two.run(60)
    assert _same_table(one.q, two.q)
    assert np.array_equal(h1, np.concatenate([h2a, h2b])) and np.array_equal(a1, np.concatenate([a2a, a2b + 60]))
    for x, y in zip(one.planning_model, two.planning_model):
        assert np.array_equal(x, y)
