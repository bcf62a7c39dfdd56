"""CPU: the NumPy model of the population's eligibility traces (tests/trace_model.py), which the GPU parity tests of
``QLearningPopulation(update_rule=..., trace_decay=lam)`` compare against.

* With ``lam = 0`` -- and with one replacing slot at any lambda -- the model is, bit for bit, ``TdRun``
  (tests/td_rules_model.py) of the same rule: this anchors its step order, draws, schedules and update arithmetic to the
  merged model, which is anchored to the oracle.  A table seeded with NaN and infinite cells is among the cases.
* With as many slots as the table has cells the model equals a dense loop written here, straight from the book: a full
  ``e[S, A]`` array, SARSA(lambda) and Watkins's Q(lambda).
* An eviction and a Watkins cut give the numbers worked out by hand below.
* Two model calls chained through the slots equal one call.
"""
import copy

import numpy as np
import pytest

from oracle import envs as oenvs
from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning, OracleSchedule
from table_mdp_model import TableMDPVecEnv, random_mdp
from td_rules_model import U64, TdRun, TdRuntime, oracle_schedule
from trace_model import TraceRun

RULES = ["sarsa", "q_learning"]
KINDS = ["replacing", "accumulating"]


def _env(kind, offset):
    if kind == "hash":
        return oenvs.HashTabularEnv(1, 60, 8, seed=3, agent_offset=offset)
    if kind == "hash_masked":  # 16 masked actions: the NumPy selection variants
        return oenvs.HashTabularEnv(1, 60, 16, seed=3, masked=True, agent_offset=offset)
    if kind == "hash_small":  # 16 cells: every one of them is visited many times
        return oenvs.HashTabularEnv(1, 4, 4, seed=3, agent_offset=offset)
    if kind == "bandit":
        return oenvs.RiggedBanditVecEnv(1, episode_len=7)
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    arrays, isd, masks = random_mdp(12, 5, 3, seed=4, masked=True)
    return TableMDPVecEnv(1, encode_table_mdp(*arrays, isd, masks), seed=3, agent_offset=offset)


def _schedules():
    return OracleSchedule("exponential", 0.9, 0.05, 0.99), OracleSchedule("linear", 0.4, None, -1e-3)


def _special_table(S, A, dt, seed, nan_row):
    """A random table with NaN, +inf and -inf cells and, if `nan_row`, one row of NaN (no selection finds a candidate
    there)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((S, A)).astype(dt)
    for count, value in ((4, np.nan), (3, np.inf), (3, -np.inf)):
        q.ravel()[rng.choice(S * A, size=count, replace=False)] = value
    if nan_row:
        q[rng.integers(0, S)] = np.nan
    return q


def _same_table(a, b):
    """Bit for bit, except that a NaN equals any NaN (sign and payload of a NaN are not part of the contract)."""
    nan = np.isnan(a)
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits[~nan], b.view(bits.dtype)[~nan])


def _same_run(got, want, K, calls=2):
    """`calls` chained calls of K steps on both; IndexError (no selectable action) must come at the same step."""
    for _ in range(calls):
        out = []
        for run in (got, want):
            try:
                out.append(run.run(K))
            except IndexError:
                out.append(None)
        assert (out[0] is None) == (out[1] is None)
        assert _same_table(got.q, want.q)
        assert got.rt.step_counter == want.rt.step_counter
        if out[0] is None:
            return False
        (h1, a1), (h2, a2) = out
        assert np.array_equal(h1, h2) and np.array_equal(a1, a2)
        assert (got.obs, got.acc[0], got.pending, got.eps, got.lr) == (want.obs, want.acc[0], want.pending, want.eps, want.lr)
    return True


# ---- 1. lambda = 0 and K = 1 replacing are the one-step rule ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("env_kind", ["hash", "hash_masked", "bandit", "table"])
@pytest.mark.parametrize("rule", RULES)
def test_lambda_zero_is_the_merged_model(rule, env_kind, kind, dt, mode):
    K, offset, seed = 150, 5, 9
    eps, lr = _schedules()
    got = TraceRun(_env(env_kind, offset), rule, 0.93, eps, lr, lam=0.0, K=4, kind=kind, seed=seed, dtype=dt, mode=mode,
                   agent_id=offset)
    eps, lr = _schedules()
    want = TdRun(_env(env_kind, offset), rule, 0.93, eps, lr, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    assert _same_run(got, want, K)
    assert got.q.any() and not got.slots[2].any()


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rule", RULES)
def test_lambda_zero_on_a_table_of_special_values(rule, kind, dt, mode):
    finished, reached = 0, 0
    for offset, masked, A in ((1, False, 8), (2, True, 8), (3, True, 16), (4, False, 8)):
        q0 = _special_table(30, A, dt, seed=offset, nan_row=offset == 4)
        runs = []
        for make in (lambda **kw: TraceRun(lam=0.0, K=3, kind=kind, **kw), TdRun):
            eps, lr = _schedules()
            runs.append(make(env=oenvs.HashTabularEnv(1, 30, A, seed=1, masked=masked, agent_offset=offset), rule=rule, gamma=0.93,
                             eps=eps, lr=lr, seed=2, dtype=dt, mode=mode, agent_id=offset, q0=q0))
        finished += _same_run(*runs, 150)
        reached = max(reached, runs[0].rt.step_counter)
        assert not np.isfinite(runs[0].q).all()
    # (under Q-learning a NaN spreads through the maxima until some row holds nothing else: those runs stop early, the
    # model and TdRun at the same step)
    assert finished or rule == "q_learning", "every run met a row without a selectable action"
    assert reached > 30


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("env_kind", ["hash", "hash_small", "bandit", "table"])
@pytest.mark.parametrize("rule", RULES)
def test_one_replacing_slot_is_the_merged_model_at_any_lambda(rule, env_kind, dt, mode):
    K, offset, seed = 150, 5, 9
    eps, lr = _schedules()
    got = TraceRun(_env(env_kind, offset), rule, 0.93, eps, lr, lam=0.9, K=1, kind="replacing", seed=seed, dtype=dt, mode=mode,
                   agent_id=offset)
    eps, lr = _schedules()
    want = TdRun(_env(env_kind, offset), rule, 0.93, eps, lr, seed=seed, dtype=dt, mode=mode, agent_id=offset)
    assert _same_run(got, want, K)
    assert got.q.any()


# ---- 2. the dense algorithm of the book -----------------------------------------------------------------------------------
class DenseRuntime(TdRuntime):
    """SARSA(lambda) / Watkins's Q(lambda) with a full trace array e[S, A] (Sutton & Barto, 1st ed., figures 7.11 and
    7.14; the selection and the draws are the oracle's).  delta is folded into ``u = lr * delta`` as the one-step update
    computes it; ``Q += u * e`` for every cell with a trace, with the arithmetic of the sweep."""

    def __init__(self, *args, lam, kind, **kw):
        super().__init__(*args, **kw)
        q = self.algorithm.q_table
        self.e = np.zeros_like(q)
        self.decay = q.dtype.type(np.float64(self.algorithm.discount_factor) * np.float64(lam))
        self.kind = kind

    def run_single_step(self, env, states, agent_rewards, reward_history):
        algo, q, e = self.algorithm, self.algorithm.q_table, self.e
        T = q.dtype.type
        k = self.step_counter
        actions = np.array([self.pending], dtype=np.int32) if self.rule == "sarsa" and self.pending is not None else self._pick(states)
        if hasattr(env, "step_index"):
            env.step_index = k
        s, a = int((states["observation"] if isinstance(states, dict) else states)[0]), int(actions[0])
        if self.rule == "q_learning" and not q[s, a] == np.max(self._valid_row(states)):
            e[:] = 0  # the action is not a greedy one
        next_states, rewards, terminateds, truncateds, infos = env.step(actions)
        agent_rewards += rewards
        lr = self.lr_schedule.get_value()
        self.lr_schedule.update(1)
        self.exploration_rate_schedule.update(1)
        self.step_counter = (k + 1) & U64
        if self.rule == "sarsa":
            nxt = self._pick(next_states)
            n = (next_states["observation"] if isinstance(next_states, dict) else next_states)[0]
            v = q[n, nxt[0]]
            self.pending = int(nxt[0])
        else:
            v = np.max(self._valid_row(next_states))
        r, term = rewards[0], bool(terminateds[0])
        if self.learn_mode == "iter":
            u = lr * (r + algo.discount_factor * (0 if term else v) - q[s, a])
        else:
            u = (lr * ((np.array([r]) + algo.discount_factor * np.array([v], dtype=q.dtype) * (1 - np.array([term]))) - q[[s], [a]]))[0]
        e[s, a] = 1 if self.kind == "replacing" else e[s, a] + T(1)
        live = e != 0
        if self.learn_mode == "vec" and q.dtype == np.float32:
            q[live] = (q[live].astype(np.float64) + np.float64(u) * e[live].astype(np.float64)).astype(np.float32)
        else:
            q[live] = q[live] + T(u) * e[live]
        e[:] = 0 if term else e * self.decay
        if terminateds[0] or truncateds[0]:
            reward_history.append(agent_rewards[0])
            agent_rewards[0] = 0
        return next_states, infos


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lam", [0.5, 1.0])
@pytest.mark.parametrize("rule", RULES)
def test_enough_slots_are_the_dense_algorithm(rule, lam, kind, dt, mode):
    offset, seed, gamma = 2, 5, 0.9
    env = oenvs.HashTabularEnv(1, 4, 4, seed=3, agent_offset=offset)
    got = TraceRun(copy.deepcopy(env), rule, gamma, *_schedules(), lam=lam, K=16, kind=kind, seed=seed, dtype=dt, mode=mode,
                   agent_id=offset)
    want = TdRun(copy.deepcopy(env), rule, gamma, *_schedules(), seed=seed, dtype=dt, mode=mode, agent_id=offset)
    algo = OracleQLearning(4, 4, gamma, seed=seed, dtype=np.dtype(dt))
    algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=env.agent_ids)
    eps, lr = _schedules()
    want.rt = DenseRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, rule=rule, lam=lam, kind=kind)
    above_one = False
    for _ in range(3):
        assert _same_run(got, want, 100, calls=1)
        above_one |= max(slot[2] for slot in got.rt.slots) > 1
        dense = np.zeros((4, 4), dtype=dt)
        states, actions, values = got.slots
        dense[states[values != 0], actions[values != 0]] = values[values != 0]
        assert np.array_equal(dense, want.rt.e)
    assert np.count_nonzero(want.rt.e) > 4 or rule == "q_learning"
    if kind == "accumulating" and lam == 1.0 and rule == "sarsa":
        assert above_one, "no trace grew past 1"


# ---- 3. by hand ---------------------------------------------------------------------------------------------------------
def _chain():
    """Three states in a row, one action: 0 -> 1 -> 2 -> end of the episode with reward 1; every episode starts in 0."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    nxt = np.array([1, 2, 0]).reshape(3, 1, 1)
    rew = np.array([0.0, 0.0, 1.0]).reshape(3, 1, 1)
    term = np.array([False, False, True]).reshape(3, 1, 1)
    return encode_table_mdp(np.ones((3, 1, 1)), nxt, rew, term)


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("rule", RULES)
def test_an_eviction_by_hand(rule, dt, mode):
    """The chain, gamma = lr = 0.5, lambda = 1 (d = 0.5), replacing, Q0 = [0.5, 0.25, 0.125]; one action, so both rules
    take the same steps and no draw matters.  Every number is a dyadic fraction: the arithmetic is exact.  K = 2:

    step 0: s = 0, s' = 1, v = 0.25: u = 0.5 (0 + 0.125 - 0.5) = -0.1875.  Slot 0 = (0, 1).
            Q[0] = 0.5 - 0.1875 = 0.3125.  Decay: e = [0.5, free].
    step 1: s = 1, s' = 2, v = 0.125: u = 0.5 (0 + 0.0625 - 0.25) = -0.09375.  Slot 1 = (1, 1).
            Q[0] = 0.3125 - 0.09375 * 0.5 = 0.265625, Q[1] = 0.25 - 0.09375 = 0.15625.  Decay: e = [0.25, 0.5].
    step 2: s = 2, r = 1, terminated: u = 0.5 (1 - 0.125) = 0.4375.  No slot is free: state 0, the smallest trace, is
            dropped for (2, 1).  Q[2] = 0.125 + 0.4375 = 0.5625, Q[1] = 0.15625 + 0.4375 * 0.5 = 0.375, Q[0] stays.
            The episode ended: every slot is free.
    With K = 3 nothing is dropped and step 2 also gives Q[0] = 0.265625 + 0.4375 * 0.25 = 0.375.
    """
    def make(K):
        return TraceRun(TableMDPVecEnv(1, _chain(), seed=1), rule, 0.5, OracleSchedule("constant", 0.0),
                        OracleSchedule("constant", 0.5), lam=1.0, K=K, seed=0, dtype=dt, mode=mode, q0=[[0.5], [0.25], [0.125]])

    run = make(2)
    want_q = [(0.3125, 0.25, 0.125), (0.265625, 0.15625, 0.125), (0.265625, 0.375, 0.5625)]
    want_slots = [([0, 0], [0.5, 0.0]), ([0, 1], [0.25, 0.5]), ([0, 0], [0.0, 0.0])]
    returns = []
    for t in range(3):
        history, _ = run.run(1)
        returns += history.tolist()
        assert tuple(run.q[:, 0]) == want_q[t], t
        states, actions, values = run.slots
        assert (states.tolist(), values.tolist()) == want_slots[t] and not actions.any(), t
    assert returns == [1.0] and run.obs == 0
    roomy = make(3)
    roomy.run(3)
    assert tuple(roomy.q[:, 0]) == (0.375, 0.375, 0.5625)


def test_a_watkins_cut_by_hand():
    """The rigged bandit (one state, reward = the action), epsilon 1: every action is an exploring one, given by the
    draws (pinned by the oracle's protocol; the test asserts the sequence it was worked out for).  gamma = lr = 0.5,
    lambda = 1 (d = 0.5), replacing, K = 2, Q0 = [0.5, 0.25].  The actions are 1, 0, 0:

    step 0: a = 1 is not greedy (0.25 != 0.5): cut (nothing to cut yet).  r = 1, v = max = 0.5:
            u = 0.5 (1 + 0.25 - 0.25) = 0.5.  Slot 0 = (a 1, e 1).  Q[1] = 0.75.  Decay: e = [0.5, free].
    step 1: a = 0 is not greedy either (0.5 != 0.75): CUT, slot 0 is freed, so action 1 gets nothing of this step.
            r = 0, v = 0.75: u = 0.5 (0 + 0.375 - 0.5) = -0.0625.  Slot 0 = (a 0, e 1).  Q[0] = 0.4375.  e = [0.5, free].
    step 2: a = 0 again, still not greedy (0.4375 != 0.75): cut.  r = 0, v = 0.75: u = 0.5 (0.375 - 0.4375) = -0.03125.
            Q[0] = 0.40625.
    Greedy actions keep their traces: see the second half.
    """
    def make(rule, seed):
        return TraceRun(oenvs.RiggedBanditVecEnv(1, episode_len=50), rule, 0.5, OracleSchedule("constant", 1.0),
                        OracleSchedule("constant", 0.5), lam=1.0, K=2, seed=seed, dtype=np.float64, q0=[[0.5, 0.25]])

    assert _actions(make("q_learning", 1), 3) == [1, 0, 0]
    run = make("q_learning", 1)
    want = [(0.5, 0.75), (0.4375, 0.75), (0.40625, 0.75)]
    slots = [([1, 0], [0.5, 0.0]), ([0, 0], [0.5, 0.0]), ([0, 0], [0.5, 0.0])]
    for t in range(3):
        run.run(1)
        assert tuple(run.q[0]) == want[t], t
        _, actions, values = run.slots
        assert (actions.tolist(), values.tolist()) == slots[t], t
    # without the cut (greedy actions keep the traces): Q0 = [0.25, 0.5], epsilon 0 -> a = 1, 1 and the second step
    # finds its own cell: u0 = 0.5 (1 + 0.25 - 0.5) = 0.375, Q[1] = 0.875; u1 = 0.5 (1 + 0.4375 - 0.875) = 0.28125,
    # Q[1] = 1.15625, one live slot
    greedy = TraceRun(oenvs.RiggedBanditVecEnv(1, episode_len=50), "q_learning", 0.5, OracleSchedule("constant", 0.0),
                      OracleSchedule("constant", 0.5), lam=1.0, K=2, seed=0, dtype=np.float64, q0=[[0.25, 0.5]])
    greedy.run(2)
    assert tuple(greedy.q[0]) == (0.25, 1.15625) and greedy.slots[2].tolist() == [0.5, 0.0]


def _actions(run, K):
    run.rt.trace = []
    run.run(K)
    return [int(a[0][0]) for a in run.rt.trace]


# ---- 4. chaining --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_kind", ["hash_small", "hash_masked", "bandit"])
@pytest.mark.parametrize("rule", RULES)
def test_two_calls_chained_through_the_slots_equal_one(rule, env_kind):
    K = 61

    def make():
        return TraceRun(_env(env_kind, 4), rule, 0.9, OracleSchedule("constant", 0.3), OracleSchedule("exponential", 0.5, 0.01, 0.99),
                        lam=0.8, K=4, kind="accumulating", seed=6, dtype=np.float32, agent_id=4)

    whole = make()
    ret, at = whole.run(2 * K)
    first = make()
    r1, a1 = first.run(K)

    def resume(slots):
        second = make()
        second.q[:] = first.q
        second.env, second.states, second.acc = copy.deepcopy(first.env), copy.deepcopy(first.states), first.acc.copy()
        second.rt.step_counter = first.rt.step_counter
        second.rt.lr_schedule.value, second.rt.exploration_rate_schedule.value = first.lr, first.eps
        second.rt.pending = first.rt.pending
        second.rt.slots = copy.deepcopy(slots)
        r2, a2 = second.run(K)
        return second, np.concatenate([r1, r2]), np.concatenate([a1, a2 + K])

    second, r12, a12 = resume(first.rt.slots)
    assert np.array_equal(second.q.view(np.uint8), whole.q.view(np.uint8))
    assert np.array_equal(r12, ret) and np.array_equal(a12, at)
    assert (second.obs, second.pending, second.lr) == (whole.obs, whole.pending, whole.lr)
    for a, b in zip(second.slots, whole.slots):
        assert np.array_equal(a, b)
    if first.slots[2].any():
        lost, _, _ = resume([[0, 0, np.float32(0)] for _ in range(4)])
        assert not np.array_equal(lost.q, whole.q)
