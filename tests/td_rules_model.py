"""NumPy model of the population's update rules (``QLearningPopulation(update_rule=...)``, ``k_rollout_runs`` /
``k_rollout_runs_td``): Q-learning, SARSA and Expected SARSA for ONE agent.

Test infrastructure.  The reference has no on-policy rule, so there is no reference to pin these against; DESIGN section
4.3c defines them and this file restates that definition.  It is built ON the pinned oracle: selection (the
dispatcher's rule for one agent, the draw protocol) is ``OracleRuntime._choose_actions`` / ``OracleQLearning``, the
environments are ``oracle.envs`` and ``table_mdp_model``.  What it adds is the step order and the bootstrap scalar:

* the update is ``single_learn`` (``learn_mode="iter"``) / ``learn_vec`` (``"vec"``) with ONE scalar replaced: where they
  take ``np.max(Q[s', valid])``, the rule's ``v`` goes in (``_update``; with rule ``q_learning`` the loop is, bit for
  bit, ``OracleRuntime`` on one agent -- tests/test_td_rules_model.py);
* ``expected_sarsa``: ``v = T((1 - e) * float64(max) + e * mean)``, mean = left-to-right float64 sum of the valid
  columns / their count, e = the NEXT step's epsilon clamped to [0, 1];
* ``sarsa``: the next action a' is picked BEFORE the update, from the row of s' as it stands then, with the draws and
  epsilon of the next step; ``v = Q[s', a']``; a' is kept as the run's pending action and is the action of the next
  step (also across ``run`` calls, and after a terminated step, where s' is the reset observation).

A step whose pick finds no selectable action raises ``IndexError`` (the list variants' -1 included): the engine flags
such a run and the tests leave it out of the comparison.
"""

from __future__ import annotations

import numpy as np

from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning, OracleRuntime, OracleSchedule

RULES = ("q_learning", "sarsa", "expected_sarsa")
U64 = 0xFFFFFFFFFFFFFFFF


def oracle_schedule(s) -> OracleSchedule:
    """An ``OracleSchedule`` with the recurrence and current value of a product schedule (or of an OracleSchedule)."""
    if isinstance(s, OracleSchedule):
        return OracleSchedule(s.kind, s.value, s.min_value, s.decay)
    name = type(s).__name__
    if name == "ExponentialSchedule":
        return OracleSchedule("exponential", s.get_value(), s.min_value, s.decay_rate)
    if name == "LinearSchedule":
        return OracleSchedule("linear", s.get_value(), None, s.decay_rate)
    return OracleSchedule("constant", s.get_value())


def env_word(env) -> int:
    """The env-internal word the device keeps per agent (``state_dict["aux"]``) for a one-agent oracle environment."""
    if hasattr(env, "episode"):   # HashTabularEnv: episode index
        return int(env.episode[0])
    if hasattr(env, "t"):         # bandit: step within the episode
        return int(env.t[0])
    if hasattr(env, "m1"):        # TicTacToe: cells of mark 1 | cells of mark 2 << 9 | agent plays mark 2 << 18
        return int(env.m1[0]) | int(env.m2[0]) << 9 | (int(env.agent_mark[0]) == 2) << 18
    return 0


def expected_value(row, eps_next, dtype):
    """Expected SARSA's bootstrap value of ``row`` (the valid columns of Q[s'], ascending, table dtype)."""
    with np.errstate(all="ignore"):
        m = np.max(row) if row.size else dtype.type(-np.inf)
        tot = np.float64(0.0)
        for x in row:
            tot = tot + np.float64(x)
        mean = tot / np.float64(row.size)
        e = 0.0 if not (eps_next > 0) else 1.0 if eps_next >= 1 else eps_next
        keep = np.float64(1.0 - e) * np.float64(m)
        spread = np.float64(e) * mean
        return dtype.type(keep + spread)


class TdRuntime(OracleRuntime):
    """``OracleRuntime`` for one agent with a choice of update rule.  ``pending``: the SARSA action already chosen for
    the next step (None: none)."""

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", rule="q_learning"):
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode)
        assert rule in RULES
        self.rule = rule
        self.pending = None

    def _pick(self, states):
        """The oracle's selection for the one agent at (step_counter, current epsilon); IndexError without a candidate."""
        actions = self._choose_actions(states)
        if actions[0] < 0:
            msg = "Cannot choose from an empty sequence"
            raise IndexError(msg)
        return actions

    def _valid_row(self, states):
        q = self.algorithm.q_table
        if isinstance(states, dict):
            return q[states["observation"][0]][np.where(states["action_mask"][0])]
        return q[states[0]]

    def _update(self, s, a, reward, v, terminated, lr):
        """single_learn (:728-768) / learn_vec (:819-891) with the bootstrap scalar handed in."""
        algo = self.algorithm
        if self.learn_mode == "iter":
            nxt = 0 if terminated else v
            target = reward + algo.discount_factor * nxt
            prediction = algo.get_q_value(s, a)
            algo.add_q_value(s, a, lr * (target - prediction))
        else:
            states, actions = np.array([s]), np.array([a])
            rewards, term = np.array([reward]), np.array([terminated])
            maxima = np.array([v], dtype=algo.q_table.dtype)
            targets = rewards + algo.discount_factor * maxima * (1 - term)
            np.add.at(algo.q_table, (states, actions), lr * (targets - algo.q_table[states, actions]))

    def run_single_step(self, env, states, agent_rewards, reward_history):
        k = self.step_counter
        if self.rule == "sarsa" and self.pending is not None:
            actions = np.array([self.pending], dtype=np.int32)
        else:
            actions = self._pick(states)
        if self.trace is not None:
            self.trace.append((actions.copy(), self.exploration_rate_schedule.get_value(), self.lr_schedule.get_value()))
        if hasattr(env, "step_index"):
            env.step_index = k
        s = (states["observation"] if isinstance(states, dict) else states)[0]
        next_states, rewards, terminateds, truncateds, infos = env.step(actions)
        agent_rewards += rewards
        lr = self.lr_schedule.get_value()
        self.lr_schedule.update(1)
        self.exploration_rate_schedule.update(1)
        self.step_counter = (k + 1) & U64
        dtype = self.algorithm.q_table.dtype
        with np.errstate(all="ignore"):
            if self.rule == "sarsa":
                nxt = self._pick(next_states)  # draws of step k + 1, epsilon after this step's advance, row before the update
                n = (next_states["observation"] if isinstance(next_states, dict) else next_states)[0]
                v = self.algorithm.q_table[n, nxt[0]]
                self.pending = int(nxt[0])
            elif self.rule == "expected_sarsa":
                v = expected_value(self._valid_row(next_states), self.exploration_rate_schedule.get_value(), dtype)
            else:
                row = self._valid_row(next_states)
                v = np.max(row) if row.size else dtype.type(-np.inf)
            self._update(s, actions[0], rewards[0], v, terminateds[0], lr)
        if terminateds[0] or truncateds[0]:
            reward_history.append(agent_rewards[0])
            agent_rewards[0] = 0
        return next_states, infos


class TdRun:
    """One run of a population as the model sees it: a one-agent oracle environment ``env`` (whose ``agent_ids`` key
    the draws where it has them, else ``agent_id``), its table, schedules and pending action.  ``run(K)`` takes K
    training steps and returns the call's episode returns and the steps (within the call) at which they ended."""

    def __init__(self, env, rule, gamma, eps, lr, *, seed, dtype, mode="iter", agent_id=0, q0=None):
        self.env = env
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        if q0 is not None:
            algo.q_table[:] = q0
        self.rt = TdRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, rule=rule)
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    def reset(self):
        self.states, _ = self.env.reset()
        self.acc = np.zeros(1, dtype=np.float32)
        self.rt.pending = None

    def run(self, K, reset=False):
        if reset or self.states is None:
            self.reset()
        history, at = [], []
        for t in range(K):
            n = len(history)
            self.states, _ = self.rt.run_single_step(self.env, self.states, self.acc, history)
            at += [t] * (len(history) - n)
        return np.array(history, dtype=np.float32), np.array(at, dtype=np.int32)

    @property
    def q(self):
        return self.rt.algorithm.q_table

    @property
    def obs(self):
        return int((self.states["observation"] if isinstance(self.states, dict) else self.states)[0])

    @property
    def pending(self):
        return -1 if self.rt.pending is None else self.rt.pending

    @property
    def eps(self):
        return self.rt.exploration_rate_schedule.get_value()

    @property
    def lr(self):
        return self.rt.lr_schedule.get_value()
