"""NumPy model of the population's double estimator (``QLearningPopulation(double_q=True)``, ``k_double_rollout`` /
``k_double_evaluate``): Double Q-learning (van Hasselt 2010; Sutton & Barto 6.7) for ONE agent.

Test infrastructure.  The reference has no Double Q-learning, so there is no reference to pin this against; DESIGN
section 4.3c defines the step and this file restates that definition.  Like ``td_rules_model.py`` it is built ON the
pinned oracle: the selection (the dispatcher's rule for one agent, the draw protocol, the NaN rule) is
``OracleRuntime._choose_actions`` / ``_greedy`` reading the table of its ``OracleQLearning`` -- which here holds the SUM
row ``z = T(A[s] + B[s])``, written just before each pick -- the update arithmetic is ``TdRuntime._update``
(``single_learn`` / ``learn_vec`` with the bootstrap scalar handed in), the environments are ``oracle.envs`` and
``table_mdp_model``.  What it adds:

* the coin: ``x3 >> 31`` of the step's policy Philox block (``oracle.draws.philox4x32`` called directly; the protocol
  leaves ``x3`` unused): 0 -> X = A, Y = B; 1 -> X = B, Y = A;
* the bootstrap scalar: ``a* = np.argmax(X[s'][valid])``, ``v = Y[s'][valid][a*]``; without a valid column ``T(-inf)``;
* the update lands in X only.

A step whose pick finds no selectable action raises ``IndexError``: the engine flags such a run and the tests leave it out
of the comparison.
"""

from __future__ import annotations

import numpy as np

from oracle.draws import STREAM_POLICY, InjectedDraws, philox4x32
from oracle.qlearn_oracle import OracleQLearning
from td_rules_model import U64, TdRuntime, oracle_schedule


def coin(seed: int, agent_id: int, step: int) -> int:
    """Which table step ``step`` of the agent updates: 0 = A, 1 = B."""
    x3 = philox4x32(agent_id, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, STREAM_POLICY, seed, seed >> 32)[3]
    return int(x3) >> 31


def bootstrap(x_row, y_row, dtype):
    """``Y[a*]`` with ``a* = np.argmax(X)`` over the valid columns handed in (ascending); empty: ``T(-inf)``."""
    if x_row.size == 0:
        return dtype.type(-np.inf)
    return y_row[np.argmax(x_row)]


class DoubleRuntime(TdRuntime):
    """``OracleRuntime`` for one agent with two tables.  ``self.algorithm.q_table`` is the table the oracle's selection
    reads: it holds sum rows only (``_present``); the learned values live in ``self.tables`` (A, B)."""

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", agent_id=0):
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode, rule="q_learning")
        self.tables = (np.zeros_like(algorithm.q_table), np.zeros_like(algorithm.q_table))
        self.agent_id = int(agent_id)
        self.coins = []  # (step, coin) of every training step, for the tests

    def _present(self, states):
        s = (states["observation"] if isinstance(states, dict) else states)[0]
        with np.errstate(all="ignore"):
            self.algorithm.q_table[s] = self.tables[0][s] + self.tables[1][s]  # one addition in the table dtype

    def present_all(self):
        with np.errstate(all="ignore"):
            self.algorithm.q_table[:] = self.tables[0] + self.tables[1]

    def run_single_step(self, env, states, agent_rewards, reward_history):
        k = self.step_counter
        self._present(states)
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
        c = coin(self.algorithm._rng.seed, self.agent_id, k)
        self.coins.append((k, c))
        X, Y = self.tables[c], self.tables[1 - c]
        if isinstance(next_states, dict):
            n, cols = next_states["observation"][0], np.where(next_states["action_mask"][0])
        else:
            n, cols = next_states[0], slice(None)
        z_table = self.algorithm.q_table
        with np.errstate(all="ignore"):
            v = bootstrap(X[n][cols], Y[n][cols], z_table.dtype)
            self.algorithm.q_table = X  # TdRuntime._update works on the algorithm's table
            try:
                self._update(s, actions[0], rewards[0], v, terminateds[0], lr)
            finally:
                self.algorithm.q_table = z_table
        if terminateds[0] or truncateds[0]:
            reward_history.append(agent_rewards[0])
            agent_rewards[0] = 0
        return next_states, infos

    def evaluate_steps(self, env, steps):
        self.present_all()
        if hasattr(env, "step_index"):
            env.step_index = self.step_counter
        return super().evaluate_steps(env, steps)

    def evaluate_episodes(self, env, episodes):
        self.present_all()
        if hasattr(env, "step_index"):
            env.step_index = self.step_counter
        return super().evaluate_episodes(env, episodes)


class DoubleRun:
    """One run of a double population as the model sees it (``td_rules_model.TdRun`` with two tables).  ``run(K)`` takes
    K training steps and returns the call's episode returns and the steps (within the call) at which they ended;
    ``evaluate_steps`` / ``evaluate_episodes`` are the greedy evaluations on the sum table: ``(total, history)``."""

    def __init__(self, env, gamma, eps, lr, *, seed, dtype, mode="iter", agent_id=0, qa0=None, qb0=None):
        self.env = env
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        self.rt = DoubleRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, agent_id=int(ids[0]))
        if qa0 is not None:
            self.rt.tables[0][:] = qa0
        if qb0 is not None:
            self.rt.tables[1][:] = qb0
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    def reset(self):
        self.states, _ = self.env.reset()
        self.acc = np.zeros(1, dtype=np.float32)

    def run(self, K, reset=False):
        if reset or self.states is None:
            self.reset()
        history, at = [], []
        for t in range(K):
            n = len(history)
            self.states, _ = self.rt.run_single_step(self.env, self.states, self.acc, history)
            at += [t] * (len(history) - n)
        return np.array(history, dtype=np.float32), np.array(at, dtype=np.int32)

    def evaluate_steps(self, env, steps):
        return self.rt.evaluate_steps(env, steps)

    def evaluate_episodes(self, env, episodes):
        return self.rt.evaluate_episodes(env, episodes)

    @property
    def qa(self):
        return self.rt.tables[0]

    @property
    def qb(self):
        return self.rt.tables[1]

    @property
    def obs(self):
        return int((self.states["observation"] if isinstance(self.states, dict) else self.states)[0])

    @property
    def eps(self):
        return self.rt.exploration_rate_schedule.get_value()

    @property
    def lr(self):
        return self.rt.lr_schedule.get_value()
