"""NumPy model of the population's eligibility traces (``QLearningPopulation(update_rule=..., trace_decay=lam)``,
``k_trace_rollout``): SARSA(lambda) and Watkins's Q(lambda) for ONE agent.

Test infrastructure, like ``n_step_model.py``, built on ``td_rules_model.py``: the pick, the valid row and the update
expressions are ``TdRuntime``'s.  DESIGN section 4.3c defines the step and this file restates it.  A run keeps ``K``
slots ``[s_i, a_i, e_i]``, ``e_i`` of the table dtype ``T``; a slot with ``e_i == 0`` is free and live slots name
distinct cells.  ``d = T(float64(gamma) * float64(lambda))``.  One step:

1. the action is the 1-step rule's (SARSA: the pending action, else a pick; Q-learning: a pick -- and unless
   ``Q[s, a] == np.max(Q[s, valid])`` every ``e_i = 0``: Watkins's cut);
2. the environment steps;
3. ``v`` is the 1-step rule's bootstrap scalar from the row of s' before any store of this step (SARSA picks a' here);
4. ``u`` is the increment of ``_update`` for ``(Q[s, a], r, v, terminated, lr)``: of type ``T``, except ``learn_vec`` on a
   float32 table, where it is the float64 ``lr * (target - Q[s, a])``, unrounded; the cell is not stored here;
5. mark: a live slot that holds ``(s, a)`` gets ``e = 1`` (replacing) or ``e + 1`` (accumulating); otherwise ``(s, a, 1)``
   goes into the lowest free slot, else into the slot of the smallest ``e`` (lowest index among equals);
6. sweep: every live slot ``Q[s_i, a_i] = Q[s_i, a_i] + u * e_i`` in ``T`` (float32 ``learn_vec``:
   ``float32(float64(Q) + u * float64(e_i))``);
7. decay: terminated: every ``e_i = 0``; else ``e_i = T(e_i * d)``.
"""

from __future__ import annotations

import numpy as np

from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning
from td_rules_model import U64, TdRun, TdRuntime, oracle_schedule

TRACE_RULES = ("sarsa", "q_learning")
TRACE_KINDS = ("replacing", "accumulating")


class TraceRuntime(TdRuntime):
    """``TdRuntime`` with ``K`` trace slots.  ``slots``: K lists ``[s, a, e]``, ``e`` a scalar of the table dtype."""

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", rule="sarsa", lam=0.0, K=16,
                 kind="replacing"):
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode, rule)
        assert rule in TRACE_RULES and kind in TRACE_KINDS and K >= 1
        self.K = int(K)
        self.kind = kind
        self.T = algorithm.q_table.dtype.type
        self.decay = self.T(np.float64(algorithm.discount_factor) * np.float64(lam))
        self.clear()

    def clear(self):
        self.slots = [[0, 0, self.T(0)] for _ in range(self.K)]

    def _increment(self, s, a, reward, v, terminated, lr):
        """The increment ``_update`` would add to Q[s, a] (single_learn / learn_vec with the scalar handed in)."""
        algo = self.algorithm
        if self.learn_mode == "iter":
            nxt = 0 if terminated else v
            target = reward + algo.discount_factor * nxt
            prediction = algo.get_q_value(s, a)
            return self.T(lr * (target - prediction))  # (what add_q_value adds to the cell: the table's dtype)
        states, actions = np.array([s]), np.array([a])
        rewards, term = np.array([reward]), np.array([terminated])
        maxima = np.array([v], dtype=algo.q_table.dtype)
        targets = rewards + algo.discount_factor * maxima * (1 - term)
        return (lr * (targets - algo.q_table[states, actions]))[0]  # float64 on either table

    def _mark(self, s, a):
        one = self.T(1)
        for slot in self.slots:
            if slot[2] != 0 and slot[0] == s and slot[1] == a:
                slot[2] = one if self.kind == "replacing" else self.T(slot[2] + one)
                return
        for slot in self.slots:
            if slot[2] == 0:
                slot[:] = [s, a, one]
                return
        lo = 0
        for i in range(1, self.K):
            if self.slots[i][2] < self.slots[lo][2]:
                lo = i
        self.slots[lo][:] = [s, a, one]

    def _sweep(self, u, terminated):
        q = self.algorithm.q_table
        wide = self.learn_mode == "vec" and q.dtype == np.float32
        for slot in self.slots:
            s, a, e = slot
            if e == 0:
                continue
            if wide:
                q[s, a] = np.float32(np.float64(q[s, a]) + np.float64(u) * np.float64(e))
            else:
                q[s, a] = self.T(q[s, a] + self.T(self.T(u) * e))
            slot[2] = self.T(0) if terminated else self.T(e * self.decay)

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
        s = int((states["observation"] if isinstance(states, dict) else states)[0])
        a = int(actions[0])
        with np.errstate(all="ignore"):
            if self.rule == "q_learning":
                row = self._valid_row(states)
                if not self.algorithm.q_table[s, a] == np.max(row):  # Watkins's cut (a NaN maximum is never equal)
                    self.clear()
        next_states, rewards, terminateds, truncateds, infos = env.step(actions)
        agent_rewards += rewards
        lr = self.lr_schedule.get_value()
        self.lr_schedule.update(1)
        self.exploration_rate_schedule.update(1)
        self.step_counter = (k + 1) & U64
        dtype = self.algorithm.q_table.dtype
        with np.errstate(all="ignore"):
            if self.rule == "sarsa":
                nxt = self._pick(next_states)  # draws of step k + 1, epsilon after this step's advance, row before the stores
                n = (next_states["observation"] if isinstance(next_states, dict) else next_states)[0]
                v = self.algorithm.q_table[n, nxt[0]]
                self.pending = int(nxt[0])
            else:
                row = self._valid_row(next_states)
                v = np.max(row) if row.size else dtype.type(-np.inf)
            terminated = bool(terminateds[0])
            u = self._increment(s, a, rewards[0], v, terminateds[0], lr)
            self._mark(s, a)
            self._sweep(u, terminated)
        if terminateds[0] or truncateds[0]:
            reward_history.append(agent_rewards[0])
            agent_rewards[0] = 0
        return next_states, infos


class TraceRun(TdRun):
    """``TdRun`` with eligibility traces: the same interface, plus the slots as the population's state dict holds them."""

    def __init__(self, env, rule, gamma, eps, lr, *, lam, K, kind="replacing", seed, dtype, mode="iter", agent_id=0, q0=None):
        self.env = env
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        if q0 is not None:
            algo.q_table[:] = q0
        self.rt = TraceRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, rule=rule, lam=lam, K=K,
                               kind=kind)
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    def reset(self):
        super().reset()
        self.rt.clear()

    @property
    def slots(self):
        """``(states, actions, values)``: the rows of ``state_dict["eligibility_traces"]`` for this run."""
        K = self.rt.K
        states, actions = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32)
        values = np.zeros(K, dtype=np.float64)
        for i, (s, a, e) in enumerate(self.rt.slots):
            if e != 0:
                states[i], actions[i], values[i] = s, a, np.float64(e)
        return states, actions, values
