"""NumPy model of the population's n-step on-policy rules (``QLearningPopulation(update_rule=..., n_step=n)``,
``k_nstep_rollout``): n-step SARSA and n-step Expected SARSA for ONE agent.

Test infrastructure, like ``td_rules_model.py``, on which it is built: the pick, the valid row, Expected SARSA's value
and the update expressions are ``TdRuntime``'s.  DESIGN section 4.3c defines the step and this file restates it.  A run
keeps a WINDOW of transitions ``(s_i, a_i, r_i)``, oldest first, at most ``n - 1`` of them between steps.  One step:

1. the action is the 1-step rule's (SARSA: the pending action, else a pick; Expected SARSA: a pick);
2. the environment steps and ``(s, a, r)`` is appended: ``L <= n`` entries;
3. ``v`` is the 1-step rule's bootstrap scalar, from the row of s' before any store of this step (SARSA picks a' here);
4. a terminated step updates every entry ``j = 0 .. L-1``, oldest first, and empties the window; otherwise ``L == n``
   updates entry 0 and pops it.  Entry ``j`` is ``_update(s_j, a_j, r_j, g_{j+1}, term_j, lr)`` -- the prediction is
   read from the table at that moment -- with ``g_L = v`` and ``g_i = T(target(r_i, g_{i+1}, term_i))`` for
   ``i = L-1`` down to ``j+1``; ``target`` is the target expression of ``_update``, ``T`` rounds to the table dtype and
   ``term_i`` is true only for ``i = L-1`` of a terminated step.

With ``n = 1`` the window holds the step's own transition alone, ``g_1 = v``, and the step is ``TdRuntime``'s
(tests/test_n_step_model.py).
"""

from __future__ import annotations

import numpy as np

from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning
from td_rules_model import U64, TdRun, TdRuntime, expected_value, oracle_schedule

N_STEP_RULES = ("sarsa", "expected_sarsa")


class NStepRuntime(TdRuntime):
    """``TdRuntime`` with the horizon ``n``.  ``window``: the transitions not yet updated, oldest first."""

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", rule="sarsa", n=1):
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode, rule)
        assert rule in N_STEP_RULES and n >= 1
        self.n = int(n)
        self.window = []

    def _target(self, reward, g, terminated):
        """The target of ``_update`` for (reward, bootstrap scalar g, terminated), rounded to the table dtype."""
        algo = self.algorithm
        dtype = algo.q_table.dtype
        if self.learn_mode == "iter":
            nxt = 0 if terminated else g
            target = reward + algo.discount_factor * nxt
            return dtype.type(target)
        rewards, term = np.array([reward]), np.array([terminated])
        maxima = np.array([g], dtype=dtype)
        targets = rewards + algo.discount_factor * maxima * (1 - term)
        return dtype.type(targets[0])

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
        self.window.append((int(s), int(actions[0]), rewards[0]))
        with np.errstate(all="ignore"):
            if self.rule == "sarsa":
                nxt = self._pick(next_states)  # draws of step k + 1, epsilon after this step's advance, row before the stores
                n = (next_states["observation"] if isinstance(next_states, dict) else next_states)[0]
                v = self.algorithm.q_table[n, nxt[0]]
                self.pending = int(nxt[0])
            else:
                v = expected_value(self._valid_row(next_states), self.exploration_rate_schedule.get_value(), dtype)
            terminated = bool(terminateds[0])
            L = len(self.window)
            updates = L if terminated else (1 if L == self.n else 0)
            for j in range(updates):
                g = v
                for i in range(L - 1, j, -1):
                    g = self._target(self.window[i][2], g, terminated and i == L - 1)
                s_j, a_j, r_j = self.window[j]
                self._update(s_j, a_j, r_j, g, terminated and j == L - 1, lr)
            if terminated:
                self.window.clear()
            elif updates:
                self.window.pop(0)
        if terminateds[0] or truncateds[0]:
            reward_history.append(agent_rewards[0])
            agent_rewards[0] = 0
        return next_states, infos


class NStepRun(TdRun):
    """``TdRun`` under an n-step rule: the same interface, plus the window as the population's state dict holds it."""

    def __init__(self, env, rule, gamma, eps, lr, *, n, seed, dtype, mode="iter", agent_id=0, q0=None):
        self.env = env
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        if q0 is not None:
            algo.q_table[:] = q0
        self.rt = NStepRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, rule=rule, n=n)
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    def reset(self):
        super().reset()
        self.rt.window.clear()  # the dropped entries are never updated

    @property
    def window(self):
        """``(length, states, actions, rewards)``: the rows of ``state_dict["n_step_window"]`` for this run."""
        w = max(self.rt.n - 1, 0)
        states, actions = np.zeros(w, dtype=np.int32), np.zeros(w, dtype=np.int32)
        rewards = np.zeros(w, dtype=np.float32)
        for i, (s, a, r) in enumerate(self.rt.window):
            states[i], actions[i], rewards[i] = s, a, r
        return len(self.rt.window), states, actions, rewards
