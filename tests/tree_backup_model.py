"""NumPy model of the population's n-step Tree Backup (``QLearningPopulation(tree_backup=n)``, ``k_tree_rollout``):
Q-learning with a bootstrapping horizon, under a greedy target policy, for ONE agent.

Test infrastructure, like ``td_rules_model.py`` and ``n_step_model.py``, on which it is built: the pick, the valid row
and the update expression are ``TdRuntime``'s (rule ``q_learning``), the fold's target expression is ``NStepRuntime``'s.
DESIGN section 4.3c defines the step and this file restates it.  A run keeps a WINDOW of entries ``(s_i, a_i, r_i,
f_i)``, oldest first, at most ``n - 1`` of them between steps.  One step:

1. ``a`` is Q-learning's pick from the row as the previous step's stores left it; ``f = (Q[s, a] == np.max(Q[s,
   valid]))`` on that row (a NaN maximum is never equal);
2. the environment steps and ``(s, a, r, f)`` is appended: ``L <= n`` entries;
3. ``v = np.max(Q[s', valid])`` from the row of s' before any store of this step;
4. a terminated step updates every entry ``j = 0 .. L-1``, oldest first, and empties the window; otherwise ``L == n``
   updates entry 0 and pops it.  Entry ``j`` is ``_update(s_j, a_j, r_j, g_{j+1}, term_j, lr)`` -- the prediction is read
   from the table at that moment -- with ``g_L = v`` and, for ``j < i < L``: ``f_i``: ``g_i = T(target(r_i, g_{i+1},
   term_i))``; not ``f_i``: ``g_i = np.max(Q[s_i, valid(s_i)])`` read from the table at the moment of this update.  Only
   the nearest non-greedy entry ``c`` after ``j`` matters: the fold runs from ``c - 1`` (``L - 1`` without one) down to
   ``j + 1``.  The flag of entry ``j`` itself is not read.

The target policy is the deterministic greedy policy that, among tied maxima, takes the action the behaviour took.  With
``n = 1`` the step is ``TdRuntime``'s Q-learning; with every flag true it is ``NStepRuntime``'s fold with ``v`` the
maximum (tests/test_tree_backup_model.py).

``counts`` says which kinds of update a run performed (tests/tree_backup_cases.py asks every GPU case for all of them):
``steady_no_cut`` / ``steady_cut_next`` / ``steady_cut_deep`` -- the single update of a step that did not terminate,
without a non-greedy entry after entry 0, with one at ``i = 1``, with the nearest one at ``i > 1``; ``flush_cut`` /
``flush_no_cut`` -- an update of a terminated step with / without one after it (``flush_no_cut`` only where there is a
later entry at all); ``cut_own_state`` -- an update whose cut state is s' or ``s_j``; ``tie_pass`` -- a fold that passed
through an entry whose flag was set while another valid column tied with the action's.
"""

from __future__ import annotations

import numpy as np

from n_step_model import NStepRuntime
from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning
from td_rules_model import U64, TdRun, TdRuntime, oracle_schedule

KINDS = ("steady_no_cut", "steady_cut_next", "steady_cut_deep", "flush_cut", "flush_no_cut", "cut_own_state", "tie_pass")


class TreeBackupRuntime(TdRuntime):
    """``TdRuntime`` (Q-learning) with the Tree Backup horizon ``n``.  ``window``: the entries not yet updated, oldest
    first, each ``(s, a, r, f, mask, tie)`` -- ``mask`` the valid columns of ``s`` (None: all), ``tie`` whether ``f`` was
    set with more than one column at the maximum."""

    _target = NStepRuntime._target

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", n=1):
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode, "q_learning")
        assert n >= 1
        self.n = int(n)
        self.window = []
        self.counts = dict.fromkeys(KINDS, 0)

    def _row_max(self, s, mask):
        row = self.algorithm.q_table[s]
        row = row if mask is None else row[np.where(mask)]
        return np.max(row) if row.size else self.algorithm.q_table.dtype.type(-np.inf)

    def run_single_step(self, env, states, agent_rewards, reward_history):
        k = self.step_counter
        q = self.algorithm.q_table
        actions = self._pick(states)
        s = int((states["observation"] if isinstance(states, dict) else states)[0])
        mask = states["action_mask"][0].copy() if isinstance(states, dict) else None
        with np.errstate(all="ignore"):
            top = self._row_max(s, mask)
            greedy = bool(q[s, actions[0]] == top)
            seen = q[s] if mask is None else q[s][np.where(mask)]
            tie = greedy and int(np.count_nonzero(seen == top)) > 1
        if self.trace is not None:
            self.trace.append((actions.copy(), self.exploration_rate_schedule.get_value(), self.lr_schedule.get_value()))
        if hasattr(env, "step_index"):
            env.step_index = k
        next_states, rewards, terminateds, truncateds, infos = env.step(actions)
        agent_rewards += rewards
        lr = self.lr_schedule.get_value()
        self.lr_schedule.update(1)
        self.exploration_rate_schedule.update(1)
        self.step_counter = (k + 1) & U64
        dtype = q.dtype
        self.window.append((s, int(actions[0]), rewards[0], greedy, mask, tie))
        n_obs = int((next_states["observation"] if isinstance(next_states, dict) else next_states)[0])
        with np.errstate(all="ignore"):
            row = self._valid_row(next_states)
            v = np.max(row) if row.size else dtype.type(-np.inf)
            terminated = bool(terminateds[0])
            L = len(self.window)
            updates = L if terminated else (1 if L == self.n else 0)
            for j in range(updates):
                cut = next((i for i in range(j + 1, L) if not self.window[i][3]), None)
                s_j, a_j, r_j = self.window[j][:3]
                if cut is None:
                    g, start = v, L - 1
                else:
                    g, start = self._row_max(self.window[cut][0], self.window[cut][4]), cut - 1
                for i in range(start, j, -1):
                    g = self._target(self.window[i][2], g, terminated and i == L - 1)
                self._count(j, L, cut, start, terminated, s_j, n_obs)
                self._update(s_j, a_j, r_j, g, terminated and j == L - 1, lr)
            if terminated:
                self.window.clear()
            elif updates:
                self.window.pop(0)
        if terminateds[0] or truncateds[0]:
            reward_history.append(agent_rewards[0])
            agent_rewards[0] = 0
        return next_states, infos

    def _count(self, j, L, cut, start, terminated, s_j, n_obs):
        c = self.counts
        if terminated:
            if cut is not None:
                c["flush_cut"] += 1
            elif L - 1 > j:
                c["flush_no_cut"] += 1
        elif cut is None:
            c["steady_no_cut"] += L - 1 > j
        else:
            c["steady_cut_next" if cut == j + 1 else "steady_cut_deep"] += 1
        if cut is not None and self.window[cut][0] in (s_j, n_obs):
            c["cut_own_state"] += 1
        c["tie_pass"] += any(self.window[i][5] for i in range(start, j, -1))


class TreeBackupRun(TdRun):
    """``TdRun`` under Tree Backup: the same interface, plus the window as the population's state dict holds it and the
    counters of the update kinds."""

    def __init__(self, env, gamma, eps, lr, *, n, seed, dtype, mode="iter", agent_id=0, q0=None):
        self.env = env
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        if q0 is not None:
            algo.q_table[:] = q0
        self.rt = TreeBackupRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, n=n)
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    def reset(self):
        super().reset()
        self.rt.window.clear()  # the dropped entries are never updated

    @property
    def counts(self):
        return self.rt.counts

    @property
    def window(self):
        """``(length, states, actions, rewards, greedy)``: the rows of ``state_dict["tree_backup_window"]`` for this run."""
        w = max(self.rt.n - 1, 0)
        states, actions = np.zeros(w, dtype=np.int32), np.zeros(w, dtype=np.int32)
        rewards, greedy = np.zeros(w, dtype=np.float32), np.zeros(w, dtype=np.uint8)
        for i, (s, a, r, f, _, _) in enumerate(self.rt.window):
            states[i], actions[i], rewards[i], greedy[i] = s, a, r, f
        return len(self.rt.window), states, actions, rewards, greedy
