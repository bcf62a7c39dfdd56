"""NumPy model of the population's prioritized sweeping (``QLearningPopulation(planning_steps=n,
planning_order="prioritized")``, ``k_sweep_rollout``) for ONE agent.

Test infrastructure, built on ``dyna_model.py``: the pick, the valid row, the environment step, the update, the model and
the visited list are ``DynaRuntime``'s.  DESIGN section 4.3c defines the step and this file restates it.  Beside the
model a run keeps

* the predecessor lists: ``lists[x]`` holds the seen cells whose model entry is ``(x, ., terminated = 0)``, most recently
  linked first (Python lists, head at index 0);
* the queue: ``K`` slots ``(cell, priority)``; a free slot is ``(-1, 0.0)``.

Notation.  ``inc(c, rho, m, tau)`` is the increment the update of ``(Q[c], rho, m, tau)`` adds to the cell with the
learning rate of the step (``_increment``: of the table dtype in ``iter`` mode; in ``vec`` mode the float64 increment
``np.add.at`` receives, which on a float32 table is rounded only with the sum).  ``P(u) = abs(float64(u))``.
``rowmax(p)`` is ``np.max(Q[p, valid(p)])`` as the table stands now (a valid NaN: NaN; no valid column: -inf).

One training step with draw counter ``k``:

1. Q-learning's step, exactly ``DynaRuntime``'s step 1; ``u0`` is its increment;
2. learn: ``old = model[s, a]``; an unseen cell is appended to the visited list; if ``old`` was linked (seen, not
   terminated) and ``old.next != s'`` or the new outcome is terminated, the cell is removed from ``lists[old.next]`` (the
   others keep their order); ``model[s, a] = (s', r, terminated)``; if the new outcome is not terminated and the cell is
   not linked now, it goes to the head of ``lists[s']``; a cell whose next state and flag did not change keeps its place;
3. if ``P(u0) > theta``: ``propagate(s)``;
4. plan, ``i = 0 .. n-1``: if the queue is empty, stop; ``c = pop()``; ``(p, rho, tau) = model[c]`` as it stands now;
   ``m = rowmax(p)``; ``Q[c] = update(...)`` with ``lr_k``, increment ``u_i``; if ``P(u_i) > theta``: ``propagate(c // A)``.

``propagate(x)``: ``m_x = rowmax(x)`` after the store just made; for each cell ``d`` of ``lists[x]``, head to tail:
``u = inc(d, model[d].reward, m_x, False)``, nothing is stored; if ``P(u) > theta``: ``insert(d, P(u))``.

``insert(c, P)``: a live slot that holds ``c`` keeps ``max(old, P)``; else ``c`` goes into the lowest free slot; else the
slot of the smallest priority (lowest index among equals) is replaced if ``P`` is strictly greater, and the newcomer is
dropped if it is not.  ``pop()``: the slot of the largest priority, lowest index among equals; it becomes free.

No draw is consumed; a NaN increment never passes ``P > theta``.  ``events`` counts what happened, for
tests/test_sweep_cases.py; it has no part in the rule.  ``skip_planning`` (``DynaRuntime``'s hook) skips steps 3 and 4.

The census beside the branches of the rule (``events``; none of it feeds back):

* ``pop_tie``: a pop with at least two live slots at the largest priority; ``pop_inf``: the popped priority is infinite;
* ``evict_tie``: an eviction with at least two slots at the smallest priority; ``dropped_equal``: a dropped newcomer whose
  priority equals the smallest; ``insert_hole``: an insert into a free slot that lies below a live one;
* ``unlink_head`` / ``unlink_tail``: the unlinked cell was the head / the last node of a list of two or more
  (``unlink_inner``, as before: neither the head, in a list of three or more);
* ``propagate_held`` / ``propagate_other``: ``propagate(x)`` with ``x`` the next observation, whose row the kernel holds
  in registers, or another state;
* ``threshold_equal_step`` / ``_plan`` / ``_propagate``: ``P == theta > 0`` at the comparison of step 3, of step 4 or of
  ``propagate``; ``smallest_compared`` is the smallest non-zero priority (not NaN) any of the three sites has compared;
* ``rowmax_hidden_nan`` / ``rowmax_valid_nan``: ``rowmax(p)`` of a row with a NaN in invalid columns only / in a valid one;
* ``held_row_turns_nan``: a planning store puts the first NaN into the valid columns of the row of the next observation
  (the kernel recomputes the NaN flag of the row it holds in registers).
"""

from __future__ import annotations

from collections import Counter

import numpy as np

from dyna_model import DynaRun, DynaRuntime, _mask_function, _Recording
from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning
from td_rules_model import oracle_schedule

QUEUE_MAX = 32


class SweepRuntime(DynaRuntime):
    """``DynaRuntime`` whose ``n`` planning updates per step are taken from a priority queue."""

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", n=1, K=16, theta=0.0, agent_id=0,
                 mask_of=None):
        assert 0 < K <= QUEUE_MAX and theta >= 0.0 and np.isfinite(theta)
        self.K = int(K)
        self.theta = float(theta)
        self.events = Counter()
        self.flag_flips = Counter()  # (cell, new flag) -> how often the cell's terminated flag changed to it
        self.smallest_compared = np.inf
        self.held = -1
        self._cols = {}
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode, n=n, agent_id=agent_id, mask_of=mask_of)

    def forget(self):
        super().forget()
        self.lists = {}  # state -> its predecessor cells, head first
        self.empty_queue()

    def empty_queue(self):
        self.cells = [-1] * self.K
        self.priorities = [0.0] * self.K

    # ---- the quantities of the definition ------------------------------------------------------------------------------------
    def _increment(self, s, a, reward, v, terminated, lr):
        """What ``_update(s, a, reward, v, terminated, lr)`` would add to the cell, operation for operation; nothing is
        stored."""
        algo = self.algorithm
        if self.learn_mode == "iter":
            nxt = 0 if terminated else v
            target = reward + algo.discount_factor * nxt
            prediction = algo.get_q_value(s, a)
            return lr * (target - prediction)
        states, actions = np.array([s]), np.array([a])
        rewards, term = np.array([reward]), np.array([terminated])
        maxima = np.array([v], dtype=algo.q_table.dtype)
        targets = rewards + algo.discount_factor * maxima * (1 - term)
        return (lr * (targets - algo.q_table[states, actions]))[0]

    @staticmethod
    def _priority(u):
        return abs(float(np.float64(u)))

    def _valid_cells_of(self, p):
        q = self.algorithm.q_table
        if self.mask_of is None:
            return q[p]
        if p not in self._cols:  # (the valid columns are a function of the observation alone: dyna_model.py)
            self._cols[p] = self.mask_of(p)
        return q[p][self._cols[p]]

    def _rowmax(self, p):
        q = self.algorithm.q_table
        row = self._valid_cells_of(p)
        if np.isnan(row).any():
            self.events["rowmax_valid_nan"] += 1
        elif np.isnan(q[p]).any():
            self.events["rowmax_hidden_nan"] += 1
        return np.max(row) if row.size else q.dtype.type(-np.inf)

    def _passes(self, P, site):
        """``P > theta`` of the named site, counted."""
        if P == self.theta > 0:
            self.events["threshold_equal_" + site] += 1
        if 0 < P < self.smallest_compared:
            self.smallest_compared = P
        return P > self.theta

    def _update(self, s, a, reward, v, terminated, lr):
        self.last_priority = self._priority(self._increment(s, a, reward, v, terminated, lr))
        super()._update(s, a, reward, v, terminated, lr)

    # ---- the queue ------------------------------------------------------------------------------------------------------------
    def insert(self, c, P):
        ev = self.events
        if c in self.cells:
            i = self.cells.index(c)
            if P > self.priorities[i]:
                self.priorities[i] = P
                ev["insert_raises"] += 1
            else:
                ev["insert_keeps" if self.priorities[i] > P else "insert_equal"] += 1
            return
        if -1 in self.cells:
            i = self.cells.index(-1)
            ev["insert_free"] += 1
            if any(c2 >= 0 for c2 in self.cells[i + 1:]):
                ev["insert_hole"] += 1
        else:
            i = int(np.argmin(self.priorities))  # (the first of the smallest)
            if not P > self.priorities[i]:
                ev["dropped"] += 1
                if P == self.priorities[i]:
                    ev["dropped_equal"] += 1
                return
            ev["evicted"] += 1
            if self.priorities.count(self.priorities[i]) >= 2:
                ev["evict_tie"] += 1
        self.cells[i], self.priorities[i] = c, P

    def pop(self):
        live = [i for i in range(self.K) if self.cells[i] >= 0]
        if not live:
            return -1
        i = max(live, key=lambda j: (self.priorities[j], -j))
        if sum(self.priorities[j] == self.priorities[i] for j in live) >= 2:
            self.events["pop_tie"] += 1
        if np.isinf(self.priorities[i]):
            self.events["pop_inf"] += 1
        c = self.cells[i]
        self.cells[i], self.priorities[i] = -1, 0.0
        return c

    def propagate(self, x, lr):
        A = self.algorithm.q_table.shape[1]
        m = self._rowmax(x)
        self.events["propagate_held" if x == self.held else "propagate_other"] += 1
        inserted = 0
        for d in list(self.lists.get(x, ())):
            u = self._increment(d // A, d % A, self.model[d][1], m, False, lr)
            P = self._priority(u)
            if P != P:
                self.events["nan_not_queued"] += 1
            if self._passes(P, "propagate"):
                self.insert(d, P)
                inserted += 1
            if d // A == x:
                self.events["self_loop"] += 1
        self.events["propagate_none" if not inserted else "propagate_some"] += 1

    def _pick(self, states):
        actions = super()._pick(states)
        s = int((states["observation"] if isinstance(states, dict) else states)[0])
        self.old_entry = self.model.get(s * self.algorithm.q_table.shape[1] + int(actions[0]))  # model[s, a] before the step
        return actions

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    def run_single_step(self, env, states, agent_rewards, reward_history):
        A = self.algorithm.q_table.shape[1]
        s = int((states["observation"] if isinstance(states, dict) else states)[0])
        lr = self.lr_schedule.get_value()
        skip, self.skip_planning = self.skip_planning, True  # (DynaRuntime's own steps 1 and 2 alone: its plan is not ours)
        try:
            next_states, infos = super().run_single_step(env, states, agent_rewards, reward_history)
        finally:
            self.skip_planning = skip
        P0 = self.last_priority
        cell = s * A + self.last_action
        # 2. the predecessor lists follow the model
        old = self.old_entry
        n, _, terminated = self.model[cell]
        was_linked = old is not None and not old[2]
        stays = was_linked and not terminated and old[0] == n
        if was_linked and not stays:
            lst = self.lists[old[0]]
            if len(lst) >= 3 and lst[0] != cell:
                self.events["unlink_inner"] += 1
            if lst[0] == cell:
                self.events["unlink_head"] += 1
            elif lst[-1] == cell:
                self.events["unlink_tail"] += 1
            lst.remove(cell)
            self.events["unlinked"] += 1
        if not terminated and not stays:
            self.lists.setdefault(n, []).insert(0, cell)
        if old is not None and old[2] != terminated:
            self.events["flag_on" if terminated else "flag_off"] += 1
            self.flag_flips[(cell, bool(terminated))] += 1
        if self.skip_planning:
            return next_states, infos
        self.held = held = int((next_states["observation"] if isinstance(next_states, dict) else next_states)[0])
        with np.errstate(all="ignore"):
            # 3. the real step's own change reaches its predecessors
            if self._passes(P0, "step"):
                self.propagate(s, lr)
            # 4. planning
            used = 0
            for _ in range(self.n):
                c = self.pop()
                if c < 0:
                    self.events["queue_ran_empty" if used else "queue_was_empty"] += 1
                    break
                used += 1
                p, rho, tau = self.model[c]
                m = self._rowmax(p)
                clean = c // A == held and not np.isnan(self._valid_cells_of(held)).any()
                self._update(c // A, c % A, rho, m, tau, lr)
                if c // A == held:
                    self.events["patched_held_row"] += 1
                    if clean and np.isnan(self._valid_cells_of(held)).any():
                        self.events["held_row_turns_nan"] += 1
                if self._passes(self.last_priority, "plan"):
                    self.propagate(c // A, lr)
            else:
                self.events["all_pops_used"] += 1
        return next_states, infos


class SweepRun(DynaRun):
    """``DynaRun`` with prioritized sweeping: the same interface, plus the lists and the queue as ``planning_model`` and
    ``sweep_queue`` hold them for this run."""

    def __init__(self, env, gamma, eps, lr, *, n, K, theta, seed, dtype, mode="iter", agent_id=0, q0=None):
        self.env = _Recording(env)
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        if q0 is not None:
            algo.q_table[:] = q0
        self.rt = SweepRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, n=n, K=K, theta=theta,
                               agent_id=int(ids[0]), mask_of=_mask_function(env))
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    @property
    def predecessors(self):
        """``(pred_head [S], pred_next [S, A])`` of this run."""
        S, A = self.rt.algorithm.q_table.shape
        head = np.full(S, -1, dtype=np.int32)
        nxt = np.full(S * A, -1, dtype=np.int32)
        for x, lst in self.rt.lists.items():
            if lst:
                head[x] = lst[0]
                nxt[lst[:-1]] = lst[1:]
        return head, nxt.reshape(S, A)

    @property
    def sweep_queue(self):
        """``(cells [K], priorities [K])`` of this run."""
        return np.array(self.rt.cells, dtype=np.int32), np.array(self.rt.priorities, dtype=np.float64)


def canonical_lists(next_states, terminated, visited, count):
    """``(pred_head [S], pred_next [S, A])`` of one run's 5-key model in the canonical order: its seen cells with
    ``terminated == 0`` linked in visited-list order, each at the head of its next state's list."""
    S, A = next_states.shape
    head = np.full(S, -1, dtype=np.int32)
    nxt = np.full(S * A, -1, dtype=np.int32)
    for c in visited[:count]:
        if not terminated.ravel()[c]:
            x = next_states.ravel()[c]
            nxt[c] = head[x]
            head[x] = c
    return head, nxt.reshape(S, A)
