"""NumPy model of the population's Dyna-Q (``QLearningPopulation(planning_steps=n)``, ``k_dyna_rollout``) for ONE agent.

Test infrastructure, like ``trace_model.py``, built on ``td_rules_model.py``: the pick, the valid row, the environment
step and the update are ``TdRuntime``'s with rule ``q_learning``.  DESIGN section 4.3c defines the step and this file
restates it.  A run keeps

* the model: for every cell ``c = s * A + a`` its last observed outcome ``(next_obs, reward float32, terminated)``, or
  nothing while the cell is unseen;
* the visited list: the seen cells in order of first observation; ``count`` is its length.

One training step with draw counter ``k``:

1. Q-learning's step, exactly ``TdRuntime.run_single_step``: pick ``a`` from the row of ``s``, step the environment to
   ``(s', r, terminated)`` (``s'`` is the observation it returns, already reset after a terminated step),
   ``m = np.max(Q[s', valid])`` before the store, ``Q[s, a] = update(...)`` with ``lr_k``; the schedules advance;
2. learn: an unseen ``(s, a)`` is appended to the list; ``model[s, a] = (s', r, terminated)`` (a later outcome overwrites);
3. plan, ``i = 0 .. n-1`` in order: ``x_i`` = word ``i & 3`` of the Philox block ``(agent_id, k_lo, k_hi,
   STREAM_PLAN | (i >> 2) << 8)`` under the seed key; ``j = mulhi32(x_i, count)``; ``c_i = visited[j]``;
   ``(p, rho, tau) = model[c_i]``; ``m_i = np.max(Q[p, valid(p)])`` as the table stands now (-inf over an empty valid set);
   ``Q[c_i] = update(Q[c_i], rho, m_i, tau, lr_k)``.  The row of ``p`` is read even when ``tau`` is set.

The valid columns of a remembered next state ``p`` are a function of the observation alone in every environment the
engine has; the model asks the oracle environment for them (``action_masks``).  ``skip_planning`` is a hook of this
model alone: the planning loop is skipped while the model and the list are still kept (tests/test_dyna_model.py anchors
the rest of the step to ``TdRun`` with it).
"""

from __future__ import annotations

import numpy as np

from oracle.draws import InjectedDraws, mulhi32, philox4x32
from oracle.qlearn_oracle import OracleQLearning
from td_rules_model import TdRun, TdRuntime, oracle_schedule

STREAM_PLAN = 2
PLANNING_MAX = 64


class DynaRuntime(TdRuntime):
    """``TdRuntime`` (rule ``q_learning``) with a learned model and ``n`` planning updates per step."""

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", n=1, agent_id=0, mask_of=None):
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode, "q_learning")
        assert 0 < n <= PLANNING_MAX
        self.n = int(n)
        self.agent_id = int(agent_id)
        self.mask_of = mask_of  # obs -> valid columns or None
        self.skip_planning = False
        self.forget()

    def forget(self):
        self.model = {}     # cell -> (next_obs, float32 reward, terminated)
        self.visited = []   # cells in order of first observation

    def plan_draws(self, k):
        """x_0 .. x_{n-1} of the step with draw counter ``k``."""
        seed = self.algorithm._rng.seed
        blocks = np.arange((self.n + 3) // 4, dtype=np.uint64)
        x = philox4x32(self.agent_id, k & 0xFFFFFFFF, (k >> 32) & 0xFFFFFFFF, STREAM_PLAN | (blocks << np.uint64(8)), seed, seed >> 32)
        return [int(w) for w in np.stack(x, axis=1).ravel()[:self.n]]  # block-major: word i & 3 of block i >> 2

    def _pick(self, states):
        actions = super()._pick(states)
        self.last_action = int(actions[0])
        return actions

    def run_single_step(self, env, states, agent_rewards, reward_history):
        k = self.step_counter
        A = self.algorithm.q_table.shape[1]
        s = int((states["observation"] if isinstance(states, dict) else states)[0])
        lr = self.lr_schedule.get_value()
        next_states, infos = super().run_single_step(env, states, agent_rewards, reward_history)  # 1. Q-learning's step
        a = self.last_action
        n = int((next_states["observation"] if isinstance(next_states, dict) else next_states)[0])
        reward, terminated = env.last_reward, env.last_terminated  # (kept by _Recording: TdRuntime does not hand them out)
        # 2. learn
        cell = s * A + a
        if cell not in self.model:
            self.visited.append(cell)
        self.model[cell] = (n, np.float32(reward), bool(terminated))
        # 3. plan
        if self.skip_planning:
            return next_states, infos
        q = self.algorithm.q_table
        dtype = q.dtype
        with np.errstate(all="ignore"):
            for x in self.plan_draws(k):
                c = self.visited[int(mulhi32(x, len(self.visited)))]
                p, rho, tau = self.model[c]
                cols = None if self.mask_of is None else self.mask_of(p)
                row = q[p] if cols is None else q[p][cols]
                m = np.max(row) if row.size else dtype.type(-np.inf)
                self._update(c // A, c % A, rho, m, tau, lr)
        return next_states, infos


class _Recording:
    """A one-agent oracle environment that remembers the reward and the flag of its latest step; everything else is the
    wrapped environment's."""

    def __init__(self, env):
        object.__setattr__(self, "_env", env)
        object.__setattr__(self, "last_reward", np.float32(0))
        object.__setattr__(self, "last_terminated", False)

    def __getattr__(self, name):
        return getattr(self._env, name)

    def __setattr__(self, name, value):
        if name in ("last_reward", "last_terminated"):
            object.__setattr__(self, name, value)
        else:
            setattr(self._env, name, value)

    def step(self, actions):
        out = self._env.step(actions)
        self.last_reward = np.float32(out[1][0])
        self.last_terminated = bool(out[2][0])
        return out


def _mask_function(env):
    """obs -> valid columns (ascending) of the row of ``obs``, or None for an environment without masks."""
    if not env.masked:
        return None
    return lambda obs: np.flatnonzero(env.action_masks(np.array([obs]))[0])


class DynaRun(TdRun):
    """``TdRun`` with Dyna-Q: the same interface, plus the model as ``planning_model`` holds it for this run."""

    def __init__(self, env, gamma, eps, lr, *, n, seed, dtype, mode="iter", agent_id=0, q0=None):
        self.env = _Recording(env)
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        if q0 is not None:
            algo.q_table[:] = q0
        self.rt = DynaRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, n=n, agent_id=int(ids[0]),
                              mask_of=_mask_function(env))
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    @property
    def planning_model(self):
        """``(next_states [S, A], rewards [S, A], terminated [S, A], visited [S * A], count)`` of this run."""
        S, A = self.rt.algorithm.q_table.shape
        nxt = np.full(S * A, -1, dtype=np.int32)
        rew = np.zeros(S * A, dtype=np.float32)
        term = np.zeros(S * A, dtype=bool)
        for c, (p, rho, tau) in self.rt.model.items():
            nxt[c], rew[c], term[c] = p, rho, tau
        visited = np.full(S * A, -1, dtype=np.int32)
        visited[:len(self.rt.visited)] = self.rt.visited
        return nxt.reshape(S, A), rew.reshape(S, A), term.reshape(S, A), visited, len(self.rt.visited)
