"""NumPy model of the population's visit counts (``QLearningPopulation(exploration_bonus=..., visit_lr=...)``,
``k_visit_rollout``) for ONE agent.

Test infrastructure, like ``dyna_model.py``, built on ``td_rules_model.py``: the valid row, the environment step and the
update are ``TdRuntime``'s with rule ``q_learning``, and the selection is the oracle's own ``_pick``.  DESIGN section 4.3c
defines the step and this file restates it.  A run keeps ``N``, a uint32 ``[S, A]`` array, zero at creation, and one
``beta``, a float64.  With ``T`` the table dtype

    bonus(beta, N) = T(0)                                 when beta == 0
                   = T(beta / sqrt(float64(N)))           otherwise: float64 sqrt and division, one rounding to T;
                                                          N == 0 gives +inf by IEEE division

and one training step with draw counter ``k`` is ``TdRuntime.run_single_step`` with three changes:

1. pick: the oracle's selection (same draws, same dispatcher variant) runs while row ``s`` of the table temporarily holds
   the score row ``Q[s, :] + bonus(beta, N[s, :])`` -- one add in ``T`` per column; the oracle itself masks the invalid
   columns --, then the row is restored: the prediction of the update is ``Q[s, a]``;
2. count: after the environment step and before the update ``N[s, a]`` becomes ``N[s, a] + 1``, saturating at 2^32 - 1;
3. rate: with ``visit_lr`` the update takes ``lr_k / float64(N[s, a])`` (the incremented count, a float64 division; the
   float32 update rounds it to float as it rounds ``lr_k``); without, ``lr_k``.

The target ``np.max(Q[s', valid])`` is taken on plain Q.
"""

from __future__ import annotations

import numpy as np

from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning
from td_rules_model import TdRun, TdRuntime, oracle_schedule

VISIT_MAX = 2 ** 32 - 1


def bonus(beta, counts, dtype):
    """``bonus(beta, N)`` of every cell of the uint32 array ``counts`` in the table dtype."""
    counts = np.asarray(counts, dtype=np.uint32)
    if beta == 0:
        return np.zeros(counts.shape, dtype=dtype)
    with np.errstate(all="ignore"):
        return (np.float64(beta) / np.sqrt(counts.astype(np.float64))).astype(dtype)


class VisitRuntime(TdRuntime):
    """``TdRuntime`` (rule ``q_learning``) with visit counts."""

    def __init__(self, algorithm, lr_schedule, exploration_rate_schedule, learn_mode="iter", beta=0.0, visit_lr=False):
        super().__init__(algorithm, lr_schedule, exploration_rate_schedule, learn_mode, "q_learning")
        assert np.isfinite(beta) and beta >= 0
        self.beta = float(beta)
        self.visit_lr = bool(visit_lr)
        self.counts = np.zeros(algorithm.q_table.shape, dtype=np.uint32)

    def _pick(self, states):
        q = self.algorithm.q_table
        s = int((states["observation"] if isinstance(states, dict) else states)[0])
        kept = q[s].copy()
        with np.errstate(all="ignore"):
            q[s] = kept + bonus(self.beta, self.counts[s], q.dtype)  # one add in T; -inf + inf is a NaN like any other
        try:
            return super()._pick(states)
        finally:
            q[s] = kept

    def _update(self, s, a, reward, v, terminated, lr):
        n = int(self.counts[s, a])
        n = n if n == VISIT_MAX else n + 1
        self.counts[s, a] = n
        if self.visit_lr:
            lr = float(np.float64(lr) / np.float64(n))  # (a Python float, as lr_k is: the float32 update rounds it once)
        super()._update(s, a, reward, v, terminated, lr)


class VisitRun(TdRun):
    """``TdRun`` with visit counts: the same interface, plus ``counts`` and ``bonus``."""

    def __init__(self, env, gamma, eps, lr, *, beta, visit_lr, seed, dtype, mode="iter", agent_id=0, q0=None, n0=None):
        self.env = env
        ids = getattr(env, "agent_ids", None)
        ids = np.array([agent_id], dtype=np.uint32) if ids is None else ids
        algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dtype))
        algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=ids)
        if q0 is not None:
            algo.q_table[:] = q0
        self.rt = VisitRuntime(algo, oracle_schedule(lr), oracle_schedule(eps), learn_mode=mode, beta=beta, visit_lr=visit_lr)
        if n0 is not None:
            self.rt.counts[:] = n0
        self.states = None
        self.acc = np.zeros(1, dtype=np.float32)

    @property
    def counts(self):
        return self.rt.counts

    @property
    def bonus(self):
        return bonus(self.rt.beta, self.rt.counts, self.q.dtype)
