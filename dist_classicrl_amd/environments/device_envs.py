"""Batched tabular environments whose state lives on the GPU next to the Q-table.

They follow the reference's vector-env contract as realised by
``SyncVectorEnv(autoreset_mode=SAME_STEP)`` (``benchmarks/throughput_benchmark.py:109-123``):

    reset(seed=None, options=None) -> (obs | {"observation", "action_mask"}, infos)
    step(actions) -> (obs, rewards float32[n], terminated bool[n], truncated bool[n], infos)

so the generic host-driven loop of ``BaseRuntime`` works with them, but their point is the fused
path: ``GpuRolloutQLearning.run_steps`` keeps select -> env.step -> learn on the device
(``qe_rollout``).  An environment must be bound to the algorithm whose GPU it shares
(:meth:`DeviceVecEnv.bind`; the runtimes do that themselves).
"""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from dist_classicrl_amd import _lib


class DeviceVecEnv:
    kind = -1
    masked = False

    def __init__(self, num_agents: int, state_size: int, action_size: int, params: _lib.EnvParams):
        self.num_agents = int(num_agents)
        self.state_size = int(state_size)
        self.action_size = int(action_size)
        self._params = params
        self._h = C.c_void_p()
        self._algo = None
        self._lib = None
        self._resident = None  # (states array, rewards array) of the state dict that mirrors the device
        self._chunk_limits = {}

    def __len__(self) -> int:
        return self.num_agents

    def __del__(self):
        self.close()

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value and self._lib is not None:
            self._lib.qe_env_destroy(h)
            self._h = C.c_void_p()

    @property
    def handle(self):
        return self._h

    def bind(self, algorithm) -> "DeviceVecEnv":
        """Create the device state on ``algorithm``'s GPU/stream (idempotent per algorithm)."""
        if self._algo is algorithm and self._h.value:
            return self
        if (algorithm.state_size, algorithm.action_size) != (self.state_size, self.action_size):
            msg = (
                f"environment is {self.state_size} states x {self.action_size} actions but the "
                f"algorithm's table is {algorithm.state_size} x {algorithm.action_size}"
            )
            raise ValueError(msg)
        self.close()
        self._resident = None
        self._chunk_limits = {}
        self._lib = _lib.load()
        self._create(algorithm)
        self._algo = algorithm
        return self

    def _create(self, algorithm) -> None:
        _lib.check(self._lib.qe_env_create(C.byref(self._h), algorithm.handle, self.num_agents,
                                           C.byref(self._params)))

    def _need(self):
        if not self._h.value:
            msg = "device environment is not bound: call env.bind(algorithm) first"
            raise RuntimeError(msg)

    def _wrap(self, obs, masks):
        if self.masked:
            return {"observation": obs, "action_mask": masks.view(np.int8)}
        return obs

    def observe(self):
        """(observations, running per-agent episode returns) as host arrays."""
        self._need()
        obs = np.empty(self.num_agents, dtype=np.int32)
        acc = np.empty(self.num_agents, dtype=np.float32)
        masks = np.empty((self.num_agents, self.action_size), dtype=np.uint8) if self.masked else None
        _lib.check(self._lib.qe_env_observe(self._h, _lib.ptr(obs, C.c_int32), _lib.ptr(masks, C.c_uint8),
                                            _lib.ptr(acc, C.c_float)))
        return self._wrap(obs, masks), acc

    def aux(self) -> np.ndarray:
        """Environment-internal per-agent state (episode counters, board marks): what an exact resume
        needs besides observations and running returns."""
        self._need()
        out = np.empty(self.num_agents, dtype=np.uint32)
        _lib.check(self._lib.qe_env_aux(self._h, _lib.ptr(out, C.c_uint32)))
        return out

    def state_dict(self) -> dict:
        """The resume dict of ``SingleThreadQLearning.run_steps`` (single_thread_runtime.py:70-75) for
        the current device state, plus ``"aux"``.  Its arrays are read-only: as long as the caller hands
        this very dict (or these very arrays) back, :meth:`is_resident` recognises it and nothing is
        copied to the device."""
        states, rewards = self.observe()
        aux = self.aux()
        obs = states["observation"] if isinstance(states, dict) else states
        for arr in (obs, rewards, aux):
            arr.flags.writeable = False
        self._resident = (obs, rewards)
        return {"states": states, "infos": [{}] * self.num_agents, "rewards": rewards, "aux": aux}

    def adopt_state(self, obs, rewards, aux) -> dict:
        """:meth:`state_dict` from arrays the engine has just filled (no further device round trip)."""
        for arr in (obs, rewards, aux):
            arr.flags.writeable = False
        self._resident = (obs, rewards)
        return {"states": obs, "infos": [{}] * self.num_agents, "rewards": rewards, "aux": aux}

    def chunk_limit(self, learn: bool) -> int:
        """Vector steps one launch may take on this environment (``qe_rollout_chunk_limit``; cached)."""
        key = bool(learn)
        if key not in self._chunk_limits:
            self._chunk_limits[key] = max(1, int(self._lib.qe_rollout_chunk_limit(self._algo.handle, self._h, 1 if learn else 0)))
        return self._chunk_limits[key]

    def is_resident(self, state_dict) -> bool:
        """True if ``state_dict`` is the (unmodified) one :meth:`state_dict` produced last and the device
        state has not been touched since."""
        if self._resident is None:
            return False
        states = state_dict.get("states")
        obs = states.get("observation") if isinstance(states, dict) else states
        rewards = state_dict.get("rewards")
        return (obs is self._resident[0] and rewards is self._resident[1]
                and not obs.flags.writeable and not rewards.flags.writeable)

    def restore(self, obs=None, agent_rewards=None, aux=None) -> None:
        self._need()
        self._resident = None
        if isinstance(obs, dict):
            obs = obs["observation"]
        o = None if obs is None else _lib.as_i32(obs)
        r = None if agent_rewards is None else np.ascontiguousarray(agent_rewards, dtype=np.float32)
        x = None if aux is None else np.ascontiguousarray(aux, dtype=np.uint32)
        for arr in (o, r, x):
            if arr is not None and arr.size != self.num_agents:
                msg = f"expected {self.num_agents} entries, got {arr.size}"
                raise ValueError(msg)
        _lib.check(self._lib.qe_env_restore(self._h, _lib.ptr(o, C.c_int32), _lib.ptr(x, C.c_uint32),
                                            _lib.ptr(r, C.c_float)))

    def reset_device(self, seed=None) -> None:
        """``reset`` without fetching the observations (the fused rollout does not need them)."""
        self._need()
        self._resident = None
        _lib.check(self._lib.qe_env_reset(self._h, 0 if seed is None else 1,
                                          0 if seed is None else int(seed) & 0xFFFFFFFF))

    def reset(self, seed=None, options=None):  # noqa: ARG002
        self.reset_device(seed)
        obs, _ = self.observe()
        return obs, [{}] * self.num_agents

    def step(self, actions):
        self._need()
        self._resident = None
        a = _lib.as_i32(actions).ravel()
        if a.size != self.num_agents:
            msg = f"expected {self.num_agents} actions, got {a.size}"
            raise ValueError(msg)
        n = self.num_agents
        obs = np.empty(n, dtype=np.int32)
        rewards = np.empty(n, dtype=np.float32)
        term = np.empty(n, dtype=np.uint8)
        masks = np.empty((n, self.action_size), dtype=np.uint8) if self.masked else None
        _lib.check(self._lib.qe_env_step(self._h, _lib.ptr(a, C.c_int32), _lib.ptr(obs, C.c_int32),
                                         _lib.ptr(rewards, C.c_float), _lib.ptr(term, C.c_uint8),
                                         _lib.ptr(masks, C.c_uint8)))
        return self._wrap(obs, masks), rewards, term.astype(bool), np.zeros(n, dtype=bool), [{}] * n


class HashTabularEnv(DeviceVecEnv):
    """Synthetic hashed MDP at the BASELINE shapes (definition: ``csrc/qe_envs.h`` / SURVEY 8d)."""

    kind = _lib.ENV_HASH

    def __init__(self, num_agents, state_size, action_size, seed=1, p_term_256=13, masked=False,
                 agent_offset=0):
        p = _lib.EnvParams(kind=self.kind, masked=int(bool(masked)), seed=int(seed) & 0xFFFFFFFF,
                           p_term_256=int(p_term_256), agent_offset=int(agent_offset))
        super().__init__(num_agents, state_size, action_size, p)
        self.masked = bool(masked)


class GridLakeEnv(DeviceVecEnv):
    """FrozenLake-style ``side x side`` grid with deterministic moves (BASELINE config 1)."""

    kind = _lib.ENV_GRID

    def __init__(self, num_agents, side=10, seed=1):
        p = _lib.EnvParams(kind=self.kind, seed=int(seed) & 0xFFFFFFFF, side=int(side))
        super().__init__(num_agents, int(side) * int(side), 4, p)


class RiggedTwoArmedBanditVecEnv(DeviceVecEnv):
    """``n`` copies of ``environments/rigged_two_armed_bandit.py:55-80`` (known-answer fixture)."""

    kind = _lib.ENV_BANDIT

    def __init__(self, num_agents, episode_len=10):
        p = _lib.EnvParams(kind=self.kind, episode_len=int(episode_len))
        super().__init__(num_agents, 1, 2, p)


class TicTacToeEnv(DeviceVecEnv):
    """``n`` games of the reference's TicTacToe against a uniformly random opponent
    (``environments/tiktaktoe_mod.py:67-237``) behind its Flatten-MultiDiscrete wrapper
    (``wrappers/flatten_multidiscrete_wrapper.py:106-161``): 19 683 states, 9 masked actions --
    the environment of every number the reference publishes (``docs/benchmarks.rst``)."""

    kind = _lib.ENV_TICTACTOE
    masked = True

    def __init__(self, num_agents, seed=1, agent_offset=0):
        p = _lib.EnvParams(kind=self.kind, masked=1, seed=int(seed) & 0xFFFFFFFF, agent_offset=int(agent_offset))
        super().__init__(num_agents, 19683, 9, p)


# ---- finite MDPs given as tables ------------------------------------------------------------------------------------
MAX_OUTCOMES = 8  # outcome slots per (state, action) the device environment supports
_TWO32 = 4294967296.0


class TableMDP(NamedTuple):
    """A finite MDP in the form the device environment stores (see :func:`encode_table_mdp`)."""

    thr: np.ndarray          # uint32[S, A, K]  sampling thresholds; 2**32 - 1 from the last outcome on
    next_state: np.ndarray   # int32[S, A, K]   (slots behind the last outcome repeat it)
    reward: np.ndarray       # float32[S, A, K]
    terminated: np.ndarray   # bool[S, A, K]
    start_thr: np.ndarray    # uint32[n_start]  thresholds of the start support (the last entry is 2**32 - 1)
    start_state: np.ndarray  # int32[n_start]   the support, ascending
    masks: np.ndarray | None  # bool[S, A] or None

    @property
    def state_size(self) -> int:
        return int(self.thr.shape[0])

    @property
    def action_size(self) -> int:
        return int(self.thr.shape[1])

    @property
    def k(self) -> int:
        return int(self.thr.shape[2])

    def outcome_weights(self) -> np.ndarray:
        """``uint64[S, A, K]``: the integer weight of every slot under the sampling rule, out of ``2**32`` -- the number
        of 32-bit words ``u`` for which the rule "first ``j < K - 1`` with ``u < thr[j]``, else slot ``K - 1``" takes
        slot ``j`` (the device records carry ``2**32 - 1`` in slot ``K - 1``, which the rule never reads).  With a
        running maximum ``t = 0``: ``w_j = max(0, thr_j - t)`` then ``t = max(t, thr_j)`` for ``j < K - 1``, and
        ``w_{K-1} = 2**32 - t``.  ``w * 2.0**-32`` is the slot's exact probability; padding copies of the last outcome
        share its mass with it."""
        return _slot_weights(self.thr)

    def start_weights(self) -> np.ndarray:
        """``uint64[n_start]``: the weights of the start support, by the rule of :meth:`outcome_weights`."""
        return _slot_weights(self.start_thr)


def _slot_weights(thr: np.ndarray) -> np.ndarray:
    """Weights out of 2**32 of "the first j below the last with u < thr[j], else the last" along the last axis."""
    t = np.asarray(thr, dtype=np.uint64)
    w = np.empty(t.shape, dtype=np.uint64)
    top = np.zeros(t.shape[:-1], dtype=np.uint64)
    for j in range(t.shape[-1] - 1):
        w[..., j] = np.where(t[..., j] > top, t[..., j] - top, np.uint64(0))
        top = np.maximum(top, t[..., j])
    w[..., -1] = np.uint64(1 << 32) - top
    return w


class MDPSolution(NamedTuple):
    """:meth:`TabularMDPEnv.solve`: value iteration's result for the MDP the environment samples from."""

    q: np.ndarray        # float64[S, A]  Q_t of the last sweep t (masked cells included)
    v: np.ndarray        # float64[S]     V_t: the maximum of the valid columns, 0.0 for a state without one
    start_value: float   # sum over the start support of p_i * V[start_state_i]
    sweeps: int          # t
    residual: float      # max_s |V_t[s] - V_{t-1}[s]|
    converged: bool      # residual <= tol (else stopped by max_sweeps)


def start_value(mdp: "TableMDP", v: np.ndarray) -> float:
    """``sum_i p_i * v[start_state_i]`` over the start support, ascending, accumulated sequentially in float64."""
    acc = 0.0
    for w, s in zip(mdp.start_weights().tolist(), mdp.start_state.tolist()):
        if w:
            acc = acc + (float(w) * 2.0 ** -32) * float(v[s])
    return acc


def check_solve_args(tol, max_sweeps) -> tuple[float, int]:
    """``(tol, max_sweeps)`` of a dynamic-programming call, or ``ValueError``."""
    try:
        tol_f = float(tol)
    except (TypeError, ValueError):
        tol_f = float("nan")
    if not (tol_f >= 0.0 and np.isfinite(tol_f)):
        msg = f"tol must be a finite number >= 0, got {tol!r}"
        raise ValueError(msg)
    if (isinstance(max_sweeps, (bool, np.bool_)) or not isinstance(max_sweeps, (int, np.integer))
            or not 1 <= max_sweeps < 2 ** 31):
        msg = f"max_sweeps must be an integer in 1 .. 2^31 - 1, got {max_sweeps!r}"
        raise ValueError(msg)
    return tol_f, int(max_sweeps)


def check_discounts(discount_factor, what="discount_factor") -> np.ndarray:
    """Discounts as a float64 array, each a finite number in [0, 1], or ``ValueError``."""
    try:
        g = np.asarray(discount_factor, dtype=np.float64)
    except (TypeError, ValueError):
        g = np.array(np.nan)
    if g.size == 0 or not ((g >= 0.0) & (g <= 1.0)).all():
        msg = f"{what}: every discount must be a finite number in [0, 1], got {discount_factor!r}"
        raise ValueError(msg)
    return g


def _thresholds(p: np.ndarray) -> np.ndarray:
    """uint32 thresholds of probability lists along the last axis (zero-probability entries compacted away)."""
    c = np.cumsum(p, axis=-1)
    t = np.floor(c / c[..., -1:] * _TWO32)
    return np.minimum(t, _TWO32 - 1.0).astype(np.uint32)


def encode_table_mdp(probs, next_states, rewards, terminated, initial_state_distrib=None, action_masks=None) -> TableMDP:
    """Encode a finite MDP for :class:`TabularMDPEnv` (and for any model that has to agree with it bit for bit).

    ``probs``, ``next_states``, ``rewards``, ``terminated`` have shape ``[S, A, K]``: outcome ``k`` of ``(s, a)``; unused
    slots have probability 0.  ``initial_state_distrib`` is a length-``S`` distribution (default: state 0), and
    ``action_masks`` an optional ``bool[S, A]``.

    Sampling is integer only.  The outcomes of ``(s, a)`` with a positive probability keep their order, outcomes of
    probability 0 are dropped (they are never taken), and every outcome but the last gets the threshold
    ``thr_k = min(floor(cumsum(p)[k] / cumsum(p)[-1] * 2**32), 2**32 - 1)`` computed in float64.  For a 32-bit word
    ``u`` the outcome is the first ``k`` with ``u < thr_k``, else the last outcome.  In the result the last outcome and
    the slots behind it (copies of it) carry ``2**32 - 1``, so that "the first slot with ``u < thr``, else the last
    slot" is the same rule.  Rewards are rounded to float32.  The start distribution is encoded the same way over its
    support (the states of positive probability, ascending).

    Raises ``ValueError`` for bad shapes, probabilities that are negative or not finite, rewards that are not finite
    after rounding to float32, an ``(s, a)`` (or a start
    distribution) without positive probability or with more than ``MAX_OUTCOMES`` outcomes of positive probability,
    and ``IndexError`` for states out of range.
    """
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 3 or p.shape[0] < 1 or p.shape[1] < 1 or p.shape[2] < 1:
        msg = f"probs must have shape [S, A, K], got {p.shape}"
        raise ValueError(msg)
    S, A, _ = p.shape
    nxt = np.asarray(next_states)
    rew64 = np.asarray(rewards, dtype=np.float64)
    term = np.asarray(terminated)
    for name, arr in (("next_states", nxt), ("rewards", rew64), ("terminated", term)):
        if arr.shape != p.shape:
            msg = f"{name} must have the shape of probs {p.shape}, got {arr.shape}"
            raise ValueError(msg)
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        msg = "outcome probabilities must be finite and >= 0"
        raise ValueError(msg)
    if not np.issubdtype(nxt.dtype, np.integer):
        msg = f"next_states must be integers, got {nxt.dtype}"
        raise ValueError(msg)
    with np.errstate(over="ignore"):
        rew = rew64.astype(np.float32)
    if not np.all(np.isfinite(rew)):
        msg = "rewards must be finite in float32 (the device env returns float32 rewards)"
        raise ValueError(msg)
    pos = p > 0
    count = pos.sum(axis=-1)
    if np.any(count == 0):
        s, a = np.argwhere(count == 0)[0]
        msg = f"(state {s}, action {a}) has no outcome of positive probability"
        raise ValueError(msg)
    k = int(count.max())
    if k > MAX_OUTCOMES:
        msg = f"at most {MAX_OUTCOMES} outcomes of positive probability per (state, action), got {k}"
        raise ValueError(msg)
    if np.any(nxt[pos] < 0) or np.any(nxt[pos] >= S):
        msg = f"next state out of range [0, {S})"
        raise IndexError(msg)
    # compact the positive outcomes to the front (stable), then slot j reads outcome min(j, count - 1)
    order = np.argsort(~pos, axis=-1, kind="stable")[..., :k]
    take = lambda arr: np.take_along_axis(arr, order, axis=-1)  # noqa: E731
    pc = take(p)
    last = np.minimum(np.arange(k)[None, None, :], (count - 1)[..., None])
    fill = lambda arr: np.take_along_axis(take(arr), last, axis=-1)  # noqa: E731
    thr = _thresholds(pc)
    thr[np.arange(k)[None, None, :] >= (count - 1)[..., None]] = np.uint32(0xFFFFFFFF)

    if initial_state_distrib is None:
        isd = np.zeros(S, dtype=np.float64)
        isd[0] = 1.0
    else:
        isd = np.asarray(initial_state_distrib, dtype=np.float64)
    if isd.shape != (S,):
        msg = f"initial_state_distrib must have shape ({S},), got {isd.shape}"
        raise ValueError(msg)
    if not np.all(np.isfinite(isd)) or np.any(isd < 0) or not np.any(isd > 0):
        msg = "initial_state_distrib must be finite, >= 0 and not all zero"
        raise ValueError(msg)
    support = np.flatnonzero(isd > 0)
    start_thr = _thresholds(isd[support])
    start_thr[-1] = np.uint32(0xFFFFFFFF)

    masks = None
    if action_masks is not None:
        masks = np.asarray(action_masks)
        if masks.shape != (S, A):
            msg = f"action_masks must have shape ({S}, {A}), got {masks.shape}"
            raise ValueError(msg)
        masks = masks != 0
    return TableMDP(thr, fill(nxt).astype(np.int32), fill(rew), fill(term != 0), start_thr,
                    support.astype(np.int32), masks)


def outcome_arrays(transitions, action_size=None):
    """``transitions[s][a]`` = list of ``(prob, next_state, reward, terminated)`` (a dict keyed by state / action, as
    gymnasium's toy-text ``P``, or nested sequences) -> ``(probs, next_states, rewards, terminated)`` of shape
    ``[S, A, K]`` with ``K`` the longest list (shorter lists padded with probability 0)."""
    keys = sorted(transitions) if isinstance(transitions, dict) else range(len(transitions))
    if list(keys) != list(range(len(keys))):
        msg = "transitions must list the states 0 .. S-1"
        raise ValueError(msg)
    S = len(keys)
    rows = [transitions[s] for s in range(S)]
    A = action_size
    for s, row in enumerate(rows):
        a_keys = sorted(row) if isinstance(row, dict) else range(len(row))
        if list(a_keys) != list(range(len(a_keys))) or (A is not None and len(a_keys) != A):
            msg = f"state {s}: the actions must be 0 .. A-1 with the same A for every state"
            raise ValueError(msg)
        A = len(a_keys)
    if S == 0 or not A:
        msg = "transitions must have at least one state and one action"
        raise ValueError(msg)
    K = max(len(rows[s][a]) for s in range(S) for a in range(A))
    if K == 0:
        msg = "every (state, action) needs at least one outcome"
        raise ValueError(msg)
    probs = np.zeros((S, A, K), dtype=np.float64)
    nxt = np.zeros((S, A, K), dtype=np.int64)
    rew = np.zeros((S, A, K), dtype=np.float64)  # (rounded to float32, and checked, by encode_table_mdp)
    term = np.zeros((S, A, K), dtype=bool)
    for s in range(S):
        for a in range(A):
            outs = rows[s][a]
            if len(outs) == 0:
                msg = f"(state {s}, action {a}) has no outcome"
                raise ValueError(msg)
            for j, out in enumerate(outs):
                if len(out) != 4:
                    msg = f"(state {s}, action {a}): outcomes are (prob, next_state, reward, terminated)"
                    raise ValueError(msg)
                p, n, r, t = out
                if isinstance(n, (bool, np.bool_)) or not float(n).is_integer():
                    msg = f"(state {s}, action {a}): next_state {n!r} is not an integer"
                    raise ValueError(msg)
                probs[s, a, j], nxt[s, a, j], rew[s, a, j], term[s, a, j] = p, int(n), r, t
    return probs, nxt, rew, term


class TabularMDPEnv(DeviceVecEnv):
    """``num_agents`` copies of a finite MDP given as tables, stepped on the GPU (``qe_env_create_table``).

    ``transitions[s][a]`` is a list of 1 .. 8 outcomes ``(prob, next_state, reward, terminated)`` (or an encoded
    :class:`TableMDP`); ``initial_state_distrib`` a length-``S`` start distribution (default: state 0);
    ``action_masks`` an optional ``bool[S, A]``, with which observations are ``{"observation", "action_mask"}``.
    Outcomes and start states are drawn from a hash of (agent, seed, vector step) by the rule of
    :func:`encode_table_mdp`; on termination the observation is already the next episode's first one (SAME_STEP
    autoreset), and nothing is ever truncated.
    """

    kind = _lib.ENV_TABLE

    def __init__(self, num_agents, transitions, initial_state_distrib=None, action_masks=None, seed=1, agent_offset=0):
        if isinstance(transitions, TableMDP):
            if initial_state_distrib is not None or action_masks is not None:
                msg = "an encoded TableMDP already holds its start distribution and masks"
                raise ValueError(msg)
            mdp = transitions
        else:
            mdp = encode_table_mdp(*outcome_arrays(transitions), initial_state_distrib, action_masks)
        p = _lib.EnvParams(kind=self.kind, masked=int(mdp.masks is not None), seed=int(seed) & 0xFFFFFFFF,
                           agent_offset=int(agent_offset))
        super().__init__(num_agents, mdp.state_size, mdp.action_size, p)
        self.mdp = mdp
        self.masked = mdp.masks is not None

    @classmethod
    def from_transition_dict(cls, P, num_agents, initial_state_distrib=None, action_masks=None, seed=1, agent_offset=0):
        """From gymnasium's toy-text dynamics: ``P[s][a] = [(prob, next_state, reward, terminated), ...]`` (pass the
        environment's ``initial_state_distrib`` along; gymnasium itself is not needed)."""
        return cls(num_agents, P, initial_state_distrib, action_masks, seed=seed, agent_offset=agent_offset)

    @classmethod
    def from_arrays(cls, num_agents, next_states, rewards, terminated, initial_state_distrib=None, action_masks=None,
                    seed=1, agent_offset=0):
        """A deterministic MDP from dense ``[S, A]`` arrays of successors, rewards and termination flags."""
        nxt = np.asarray(next_states)
        if nxt.ndim != 2:
            msg = f"next_states must have shape [S, A], got {nxt.shape}"
            raise ValueError(msg)
        rew = np.broadcast_to(np.asarray(rewards, dtype=np.float64), nxt.shape)
        term = np.broadcast_to(np.asarray(terminated), nxt.shape)
        mdp = encode_table_mdp(np.ones(nxt.shape + (1,)), nxt[..., None], rew[..., None], term[..., None],
                               initial_state_distrib, action_masks)
        return cls(num_agents, mdp, seed=seed, agent_offset=agent_offset)

    def solve(self, discount_factor, tol=1e-12, max_sweeps=100_000) -> MDPSolution:
        """Q*, V* of the MDP by value iteration on the device (``qe_env_table_solve``; needs a bound environment).
        ``V_0 = 0``; sweep ``t`` backs every cell up over ``V_{t-1}`` and stops at the first ``t`` whose residual
        ``max_s |V_t[s] - V_{t-1}[s]|`` is ``<= tol``, else at ``max_sweeps``.  The law is the integer one the
        environment samples from (:meth:`TableMDP.outcome_weights`), all arithmetic float64: the result is defined to
        the bit.  Nothing of the environment's or the algorithm's state is touched."""
        gamma = check_discounts(discount_factor)
        if gamma.ndim != 0:
            msg = f"discount_factor must be one number, got {discount_factor!r}"
            raise ValueError(msg)
        tol, max_sweeps = check_solve_args(tol, max_sweeps)
        self._need()
        q = np.empty((self.state_size, self.action_size), dtype=np.float64)
        v = np.empty(self.state_size, dtype=np.float64)
        sweeps = C.c_int32()
        residual = C.c_double()
        rc = self._lib.qe_env_table_solve(self._h, float(gamma), tol, max_sweeps, _lib.ptr(q, C.c_double),
                                          _lib.ptr(v, C.c_double), C.byref(sweeps), C.byref(residual))
        _lib.check(rc)
        return MDPSolution(q, v, start_value(self.mdp, v), int(sweeps.value), float(residual.value), rc == 1)

    def _create(self, algorithm) -> None:
        m = self.mdp
        # (C-contiguous copies that live through the call: the engine copies them to the device)
        thr = np.ascontiguousarray(m.thr, dtype=np.uint32)
        nxt = np.ascontiguousarray(m.next_state, dtype=np.int32)
        rew = np.ascontiguousarray(m.reward, dtype=np.float32)
        term = np.ascontiguousarray(m.terminated, dtype=np.uint8)
        sthr = np.ascontiguousarray(m.start_thr, dtype=np.uint32)
        sst = np.ascontiguousarray(m.start_state, dtype=np.int32)
        masks = None if m.masks is None else np.ascontiguousarray(m.masks, dtype=np.uint8)
        t = _lib.TableMdp(k=m.k, n_start=len(sst), thr=_lib.ptr(thr, C.c_uint32), next_state=_lib.ptr(nxt, C.c_int32),
                          reward=_lib.ptr(rew, C.c_float), terminated=_lib.ptr(term, C.c_uint8),
                          start_thr=_lib.ptr(sthr, C.c_uint32), start_state=_lib.ptr(sst, C.c_int32),
                          masks=_lib.ptr(masks, C.c_uint8))
        _lib.check(self._lib.qe_env_create_table(C.byref(self._h), algorithm.handle, self.num_agents,
                                                 C.byref(self._params), C.byref(t)))
