"""``QLearningPopulation``: many independent single-agent Q-learners trained in one launch.

The case of 20 to 1000 seeds for a confidence band, or a grid over learning rate, exploration schedule and discount:
each run is the classic one-environment ``SingleThreadQLearning`` of the reference, and all of them step together on
the GPU, one lane per run (``qe_population_rollout``, kernel ``k_rollout_runs``).

Contract: a population of ``M`` runs over one environment object of ``num_agents = M`` and one seed.  Run ``r`` after
``K`` steps is, bit for bit (table, episode returns and their steps, final observation, env-internal state, running
return), the standalone run

    algo = OptimalQLearningBase(S, A, discount_factor[r], seed, dtype=dtype)
    GpuRolloutQLearning(algo, lr_schedule[r], exploration_rate_schedule[r], learn_mode).run_steps(K, env_r)

where ``env_r`` is the same environment kind and parameters with one agent and ``agent_offset = env_offset + r``.
Calls chain: one call of 2K steps equals two calls of K steps, schedule values included.
"""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from dist_classicrl_amd import _lib
from dist_classicrl_amd.environments.device_envs import DeviceVecEnv
from dist_classicrl_amd.schedules import BaseSchedule, ConstantSchedule, ExponentialSchedule, LinearSchedule

SCHED_CONSTANT, SCHED_LINEAR, SCHED_EXPONENTIAL = 0, 1, 2
# qe_run_schedule as a NumPy record (the per-run descriptor arrays handed to qe_population_configure)
_DESCRIPTOR = np.dtype([("value", "<f8"), ("min_value", "<f8"), ("factor", "<f8"), ("kind", "<i4"), ("reserved", "<i4")])


def schedule_descriptor(schedule) -> tuple[int, float, float, float]:
    """``(kind, value, min_value, factor)`` of one of the three schedules, ``factor`` computed as their ``update(1)``
    does (``decay_rate ** 1`` / ``1 * decay_rate``).  Any other schedule raises ``TypeError``: the kernel can only
    restate these recurrences."""
    kind = type(schedule)
    if kind is ConstantSchedule:
        return SCHED_CONSTANT, float(schedule.get_value()), float(schedule.min_value), 0.0
    if kind is LinearSchedule:
        return SCHED_LINEAR, float(schedule.get_value()), float(schedule.min_value), float(1 * schedule.decay_rate)
    if kind is ExponentialSchedule:
        return SCHED_EXPONENTIAL, float(schedule.get_value()), float(schedule.min_value), float(schedule.decay_rate**1)
    if isinstance(schedule, BaseSchedule):
        msg = f"{kind.__name__} has no device form: a population takes ConstantSchedule, LinearSchedule or ExponentialSchedule"
    else:
        msg = f"expected a schedule, got {kind.__name__}"
    raise TypeError(msg)


def advance_descriptor(kind: int, value: float, min_value: float, factor: float, count: int) -> np.ndarray:
    """The values the kernel reads at ``count`` consecutive steps (its recurrence, restated)."""
    out = np.empty(count, dtype=np.float64)
    v = float(value)
    for t in range(count):
        out[t] = v
        if kind == SCHED_LINEAR:
            v = v + factor
        elif kind == SCHED_EXPONENTIAL:
            x = v * factor
            v = min_value if min_value > x else x
    return out


class PopulationRun(NamedTuple):
    """Result of one :meth:`QLearningPopulation.run_steps` call."""

    mean_returns: np.ndarray    # float32 [M]: sequential float32 sum of the run's returns / their count; NaN if none
    episode_counts: np.ndarray  # int64 [M]
    returns: np.ndarray         # float32, every run's returns in order, run after run (empty without the log)
    offsets: np.ndarray         # int64 [M + 1]: run r's returns are returns[offsets[r]:offsets[r + 1]]
    steps: np.ndarray           # int32, step within the call at which each of those episodes ended
    state_dict: dict            # what an exact resume needs (pass it to the next call / restore_training_state)

    def run_returns(self, r: int) -> np.ndarray:
        return self.returns[self.offsets[r]:self.offsets[r + 1]]

    def run_steps(self, r: int) -> np.ndarray:
        return self.steps[self.offsets[r]:self.offsets[r + 1]]


def _per_run(value, runs, what):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != runs:
            msg = f"{what}: expected one entry per run ({runs}), got {len(value)}"
            raise ValueError(msg)
        return list(value)
    return [value] * runs


class QLearningPopulation:
    """``runs`` independent single-agent Q-learners over ``state_size`` x ``action_size`` (at most 64 actions).

    ``discount_factor``, ``lr_schedule`` and ``exploration_rate_schedule`` take one value / schedule for every run or a
    sequence of ``runs``.  Schedules are ``ConstantSchedule``, ``LinearSchedule`` or ``ExponentialSchedule``; after each
    call they are left advanced (``set_value``), as :class:`GpuRolloutQLearning` leaves them."""

    def __init__(self, runs, state_size, action_size, discount_factor=0.97, lr_schedule=None,
                 exploration_rate_schedule=None, seed=0, dtype=np.float64, learn_mode="iter", device=0):
        self.runs = int(runs)
        self.state_size = int(state_size)
        self.action_size = int(action_size)
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            msg = "dtype must be float32 or float64"
            raise ValueError(msg)
        if learn_mode not in ("iter", "vec"):
            msg = "learn_mode must be 'iter' (reference `learn`, sequential) or 'vec' (`learn_vec`)"
            raise ValueError(msg)
        if self.runs <= 0:
            msg = "runs must be positive"
            raise ValueError(msg)
        self.learn_mode = learn_mode
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.discount_factor = np.ascontiguousarray(_per_run(discount_factor, self.runs, "discount_factor"), dtype=np.float64)
        lr_schedule = ConstantSchedule(0.1) if lr_schedule is None else lr_schedule
        exploration_rate_schedule = ConstantSchedule(0.1) if exploration_rate_schedule is None else exploration_rate_schedule
        self.lr_schedules = _per_run(lr_schedule, self.runs, "lr_schedule")
        self.exploration_rate_schedules = _per_run(exploration_rate_schedule, self.runs, "exploration_rate_schedule")
        for s in self.lr_schedules + self.exploration_rate_schedules:
            schedule_descriptor(s)  # TypeError before anything is allocated
        self.last_stats = None
        self._lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self._lib.qe_create_population(C.byref(self._h), self.runs, self.state_size, self.action_size, self.seed,
                                                  _lib.QE_F32 if self.dtype == np.float32 else _lib.QE_F64, int(device)))
        _lib.check(self._lib.qe_population_configure(self._h, None, None, _lib.ptr(self.discount_factor, C.c_double)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.qe_destroy(h)
            self._h = C.c_void_p()

    @property
    def handle(self):
        """The population's ``qe_engine*`` (environments bind to it)."""
        return self._h

    @property
    def step_counter(self) -> int:
        """Index of the next step in the draw protocol (shared by all runs)."""
        return int(self._lib.qe_get_step_counter(self._h))

    @step_counter.setter
    def step_counter(self, value: int) -> None:
        _lib.check(self._lib.qe_set_step_counter(self._h, int(value)))

    # ------------------------------------------------------------------ tables
    @property
    def q_tables(self) -> np.ndarray:
        """All tables, ``(runs, state_size, action_size)``."""
        host = np.empty((self.runs, self.state_size, self.action_size), dtype=self.dtype)
        _lib.check(self._lib.qe_table_download(self._h, host.ctypes.data, _lib.QE_F32 if self.dtype == np.float32 else _lib.QE_F64))
        return host

    def q_table(self, r: int) -> np.ndarray:
        """Run ``r``'s table, ``(state_size, action_size)``."""
        r = int(r)
        if not 0 <= r < self.runs:
            msg = f"run {r} out of range [0, {self.runs})"
            raise IndexError(msg)
        host = np.empty((self.state_size, self.action_size), dtype=self.dtype)
        _lib.check(self._lib.qe_table_download_rows(self._h, host.ctypes.data, r * self.state_size, self.state_size))
        return host

    def set_q_tables(self, tables) -> None:
        """``(state_size, action_size)`` (every run starts from it) or ``(runs, state_size, action_size)``."""
        arr = np.asarray(tables)
        one = (self.state_size, self.action_size)
        if arr.shape == one:
            arr = np.broadcast_to(arr, (self.runs, *one))
        elif arr.shape != (self.runs, *one):
            msg = f"tables must have shape {one} or {(self.runs, *one)}, got {arr.shape}"
            raise ValueError(msg)
        up = np.float32 if arr.dtype == np.float32 else np.float64
        arr = np.ascontiguousarray(arr, dtype=up)
        _lib.check(self._lib.qe_table_upload(self._h, arr.ctypes.data, _lib.QE_F32 if up == np.float32 else _lib.QE_F64))

    def save(self, filename) -> None:
        """The ``(runs, state_size, action_size)`` tables as one ``.npy``."""
        np.save(filename, self.q_tables)

    def load(self, filename) -> None:
        self.set_q_tables(np.load(filename))

    # ------------------------------------------------------------------ training
    def _descriptors(self, schedules):
        # (one descriptor per distinct schedule object: a schedule shared by 65 536 runs is encoded once)
        rows = np.zeros(self.runs, dtype=_DESCRIPTOR)
        seen = {}
        for r, s in enumerate(schedules):
            d = seen.get(id(s))
            if d is None:
                kind, value, lo, factor = schedule_descriptor(s)
                d = seen[id(s)] = np.array((value, lo, factor, kind, 0), dtype=_DESCRIPTOR)
            rows[r] = d
        return rows

    def _adopt_schedule_values(self):
        eps = np.empty(self.runs, dtype=np.float64)
        lr = np.empty(self.runs, dtype=np.float64)
        _lib.check(self._lib.qe_population_schedules(self._h, _lib.ptr(eps, C.c_double), _lib.ptr(lr, C.c_double)))
        for schedules, values in ((self.exploration_rate_schedules, eps), (self.lr_schedules, lr)):
            last = {id(s): (s, r) for r, s in enumerate(schedules)}  # (a shared schedule: its runs hold the same value)
            for s, r in last.values():
                s.set_value(float(values[r]))
        return eps, lr

    def run_steps(self, steps, env, curr_state_dict=None, log=True) -> PopulationRun:
        """``steps`` steps of every run on ``env`` (a device environment of ``num_agents == runs``).  ``curr_state_dict``
        None resets the environment, as the reference's ``run_steps``; the dict of the previous call continues it.
        ``log=False`` skips the per-episode returns (counts and means are always produced).  A run that meets a state
        without a selectable action raises ``IndexError`` naming the runs (``.runs``; ``.result`` holds the call's
        result, in which the other runs are unaffected)."""
        if not isinstance(env, DeviceVecEnv):
            msg = "a population runs on a device environment (dist_classicrl_amd.environments)"
            raise TypeError(msg)
        steps = int(steps)
        env.bind(self)
        if curr_state_dict is None:
            env.reset_device()
        elif not env.is_resident(curr_state_dict):
            env.restore(curr_state_dict["states"], curr_state_dict["rewards"], curr_state_dict.get("aux"))
        eps_d = self._descriptors(self.exploration_rate_schedules)
        lr_d = self._descriptors(self.lr_schedules)
        sched_p = C.POINTER(_lib.RunSchedule)
        _lib.check(self._lib.qe_population_configure(self._h, eps_d.ctypes.data_as(sched_p), lr_d.ctypes.data_as(sched_p), None))
        M = self.runs
        counts = np.empty(M, dtype=np.int64)
        sums = np.empty(M, dtype=np.float32)
        state = np.empty(3 * M, dtype=np.uint32)  # observations | env-internal state | running returns
        status = np.empty(M, dtype=np.uint32)
        st = _lib.RolloutStats()
        mode = _lib.LEARN_ITER if self.learn_mode == "iter" else _lib.LEARN_VEC
        base = state.ctypes.data
        total = self._lib.qe_population_rollout(
            self._h, env.handle, steps, mode, 1 if log else 0, C.byref(st), _lib.ptr(counts, C.c_int64),
            _lib.ptr(sums, C.c_float), C.cast(base, C.POINTER(C.c_int32)), C.cast(base + 4 * M, C.POINTER(C.c_uint32)),
            C.cast(base + 8 * M, C.POINTER(C.c_float)), _lib.ptr(status, C.c_uint32))
        empty = total == _lib.ERR_INDEX
        if total < 0 and not empty:
            _lib.check(total)
        eps_v, lr_v = self._adopt_schedule_values()
        self.last_stats = {f: getattr(st, f) for f, _ in st._fields_}
        total = int(counts.sum())
        rets = np.empty(total if log else 0, dtype=np.float32)
        at = np.empty(total if log else 0, dtype=np.int32)
        if log and total:
            n = self._lib.qe_population_log(self._h, total, _lib.ptr(at, C.c_int32), _lib.ptr(rets, C.c_float))
            _lib.check(n)
        offsets = np.zeros(M + 1, dtype=np.int64)
        if log:
            np.cumsum(counts, out=offsets[1:])
        with np.errstate(divide="ignore", invalid="ignore"):
            means = sums / counts.astype(np.float32)  # float32, as the standalone's float32 sum / len
        means[counts == 0] = np.nan
        obs, aux, rewards = state[:M].view(np.int32), state[M:2 * M], state[2 * M:].view(np.float32)
        state_dict = env.adopt_state(obs, rewards, aux)
        state_dict["rng_step"] = self.step_counter
        state_dict["lr"] = lr_v
        state_dict["exploration_rate"] = eps_v
        result = PopulationRun(means, counts, rets, offsets, at, state_dict)
        if empty:
            bad = np.flatnonzero(status).tolist()
            err = IndexError(f"Cannot choose from an empty sequence (runs {', '.join(map(str, bad))})")
            err.runs = bad
            err.result = result
            raise err
        return result

    def restore_training_state(self, state_dict) -> None:
        """Continue exactly where ``state_dict`` (of ``run_steps``, e.g. un-pickled in a fresh process) left off: draw
        counter and every run's schedule values.  Tables: :meth:`load`; environments: pass the dict to ``run_steps``."""
        self.step_counter = int(state_dict["rng_step"])
        for schedules, key in ((self.lr_schedules, "lr"), (self.exploration_rate_schedules, "exploration_rate")):
            values = np.broadcast_to(np.asarray(state_dict[key], dtype=np.float64), (self.runs,))
            last = {id(s): (s, r) for r, s in enumerate(schedules)}
            for s, r in last.values():
                s.set_value(float(values[r]))


__all__ = ["PopulationRun", "QLearningPopulation", "advance_descriptor", "schedule_descriptor"]
