"""Shared helpers for the parity tests (oracle side only; no product imports here)."""

from __future__ import annotations

import mmap
import sys
from pathlib import Path

import numpy as np

from oracle.draws import InjectedDraws
from oracle.envs import (GridLakeEnv, HashTabularEnv, RiggedBanditVecEnv, TicTacToeVecEnv, clock_env, env_aux,
                         make_env)
from oracle.qlearn_oracle import OracleQLearning, OracleRuntime, OracleSchedule

GOLDEN = Path(__file__).resolve().parent / "golden"

# must mirror tests/golden/make_golden.py:TRACE_CASES (name -> env spec, steps, dtype, schedules, learn).  (The tables of
# the evaluation / train goldens, EVAL_CASES and TRAIN_CASES, have no mirror: generator and tests both import them from
# tests/golden/make_golden_cases.py.)
TRACE_CASES = {
    "c1_grid_n1": (("grid", 1, 10), 80, "f8", "bench", "iter"),
    "grid4_n1": (("grid", 1, 4), 300, "f8", "bench", "iter"),
    "grid4_n16": (("grid", 16, 4), 100, "f4", "const", "iter"),
    "grid4_n16_f8": (("grid", 16, 4), 100, "f8", "const", "iter"),
    "c2_hash_n128": (("hash", 128, 10000, 8, False), 50, "f4", "bench", "iter"),
    "c2_hash_n128_const": (("hash", 128, 10000, 8, False), 50, "f4", "const", "iter"),
    "hash_dense_n256": (("hash", 256, 64, 16, False), 40, "f4", "const", "iter"),
    "hash_dense_n256_f8": (("hash", 256, 64, 16, False), 40, "f8", "const", "iter"),
    "hash_dense_n256_vec": (("hash", 256, 64, 16, False), 40, "f8", "const", "vec"),
    "c5_hash_masked_n128": (("hash", 128, 500, 64, True), 40, "f4", "const", "iter"),
    "hash_masked_a9_n64": (("hash", 64, 300, 9, True), 40, "f8", "const", "iter"),
    "bandit_n4": (("bandit", 4, 5), 23, "f8", "kat", "iter"),
    "bandit_n128": (("bandit", 128, 7), 30, "f4", "const", "iter"),
    "ttt_n64": (("ttt", 64), 60, "f8", "bench", "iter"),
    "ttt_n128_f4": (("ttt", 128), 50, "f4", "const", "iter"),
}


def make_oracle_env(spec):
    if spec[0] == "hash":
        _, n, S, A, masked = spec
        return HashTabularEnv(n, S, A, seed=1, masked=masked)
    if spec[0] == "grid":
        return GridLakeEnv(spec[1], side=spec[2], seed=1)
    if spec[0] == "ttt":
        return TicTacToeVecEnv(spec[1], seed=1)
    return RiggedBanditVecEnv(spec[1], episode_len=spec[2])


def schedule_params(kind):
    """(lr, eps) as (kind, value, min, decay) tuples."""
    if kind == "bench":
        return ("exponential", 0.1, 1e-5, 0.995), ("exponential", 1.0, 0.01, 0.995)
    if kind == "const":
        return ("constant", 0.1, None, None), ("constant", 0.1, None, None)
    if kind == "nan":  # diverging: lr = 1 with colliding learn_vec increments overflows float32 within tens of steps
        return ("constant", 1.0, None, None), ("constant", 0.3, None, None)
    if kind == "explore":  # every pick exploratory: no greedy selection ever meets a NaN row
        return ("constant", 0.25, None, None), ("constant", 1.0, None, None)
    return ("constant", 1.0, None, None), ("linear", 0.05, None, 0.001)


def run_oracle_trace(spec, steps, dt, sched, learn_mode, gamma=0.99, seed=0, q0=None):
    env = make_oracle_env(spec)
    algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dt))
    if q0 is not None:
        algo.q_table = np.array(q0, dtype=np.dtype(dt))
    lr_p, eps_p = schedule_params(sched)
    rt = OracleRuntime(algo, OracleSchedule(*lr_p), OracleSchedule(*eps_p), learn_mode=learn_mode)
    rt.trace = []
    states, _ = env.reset()
    acc = np.zeros(env.num_agents, dtype=np.float32)
    history = []
    for _ in range(steps):
        states, _ = rt.run_single_step(env, states, acc, history)
    obs = states["observation"] if isinstance(states, dict) else states
    return {
        "actions": np.stack([a for a, _, _ in rt.trace]),
        "eps": np.array([e for _, e, _ in rt.trace]),
        "lr": np.array([v for _, _, v in rt.trace]),
        "q": algo.q_table,
        "history": np.array(history, dtype=np.float32),
        "final_obs": np.asarray(obs, dtype=np.int32),
        "agent_rewards": acc,
        "final_sched": np.array([rt.lr_schedule.get_value(), rt.exploration_rate_schedule.get_value()]),
    }


def dense_from_sparse(idx, val, shape, dtype):
    q = np.zeros(shape, dtype=dtype)
    q.ravel()[idx] = val
    return q


def run_oracle_chunks(spec, chunks, dt, sched, learn_mode, gamma=0.99, seed=0, q0=None, env=None):
    """The closed loop in `chunks` consecutive run_steps-sized pieces.  Returns one dict per chunk with the state at
    its end (q, history so far, obs, acc); a chunk in which the reference's selection raises IndexError (a NaN row
    maximum under a NumPy variant: random.choice([]), q_learning_optimal.py:470, :563) ends the list with
    {"raised": True}.  `env`: an oracle-side environment to drive instead of the one `spec` names."""
    env = make_oracle_env(spec) if env is None else env
    algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dt))
    if q0 is not None:
        algo.q_table = np.array(q0, dtype=np.dtype(dt))
    lr_p, eps_p = schedule_params(sched)
    rt = OracleRuntime(algo, OracleSchedule(*lr_p), OracleSchedule(*eps_p), learn_mode=learn_mode)
    rt.trace = []
    states, _ = env.reset()
    acc = np.zeros(env.num_agents, dtype=np.float32)
    history, out = [], []
    for k in chunks:
        try:
            with np.errstate(all="ignore"):
                for _ in range(k):
                    states, _ = rt.run_single_step(env, states, acc, history)
        except IndexError:
            out.append({"raised": True})
            break
        obs = states["observation"] if isinstance(states, dict) else states
        out.append({"raised": False, "q": algo.q_table.copy(), "history": np.array(history, dtype=np.float32),
                    "final_obs": np.asarray(obs, dtype=np.int32).copy(), "agent_rewards": acc.copy(),
                    "actions": np.stack([a for a, _, _ in rt.trace]) if rt.trace else None})
    return out


def nan_table(S, A, dt, cells, seed):
    """The initial table of the NaN-regime goldens (same construction as tests/golden/make_golden_r3.py)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((S, A)).astype(dt)
    if cells:
        q.ravel()[rng.choice(S * A, size=cells, replace=False)] = np.nan
    return q


def spec_shape(spec):
    if spec[0] == "ttt":
        return 19683, 9
    if spec[0] == "bandit":
        return 1, 2
    if spec[0] == "grid":
        return spec[2] * spec[2], 4
    return spec[2], spec[3]


def golden_nan_trace(g, name, spec, dt, cells, tseed):
    """Chunk-end states of one closed-loop NaN-regime golden (real reference) in run_oracle_chunks' format."""
    S, A = spec_shape(spec)
    base = nan_table(S, A, dt, cells, tseed) if cells else np.zeros((S, A), dtype=dt)
    u = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    n_ok, raised = int(g[f"{name}/n_ok"][0]), int(g[f"{name}/raised_in_chunk"][0])
    actions = g[f"{name}/actions"].astype(np.int32)
    out = []
    for c in range(n_ok):
        q = (g[f"{name}/qx{c}"] ^ base.view(u)).view(np.dtype(dt))
        assert np.array_equal(np.flatnonzero(np.isnan(q)), g[f"{name}/nan_cells{c}"])
        out.append({"raised": False, "q": q, "history": g[f"{name}/history{c}"], "final_obs": g[f"{name}/final_obs{c}"],
                    "agent_rewards": g[f"{name}/agent_rewards{c}"], "actions": actions})
    if raised >= 0:
        out.append({"raised": True})
    return out, base


def run_oracle_delta_log(env, steps, dt, sched, learn_mode, gamma=0.99, seed=0):
    """The closed loop on the NumPy oracle plus the content of the engine's delta log: one (cell = s * A + a, float32
    increment) record per agent and step in (step, agent) order.  ``OracleRuntime._learn`` is wrapped: the records are
    computed from its arguments by the reference's own arithmetic on a copy of the table -- ``learn_iter``: the
    ``lr * (target - Q[s, a])`` of ``single_learn`` when agent i is processed, i.e. after agents 0..i-1 of the step have
    written; ``learn_vec``: the increment array handed to ``np.add.at`` -- and the copy must end equal to the table the
    oracle itself produced."""
    algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dt))
    lr_p, eps_p = schedule_params(sched)
    rt = OracleRuntime(algo, OracleSchedule(*lr_p), OracleSchedule(*eps_p), learn_mode=learn_mode)
    rt.trace = []
    A, cells, deltas = env.action_size, [], []
    inner = rt._learn

    def learn(states, actions, rewards, next_states, terminateds):
        masked = isinstance(next_states, dict)
        s = np.asarray(states["observation"] if masked else states)
        s2 = np.asarray(next_states["observation"] if masked else next_states)
        masks = next_states["action_mask"] if masked else None
        lr = rt.lr_schedule.get_value()
        q = algo.q_table.copy()
        cells.append(s.astype(np.int64) * A + actions)
        with np.errstate(all="ignore"):
            if learn_mode == "iter":  # single_learn, agent by agent
                inc = np.empty(len(s), dtype=np.float32)
                for i in range(len(s)):
                    if terminateds[i]:
                        nxt = 0
                    else:
                        nxt = np.max(q[s2[i]]) if masks is None else np.max(q[s2[i]][np.where(masks[i])])
                    u = lr * ((rewards[i] + gamma * nxt) - q[s[i], actions[i]])
                    inc[i] = u
                    q[s[i], actions[i]] += u
            else:  # learn_vec
                rows = q[s2]
                if masks is not None:
                    rows = np.where(masks, rows, -np.inf)
                targets = rewards + gamma * np.max(rows, axis=1) * (1 - terminateds)
                u = lr * (targets - q[s, actions])
                inc = u.astype(np.float32)
                np.add.at(q, (s, actions), u)
        deltas.append(inc)
        inner(states, actions, rewards, next_states, terminateds)
        assert np.array_equal(q, algo.q_table, equal_nan=True), "the records do not add up to the oracle's own update"

    rt._learn = learn
    states, _ = env.reset()
    acc = np.zeros(env.num_agents, dtype=np.float32)
    history = []
    for _ in range(steps):
        states, _ = rt.run_single_step(env, states, acc, history)
    obs = states["observation"] if isinstance(states, dict) else states
    return {"actions": np.stack([a for a, _, _ in rt.trace]), "cells": np.concatenate(cells).astype(np.uint32),
            "deltas": np.concatenate(deltas), "q": algo.q_table, "history": np.array(history, dtype=np.float32),
            "final_obs": np.asarray(obs, dtype=np.int32), "agent_rewards": acc}


def shares_a_cell_within_a_step(cells, n):
    """True if some step's `n` records name one cell more than once (the case is not contention-free)."""
    by_step = np.sort(np.asarray(cells).reshape(-1, n), axis=1)
    return bool((by_step[:, 1:] == by_step[:, :-1]).any())


# ------------------------------------------------------------------------------- the replay ring fed by the closed loop
def run_oracle_transitions(env, chunks, dt, sched, learn_mode, gamma=0.99, seed=0):
    """The closed loop of ``OracleRuntime`` on `env` in `chunks` consecutive run_steps-sized pieces, plus what a host loop
    calling ``ExperienceReplay.push`` after every ``env.step`` would push: ``(s, a, r, s', terminated)`` of every agent
    and step in (step, agent) order.  ``OracleRuntime._learn`` is wrapped and the records are its arguments: `s` and
    `s'` are the ``"observation"`` entries of a masked environment, `done` is ``terminateds`` (not ``truncateds``).

    Returns ``{"s", "a", "r", "s2", "d"}`` (int64, int64, float32, int64, bool; steps * agents entries each), ``"n"``
    (agents) and ``"chunks"``: per chunk the table, the history so far, the observations, the running returns and the
    number of vector steps (``"steps"``) at its end."""
    algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dt))
    lr_p, eps_p = schedule_params(sched)
    rt = OracleRuntime(algo, OracleSchedule(*lr_p), OracleSchedule(*eps_p), learn_mode=learn_mode)
    rec = {k: [] for k in ("s", "a", "r", "s2", "d")}
    inner = rt._learn

    def learn(states, actions, rewards, next_states, terminateds):
        masked = isinstance(next_states, dict)
        rec["s"].append(np.array(states["observation"] if masked else states, dtype=np.int64))
        rec["a"].append(np.array(actions, dtype=np.int64))
        rec["r"].append(np.array(rewards, dtype=np.float32))
        rec["s2"].append(np.array(next_states["observation"] if masked else next_states, dtype=np.int64))
        rec["d"].append(np.array(terminateds, dtype=bool))
        inner(states, actions, rewards, next_states, terminateds)

    rt._learn = learn
    states, _ = env.reset()
    acc = np.zeros(env.num_agents, dtype=np.float32)
    history, out, done = [], [], 0
    for k in chunks:
        for _ in range(k):
            states, _ = rt.run_single_step(env, states, acc, history)
        done += k
        obs = states["observation"] if isinstance(states, dict) else states
        out.append({"q": algo.q_table.copy(), "history": np.array(history, dtype=np.float32),
                    "final_obs": np.asarray(obs, dtype=np.int32).copy(), "agent_rewards": acc.copy(), "steps": done})
    res = {k: np.concatenate(v) for k, v in rec.items()}
    res.update(n=env.num_agents, chunks=out)
    return res


def ring_after(transitions, capacity, position0=0, full0=False):
    """The ring a host loop leaves that pushes `transitions` (``(s, a, r, s', d)``, five equally long arrays) one entry
    at a time into an ``ExperienceReplay`` of `capacity` slots standing at `position0` / `full0`: push k goes to slot
    ``(position0 + k) % capacity``, and a slot holds the entry of the LARGEST push index that maps to it.

    Returns the five buffers (the reference's dtypes; slots these pushes did not write hold zero), ``position``,
    ``full``, ``len`` and ``written``: bool[capacity], the slots these pushes wrote."""
    s, a, r, s2, d = (np.asarray(x) for x in transitions)
    k = len(s)
    assert len(a) == len(r) == len(s2) == len(d) == k and 0 <= position0 < capacity
    out = {"state": np.zeros(capacity, dtype=np.int64), "action": np.zeros(capacity, dtype=np.int64),
           "reward": np.zeros(capacity, dtype=np.float64), "next_state": np.zeros(capacity, dtype=np.int64),
           "done": np.zeros(capacity, dtype=bool), "written": np.zeros(capacity, dtype=bool)}
    push = np.arange(max(0, k - capacity), k)  # the last `capacity` pushes: one per slot, nothing overwrites them
    slot = (position0 + push) % capacity
    assert len(np.unique(slot)) == len(slot)
    for name, src in (("state", s), ("action", a), ("reward", r), ("next_state", s2), ("done", d)):
        out[name][slot] = src[push]
    out["written"][slot] = True
    out["position"] = (position0 + k) % capacity
    out["full"] = bool(full0 or position0 + k >= capacity)
    out["len"] = capacity if out["full"] else out["position"]
    return out


def transitions_of(want, first_step=0, last_step=None):
    """The five arrays of ``run_oracle_transitions``' result, vector steps [first_step, last_step)."""
    n = want["n"]
    lo, hi = first_step * n, None if last_step is None else last_step * n
    return tuple(want[k][lo:hi] for k in ("s", "a", "r", "s2", "d"))


# ------------------------------------------------------------------------------- tables too large for the host
def lazy_zero_table(S, A, dtype):
    """An all-zero (S, A) table that costs memory only where it is touched: an anonymous private mapping (zero pages on
    first touch, 4 KiB each: transparent huge pages are declined, NumPy asks for them on large allocations of its own and
    one touched row would then cost 2 MiB).  For tables of tens of GiB of which a run visits a few thousand rows: index it
    by rows only -- no whole-array operation, no copy."""
    dtype = np.dtype(dtype)
    noreserve = getattr(mmap, "MAP_NORESERVE", 0x4000 if sys.platform.startswith("linux") else 0)
    m = mmap.mmap(-1, S * A * dtype.itemsize, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | noreserve)
    if hasattr(mmap, "MADV_NOHUGEPAGE"):
        m.madvise(mmap.MADV_NOHUGEPAGE)
    return np.frombuffer(m, dtype=dtype).reshape(S, A)


def resident_bytes():
    """Resident set size of this process (Linux)."""
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * mmap.PAGESIZE


def edge_q0(rows, A, dtype):
    """q0[row, col] of the large-table tests: a cheap function of (row, col), never zero, different from row to row and
    exact in float32 (a multiple of 2^-18 in (0, 0.25])."""
    r = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    c = np.arange(A, dtype=np.uint64).reshape(1, -1)
    h = (r * np.uint64(0x9E3779B1) + c * np.uint64(0x85EBCA77) + np.uint64(0x2545F491)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return ((h & np.uint64(0xFFFF)) + np.uint64(1)).astype(np.dtype(dtype)) * np.dtype(dtype).type(2.0**-18)


def run_sparse_hash_oracle(n, S, A, steps, dt, mode, eps, lr, *, masked=False, placed=(), step0=0, agent_offset=0, seed=0):
    """The closed loop of the C oracle on a hash environment whose table is never materialised: every row the run reads
    or writes starts as ``edge_q0`` of it, every other row as zero -- on a ``lazy_zero_table``.  `placed`: start rows of
    agents 0, 1, ... instead of the environment's reset; `eps` / `lr`: one value per step.

    The set of rows is the fixed point of "seed the rows found so far, run, collect s and s'".  Whole-run passes reach it
    one step of depth per pass (a newly seeded row changes the greedy action taken there and with it everything behind),
    so it is built step by step instead: a step selects from the rows the agents stand on (known and seeded before it
    runs) and reads their successors; a successor that is new is seeded -- nothing has read or written it yet -- and the
    step is run again from the saved state.  Then ONE whole run from a fresh table with exactly those rows seeded is the
    reference, and it must touch no row outside the set (the set has stopped growing).

    Returns the C oracle's run dict plus ``rows`` (ascending), ``q_rows`` (their final content), ``reset_obs``,
    ``final_obs``, ``agent_rewards`` and ``next_obs`` (s' of every record, in record order)."""
    from oracle import c_oracle

    dt = np.dtype(dt)
    eps, lr = np.asarray(eps, dtype=np.float64), np.asarray(lr, dtype=np.float64)
    placed = np.asarray(placed, dtype=np.int32)

    def fresh(rows):
        ref = c_oracle.CHashRollout(n, S, A, masked=masked, agent_offset=agent_offset, seed=seed, dtype=dt, mode=mode,
                                    q=lazy_zero_table(S, A, dt))
        reset_obs = ref.obs.copy()
        ref.obs[:placed.size] = placed
        ref.step = step0
        if len(rows):
            ref.q[rows] = edge_q0(rows, A, dt)
        return ref, reset_obs

    ref, _ = fresh(())
    seeded = np.unique(ref.obs)
    ref.q[seeded] = edge_q0(seeded, A, dt)
    for t in range(steps):
        state = ref.obs.copy(), ref.episode.copy(), ref.acc.copy()
        stood_on = np.unique(ref.obs)
        saved = ref.q[stood_on]  # (fancy indexing: a copy of these rows only -- the only rows step t writes)
        ref.run(eps[t:t + 1], lr[t:t + 1], log_episodes=False)
        new = np.setdiff1d(ref.obs, seeded)
        if new.size:
            ref.q[stood_on] = saved
            ref.obs[:], ref.episode[:], ref.acc[:] = state
            ref.step = step0 + t
            ref.q[new] = edge_q0(new, A, dt)
            seeded = np.union1d(seeded, new)
            ref.run(eps[t:t + 1], lr[t:t + 1], log_episodes=False)
            assert not np.setdiff1d(ref.obs, seeded).size, "the successors of a step moved when they were seeded"
    del ref
    ref, reset_obs = fresh(seeded)
    first_obs = ref.obs.copy()
    out = ref.run(eps, lr, trace=True, delta_log=True)
    s = (out["cells"].astype(np.int64) // A).reshape(steps, n)
    assert np.array_equal(s[0], first_obs)
    next_obs = np.concatenate([s[1:], ref.obs[None, :].astype(np.int64)]).reshape(-1)  # obs of step t + 1 IS s' of step t
    touched = np.union1d(s.reshape(-1), next_obs)
    assert np.isin(touched, seeded).all(), "not a fixed point: the run from the seeded table touched an unseeded row"
    out.update(rows=seeded.astype(np.int64), q_rows=ref.q[seeded], reset_obs=reset_obs, final_obs=ref.obs.copy(),
               agent_rewards=ref.acc.copy(), next_obs=next_obs, touched=touched)
    return out


# ------------------------------------------------------------------------------- greedy evaluation and train()
def _obs_of(env):
    return np.asarray(env.obs if hasattr(env, "obs") else env._obs()["observation"], dtype=np.int32)


def masks_of_every_state(spec):
    """bool[S, A] action masks of a masked hash spec as evaluation sees them (reset(seed=42) re-seeds the masks)."""
    env = make_env(spec)
    if not env.masked:
        return None
    env.reset(seed=42)
    return env.action_masks(np.arange(env.state_size, dtype=np.int32)).astype(bool)


ORACLE_MAX_CALLS = 5000  # selections per oracle runtime: a greedy policy that never ends an episode fails, it does not hang


def _oracle_runtime(env_like, dt, sched, learn_mode, seed, agent_offset, q0=None, start=0, max_calls=ORACLE_MAX_CALLS):
    algo = OracleQLearning(env_like.state_size, env_like.action_size, 0.99, seed=seed, dtype=np.dtype(dt))
    if agent_offset:
        algo._rng = algo._np_rng = InjectedDraws(seed, np.arange(agent_offset, agent_offset + 4096, dtype=np.uint32))
    if q0 is not None:
        algo.q_table = np.array(q0, dtype=np.dtype(dt))
    lr_p, eps_p = schedule_params(sched)
    rt = OracleRuntime(algo, OracleSchedule(*lr_p), OracleSchedule(*eps_p), learn_mode=learn_mode)
    rt.step_counter = int(start)
    rt.calls = 0
    inner = algo.choose_actions

    def choose_actions(*args, **kw):
        # counts the calls; an agent without a candidate (-1 from a list variant, q_learning_optimal.py:302, :348) is
        # reported as the engine reports it on every path: IndexError (include/qlearn_engine.h)
        rt.calls += 1
        if rt.calls > max_calls:
            msg = f"more than {max_calls} selections: the evaluated policy does not end episodes (choose another case)"
            raise RuntimeError(msg)
        actions = inner(*args, **kw)
        if (np.asarray(actions) < 0).any():
            msg = "no selectable action (-1 from a list variant)"
            raise IndexError(msg)
        return actions

    algo.choose_actions = choose_actions
    return rt


def run_oracle_eval(spec, dt, q0, start, mode, count, seed=0, agent_offset=0, rt=None, max_calls=ORACLE_MAX_CALLS):
    """``OracleRuntime.evaluate_steps`` / ``evaluate_episodes`` (`mode`) on a fresh environment of `spec`, from step
    index `start` on table `q0`; with `rt` on that runtime as it stands (its table and counter).  Returns total,
    history, the environment's observations and internal state after the call, the runtime's step counter, the number
    of ``choose_actions`` calls and whether IndexError was raised."""
    env = make_env(spec, agent_offset=agent_offset)
    if rt is None:
        rt = _oracle_runtime(env, dt, "const", "iter", seed, agent_offset, q0, start, max_calls)
    clock_env(env, lambda: rt.step_counter)
    calls0, raised, total, history = rt.calls, False, 0.0, []
    try:
        with np.errstate(all="ignore"):
            total, history = getattr(rt, "evaluate_" + mode)(env, count)
    except IndexError:
        raised = True
    return {"total": total, "history": np.array(history, dtype=np.float32), "obs": _obs_of(env), "aux": env_aux(env),
            "step_counter": rt.step_counter, "calls": rt.calls - calls0, "raised": raised, "rt": rt,
            "acc": None if raised else rt.eval_running_returns}


def run_oracle_train(spec, val_n, dt, sched, learn_mode, steps, every, val, seed=0, agent_offset=0):
    """``OracleRuntime.train`` on fresh training / validation environments of `spec` (`val_n` validation agents);
    `val` is ("steps" | "episodes", count)."""
    env = make_env(spec, agent_offset=agent_offset)
    val_env = make_env((spec[0], val_n) + tuple(spec[2:]), agent_offset=agent_offset)
    rt = _oracle_runtime(env, dt, sched, learn_mode, seed, agent_offset)
    clock_env(env, lambda: rt.step_counter)
    clock_env(val_env, lambda: rt.step_counter)
    kw = {"val_steps": val[1]} if val[0] == "steps" else {"val_episodes": val[1]}
    rewards, val_rewards, _, sd = rt.train(env, steps, val_env, every, **kw)
    states = sd["states"]
    return {"reward_history": np.array(rewards, dtype=np.float32), "val_reward_history": np.array(val_rewards, dtype=np.float64),
            "q": rt.algorithm.q_table, "final_sched": np.array([rt.lr_schedule.get_value(), rt.exploration_rate_schedule.get_value()]),
            "obs": np.asarray(states["observation"] if isinstance(states, dict) else states, dtype=np.int32),
            "agent_rewards": np.asarray(sd["rewards"], dtype=np.float32), "aux": env_aux(env), "val_obs": _obs_of(val_env),
            "val_aux": env_aux(val_env), "step_counter": rt.step_counter, "calls": rt.calls}


def golden_eval_record(g, name, mode):
    meta = g[f"eval/{name}/{mode}/meta"]
    state = g[f"eval/{name}/{mode}/state"]
    return {"print": meta[:2], "raised": bool(meta[2]), "no_candidate": bool(meta[3]), "start": int(meta[4]),
            "calls": int(meta[5]), "total": float(meta[6:7].view(np.float64)[0]), "history": g[f"eval/{name}/{mode}/history"],
            "obs": state[0].view(np.int32), "aux": state[1]}


def golden_train_record(g, name, shape, dt):
    p = f"train/{name}/"
    meta, state, val_state = g[p + "meta"], g[p + "state"], g[p + "val_state"]
    return {"reward_history": g[p + "reward_history"], "val_reward_history": g[p + "val_reward_history"],
            "q": dense_from_sparse(g[p + "q_idx"], g[p + "q_val"], shape, np.dtype(dt)), "final_sched": meta[:2],
            "calls": int(meta[2]), "obs": state[0].view(np.int32), "aux": state[1], "agent_rewards": state[2].view(np.float32),
            "val_obs": val_state[0].view(np.int32), "val_aux": val_state[1]}
