"""Device-free builders of the environment transition cases (tests/test_gpu_env_transitions.py restores and steps them on
the GPU; tests/test_env_transition_cases.py checks the builders themselves and the conditions the cases are chosen for).

A case is what one host-driven call sequence needs and what must come back:

    restore(obs, zeros, aux); step_counter = step + 1; step(actions)
        -> next_obs, next_aux, reward, terminated, masks of next_obs (masked environments)

Expected values come from ``oracle/envs.py`` (hash, grid, bandit, and TicTacToe where the reference has no answer),
``tests/table_mdp_model.py`` (table environments) and, for TicTacToe, the golden table of the reference's own
environment (``tests/golden/ttt_transitions.npz``) combined with the draw protocol of ``TicTacToeVecEnv``.
"""

from __future__ import annotations

from pathlib import Path
from typing import NamedTuple

import numpy as np

from oracle.draws import mulhi32
from oracle.envs import (GridLakeEnv, HashTabularEnv, RiggedBanditVecEnv, TicTacToeVecEnv, env_aux)
from table_mdp_model import TableMDPVecEnv

GOLDEN = Path(__file__).resolve().parent / "golden"
HIGH_STEP = (1 << 32) + 5       # the high word of the step index enters the hash
RESET_STEP = (1 << 64) - 1      # the index reset() draws at: what qe_env_step reads at step_counter == 0


def crossing_offset(n):
    """An agent_offset with which the ids of `n` agents cross 2^32 in the middle (one agent: the top id)."""
    return (1 << 32) - max(1, n // 2)


class Case(NamedTuple):
    obs: np.ndarray          # int32[n]   restored observations
    aux: np.ndarray          # uint32[n]  restored environment-internal state
    actions: np.ndarray      # int32[n]
    agent_offset: int        # the device environment's agent_offset: agent i has id (agent_offset + i) mod 2^32
    step: int                # vector step the draws belong to
    next_obs: np.ndarray     # int32[n]
    next_aux: np.ndarray     # uint32[n]
    reward: np.ndarray       # float32[n]
    terminated: np.ndarray   # bool[n]
    start_masks: np.ndarray | None  # bool[n, A]: masks of obs
    masks: np.ndarray | None        # bool[n, A]: masks of next_obs
    info: dict               # what the conditions on the inputs are checked from

    @property
    def n(self) -> int:
        return len(self.obs)


def agent_ids(offset, n):
    return ((int(offset) + np.arange(n, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)


# ---- TicTacToe ------------------------------------------------------------------------------------------------------
TTT_D = 32       # replicas of every (position, action) pair, as consecutive agents
TTT_SEED = 1
TTT_STEPS = (0, HIGH_STEP)
TTT_COUNTS = {"positions": 4520, "pairs": 16167, "agent_ends": 2862, "reply_rows": 43644, "rows": 46506}
_POW3 = 3 ** np.arange(8, -1, -1, dtype=np.int64)
_CELLS = np.arange(9, dtype=np.int64)


class TttTable(NamedTuple):
    cols: dict               # the golden columns as int64
    pos_row: np.ndarray      # [positions]  first row of every position (board and the agent's mark)
    pair_row: np.ndarray     # [pairs]      first row of every (position, action) pair
    pair_of_row: np.ndarray  # [rows]
    row_of: np.ndarray       # [pairs, 10]  row of (pair, reply), -1 where the reference offers no such reply
    empties: np.ndarray      # [pairs, 9]   empty cells after the agent's move, ascending, then the occupied ones
    n_empty: np.ndarray      # [pairs]


_ttt_cache = []


def ttt_table() -> TttTable:
    if _ttt_cache:
        return _ttt_cache[0]
    with np.load(GOLDEN / "ttt_transitions.npz") as g:
        c = {k: g[k].astype(np.int64) for k in g.files}
    key = ((c["mark"] * 512 + c["m1"]) * 512 + c["m2"]) * 9 + c["action"]
    assert (np.diff(key) >= 0).all()  # rows are ordered by (mark, m1, m2, action, reply)
    _, pair_row, pair_of_row = np.unique(key, return_index=True, return_inverse=True)
    _, pos_row = np.unique(key // 9, return_index=True)
    row_of = np.full((len(pair_row), 10), -1, dtype=np.int64)
    row_of[pair_of_row, c["reply"]] = np.arange(len(key))
    occupied = (c["m1"] | c["m2"] | (1 << c["action"]))[pair_row]
    empty = ((occupied[:, None] >> _CELLS[None, :]) & 1) == 0
    empties = np.argsort(~empty, axis=1, kind="stable")
    t = TttTable(c, pos_row, pair_row, pair_of_row, row_of, empties, empty.sum(axis=1))
    _ttt_cache.append(t)
    return t


def ttt_encode_vec(m1, m2):
    """Base-3 board id, cell 0 the most significant digit (checked against the reference's ids in the CPU tests)."""
    m1, m2 = np.asarray(m1, dtype=np.int64), np.asarray(m2, dtype=np.int64)
    digits = ((m1[:, None] >> _CELLS) & 1) + 2 * ((m2[:, None] >> _CELLS) & 1)
    return (digits * _POW3).sum(axis=1).astype(np.int32)


def ttt_aux(m1, m2, mark):
    return (np.asarray(m1, np.int64) | (np.asarray(m2, np.int64) << 9)
            | ((np.asarray(mark) == 2).astype(np.int64) << 18)).astype(np.uint32)


def ttt_words(ids, step, seed):
    env = TicTacToeVecEnv(1, seed=seed)
    env.agent_ids = np.asarray(ids, dtype=np.uint32)
    return env._words(int(step))


def ttt_case(step, pairs=None, replicas=TTT_D, seed=TTT_SEED, agent_offset=0) -> Case:
    """Every (position, action) pair of the golden table (or `pairs`), `replicas` consecutive agents each, stepped at
    `step`: the reply is the ``mulhi32(h0, n_empty)``-th empty cell, the result the golden row of (pair, reply), and a
    finished episode reopens from ``h1 & 1`` (agent starts) and ``mulhi32(h2, 9)`` (the machine's opening cell)."""
    t = ttt_table()
    c = t.cols
    pairs = np.arange(len(t.pair_row)) if pairs is None else np.asarray(pairs)
    pair = np.repeat(pairs, replicas)
    ids = agent_ids(agent_offset, len(pair))
    h0, h1, h2 = ttt_words(ids, step, seed)
    agent_ends = t.row_of[pair, 9] >= 0
    k = mulhi32(h0, np.where(agent_ends, 1, t.n_empty[pair])).astype(np.int64)
    reply = np.where(agent_ends, 9, t.empties[pair, k])
    row = t.row_of[pair, reply]
    assert (row >= 0).all()  # the k-th empty cell is a reply the reference offers
    terminated = c["terminated"][row] == 1
    # ways an episode can open: 0 = the agent starts, 1 + cell = the machine opened on that cell
    opening = np.where((h1 & np.uint32(1)) == 0, 0, 1 + mulhi32(h2, 9).astype(np.int64))
    m1 = np.where(terminated, np.where(opening > 0, 1 << np.maximum(opening - 1, 0), 0), c["out_m1"][row])
    m2 = np.where(terminated, 0, c["out_m2"][row])
    mark = np.where(terminated, np.where(opening > 0, 2, 1), c["mark"][row])
    first = t.pair_row[pair]
    return Case(
        obs=c["obs"][first].astype(np.int32), aux=ttt_aux(c["m1"][first], c["m2"][first], c["mark"][first]),
        actions=c["action"][first].astype(np.int32), agent_offset=agent_offset, step=int(step),
        next_obs=ttt_encode_vec(m1, m2), next_aux=ttt_aux(m1, m2, mark), reward=c["reward"][row].astype(np.float32),
        terminated=terminated, start_masks=_ttt_empty(c["m1"][first] | c["m2"][first]), masks=_ttt_empty(m1 | m2),
        info={"row": row, "opening": np.where(terminated, opening, -1), "ids": ids, "seed": seed})


def _ttt_empty(occupied):
    return ((np.asarray(occupied, dtype=np.int64)[:, None] >> _CELLS) & 1) == 0


def ttt_oracle_case(m1, m2, mark, actions, step, seed=TTT_SEED, agent_offset=0) -> Case:
    """``TicTacToeVecEnv.step`` itself on boards set directly: for what the reference has no answer to (an action on an
    occupied cell, where it asserts) and as the per-agent restatement the vectorised builder is checked against."""
    n = len(m1)
    env = TicTacToeVecEnv(n, seed=seed)
    env.agent_ids = agent_ids(agent_offset, n)
    env.m1[:], env.m2[:], env.agent_mark[:] = m1, m2, mark
    env.step_index = int(step)
    obs0 = ttt_encode_vec(m1, m2)
    aux0 = env_aux(env)
    start_masks = env.action_masks(obs0).astype(bool)
    obs, reward, terminated, truncated, _ = env.step(np.asarray(actions))
    assert not truncated.any()
    return Case(obs=obs0, aux=aux0, actions=np.asarray(actions, dtype=np.int32), agent_offset=agent_offset, step=int(step),
                next_obs=obs["observation"].astype(np.int32), next_aux=env_aux(env), reward=reward.astype(np.float32),
                terminated=terminated.astype(bool), start_masks=start_masks, masks=obs["action_mask"].astype(bool),
                info={"ids": env.agent_ids, "seed": seed})


def ttt_occupied_cell_case(step=3) -> Case:
    """Every (position, occupied cell) as the action.  The reference asserts there and the fused paths never take such an
    action, but the host-driven entry point accepts it: the oracle defines the outcome."""
    t = ttt_table()
    c = t.cols
    pos = t.pos_row
    m1, m2, mark = c["m1"][pos], c["m2"][pos], c["mark"][pos]
    occupied = (((m1 | m2)[:, None] >> _CELLS) & 1) == 1
    p, cell = np.nonzero(occupied)
    return ttt_oracle_case(m1[p], m2[p], mark[p], cell, step)


def ttt_reset_expected(n, seed, agent_offset, reseed=None):
    """(observations, masks, aux) of ``TicTacToeVecEnv.reset`` for agents ``(agent_offset + i) mod 2^32``."""
    env = TicTacToeVecEnv(n, seed=seed)
    env.agent_ids = agent_ids(agent_offset, n)
    obs, _ = env.reset(seed=reseed)
    return obs["observation"].astype(np.int32), obs["action_mask"].astype(bool), env_aux(env)


# ---- hash environment -----------------------------------------------------------------------------------------------
HASH_SHAPES = [(1, 1, False), (7, 3, False), (1000, 8, False), (300, 31, True), (300, 32, True), (300, 33, True),
               (50, 63, True), (50, 64, True), (40, 65, True), (20, 256, True)]
HASH_P_TERM = (0, 13, 128, 256)
HASH_EPISODES = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32)
HASH_SEED = 1


def hash_case(S, A, masked, p_term_256, agent_offset=0, seed=HASH_SEED, n=None, step=0) -> Case:
    """All (s, a) pairs as agents (or, with `n`, the `n` pairs ``37 * i mod S * A``), episode counters 0, 1 and 2^32 - 1
    spread over them so that every counter value meets every action."""
    cells = np.arange(S * A, dtype=np.int64) if n is None else (37 * np.arange(n, dtype=np.int64)) % (S * A)
    s, a = cells // A, cells % A
    env = HashTabularEnv(len(cells), S, A, seed=seed, p_term_256=p_term_256, masked=masked)
    env.agent_ids = agent_ids(agent_offset, len(cells))
    env.obs = s.astype(np.int32)
    env.episode = HASH_EPISODES[(cells + cells // A) % 3].copy()
    aux0 = env.episode.copy()
    start_masks = env.action_masks(env.obs).astype(bool) if masked else None
    nxt, reward, terminated, truncated, _ = env.step(a)
    assert not truncated.any()
    return Case(obs=s.astype(np.int32), aux=aux0, actions=a.astype(np.int32), agent_offset=agent_offset, step=int(step),
                next_obs=(nxt["observation"] if masked else nxt).astype(np.int32), next_aux=env.episode.astype(np.uint32),
                reward=reward.astype(np.float32), terminated=terminated.astype(bool), start_masks=start_masks,
                masks=nxt["action_mask"].astype(bool) if masked else None,
                info={"S": S, "A": A, "masked": masked, "p_term_256": p_term_256, "seed": seed})


def hash_reset_expected(n, S, A, seed, agent_offset, reseed=None):
    env = HashTabularEnv(n, S, A, seed=seed)
    env.agent_ids = agent_ids(agent_offset, n)
    obs, _ = env.reset(seed=reseed)
    return obs.astype(np.int32), env.episode.astype(np.uint32)


# ---- grid -----------------------------------------------------------------------------------------------------------
GRID_SIDES = (2, 3, 10, 31)
GRID_SEEDS = (1, 7)


def grid_case(side, seed) -> Case:
    """Every (cell, action), holes and the goal included as starting cells (the oracle defines these)."""
    cells = np.arange(side * side * 4, dtype=np.int64)
    s, a = cells // 4, cells % 4
    env = GridLakeEnv(len(cells), side=side, seed=seed)
    env.obs = s.astype(np.int32)
    nxt, reward, terminated, truncated, _ = env.step(a)
    assert not truncated.any()
    zeros = np.zeros(len(cells), dtype=np.uint32)
    return Case(obs=s.astype(np.int32), aux=zeros, actions=a.astype(np.int32), agent_offset=0, step=0,
                next_obs=nxt.astype(np.int32), next_aux=zeros, reward=reward.astype(np.float32),
                terminated=terminated.astype(bool), start_masks=None, masks=None,
                info={"holes": env.holes(), "side": side, "seed": seed})


# ---- bandit ---------------------------------------------------------------------------------------------------------
BANDIT_LENGTHS = (1, 2, 10)


def bandit_case(episode_len) -> Case:
    """The step within the episode at every value below the length, both actions."""
    t0, a = np.divmod(np.arange(2 * episode_len, dtype=np.int64), 2)
    env = RiggedBanditVecEnv(len(a), episode_len=episode_len)
    env.t[:] = t0
    nxt, reward, terminated, truncated, _ = env.step(a)
    assert not truncated.any()
    return Case(obs=np.zeros(len(a), dtype=np.int32), aux=t0.astype(np.uint32), actions=a.astype(np.int32), agent_offset=0,
                step=0, next_obs=nxt.astype(np.int32), next_aux=env.t.astype(np.uint32), reward=reward.astype(np.float32),
                terminated=terminated.astype(bool), start_masks=None, masks=None, info={"episode_len": episode_len})


# ---- table environments ---------------------------------------------------------------------------------------------
TABLE_D = 128   # replicas of every (state, action)
TABLE_SEED = 1
TABLE_STEPS = (0, HIGH_STEP)
# name -> (S, A, K, start support, masked)
TABLE_SHAPES = {"k1": (5, 3, 1, 1, False), "k2": (6, 2, 2, 2, False), "k3": (7, 3, 3, 3, False), "k8": (9, 4, 8, 7, False),
                "masked_a9": (8, 9, 3, 3, True), "masked_a40": (4, 40, 2, 2, True)}
# weights of the outcome slots in eighths; the last slot's weight is positive by the encoding (2^32 minus the largest
# threshold), zero-weight slots stand in front of it and between the others
_EIGHTHS = {1: [(8,)], 2: [(4, 4), (0, 8), (7, 1), (1, 7)], 3: [(2, 0, 6), (0, 0, 8), (3, 4, 1), (1, 1, 6), (0, 7, 1)],
            8: [(1, 0, 2, 0, 1, 1, 0, 3), (1, 1, 1, 1, 1, 1, 1, 1), (0, 0, 0, 0, 0, 0, 0, 8), (0, 3, 0, 0, 2, 0, 2, 1)]}
_START_EIGHTHS = {1: (8,), 2: (3, 5), 3: (1, 4, 3), 7: (1, 1, 1, 1, 1, 1, 2)}


def _eighth_thresholds(w):
    thr = (np.cumsum(np.asarray(w, dtype=np.uint64), axis=-1) << np.uint64(29)).astype(np.uint64)
    thr[..., -1] = 0xFFFFFFFF
    assert (thr <= 0xFFFFFFFF).all()
    return thr.astype(np.uint32)


def table_mdp(name):
    """A hand-built MDP in the encoded form (``TableMDP``): thresholds that are multiples of 2^29, so every slot's weight is
    a multiple of 1/8 -- some of them 0, which ``encode_table_mdp`` would have compacted away -- and every slot of every
    cell has a reward of its own (``cell * K + slot`` eighths, minus 3), so a result names the slot that was drawn."""
    from dist_classicrl_amd.environments.device_envs import TableMDP

    S, A, K, n_start, masked = TABLE_SHAPES[name]
    s, a, k = np.meshgrid(np.arange(S), np.arange(A), np.arange(K), indexing="ij")
    cell = s * A + a
    patterns = np.array(_EIGHTHS[K], dtype=np.int64)
    weights = patterns[(cell[..., 0] + s[..., 0]) % len(patterns)]
    slot = cell * K + k
    masks = None
    if masked:
        ms, ma = np.meshgrid(np.arange(S), np.arange(A), indexing="ij")
        masks = (((ms * A + ma) * 2654435761 >> 7) & 1) == 1
        masks[np.arange(S), (np.arange(S) * 11) % A] = True  # at least one valid action per state
    start_state = (np.arange(n_start) * (S // n_start)).astype(np.int32)
    mdp = TableMDP(thr=_eighth_thresholds(weights), next_state=((s * 5 + a * 3 + k * 7 + 1) % S).astype(np.int32),
                   reward=(slot / 8.0 - 3.0).astype(np.float32), terminated=(s + a + k) % 2 == 0,
                   start_thr=_eighth_thresholds(_START_EIGHTHS[n_start]), start_state=start_state, masks=masks)
    assert np.array_equal(mdp.outcome_weights(), weights.astype(np.uint64) << np.uint64(29))
    assert len(np.unique(mdp.reward)) == mdp.reward.size
    return mdp


def table_case(name, step, replicas=TABLE_D, seed=TABLE_SEED, agent_offset=0) -> Case:
    mdp = table_mdp(name)
    S, A, K = mdp.thr.shape
    cells = np.repeat(np.arange(S * A, dtype=np.int64), replicas)
    s, a = cells // A, cells % A
    env = TableMDPVecEnv(len(cells), mdp, seed=seed)
    env.agent_ids = agent_ids(agent_offset, len(cells))
    env.obs = s.astype(np.int32)
    env.step_index = int(step)
    start_masks = env.action_masks(env.obs).astype(bool) if env.masked else None
    nxt, reward, terminated, truncated, _ = env.step(a)
    assert not truncated.any()
    zeros = np.zeros(len(cells), dtype=np.uint32)
    return Case(obs=s.astype(np.int32), aux=zeros, actions=a.astype(np.int32), agent_offset=agent_offset, step=int(step),
                next_obs=(nxt["observation"] if env.masked else nxt).astype(np.int32), next_aux=zeros,
                reward=reward.astype(np.float32), terminated=terminated.astype(bool), start_masks=start_masks,
                masks=nxt["action_mask"].astype(bool) if env.masked else None, info={"mdp": mdp, "seed": seed})


# ---- two environments on one engine ---------------------------------------------------------------------------------
TWO_ENV = {"S": 50, "A": 8, "A_agents": 96, "B_agents": 64, "A_seed": 1, "B_seed": 2, "steps": 40, "more": 30}


def two_env_curriculum(first="A"):
    """One oracle algorithm and runtime (constant schedules, ``learn``) run `first` for 40 steps, then the other
    environment for 40 steps, then `first` for 30 more: table, draw counter and schedules are shared, as they are on one
    engine.  Returns per stage ``{"obs", "acc", "aux", "history"}`` of the environment that stage ran (copies)."""
    from helpers import schedule_params
    from oracle.qlearn_oracle import OracleQLearning, OracleRuntime, OracleSchedule

    p = TWO_ENV
    envs = {"A": HashTabularEnv(p["A_agents"], p["S"], p["A"], seed=p["A_seed"]),
            "B": HashTabularEnv(p["B_agents"], p["S"], p["A"], seed=p["B_seed"])}
    second = "B" if first == "A" else "A"
    algo = OracleQLearning(p["S"], p["A"], 0.99, seed=0, dtype=np.dtype("f4"))
    lr_p, eps_p = schedule_params("const")
    rt = OracleRuntime(algo, OracleSchedule(*lr_p), OracleSchedule(*eps_p), learn_mode="iter")
    state, stages = {}, []
    for name, steps in ((first, p["steps"]), (second, p["steps"]), (first, p["more"])):
        env = envs[name]
        if name not in state:
            obs, _ = env.reset()
            state[name] = (obs, np.zeros(env.num_agents, dtype=np.float32))
        obs, acc = state[name]
        history = []
        for _ in range(steps):
            obs, _ = rt.run_single_step(env, obs, acc, history)
        state[name] = (obs, acc)
        stages.append({"env": name, "obs": np.array(obs, dtype=np.int32), "acc": acc.copy(), "aux": env_aux(env).copy(),
                       "history": np.array(history, dtype=np.float32), "q": algo.q_table.copy(),
                       "step_counter": rt.step_counter})
    return stages
