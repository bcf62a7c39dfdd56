"""NumPy model of the table-driven device environment (``TabularMDPEnv``, ``csrc/qe_envs.h:TableEnv``).

Test infrastructure: it restates the environment's semantics so that ``oracle.qlearn_oracle.OracleRuntime`` can drive
it as it drives ``oracle.envs.TicTacToeVecEnv``.  It consumes the encoded form (``encode_table_mdp``), whose thresholds
the CPU tests check on hand-computed cases.

    h0    = mix32(mix32(agent ^ seed ^ C_TABLE) + step_lo * 0x9E3779B9 + step_hi)    (TttEnv::word0 with C_TABLE)
    step  : u = mix32(h0 ^ C_TABLE_STEP); outcome = first slot with u < thr, else the last slot
    start : u = mix32(h0 ^ C_TABLE_START); state = first support entry below the last with u < start_thr, else the last
            (after a termination, with h0 of that step; on reset, with h0 of the reserved step 2**64 - 1)

SAME_STEP autoreset; nothing truncates; the env keeps no per-agent state beyond the observation (aux = 0).
"""

from __future__ import annotations

import numpy as np

from oracle.draws import mix32
from oracle.envs import _VecEnvBase

C_TABLE = 0x3C6EF372
C_TABLE_STEP = 0x27D4EB2F
C_TABLE_START = 0x165667B1
RESET_STEP = 0xFFFFFFFFFFFFFFFF


class TableMDPVecEnv(_VecEnvBase):
    def __init__(self, num_agents, mdp, seed=1, agent_offset=0):
        self.num_agents = int(num_agents)
        self.mdp = mdp
        self.state_size, self.action_size = mdp.thr.shape[:2]
        self.masked = mdp.masks is not None
        self.seed = int(seed) & 0xFFFFFFFF
        self.agent_ids = np.arange(agent_offset, agent_offset + self.num_agents, dtype=np.uint32)
        self.obs = np.zeros(self.num_agents, dtype=np.int32)
        self.step_index = 0  # vector step of the draw protocol the next step() belongs to

    def _h0(self, step):
        inner = mix32(self.agent_ids ^ np.uint32(self.seed ^ C_TABLE)).astype(np.uint64)
        mixed = inner + np.uint64(step & 0xFFFFFFFF) * np.uint64(0x9E3779B9) + np.uint64(step >> 32)
        return mix32(mixed & np.uint64(0xFFFFFFFF))

    def _start(self, h0):
        u = mix32(h0 ^ np.uint32(C_TABLE_START))
        # the number of thresholds (all but the last entry's) that are <= u = the first entry with u < thr
        idx = np.searchsorted(self.mdp.start_thr[:-1], u, side="right")
        return self.mdp.start_state[idx].astype(np.int32)

    def action_masks(self, obs):
        return self.mdp.masks[np.asarray(obs)].astype(np.int8)

    def reset(self, seed=None, options=None):  # noqa: ARG002
        if seed is not None:
            self.seed = int(seed) & 0xFFFFFFFF
        self.obs = self._start(self._h0(RESET_STEP))
        return self._wrap(self.obs), [{} for _ in range(self.num_agents)]

    def step(self, actions):
        h0 = self._h0(self.step_index)
        self.step_index += 1
        a = np.asarray(actions, dtype=np.int64)
        thr = self.mdp.thr[self.obs, a]  # [n, K]
        u = mix32(h0 ^ np.uint32(C_TABLE_STEP))
        below = u[:, None] < thr
        k = np.where(below.any(axis=1), below.argmax(axis=1), thr.shape[1] - 1)
        nxt = self.mdp.next_state[self.obs, a, k].astype(np.int32)
        rewards = self.mdp.reward[self.obs, a, k].astype(np.float32)
        terminated = self.mdp.terminated[self.obs, a, k].astype(bool)
        self.obs = np.where(terminated, self._start(h0), nxt).astype(np.int32)
        n = self.num_agents
        return self._wrap(self.obs), rewards, terminated, np.zeros(n, dtype=bool), [{}] * n


# ---- MDPs the tests use ---------------------------------------------------------------------------------------------
FROZEN_4x4 = ["SFFF", "FHFH", "FFFH", "HFFG"]
FROZEN_8x8 = ["SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF", "FFFHFFFG"]


def frozen_lake_P(desc, is_slippery):
    """gymnasium's FrozenLake dynamics, restated: ``P[s][a] = [(prob, next_state, reward, terminated), ...]`` with
    actions 0 left, 1 down, 2 right, 3 up; a slippery move goes in the intended direction or either perpendicular one,
    1/3 each (duplicates are listed separately, as gymnasium does)."""
    nrow, ncol = len(desc), len(desc[0])
    P = {s: {a: [] for a in range(4)} for s in range(nrow * ncol)}

    def inc(r, c, a):
        if a == 0:
            c = max(c - 1, 0)
        elif a == 1:
            r = min(r + 1, nrow - 1)
        elif a == 2:
            c = min(c + 1, ncol - 1)
        else:
            r = max(r - 1, 0)
        return r, c

    for r in range(nrow):
        for c in range(ncol):
            s = r * ncol + c
            for a in range(4):
                li = P[s][a]
                if desc[r][c] in "GH":
                    li.append((1.0, s, 0.0, True))
                    continue
                for b in ([(a - 1) % 4, a, (a + 1) % 4] if is_slippery else [a]):
                    nr, nc = inc(r, c, b)
                    ns = nr * ncol + nc
                    li.append((1.0 / 3.0 if is_slippery else 1.0, ns, float(desc[nr][nc] == "G"), desc[nr][nc] in "GH"))
    return P


def frozen_lake_isd(desc):
    flat = np.array(list("".join(desc)))
    isd = (flat == "S").astype(np.float64)
    return isd / isd.sum()


def random_mdp(S, A, K, seed, masked=False, start_support=7):
    """A random stochastic MDP in outcome-array form ([S, A, K], some zero-probability slots) plus a start
    distribution over `start_support` states and, if `masked`, per-state masks with at least one valid action."""
    rng = np.random.default_rng(seed)
    probs = rng.random((S, A, K))
    probs[rng.random((S, A, K)) < 0.2] = 0.0
    probs[..., 0] += 0.01  # every (s, a) keeps an outcome of positive probability
    nxt = rng.integers(0, S, size=(S, A, K))
    rew = rng.standard_normal((S, A, K)).astype(np.float32)
    term = rng.random((S, A, K)) < 0.05
    isd = np.zeros(S)
    isd[rng.choice(S, size=start_support, replace=False)] = rng.random(start_support) + 0.1
    masks = None
    if masked:
        masks = rng.random((S, A)) < 0.5
        masks[np.arange(S), rng.integers(0, A, size=S)] = True
    return (probs, nxt, rew, term), isd, masks


def grid_lake_tables(side, seed=1):
    """``GridLakeEnv(side, seed)``'s dynamics (``oracle/envs.py:GridLakeEnv``) as dense [S, A] arrays: the table
    equivalent of the built-in environment (deterministic, start state 0)."""
    from oracle.envs import GridLakeEnv

    S = side * side
    holes = GridLakeEnv(1, side=side, seed=seed).holes()
    row, col = np.divmod(np.arange(S)[:, None], side)
    a = np.arange(4)[None, :]
    col = np.clip(col + (a == 2) - (a == 0), 0, side - 1)
    row = np.clip(row + (a == 1) - (a == 3), 0, side - 1)
    n = row * side + col
    goal = n == S - 1
    term = goal | holes[n]
    return np.where(term, 0, n), goal.astype(np.float32), term
