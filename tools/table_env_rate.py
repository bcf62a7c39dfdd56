"""Env-steps/s of the table-driven device environment (TabularMDPEnv) against the alternatives:

* FrozenLake-8x8 (slippery) at 128 and 4096 agents: the device table env (fused rollout) vs the same MDP as a NumPy
  vector env, which GpuRolloutQLearning.run_steps drives through its host path (one round trip per vector step);
* GridLakeEnv(side=10) vs its table equivalent at 128 agents: the cost of the table load inside the fused step.

    python tools/table_env_rate.py [--steps N]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))  # the MDPs the tests use (FrozenLake's P, GridLake as dense tables)
from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase  # noqa: E402
from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning  # noqa: E402
from dist_classicrl_amd.environments import GridLakeEnv, TabularMDPEnv  # noqa: E402
from dist_classicrl_amd.environments.device_envs import encode_table_mdp, outcome_arrays  # noqa: E402
from dist_classicrl_amd.schedules import ExponentialSchedule  # noqa: E402
from table_mdp_model import FROZEN_8x8, frozen_lake_P, grid_lake_tables  # noqa: E402


class NumpyTableEnv:
    """The same MDP as a plain NumPy vector env (SAME_STEP autoreset), for the host path."""

    def __init__(self, num_agents, probs, nxt, rew, term, seed=1):
        self.num_agents, self.state_size, self.action_size = num_agents, probs.shape[0], probs.shape[1]
        self.cum = np.cumsum(probs, axis=-1) / probs.sum(axis=-1, keepdims=True)
        self.nxt, self.rew, self.term = nxt, rew.astype(np.float32), term
        self.rng = np.random.default_rng(seed)
        self.obs = np.zeros(num_agents, dtype=np.int32)

    def __len__(self):
        return self.num_agents

    def reset(self, seed=None, options=None):  # noqa: ARG002
        self.obs[:] = 0
        return self.obs.copy(), [{}] * self.num_agents

    def step(self, actions):
        a = np.asarray(actions, dtype=np.int64)
        u = self.rng.random(self.num_agents)
        k = np.minimum((u[:, None] >= self.cum[self.obs, a]).sum(axis=1), self.cum.shape[2] - 1)
        nxt, r, te = self.nxt[self.obs, a, k], self.rew[self.obs, a, k], self.term[self.obs, a, k]
        self.obs = np.where(te, 0, nxt).astype(np.int32)
        n = self.num_agents
        return self.obs.copy(), r, te.astype(bool), np.zeros(n, dtype=bool), [{}] * n


def rate(env, state_size, steps, warmup):
    algo = OptimalQLearningBase(state_size, 4, 0.99, seed=0)
    rt = GpuRolloutQLearning(algo, ExponentialSchedule(0.1, 1e-5, 0.995), ExponentialSchedule(1.0, 0.01, 0.995))
    _, _, _, sd = rt.run_steps(warmup, env, None)
    t0 = time.perf_counter()
    rt.run_steps(steps, env, sd)
    el = time.perf_counter() - t0
    return len(env) * steps / el


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--host-steps", type=int, default=200)
    args = ap.parse_args()
    arrays = outcome_arrays(frozen_lake_P(FROZEN_8x8, is_slippery=True))
    mdp = encode_table_mdp(*arrays)
    print(f"{'case':44s} {'env-steps/s':>14s}")
    for n in (128, 4096):
        dev = rate(TabularMDPEnv(n, mdp, seed=1), 64, args.steps, 200)
        host = rate(NumpyTableEnv(n, *arrays), 64, args.host_steps, 20)
        print(f"{f'FrozenLake-8x8 slippery, {n} agents, device table':44s} {dev:14.4g}")
        print(f"{f'FrozenLake-8x8 slippery, {n} agents, NumPy host':44s} {host:14.4g}   device / host = {dev / host:.1f}x")
    built_in = rate(GridLakeEnv(128, side=10, seed=1), 100, args.steps * 5, 500)
    nxt, rew, term = grid_lake_tables(10, seed=1)
    table = rate(TabularMDPEnv.from_arrays(128, nxt, rew, term, seed=1), 100, args.steps * 5, 500)
    print(f"{'GridLake side 10, 128 agents, GridLakeEnv':44s} {built_in:14.4g}")
    print(f"{'GridLake side 10, 128 agents, table':44s} {table:14.4g}   built-in / table = {built_in / table:.2f}x")


if __name__ == "__main__":
    main()
