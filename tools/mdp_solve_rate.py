"""Diagnostic: device time per sweep of the dynamic-programming entry points (csrc/qe_mdp_solve.h).

    python tools/mdp_solve_rate.py [--out DIR] [--states 1000000] [--actions 16] [--runs 4096] [--reps 3]

Value iteration on random MDPs of `states` x `actions` with K = 1 and K = 8 outcome records per cell, and the policy
sweep of `runs` runs on a 64 x 4 MDP (K = 2).  Every figure is event time on the engine's stream around whole calls with
tol = 0 (no sweep is skipped): per sweep = (time of 192 sweeps - time of 64 sweeps) / 128, which cancels the call's fixed
cost and keeps the one host synchronisation per batch of 32 sweeps that a real call pays.  Beside it: the bytes a sweep
moves by definition, the share of the HBM peak they imply, and the NumPy model's time per sweep on one host core
(tests/mdp_solver_model.py, timed on `--model-states` states and scaled to `states`).  Needs a GPU; writes
DIR/mdp_solve_rate.json.

The host-core column is the test suite's model: this tool puts tests/ on sys.path and imports `mdp_solver_model` from
there, so it runs from a source checkout only and is a diagnostic, not part of the installed package.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np
import torch

import mdp_solver_model as model
from dist_classicrl_amd import _lib
from dist_classicrl_amd.algorithms import QLearningPopulation
from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
from dist_classicrl_amd.environments.device_envs import TableMDP, TabularMDPEnv

HBM_PEAK = 8.0e12  # bytes/s, MI355X data sheet
SHORT, LONG = 64, 192


def random_table_mdp(S, A, K, seed):
    """A random encoded MDP built slot by slot (no float64 probability arrays: 1.3e8 slots at the largest shape)."""
    rng = np.random.default_rng(seed)
    thr = np.sort(rng.integers(0, 1 << 32, size=(S, A, K), dtype=np.uint32), axis=-1)
    thr[..., -1] = 0xFFFFFFFF
    nxt = rng.integers(0, S, size=(S, A, K), dtype=np.int32)
    rew = rng.standard_normal((S, A, K), dtype=np.float32)
    term = rng.random((S, A, K), dtype=np.float32) < 0.02
    return TableMDP(thr, nxt, rew, term, np.array([0xFFFFFFFF], np.uint32), np.array([0], np.int32), None)


def event_ms(stream, call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record(stream)
        rc = call()
        t1.record(stream)
    t1.synchronize()
    _lib.check(rc)
    return t0.elapsed_time(t1)


def per_sweep_us(stream, call, reps):
    call(SHORT)  # warm-up: code objects, allocator
    out = []
    for _ in range(reps):
        short = event_ms(stream, lambda: call(SHORT))
        long_ = event_ms(stream, lambda: call(LONG))
        out.append(1e3 * (long_ - short) / (LONG - SHORT))
    return sorted(out)


def model_seconds_per_sweep(mdp, sweep, reps=2):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        sweep()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_outputs")
    ap.add_argument("--states", type=int, default=1_000_000)
    ap.add_argument("--actions", type=int, default=16)
    ap.add_argument("--runs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model-states", type=int, default=100_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures device time and has no fallback")
    lib = _lib.load()
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    results = []
    S, A = args.states, args.actions
    for K in (1, 8):
        algo = OptimalQLearningBase(S, A, 0.99, seed=0)
        _lib.check(lib.qe_set_stream(algo.handle, C.c_void_p(stream.cuda_stream)))
        env = TabularMDPEnv(1, random_table_mdp(S, A, K, seed=K)).bind(algo)
        us = per_sweep_us(stream, lambda n: lib.qe_env_table_solve(env.handle, 0.99, 0.0, n, None, None, None, None), args.reps)
        small = random_table_mdp(args.model_states, A, K, seed=K)
        law = model.law_of(small)
        v = np.zeros(args.model_states)
        host = model_seconds_per_sweep(small, lambda: model.row_max(model.backup(law, v, 0.99), law.valid)) * S / args.model_states
        unique = S * A * K * 16 + 2 * S * 8
        results.append({"what": "value_iteration", "states": S, "actions": A, "k": K, "us_per_sweep": us,
                        "bytes_per_sweep": unique, "gathered_value_bytes": S * A * K * 8,
                        "hbm_fraction": unique / (us[len(us) // 2] * 1e-6) / HBM_PEAK, "model_s_per_sweep_one_core": host,
                        "model_timed_on_states": args.model_states})
        print(json.dumps(results[-1]), flush=True)
        env.close()
        del env, algo
    M, S2, A2, K2 = args.runs, 64, 4, 2
    mdp = random_table_mdp(S2, A2, K2, seed=3)
    pop = QLearningPopulation(M, S2, A2, 0.99, seed=0)
    _lib.check(lib.qe_set_stream(pop.handle, C.c_void_p(stream.cuda_stream)))
    tables = np.random.default_rng(3).integers(0, 2, size=(M, S2, A2)).astype(np.float64)
    pop.set_q_tables(tables)
    env = TabularMDPEnv(M, mdp).bind(pop)
    us = per_sweep_us(stream, lambda n: lib.qe_population_policy_values(pop.handle, env.handle, None, 0.0, n, None, None, None, None),
                      args.reps)
    law = model.law_of(mdp)
    G, _ = model.tie_sets(law, tables)
    host = model_seconds_per_sweep(mdp, lambda: model.policy_values(mdp, tables, 0.99, 0.0, 1, law=law))
    requested = int(G.sum()) * K2 * 16 + M * S2 * 8 * 3  # the tie sets' records, values in and out, the tie-set words
    unique = S2 * A2 * K2 * 16 + M * S2 * 8 * 3          # ... of which the records are one small table shared by every run
    results.append({"what": "policy_sweep", "runs": M, "states": S2, "actions": A2, "k": K2, "us_per_sweep": us,
                    "bytes_per_sweep_requested": requested, "bytes_per_sweep": unique,
                    "hbm_fraction": unique / (us[len(us) // 2] * 1e-6) / HBM_PEAK, "model_s_per_sweep_one_core": host})
    print(json.dumps(results[-1]), flush=True)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "mdp_solve_rate.json").write_text(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
