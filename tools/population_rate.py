"""Aggregate env-steps/s of the population path (QLearningPopulation, k_rollout_runs) against the standalone one-agent
rollout on the same environment, measured in the same process.

    python tools/population_rate.py --out DIR [--steps 10000] [--dtype float32] [--quick] [--evaluate]
                                    [--rule q_learning|sarsa|expected_sarsa] [--n-step N] [--double] [--actions A]
                                    [--trace-decay LAMBDA [--trace-length K] [--trace-kind replacing|accumulating]]
                                    [--planning-steps N] [--exploration-bonus B] [--visit-lr] [--tree-backup N]

Workloads: a FrozenLake-8x8-slippery-like TabularMDPEnv (64 states x 4 actions, 3 outcomes per move, built here) at
M in {64, 1024, 4096, 65536} runs with and without the episode log; TicTacToe at M = 1024; a 1e4 x 8 HashTabularEnv at
M = 4096.  Rate = M x steps / wall time of one timed call (after a warm-up call; the call returns after the device has
finished).  Writes DIR/population_rate.json and prints one line per workload.  For kernel time and bytes per env-step,
run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/population_rate.py --out DIR --quick`.

--rule trains with that update rule (k_rollout_runs_td for sarsa / expected_sarsa; the standalone baseline is always
the Q-learning one-agent rollout) and writes DIR/population_rate_<rule>.json for a rule other than q_learning.
--n-step N (2 .. 16, with --rule sarsa / expected_sarsa) trains with the n-step form of the rule (k_nstep_rollout) and
writes DIR/population_rate_<rule>_n<N>.json.
--trace-decay LAMBDA (with --rule q_learning / sarsa) trains with eligibility traces (k_trace_rollout: Watkins's
Q(lambda) / SARSA(lambda)) of --trace-length K slots (default 16) and --trace-kind (default replacing), and writes
DIR/population_rate_<rule>_trace<K>.json.
--planning-steps N (1 .. 64, with --rule q_learning) trains with Dyna-Q (k_dyna_rollout): N planning updates from the
run's learned model after every step; writes DIR/population_rate_dyna<N>.json, with the event time per table update
(env-step time / (1 + N)) beside the time per env-step.
--exploration-bonus B (B >= 0) and --visit-lr (with --rule q_learning) train with visit counts (k_visit_rollout): the
bonus B / sqrt(N(s, a)) on the pick and / or the learning rate divided by N(s, a); writes DIR/population_rate_visit.json,
with the event time per env-step beside the wall rate.
--tree-backup N (2 .. 16, with --rule q_learning; 1 is the plain run) trains with n-step Tree Backup (k_tree_rollout) and
writes DIR/population_rate_tree<N>.json, with the event time per env-step beside the wall rate.
--double trains (or, with --evaluate, evaluates) a Double Q-learning population (double_q=True: k_double_rollout /
k_double_evaluate, two tables per run) against the same single-table standalone baseline and writes
DIR/population_rate_double.json (DIR/population_eval_rate_double.json).
--actions A adds a HashTabularEnv of 1e4 states x A actions at M = 4096 (the wide-row builds: A = 64 is NV = 16).

--evaluate measures greedy evaluation instead (QLearningPopulation.evaluate_steps, k_evaluate_runs) on the same
workloads and M values, against the standalone one-agent evaluate_steps, after 200 training steps, and writes
DIR/population_eval_rate.json.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from dist_classicrl_amd.algorithms import QLearningPopulation  # noqa: E402
from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase  # noqa: E402
from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning  # noqa: E402
from dist_classicrl_amd.environments import HashTabularEnv, TabularMDPEnv, TicTacToeEnv  # noqa: E402
from dist_classicrl_amd.schedules import ExponentialSchedule  # noqa: E402

FROZEN_8x8 = ["SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF", "FFFHFFFG"]


def frozen_lake_8x8_slippery():
    """gymnasium's FrozenLake-v1 8x8, is_slippery=True, as a transition dict P[s][a] = [(p, s', r, terminated)]."""
    n = 8
    moves = {0: (0, -1), 1: (1, 0), 2: (0, 1), 3: (-1, 0)}  # left, down, right, up
    P = {}
    for s in range(n * n):
        row, col = divmod(s, n)
        P[s] = {}
        for a in range(4):
            out = []
            for b in ((a - 1) % 4, a, (a + 1) % 4):
                if FROZEN_8x8[row][col] in "GH":
                    out.append((1.0 / 3.0, s, 0.0, True))
                    continue
                dr, dc = moves[b]
                r2, c2 = min(max(row + dr, 0), n - 1), min(max(col + dc, 0), n - 1)
                cell = FROZEN_8x8[r2][c2]
                out.append((1.0 / 3.0, r2 * n + c2, 1.0 if cell == "G" else 0.0, cell in "GH"))
            P[s][a] = out
    isd = np.zeros(n * n)
    isd[0] = 1.0
    return P, isd


def schedules():
    return ExponentialSchedule(0.1, 1e-3, 0.9995), ExponentialSchedule(1.0, 0.05, 0.9995)


def population_rate(make_env, M, S, A, steps, dtype, log, rule="q_learning", double_q=False, n_step=1, traces=None,
                    planning=0, bonus=None, visit_lr=False, tree_backup=1):
    lr, eps = schedules()
    kw = {} if rule == "q_learning" else {"update_rule": rule}
    if n_step != 1:
        kw["n_step"] = n_step
    if double_q:
        kw["double_q"] = True
    if traces is not None:
        kw.update(trace_decay=traces[0], trace_length=traces[1], trace_kind=traces[2])
    if planning:
        kw["planning_steps"] = planning
    if bonus is not None:
        kw["exploration_bonus"] = bonus
    if visit_lr:
        kw["visit_lr"] = True
    if tree_backup != 1:
        kw["tree_backup"] = tree_backup
    pop = QLearningPopulation(M, S, A, 0.99, lr, eps, seed=1, dtype=dtype, **kw)
    env = make_env(M)
    res = pop.run_steps(min(200, steps), env, log=log)  # warm-up: code objects, allocations
    t0 = time.perf_counter()
    res = pop.run_steps(steps, env, res.state_dict, log=log)
    wall = time.perf_counter() - t0
    return {"runs": M, "steps": steps, "wall_s": wall, "env_steps_per_s": M * steps / wall,
            "kernel_ms": pop.last_stats["kernel_ms"], "launches": int(pop.last_stats["launches"]),
            "episodes": int(res.episode_counts.sum()), "kernel_variant": int(pop.last_stats["kernel_variant"])}


def population_eval_rate(make_env, M, S, A, steps, dtype, log, double_q=False):
    lr, eps = schedules()
    pop = QLearningPopulation(M, S, A, 0.99, lr, eps, seed=1, dtype=dtype, **({"double_q": True} if double_q else {}))
    pop.run_steps(200, make_env(M), log=False)  # tables that are not all zero
    env = make_env(M)
    pop.evaluate_steps(env, min(200, steps), log=log)  # warm-up: code objects, allocations
    t0 = time.perf_counter()
    res = pop.evaluate_steps(env, steps, log=log)
    wall = time.perf_counter() - t0
    return {"runs": M, "steps": steps, "wall_s": wall, "env_steps_per_s": M * steps / wall,
            "kernel_ms": pop.last_stats["kernel_ms"], "launches": int(pop.last_stats["launches"]),
            "episodes": int(res.episode_counts.sum()), "kernel_variant": int(pop.last_stats["kernel_variant"])}


def standalone_eval_rate(make_env, S, A, steps, dtype):
    lr, eps = schedules()
    algo = OptimalQLearningBase(S, A, 0.99, seed=1, dtype=dtype)
    rt = GpuRolloutQLearning(algo, lr, eps)
    rt.history_type = "array"
    rt.run_steps(200, make_env(1))
    env = make_env(1)
    rt.evaluate_steps(env, min(200, steps))
    t0 = time.perf_counter()
    rt.evaluate_steps(env, steps)
    wall = time.perf_counter() - t0
    return {"steps": steps, "wall_s": wall, "env_steps_per_s": steps / wall}


def standalone_rate(make_env, S, A, steps, dtype):
    lr, eps = schedules()
    algo = OptimalQLearningBase(S, A, 0.99, seed=1, dtype=dtype)
    rt = GpuRolloutQLearning(algo, lr, eps)
    rt.history_type = "array"
    env = make_env(1)
    _, _, _, sd = rt.run_steps(min(200, steps), env)
    t0 = time.perf_counter()
    rt.run_steps(steps, env, sd)
    wall = time.perf_counter() - t0
    return {"steps": steps, "wall_s": wall, "env_steps_per_s": steps / wall}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, type=Path)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--dtype", choices=["float32", "float64"], default="float32")
    ap.add_argument("--quick", action="store_true", help="fewer steps and shapes (profiling runs)")
    ap.add_argument("--evaluate", action="store_true", help="greedy evaluation (evaluate_steps) instead of training")
    ap.add_argument("--rule", choices=["q_learning", "sarsa", "expected_sarsa"], default="q_learning",
                    help="update rule of the trained population (not with --evaluate: evaluation does not depend on it)")
    ap.add_argument("--n-step", type=int, default=1, help="bootstrapping horizon of the on-policy rules (1 .. 16)")
    ap.add_argument("--double", action="store_true", help="Double Q-learning: two tables per run (q_learning only)")
    ap.add_argument("--trace-decay", type=float, default=None, help="lambda of the eligibility traces (default: none)")
    ap.add_argument("--trace-length", type=int, default=16, help="trace slots per run (1 .. 32)")
    ap.add_argument("--trace-kind", choices=["replacing", "accumulating"], default="replacing")
    ap.add_argument("--planning-steps", type=int, default=0, help="Dyna-Q planning updates per step (0 .. 64; q_learning only)")
    ap.add_argument("--exploration-bonus", type=float, default=None, help="beta of the count-based bonus beta / sqrt(N(s, a)) (q_learning only)")
    ap.add_argument("--visit-lr", action="store_true", help="learning rate divided by the visit count N(s, a) (q_learning only)")
    ap.add_argument("--tree-backup", type=int, default=1, help="horizon of n-step Tree Backup (1 .. 16; q_learning only)")
    ap.add_argument("--actions", type=int, default=0, help="also measure a 1e4-state HashTabularEnv with this many actions")
    args = ap.parse_args()
    if args.evaluate and args.rule != "q_learning":
        ap.error("--rule applies to training runs only")
    if args.double and args.rule != "q_learning":
        ap.error("--double is Double Q-learning: it goes with --rule q_learning")
    if args.n_step != 1 and (args.rule == "q_learning" or args.evaluate):
        ap.error("--n-step goes with --rule sarsa or expected_sarsa (training runs)")
    if args.trace_decay is not None and (args.rule == "expected_sarsa" or args.double or args.n_step != 1 or args.evaluate):
        ap.error("--trace-decay goes with --rule q_learning or sarsa (training runs), without --double and --n-step")
    if args.planning_steps and (args.rule != "q_learning" or args.double or args.n_step != 1 or args.trace_decay is not None
                                or args.evaluate):
        ap.error("--planning-steps goes with --rule q_learning (training runs), without --double, --n-step and --trace-decay")
    counting = args.exploration_bonus is not None or args.visit_lr
    if counting and (args.rule != "q_learning" or args.double or args.n_step != 1 or args.trace_decay is not None or args.planning_steps
                     or args.evaluate):
        ap.error("--exploration-bonus and --visit-lr go with --rule q_learning (training runs), without --double, --n-step, "
                 "--trace-decay and --planning-steps")
    if args.tree_backup != 1 and (args.rule != "q_learning" or args.double or args.n_step != 1 or args.trace_decay is not None
                                  or args.planning_steps or counting or args.evaluate):
        ap.error("--tree-backup goes with --rule q_learning (training runs), without --double, --n-step, --trace-decay, "
                 "--planning-steps, --exploration-bonus and --visit-lr")
    traces = None if args.trace_decay is None else (args.trace_decay, args.trace_length, args.trace_kind)
    dtype = np.dtype(args.dtype)
    steps = 1000 if args.quick else args.steps
    P, isd = frozen_lake_8x8_slippery()

    def lake(n):
        return TabularMDPEnv.from_transition_dict(P, n, initial_state_distrib=isd, seed=1)

    def ttt(n):
        return TicTacToeEnv(n, seed=1)

    def hashed(n):
        return HashTabularEnv(n, 10000, 8, seed=1)

    plan = [("frozenlake8x8", lake, 64, 4, M, steps, log) for M in ((4096, 65536) if args.quick else (64, 1024, 4096, 65536))
            for log in (True, False)]
    plan += [("tictactoe", ttt, 19683, 9, 1024, steps // 5, True), ("hash1e4x8", hashed, 10000, 8, 4096, steps, True)]
    if args.actions:
        plan.append((f"hash1e4x{args.actions}", lambda n: HashTabularEnv(n, 10000, args.actions, seed=1), 10000, args.actions,
                     4096, steps, True))
    base_cache = {}
    lines = []
    for name, make_env, S, A, M, k, log in plan:
        if name not in base_cache:
            base_cache[name] = (standalone_eval_rate if args.evaluate else standalone_rate)(make_env, S, A, min(k, 5000), dtype)
        if args.evaluate:
            pop = population_eval_rate(make_env, M, S, A, k, dtype, log, args.double)
        else:
            pop = population_rate(make_env, M, S, A, k, dtype, log, args.rule, args.double, args.n_step, traces,
                                  args.planning_steps, args.exploration_bonus, args.visit_lr, args.tree_backup)
            if args.tree_backup != 1:
                pop["tree_backup"] = args.tree_backup
                pop["event_ns_per_env_step"] = pop["kernel_ms"] * 1e6 / (pop["runs"] * pop["steps"])
            if counting:
                pop["exploration_bonus"] = args.exploration_bonus
                pop["visit_lr"] = args.visit_lr
                pop["event_ns_per_env_step"] = pop["kernel_ms"] * 1e6 / (pop["runs"] * pop["steps"])
            if args.planning_steps:
                pop["planning_steps"] = args.planning_steps
                pop["event_ns_per_env_step"] = pop["kernel_ms"] * 1e6 / (pop["runs"] * pop["steps"])
                pop["event_ns_per_table_update"] = pop["event_ns_per_env_step"] / (1 + args.planning_steps)
        base = base_cache[name]
        line = {"workload": name, "evaluate": args.evaluate, "rule": args.rule, **({"n_step": args.n_step} if args.n_step != 1 else {}), **({"trace_decay": traces[0], "trace_length": traces[1], "trace_kind": traces[2]} if traces else {}), **({"double": True} if args.double else {}), "dtype": args.dtype, "log": log, **pop, "standalone_env_steps_per_s": base["env_steps_per_s"],
                "speedup_vs_standalone": pop["env_steps_per_s"] / base["env_steps_per_s"]}
        lines.append(line)
        print(f"{name:14s} M={M:6d} log={int(log)} {pop['env_steps_per_s'] / 1e6:10.1f} M env-steps/s "
              f"(standalone {base['env_steps_per_s'] / 1e6:.3f} M/s, x{line['speedup_vs_standalone']:.0f}; "
              f"{pop['launches']} launches, kernel {pop['kernel_ms']:.1f} ms)", flush=True)
    args.out.mkdir(parents=True, exist_ok=True)
    name = "population_eval_rate.json" if args.evaluate else "population_rate.json"
    if args.rule != "q_learning":
        name = f"population_rate_{args.rule}.json" if args.n_step == 1 else f"population_rate_{args.rule}_n{args.n_step}.json"
    if traces:
        name = f"population_rate_{args.rule}_trace{args.trace_length}.json"
    if args.planning_steps:
        name = f"population_rate_dyna{args.planning_steps}.json"
    if counting:
        name = "population_rate_visit.json"
    if args.tree_backup != 1:
        name = f"population_rate_tree{args.tree_backup}.json"
    if args.double:
        name = name.replace(".json", "_double.json")
    (args.out / name).write_text(json.dumps(lines, indent=1))


if __name__ == "__main__":
    main()
