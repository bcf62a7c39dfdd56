"""GPU: standalone greedy evaluation (``k_eval``, csrc/qe_kernels.h, and the launch protocol of
``GpuRolloutQLearning.evaluate_steps`` / ``evaluate_episodes``) and ``train`` against the REAL reference's recorded
results (``tests/golden/eval.npz``) and, at fresh seeds and agent offsets, against the oracle that
``tests/test_oracle_eval_golden.py`` pins to the same records.  Every comparison is exact.

The cases (``tests/golden/make_golden_cases.py``) walk the row widths 1 .. 64 lanes, both dtypes, masked and unmasked,
both sides of the list / NumPy selection threshold (10 actions), NaN tables, ties on most picks, a step index that
crosses 2**32, and episode targets that need three launches and stop inside a step in which several agents finish.
This file reads ``tests/golden/`` and ``oracle/`` only."""

import numpy as np
import pytest

from golden.make_golden_cases import EVAL_CASES, EVAL_SEED, TRAIN_CASES, eval_table, tie_rich_table
from helpers import (GOLDEN, golden_eval_record, golden_train_record, masks_of_every_state, run_oracle_eval,
                     run_oracle_train, schedule_params, spec_shape, _oracle_runtime)
from oracle.envs import clock_env, env_aux, make_env

pytestmark = pytest.mark.gpu

EVAL_RECORDS = [(c[0], mode) for c in EVAL_CASES for mode in ("steps", "episodes") if mode == "steps" or c[7] is not None]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "eval.npz")


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return OptimalQLearningBase, GpuRolloutQLearning, environments, schedules, _lib


def _device_env(spec, agent_offset=0):
    envs = _product()[2]
    kind = spec[0]
    if kind == "hash":
        extra = {"p_term_256": spec[5]} if len(spec) > 5 else {}
        return envs.HashTabularEnv(spec[1], spec[2], spec[3], seed=1, masked=spec[4], agent_offset=agent_offset, **extra)
    if kind == "ttt":
        return envs.TicTacToeEnv(spec[1], seed=1, agent_offset=agent_offset)
    env = envs.GridLakeEnv(spec[1], side=spec[2], seed=1) if kind == "grid" else envs.RiggedTwoArmedBanditVecEnv(spec[1], episode_len=spec[2])
    env._params.agent_offset = agent_offset  # (only the policy draws of these two depend on the agent's number)
    return env


def _runtime(spec, dt, sched="const", learn_mode="iter", seed=0, agent_offset=0, q0=None, start=0, max_eval_steps=5000):
    Algo, Runtime, _, sch, _lib = _product()
    S, A = spec_shape(spec)
    algo = Algo(S, A, 0.99, seed=seed, dtype=np.dtype(dt))
    if agent_offset:
        _lib.check(_lib.load().qe_set_agent_offset(algo.handle, agent_offset))
    if q0 is not None:
        algo.q_table = q0
    algo.step_counter = start

    def make(p):
        kind, value, lo, decay = p
        if kind == "exponential":
            return sch.ExponentialSchedule(value, lo, decay)
        return sch.LinearSchedule(value, decay) if kind == "linear" else sch.ConstantSchedule(value)

    lr_p, eps_p = schedule_params(sched)
    rt = Runtime(algo, make(lr_p), make(eps_p), learn_mode=learn_mode)
    inner, spent = rt._rollout, [0]

    def rollout(env, steps, learn, as_list=False):
        # an evaluation that does not end its episodes (a wrong pick can walk into a cycle) fails; it does not hang
        if not learn:
            spent[0] += steps
            assert spent[0] <= max_eval_steps, f"more than {max_eval_steps} greedy vector steps on this runtime"
        return inner(env, steps, learn, as_list)

    rt._rollout = rollout
    return rt


def _env_state(env):
    states, acc = env.observe()
    return (states["observation"] if isinstance(states, dict) else states), env.aux(), acc


def _evaluate(rt, env, mode, count):
    """(raised, total, history float32, observations, env-internal state, running returns, step counter)."""
    _lib = _product()[4]
    try:
        total, history = getattr(rt, "evaluate_" + mode)(env, count)
    except IndexError:
        return {"raised": True}
    assert _lib.decode_variant(rt.last_stats["kernel_variant"])["path"] == "eval", rt.last_stats
    obs, aux, acc = _env_state(env)
    return {"raised": False, "total": total, "history": np.array(history, dtype=np.float32), "obs": obs, "aux": aux,
            "acc": acc, "step_counter": rt.algorithm.step_counter}


def _same_evaluation(got, want, start, label):
    assert got["raised"] == want["raised"], label
    if want["raised"]:
        return
    assert np.array_equal(got["history"], want["history"]), (label, "history")
    assert float(got["total"]) == float(want["total"]), (label, "total", got["total"], want["total"])
    assert np.array_equal(got["obs"], want["obs"]), (label, "observations")
    assert np.array_equal(got["aux"], want["aux"]), (label, "environment-internal state")
    assert got["step_counter"] == start + want["calls"], (label, "step counter", got["step_counter"], start, want["calls"])
    if want.get("acc") is not None:
        assert np.array_equal(got["acc"], want["acc"]), (label, "running returns")


def _case(name):
    _, spec, dt, table, start, vsteps, extra, episodes, raises = next(c for c in EVAL_CASES if c[0] == name)
    S, A = spec_shape(spec)
    q0 = eval_table(table, S, A, np.dtype(dt), masks_of_every_state(spec) if spec[0] == "hash" else None)
    return spec, dt, q0, start, {"steps": vsteps * spec[1] + extra, "episodes": episodes}, raises


# ---------------------------------------------------------------------------------------------- 1. the reference's records
@pytest.mark.parametrize(("name", "mode"), EVAL_RECORDS)
def test_evaluation_matches_the_reference(golden, name, mode):
    spec, dt, q0, start, counts, raises = _case(name)
    want = golden_eval_record(golden, name, mode)
    rt = _runtime(spec, dt, seed=EVAL_SEED, q0=q0, start=start)
    env = _device_env(spec)
    got = _evaluate(rt, env, mode, counts[mode])
    _same_evaluation(got, want, start, (name, mode))
    assert np.array_equal(np.asarray(rt.algorithm.q_table), q0, equal_nan=True)  # evaluation does not learn
    if raises:
        # the engine is usable after the error: the same call on a clean table succeeds and matches the oracle
        S, A = spec_shape(spec)
        clean = tie_rich_table(77, S, A, np.dtype(dt))
        rt.algorithm.q_table = clean
        rt.algorithm.step_counter = start
        again = _evaluate(rt, env, mode, counts[mode])
        _same_evaluation(again, run_oracle_eval(spec, dt, clean, start, mode, counts[mode], seed=EVAL_SEED), start,
                         (name, mode, "after the error"))


# ---------------------------------------------------------------------------------------------- 2. fresh seeds, offsets
@pytest.mark.parametrize("k", range(len(EVAL_CASES)), ids=[c[0] for c in EVAL_CASES])
def test_evaluation_matches_the_oracle_at_fresh_seeds_and_agent_offsets(k):
    name = EVAL_CASES[k][0]
    spec, dt, q0, start, counts, _ = _case(name)
    seed, offset = 0x5EED0000 + 977 * k, 3 + 61 * k
    start = start + 5 * k + 1
    rt = _runtime(spec, dt, seed=seed, agent_offset=offset, q0=q0, start=start)
    for mode in ("steps", "episodes"):
        if counts[mode] is None:
            continue
        # (the golden targets are tuned to the golden draws; at other draws the run still takes ~200 steps)
        want = run_oracle_eval(spec, dt, q0, start, mode, counts[mode], seed=seed, agent_offset=offset)
        rt.algorithm.step_counter = start
        got = _evaluate(rt, _device_env(spec, offset), mode, counts[mode])
        _same_evaluation(got, want, start, (name, mode))


# ---------------------------------------------------------------------------------------------- 3. between trainings
@pytest.mark.parametrize(("spec", "val_n", "dt", "mode"), [
    (("hash", 96, 500, 8, False), 150, "f4", "iter"),
    (("hash", 64, 300, 9, True), 100, "f8", "iter"),
    (("hash", 128, 2000, 16, False), 40, "f4", "vec"),
    (("ttt", 64), 90, "f4", "iter"),
])
def test_evaluation_between_trainings_on_one_engine_matches_the_oracle(spec, val_n, dt, mode):
    """Train on the persistent path, evaluate (steps), train on, evaluate (episodes), train on: the draw counter is
    handed from launch to launch and nothing of one path is left over for the other."""
    _lib = _product()[4]
    val_spec = (spec[0], val_n) + tuple(spec[2:])
    K = (25, 30, 20)
    rt = _runtime(spec, dt, sched="bench", learn_mode=mode, seed=9)
    rt.algorithm.set_rollout_path("persistent")
    rt.trace_actions = True  # (keeps run_steps off the one-call form: the launches are the persistent path's own)
    env = _device_env(spec)
    ora = _oracle_runtime(make_env(spec), dt, "bench", mode, 9, 0)
    oenv = clock_env(make_env(spec), lambda: ora.step_counter)
    sd = osd = None
    evals = (("steps", val_n * 20), ("episodes", 3 * val_n), None)
    for k, ev in zip(K, evals):
        _, history, _, sd = rt.run_steps(k, env, sd)
        assert _lib.decode_variant(rt.last_stats["kernel_variant"])["path"] == "persistent"
        _, ohistory, _, osd = ora.run_steps(k, oenv, osd)
        assert np.array_equal(np.array(history, np.float32), np.array(ohistory, np.float32))
        assert np.array_equal(np.asarray(rt.algorithm.q_table), ora.algorithm.q_table)
        assert rt.algorithm.step_counter == ora.step_counter
        if ev is not None:
            start = ora.step_counter
            want = run_oracle_eval(val_spec, dt, None, start, ev[0], ev[1], rt=ora)
            got = _evaluate(rt, _device_env(val_spec), ev[0], ev[1])
            _same_evaluation(got, want, start, (spec, ev))
    obs, aux, acc = _env_state(env)
    ostates = osd["states"]
    assert np.array_equal(obs, ostates["observation"] if isinstance(ostates, dict) else ostates)
    assert np.array_equal(aux, env_aux(oenv)) and np.array_equal(acc, osd["rewards"])


# ---------------------------------------------------------------------------------------------- 4. split launches
@pytest.mark.slow  # (the oracle's side takes most of a minute: deselect with -m "not slow")
def test_evaluate_steps_split_into_three_launches_matches_the_oracle():
    """One agent for 2 * chunk_limit + 1 vector steps: the smallest agents x steps that takes three launches (the
    limit is 65 536 steps per launch up to 64 agents and halves from 65 agents on, so more agents only cost more).  The
    oracle's side of this case (131 073 interpreted steps, each with its own Philox block in NumPy) measured 46 s of one
    CPU core; the engine's side is three launches."""
    spec = ("hash", 1, 50, 4, False, 40)
    dt, start, seed = "f4", 2**32 - 70000, 21
    q0 = tie_rich_table(5, 50, 4, np.dtype(dt))
    rt = _runtime(spec, dt, seed=seed, q0=q0, start=start, max_eval_steps=200000)
    env = _device_env(spec)
    env.bind(rt.algorithm)
    limit = env.chunk_limit(False)
    vsteps = 2 * limit + 1
    got = _evaluate(rt, env, "steps", vsteps)
    assert rt.last_stats["launches"] >= 3 and len(got["history"]) > 1000
    _same_evaluation(got, run_oracle_eval(spec, dt, q0, start, "steps", vsteps, seed=seed, max_calls=200000), start, "split")


# ---------------------------------------------------------------------------------------------- 5. train()
def _train(spec, val_n, dt, sched, learn_mode, steps, every, val, seed=0, agent_offset=0):
    rt = _runtime(spec, dt, sched=sched, learn_mode=learn_mode, seed=seed, agent_offset=agent_offset)
    env = _device_env(spec, agent_offset)
    val_env = _device_env((spec[0], val_n) + tuple(spec[2:]), agent_offset)
    kw = {"val_steps": val[1]} if val[0] == "steps" else {"val_episodes": val[1]}
    rewards, val_rewards, env_out, sd = rt.train(env, steps, val_env, every, **kw)
    assert env_out is env
    states = sd["states"]
    val_obs, val_aux, _ = _env_state(val_env)
    return {"reward_history": np.array(rewards, dtype=np.float32), "val_reward_history": np.array(val_rewards, dtype=np.float64),
            "q": np.asarray(rt.algorithm.q_table), "final_sched": np.array([rt.lr_schedule.get_value(), rt.exploration_rate_schedule.get_value()]),
            "obs": np.asarray(states["observation"] if isinstance(states, dict) else states), "aux": np.asarray(sd["aux"]),
            "agent_rewards": np.asarray(sd["rewards"]), "val_obs": val_obs, "val_aux": val_aux,
            "step_counter": rt.algorithm.step_counter, "fused": "kernel_variants" in rt.last_stats}


TRAIN_KEYS = ("reward_history", "val_reward_history", "q", "final_sched", "obs", "aux", "agent_rewards", "val_obs", "val_aux")


@pytest.mark.parametrize("name", [c[0] for c in TRAIN_CASES])
def test_train_matches_the_reference_and_the_oracle(golden, name):
    _, spec, val_n, dt, sched, learn_fn, steps, every, val = next(c for c in TRAIN_CASES if c[0] == name)
    mode = "vec" if learn_fn == "learn_vec" else "iter"
    want = golden_train_record(golden, name, spec_shape(spec), dt)
    got = _train(spec, val_n, dt, sched, mode, steps, every, val, seed=EVAL_SEED)
    for k in TRAIN_KEYS:
        assert np.array_equal(got[k], want[k]), (name, k)
    assert got["step_counter"] == want["calls"]
    # (a seed at which the trained policy of every case still ends its validation episodes: one that walks every agent
    # into a cycle without terminal state never reaches an episode target, in the reference as here)
    seed, offset = 0xABCD + 100 + len(name), 17
    want = run_oracle_train(spec, val_n, dt, sched, mode, steps, every, val, seed=seed, agent_offset=offset)
    got = _train(spec, val_n, dt, sched, mode, steps, every, val, seed=seed, agent_offset=offset)
    for k in TRAIN_KEYS:
        assert np.array_equal(got[k], want[k]), (name, k, "fresh seed")
    assert got["step_counter"] == want["step_counter"]
