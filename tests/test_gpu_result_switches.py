"""GPU: the engine's "tuning knobs (never change results)" switched away from their defaults, against the oracle.

``include/qlearn_engine.h`` declares ``QE_OPT_USE_GRAPH``, ``QE_OPT_HOST_BLOCK``, ``QE_OPT_EVENT_TIMING`` and
``QE_OPT_TURN_POLL`` and ``qe_create`` reads ``QE_USE_GRAPH``, ``QE_HOST_BLOCK``, ``QE_EVENT_TIMING``,
``QE_TOKEN_ROUNDS`` and ``QE_LISTED_MIN_AGENTS`` from the environment.  They are live switches: ``bench.py`` times the
headline with event timing off, the profiles are collected without graphs, and without the host result block a
persistent rollout has another chunk limit and fetches its control words, episode log and observations by stream
synchronisation and copies (``read_control``, ``fetch_episode_log``; no ``mirror_*`` shortcut for the state dict).
Every case here runs one such configuration as a user would (``run_steps``, call by call with the state dict handed
back, and as one pipelined call of three launches) and compares table, returns, observations, running returns and
draw counter with the oracle -- never one configuration with another.
"""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import run_oracle_trace
from test_gpu_shipped_builds import _assert_lane_build, _bench_runtime, _c_oracle_run, _product, _run_in_calls

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EP_CAP = 2**22


def _set(algo, _lib, options):
    for name, value in options.items():
        algo.set_engine_option(getattr(_lib, name), value)


def _run(rt, env, steps, calls):
    """`calls` = "20": run_steps in calls of 20 steps, the state dict handed back; "pipelined": ONE run_steps whose
    launches are 20 steps long, so that the call goes through qe_rollout_begin / qe_rollout_end three times (the
    history of numpy.float32 scalars keeps an unmasked call off the one-call path, which has no launches to pipeline)."""
    if calls == "pipelined":
        rt._PIPELINE_CHUNK = 20
        rt.history_type = "float32"
        out = _run_in_calls(rt, env, [steps])
        assert rt.last_stats["launches"] == -(-steps // 20) >= 3
        return out
    return _run_in_calls(rt, env, [20] * (steps // 20) + ([steps % 20] if steps % 20 else []))


def _same_results(algo, history, sd, ref, want, steps, masked=False):
    assert np.array_equal(np.asarray(algo.q_table), ref.q)
    assert np.array_equal(np.array(history, dtype=np.float32), want["history"])
    assert np.array_equal(sd["states"]["observation"] if masked else sd["states"], ref.obs)
    assert np.array_equal(sd["rewards"], ref.acc)
    assert sd["rng_step"] == steps == algo.step_counter


# ================================================================================================ host block / event timing
RESULT_SWITCHES = {
    "no-host-block": {"OPT_HOST_BLOCK": 0},
    "no-event-timing": {"OPT_EVENT_TIMING": 0},
    "neither": {"OPT_HOST_BLOCK": 0, "OPT_EVENT_TIMING": 0},
}


def _assert_switches_took_effect(rt, env, options):
    n = env.num_agents
    if options.get("OPT_HOST_BLOCK", 1) == 0:
        assert env.chunk_limit(True) == EP_CAP // n  # the device log's limit, not the host result block's
    else:
        assert env.chunk_limit(True) == 2**18 // n
        # the fast path without events reports the in-kernel clock, and nothing else, as the rollout's time
        assert rt.last_stats["kernel_ms"] == rt.last_stats["device_clock_ms"] > 0


@pytest.mark.parametrize("calls", ["20", "pipelined"])
@pytest.mark.parametrize("switches", list(RESULT_SWITCHES))
@pytest.mark.parametrize("ordered_path", [1, 2, 3])  # dataflow kernel / full build / sparse build
@pytest.mark.parametrize(("S", "contested"), [(60, True), (4000, False)])
def test_persistent_rollouts_without_host_block_or_event_timing(S, contested, ordered_path, switches, calls):
    _lib, Algo, Runtime, envs, sch = _product()
    n, A, steps, options = 128, 16, 60, RESULT_SWITCHES[switches]
    algo = Algo(S, A, 0.99, seed=0)
    algo.set_engine_option(_lib.OPT_LANE_ORDERED_PATH, ordered_path)
    _set(algo, _lib, options)
    rt = _bench_runtime(algo, sch, Runtime)
    env = envs.HashTabularEnv(n, S, A, seed=1)
    history, sd, variants, complex_steps = _run(rt, env, steps, calls)
    _assert_lane_build(_lib, variants, lean=1, choice=ordered_path, nv=A // 4, masked=False)
    assert not contested or complex_steps > steps // 2
    _assert_switches_took_effect(rt, env, options)
    ref, want = _c_oracle_run(n, S, A, steps)
    _same_results(algo, history, sd, ref, want, steps)


@pytest.mark.parametrize("calls", ["20", "pipelined"])
@pytest.mark.parametrize("switches", list(RESULT_SWITCHES))
def test_512_agent_rollouts_without_host_block_or_event_timing(switches, calls):
    _lib, Algo, Runtime, envs, sch = _product()
    n, S, A, steps, options = 512, 2000, 16, 60, RESULT_SWITCHES[switches]
    algo = Algo(S, A, 0.99, seed=0)
    _set(algo, _lib, options)
    rt = _bench_runtime(algo, sch, Runtime)
    env = envs.HashTabularEnv(n, S, A, seed=1)
    history, sd, variants, _ = _run(rt, env, steps, calls)
    for v in variants:
        d = _lib.decode_variant(v)
        assert d["path"] == "persistent" and d["cap512"] and d["lean"] == 0, d
    _assert_switches_took_effect(rt, env, options)
    ref, want = _c_oracle_run(n, S, A, steps)
    _same_results(algo, history, sd, ref, want, steps)


@pytest.fixture(scope="module")
def tictactoe_oracle():
    want = run_oracle_trace(("ttt", 64), 60, "f4", "bench", "iter")
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want


@pytest.mark.parametrize("calls", ["20", "pipelined"])
@pytest.mark.parametrize("switches", list(RESULT_SWITCHES))
def test_tictactoe_rollouts_without_host_block_or_event_timing(tictactoe_oracle, switches, calls):
    """A masked environment: ``run_steps`` goes through ``_rollout`` (begin / end), never the one-call path."""
    _lib, Algo, Runtime, envs, sch = _product()
    n, steps, options = 64, 60, RESULT_SWITCHES[switches]
    algo = Algo(19683, 9, 0.99, seed=0)
    _set(algo, _lib, options)
    rt = _bench_runtime(algo, sch, Runtime)
    env = envs.TicTacToeEnv(n, seed=1)
    history, sd, variants, _ = _run(rt, env, steps, calls)
    for v in variants:
        d = _lib.decode_variant(v)
        assert d["path"] == "persistent" and d["masked"] and d["lean"] == 1 and d["nv"] == 4, d
    _assert_switches_took_effect(rt, env, options)
    want = tictactoe_oracle
    assert np.array_equal(np.asarray(algo.q_table), want["q"])
    assert np.array_equal(np.array(history, dtype=np.float32), want["history"])
    assert np.array_equal(sd["states"]["observation"], want["final_obs"])
    assert np.array_equal(sd["rewards"], want["agent_rewards"])
    assert sd["rng_step"] == steps


# ================================================================================================ without HIP graphs
# (id, set_rollout_path, options, agents, states, the path that must run)
GRAPH_CASES = [
    ("stepwise", "stepwise", {}, 600, 900, "stepwise"),
    ("turnstile", "auto", {}, 600, 900, "turnstile"),
    ("wide-bitmaps", "wide", {}, 2100, 3000, "wide"),
    ("wide-lists", "wide", {"OPT_LISTED_MIN_AGENTS": 1, "OPT_TOKEN_ROUNDS": 7}, 2100, 3000, "wide"),
]
GRAPH_CALLS = [130, 130]  # by default each call would capture a graph of 50 steps and replay it; the second one resumes


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("case", GRAPH_CASES, ids=[c[0] for c in GRAPH_CASES])
def test_stepwise_kernels_launched_one_by_one(case, mode):
    """``QE_OPT_USE_GRAPH 0`` (how the profiles are collected): every kernel of every step is launched by the host."""
    _lib, Algo, Runtime, envs, sch = _product()
    _, path, options, n, S, want_path = case
    A, steps = 16, sum(GRAPH_CALLS)
    algo = Algo(S, A, 0.99, seed=0)
    algo.set_rollout_path(path)
    algo.set_engine_option(_lib.OPT_USE_GRAPH, 0)
    _set(algo, _lib, options)
    rt = Runtime(algo, sch.ExponentialSchedule(0.1, 1e-5, 0.995), sch.ExponentialSchedule(1.0, 0.01, 0.995), learn_mode=mode)
    history, sd, variants, _ = _run_in_calls(rt, envs.HashTabularEnv(n, S, A, seed=1), GRAPH_CALLS)
    assert {_lib.decode_variant(v)["path"] for v in variants} == {want_path}
    ref, want = _c_oracle_run(n, S, A, steps, mode=mode)
    _same_results(algo, history, sd, ref, want, steps)


# ================================================================================================ the turnstile's other poll
@pytest.mark.parametrize("forward", [0, 1])
@pytest.mark.parametrize("dt", ["f4", "f8"])
def test_turnstile_polling_with_loads(dt, forward):
    """``QE_OPT_TURN_POLL 1``: progress words polled with agent-scope loads, not returning atomics; 4096 agents on
    3000 rows hand every row on, with and without value forwarding (``QE_OPT_TURN_FORWARD``; float32 tables use it)."""
    _lib, Algo, Runtime, envs, sch = _product()
    n, S, A, steps = 4096, 3000, 16, 60
    algo = Algo(S, A, 0.99, seed=0, dtype=np.dtype(dt))
    _set(algo, _lib, {"OPT_TURN_POLL": 1, "OPT_TURN_FORWARD": forward})
    rt = _bench_runtime(algo, sch, Runtime)
    history, sd, variants, _ = _run_in_calls(rt, envs.HashTabularEnv(n, S, A, seed=1), [20, 20, 20])
    assert {_lib.decode_variant(v)["path"] for v in variants} == {"turnstile"}
    ref, want = _c_oracle_run(n, S, A, steps, dtype=np.dtype(dt))
    _same_results(algo, history, sd, ref, want, steps)


# ================================================================================================ the environment variables
CHILD = r"""
import sys

import numpy as np

root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from dist_classicrl_amd import _lib, environments, schedules
from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

results = {}
for name, n, S, path, calls in (("persistent", 128, 4000, None, [20, 20, 20]), ("wide", 2100, 3000, "wide", [130])):
    algo = OptimalQLearningBase(S, 16, 0.99, seed=0)
    if path:
        algo.set_rollout_path(path)
    rt = GpuRolloutQLearning(algo, schedules.ExponentialSchedule(0.1, 1e-5, 0.995),
                             schedules.ExponentialSchedule(1.0, 0.01, 0.995))
    env = environments.HashTabularEnv(n, S, 16, seed=1)
    sd, history, variants = None, [], set()
    for k in calls:
        _avg, h, env, sd = rt.run_steps(k, env, sd)
        history += h
        variants.update(rt.last_stats["kernel_variants"])
    print(name, "chunk_limit", env.chunk_limit(True), flush=True)
    results[name + "_q"] = np.asarray(algo.q_table)
    results[name + "_history"] = np.array(history, dtype=np.float32)
    results[name + "_obs"] = sd["states"]
    results[name + "_acc"] = sd["rewards"]
    results[name + "_rng_step"] = np.int64(sd["rng_step"])
    results[name + "_paths"] = np.array(sorted({_lib.decode_variant(v)["path"] for v in variants}))
np.savez(out, **results)
"""


def test_switches_read_from_the_environment_at_qe_create(tmp_path):
    """A fresh process with all five variables set runs one persistent and one wide case; its results are the
    oracle's and its persistent chunk limit is the device log's (``QE_HOST_BLOCK=0`` arrived)."""
    out = tmp_path / "child.npz"
    env = dict(os.environ, QE_HOST_BLOCK="0", QE_EVENT_TIMING="0", QE_USE_GRAPH="0", QE_TOKEN_ROUNDS="7",
               QE_LISTED_MIN_AGENTS="1")
    child = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(out)], env=env, cwd=str(ROOT), timeout=120,
                           capture_output=True, text=True, check=False)
    assert child.returncode == 0, child.stdout + child.stderr  # (nothing else is started after a failed child)
    limits = {line.split()[0]: int(line.split()[2]) for line in child.stdout.splitlines() if " chunk_limit " in line}
    assert limits["persistent"] == EP_CAP // 128
    assert limits["wide"] == (EP_CAP // 64) // -(-2100 // 64)
    got = np.load(out)
    for name, n, S, steps, path in (("persistent", 128, 4000, 60, "persistent"), ("wide", 2100, 3000, 130, "wide")):
        assert list(got[name + "_paths"]) == [path]
        ref, want = _c_oracle_run(n, S, 16, steps)
        assert np.array_equal(got[name + "_q"], ref.q)
        assert np.array_equal(got[name + "_history"], want["history"])
        assert np.array_equal(got[name + "_obs"], ref.obs)
        assert np.array_equal(got[name + "_acc"], ref.acc)
        assert int(got[name + "_rng_step"]) == steps
