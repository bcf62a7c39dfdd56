"""GPU: the main engine's episode log where it is FULL, against the C oracle.

The log has three implementations, each with a capacity edge and a hand-written overflow guard:

* the persistent kernels (``k_rollout_lane``, ``k_rollout_df``) stage episode ends in LDS (``EP_STAGE`` = 1024 entries,
  flushed every 32 steps); what does not fit the stage goes straight to memory under another guard;
* their linear log is the host result block (``HOST_LOG_CAP`` = 2^18 entries in page-locked memory) or, with an action
  trace or ``QE_OPT_HOST_BLOCK 0``, the device log (``ep_cap`` = 2^22 entries);
* the step-wise, turnstile, wide and evaluation kernels write 64 segments of ``ep_cap / 64`` = 65 536 entries, chosen by
  ``(agent + step) & 63``, which ``k_log_gather`` packs.

``HashTabularEnv(..., p_term_256=256)`` ends an episode of every agent in every step (``csrc/qe_envs.h``; the C oracle
is pinned to the NumPy oracle at that rate in ``tests/test_oracle_c.py``), so a few dozen steps overflow the stage and
``qe_rollout_chunk_limit`` steps fill a log to its last entry.  Every case compares the whole table, the final
observations, the running returns, the environment's episode counters, ``stats.episodes`` / ``episodes_dropped`` and
the log as (step, agent, return) triples in order with ``oracle/c_oracle.py`` -- exactly; no engine configuration is
compared with another one.  The large cases are as large as the engine's constants make them, not larger.
"""

import ctypes as C

import numpy as np
import pytest

from helpers import run_oracle_eval

pytestmark = pytest.mark.gpu

EPS, LR = 0.3, 0.1  # constant schedules of every case
S_SMALL = 300       # fewer rows than most cases have agents: rows are shared in every step
HOST_LOG_CAP, EP_CAP, SEGMENTS = 2**18, 2**22, 64


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return _lib, OptimalQLearningBase, GpuRolloutQLearning, environments, schedules


# ------------------------------------------------------------------------------------------------ the oracle, once per shape
@pytest.fixture(scope="module")
def oracle():
    """``get(n, S, A, steps, dt, mode, masked)`` -> the C oracle's run of `steps` steps at p_term_256 = 256 and its
    continuation by 3 more (``["more"]``), computed once per shape, shared between the tests and read-only."""
    from oracle import c_oracle

    cache = {}

    def snapshot(ref, out):
        got = {"q": ref.q.copy(), "obs": ref.obs.copy(), "acc": ref.acc.copy(), "episode": ref.episode.copy(),
               "actions": out["actions"], "ep_step": out["ep_step"], "ep_agent": out["ep_agent"], "ep_ret": out["history"],
               "episodes": out["episodes"]}
        for v in got.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return got

    def get(n, S, A, steps, dt="f4", mode="iter", masked=False):
        key = (n, S, A, steps, dt, mode, masked)
        if key not in cache:
            ref = c_oracle.CHashRollout(n, S, A, masked=masked, p_term_256=256, dtype=np.dtype(dt), mode=mode)
            out = ref.run(np.full(steps, EPS), np.full(steps, LR), trace=steps * n <= 1 << 20)
            # (the C oracle at this rate is pinned in tests/test_oracle_c.py; its log is every (t, i), t-major)
            assert out["episodes"] == steps * n
            first = snapshot(ref, out)
            first["more"] = snapshot(ref, ref.run(np.full(3, EPS), np.full(3, LR), trace=True))
            cache[key] = first
        return cache[key]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------ the engine through the C ABI
def _engine(n, S, A, *, dt="f4", masked=False, options=(), path=None):
    _lib, Algo, _, envs, _ = _product()
    algo = Algo(S, A, 0.99, seed=0, dtype=np.dtype(dt))
    for option, value in options:
        algo.set_engine_option(option, value)
    if path is not None:
        algo.set_rollout_path(path)
    env = envs.HashTabularEnv(n, S, A, seed=1, p_term_256=256, masked=masked)
    env.bind(algo)
    env.reset_device()
    return algo, env


def _rollout(algo, env, steps, mode="iter", trace=False):
    """One ``qe_rollout`` of `steps` steps (no cap of the Python runtime in between); returns (stats, trace)."""
    _lib = _product()[0]
    lib = _lib.load()
    eps, lr = np.full(steps, EPS), np.full(steps, LR)
    actions = np.empty((steps, env.num_agents), dtype=np.int32) if trace else None
    st = _lib.RolloutStats()
    _lib.check(lib.qe_rollout(algo.handle, env.handle, steps, _lib.ptr(eps, C.c_double), _lib.ptr(lr, C.c_double),
                              _lib.LEARN_ITER if mode == "iter" else _lib.LEARN_VEC, _lib.ptr(actions, C.c_int32), C.byref(st)))
    return st, actions


def _episode_log(algo, room):
    """The latest call's log through ``qe_episode_log`` with all three outputs: (count, step, agent, return)."""
    _lib = _product()[0]
    step, agent = np.full(room, -1, dtype=np.int32), np.full(room, -1, dtype=np.int32)
    ret = np.full(room, np.nan, dtype=np.float32)
    count = int(_lib.load().qe_episode_log(algo.handle, room, _lib.ptr(step, C.c_int32), _lib.ptr(agent, C.c_int32),
                                           _lib.ptr(ret, C.c_float)))
    return count, step, agent, ret


def _variant(st_or_int):
    _lib = _product()[0]
    return _lib.decode_variant(getattr(st_or_int, "kernel_variant", st_or_int))


def _same_state(algo, env, want):
    """Table, final observations, running returns and the environment's episode counters."""
    assert np.array_equal(np.asarray(algo.q_table), want["q"])
    states, acc = env.observe()
    assert np.array_equal(states["observation"] if isinstance(states, dict) else states, want["obs"])
    assert np.array_equal(acc, want["acc"])
    assert np.array_equal(env.aux(), want["episode"])


def _same_full_log(algo, st, want):
    """Nothing dropped, and the log equals the oracle's triple by triple, in order."""
    total = int(want["episodes"])
    assert st.episodes == total and st.episodes_dropped == 0, (st.episodes, st.episodes_dropped, total)
    count, step, agent, ret = _episode_log(algo, total + 8)  # (room behind the end: nothing may be written there)
    assert count == total
    assert np.array_equal(step[:total], want["ep_step"])
    assert np.array_equal(agent[:total], want["ep_agent"])
    assert np.array_equal(ret[:total], want["ep_ret"])
    assert (step[total:] == -1).all() and (agent[total:] == -1).all() and np.isnan(ret[total:]).all()


def _assert_persistent_build(st, build, *, n, masked=False):
    """`build`: "df" the dataflow kernel, "full" / "sparse" the LEAN builds of k_rollout_lane, "generic" the 512-agent
    build without LEAN (traced, float64, learn_vec, masked, rows of one 16-byte load, or more than 128 agents)."""
    d = _variant(st)
    assert d["path"] == "persistent" and d["masked"] == masked, d
    if build == "generic":
        assert d["lean"] == 0 and d["cap512"] and not d["dataflow"] and not d["help"], d
        return
    assert d["lean"] == 1 and not d["cap512"] and d["full"] == (n % 64 == 0), d
    assert d["dataflow"] == (build == "df") and d["light"] == (build != "full"), d


# ================================================================================================ a. the LDS stage overflows
# (id, agents, A, dtype, mode, masked, QE_OPT_LANE_ORDERED_PATH, action trace, the build that must run)
STAGE_CASES = [
    ("n33", 33, 16, "f4", "iter", False, 0, False, "df"),              # a partly filled wavefront; 33 x 32 = 1056 > 1024
    ("n64", 64, 16, "f4", "iter", False, 0, False, "df"),
    ("n128-df", 128, 16, "f4", "iter", False, 1, False, "df"),         # k_rollout_df has its own copy of the log code
    ("n128-full", 128, 16, "f4", "iter", False, 2, False, "full"),
    ("n128-sparse", 128, 16, "f4", "iter", False, 3, False, "sparse"),
    ("n512", 512, 16, "f4", "iter", False, 0, False, "generic"),       # 16 384 ends per window, 15 360 past the stage
    ("n128-traced", 128, 16, "f4", "iter", False, 0, True, "generic"),  # the device log, not the host result block
    ("n33-a4", 33, 4, "f4", "iter", False, 0, False, "generic"),
    ("n128-a4", 128, 4, "f4", "iter", False, 0, False, "generic"),
    ("n128-a8-df", 128, 8, "f4", "iter", False, 1, False, "df"),       # the other row width that has LEAN builds
    ("n128-f8", 128, 16, "f8", "iter", False, 0, False, "generic"),
    ("n64-masked", 64, 12, "f4", "iter", True, 0, False, "generic"),
    ("n128-vec", 128, 16, "f4", "vec", False, 0, False, "generic"),
    ("n512-a4-vec", 512, 4, "f4", "vec", False, 0, False, "generic"),
    ("n33-f8-vec", 33, 16, "f8", "vec", False, 0, False, "generic"),
]


@pytest.mark.parametrize("steps", [1, 32, 64, 70])  # one entry per agent / windows that end on a flush / a partial last window
@pytest.mark.parametrize("case", STAGE_CASES, ids=[c[0] for c in STAGE_CASES])
def test_more_episode_ends_in_a_flush_window_than_the_stage_holds(oracle, case, steps):
    """33 agents and more x 32 steps of a window > EP_STAGE: the surplus takes the "straight to memory" store."""
    _lib = _product()[0]
    _, n, A, dt, mode, masked, ordered_path, trace, build = case
    algo, env = _engine(n, S_SMALL, A, dt=dt, masked=masked,
                        options=[(_lib.OPT_LANE_ORDERED_PATH, ordered_path)] if ordered_path else ())
    st, actions = _rollout(algo, env, steps, mode, trace)
    _assert_persistent_build(st, build, n=n, masked=masked)
    if not trace:
        assert st.device_clock_ms > 0  # published through the host result block
    want = oracle(n, S_SMALL, A, steps, dt, mode, masked)
    if trace:
        assert np.array_equal(actions, want["actions"])
    _same_state(algo, env, want)
    _same_full_log(algo, st, want)


# ================================================================================================ b. a full linear log
N_LINEAR = 512


def _runtime(algo):
    _, _, Runtime, _, sch = _product()
    return Runtime(algo, sch.ConstantSchedule(LR), sch.ConstantSchedule(EPS))


def _linear_engine():
    _, Algo, _, envs, _ = _product()
    algo = Algo(S_SMALL, 16, 0.99, seed=0)
    return algo, envs.HashTabularEnv(N_LINEAR, S_SMALL, 16, seed=1, p_term_256=256)


def test_host_result_block_filled_to_its_last_entry_by_one_fused_call(oracle):
    """512 agents x 512 steps = 2^18 returns: ``run_steps`` takes the one-call path (``qe_rollout_fused``), whose
    4096-entry fast buffer the log exceeds 64 times over."""
    algo, env = _linear_engine()
    rt = _runtime(algo)
    env.bind(algo)
    limit = env.chunk_limit(True)
    assert limit == HOST_LOG_CAP // N_LINEAR
    fused_calls, inner = [], rt._run_steps_fused
    rt._run_steps_fused = lambda steps, env: fused_calls.append(steps) or inner(steps, env)
    avg, history, env, sd = rt.run_steps(limit, env, None)
    stats = rt.last_stats
    assert fused_calls == [limit] and stats["launches"] == 1  # one engine call
    d = _variant(stats["kernel_variant"])
    assert d["path"] == "persistent" and d["cap512"] and d["lean"] == 0, d
    assert stats["device_clock_ms"] > 0  # the host result block
    want = oracle(N_LINEAR, S_SMALL, 16, limit)
    assert stats["episodes"] == HOST_LOG_CAP == want["episodes"] and stats["episodes_dropped"] == 0
    assert np.array_equal(np.array(history, dtype=np.float32), want["ep_ret"])
    assert avg == np.cumsum(want["ep_ret"], dtype=np.float32)[-1] / len(history)  # single_thread_runtime.py:67
    count, step, agent, ret = _episode_log(algo, HOST_LOG_CAP)
    assert count == HOST_LOG_CAP
    assert np.array_equal(step, want["ep_step"]) and np.array_equal(agent, want["ep_agent"])
    assert np.array_equal(ret, want["ep_ret"])
    assert np.array_equal(sd["states"], want["obs"]) and np.array_equal(sd["rewards"], want["acc"])
    assert np.array_equal(sd["aux"], want["episode"])
    assert sd["rng_step"] == limit
    _same_state(algo, env, want)


@pytest.mark.parametrize("launches", [2, 3])
def test_full_host_result_blocks_behind_a_chunk_boundary(oracle, launches):
    """``limit + 1`` steps: a full slot 0 and a one-step slot 1; ``2 * limit + 1``: both slots full, then slot 0 again.
    The second case hands its state dict back for 3 more steps."""
    algo, env = _linear_engine()
    rt = _runtime(algo)
    env.bind(algo)
    limit = env.chunk_limit(True)
    assert limit == HOST_LOG_CAP // N_LINEAR
    steps = (launches - 1) * limit + 1
    _avg, history, env, sd = rt.run_steps(steps, env, None)
    assert rt.last_stats["launches"] == launches
    for v in rt.last_stats["kernel_variants"]:
        assert _variant(v)["path"] == "persistent" and _variant(v)["cap512"]
    assert rt.last_stats["device_clock_ms"] > 0
    want = oracle(N_LINEAR, S_SMALL, 16, steps)
    assert rt.last_stats["episodes"] == steps * N_LINEAR and rt.last_stats["episodes_dropped"] == 0
    assert np.array_equal(np.array(history, dtype=np.float32), want["ep_ret"])
    assert np.array_equal(sd["states"], want["obs"]) and np.array_equal(sd["rewards"], want["acc"])
    assert sd["rng_step"] == steps
    # the log of the last launch: one step, steps counted within that launch
    count, step, agent, ret = _episode_log(algo, N_LINEAR)
    assert count == N_LINEAR and not step.any() and np.array_equal(agent, np.arange(N_LINEAR))
    assert np.array_equal(ret, want["ep_ret"][-N_LINEAR:])
    if launches == 3:
        _avg, history, env, sd = rt.run_steps(3, env, sd)
        more = want["more"]
        assert np.array_equal(np.array(history, dtype=np.float32), more["ep_ret"])
        assert np.array_equal(sd["states"], more["obs"]) and np.array_equal(sd["rewards"], more["acc"])
        assert sd["rng_step"] == steps + 3
        want = more
    _same_state(algo, env, want)


def test_device_log_filled_to_its_last_slot_without_the_host_block(oracle):
    """``QE_OPT_HOST_BLOCK 0``: the chunk limit becomes the device log's, and one ``qe_rollout`` of exactly that many
    steps writes 2^22 entries -- control words, log and observations come back by stream synchronisation and copies."""
    _lib = _product()[0]
    algo, env = _engine(N_LINEAR, S_SMALL, 16, options=[(_lib.OPT_HOST_BLOCK, 0)])
    limit = env.chunk_limit(True)
    assert limit == EP_CAP // N_LINEAR
    st, _ = _rollout(algo, env, limit)
    d = _variant(st)
    assert d["path"] == "persistent" and d["cap512"], d
    want = oracle(N_LINEAR, S_SMALL, 16, limit)
    assert want["episodes"] == EP_CAP
    _same_state(algo, env, want)
    _same_full_log(algo, st, want)


# ================================================================================================ c. a full segmented log
# (id, set_rollout_path, options by name, the path that must run)
SEGMENTED_PATHS = [
    ("stepwise", "stepwise", (), "stepwise"),
    ("turnstile", "auto", (), "turnstile"),
    ("wide-bitmaps", "wide", (), "wide"),
    ("wide-lists", "wide", (("OPT_LISTED_MIN_AGENTS", 1), ("OPT_TOKEN_ROUNDS", 7)), "wide"),
]


def _segmented_engine(n, path, options, dt="f4"):
    _lib = _product()[0]
    return _engine(n, S_SMALL, 16, dt=dt, path=path, options=[(getattr(_lib, k), v) for k, v in options])


@pytest.mark.parametrize("n", [1024, 1000])  # every segment exactly full / uneven segments, other gather offsets
@pytest.mark.parametrize("case", SEGMENTED_PATHS, ids=[c[0] for c in SEGMENTED_PATHS])
def test_segmented_log_at_the_chunk_limit(oracle, case, n):
    """1024 agents x 4096 steps put exactly 65 536 entries into each of the 64 segments; 1000 agents fill them unevenly
    (15 or 16 entries per segment and step), so ``k_log_gather`` packs at offsets that differ from segment to segment."""
    _, path, options, want_path = case
    algo, env = _segmented_engine(n, path, options)
    limit = env.chunk_limit(True)
    assert limit == (EP_CAP // SEGMENTS) // -(-n // SEGMENTS) == 4096
    st, _ = _rollout(algo, env, limit)
    assert _variant(st)["path"] == want_path, _variant(st)
    want = oracle(n, S_SMALL, 16, limit)
    seg_count = np.bincount((want["ep_agent"] + want["ep_step"]) & 63, minlength=SEGMENTS)
    assert seg_count.max() <= EP_CAP // SEGMENTS and (n != 1024 or (seg_count == EP_CAP // SEGMENTS).all())
    _same_state(algo, env, want)
    _same_full_log(algo, st, want)


def test_evaluation_log_at_the_chunk_limit():
    """``qe_evaluate`` (``k_eval``) for ``chunk_limit(False)`` steps at 1024 agents: the log's structure -- every
    (t, i) exactly once, in order, nothing dropped -- at full length, the returns against the NumPy oracle's greedy
    evaluation (``helpers.run_oracle_eval``) on the first 30 steps.  (The NumPy oracle is too slow for the 4 million
    agent-steps of the whole call and the C oracle does not evaluate; the process is deterministic, so the prefix of
    the long run is the short run.  Nothing else is loosened.)"""
    _lib, Algo, _, envs, _ = _product()
    lib = _lib.load()
    n, S, A, prefix = 1024, S_SMALL, 16, 30
    q0 = np.random.default_rng(11).standard_normal((S, A)).astype(np.float32)
    algo = Algo(S, A, 0.99, seed=0)
    algo.q_table = q0
    env = envs.HashTabularEnv(n, S, A, seed=1, p_term_256=256)
    env.bind(algo)
    env.reset_device(seed=42)  # evaluate_steps, base_runtime.py:293-336
    steps = env.chunk_limit(False)
    assert steps == 4096
    st = _lib.RolloutStats()
    _lib.check(lib.qe_evaluate(algo.handle, env.handle, steps, C.byref(st)))
    assert _variant(st)["path"] == "eval"
    total = steps * n
    assert st.episodes == total == EP_CAP and st.episodes_dropped == 0
    count, step, agent, ret = _episode_log(algo, total)
    assert count == total
    assert np.array_equal(step, np.repeat(np.arange(steps, dtype=np.int32), n))
    assert np.array_equal(agent, np.tile(np.arange(n, dtype=np.int32), steps))
    assert np.isfinite(ret).all()
    want = run_oracle_eval(("hash", n, S, A, False, 256), "f4", q0, 0, "steps", prefix * n)
    assert want["calls"] == prefix and want["history"].size == prefix * n
    assert np.array_equal(ret[:prefix * n], want["history"])
    assert algo.step_counter == steps
    assert np.array_equal(np.asarray(algo.q_table), q0)  # evaluation does not learn
    assert np.array_equal(env.aux(), np.full(n, steps, dtype=np.uint32))  # one episode per agent and step


# ================================================================================================ d. one step past the limit
def _same_kept_log(algo, st, want, n, steps, dropped):
    """An overflowing log: the count of what was dropped, no kept entry twice, each kept entry the oracle's."""
    total = steps * n
    assert st.episodes == total == want["episodes"]
    assert st.episodes_dropped == dropped
    kept = total - dropped
    count, step, agent, ret = _episode_log(algo, total)
    assert count == kept
    step, agent, ret = step[:kept].astype(np.int64), agent[:kept].astype(np.int64), ret[:kept]
    assert (step >= 0).all() and (step < steps).all() and (agent >= 0).all() and (agent < n).all()
    at = step * n + agent  # the oracle's log holds (t, i) at t * n + i
    assert np.unique(at).size == kept
    assert (np.diff(at) > 0).all()  # sorted by (step, agent)
    assert np.array_equal(ret, want["ep_ret"][at])


OVERFLOW_CASES = [
    ("host-block-512", 512, None, (), "persistent"),
    ("stepwise-1024", 1024, "stepwise", (), "stepwise"),
    ("stepwise-1000", 1000, "stepwise", (), "stepwise"),
    ("turnstile-1024", 1024, "auto", (), "turnstile"),
    ("wide-lists-1000", 1000, "wide", (("OPT_LISTED_MIN_AGENTS", 1), ("OPT_TOKEN_ROUNDS", 7)), "wide"),
]


@pytest.mark.parametrize("case", OVERFLOW_CASES, ids=[c[0] for c in OVERFLOW_CASES])
def test_one_step_past_the_chunk_limit_is_counted_not_written(oracle, case):
    """The header leaves the chopping to the caller and says an overflow is counted, not written (``pos < out_cap``,
    ``ep_base + ep_slot < ep_cap``, ``p < seg_cap``): ``limit + 1`` steps in one ``qe_rollout``.  Learning must not
    notice, and nothing may be left over for the next call."""
    _, n, path, options, want_path = case
    algo, env = _segmented_engine(n, path, options)
    limit = env.chunk_limit(True)
    steps = limit + 1
    st, _ = _rollout(algo, env, steps)
    assert _variant(st)["path"] == want_path, _variant(st)
    want = oracle(n, S_SMALL, 16, steps)
    if want_path == "persistent":
        assert limit == HOST_LOG_CAP // n and st.device_clock_ms > 0
        dropped = n  # the linear log: the whole last step
    else:
        assert limit == 4096
        seg_count = np.bincount((want["ep_agent"] + want["ep_step"]) & 63, minlength=SEGMENTS)
        dropped = int(np.maximum(0, seg_count - EP_CAP // SEGMENTS).sum())
        assert dropped == (n if n == 1024 else 0)  # (1000 agents: 64 016 entries per segment at most, still room)
    _same_kept_log(algo, st, want, n, steps, dropped)
    _same_state(algo, env, want)
    st, _ = _rollout(algo, env, 3)
    assert _variant(st)["path"] == want_path
    more = want["more"]
    _same_state(algo, env, more)
    _same_full_log(algo, st, more)
