"""GPU: the device-resident ExperienceReplay.

* the ring's host API against the real reference's fixture;
* the ring as the fused rollouts fill it -- every entry point (``qe_rollout``, ``qe_rollout_fused`` with and without the
  host result block, the pipelined ``qe_rollout_begin`` / ``qe_rollout_end`` pair), every environment, every kernel
  path (persistent, step-wise, wide, turnstile; eager launches and graph replay), chained / detached / moved rings,
  rings smaller than one vector step and calls the engine refuses -- against ``helpers.run_oracle_transitions`` and
  ``helpers.ring_after``: the ring over its written slots with ``(position, full, len)``, and the table, the episode
  returns and the final observations of the same run.  Nothing the device returned feeds an expectation;
* ``learn_from`` / ``qe_replay_gather`` against sampling + ``learn`` done by the oracle.

Everything is bit for bit."""

import ctypes as C
import functools
import gc
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import make_oracle_env, ring_after, run_oracle_transitions, schedule_params, transitions_of
from test_oracle_replay import replay_script

pytestmark = pytest.mark.gpu

FIELDS = ("state", "action", "reward", "next_state", "done")


def _classes():
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.buffers import ExperienceReplay

    return ExperienceReplay, OptimalQLearningBase


def test_replay_matches_reference_fixture():
    replay_script(_classes()[0])


def test_push_batch_wraps_like_repeated_push():
    from oracle.replay_oracle import OracleReplay

    Replay = _classes()[0]
    rng = np.random.default_rng(0)
    for capacity, n in [(10, 3), (10, 10), (10, 27), (64, 500), (7, 7)]:
        rb, ref = Replay(capacity, 1), OracleReplay(capacity, 1)
        for _ in range(3):
            s, a = rng.integers(1 << 40, size=n), rng.integers(100, size=n)
            r, nx, d = rng.standard_normal(n), rng.integers(1 << 40, size=n), rng.random(n) < 0.3
            rb.push_batch(s, a, r, nx, d)
            for e in zip(s, a, r, nx, d):
                ref.push(e)
            assert (rb.position, rb.full, len(rb)) == (ref.position, ref.full, len(ref))
            k = len(ref)  # slots 0..k-1 hold data (the rest of the ring was never written)
            assert np.array_equal(rb.state_buffer[:k], ref.state_buffer[:k])
            assert np.array_equal(rb.action_buffer[:k], ref.action_buffer[:k])
            assert np.array_equal(rb.reward_buffer[:k], ref.reward_buffer[:k])
            assert np.array_equal(rb.next_state_buffer[:k], ref.next_state_buffer[:k])
            assert np.array_equal(rb.done_buffer[:k], ref.done_buffer[:k])
        got, want = rb.sample_arrays(min(5, len(ref))), ref.sample_arrays(min(5, len(ref)))
        assert all(np.array_equal(x, y) for x, y in zip(got, want))


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_learn_from_replay_on_device_equals_sample_then_learn(mode, dt):
    from oracle.qlearn_oracle import OracleQLearning
    from oracle.replay_oracle import OracleReplay

    Replay, Algo = _classes()
    S, A, capacity, batch = 40, 6, 300, 128
    rng = np.random.default_rng(3)
    rb, ref_rb = Replay(capacity, 9), OracleReplay(capacity, 9)
    n = 450  # wraps
    s, a = rng.integers(S, size=n), rng.integers(A, size=n)
    r, nx, d = rng.random(n).astype(np.float32).astype(np.float64), rng.integers(S, size=n), rng.random(n) < 0.2
    rb.push_batch(s, a, r, nx, d)
    for e in zip(s, a, r, nx, d):
        ref_rb.push(e)
    q0 = rng.standard_normal((S, A)).astype(dt)
    algo, ref = Algo(S, A, 0.9, seed=0, dtype=np.dtype(dt)), OracleQLearning(S, A, 0.9, dtype=np.dtype(dt))
    algo.q_table = q0
    ref.q_table = q0.copy()
    for _ in range(4):
        idx = rb.learn_from(algo, batch, 0.1, mode=mode)
        bs, ba, br, bn, bd = ref_rb.sample_arrays(batch)
        fn = ref.learn if mode == "iter" else ref.learn_vec
        fn(bs.astype(np.int32), ba.astype(np.int32), br.astype(np.float32), bn.astype(np.int32), bd, 0.1)
        assert np.array_equal(np.asarray(algo.q_table), ref.q_table)


def test_replay_errors():
    Replay, Algo = _classes()
    rb = Replay(8, 0)
    rb.push((1, 2, 0.5, 3, False))
    with pytest.raises(ValueError):
        rb.sample(2)  # numpy: cannot take a larger sample than population when replace=False
    with pytest.raises(ValueError):
        rb.push_batch([1, 2], [0], [0.0], [1], [False])
    rb.push((99, 0, 0.0, 1, False))  # a state the table below does not have
    with pytest.raises(IndexError):
        rb.learn_from(Algo(10, 3, 0.9, seed=0), 2, 0.1)


@pytest.mark.parametrize(("n", "S", "A", "steps", "capacity", "path"), [
    (96, 500, 8, 25, 96 * 25 + 17, "auto"),      # persistent kernel, everything fits the ring
    (96, 500, 8, 40, 1000, "auto"),              # ... and wrapping around it
    (600, 3000, 16, 12, 600 * 12, "stepwise"),   # step-wise kernels
    (600, 3000, 16, 12, 600 * 12, "auto"),       # one launch per step (turnstile path)
    (2100, 3000, 16, 9, 5000, "wide"),           # token rounds
])
def test_fused_rollout_pushes_every_transition_into_the_ring(n, S, A, steps, capacity, path):
    """experience_replay.py:68-86 wired to the fused loop: the ring holds (s, a, r, s', done) of every agent and
    vector step in (step, agent) order -- what a host loop pushing after every env.step would store."""
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning
    from dist_classicrl_amd.environments import HashTabularEnv
    from dist_classicrl_amd.schedules import ConstantSchedule
    from oracle.envs import HashTabularEnv as OracleEnv

    Replay, Algo = _classes()
    algo = Algo(S, A, 0.99, seed=0)
    algo.set_rollout_path(path)
    rb = Replay(capacity, 1)
    rb.attach(algo)
    rt = GpuRolloutQLearning(algo, ConstantSchedule(0.1), ConstantSchedule(0.3))
    rt.trace_actions = True
    try:
        rt.run_steps(steps, HashTabularEnv(n, S, A, seed=1), None)
    except ZeroDivisionError:
        pass
    actions = rt.last_trace
    # the same environment driven by those actions on the CPU
    env = OracleEnv(n, S, A, seed=1)
    obs, _ = env.reset()
    want = []
    for t in range(steps):
        nxt, r, term, _, _ = env.step(actions[t])
        want.append((obs.copy(), actions[t].copy(), r.copy(), nxt.copy(), term.copy()))
        obs = nxt
    ws, wa, wr, wn, wd = (np.concatenate([w[k] for w in want]) for k in range(5))
    total = steps * n
    assert (rb.position, rb.full, len(rb)) == (total % capacity, total >= capacity, min(total, capacity))
    slots = np.arange(total) % capacity
    live = np.arange(total) >= total - capacity  # later pushes overwrite earlier ones
    gs, ga, gr, gn, gd = rb.state_buffer, rb.action_buffer, rb.reward_buffer, rb.next_state_buffer, rb.done_buffer
    assert np.array_equal(gs[slots[live]], ws[live]) and np.array_equal(ga[slots[live]], wa[live])
    assert np.array_equal(gr[slots[live]], wr[live].astype(np.float64)) and np.array_equal(gn[slots[live]], wn[live])
    assert np.array_equal(gd[slots[live]], wd[live].astype(bool))
    before = np.asarray(algo.q_table).copy()
    rb.learn_from(algo, 64, 0.1)  # the optional replay phase: sample -> learn without leaving the device
    assert not np.array_equal(before, np.asarray(algo.q_table))
    rb.detach(algo)
    pos = rb.position
    try:
        rt.run_steps(3, HashTabularEnv(n, S, A, seed=1), None)
    except ZeroDivisionError:
        pass
    assert rb.position == pos  # detached: nothing is pushed any more


# =====================================================================================================================
# The ring as the fused rollouts fill it, against the oracle's closed loop
# =====================================================================================================================
def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    Replay, Algo = _classes()
    return _lib, Algo, GpuRolloutQLearning, environments, schedules, Replay


@functools.lru_cache(maxsize=None)
def _table_mdp(S, A, K, seed):
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp
    from table_mdp_model import random_mdp

    arrays, isd, masks = random_mdp(S, A, K, seed=seed, masked=True)
    return encode_table_mdp(*arrays, isd, masks)


def _device_env(envs, spec):
    """Specs as ``helpers.make_oracle_env`` takes them, plus ("table", agents, S, A, K, seed): a small masked random MDP."""
    kind = spec[0]
    if kind == "hash":
        return envs.HashTabularEnv(spec[1], spec[2], spec[3], seed=1, masked=spec[4])
    if kind == "grid":
        return envs.GridLakeEnv(spec[1], side=spec[2], seed=1)
    if kind == "ttt":
        return envs.TicTacToeEnv(spec[1], seed=1)
    if kind == "bandit":
        return envs.RiggedTwoArmedBanditVecEnv(spec[1], episode_len=spec[2])
    return envs.TabularMDPEnv(spec[1], _table_mdp(*spec[2:]), seed=1)


def _oracle_env(spec):
    if spec[0] == "table":
        from table_mdp_model import TableMDPVecEnv

        return TableMDPVecEnv(spec[1], _table_mdp(*spec[2:]), seed=1)
    return make_oracle_env(spec)


@functools.lru_cache(maxsize=None)
def _want(spec, calls, dt, sched, mode):
    """The oracle's run of one case: computed once, shared by every test that needs it and never modified."""
    return run_oracle_transitions(_oracle_env(spec), list(calls), dt, sched, mode)


def _schedules(sch, kind):
    def make(p):
        kind_, value, lo, decay = p
        return sch.ExponentialSchedule(value, lo, decay) if kind_ == "exponential" else sch.ConstantSchedule(value)

    lr_p, eps_p = schedule_params(kind)
    return make(lr_p), make(eps_p)


def _setup(spec, dt, mode, capacity, *, path="auto", options=(), sched="const", ring_seed=1):
    """Engine + runtime + environment of `spec`, with a ring of `capacity` attached (None: no ring)."""
    _lib, Algo, Runtime, envs, sch, Replay = _product()
    env = _device_env(envs, spec)
    algo = Algo(env.state_size, env.action_size, 0.99, seed=0, dtype=np.dtype(dt))
    algo.set_rollout_path(path)
    for opt, value in options:
        algo.set_engine_option(getattr(_lib, opt), value)
    rt = Runtime(algo, *_schedules(sch, sched), learn_mode=mode)
    rb = None
    if capacity is not None:
        rb = Replay(capacity, ring_seed)
        rb.attach(algo)
    return SimpleNamespace(algo=algo, rt=rt, env=env, rb=rb, history=[], sd=None, spec=spec, entries=[])


def _spy_entry_points(run):
    """Records in run.entries which of the runtime's two ways into the engine a ``run_steps`` call took."""
    fused, rollout = run.rt._run_steps_fused, run.rt._rollout

    def spy_fused(*a, **kw):
        run.entries.append("fused")
        return fused(*a, **kw)

    def spy_rollout(*a, **kw):
        run.entries.append("rollout")
        return rollout(*a, **kw)

    run.rt._run_steps_fused, run.rt._rollout = spy_fused, spy_rollout


def _path_is(path, **bits):
    def check(d):
        assert d["path"] == path, d
        for name, value in bits.items():
            assert d[name] == value, (name, d)
    return check


GENERIC = _path_is("persistent", lean=0, cap512=True)  # the persistent build of every rollout with a ring attached


def _call(run, steps, check, env=None):
    """One ``run_steps`` call; `check(decoded variant)` for every kernel build it ran."""
    _lib = _product()[0]
    if env is not None:
        run.env = env
    try:
        _avg, h, _env, run.sd = run.rt.run_steps(steps, run.env, run.sd)
    except ZeroDivisionError:  # no episode ended in this call (reference quirk); the state moved on all the same
        h, run.sd = [], run.env.state_dict()
    run.history += list(h)
    assert run.rt.last_stats["kernel_variants"], "no launch was recorded"
    for v in run.rt.last_stats["kernel_variants"]:
        check(_lib.decode_variant(v))


def _check_state(run, chunk):
    assert np.array_equal(np.asarray(run.algo.q_table), chunk["q"], equal_nan=True), "table"
    assert np.array_equal(np.array(run.history, dtype=np.float32), chunk["history"]), "episode returns"
    obs = run.sd["states"]["observation"] if isinstance(run.sd["states"], dict) else run.sd["states"]
    assert np.array_equal(obs, chunk["final_obs"]), "final observations"
    assert np.array_equal(run.sd["rewards"], chunk["agent_rewards"]), "running returns"


def _buffers(rb):
    return dict(zip(FIELDS, rb._all()))


def _check_ring(rb, want):
    """`want`: ``ring_after``'s result.  Every written slot holds all five fields of the push ``ring_after`` names."""
    assert (rb.position, rb.full, len(rb)) == (want["position"], want["full"], want["len"])
    got, w = _buffers(rb), want["written"]
    wrong = {}
    for name in FIELDS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        a, b = got[name][w], want[name][w]
        bad = a.view(np.uint64) != b.view(np.uint64) if name == "reward" else a != b  # (rewards: bit for bit)
        if bad.any():
            wrong[name] = np.flatnonzero(w)[bad]
    assert not wrong, {k: (len(v), v[:8].tolist()) for k, v in wrong.items()}


def _concat(*parts):
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(5))


def _inputs_are_hard(want, same_state=True):
    """Conditions on a case's inputs, from the oracle's records alone: a terminated transition, a transition with
    s' == s (where the environment's rules allow one) and a step in which two agents stand on one row."""
    s, _a, _r, s2, d = transitions_of(want)
    assert d.any(), "no terminated transition"
    assert not same_state or (s2 == s).any(), "no transition with s' == s"
    by_step = np.sort(s.reshape(-1, want["n"]), axis=1)
    assert (by_step[:, 1:] == by_step[:, :-1]).any(), "no step in which two agents share a row"


def _ring_case(spec, dt, mode, calls, capacity, check, *, path="auto", options=(), sched="const", prepare=None,
               same_state=True):
    """`calls` consecutive ``run_steps`` calls with a ring attached; after EVERY call the ring and the run's state
    against the oracle.  Returns the run and the oracle's records."""
    want = _want(spec, tuple(calls), dt, sched, mode)
    _inputs_are_hard(want, same_state)
    run = _setup(spec, dt, mode, capacity, path=path, options=options, sched=sched)
    if prepare:
        prepare(run)
    for k, chunk in zip(calls, want["chunks"]):
        _call(run, k, check)
        _check_ring(run.rb, ring_after(transitions_of(want, 0, chunk["steps"]), capacity))
        _check_state(run, chunk)
    return run, want


# ---------------------------------------------------------------------------------------------- a. entry points
ENTRY_SPEC = ("hash", 96, 500, 8, False)


@pytest.mark.parametrize("capacity", [96 * 40 + 17, 1000])
@pytest.mark.parametrize("host_block", [1, 0])
def test_one_call_entry_point_fills_the_ring(host_block, capacity):
    """What a user gets by default: unmasked, untraced, one chunk -> ``qe_rollout_fused``; with the host result block
    (the kernel's own clock is reported) and without it."""
    def prepare(run):
        _spy_entry_points(run)

    run, _ = _ring_case(ENTRY_SPEC, "f4", "iter", [40], capacity, GENERIC, prepare=prepare,
                        options=(("OPT_HOST_BLOCK", host_block),))
    assert run.entries == ["fused"]
    assert run.rt.last_stats["launches"] == 1
    assert (run.rt.last_stats["device_clock_ms"] > 0) == bool(host_block)


@pytest.mark.parametrize("capacity", [96 * 40 + 17, 1000, 50])
def test_pipelined_entry_points_fill_the_ring(capacity):
    """``qe_rollout_begin`` / ``qe_rollout_end`` with six chunks (7, 7, 7, 7, 7, 5 steps), both slots alternating.  (An
    unmasked, untraced call leaves the one-call form only for a history type other than "float" or a call beyond
    the chunk limit: the former here.)"""
    def prepare(run):
        _spy_entry_points(run)
        run.rt._PIPELINE_CHUNK = 7
        run.rt.history_type = "float32"

    run, _ = _ring_case(ENTRY_SPEC, "f4", "iter", [40], capacity, GENERIC, prepare=prepare)
    assert run.entries == ["rollout"]
    assert run.rt.last_stats["launches"] == 6


# ---------------------------------------------------------------------------------------------- b. environments and types
ENV_CASES = {
    "grid6": (("grid", 48, 6), 30, True),
    "bandit": (("bandit", 40, 5), 23, True),
    # (TicTacToe: a move always changes the board, and no game ends within its first moves: s' == s cannot happen)
    "ttt": (("ttt", 64), 40, False),
    "hash_masked_a12": (("hash", 64, 300, 12, True), 30, True),
    "hash_masked_a64": (("hash", 128, 500, 64, True), 30, True),
    "table_masked": (("table", 48, 60, 9, 3, 6), 30, True),
}


def _env_case(name, dt, mode):
    spec, steps, same_state = ENV_CASES[name]
    n = spec[1]
    masked = spec[0] in ("ttt", "table") or (spec[0] == "hash" and spec[4])
    check = _path_is("persistent", lean=0, cap512=True, masked=masked)
    return _ring_case(spec, dt, mode, [steps], n * steps * 2 // 3 + 5, check, same_state=same_state, sched="bench")


@pytest.mark.parametrize(("name", "dt", "mode"), [
    ("grid6", "f4", "iter"), ("grid6", "f8", "vec"),
    ("bandit", "f8", "iter"), ("bandit", "f4", "vec"),
    ("ttt", "f4", "iter"), ("ttt", "f8", "vec"),
    ("hash_masked_a12", "f8", "iter"), ("hash_masked_a12", "f4", "vec"),
    ("hash_masked_a64", "f4", "iter"), ("hash_masked_a64", "f8", "vec"),
    ("table_masked", "f4", "iter"), ("table_masked", "f8", "vec"),
])
def test_every_environment_fills_the_ring(name, dt, mode):
    """Each environment's own ``Env::step`` feeding ``replay_put`` (masked ones through the pipelined entry points), a
    ring that wraps."""
    _env_case(name, dt, mode)


# ---------------------------------------------------------------------------------------------- c. paths and graph replay
PATH_SPEC = ("hash", 64, 300, 16, False)


@pytest.mark.parametrize(("mode", "graph"), [("iter", 1), ("vec", 1), ("iter", 0)])
@pytest.mark.parametrize("path", ["stepwise", "wide", "turnstile"])
def test_one_launch_per_step_paths_fill_the_ring(path, mode, graph):
    """140 steps: 32 eager steps, two replays of the 50-step graph, 7 eager steps and the closing learn; and the same
    steps all eager (QE_OPT_USE_GRAPH 0, once per path)."""
    _ring_case(PATH_SPEC, "f4", mode, [140], 64 * 140 - 1000, _path_is(path), path=path,
               options=(("OPT_USE_GRAPH", graph),))


# ---------------------------------------------------------------------------------------------- d. call patterns
CALLS = [13, 1, 26]


def test_chained_calls_equal_one_call():
    """Three calls on a ring that wraps in the middle of the second one (the third on a fresh environment object from
    the state dict, so the device state is restored) leave the ring, and the table, that one call of 40 steps leaves."""
    n = ENTRY_SPEC[1]
    capacity = 13 * n + 50
    want = _want(ENTRY_SPEC, tuple(CALLS), "f4", "const", "iter")
    envs = _product()[3]
    run = _setup(ENTRY_SPEC, "f4", "iter", capacity)
    for j, (k, chunk) in enumerate(zip(CALLS, want["chunks"])):
        if j == 2:
            run.sd = {key: (np.array(v) if isinstance(v, np.ndarray) else v) for key, v in run.sd.items()}
        _call(run, k, GENERIC, env=_device_env(envs, ENTRY_SPEC) if j == 2 else None)
        _check_ring(run.rb, ring_after(transitions_of(want, 0, chunk["steps"]), capacity))
        _check_state(run, chunk)
    one, want_one = _ring_case(ENTRY_SPEC, "f4", "iter", [40], capacity, GENERIC)
    for name in ("s", "a", "r", "s2", "d"):
        assert np.array_equal(want_one[name], want[name])
    a, b = _buffers(run.rb), _buffers(one.rb)
    assert all(np.array_equal(a[name], b[name]) for name in FIELDS)  # (40 * 96 pushes: every slot was written)


def test_detached_for_the_middle_call():
    n = ENTRY_SPEC[1]
    capacity = 20 * n + 11
    want = _want(ENTRY_SPEC, tuple(CALLS), "f4", "const", "iter")
    run = _setup(ENTRY_SPEC, "f4", "iter", capacity)
    _call(run, 13, GENERIC)
    first = ring_after(transitions_of(want, 0, 13), capacity)
    _check_ring(run.rb, first)
    run.rb.detach(run.algo)
    _call(run, 1, _path_is("persistent", lean=1))  # no ring: a plain training rollout again
    _check_ring(run.rb, first)
    run.rb.attach(run.algo)
    _call(run, 26, GENERIC)
    _check_ring(run.rb, ring_after(_concat(transitions_of(want, 0, 13), transitions_of(want, 14, 40)), capacity))
    _check_state(run, want["chunks"][2])


def test_ring_moved_to_a_second_engine():
    n = ENTRY_SPEC[1]
    capacity = 30 * n
    want = _want(ENTRY_SPEC, tuple(CALLS), "f4", "const", "iter")
    run = _setup(ENTRY_SPEC, "f4", "iter", capacity)
    other = _setup(ENTRY_SPEC, "f4", "iter", None)
    _call(run, 13, GENERIC)
    run.rb.attach(other.algo)
    first = ring_after(transitions_of(want, 0, 13), capacity)
    _call(run, 1, _path_is("persistent", lean=1))  # the first engine pushes nothing any more
    _check_ring(run.rb, first)
    _check_state(run, want["chunks"][1])
    _call(other, 13, GENERIC)
    _check_ring(run.rb, ring_after(_concat(transitions_of(want, 0, 13), transitions_of(want, 0, 13)), capacity))
    _check_state(other, want["chunks"][0])


def test_ring_deleted_while_attached():
    want = _want(ENTRY_SPEC, tuple(CALLS), "f4", "const", "iter")
    run = _setup(ENTRY_SPEC, "f4", "iter", 777)
    _call(run, 13, GENERIC)
    run.rb = None
    gc.collect()
    _call(run, 1, _path_is("persistent", lean=1))
    _call(run, 26, _path_is("persistent", lean=1))
    _check_state(run, want["chunks"][2])


# ---------------------------------------------------------------------------------------------- e. small rings
SMALL = {
    "persistent": (("hash", 96, 500, 8, False), 9, "auto", GENERIC),
    "stepwise": (("hash", 600, 3000, 16, False), 5, "stepwise", _path_is("stepwise")),
    "wide": (("hash", 600, 3000, 16, False), 5, "wide", _path_is("wide")),
    "turnstile": (("hash", 600, 3000, 16, False), 5, "auto", _path_is("turnstile")),
}


@pytest.mark.parametrize("cap_of", ["1", "n-1", "n", "n+1", "2n-1"])
@pytest.mark.parametrize("path", list(SMALL))
def test_rings_around_one_vector_step(path, cap_of):
    """Rings of 1, N - 1, N, N + 1 and 2N - 1 slots under N agents: with fewer slots than agents, agents i and
    i + capacity of ONE step map to one slot, and that slot must hold all five fields of the later of them."""
    spec, steps, forced, check = SMALL[path]
    n = spec[1]
    capacity = {"1": 1, "n-1": n - 1, "n": n, "n+1": n + 1, "2n-1": 2 * n - 1}[cap_of]
    # (600 agents on 3000 states meet no s' == s within five steps; the other two input conditions hold)
    _ring_case(spec, "f4", "iter", [steps], capacity, check, path=forced, same_state=n < 600)


# ---------------------------------------------------------------------------------------------- f. refused calls
@pytest.mark.parametrize("entry", ["fused", "pipelined", "traced"])
def test_refused_rollout_leaves_the_ring_alone(entry):
    """A forced persistent path with 600 agents is refused (QE_ERR_UNSUPPORTED); the ring must not have moved, and the
    next call writes from the slot it stood at."""
    spec = ("hash", 600, 3000, 16, False)
    capacity = 5 + 3 * 600 + 7
    want = _want(spec, (3,), "f4", "const", "iter")
    run = _setup(spec, "f4", "iter", capacity, path="persistent")
    rng = np.random.default_rng(5)
    pre = (rng.integers(3000, size=5), rng.integers(16, size=5), rng.standard_normal(5), rng.integers(3000, size=5),
           rng.random(5) < 0.5)
    run.rb.push_batch(*pre)
    assert (run.rb.position, run.rb.full, len(run.rb)) == (5, False, 5)
    before = _buffers(run.rb)
    if entry == "pipelined":
        run.rt.history_type = "float32"
    if entry == "traced":
        run.rt.trace_actions = True
    with pytest.raises(NotImplementedError):
        run.rt.run_steps(3, run.env, None)
    assert (run.rb.position, run.rb.full, len(run.rb)) == (5, False, 5)
    after = _buffers(run.rb)
    assert all(np.array_equal(before[name].view(np.uint8), after[name].view(np.uint8)) for name in FIELDS)
    run.algo.set_rollout_path("auto")
    _call(run, 3, _path_is("turnstile"))
    _check_ring(run.rb, ring_after(_concat(pre, transitions_of(want)), capacity))
    _check_state(run, want["chunks"][0])


# =====================================================================================================================
# learn_from, sampling and gather
# =====================================================================================================================
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize(("S", "A"), [(40, 6), (300, 20)])
def test_learn_from_batches_around_one_block(S, A, dt, mode):
    """Batches of 1, 256, 257 and 700 from a full ring of 700 (k_replay_to_batch: one block, one full block, a second
    block of one thread, a ragged third); rewards are arbitrary float64 values, which the batch narrows to float32."""
    from oracle.qlearn_oracle import OracleQLearning
    from oracle.replay_oracle import OracleReplay

    Replay, Algo = _classes()
    capacity, n = 700, 950  # wraps
    rng = np.random.default_rng(S)
    s, a = rng.integers(S, size=n), rng.integers(A, size=n)
    r, nx, d = rng.standard_normal(n), rng.integers(S, size=n), rng.random(n) < 0.2
    assert (r[-capacity:].astype(np.float32).astype(np.float64) != r[-capacity:]).any()  # the narrowing rounds
    rb, ref_rb = Replay(capacity, 9), OracleReplay(capacity, 9)
    rb.push_batch(s, a, r, nx, d)
    for e in zip(s, a, r, nx, d):
        ref_rb.push(e)
    q0 = rng.standard_normal((S, A)).astype(dt)
    algo, ref = Algo(S, A, 0.9, seed=0, dtype=np.dtype(dt)), OracleQLearning(S, A, 0.9, dtype=np.dtype(dt))
    algo.q_table = q0
    ref.q_table = q0.copy()
    for batch in (1, 256, 257, 700):
        i = ref_rb.indices(batch)
        bs, ba, br, bn, bd = (getattr(ref_rb, name + "_buffer")[i] for name in FIELDS)
        if batch > 1:  # conditions on the sampled batch
            assert len(np.unique(bs * A + ba)) < batch, "no repeated (s, a) cell in the batch"
            assert bd.any() and not bd.all()
        idx = rb.learn_from(algo, batch, 0.1, mode=mode)
        assert np.array_equal(idx, i)
        fn = ref.learn if mode == "iter" else ref.learn_vec
        fn(bs.astype(np.int32), ba.astype(np.int32), br.astype(np.float32), bn.astype(np.int32), bd, 0.1)
        assert np.array_equal(np.asarray(algo.q_table), ref.q_table), batch


@pytest.mark.parametrize(("name", "dt", "mode"), [
    ("hash_masked_a12", "f8", "iter"), ("hash_masked_a64", "f8", "vec"), ("ttt", "f4", "iter"), ("ttt", "f8", "vec"),
])
def test_learn_from_a_ring_the_device_filled(name, dt, mode):
    """The optional replay phase after a masked rollout: the reference's unmasked ``learn`` / ``learn_vec`` on
    ``sample_arrays`` of the ring the oracle's transitions leave, same seed."""
    from oracle.qlearn_oracle import OracleQLearning
    from oracle.replay_oracle import OracleReplay

    run, want = _env_case(name, dt, mode)
    ring = ring_after(transitions_of(want), run.rb.capacity)
    assert ring["written"].all()
    ref_rb = OracleReplay(run.rb.capacity, 1)
    for field in FIELDS:
        setattr(ref_rb, field + "_buffer", ring[field])
    ref_rb.position, ref_rb.full = ring["position"], ring["full"]
    ref = OracleQLearning(run.env.state_size, run.env.action_size, 0.99, dtype=np.dtype(dt))
    ref.q_table = want["chunks"][-1]["q"].copy()
    for batch in (300, 77):
        bs, ba, br, bn, bd = ref_rb.sample_arrays(batch)
        fn = ref.learn if mode == "iter" else ref.learn_vec
        fn(bs.astype(np.int32), ba.astype(np.int32), br.astype(np.float32), bn.astype(np.int32), bd, 0.05)
        run.rb.learn_from(run.algo, batch, 0.05, mode=mode)
        assert np.array_equal(np.asarray(run.algo.q_table), ref.q_table)


def _raw_gather(rb, idx):
    """``qe_replay_gather`` into sentinel-filled outputs; returns (status, outputs)."""
    from dist_classicrl_amd import _lib

    idx = np.ascontiguousarray(idx, dtype=np.int64)
    k = idx.size
    s, a, n = (np.full(k, -77, dtype=np.int64) for _ in range(3))
    r, d = np.full(k, -77.0, dtype=np.float64), np.full(k, 77, dtype=np.uint8)
    rc = rb._lib.qe_replay_gather(rb._h, _lib.ptr(idx, C.c_int64), k, _lib.ptr(s, C.c_int64), _lib.ptr(a, C.c_int64),
                                  _lib.ptr(r, C.c_double), _lib.ptr(n, C.c_int64), _lib.ptr(d, C.c_uint8))
    return rc, (s, a, r, n, d)


def test_gather_takes_indices_like_numpy():
    from dist_classicrl_amd import _lib

    Replay = _classes()[0]
    capacity = 300  # (two blocks of k_replay_gather, the second ragged, for the 300-index gathers below)
    rng = np.random.default_rng(11)
    host = (rng.integers(1 << 40, size=capacity), rng.integers(100, size=capacity), rng.standard_normal(capacity),
            rng.integers(1 << 40, size=capacity), (rng.random(capacity) < 0.3).astype(np.uint8))
    rb = Replay(capacity, 0)
    rb.push_batch(*host)
    for idx in (np.array([-1, -capacity, 0, capacity - 1, -7, 7, -1]), rng.integers(-capacity, capacity, size=300),
                np.arange(-1, -capacity - 1, -1)):
        rc, got = _raw_gather(rb, idx)
        assert rc == 0
        for g, h in zip(got, host):
            assert np.array_equal(g, h[idx])
    before = _buffers(rb)
    for bad in (capacity, -capacity - 1):
        rc, got = _raw_gather(rb, np.array([3, bad, 5]))
        assert rc == _lib.ERR_INDEX
        with pytest.raises(IndexError):
            _lib.check(rc)
        assert all((g == -77).all() for g in got[:4]) and (got[4] == 77).all()  # outputs untouched
        assert (rb.position, rb.full, len(rb)) == (0, True, capacity)
        after = _buffers(rb)
        assert all(np.array_equal(before[name], after[name]) for name in FIELDS)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_terminated_entry_with_a_next_state_outside_the_table(dt):
    """``learn`` never reads the next state of a terminated transition, ``learn_vec`` reads every one (its row
    maximum is multiplied by zero afterwards): ``learn_from`` learns from such an entry in "iter" mode and raises in
    "vec" mode -- refused by the batch kernel's count before anything touches the table."""
    from oracle.qlearn_oracle import OracleQLearning

    Replay, Algo = _classes()
    S, A, n = 40, 6, 64
    rng = np.random.default_rng(2)
    s, a, r = rng.integers(S, size=n), rng.integers(A, size=n), rng.standard_normal(n)
    nx, d = rng.integers(S, size=n), rng.random(n) < 0.3
    d[[3, 40, 63]] = True
    nx[[3, 40, 63]] = [S, S + 12345, -4]
    rb = Replay(n, 4)
    rb.push_batch(s, a, r, nx, d)
    q0 = rng.standard_normal((S, A)).astype(dt)
    algo, ref = Algo(S, A, 0.9, seed=0, dtype=np.dtype(dt)), OracleQLearning(S, A, 0.9, dtype=np.dtype(dt))
    algo.q_table = q0
    ref.q_table = q0.copy()
    with pytest.raises(IndexError):
        rb.learn_from(algo, n, 0.1, mode="vec")
    assert np.array_equal(np.asarray(algo.q_table).view(np.uint8), q0.view(np.uint8))
    rb.rng = np.random.default_rng(4)
    i = np.random.default_rng(4).choice(n, n, replace=False)
    idx = rb.learn_from(algo, n, 0.1, mode="iter")
    assert np.array_equal(idx, i)
    ref.learn(s[i].astype(np.int32), a[i].astype(np.int32), r[i].astype(np.float32), nx[i], d[i], 0.1)
    assert np.array_equal(np.asarray(algo.q_table), ref.q_table)
    # a NON-terminated entry outside the table is refused in both modes
    rb.push((1, 1, 0.5, S + 1, False))
    for mode in ("iter", "vec"):
        with pytest.raises(IndexError):
            rb.learn_from(algo, n, 0.1, mode=mode)
        assert np.array_equal(np.asarray(algo.q_table), ref.q_table)
