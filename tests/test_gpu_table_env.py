"""GPU: ``TabularMDPEnv`` (a finite MDP given as tables, ``csrc/qe_envs.h:TableEnv``) through every path of the engine,
bit for bit against the unchanged oracle runtime driving the NumPy model of the environment (tests/table_mdp_model.py):
Q-table, final observations, running returns and episode history, with the kernel build each case means to cover
asserted from ``kernel_variant``."""

import numpy as np
import pytest

from helpers import schedule_params
from oracle.qlearn_oracle import OracleQLearning, OracleRuntime, OracleSchedule
from table_mdp_model import (FROZEN_4x4, FROZEN_8x8, TableMDPVecEnv, frozen_lake_isd, frozen_lake_P, grid_lake_tables,
                             random_mdp)

pytestmark = pytest.mark.gpu


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return OptimalQLearningBase, GpuRolloutQLearning, environments, schedules, _lib


def _mdp(name):
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp, outcome_arrays

    if name == "frozen4":
        return encode_table_mdp(*outcome_arrays(frozen_lake_P(FROZEN_4x4, False)), frozen_lake_isd(FROZEN_4x4))
    if name == "frozen8_slippery":
        return encode_table_mdp(*outcome_arrays(frozen_lake_P(FROZEN_8x8, True)), frozen_lake_isd(FROZEN_8x8))
    if name == "random":
        arrays, isd, _ = random_mdp(500, 6, 3, seed=5)
        return encode_table_mdp(*arrays, isd)
    if name == "random_large":
        arrays, isd, _ = random_mdp(20000, 6, 3, seed=8)
        return encode_table_mdp(*arrays, isd)
    if name == "masked_a9":
        arrays, isd, masks = random_mdp(300, 9, 3, seed=6, masked=True)
        return encode_table_mdp(*arrays, isd, masks)
    if name == "masked_a40":  # two mask words per state
        arrays, isd, masks = random_mdp(200, 40, 2, seed=7, masked=True)
        return encode_table_mdp(*arrays, isd, masks)
    raise KeyError(name)


def _schedules(sch, kind):
    def make(p):
        kind_, value, lo, decay = p
        if kind_ == "exponential":
            return sch.ExponentialSchedule(value, lo, decay)
        if kind_ == "linear":
            return sch.LinearSchedule(value, decay)
        return sch.ConstantSchedule(value)

    lr_p, eps_p = schedule_params(kind)
    return make(lr_p), make(eps_p)


def _oracle(mdp, n, steps, dt, mode, sched="const"):
    env = TableMDPVecEnv(n, mdp, seed=1)
    algo = OracleQLearning(env.state_size, env.action_size, 0.99, seed=0, dtype=np.dtype(dt))
    lr_p, eps_p = schedule_params(sched)
    rt = OracleRuntime(algo, OracleSchedule(*lr_p), OracleSchedule(*eps_p), learn_mode=mode)
    states, _ = env.reset()
    acc = np.zeros(n, dtype=np.float32)
    history = []
    for _ in range(steps):
        states, _ = rt.run_single_step(env, states, acc, history)
    obs = states["observation"] if isinstance(states, dict) else states
    return {"q": algo.q_table, "history": np.array(history, dtype=np.float32), "final_obs": np.asarray(obs, np.int32),
            "agent_rewards": acc, "rt": rt, "env": env}


def _run(mdp, n, steps, dt, mode, path="auto", sched="const", options=()):
    Algo, Runtime, envs, sch, _lib = _product()
    env = envs.TabularMDPEnv(n, mdp, seed=1)
    algo = Algo(env.state_size, env.action_size, 0.99, seed=0, dtype=np.dtype(dt))
    algo.set_rollout_path(path)
    for opt, value in options:
        algo.set_engine_option(opt, value)
    rt = Runtime(algo, *_schedules(sch, sched), learn_mode=mode)
    _avg, history, _env, sd = rt.run_steps(steps, env, None)
    obs, acc = env.observe()
    return {"q": np.asarray(algo.q_table), "history": np.array(history, dtype=np.float32),
            "final_obs": obs["observation"] if isinstance(obs, dict) else obs, "agent_rewards": acc,
            "variant": _lib.decode_variant(rt.last_stats["kernel_variant"]), "rt": rt, "env": env, "sd": sd,
            "algo": algo}


def _same(got, want):
    for k in ("q", "history", "final_obs", "agent_rewards"):
        assert np.array_equal(got[k], want[k]), k
    assert len(want["history"]) > 0  # episodes did end: the start distribution was exercised


# ------------------------------------------------------------------------------- persistent path
@pytest.mark.parametrize(("dt", "mode"), [("f4", "iter"), ("f8", "iter"), ("f4", "vec"), ("f8", "vec")])
@pytest.mark.parametrize("n", [16, 128, 512])
@pytest.mark.parametrize("name", ["frozen4", "frozen8_slippery", "random"])
def test_persistent_path_matches_the_oracle(name, n, dt, mode):
    mdp = _mdp(name)
    steps = 40
    got = _run(mdp, n, steps, dt, mode, path="persistent")
    assert got["variant"]["path"] == "persistent" and not got["variant"]["masked"], got["variant"]
    _same(got, _oracle(mdp, n, steps, dt, mode))


# ------------------------------------------------------------------------------- one launch per step
@pytest.mark.parametrize(("dt", "mode"), [("f4", "iter"), ("f8", "iter"), ("f4", "vec")])
def test_turnstile_path_matches_the_oracle(dt, mode):
    mdp = _mdp("random")
    got = _run(mdp, 4096, 12, dt, mode, path="turnstile")
    assert got["variant"]["path"] == "turnstile", got["variant"]
    _same(got, _oracle(mdp, 4096, 12, dt, mode))


@pytest.mark.parametrize("path", ["stepwise", "wide"])
@pytest.mark.parametrize(("dt", "mode"), [("f4", "iter"), ("f8", "vec")])
def test_forced_step_wise_and_wide_paths_match_the_oracle(path, dt, mode):
    mdp = _mdp("random")
    got = _run(mdp, 1000, 15, dt, mode, path=path)
    assert got["variant"]["path"] == path, got["variant"]
    _same(got, _oracle(mdp, 1000, 15, dt, mode))


def test_more_than_sixty_thousand_agents_match_the_oracle():
    # (the turnstile path takes up to 60 000 agents, csrc/qe_host.h:turn_fits; beyond it the automatic choice is the
    # step-wise / wide path)
    mdp = _mdp("random_large")
    got = _run(mdp, 70000, 6, "f4", "vec")
    assert got["variant"]["path"] in ("stepwise", "wide"), got["variant"]
    _same(got, _oracle(mdp, 70000, 6, "f4", "vec"))


# ------------------------------------------------------------------------------- masks
@pytest.mark.parametrize(("n", "path", "dt", "mode"), [
    (64, "persistent", "f4", "iter"), (128, "persistent", "f8", "vec"), (700, "turnstile", "f4", "iter"),
    (600, "stepwise", "f8", "iter"),
])
@pytest.mark.parametrize("name", ["masked_a9", "masked_a40"])
def test_masked_tables_match_the_oracle(name, n, path, dt, mode):
    mdp = _mdp(name)
    got = _run(mdp, n, 30, dt, mode, path=path)
    assert got["variant"]["path"] == path, got["variant"]
    if path == "persistent":
        assert got["variant"]["masked"]
    _same(got, _oracle(mdp, n, 30, dt, mode))
    obs, _ = got["env"].observe()
    assert np.array_equal(obs["action_mask"].astype(bool), mdp.masks[obs["observation"]])


def test_all_false_mask_row_raises_index_error():
    _, _, envs, _, _ = _product()
    nxt, rew, term = grid_lake_tables(4)
    masks = np.ones((16, 4), dtype=bool)
    masks[0] = False  # the start state has no valid action
    mdp = envs.TabularMDPEnv.from_arrays(8, nxt, rew, term, action_masks=masks).mdp
    with pytest.raises(IndexError):
        _run(mdp, 8, 5, "f4", "iter", sched="explore")


@pytest.mark.parametrize("how", ["evaluate_steps", "evaluate_episodes"])
def test_evaluating_from_a_fully_masked_start_state_raises_index_error(how):
    # (greedy evaluation reports an agent without a selectable action as the training kernels do, and steps the table
    # with action 0 instead: the action indexes the outcome records)
    Algo, Runtime, envs, sch, _ = _product()
    nxt, rew, term = grid_lake_tables(4)
    masks = np.ones((16, 4), dtype=bool)
    masks[0] = False
    env = envs.TabularMDPEnv.from_arrays(8, nxt, rew, term, action_masks=masks)
    rt = Runtime(Algo(16, 4, 0.99, seed=0), *_schedules(sch, "const"))
    with pytest.raises(IndexError):
        getattr(rt, how)(env, 40 if how == "evaluate_steps" else 5)


@pytest.mark.parametrize("kind", ["table", "hash"])
def test_evaluating_a_nan_table_raises_index_error(kind):
    # 12 actions: greedy evaluation takes np.max of the row (the reference's NumPy variants), a NaN maximum ties with
    # no action and the reference raises IndexError (q_learning_optimal.py:470) -- for the built-in environments too
    Algo, Runtime, envs, sch, _ = _product()
    if kind == "table":
        arrays, isd, _ = random_mdp(50, 12, 2, seed=9)
        env = envs.TabularMDPEnv(16, _encode(arrays, isd))
    else:
        env = envs.HashTabularEnv(16, 50, 12, seed=1)
    algo = Algo(50, 12, 0.99, seed=0)
    algo.q_table = np.full((50, 12), np.nan, dtype=np.float32)
    rt = Runtime(algo, *_schedules(sch, "const"))
    with pytest.raises(IndexError):
        rt.evaluate_steps(env, 16 * 10)


def _encode(arrays, isd=None, masks=None):
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    return encode_table_mdp(*arrays, isd, masks)


# ------------------------------------------------------------------------------- host-driven loop, evaluation, resume
@pytest.mark.parametrize("name", ["frozen8_slippery", "masked_a9"])
def test_host_driven_env_step_matches_the_model(name):
    Algo, _, envs, _, _ = _product()
    mdp = _mdp(name)
    n = 200
    env = envs.TabularMDPEnv(n, mdp, seed=3)
    model = TableMDPVecEnv(n, mdp, seed=3)
    algo = Algo(env.state_size, env.action_size, 0.99, seed=0)
    env.bind(algo)
    obs, _ = env.reset()
    want, _ = model.reset()
    rng = np.random.default_rng(0)
    ended = 0
    for t in range(25):
        o = obs["observation"] if isinstance(obs, dict) else obs
        w = want["observation"] if isinstance(want, dict) else want
        assert np.array_equal(o, w), t
        if isinstance(obs, dict):
            assert np.array_equal(obs["action_mask"], want["action_mask"]), t
            valid = obs["action_mask"].astype(bool)
            actions = np.array([rng.choice(np.flatnonzero(v)) for v in valid], dtype=np.int32)
        else:
            actions = rng.integers(0, env.action_size, size=n).astype(np.int32)
        algo.choose_actions(o, 0.5, action_masks=obs["action_mask"] if isinstance(obs, dict) else None)  # step index
        model.step_index = t
        obs, r, te, tr, _ = env.step(actions)
        want, wr, wte, wtr, _ = model.step(actions)
        assert np.array_equal(r, wr) and np.array_equal(te, wte) and not tr.any(), t
        ended += int(te.sum())
    assert ended > 0
    assert np.array_equal(env.aux(), np.zeros(n, dtype=np.uint32))
    obs2, _ = env.reset(seed=9)  # re-seeds, as TicTacToe does
    want2, _ = model.reset(seed=9)
    o2 = obs2["observation"] if isinstance(obs2, dict) else obs2
    w2 = want2["observation"] if isinstance(want2, dict) else want2
    assert np.array_equal(o2, w2)


def test_evaluate_steps_and_episodes_match_the_oracle():
    mdp = _mdp("frozen8_slippery")
    n = 128
    got = _run(mdp, n, 60, "f4", "iter", sched="bench")
    want = _oracle(mdp, n, 60, "f4", "iter", sched="bench")
    _same(got, want)
    total, hist = got["rt"].evaluate_steps(got["env"], 30 * n)
    assert got["rt"].last_stats and _product()[4].decode_variant(got["rt"].last_stats["kernel_variant"])["path"] == "eval"
    wtotal, whist = want["rt"].evaluate_steps(want["env"], 30 * n)
    assert np.array_equal(np.array(hist, np.float32), np.array(whist, np.float32)) and total == wtotal
    total, hist = got["rt"].evaluate_episodes(got["env"], 100)
    wtotal, whist = want["rt"].evaluate_episodes(want["env"], 100)
    assert np.array_equal(np.array(hist, np.float32), np.array(whist, np.float32)) and total == wtotal
    assert np.array_equal(np.asarray(got["algo"].q_table), want["q"])  # evaluation does not learn


@pytest.mark.parametrize("name", ["random", "masked_a9"])
def test_two_resumed_calls_equal_one(name):
    Algo, Runtime, envs, sch, _ = _product()
    mdp = _mdp(name)
    n = 96
    one = _run(mdp, n, 100, "f4", "iter", sched="bench")
    algo = Algo(mdp.state_size, mdp.action_size, 0.99, seed=0)
    rt = Runtime(algo, *_schedules(sch, "bench"))
    _, h1, _, sd = rt.run_steps(50, envs.TabularMDPEnv(n, mdp, seed=1), None)
    sd = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in sd.items()}  # a copy: not resident
    env2 = envs.TabularMDPEnv(n, mdp, seed=1)  # a fresh environment object: the state comes from the dict
    _, h2, _, sd2 = rt.run_steps(50, env2, sd)
    assert np.array_equal(np.asarray(algo.q_table), one["q"])
    assert np.array_equal(np.array(list(h1) + list(h2), np.float32), one["history"])
    obs = sd2["states"]["observation"] if isinstance(sd2["states"], dict) else sd2["states"]
    assert np.array_equal(obs, one["final_obs"])


# ------------------------------------------------------------------------------- cross-check without the oracle
@pytest.mark.parametrize(("n", "dt", "mode"), [(64, "f4", "iter"), (512, "f8", "vec"), (3000, "f4", "iter")])
def test_table_listing_grid_lake_equals_grid_lake(n, dt, mode):
    Algo, Runtime, envs, sch, _ = _product()
    out = []
    for env in (envs.GridLakeEnv(n, side=6, seed=1), envs.TabularMDPEnv.from_arrays(n, *grid_lake_tables(6, seed=1))):
        algo = Algo(36, 4, 0.99, seed=0, dtype=np.dtype(dt))
        rt = Runtime(algo, *_schedules(sch, "bench"), learn_mode=mode)
        _, hist, _, sd = rt.run_steps(80, env, None)
        out.append((np.asarray(algo.q_table), np.array(hist, np.float32), np.asarray(sd["states"]), sd["rewards"]))
    assert len(out[0][1]) > 0
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------- rejected tables
def test_the_engine_rejects_bad_tables():
    Algo, _, envs, _, _lib = _product()
    good = _mdp("frozen4")
    algo = Algo(16, 4, 0.99, seed=0)

    def bind(mdp):
        envs.TabularMDPEnv(4, mdp).bind(algo)

    bind(good)
    bad_next = good.next_state.copy()
    bad_next[3, 2, 0] = 16
    with pytest.raises(IndexError):
        bind(good._replace(next_state=bad_next))
    with pytest.raises(IndexError):
        bind(good._replace(start_state=np.array([-1], np.int32)))
    wide = lambda a: np.repeat(a, 9, axis=2)  # noqa: E731
    with pytest.raises(ValueError):  # nine outcome slots
        bind(good._replace(thr=wide(good.thr), next_state=wide(good.next_state), reward=wide(good.reward),
                           terminated=wide(good.terminated)))
    with pytest.raises(ValueError):  # start thresholds out of order
        bind(good._replace(start_thr=np.array([5, 3], np.uint32), start_state=np.array([0, 1], np.int32)))
    with pytest.raises(ValueError):  # the table's shape is not the algorithm's
        envs.TabularMDPEnv(4, _mdp("random")).bind(algo)
    plain = envs.DeviceVecEnv(4, 16, 4, _lib.EnvParams(kind=_lib.ENV_TABLE))  # tables only through qe_env_create_table
    with pytest.raises(ValueError):
        plain.bind(algo)
