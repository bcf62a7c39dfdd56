"""GPU: every transition of the device environments through the host-driven entry points (``qe_env_restore``,
``qe_env_step``, ``qe_env_observe`` with masks, ``qe_env_aux``, ``qe_env_reset`` with a seed), bit for bit against the
cases of tests/env_cases.py -- the reference's TicTacToe table, the oracle's environments and the table model.  These
entry points run the ``Env::step`` / ``Env::valid4`` / ``Env::reset`` bodies of ``csrc/qe_envs.h`` that every fused
kernel inlines, and with restore + step counter any agent can be put in any state at any draw index: the environments are
checked exhaustively, not along a trajectory.  Plus: what an environment reports after a rollout of ANOTHER environment
on the same engine (the page-locked result blocks belong to the engine's slots, not to an environment)."""

import ctypes as C

import numpy as np
import pytest

import env_cases as ec
from helpers import schedule_params
from oracle.envs import HashTabularEnv as OracleHashEnv

pytestmark = pytest.mark.gpu


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return OptimalQLearningBase, GpuRolloutQLearning, environments, schedules, _lib


def _split(env, states):
    if env.masked:
        return states["observation"], states["action_mask"].astype(bool)
    return states, None


def _observed(env, obs, masks, acc, aux, what):
    got, got_acc = env.observe()
    got_obs, got_masks = _split(env, got)
    assert np.array_equal(got_obs, obs), what + ": observe() observations"
    assert np.array_equal(got_acc, acc), what + ": observe() running returns"
    if env.masked:
        assert np.array_equal(got_masks, masks), what + ": observe() masks"
    assert np.array_equal(env.aux(), aux), what + ": aux()"


def _check(env, algo, case, what=""):
    """restore -> (observe: the restored state and its masks) -> step at the case's draw index -> compare -> observe."""
    zeros = np.zeros(case.n, dtype=np.float32)
    env.restore(case.obs, zeros, case.aux)
    _observed(env, case.obs, case.start_masks, zeros, case.aux, what + " restored")
    algo.step_counter = (case.step + 1) & 0xFFFFFFFFFFFFFFFF  # qe_env_step draws at step_counter - 1
    states, reward, terminated, truncated, _ = env.step(case.actions)
    obs, masks = _split(env, states)
    assert np.array_equal(obs, case.next_obs), what + ": next observations"
    assert np.array_equal(reward, case.reward), what + ": rewards"
    assert np.array_equal(terminated, case.terminated), what + ": terminated"
    assert not truncated.any()
    if env.masked:
        assert np.array_equal(masks, case.masks), what + ": masks returned by step"
    _observed(env, case.next_obs, case.masks, zeros, case.next_aux, what + " stepped")


# ------------------------------------------------------------------------------- TicTacToe
@pytest.fixture(scope="module")
def ttt_engine():
    Algo, _, envs, _, _ = _product()
    return Algo(19683, 9, 0.99, seed=0), envs


def test_tictactoe_every_position_action_and_reply_equals_the_reference(ttt_engine):
    """All 16 167 (position, action) pairs x 32 replicas at step 0 and at 2^32 + 5: together every one of the 43 644
    replies the reference offers and all 10 openings (tests/test_env_transition_cases.py asserts both)."""
    algo, envs = ttt_engine
    env = envs.TicTacToeEnv(len(ec.ttt_table().pair_row) * ec.TTT_D, seed=ec.TTT_SEED).bind(algo)
    for step in ec.TTT_STEPS:
        _check(env, algo, ec.ttt_case(step), f"step {step}")


def test_tictactoe_masks_of_every_observation_id(ttt_engine):
    from oracle.envs import TicTacToeVecEnv

    algo, envs = ttt_engine
    ids = np.arange(19683, dtype=np.int32)
    env = envs.TicTacToeEnv(len(ids), seed=ec.TTT_SEED).bind(algo)
    env.restore(ids, None, None)
    got, _ = env.observe()
    assert np.array_equal(got["observation"], ids)
    assert np.array_equal(got["action_mask"], TicTacToeVecEnv(1).action_masks(ids))


def test_tictactoe_step_at_the_reset_word(ttt_engine):
    """step_counter == 0: the step index is 2^64 - 1, the word reset() draws from."""
    algo, envs = ttt_engine
    t = ec.ttt_table()
    c, first = t.cols, t.pair_row
    case = ec.ttt_oracle_case(c["m1"][first], c["m2"][first], c["mark"][first], c["action"][first], ec.RESET_STEP)
    env = envs.TicTacToeEnv(case.n, seed=ec.TTT_SEED).bind(algo)
    _check(env, algo, case, "reset word")
    assert algo.step_counter == 0


def test_tictactoe_actions_on_occupied_cells_equal_the_oracle(ttt_engine):
    algo, envs = ttt_engine
    case = ec.ttt_occupied_cell_case()
    env = envs.TicTacToeEnv(case.n, seed=ec.TTT_SEED).bind(algo)
    _check(env, algo, case, "occupied cells")


@pytest.mark.parametrize("crossing", [False, True])
def test_tictactoe_reset_with_and_without_a_seed(ttt_engine, crossing):
    algo, envs = ttt_engine
    n = 300
    offset = ec.crossing_offset(n) if crossing else 0
    env = envs.TicTacToeEnv(n, seed=ec.TTT_SEED, agent_offset=offset).bind(algo)
    zeros = np.zeros(n, dtype=np.float32)
    # the constructor's seed, then seed 9, then no seed again: the environment keeps seed 9
    for made_with, reseed in ((ec.TTT_SEED, None), (ec.TTT_SEED, 9), (9, None)):
        obs, masks, aux = ec.ttt_reset_expected(n, made_with, offset, reseed)
        env.restore(np.full(n, 7, dtype=np.int32), np.ones(n, dtype=np.float32), np.full(n, 3, dtype=np.uint32))
        got, _ = env.reset(seed=reseed)
        assert np.array_equal(got["observation"], obs) and np.array_equal(got["action_mask"].astype(bool), masks), reseed
        _observed(env, obs, masks, zeros, aux, f"reset(seed={reseed})")
        assert len(np.unique(aux)) == 10  # every opening among the 300 agents


# ------------------------------------------------------------------------------- hash
@pytest.mark.parametrize(("S", "A", "masked"), ec.HASH_SHAPES)
def test_hash_every_state_action_pair(S, A, masked):
    Algo, _, envs, _, _ = _product()
    algo = Algo(S, A, 0.99, seed=0)
    n = S * A
    for offset in (0, ec.crossing_offset(n)):
        for p in ec.HASH_P_TERM:
            env = envs.HashTabularEnv(n, S, A, seed=ec.HASH_SEED, p_term_256=p, masked=masked, agent_offset=offset).bind(algo)
            _check(env, algo, ec.hash_case(S, A, masked, p, agent_offset=offset), f"p_term {p}, offset {offset}")
        env = envs.HashTabularEnv(n, S, A, seed=ec.HASH_SEED, p_term_256=128, masked=masked, agent_offset=offset).bind(algo)
        obs, aux = ec.hash_reset_expected(n, S, A, ec.HASH_SEED, offset, reseed=5)
        got, _ = env.reset(seed=5)  # start states, and from here on successors, rewards and masks, are those of seed 5
        assert np.array_equal(_split(env, got)[0], obs) and np.array_equal(env.aux(), aux)
        _check(env, algo, ec.hash_case(S, A, masked, 128, agent_offset=offset, seed=5), f"re-seeded, offset {offset}")


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_hash_tail_blocks_and_refusals(n):
    """The last block of ``k_env_step`` (256 agents per block) and, at one agent of 33 actions, of ``k_env_masks``; and the
    calls the entry points refuse leave the environment as it was."""
    Algo, _, envs, _, _ = _product()
    S, A = 300, 33
    algo = Algo(S, A, 0.99, seed=0)
    for offset in (0, ec.crossing_offset(n)):
        env = envs.HashTabularEnv(n, S, A, seed=ec.HASH_SEED, p_term_256=128, masked=True, agent_offset=offset).bind(algo)
        case = ec.hash_case(S, A, True, 128, agent_offset=offset, n=n)
        _check(env, algo, case, f"offset {offset}")
        zeros = np.zeros(n, dtype=np.float32)
        for bad in (S, -1):
            obs = case.obs.copy()
            obs[n - 1] = bad
            with pytest.raises(IndexError):
                env.restore(obs, np.ones(n, dtype=np.float32), case.aux)
        for bad in (A, -1):
            actions = case.actions.copy()
            actions[n - 1] = bad
            with pytest.raises(IndexError):
                env.step(actions)
        _observed(env, case.next_obs, case.masks, zeros, case.next_aux, "after the refused calls")
        assert algo.step_counter == case.step + 1


# ------------------------------------------------------------------------------- grid
@pytest.mark.parametrize("side", ec.GRID_SIDES)
def test_grid_every_cell_and_action(side):
    Algo, _, envs, _, _ = _product()
    algo = Algo(side * side, 4, 0.99, seed=0)
    n = 4 * side * side
    made = {seed: envs.GridLakeEnv(n, side=side, seed=seed).bind(algo) for seed in ec.GRID_SEEDS}
    for seed, env in made.items():
        _check(env, algo, ec.grid_case(side, seed), f"seed {seed}")
    env = made[1]
    got, _ = env.reset(seed=7)  # moves the holes
    assert not got.any() and not env.aux().any()
    _check(env, algo, ec.grid_case(side, 7), "seed 1 re-seeded with 7")


# ------------------------------------------------------------------------------- bandit
@pytest.mark.parametrize("episode_len", ec.BANDIT_LENGTHS)
def test_bandit_every_position_in_the_episode(episode_len):
    Algo, _, envs, _, _ = _product()
    algo = Algo(1, 2, 0.99, seed=0)
    env = envs.RiggedTwoArmedBanditVecEnv(2 * episode_len, episode_len=episode_len).bind(algo)
    _check(env, algo, ec.bandit_case(episode_len))


# ------------------------------------------------------------------------------- table
@pytest.mark.parametrize("name", list(ec.TABLE_SHAPES))
def test_table_every_cell_slot_and_start_state(name):
    Algo, _, envs, _, _ = _product()
    mdp = ec.table_mdp(name)
    algo = Algo(mdp.state_size, mdp.action_size, 0.99, seed=0)
    n = mdp.state_size * mdp.action_size * ec.TABLE_D
    for offset in (0, ec.crossing_offset(n)):
        env = envs.TabularMDPEnv(n, mdp, seed=ec.TABLE_SEED, agent_offset=offset).bind(algo)
        for step in ec.TABLE_STEPS:
            _check(env, algo, ec.table_case(name, step, agent_offset=offset), f"step {step}, offset {offset}")


# ------------------------------------------------------------------------------- two environments on one engine
def _const_schedules(sch):
    lr_p, eps_p = schedule_params("const")
    return sch.ConstantSchedule(lr_p[1]), sch.ConstantSchedule(eps_p[1])


def _two_envs(envs):
    p = ec.TWO_ENV
    return {"A": envs.HashTabularEnv(p["A_agents"], p["S"], p["A"], seed=p["A_seed"]),
            "B": envs.HashTabularEnv(p["B_agents"], p["S"], p["A"], seed=p["B_seed"])}


def _reports(env, stage, what):
    """observe(), aux() and state_dict() of `env` are the oracle's state of that environment after `stage`."""
    _observed(env, stage["obs"], None, stage["acc"], stage["aux"], what)
    sd = env.state_dict()
    assert np.array_equal(sd["states"], stage["obs"]), what + ": state_dict() observations"
    assert np.array_equal(sd["rewards"], stage["acc"]), what + ": state_dict() running returns"
    assert np.array_equal(sd["aux"], stage["aux"]), what + ": state_dict() aux"
    return sd


@pytest.mark.parametrize("through_slot_1", [False, True])
@pytest.mark.parametrize("first", ["A", "B"])
def test_an_environment_reports_its_own_state_after_a_rollout_of_another(first, through_slot_1):
    Algo, Runtime, envs, sch, _lib = _product()
    p = ec.TWO_ENV
    stages = ec.two_env_curriculum(first)
    made = _two_envs(envs)
    x, y = made[first], made["B" if first == "A" else "A"]
    algo = Algo(p["S"], p["A"], 0.99, seed=0)
    rt = Runtime(algo, *_const_schedules(sch))

    _, history, _, _ = rt.run_steps(p["steps"], x, None)
    assert _lib.decode_variant(rt.last_stats["kernel_variant"])["path"] == "persistent"
    assert np.array_equal(np.array(history, dtype=np.float32), stages[0]["history"])
    _reports(x, stages[0], "first environment after its own rollout")

    if through_slot_1:
        lib = _lib.load()
        y.bind(algo)
        y.reset_device()
        lr_p, eps_p = schedule_params("const")
        eps, lr = np.full(p["steps"], eps_p[1]), np.full(p["steps"], lr_p[1])
        st = _lib.RolloutStats()
        _lib.check(lib.qe_rollout_begin(algo.handle, y.handle, p["steps"], _lib.ptr(eps, C.c_double),
                                        _lib.ptr(lr, C.c_double), _lib.LEARN_ITER, 1))
        _lib.check(lib.qe_rollout_end(algo.handle, 1, C.byref(st)))
        variant, episodes = st.kernel_variant, int(st.episodes)
    else:
        _, history, _, _ = rt.run_steps(p["steps"], y, None)
        variant, episodes = rt.last_stats["kernel_variant"], len(history)
    assert _lib.decode_variant(variant)["path"] == "persistent"
    assert episodes == len(stages[1]["history"])
    assert algo.step_counter == stages[1]["step_counter"]

    sd = _reports(x, stages[0], "first environment after the other one's rollout")
    _reports(y, stages[1], "second environment after its own rollout")
    _reports(x, stages[0], "first environment, asked again")

    # the checkpoint a curriculum would write, handed back as a copy (so that it is restored, not recognised)
    sd = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in sd.items()}
    _, history, _, sd2 = rt.run_steps(p["more"], x, sd)
    assert _lib.decode_variant(rt.last_stats["kernel_variant"])["path"] == "persistent"
    assert np.array_equal(np.array(history, dtype=np.float32), stages[2]["history"])
    assert np.array_equal(np.asarray(algo.q_table), stages[2]["q"])
    assert np.array_equal(sd2["states"], stages[2]["obs"]) and np.array_equal(sd2["rewards"], stages[2]["acc"])
    _reports(x, stages[2], "first environment after its second rollout")
    _reports(y, stages[1], "second environment after the first one's second rollout")


def test_a_host_driven_step_after_a_rollout_shows_the_stepped_state():
    Algo, Runtime, envs, sch, _lib = _product()
    p = ec.TWO_ENV
    stage = ec.two_env_curriculum("A")[0]
    env = _two_envs(envs)["A"]
    algo = Algo(p["S"], p["A"], 0.99, seed=0)
    rt = Runtime(algo, *_const_schedules(sch))
    rt.run_steps(p["steps"], env, None)
    assert _lib.decode_variant(rt.last_stats["kernel_variant"])["path"] == "persistent"
    model = OracleHashEnv(p["A_agents"], p["S"], p["A"], seed=p["A_seed"])
    model.obs, model.episode = stage["obs"].copy(), stage["aux"].copy()
    actions = ((np.arange(p["A_agents"]) * 3) % p["A"]).astype(np.int32)
    want, reward, terminated, _, _ = model.step(actions)
    got, got_reward, got_terminated, _, _ = env.step(actions)
    assert np.array_equal(got, want) and np.array_equal(got_reward, reward) and np.array_equal(got_terminated, terminated)
    assert not np.array_equal(want, stage["obs"])  # the step moved the agents: the mirror of the rollout would be stale
    _observed(env, want, None, stage["acc"], model.episode, "after the host-driven step")
