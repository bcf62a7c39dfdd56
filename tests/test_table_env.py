"""CPU: the encoding of a finite MDP for ``TabularMDPEnv`` (thresholds, support lists, gymnasium's ``P`` format), the
validation that happens before the engine is reached, and the code generation of the ``TableEnv`` kernel builds."""

import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from table_mdp_model import FROZEN_4x4, TableMDPVecEnv, frozen_lake_isd, frozen_lake_P

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TOP = 0xFFFFFFFF


def _enc(outcomes, isd=None, masks=None, S=None):
    """One (state, action) with the given [(prob, next, reward, term), ...] (or an [S, A, K] list of lists)."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp, outcome_arrays

    if S is not None:
        outcomes = [[outcomes]] + [[[(1.0, 0, 0.0, False)]] for _ in range(S - 1)]
    return encode_table_mdp(*outcome_arrays(outcomes), isd, masks)


# ------------------------------------------------------------------------------- encoding
def test_thresholds_hand_computed():
    m = _enc([(0.25, 1, 1.0, False), (0.5, 2, 2.0, False), (0.25, 3, 3.0, True)], S=4)
    assert m.k == 3
    assert m.thr[0, 0].tolist() == [2**30, 3 * 2**30, TOP]
    assert m.next_state[0, 0].tolist() == [1, 2, 3]
    assert m.reward[0, 0].tolist() == [1.0, 2.0, 3.0]
    assert m.terminated[0, 0].tolist() == [False, False, True]
    # the other states: one outcome, padded with copies of it
    assert m.thr[1, 0].tolist() == [TOP] * 3 and m.next_state[1, 0].tolist() == [0, 0, 0]
    # default start distribution: state 0
    assert m.start_state.tolist() == [0] and m.start_thr.tolist() == [TOP]


def test_probabilities_that_do_not_sum_to_one():
    # 1 : 3 -> thr_0 = floor(0.25 * 2^32)
    m = _enc([(2.0, 1, 0.0, False), (6.0, 2, 0.0, False)], S=3)
    assert m.thr[0, 0].tolist() == [2**30, TOP]
    # 1/3 in float64: floor(cumsum / sum * 2^32) exactly as documented
    m = _enc([(0.1, 1, 0.0, False), (0.2, 2, 0.0, False)], S=3)
    assert m.thr[0, 0, 0] == int(np.floor(0.1 / (0.1 + 0.2) * 2.0**32))


def test_zero_probability_outcomes_are_dropped():
    m = _enc([(0.0, 1, 9.0, True), (0.5, 2, 2.0, False), (0.0, 3, 9.0, True), (0.5, 4, 4.0, False), (0.0, 1, 9.0, True)],
             S=5)
    assert m.k == 2
    assert m.thr[0, 0].tolist() == [2**31, TOP]
    assert m.next_state[0, 0].tolist() == [2, 4]
    assert m.reward[0, 0].tolist() == [2.0, 4.0]


def test_single_outcome_and_rewards_rounded_to_float32():
    m = _enc([(0.7, 1, 0.1, True)], S=2)
    assert m.k == 1 and m.thr[0, 0].tolist() == [TOP]
    assert m.reward.dtype == np.float32 and m.reward[0, 0, 0] == np.float32(0.1)
    assert m.terminated[0, 0, 0]


def test_eight_outcomes():
    m = _enc([(1.0, j, float(j), False) for j in range(8)], S=8)
    assert m.k == 8
    assert m.thr[0, 0].tolist() == [(j + 1) * 2**29 for j in range(7)] + [TOP]
    assert m.next_state[0, 0].tolist() == list(range(8))


def test_threshold_clamped_below_two_to_the_32():
    # cumsum / sum == 1.0 before the last outcome (a zero tail is dropped, a tiny one is not): clamp to 2^32 - 1
    m = _enc([(1.0, 1, 0.0, False), (1e-30, 2, 0.0, False)], S=3)
    assert m.thr[0, 0].tolist() == [TOP, TOP]


def test_start_support():
    isd = np.zeros(6)
    isd[[1, 4, 5]] = [1.0, 0.0, 3.0]
    isd[2] = 0.0
    m = _enc([(1.0, 0, 0.0, False)], isd=isd, S=6)
    assert m.start_state.tolist() == [1, 5]
    assert m.start_thr.tolist() == [2**30, TOP]


def test_frozen_lake_4x4_slippery_transition_dict():
    from dist_classicrl_amd.environments import TabularMDPEnv

    P = frozen_lake_P(FROZEN_4x4, is_slippery=True)
    env = TabularMDPEnv.from_transition_dict(P, 3, initial_state_distrib=frozen_lake_isd(FROZEN_4x4))
    m = env.mdp
    assert (env.state_size, env.action_size, m.k) == (16, 4, 3)
    third = [int(np.floor(1 / 3 * 2.0**32)), int(np.floor((1 / 3 + 1 / 3) / (1 / 3 + 1 / 3 + 1 / 3) * 2.0**32)), TOP]
    assert m.thr[0, 0].tolist() == third
    assert m.next_state[0, 0].tolist() == [0, 0, 4]  # left from the corner: up, left stay; down to 4
    assert m.next_state[14, 2].tolist() == [14, 15, 10]  # right, next to the goal on the bottom row: down, right, up
    assert m.reward[14, 2].tolist() == [0.0, 1.0, 0.0]
    assert m.terminated[14, 2].tolist() == [False, True, False]
    assert m.terminated[5, 1].tolist() == [True] * 3 and m.thr[5, 1].tolist() == [TOP] * 3  # hole: absorbing, K = 1
    assert m.start_state.tolist() == [0] and not env.masked


def test_dense_constructor():
    from dist_classicrl_amd.environments import TabularMDPEnv

    nxt = np.array([[1, 0], [1, 0]])
    env = TabularMDPEnv.from_arrays(2, nxt, np.array([[0.5, 0], [1, 0]]), np.array([[False, False], [True, False]]),
                                    action_masks=np.array([[1, 1], [0, 1]]))
    assert env.mdp.k == 1 and env.masked
    assert env.mdp.next_state[..., 0].tolist() == [[1, 0], [1, 0]]
    assert env.mdp.masks.tolist() == [[True, True], [False, True]]


def test_model_samples_by_the_documented_rule():
    """The NumPy model's draw: frequencies of a 1:2:1 outcome list over many agents are close to the probabilities."""
    m = _enc([(0.25, 1, 0.0, False), (0.5, 2, 0.0, False), (0.25, 3, 0.0, False)], S=4)
    env = TableMDPVecEnv(20000, m, seed=3)
    env.reset()
    obs, *_ = env.step(np.zeros(20000, dtype=np.int32))
    freq = np.bincount(obs, minlength=4) / 20000
    assert np.allclose(freq, [0, 0.25, 0.5, 0.25], atol=0.02)


# ------------------------------------------------------------------------------- validation
@pytest.mark.parametrize(("outcomes", "exc"), [
    ([(1.0, 5, 0.0, False)], IndexError),                         # next state out of range
    ([(1.0, -1, 0.0, False)], IndexError),
    ([(-0.5, 1, 0.0, False), (1.5, 1, 0.0, False)], ValueError),  # negative probability
    ([(0.0, 1, 0.0, False)], ValueError),                         # no positive probability
    ([(float("nan"), 1, 0.0, False)], ValueError),
    ([(0.1, 1, 0.0, False)] * 9, ValueError),                      # more than eight outcomes
    ([(1.0, 1, 0.0)], ValueError),                                # not a 4-tuple
    ([], ValueError),                                             # no outcome
    ([(1.0, 1.5, 0.0, False)], ValueError),                       # next state not an integer
    ([(1.0, 1, float("inf"), False)], ValueError),                # reward not finite
    ([(1.0, 1, float("nan"), False)], ValueError),
    ([(1.0, 1, 1e39, False)], ValueError),                        # reward overflows float32
])
def test_bad_transitions_are_rejected_in_python(outcomes, exc):
    from dist_classicrl_amd.environments import TabularMDPEnv

    with pytest.raises(exc):
        TabularMDPEnv(4, [[outcomes], [[(1.0, 0, 0.0, False)]]])


def test_bad_shapes_are_rejected_in_python():
    from dist_classicrl_amd.environments import TabularMDPEnv

    ok = [[[(1.0, 1, 0.0, False)], [(1.0, 0, 0.0, False)]], [[(1.0, 0, 0.0, True)], [(1.0, 1, 0.0, False)]]]
    TabularMDPEnv(2, ok)
    with pytest.raises(ValueError):
        TabularMDPEnv(2, [ok[0], ok[1][:1]])  # ragged action count
    with pytest.raises(ValueError):
        TabularMDPEnv(2, ok, initial_state_distrib=[1.0, 0.0, 0.0])  # wrong length
    with pytest.raises(ValueError):
        TabularMDPEnv(2, ok, initial_state_distrib=[0.0, 0.0])  # no support
    with pytest.raises(ValueError):
        TabularMDPEnv(2, ok, initial_state_distrib=[-1.0, 2.0])
    with pytest.raises(ValueError):
        TabularMDPEnv(2, ok, action_masks=np.ones((2, 3), dtype=bool))
    with pytest.raises(ValueError):
        TabularMDPEnv(2, {0: ok[0], 2: ok[1]})  # states must be 0 .. S-1
    with pytest.raises(IndexError):
        TabularMDPEnv.from_arrays(2, np.array([[0, 2], [1, 1]]), 0.0, False)
    with pytest.raises(ValueError):
        TabularMDPEnv.from_arrays(2, np.array([0, 1]), 0.0, False)
    with pytest.raises(ValueError):  # a reward that does not fit float32
        TabularMDPEnv.from_arrays(2, np.array([[0, 1], [1, 1]]), np.array([[0.0, 3.5e38], [0.0, 0.0]]), False)
    with pytest.raises(ValueError):
        TabularMDPEnv.from_arrays(2, np.array([[0.0, 1.5], [1.0, 1.0]]), 0.0, False)  # next states not integers


def test_integral_next_states_and_largest_float32_reward_are_accepted():
    from dist_classicrl_amd.environments import TabularMDPEnv

    big = float(np.finfo(np.float32).max)
    env = TabularMDPEnv(2, [[[(1.0, 1.0, big, False)]], [[(1.0, np.int64(0), -big, True)]]])
    assert env.mdp.next_state[..., 0].tolist() == [[1], [0]]
    assert env.mdp.reward[..., 0].tolist() == [[big], [-big]]


# ------------------------------------------------------------------------------- code generation
def _assembly(unit, tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_table") / f"{unit}.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
           "-DQE_INST_T=float", "-DQE_INST_ENV=TableEnv", "-S", "--cuda-device-only", str(CSRC / f"qe_inst_{unit}.hip"),
           "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def _kernels(lines):
    """{kernel symbol: {NumVgprs, ScratchSize}} of every TableEnv kernel in a listing."""
    out, name = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+TableEnv\w*):", l)
        if m:
            name = m.group(1)
        m = re.search(r"; (NumVgprs|ScratchSize): (\d+)", l)
        if name and m:
            out.setdefault(name, {})[m.group(1)] = int(m.group(2))
        if name and "; Occupancy" in l:
            name = None
    return out


@pytest.fixture(scope="module")
def table_kernels(tmp_path_factory):
    return {unit: _kernels(_assembly(unit, tmp_path_factory)) for unit in ("lane", "step")}


# The generic 512-agent persistent builds for rows of 16 loads (33 .. 64 actions) spill for every environment that has
# them, HashEnv's included; they are the register file's limit of that build, not the table's.
SPILLING_GENERIC = ("k_rollout_laneIfNS_8TableEnvELi16ELi512E",)


def test_table_env_builds_do_not_spill(table_kernels):
    assert any("k_rollout_lane" in k for k in table_kernels["lane"])
    assert any("k_step_turn" in k for k in table_kernels["step"])
    checked = 0
    for unit, ks in table_kernels.items():
        for name, meta in ks.items():
            if any(p in name for p in SPILLING_GENERIC):
                continue
            assert meta.get("ScratchSize") == 0, (unit, name, meta)
            checked += 1
    assert checked >= 25


def test_table_env_turnstile_kernel_keeps_four_workgroups_per_cu(table_kernels):
    turn = {k: v for k, v in table_kernels["step"].items() if "k_step_turnIfNS_8TableEnvELi0E" in k}
    assert len(turn) == 2, list(table_kernels["step"])  # learn_iter and learn_vec builds
    for name, meta in turn.items():
        assert meta["NumVgprs"] <= 128, (name, meta)
