"""CPU: the population's n-step rules (k_nstep_rollout, ``QLearningPopulation(n_step=...)``) without a device.

* Code generation: every k_nstep_rollout instantiation of qe_inst_runs_nstep.hip, compiled to gfx950 assembly, uses no
  scratch, no static LDS (the window is dynamic LDS, sized at launch), no barrier and no atomic.  No build is refused:
  the widest one (fp64, 64 masked actions, Expected SARSA) fits the register file as well.
* Argument and ABI checks that need no device.
"""
import ctypes
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from dist_classicrl_amd import _lib
from dist_classicrl_amd.algorithms.population import QLearningPopulation, window_arrays
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]


@pytest.fixture(scope="module")
def nstep_asm(tmp_path_factory):
    unit = CSRC / "qe_inst_runs_nstep.hip"
    assert unit.exists(), "the n-step kernels have a translation unit of their own"
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_nstep_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"nstep_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(unit), "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_nstep_kernels_are_free_of_scratch_static_lds_and_inter_lane_work(nstep_asm, pair):
    kernels = _kernels(nstep_asm[pair])
    ns = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe15k_nstep_rollout")}
    # nothing that the sibling tests would count as a k_rollout_runs / k_rollout_runs_td
    assert not [n for n in kernels if "k_rollout_runs" in n]
    # two rules x (HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1)
    assert len(ns) == 2 * {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1), sorted(ns)
    for rule in (1, 2):  # the last template argument: TD_SARSA, TD_EXPECTED_SARSA
        assert len([n for n in ns if re.search(rf"Li{rule}EEEv", n)]) == len(ns) // 2, sorted(ns)
    for name, (body, desc, meta) in ns.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert [x.split()[1] for x in desc if x.strip().startswith(".amdhsa_private_segment_fixed_size")] == ["0"], name
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)  # the window is dynamic
        assert meta["LDSByteSize"] == 0, (name, meta)
        assert meta["Occupancy"] >= 1, (name, meta)
        code = [x.strip() for x in body if x.startswith("\t") and not x.strip().startswith((";", "."))]
        assert code, name
        assert not [x for x in code if x.startswith("s_barrier")], name
        assert not [x for x in code if "atomic" in x.split()[0]], name
        assert not [x for x in code if x.startswith(("scratch_", "buffer_"))], name  # no spill traffic of any kind
        assert [x for x in code if x.startswith("ds_")], name  # ... and the window is where it is said to be


def test_n_step_is_checked_before_anything_is_allocated():
    for bad in (0, 17, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="n_step must be an integer in 1 .. 16"):
            QLearningPopulation(4, 10, 4, update_rule="sarsa", n_step=bad)
    for kw in ({}, {"update_rule": "q_learning"}):
        with pytest.raises(ValueError, match="n_step=2 .* not an off-policy method"):
            QLearningPopulation(4, 10, 4, n_step=2, **kw)
    with pytest.raises(ValueError, match="update_rule"):  # double_q is refused with the on-policy rules as before
        QLearningPopulation(4, 10, 4, update_rule="sarsa", double_q=True, n_step=2)
    pop = QLearningPopulation.__new__(QLearningPopulation)
    with pytest.raises(ValueError, match="n_step"):
        pop.__init__(4, 10, 4, update_rule="expected_sarsa", n_step=40)
    assert not hasattr(pop, "_h")
    with pytest.raises(ValueError, match="double estimator is a one-step method"):
        pop.__init__(4, 10, 4, double_q=True, n_step=np.int64(3))
    assert not hasattr(pop, "_h")


def test_window_arrays_are_checked():
    assert window_arrays(None, 5, 3) is None
    good = {"length": [0, 1, 2, 0, 1], "states": np.zeros((5, 2), dtype=np.int64), "actions": np.ones((5, 2), dtype=np.int32),
            "rewards": np.zeros((5, 2))}
    length, states, actions, rewards = window_arrays(good, 5, 3)
    assert length.dtype == states.dtype == actions.dtype == np.int32 and rewards.dtype == np.float32
    assert all(a.flags.c_contiguous for a in (length, states, actions, rewards)) and length.tolist() == [0, 1, 2, 0, 1]
    for bad in (dict(good, length=np.zeros(5)), dict(good, states=np.zeros((5, 3), dtype=np.int32)),
                dict(good, actions=np.zeros((5, 2))), dict(good, rewards=np.zeros((2, 5))), dict(good, extra=1),
                {k: v for k, v in good.items() if k != "rewards"}, (1, 2, 3, 4), 3):
        with pytest.raises(ValueError, match="n_step_window"):
            window_arrays(bad, 5, 3)


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    assert _lib.N_STEP_MAX == 16
    out = np.zeros(4, dtype=np.int32)
    p = _lib.ptr(out, ctypes.c_int32)
    for rc in (lib.qe_population_set_n_step(None, 2), lib.qe_population_set_n_step(None, 99), lib.qe_population_n_step(None),
               lib.qe_population_window(None, p, None, None, None), lib.qe_population_set_window(None, None, None, None, None)):
        assert rc == _lib.ERR_INVALID
        assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in ("qe_population_set_n_step", "qe_population_n_step", "qe_population_window", "qe_population_set_window"):
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
    assert "bits 24-28" in header


def test_variant_decoding():
    d = _lib.decode_variant(11 | (1 << 4) | (4 << 12) | (1 << 20) | (3 << 24))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["n_step"]) == ("population_nstep", "sarsa", 4, True, 3)
    d = _lib.decode_variant(11 | (2 << 4) | (16 << 12) | (16 << 24))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["n_step"]) == ("population_nstep", "expected_sarsa", 16, False, 16)
    # the one-step paths: unchanged, and n_step reads 1
    d = _lib.decode_variant(8 | (1 << 4) | (4 << 12) | (1 << 20))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["n_step"]) == ("population_td", "sarsa", 4, True, 1)
    d = _lib.decode_variant(6 | (2 << 12) | (1 << 20))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["lean"], d["n_step"]) == ("population", "q_learning", 2, True, 0, 1)
    assert _lib.decode_variant(2 | (1 << 4))["lean"] == 1 and _lib.decode_variant(9)["n_step"] == 1
