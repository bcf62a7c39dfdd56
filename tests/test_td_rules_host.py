"""CPU: the population's on-policy update rules (k_rollout_runs_td, ``QLearningPopulation(update_rule=...)``) without a
device.

* Code generation: every k_rollout_runs_td instantiation of qe_inst_runs_td.hip, compiled to gfx950 assembly, uses no
  scratch, no LDS, no barrier and no atomic -- like its sibling k_rollout_runs, occupancy is all that hides latency.
  No build is refused: the widest one (fp64, 64 masked actions, Expected SARSA) fits the register file as well.
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
from dist_classicrl_amd.algorithms.population import QLearningPopulation, pending_array

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]
REFUSED = []  # (dtype, NV, masked, rule) builds answered with QE_ERR_UNSUPPORTED instead of compiled: none


@pytest.fixture(scope="module")
def td_asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_td_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"runs_td_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(CSRC / "qe_inst_runs_td.hip"),
               "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


def _kernels(lines):
    """{symbol: (body lines, kernel-descriptor lines, metadata)} of every kernel in an assembly listing."""
    names = [m.group(1) for l in lines if (m := re.match(r"^\s*\.amdhsa_kernel (\S+)", l))]
    found = {}
    for name in names:
        i = next(j for j, l in enumerate(lines) if l.startswith(f"{name}:"))
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        meta_end = next(j for j in range(end, len(lines)) if "; Occupancy" in lines[j])
        meta = {}
        for x in lines[end:meta_end + 1]:
            mm = re.search(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", x)
            if mm:
                meta[mm.group(1)] = int(mm.group(2))
        d0 = next(j for j in range(len(lines)) if lines[j].strip() == f".amdhsa_kernel {name}")
        d1 = next(j for j in range(d0, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        found[name] = (lines[i:end], lines[d0:d1], meta)
    return found


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_td_kernels_are_free_of_scratch_and_inter_lane_work(td_asm, pair):
    kernels = _kernels(td_asm[pair])
    td = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe17k_rollout_runs_td")}
    # nothing that test_population_host.py would count as a k_rollout_runs
    assert not [n for n in kernels if n.startswith("_ZN2qe14k_rollout_runs")]
    # two rules x (HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1)
    assert len(td) == 2 * {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1) - len(REFUSED), sorted(td)
    for rule in (1, 2):  # the last template argument: TD_SARSA, TD_EXPECTED_SARSA
        assert len([n for n in td if re.search(rf"Li{rule}EEEv", n)]) == len(td) // 2, sorted(td)
    for name, (body, desc, meta) in td.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert [x.split()[1] for x in desc if x.strip().startswith(".amdhsa_private_segment_fixed_size")] == ["0"], name
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        assert meta["Occupancy"] >= 1, (name, meta)
        code = [x.strip() for x in body if x.startswith("\t") and not x.strip().startswith((";", "."))]
        assert code, name
        assert not [x for x in code if x.startswith("s_barrier")], name
        assert not [x for x in code if "atomic" in x.split()[0]], name
        assert not [x for x in code if x.startswith("ds_")], name
        assert not [x for x in code if x.startswith(("scratch_", "buffer_"))], name  # no spill traffic of any kind


def test_update_rule_is_checked_before_anything_is_allocated():
    for bad in ("Sarsa", "double_q", "", None, 1):
        with pytest.raises(ValueError, match="update_rule"):
            QLearningPopulation(4, 10, 4, update_rule=bad)
    # ... also ahead of the other arguments' device-free checks having passed: no handle exists afterwards
    pop = QLearningPopulation.__new__(QLearningPopulation)
    with pytest.raises(ValueError, match="update_rule"):
        pop.__init__(4, 10, 4, update_rule="td0")
    assert not hasattr(pop, "_h")


def test_pending_arrays_are_checked():
    assert pending_array(None, 5) is None
    got = pending_array([0, -1, 3, 2, 1], 5)
    assert got.dtype == np.int32 and got.flags.c_contiguous and got.tolist() == [0, -1, 3, 2, 1]
    assert pending_array(np.arange(4, dtype=np.int64), 4).dtype == np.int32
    for bad in (np.zeros(4), np.zeros((5, 1), dtype=np.int32), np.zeros(6, dtype=np.int32), 3):
        with pytest.raises(ValueError, match="pending_actions"):
            pending_array(bad, 5)


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    assert (_lib.RULE_Q_LEARNING, _lib.RULE_SARSA, _lib.RULE_EXPECTED_SARSA) == (0, 1, 2)
    assert _lib.UPDATE_RULES == {"q_learning": 0, "sarsa": 1, "expected_sarsa": 2}
    out = np.zeros(4, dtype=np.int32)
    for rc in (lib.qe_population_set_update_rule(None, _lib.RULE_SARSA), lib.qe_population_set_update_rule(None, 7),
               lib.qe_population_update_rule(None), lib.qe_population_pending_actions(None, _lib.ptr(out, ctypes.c_int32)),
               lib.qe_population_set_pending_actions(None, None)):
        assert rc == _lib.ERR_INVALID
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    assert re.search(r"enum qe_update_rule \{ QE_RULE_Q_LEARNING = 0, QE_RULE_SARSA = 1, QE_RULE_EXPECTED_SARSA = 2 \};", header)


def test_variant_decoding():
    d = _lib.decode_variant(8 | (1 << 4) | (4 << 12) | (1 << 20))
    assert (d["path"], d["rule"], d["nv"], d["masked"]) == ("population_td", "sarsa", 4, True)
    d = _lib.decode_variant(8 | (2 << 4) | (16 << 12))
    assert (d["path"], d["rule"], d["nv"], d["masked"]) == ("population_td", "expected_sarsa", 16, False)
    d = _lib.decode_variant(6 | (2 << 12) | (1 << 20))  # the Q-learning population: unchanged
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["lean"]) == ("population", "q_learning", 2, True, 0)
    assert _lib.decode_variant(2 | (1 << 4))["lean"] == 1  # the persistent path keeps bits 4-5 for LEAN
