"""CPU: the population's eligibility traces (k_trace_rollout, ``QLearningPopulation(trace_decay=...)``) without a device.

* Code generation: every k_trace_rollout instantiation of qe_inst_runs_trace.hip compiles for gfx950 and, by the kernel
  metadata, uses no scratch and no static LDS (the slots are dynamic LDS, sized at launch) and is launchable.
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
from dist_classicrl_amd.algorithms.population import QLearningPopulation, trace_arrays
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]


@pytest.fixture(scope="module")
def trace_asm(tmp_path_factory):
    unit = CSRC / "qe_inst_runs_trace.hip"
    assert unit.exists(), "the trace kernels have a translation unit of their own"
    assert "trace_$(1)_$(2).o: qe_inst_runs_trace.hip" in (CSRC / "Makefile").read_text()
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_trace_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"trace_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(unit), "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_trace_kernels_are_free_of_scratch_and_static_lds(trace_asm, pair):
    kernels = _kernels(trace_asm[pair])
    ks = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe15k_trace_rollout")}
    # nothing that the sibling tests would count as one of theirs
    assert not [n for n in kernels if "k_rollout_runs" in n or "k_nstep_rollout" in n]
    # two rules x (HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1)
    assert len(ks) == 2 * {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1), sorted(ks)
    for rule in (0, 1):  # the last template argument: TD_Q_LEARNING, TD_SARSA
        assert len([n for n in ks if re.search(rf"Li{rule}EEEv", n)]) == len(ks) // 2, sorted(ks)
    for name, (_, desc, meta) in ks.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert meta["LDSByteSize"] == 0, (name, meta)  # the slots are dynamic
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        assert meta["Occupancy"] >= 1, (name, meta)


def test_trace_arguments_are_checked_before_anything_is_allocated():
    def refused(match, *args, **kw):
        pop = QLearningPopulation.__new__(QLearningPopulation)
        with pytest.raises(ValueError, match=match):
            pop.__init__(*args, **kw)
        assert not hasattr(pop, "_h")

    refused("policy-probability weighting", 4, 10, 4, update_rule="expected_sarsa", trace_decay=0.5)
    refused("double estimator has no trace form", 4, 10, 4, double_q=True, trace_decay=0.5)
    refused("one multi-step method at a time", 4, 10, 4, update_rule="sarsa", n_step=2, trace_decay=0.5)
    for bad in (-0.1, 1.0001, np.nan, np.inf, -np.inf, [0.5, 0.5, 0.5, 2.0], [0.5, 0.5, np.nan, 0.5], "x"):
        refused("trace_decay", 4, 10, 4, update_rule="sarsa", trace_decay=bad)
    refused("one entry per run", 4, 10, 4, trace_decay=[0.5, 0.5])
    for bad in (0, 33, -1, 2.0, "2", None, True):
        refused("trace_length must be an integer in 1 .. 32", 4, 10, 4, trace_decay=0.5, trace_length=bad)
    for bad in ("dutch", 0, None):
        refused("trace_kind must be one of 'replacing', 'accumulating'", 4, 10, 4, trace_decay=0.5, trace_kind=bad)
    # the decay factor T(gamma * lambda) must lie in [0, 1]
    refused("decay factor .* is outside", 4, 10, 4, discount_factor=1.25, trace_decay=0.9)
    refused("decay factor .* is outside", 4, 10, 4, discount_factor=[0.9, 0.9, -0.5, 0.9], trace_decay=0.5)
    refused("decay factor .* is outside", 4, 10, 4, discount_factor=np.nan, trace_decay=0.0)
    # without trace_decay the other two arguments are not looked at: today's constructor
    refused("n_step", 4, 10, 4, n_step=2, trace_length=99, trace_kind="dutch")


def test_trace_arrays_are_checked():
    assert trace_arrays(None, 5, 3) is None
    good = {"states": np.zeros((5, 3), dtype=np.int64), "actions": np.ones((5, 3), dtype=np.int32), "values": np.zeros((5, 3))}
    states, actions, values = trace_arrays(good, 5, 3)
    assert states.dtype == actions.dtype == np.int32 and values.dtype == np.float64
    assert all(a.flags.c_contiguous and a.shape == (5, 3) for a in (states, actions, values))
    assert trace_arrays(dict(good, values=np.ones((5, 3), dtype=np.float32)), 5, 3)[2].dtype == np.float64
    for bad in (dict(good, states=np.zeros((5, 3))), dict(good, states=np.zeros((5, 4), dtype=np.int32)),
                dict(good, actions=np.zeros((3, 5), dtype=np.int32)), dict(good, values=np.zeros((5, 3), dtype=complex)),
                dict(good, values=np.zeros(15)), dict(good, extra=1), {k: v for k, v in good.items() if k != "values"},
                (1, 2, 3), 3):
        with pytest.raises(ValueError, match="eligibility_traces"):
            trace_arrays(bad, 5, 3)


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    assert _lib.TRACE_MAX == 32 and _lib.TRACE_KINDS == {"replacing": 0, "accumulating": 1}
    out = np.zeros(4, dtype=np.int32)
    val = np.zeros(4)
    p, v = _lib.ptr(out, ctypes.c_int32), _lib.ptr(val, ctypes.c_double)
    for rc in (lib.qe_population_set_traces(None, 4, 0, v), lib.qe_population_set_traces(None, 99, 7, None),
               lib.qe_population_trace_config(None, None, None, None), lib.qe_population_traces(None, p, p, v),
               lib.qe_population_set_trace_state(None, None, None, None), lib.qe_population_set_trace_state(None, p, p, v)):
        assert rc == _lib.ERR_INVALID
        assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in ("qe_population_set_traces", "qe_population_trace_config", "qe_population_traces", "qe_population_set_trace_state"):
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
    assert "path 12" in header and "bits 24-29" in header and "bit 30" in header
    assert re.search(r"enum qe_trace_kind \{ QE_TRACE_REPLACING = 0, QE_TRACE_ACCUMULATING = 1 \}", header)


def test_variant_decoding():
    d = _lib.decode_variant(12 | (1 << 4) | (4 << 12) | (1 << 20) | (8 << 24))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["trace_length"], d["trace_kind"], d["n_step"]) == (
        "population_trace", "sarsa", 4, True, 8, "replacing", 1)
    d = _lib.decode_variant(12 | (16 << 12) | (32 << 24) | (1 << 30))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["trace_length"], d["trace_kind"]) == (
        "population_trace", "q_learning", 16, False, 32, "accumulating")
    assert _lib.decode_variant(12 | (1 << 24))["trace_length"] == 1
    # the older paths: every value they returned before, and the two new keys read 0 / None
    old = {
        0: ("none", "q_learning", 1), 1: ("stepwise", "q_learning", 1), 2 | (1 << 4): ("persistent", "q_learning", 1),
        3: ("wide", "q_learning", 1), 4: ("turnstile", "q_learning", 1), 5: ("eval", "q_learning", 1),
        6 | (2 << 12) | (1 << 20): ("population", "q_learning", 1), 7 | (1 << 12): ("population_eval", "q_learning", 1),
        8 | (1 << 4) | (4 << 12) | (1 << 20): ("population_td", "sarsa", 1), 8 | (2 << 4): ("population_td", "expected_sarsa", 1),
        9 | (8 << 12): ("population_double", "q_learning", 1), 10: ("population_double_eval", "q_learning", 1),
        11 | (2 << 4) | (16 << 12) | (16 << 24): ("population_nstep", "expected_sarsa", 16),
        11 | (1 << 4) | (3 << 24) | (1 << 20): ("population_nstep", "sarsa", 3),
    }
    for v, (path, rule, n) in old.items():
        d = _lib.decode_variant(v)
        assert (d["path"], d["rule"], d["n_step"], d["trace_length"], d["trace_kind"]) == (path, rule, n, 0, None), v
        assert (d["lean"], d["nv"], d["masked"]) == ((v >> 4) & 3, (v >> 12) & 255, bool((v >> 20) & 1)), v
        assert (d["help"], d["full"], d["light"], d["cap512"], d["dataflow"]) == tuple(bool((v >> b) & 1) for b in (6, 7, 8, 9, 10))
    assert sorted(_lib.decode_variant(6)) == sorted(["path", "rule", "lean", "help", "full", "light", "cap512", "dataflow", "nv",
                                                     "masked", "n_step", "trace_length", "trace_kind"])
