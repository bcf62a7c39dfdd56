"""CPU: the population's Dyna-Q (k_dyna_rollout, ``QLearningPopulation(planning_steps=n)``) without a device.

* Code generation: every k_dyna_rollout instantiation of qe_inst_runs_dyna.hip compiles for gfx950 and, by the kernel
  metadata, uses no scratch and no LDS and is launchable.
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
from dist_classicrl_amd.algorithms.population import QLearningPopulation, model_arrays
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]


@pytest.fixture(scope="module")
def dyna_asm(tmp_path_factory):
    unit = CSRC / "qe_inst_runs_dyna.hip"
    assert unit.exists(), "the Dyna-Q kernels have a translation unit of their own"
    assert "dyna_$(1)_$(2).o: qe_inst_runs_dyna.hip" in (CSRC / "Makefile").read_text()
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_dyna_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"dyna_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(unit), "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_dyna_kernels_are_free_of_scratch_and_lds(dyna_asm, pair):
    kernels = _kernels(dyna_asm[pair])
    ks = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe14k_dyna_rollout")}
    # nothing that the sibling tests would count as one of theirs
    assert not [n for n in kernels if "k_rollout_runs" in n or "k_nstep_rollout" in n or "k_trace_rollout" in n]
    # HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1
    assert len(ks) == {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1), sorted(ks)
    for name, (_, desc, meta) in ks.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert meta["LDSByteSize"] == 0, (name, meta)
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        assert meta["Occupancy"] >= 1, (name, meta)


def test_planning_arguments_are_checked_before_anything_is_allocated():
    def refused(match, *args, **kw):
        pop = QLearningPopulation.__new__(QLearningPopulation)
        with pytest.raises(ValueError, match=match):
            pop.__init__(*args, **kw)
        assert not hasattr(pop, "_h")

    for bad in (-1, 65, 1000, True, False, 2.0, 0.0, "2", None, np.bool_(True), np.float32(1)):
        refused("planning_steps must be an integer in 0 .. 64", 4, 10, 4, planning_steps=bad)
    for rule in ("sarsa", "expected_sarsa"):
        refused("needs update_rule='q_learning'", 4, 10, 4, update_rule=rule, planning_steps=1)
    refused("double_q=True: Dyna-Q plans on one table", 4, 10, 4, double_q=True, planning_steps=3)
    # (n_step > 1 needs an on-policy rule and planning needs Q-learning: whichever check comes first refuses)
    refused("n_step|planning_steps", 4, 10, 4, update_rule="sarsa", n_step=2, planning_steps=3)
    refused("n_step|planning_steps", 4, 10, 4, n_step=2, planning_steps=3)
    refused("with trace_decay: Dyna-Q is a one-step method", 4, 10, 4, trace_decay=0.5, planning_steps=64)
    refused("state_size \\* action_size must be below 2\\^31", 4, 2 ** 26, 32, planning_steps=1)
    # planning_steps=0 is today's constructor: its other refusals come as before
    refused("n_step", 4, 10, 4, n_step=2, planning_steps=0)
    assert _lib.PLANNING_MAX == 64


def test_model_arrays_are_checked():
    R, S, A = 3, 5, 2
    assert model_arrays(None, R, S, A) is None
    good = {"next_states": np.full((R, S, A), -1, dtype=np.int64), "rewards": np.zeros((R, S, A), dtype=np.float32),
            "terminated": np.zeros((R, S, A), dtype=bool), "visited": np.full((R, S * A), -1, dtype=np.int32),
            "count": np.zeros(R, dtype=np.int64)}
    nxt, rew, term, visited, count = model_arrays(good, R, S, A)
    assert nxt.dtype == visited.dtype == count.dtype == np.int32 and rew.dtype == np.float32 and term.dtype == np.uint8
    assert all(a.flags.c_contiguous for a in (nxt, rew, term, visited, count))
    assert (nxt.shape, rew.shape, term.shape, visited.shape, count.shape) == ((R, S, A),) * 3 + ((R, S * A), (R,))
    assert model_arrays(dict(good, rewards=np.full((R, S, A), 0.5)), R, S, A)[1].dtype == np.float32  # exact in float32
    for bad in (dict(good, next_states=np.zeros((R, S, A))), dict(good, next_states=np.zeros((R, S * A), dtype=np.int32)),
                dict(good, next_states=np.full((R, S, A), 2 ** 31)),
                dict(good, rewards=np.zeros((R, S, A), dtype=np.int32)), dict(good, rewards=np.full((R, S, A), 0.1)),
                dict(good, rewards=np.zeros((R, S))), dict(good, terminated=np.zeros((R, S, A), dtype=np.int32)),
                dict(good, terminated=np.zeros((R, S, A + 1), dtype=bool)), dict(good, visited=np.zeros((R, S, A), dtype=np.int32)),
                dict(good, visited=np.zeros((R, S * A))), dict(good, count=np.zeros(R + 1, dtype=np.int32)),
                dict(good, count=np.zeros(R)), dict(good, extra=1), {k: v for k, v in good.items() if k != "count"},
                (1, 2, 3), 3):
        with pytest.raises(ValueError, match="planning_model"):
            model_arrays(bad, R, S, A)


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    i32 = np.zeros(4, dtype=np.int32)
    f32 = np.zeros(4, dtype=np.float32)
    u8 = np.zeros(4, dtype=np.uint8)
    p, f, b = _lib.ptr(i32, ctypes.c_int32), _lib.ptr(f32, ctypes.c_float), _lib.ptr(u8, ctypes.c_uint8)
    for rc in (lib.qe_population_set_planning(None, 4), lib.qe_population_set_planning(None, 99), lib.qe_population_planning(None),
               lib.qe_population_model(None, p, f, b, p, p), lib.qe_population_model(None, None, None, None, None, None),
               lib.qe_population_set_model(None, None, None, None, None, None), lib.qe_population_set_model(None, p, f, b, p, p)):
        assert rc == _lib.ERR_INVALID
        assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in ("qe_population_set_planning", "qe_population_planning", "qe_population_model", "qe_population_set_model"):
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
    assert "path 13" in header and "bits 24-30" in header
    device = (CSRC / "qe_device.h").read_text()
    assert re.search(r"constexpr uint32_t STREAM_POLICY = 0;\nconstexpr uint32_t STREAM_ENV = 1;\nconstexpr uint32_t STREAM_PLAN = 2;", device)


def test_variant_decoding():
    d = _lib.decode_variant(13 | (4 << 12) | (1 << 20) | (16 << 24))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["planning_steps"]) == ("population_dyna", "q_learning", 4, True, 16)
    assert (d["n_step"], d["trace_length"], d["trace_kind"]) == (1, 0, None)
    d = _lib.decode_variant(13 | (16 << 12) | (64 << 24))
    assert (d["path"], d["nv"], d["masked"], d["planning_steps"]) == ("population_dyna", 16, False, 64)
    assert _lib.decode_variant(13 | (1 << 24))["planning_steps"] == 1
    # the older paths: every value they returned before, and no new key
    old = {
        0: ("none", "q_learning", 1, 0, None), 1: ("stepwise", "q_learning", 1, 0, None),
        2 | (1 << 4): ("persistent", "q_learning", 1, 0, None), 3: ("wide", "q_learning", 1, 0, None),
        4: ("turnstile", "q_learning", 1, 0, None), 5: ("eval", "q_learning", 1, 0, None),
        6 | (2 << 12) | (1 << 20): ("population", "q_learning", 1, 0, None), 7 | (1 << 12): ("population_eval", "q_learning", 1, 0, None),
        8 | (1 << 4) | (4 << 12) | (1 << 20): ("population_td", "sarsa", 1, 0, None),
        8 | (2 << 4): ("population_td", "expected_sarsa", 1, 0, None),
        9 | (8 << 12): ("population_double", "q_learning", 1, 0, None), 10: ("population_double_eval", "q_learning", 1, 0, None),
        11 | (2 << 4) | (16 << 12) | (16 << 24): ("population_nstep", "expected_sarsa", 16, 0, None),
        12 | (1 << 4) | (4 << 12) | (8 << 24): ("population_trace", "sarsa", 1, 8, "replacing"),
        12 | (32 << 24) | (1 << 30): ("population_trace", "q_learning", 1, 32, "accumulating"),
    }
    keys = sorted(["path", "rule", "lean", "help", "full", "light", "cap512", "dataflow", "nv", "masked", "n_step", "trace_length",
                   "trace_kind"])
    for v, want in old.items():
        d = _lib.decode_variant(v)
        assert (d["path"], d["rule"], d["n_step"], d["trace_length"], d["trace_kind"]) == want, v
        assert (d["lean"], d["nv"], d["masked"]) == ((v >> 4) & 3, (v >> 12) & 255, bool((v >> 20) & 1)), v
        assert sorted(d) == keys, v
    assert sorted(_lib.decode_variant(13)) == sorted([*keys, "planning_steps"])
