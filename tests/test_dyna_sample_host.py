"""CPU: the population's Dyna-Q over a sample model (k_dyna_sample_rollout, ``QLearningPopulation(planning_steps=n,
model_outcomes=K)``) without a device.

* Code generation: every k_dyna_sample_rollout instantiation of qe_inst_runs_dyna_sample.hip compiles for gfx950 and, by
  the kernel metadata, uses no scratch and no LDS and is launchable.
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
from dist_classicrl_amd.algorithms.population import QLearningPopulation, outcome_model_arrays
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed"]


@pytest.fixture(scope="module")
def sample_asm(tmp_path_factory):
    unit = CSRC / "qe_inst_runs_dyna_sample.hip"
    assert unit.exists(), "the sample-model kernels have a translation unit of their own"
    makefile = (CSRC / "Makefile").read_text()
    assert "dyna_sample_$(1)_$(2).o: qe_inst_runs_dyna_sample.hip" in makefile and "qe_rollout_dyna_sample.h" in makefile
    assert "$(OBJ)/dyna_sample_$(t)_$(v).o" in makefile
    assert "dyna_sample" not in (CSRC / "qe_inst_runs_dyna.hip").read_text()
    assert "dyna_sample" not in (CSRC / "qe_rollout_dyna.h").read_text()
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_dyna_sample_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"dyna_sample_{t}_{v}.s"
        cmd = [HIPCC, *FLAGS, f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(unit), "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_sample_model_kernels_are_free_of_scratch_and_lds(sample_asm, pair):
    kernels = _kernels(sample_asm[pair])
    ks = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe21k_dyna_sample_rollout")}
    # nothing that the sibling tests would count as one of theirs
    assert not [n for n in kernels if "k_rollout_runs" in n or "k_dyna_rollout" in n or "k_sweep_rollout" in n or "k_trace_rollout" in n]
    dtype = "float32" if pair[0] == "float" else "float64"
    refused = {nv for name, nv in _lib.DYNA_SAMPLE_REFUSED if name == dtype}
    assert refused <= {8, 16}, "only the two widest builds may be left out"
    # HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1 (NV <= 4: never refused)
    built = {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1)
    assert len(ks) == built - (2 * len(refused) if built == 10 else 0), sorted(ks)
    for nv in (1, 2, 4):
        if built == 10:
            assert len([n for n in ks if re.search(rf"ELi{nv}ELb[01]EEEv", n)]) == 2, (nv, sorted(ks))
    for name, (_, desc, meta) in ks.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert meta["LDSByteSize"] == 0, (name, meta)
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        assert meta["Occupancy"] >= 1, (name, meta)


def test_the_refused_builds_are_the_same_in_the_library_and_in_python():
    host = (CSRC / "qe_host.h").read_text()
    body = re.search(r"constexpr bool dyna_sample_supported\(bool f32, int nv\) \{ return (.*?); \}", host)
    assert body, "dyna_sample_supported is one expression"
    if not _lib.DYNA_SAMPLE_REFUSED:
        assert body.group(1) == "true"
    else:
        for dtype, nv in _lib.DYNA_SAMPLE_REFUSED:
            assert dtype in ("float32", "float64") and str(nv) in body.group(1), (dtype, nv)
    for dt in (np.float32, np.float64):
        for A in (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64):
            nv = max(4, 1 << (A - 1).bit_length()) // 4
            assert _lib.dyna_sample_build_shipped(dt, A) == ((np.dtype(dt).name, nv) not in _lib.DYNA_SAMPLE_REFUSED)
    assert all(_lib.dyna_sample_build_shipped(dt, A) for dt in (np.float32, np.float64) for A in (1, 2, 4, 5, 8, 9, 16))


def test_model_outcomes_is_checked_before_anything_is_allocated():
    def refused(match, *args, **kw):
        pop = QLearningPopulation.__new__(QLearningPopulation)
        with pytest.raises(ValueError, match=match):
            pop.__init__(*args, **kw)
        assert not hasattr(pop, "_h")

    for bad in (0, 9, -1, 1000, True, False, 2.0, 1.0, "2", None, np.bool_(True), np.float32(2)):
        refused("model_outcomes must be an integer in 1 .. 8", 4, 10, 4, planning_steps=2, model_outcomes=bad)
    refused("model_outcomes=2 sizes the planning model: it needs planning_steps >= 1", 4, 10, 4, model_outcomes=2)
    refused("model_outcomes=8 sizes the planning model: it needs planning_steps >= 1", 4, 10, 4, planning_steps=0, model_outcomes=8)
    refused("model_outcomes=3 with planning_order='prioritized': sweeping over a sample model needs expected updates, which are not built",
            4, 10, 4, planning_steps=2, planning_order="prioritized", model_outcomes=3)
    # everything Dyna-Q refuses stays refused, in Dyna-Q's words
    for rule in ("sarsa", "expected_sarsa"):
        refused("needs update_rule='q_learning'", 4, 10, 4, update_rule=rule, planning_steps=1, model_outcomes=2)
    refused("double_q=True: Dyna-Q plans on one table", 4, 10, 4, double_q=True, planning_steps=3, model_outcomes=2)
    refused("n_step|planning_steps", 4, 10, 4, n_step=2, planning_steps=3, model_outcomes=2)
    refused("with trace_decay: Dyna-Q is a one-step method", 4, 10, 4, trace_decay=0.5, planning_steps=64, model_outcomes=2)
    refused("state_size \\* action_size must be below 2\\^31", 4, 2 ** 26, 32, planning_steps=1, model_outcomes=2)
    refused("tree_backup=2 with planning_steps=3", 4, 10, 4, tree_backup=2, planning_steps=3, model_outcomes=2)
    refused("visit counts are built for the step without planning", 4, 10, 4, planning_steps=3, model_outcomes=2, exploration_bonus=0.5)
    # model_outcomes=1 is today's constructor: its refusals come as before
    refused("n_step", 4, 10, 4, n_step=2, planning_steps=0, model_outcomes=1)
    refused("needs planning_steps >= 1", 4, 10, 4, planning_order="prioritized", model_outcomes=1)
    for dtype, nv in _lib.DYNA_SAMPLE_REFUSED:
        refused("model_outcomes=2: the kernel for .* is not built", 4, 10, 4 * nv, dtype=np.dtype(dtype), planning_steps=1, model_outcomes=2)
    assert _lib.MODEL_OUTCOMES_MAX == 8


def _good(R, S, A, K):
    slots = (R, S, A, K)
    return {"next_states": np.full(slots, -1, dtype=np.int64), "rewards": np.zeros(slots, dtype=np.float32),
            "terminated": np.zeros(slots, dtype=bool), "outcome_counts": np.zeros(slots, dtype=np.uint32),
            "visited": np.full((R, S * A), -1, dtype=np.int32), "count": np.zeros(R, dtype=np.int64)}


def test_outcome_model_arrays_are_checked():
    R, S, A, K = 3, 5, 2, 4
    slots = (R, S, A, K)
    assert outcome_model_arrays(None, R, S, A, K) is None
    good = _good(R, S, A, K)
    nxt, rew, term, cnt, visited, count = outcome_model_arrays(good, R, S, A, K)
    assert nxt.dtype == visited.dtype == count.dtype == np.int32 and rew.dtype == np.float32 and term.dtype == np.uint8
    assert cnt.dtype == np.uint32
    assert all(a.flags.c_contiguous for a in (nxt, rew, term, cnt, visited, count))
    assert (nxt.shape, rew.shape, term.shape, cnt.shape, visited.shape, count.shape) == (slots,) * 4 + ((R, S * A), (R,))
    # the counts fill uint32: signed 64-bit input is taken when every value fits
    top = outcome_model_arrays(dict(good, outcome_counts=np.full(slots, 2 ** 32 - 1, dtype=np.int64)), R, S, A, K)[3]
    assert top.dtype == np.uint32 and (top == 2 ** 32 - 1).all()
    assert outcome_model_arrays(dict(good, rewards=np.full(slots, 0.5)), R, S, A, K)[1].dtype == np.float32  # exact in float32
    # the 5-key dict of a last-outcome population: the five arrays of model_arrays
    five = {"next_states": np.full((R, S, A), -1, dtype=np.int32), "rewards": np.zeros((R, S, A), dtype=np.float32),
            "terminated": np.zeros((R, S, A), dtype=bool), "visited": good["visited"], "count": good["count"]}
    got = outcome_model_arrays(five, R, S, A, K)
    assert len(got) == 5 and got[0].shape == (R, S, A)
    for bad in (dict(good, next_states=np.zeros(slots)), dict(good, next_states=np.zeros((R, S, A), dtype=np.int32)),
                dict(good, next_states=np.full(slots, 2 ** 31)),
                dict(good, rewards=np.zeros(slots, dtype=np.int32)), dict(good, rewards=np.full(slots, 0.1)),
                dict(good, rewards=np.zeros((R, S, A))), dict(good, terminated=np.zeros(slots, dtype=np.int32)),
                dict(good, terminated=np.zeros((R, S, A, K + 1), dtype=bool)),
                dict(good, outcome_counts=np.zeros(slots)), dict(good, outcome_counts=np.zeros((R, S, A), dtype=np.uint32)),
                dict(good, outcome_counts=np.zeros((R, S, A, K - 1), dtype=np.uint32)),
                dict(good, outcome_counts=np.full(slots, -1)), dict(good, outcome_counts=np.full(slots, 2 ** 32)),
                dict(good, outcome_counts=np.zeros(slots, dtype=bool)),
                dict(good, visited=np.zeros((R, S, A), dtype=np.int32)),
                dict(good, visited=np.zeros((R, S * A))), dict(good, count=np.zeros(R + 1, dtype=np.int32)),
                dict(good, count=np.zeros(R)), dict(good, extra=1), {k: v for k, v in good.items() if k != "count"},
                {k: v for k, v in good.items() if k != "outcome_counts"}, dict(five, extra=1),
                dict(five, next_states=np.zeros(slots, dtype=np.int32)), (1, 2, 3), 3):
        with pytest.raises(ValueError, match="planning_model"):
            outcome_model_arrays(bad, R, S, A, K)


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    i32 = np.zeros(4, dtype=np.int32)
    f32 = np.zeros(4, dtype=np.float32)
    u8 = np.zeros(4, dtype=np.uint8)
    u32 = np.zeros(4, dtype=np.uint32)
    p, f, b, u = (_lib.ptr(i32, ctypes.c_int32), _lib.ptr(f32, ctypes.c_float), _lib.ptr(u8, ctypes.c_uint8),
                  _lib.ptr(u32, ctypes.c_uint32))
    for rc in (lib.qe_population_set_model_outcomes(None, 2), lib.qe_population_set_model_outcomes(None, 99),
               lib.qe_population_model_outcomes(None),
               lib.qe_population_outcome_model(None, p, f, b, u, p, p), lib.qe_population_outcome_model(None, None, None, None, None, None, None),
               lib.qe_population_set_outcome_model(None, None, None, None, None, None, None),
               lib.qe_population_set_outcome_model(None, p, f, b, u, p, p)):
        assert rc == _lib.ERR_INVALID
        assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in ("qe_population_set_model_outcomes", "qe_population_model_outcomes", "qe_population_outcome_model",
                 "qe_population_set_outcome_model"):
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
    assert re.search(r"int qe_population_set_outcome_model\(qe_engine\* e, const int32_t\* next_states, const float\* rewards, "
                     r"const uint8_t\* terminated,\s+const uint32_t\* counts, const int32_t\* visited, const int32_t\* count\);", header)
    assert "bits 21-23" in header
    device = (CSRC / "qe_device.h").read_text()
    assert re.search(r"constexpr uint32_t STREAM_PLAN = 2;[^\n]*\nconstexpr uint32_t STREAM_OUTCOME = 3;", device)
    from dyna_sample_model import OUTCOMES_MAX, STREAM_OUTCOME

    assert STREAM_OUTCOME == 3 and OUTCOMES_MAX == _lib.MODEL_OUTCOMES_MAX
    sample = (CSRC / "qe_rollout_dyna_sample.h").read_text()
    assert "constexpr int DYNA_OUTCOMES_MAX = 8;" in sample and "k_dyna_sample_rollout" in sample


def test_variant_decoding():
    d = _lib.decode_variant(13 | (4 << 12) | (1 << 20) | (3 << 21) | (16 << 24))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["planning_steps"], d["model_outcomes"]) == ("population_dyna", "q_learning", 4, True, 16, 4)
    assert "prioritized" not in d and (d["n_step"], d["trace_length"], d["trace_kind"]) == (1, 0, None)
    for K in range(2, 9):
        d = _lib.decode_variant(13 | (16 << 12) | ((K - 1) << 21) | (64 << 24))
        assert (d["nv"], d["masked"], d["planning_steps"], d["model_outcomes"]) == (16, False, 64, K)
    # the older paths: every value they returned before, and no new key
    keys = sorted(["path", "rule", "lean", "help", "full", "light", "cap512", "dataflow", "nv", "masked", "n_step", "trace_length",
                   "trace_kind"])
    old = {
        0: ("none", "q_learning", 1, 0, None), 1: ("stepwise", "q_learning", 1, 0, None),
        2 | (1 << 4): ("persistent", "q_learning", 1, 0, None), 3: ("wide", "q_learning", 1, 0, None),
        4: ("turnstile", "q_learning", 1, 0, None), 5: ("eval", "q_learning", 1, 0, None),
        6 | (2 << 12) | (1 << 20): ("population", "q_learning", 1, 0, None), 7 | (1 << 12): ("population_eval", "q_learning", 1, 0, None),
        8 | (1 << 4) | (4 << 12) | (1 << 20): ("population_td", "sarsa", 1, 0, None),
        9 | (8 << 12): ("population_double", "q_learning", 1, 0, None), 10: ("population_double_eval", "q_learning", 1, 0, None),
        11 | (2 << 4) | (16 << 12) | (16 << 24): ("population_nstep", "expected_sarsa", 16, 0, None),
        12 | (1 << 4) | (4 << 12) | (8 << 24): ("population_trace", "sarsa", 1, 8, "replacing"),
    }
    for v, want in old.items():
        d = _lib.decode_variant(v)
        assert (d["path"], d["rule"], d["n_step"], d["trace_length"], d["trace_kind"]) == want, v
        assert sorted(d) == keys, v
    assert sorted(_lib.decode_variant(13 | (4 << 24))) == sorted([*keys, "planning_steps"])
    assert sorted(_lib.decode_variant(13 | (1 << 4) | (7 << 5) | (4 << 24))) == sorted([*keys, "planning_steps", "prioritized", "queue_length"])
    assert sorted(_lib.decode_variant(14 | (1 << 4))) == sorted([*keys, "visit_lr", "bonus"])
    assert sorted(_lib.decode_variant(15 | (4 << 24))) == sorted([*keys, "tree_backup"])
    assert sorted(_lib.decode_variant(13 | (1 << 21) | (4 << 24))) == sorted([*keys, "planning_steps", "model_outcomes"])
