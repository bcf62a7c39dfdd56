"""CPU: the population's greedy evaluation (k_evaluate_runs, qe_population_evaluate) without a device.

* Code generation: every k_evaluate_runs instantiation of qe_inst_runs.hip, compiled to gfx950 assembly, uses no
  scratch, no LDS, no barrier and no atomic, like k_rollout_runs.
* kernel_variant path 7 decodes as the population evaluation.
* Argument validation that needs no device (C entry points and the Python front end).
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
from dist_classicrl_amd.algorithms import PopulationEval, PopulationTraining, QLearningPopulation

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]


@pytest.fixture(scope="module")
def runs_asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("eval_runs_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"runs_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(CSRC / "qe_inst_runs.hip"),
               "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


def _eval_kernels(lines):
    """{symbol: (body lines, kernel-descriptor lines, metadata)} of every k_evaluate_runs in an assembly listing."""
    found = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN2qe15k_evaluate_runs\S*):", l)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        meta_end = next(j for j in range(end, len(lines)) if "; Occupancy" in lines[j])
        meta = {}
        for x in lines[end:meta_end + 1]:
            mm = re.search(r"; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", x)
            if mm:
                meta[mm.group(1)] = int(mm.group(2))
        d0 = next(j for j in range(len(lines)) if lines[j].strip() == f".amdhsa_kernel {name}")
        d1 = next(j for j in range(d0, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        found[name] = (lines[i:end], lines[d0:d1], meta)
    return found


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_evaluation_kernel_is_free_of_inter_lane_work(runs_asm, pair):
    kernels = _eval_kernels(runs_asm[pair])
    # HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake and the bandit: 1
    assert len(kernels) == {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1), sorted(kernels)
    for name, (body, desc, meta) in kernels.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        code = [x.strip() for x in body if x.startswith("\t") and not x.strip().startswith((";", "."))]
        assert not [x for x in code if x.startswith("s_barrier")], name
        assert not [x for x in code if "atomic" in x.split()[0]], name
        assert not [x for x in code if x.startswith("ds_")], name
        # no table store: the only global stores are the per-run state, counts, log segment and flags
        assert not [x for x in code if x.startswith("scratch_")], name


@pytest.mark.parametrize("nv", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("masked", [False, True])
def test_decode_variant_of_the_evaluation_path(nv, masked):
    d = _lib.decode_variant(7 | (nv << 12) | (int(masked) << 20))
    assert d["path"] == "population_eval" and d["nv"] == nv and d["masked"] == masked
    assert _lib.decode_variant(6 | (nv << 12))["path"] == "population"


def test_c_entry_points_reject_a_missing_engine():
    lib = _lib.load()
    assert lib.qe_population_evaluate(None, None, 1, 0, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert "NULL" in lib.qe_last_error().decode()
    out = np.zeros(4, dtype=np.uint64)
    assert lib.qe_population_step_counters(None, _lib.ptr(out, ctypes.c_uint64)) == _lib.ERR_INVALID
    assert lib.qe_population_set_step_counters(None, _lib.ptr(out, ctypes.c_uint64)) == _lib.ERR_INVALID


def _deviceless(runs=4):
    """A population object whose engine was never created: the checks below must fail before they need it."""
    pop = object.__new__(QLearningPopulation)
    pop.runs = runs
    return pop


def test_python_arguments_are_checked_before_the_device():
    from dist_classicrl_amd.environments import HashTabularEnv

    pop = _deviceless(4)
    with pytest.raises(TypeError):
        pop.evaluate_steps(object(), 10)
    with pytest.raises(TypeError):
        pop.evaluate_episodes([1, 2, 3, 4], 2)
    with pytest.raises(ValueError):
        pop.evaluate_steps(HashTabularEnv(5, 10, 4), 10)  # one agent per run
    with pytest.raises(ValueError):
        pop.evaluate_steps(HashTabularEnv(4, 10, 4), -1)
    with pytest.raises(ValueError):
        pop.evaluate_episodes(HashTabularEnv(4, 10, 4), -1)
    with pytest.raises(ValueError):
        pop.evaluate_episodes(HashTabularEnv(4, 10, 4), 2, max_steps=-5)
    env = HashTabularEnv(4, 10, 4)
    with pytest.raises(ValueError, match="Exactly one"):
        pop.train(env, 10, env, 5)
    with pytest.raises(ValueError, match="Exactly one"):
        pop.train(env, 10, env, 5, val_steps=2, val_episodes=2)
    with pytest.raises(TypeError):
        pop.train(env, 10, object(), 5, val_steps=2)
    with pytest.raises(ValueError):
        pop.train(HashTabularEnv(3, 10, 4), 10, env, 5, val_episodes=2)


def test_result_types():
    M = 3
    ev = PopulationEval(np.zeros(M, np.float32), np.array([1, 0, 2]), np.array([1.0, 2.0, 3.0], np.float32),
                        np.array([0, 1, 1, 3]), np.full(M, 5), np.ones(M, bool))
    assert np.array_equal(ev.run_returns(2), [2.0, 3.0]) and ev.run_returns(1).size == 0
    tr = PopulationTraining(np.array([4.0, 5.0], np.float32), np.array([0, 0, 2, 2]), np.zeros((2, M), np.float32),
                            np.ones((2, M), bool), [], {})
    assert np.array_equal(tr.run_reward_history(1), [4.0, 5.0])
