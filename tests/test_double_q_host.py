"""CPU: the population's double estimator (k_double_rollout / k_double_evaluate, ``QLearningPopulation(double_q=True)``)
without a device.

* Code generation: every kernel of qe_inst_runs_double.hip, compiled to gfx950 assembly for all ten (dtype, environment)
  pairs, uses no scratch, no LDS, no barrier and no atomic -- like its siblings, occupancy is all that hides latency.
  No build is refused: the widest one (fp64, 64 masked actions) fits the register file (its overflow goes to accumulator
  registers, not to memory).
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
from dist_classicrl_amd.algorithms.population import QLearningPopulation

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]
REFUSED = []  # (dtype, NV, masked, kernel) builds answered with QE_ERR_UNSUPPORTED instead of compiled: none
NEW_FUNCTIONS = ["qe_population_set_double", "qe_population_double", "qe_population_table_b_upload",
                 "qe_population_table_b_download", "qe_population_table_b_download_rows"]


@pytest.fixture(scope="module")
def double_asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_double_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"runs_double_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(CSRC / "qe_inst_runs_double.hip"),
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
def test_double_kernels_are_free_of_scratch_and_inter_lane_work(double_asm, pair):
    kernels = _kernels(double_asm[pair])
    rollout = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe16k_double_rollout")}
    evaluate = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe17k_double_evaluate")}
    # nothing that the sibling units' tests would count as one of theirs
    assert not [n for n in kernels if re.match(r"_ZN2qe\d+k_(rollout|evaluate)_runs", n)], sorted(kernels)
    # HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1
    builds = {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1)
    assert len(rollout) + len(evaluate) == 2 * builds - len(REFUSED), sorted(kernels)
    assert len(rollout) == builds - len([x for x in REFUSED if x[3] == "k_double_rollout"]), sorted(rollout)
    # (the unit's headers bring a few small file-local helper kernels along, as in the sibling units: every kernel of
    # the listing is held to the no-scratch rule, the population's own to all of them)
    for name, (_, desc, meta) in kernels.items():
        assert meta["ScratchSize"] == 0, (name, meta)
    for name, (body, desc, meta) in {**rollout, **evaluate}.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert [x.split()[1] for x in desc if x.strip().startswith(".amdhsa_private_segment_fixed_size")] == ["0"], name
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        assert meta["LDSByteSize"] == 0, (name, meta)
        assert meta["Occupancy"] >= 1, (name, meta)
        code = [x.strip() for x in body if x.startswith("\t") and not x.strip().startswith((";", "."))]
        assert code, name
        assert not [x for x in code if x.startswith("s_barrier")], name
        assert not [x for x in code if "atomic" in x.split()[0]], name
        assert not [x for x in code if x.startswith("ds_")], name
        assert not [x for x in code if x.startswith(("scratch_", "buffer_"))], name  # no spill traffic of any kind


def test_double_q_with_another_rule_is_refused_before_anything_is_allocated():
    for rule in ("sarsa", "expected_sarsa"):
        pop = QLearningPopulation.__new__(QLearningPopulation)
        with pytest.raises(ValueError, match="double_q"):
            pop.__init__(4, 10, 4, update_rule=rule, double_q=True)
        assert not hasattr(pop, "_h")


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    for name in NEW_FUNCTIONS:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    buf = np.zeros(8, dtype=np.float64)
    for rc in (lib.qe_population_set_double(None, 1), lib.qe_population_set_double(None, 0), lib.qe_population_double(None),
               lib.qe_population_table_b_upload(None, buf.ctypes.data, _lib.QE_F64),
               lib.qe_population_table_b_download(None, buf.ctypes.data, _lib.QE_F64),
               lib.qe_population_table_b_download_rows(None, buf.ctypes.data, 0, 1)):
        assert rc == _lib.ERR_INVALID
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    assert _lib.UPDATE_RULES == {"q_learning": 0, "sarsa": 1, "expected_sarsa": 2}  # the switch is no fourth rule
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in NEW_FUNCTIONS:
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
    assert "#define QE_ABI_VERSION 2" in header


def test_variant_decoding():
    d = _lib.decode_variant(9 | (4 << 12) | (1 << 20))
    assert (d["path"], d["rule"], d["nv"], d["masked"]) == ("population_double", "q_learning", 4, True)
    d = _lib.decode_variant(10 | (16 << 12))
    assert (d["path"], d["rule"], d["nv"], d["masked"]) == ("population_double_eval", "q_learning", 16, False)
    d = _lib.decode_variant(6 | (2 << 12) | (1 << 20))  # the single-table population: unchanged
    assert (d["path"], d["nv"], d["masked"]) == ("population", 2, True)
    assert _lib.decode_variant(7 | (1 << 12))["path"] == "population_eval"
