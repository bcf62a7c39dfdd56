"""CPU: the population's prioritized sweeping (k_sweep_rollout, ``QLearningPopulation(planning_order="prioritized")``)
without a device.

* Code generation: every k_sweep_rollout instantiation of qe_inst_runs_sweep.hip compiles for gfx950 and, by the kernel
  metadata, uses no scratch and no static LDS (the queue is dynamic LDS, sized at launch) and is launchable.  At most the
  NV = 8 / 16 builds may be absent (``_lib.SWEEP_REFUSED``); NV <= 4 are all there.
* The Dyna-Q unit is untouched: the assembly of its float / HashEnv build is the one recorded before this kernel existed.
* Argument and ABI checks that need no device.
"""
import ctypes
import hashlib
import json
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from dist_classicrl_amd import _lib
from dist_classicrl_amd.algorithms.population import QLearningPopulation, model_arrays, queue_arrays, sweep_model_arrays
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed"]


def _assembly(unit, t, v, out):
    cmd = [HIPCC, *FLAGS, f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(unit), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return out.read_text()


@pytest.fixture(scope="module")
def sweep_asm(tmp_path_factory):
    unit = CSRC / "qe_inst_runs_sweep.hip"
    assert unit.exists(), "the sweeping kernels have a translation unit of their own"
    makefile = (CSRC / "Makefile").read_text()
    assert "sweep_$(1)_$(2).o: qe_inst_runs_sweep.hip" in makefile and "qe_rollout_sweep.h" in makefile
    assert "qe_rollout_sweep.h" not in (CSRC / "qe_inst_runs_dyna.hip").read_text()
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_sweep_isa")
    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(lambda pair: (pair, _assembly(unit, *pair, out_dir / f"sweep_{pair[0]}_{pair[1]}.s").split("\n")), PAIRS))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_sweep_kernels_are_free_of_scratch_and_static_lds(sweep_asm, pair):
    kernels = _kernels(sweep_asm[pair])
    ks = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe15k_sweep_rollout")}
    # nothing that the sibling tests would count as one of theirs
    assert not [n for n in kernels if "k_rollout_runs" in n or "k_dyna_rollout" in n or "k_trace_rollout" in n]
    dtype = "float32" if pair[0] == "float" else "float64"
    refused = {nv for name, nv in _lib.SWEEP_REFUSED if name == dtype}
    assert refused <= {8, 16}, "only the two widest builds may be left out"
    # HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1 (NV <= 4: never refused)
    built = {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1)
    assert len(ks) == built - (2 * len(refused) if built == 10 else 0), sorted(ks)
    for nv in (1, 2, 4):
        if built == 10:
            assert len([n for n in ks if re.search(rf"ELi{nv}ELb[01]EEEv", n)]) == 2, (nv, sorted(ks))
    for name, (_, desc, meta) in ks.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert meta["LDSByteSize"] == 0, (name, meta)  # the queue is dynamic
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        assert meta["Occupancy"] >= 1, (name, meta)


def test_the_dyna_unit_compiles_to_the_assembly_it_had_before(tmp_path):
    """tests/golden/dyna_float_HashEnv_asm.json holds the SHA-256 of that unit's device assembly as it was before
    k_sweep_rollout was added, with every ``__hip_cuid_<id>`` (the compilation-unit id, a hash of the source path) cut to
    ``__hip_cuid_``, and the compiler that produced it.  Another compiler's output says nothing about the source."""
    want = json.loads((ROOT / "tests" / "golden" / "dyna_float_HashEnv_asm.json").read_text())
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    version = subprocess.run([HIPCC, "--version"], check=True, capture_output=True, text=True).stdout.splitlines()[:2]
    if version != want["compiler"]:
        pytest.skip(f"the digest was recorded with {want['compiler']}, this is {version}")
    text = _assembly(CSRC / "qe_inst_runs_dyna.hip", "float", "HashEnv", tmp_path / "dyna.s")
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)
    assert text.count("\n") == want["lines"]
    assert hashlib.sha256(text.encode()).hexdigest() == want["sha256"]


def test_sweeping_arguments_are_checked_before_anything_is_allocated():
    def refused(match, *args, **kw):
        pop = QLearningPopulation.__new__(QLearningPopulation)
        with pytest.raises(ValueError, match=match):
            pop.__init__(*args, **kw)
        assert not hasattr(pop, "_h")

    for bad in ("sweeping", "Prioritized", None, 1, True):
        refused("planning_order must be one of 'uniform', 'prioritized'", 4, 10, 4, planning_steps=2, planning_order=bad)
    refused("needs planning_steps >= 1", 4, 10, 4, planning_order="prioritized")
    refused("needs planning_steps >= 1", 4, 10, 4, planning_steps=0, planning_order="prioritized")
    for bad in (0, 33, -1, True, 2.0, "4", None):
        refused("queue_length must be an integer in 1 .. 32", 4, 10, 4, planning_steps=2, planning_order="prioritized", queue_length=bad)
    for bad in (-1e-9, np.inf, np.nan, [0.0, 0.0, -1.0, 0.0], True):
        refused("sweep_threshold: every threshold must be a finite number >= 0", 4, 10, 4, planning_steps=2,
                planning_order="prioritized", sweep_threshold=bad)
    refused("sweep_threshold must be a finite number >= 0 or a sequence of 4", 4, 10, 4, planning_steps=2, planning_order="prioritized",
            sweep_threshold="x")
    refused("sweep_threshold: expected one entry per run", 4, 10, 4, planning_steps=2, planning_order="prioritized",
            sweep_threshold=[0.0, 0.1])
    # every combination Dyna-Q refuses is refused here too, in Dyna-Q's words
    for rule in ("sarsa", "expected_sarsa"):
        refused("needs update_rule='q_learning'", 4, 10, 4, update_rule=rule, planning_steps=1, planning_order="prioritized")
    refused("double_q=True: Dyna-Q plans on one table", 4, 10, 4, double_q=True, planning_steps=3, planning_order="prioritized")
    refused("n_step|planning_steps", 4, 10, 4, n_step=2, planning_steps=3, planning_order="prioritized")
    refused("with trace_decay: Dyna-Q is a one-step method", 4, 10, 4, trace_decay=0.5, planning_steps=64, planning_order="prioritized")
    refused("state_size \\* action_size must be below 2\\^31", 4, 2 ** 26, 32, planning_steps=1, planning_order="prioritized")
    refused("tree_backup=2 with planning_steps=3", 4, 10, 4, tree_backup=2, planning_steps=3, planning_order="prioritized")
    refused("visit counts are built for the step without planning", 4, 10, 4, planning_steps=3, planning_order="prioritized",
            exploration_bonus=0.5)
    # under the uniform order the two arguments of the other order are not read
    refused("n_step", 4, 10, 4, n_step=2, planning_order="uniform", queue_length=99, sweep_threshold=-1)
    assert _lib.QUEUE_MAX == 32 and _lib.PLANNING_ORDERS == ("uniform", "prioritized")
    for dtype, nv in _lib.SWEEP_REFUSED:
        refused("prioritized sweeping: the kernel for .* is not built", 4, 10, 4 * nv, dtype=np.dtype(dtype), planning_steps=1,
                planning_order="prioritized")
    assert all(_lib.sweep_build_shipped(dt, A) for dt in (np.float32, np.float64) for A in (1, 2, 4, 5, 8, 9, 16))


def _good(R, S, A):
    return {"next_states": np.full((R, S, A), -1, dtype=np.int64), "rewards": np.zeros((R, S, A), dtype=np.float32),
            "terminated": np.zeros((R, S, A), dtype=bool), "visited": np.full((R, S * A), -1, dtype=np.int32),
            "count": np.zeros(R, dtype=np.int64), "pred_head": np.full((R, S), -1, dtype=np.int64),
            "pred_next": np.full((R, S, A), -1, dtype=np.int32)}


def test_seven_key_model_arrays_are_checked():
    R, S, A = 3, 5, 2
    assert sweep_model_arrays(None, R, S, A) is None
    good = _good(R, S, A)
    arrays = sweep_model_arrays(good, R, S, A)
    assert len(arrays) == 7 and all(a.flags.c_contiguous for a in arrays)
    assert arrays[5].dtype == arrays[6].dtype == np.int32 and (arrays[5].shape, arrays[6].shape) == ((R, S), (R, S, A))
    five = {k: v for k, v in good.items() if not k.startswith("pred_")}
    assert len(sweep_model_arrays(five, R, S, A)) == 5  # a Dyna-Q model: the library rebuilds the lists
    for a, b in zip(sweep_model_arrays(five, R, S, A), model_arrays(five, R, S, A)):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    for bad in (dict(good, pred_head=np.zeros((R, S))), dict(good, pred_head=np.zeros((R, S + 1), dtype=np.int32)),
                dict(good, pred_head=np.full((R, S), 2 ** 31)), dict(good, pred_next=np.zeros((R, S * A), dtype=np.int32)),
                dict(good, pred_next=np.zeros((R, S, A), dtype=bool)), dict(good, extra=1),
                {k: v for k, v in good.items() if k != "pred_next"}, {k: v for k, v in good.items() if k != "count"},
                dict(five, pred_head=good["pred_head"]), dict(five, rewards=np.full((R, S, A), 0.1)), (1, 2, 3), 3):
        with pytest.raises(ValueError, match="planning_model"):
            sweep_model_arrays(bad, R, S, A)
    with pytest.raises(ValueError, match="planning_model"):  # the 5-key checker keeps its five keys
        model_arrays(good, R, S, A)


def test_queue_arrays_are_checked():
    R, K = 3, 4
    assert queue_arrays(None, R, K) is None
    good = {"cells": np.full((R, K), -1, dtype=np.int64), "priorities": np.zeros((R, K), dtype=np.float32)}
    cells, priorities = queue_arrays(good, R, K)
    assert cells.dtype == np.int32 and priorities.dtype == np.float64 and cells.shape == priorities.shape == (R, K)
    for bad in (dict(good, cells=np.zeros((R, K))), dict(good, cells=np.zeros((R, K + 1), dtype=np.int32)),
                dict(good, cells=np.full((R, K), 2 ** 31)), dict(good, priorities=np.zeros((R,))),
                dict(good, priorities=np.zeros((R, K), dtype=bool)), dict(good, extra=1), {"cells": good["cells"]}, [1, 2], 3):
        with pytest.raises(ValueError, match="sweep_queue"):
            queue_arrays(bad, R, K)


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    i32 = np.zeros(4, dtype=np.int32)
    f64 = np.zeros(4, dtype=np.float64)
    p, d = _lib.ptr(i32, ctypes.c_int32), _lib.ptr(f64, ctypes.c_double)
    for rc in (lib.qe_population_set_sweeping(None, 4, d), lib.qe_population_set_sweeping(None, 0, None),
               lib.qe_population_set_sweeping(None, 99, d), lib.qe_population_sweeping(None),
               lib.qe_population_predecessors(None, p, p), lib.qe_population_predecessors(None, None, None),
               lib.qe_population_set_predecessors(None, p, p), lib.qe_population_set_predecessors(None, None, None),
               lib.qe_population_queue(None, p, d), lib.qe_population_queue(None, None, None),
               lib.qe_population_set_queue(None, p, d), lib.qe_population_set_queue(None, None, None)):
        assert rc == _lib.ERR_INVALID
        assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in ("qe_population_set_sweeping", "qe_population_sweeping", "qe_population_predecessors",
                 "qe_population_set_predecessors", "qe_population_queue", "qe_population_set_queue"):
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
        assert name in _lib.PROTOTYPES
        assert re.search(rf"^ \*   .*\b{name}\b", header, re.M), f"{name} is not documented in the header comment"
    assert "bits 5-9" in header
    host = (CSRC / "qe_host.h").read_text()
    assert "constexpr bool sweep_supported(bool f32, int nv)" in host


def test_variant_decoding():
    keys = sorted(["path", "rule", "lean", "help", "full", "light", "cap512", "dataflow", "nv", "masked", "n_step", "trace_length",
                   "trace_kind", "planning_steps"])
    plain = 13 | (4 << 12) | (1 << 20) | (16 << 24)
    d = _lib.decode_variant(plain)
    assert sorted(d) == keys and "prioritized" not in d and "queue_length" not in d
    for K in (1, 4, 16, 32):
        s = _lib.decode_variant(plain | (1 << 4) | ((K - 1) << 5))
        assert sorted(s) == sorted([*keys, "prioritized", "queue_length"])
        assert s["prioritized"] is True and s["queue_length"] == K
        assert {k: s[k] for k in ("path", "rule", "nv", "masked", "planning_steps", "n_step", "trace_length", "trace_kind")} == \
               {k: d[k] for k in ("path", "rule", "nv", "masked", "planning_steps", "n_step", "trace_length", "trace_kind")}
    # bit 4 means something else on every other path: no new key there
    for v in (2 | (1 << 4), 8 | (1 << 4), 11 | (1 << 4), 12 | (1 << 4), 14 | (1 << 4), 6, 15 | (3 << 24)):
        assert "prioritized" not in _lib.decode_variant(v) and "queue_length" not in _lib.decode_variant(v), v
