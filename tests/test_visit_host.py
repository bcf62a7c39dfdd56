"""CPU: the population's visit counts (k_visit_rollout, ``QLearningPopulation(exploration_bonus=..., visit_lr=...)``)
without a device.

* Code generation: every k_visit_rollout instantiation of qe_inst_runs_visit.hip, compiled to gfx950 assembly, uses no
  scratch, no LDS, no barrier and no atomic, and the set of builds that ships is the set DESIGN section 4.3c lists.
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
from dist_classicrl_amd.algorithms.population import QLearningPopulation, visit_count_array
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]
NAME = re.compile(r"^_ZN2qe15k_visit_rolloutI([fd])NS_\d+(\w+?)ELi(\d+)ELb([01])EEEv")


def _design_builds():
    """{(dtype, NV)}: the rows of the register table of DESIGN's visit-count subsection, and the shapes it lists as refused."""
    text = (ROOT / "DESIGN.md").read_text()
    section = text[text.index("* **Visit counts: an optimism bonus and the 1/N learning rate**"):text.index("### 4.3d")]
    rows = re.findall(r"^\s*\| (float32|float64) \| (\d+) \|", section, flags=re.M)
    refused = re.search(r"^\s*Refused shapes: (.*)$", section, flags=re.M).group(1)
    return {(t, int(nv)) for t, nv in rows}, refused


@pytest.fixture(scope="module")
def visit_asm(tmp_path_factory):
    unit = CSRC / "qe_inst_runs_visit.hip"
    assert unit.exists(), "the visit-count kernels have a translation unit of their own"
    assert "visit_$(1)_$(2).o: qe_inst_runs_visit.hip" in (CSRC / "Makefile").read_text()
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_visit_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"visit_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(unit), "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_visit_kernels_are_free_of_scratch_and_inter_lane_work(visit_asm, pair):
    kernels = _kernels(visit_asm[pair])
    ks = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe15k_visit_rollout")}
    # nothing that the sibling tests would count as one of theirs
    assert not [n for n in kernels if "k_rollout_runs" in n or "k_dyna_rollout" in n or "k_trace_rollout" in n]
    listed, _ = _design_builds()
    dtype = "float32" if pair[0] == "float" else "float64"
    widths = {"HashEnv": (1, 2, 4, 8, 16), "TableEnv": (1, 2, 4, 8, 16), "TttEnv": (4,)}.get(pair[1], (1,))
    masks = {"HashEnv": (0, 1), "TableEnv": (0, 1), "TttEnv": (1,)}.get(pair[1], (0,))
    want = {(nv, mk) for nv in widths if (dtype, nv) in listed for mk in masks}
    got = set()
    for name in ks:
        m = NAME.match(name)
        assert m and m.group(1) == pair[0][0] and m.group(2) == pair[1], name
        got.add((int(m.group(3)), int(m.group(4))))
    assert got == want and len(ks) == len(want), (sorted(got), sorted(want))
    for name, (body, desc, meta) in ks.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert [x.split()[1] for x in desc if x.strip().startswith(".amdhsa_private_segment_fixed_size")] == ["0"], name
        assert meta["LDSByteSize"] == 0, (name, meta)
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        assert meta["Occupancy"] >= 1, (name, meta)
        code = [x.strip() for x in body if x.startswith("\t") and not x.strip().startswith((";", "."))]
        assert code, name
        assert not [x for x in code if x.startswith("s_barrier")], name
        assert not [x for x in code if "atomic" in x.split()[0]], name
        assert not [x for x in code if x.startswith("ds_")], name
        assert not [x for x in code if x.startswith(("scratch_", "buffer_"))], name  # no spill traffic of any kind


def test_the_shipped_set_is_the_set_design_lists():
    listed, refused = _design_builds()
    every = {(t, nv) for t in ("float32", "float64") for nv in (1, 2, 4, 8, 16)}
    assert listed <= every
    # all builds of up to 16 actions ship in both dtypes
    assert {(t, nv) for t in ("float32", "float64") for nv in (1, 2, 4)} <= listed
    assert {(np.dtype(t).name, nv) for t, nv in every - listed} == set(_lib.VISIT_REFUSED)
    assert (refused.strip() == "none.") == (listed == every)
    for t, nv in every:
        for A in {1: (1, 4), 2: (5, 8), 4: (9, 16), 8: (17, 32), 16: (33, 64)}[nv]:
            assert _lib.visit_build_shipped(np.dtype(t), A) == ((t, nv) in listed), (t, A)
    # the host-side table the setter consults (visit_supported) says the same
    host = (CSRC / "qe_host.h").read_text()
    body = re.search(r"constexpr bool visit_supported\(bool f32, int nv\) \{ return (.*?); \}", host).group(1)
    assert (body == "true") == (listed == every), body


def test_visit_arguments_are_checked_before_anything_is_allocated():
    def refused(match, *args, **kw):
        pop = QLearningPopulation.__new__(QLearningPopulation)
        with pytest.raises(ValueError, match=match):
            pop.__init__(*args, **kw)
        assert not hasattr(pop, "_h")

    for kw in ({"exploration_bonus": 0.5}, {"visit_lr": True}, {"exploration_bonus": 0.0}):
        for rule in ("sarsa", "expected_sarsa"):
            refused("needs update_rule='q_learning'", 4, 10, 4, update_rule=rule, **kw)
        refused("with double_q=True", 4, 10, 4, double_q=True, **kw)
        # (n_step > 1 needs an on-policy rule and counting needs Q-learning: whichever check comes first refuses)
        refused("n_step|needs update_rule='q_learning'", 4, 10, 4, update_rule="sarsa", n_step=2, **kw)
        refused("n_step", 4, 10, 4, n_step=2, **kw)
        refused("with trace_decay", 4, 10, 4, trace_decay=0.5, **kw)
        refused("with planning_steps=3", 4, 10, 4, planning_steps=3, **kw)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), [0.1, 0.2, -1e-300, 0.0], [0.0, 0.0, 0.0, np.nan]):
        refused("every beta must be a finite number >= 0", 4, 10, 4, exploration_bonus=bad)
    refused("one entry per run", 4, 10, 4, exploration_bonus=[0.1, 0.2])
    refused("exploration_bonus must be None, a finite number", 4, 10, 4, exploration_bonus="much")
    for bad in (1, 0, "yes", None, 1.0):
        refused("visit_lr must be a bool", 4, 10, 4, visit_lr=bad)
    # the defaults are today's constructor: its other refusals come as before
    refused("n_step", 4, 10, 4, n_step=2, exploration_bonus=None, visit_lr=False)


def test_visit_count_arrays_are_checked():
    R, S, A = 3, 5, 2
    assert visit_count_array(None, R, S, A) is None
    got = visit_count_array(np.arange(R * S * A, dtype=np.int64).reshape(R, S, A), R, S, A)
    assert got.dtype == np.uint32 and got.flags.c_contiguous and got.shape == (R, S, A) and got[2, 4, 1] == R * S * A - 1
    top = visit_count_array(np.full((R, S, A), 2 ** 32 - 1, dtype=np.uint64), R, S, A)
    assert top.dtype == np.uint32 and (top == 2 ** 32 - 1).all()
    assert visit_count_array(np.zeros((R, S, A), dtype=np.uint8)[:, :, ::1], R, S, A).dtype == np.uint32
    for bad in (np.zeros((R, S, A)), np.zeros((R, S, A), dtype=np.float32), np.zeros((R, S * A), dtype=np.uint32),
                np.zeros((R, S, A + 1), dtype=np.uint32), np.zeros((S, A), dtype=np.uint32), np.zeros((R, S, A), dtype=bool),
                np.full((R, S, A), -1), np.full((R, S, A), 2 ** 32), 3, "counts", {}):
        with pytest.raises(ValueError, match="visit_counts"):
            visit_count_array(bad, R, S, A)


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    u32 = np.zeros(4, dtype=np.uint32)
    i32 = np.zeros(4, dtype=np.int32)
    f64 = np.zeros(4, dtype=np.float64)
    u, i, f = _lib.ptr(u32, ctypes.c_uint32), _lib.ptr(i32, ctypes.c_int32), _lib.ptr(f64, ctypes.c_double)
    for rc in (lib.qe_population_set_visits(None, f, 1), lib.qe_population_set_visits(None, None, 0),
               lib.qe_population_visits(None, i, i, f), lib.qe_population_visit_counts(None, u),
               lib.qe_population_set_visit_counts(None, None), lib.qe_population_set_visit_counts(None, u),
               lib.qe_population_visit_bonus(None, f64.ctypes.data, _lib.QE_F64)):
        assert rc == _lib.ERR_INVALID
        assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in ("qe_population_set_visits", "qe_population_visits", "qe_population_visit_counts",
                 "qe_population_set_visit_counts", "qe_population_visit_bonus"):
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
    assert "path 14" in header


def test_variant_decoding():
    d = _lib.decode_variant(14 | (1 << 4) | (1 << 5) | (4 << 12) | (1 << 20))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["visit_lr"], d["bonus"]) == ("population_visit", "q_learning", 4, True, True, True)
    assert (d["n_step"], d["trace_length"], d["trace_kind"]) == (1, 0, None)
    d = _lib.decode_variant(14 | (16 << 12))
    assert (d["path"], d["nv"], d["masked"], d["visit_lr"], d["bonus"]) == ("population_visit", 16, False, False, False)
    assert _lib.decode_variant(14 | (1 << 5))["bonus"] and not _lib.decode_variant(14 | (1 << 5))["visit_lr"]
    # the older paths: no new key
    keys = sorted(["path", "rule", "lean", "help", "full", "light", "cap512", "dataflow", "nv", "masked", "n_step", "trace_length",
                   "trace_kind"])
    for v in (0, 1, 2 | (1 << 4), 3, 4, 5, 6 | (2 << 12) | (1 << 20), 7, 8 | (1 << 4), 9, 10, 11 | (2 << 4) | (16 << 24), 12 | (8 << 24)):
        assert sorted(_lib.decode_variant(v)) == keys, v
    assert sorted(_lib.decode_variant(13)) == sorted([*keys, "planning_steps"])
    assert sorted(_lib.decode_variant(14)) == sorted([*keys, "visit_lr", "bonus"])
