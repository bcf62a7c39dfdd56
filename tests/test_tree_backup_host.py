"""CPU: the population's n-step Tree Backup (k_tree_rollout, ``QLearningPopulation(tree_backup=...)``) without a device.

* Code generation: every k_tree_rollout instantiation of qe_inst_runs_tree.hip, compiled to gfx950 assembly, uses no
  scratch, no static LDS (the window is dynamic LDS, sized at launch), no barrier and no atomic.  No build is refused:
  the widest one (fp64, 64 masked actions) fits the register file as well.
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
from dist_classicrl_amd.algorithms import population
from dist_classicrl_amd.algorithms.population import QLearningPopulation, tree_window_arrays
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]


@pytest.fixture(scope="module")
def tree_asm(tmp_path_factory):
    unit = CSRC / "qe_inst_runs_tree.hip"
    assert unit.exists(), "the Tree Backup kernels have a translation unit of their own"
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_tree_isa")

    def one(pair):
        t, v = pair
        out = out_dir / f"tree_{t}_{v}.s"
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
               f"-DQE_INST_T={t}", f"-DQE_INST_ENV={v}", "-S", "--cuda-device-only", str(unit), "-o", str(out)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        return pair, out.read_text().split("\n")

    with ThreadPoolExecutor(4) as pool:
        return dict(pool.map(one, PAIRS))


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{t}-{v}" for t, v in PAIRS])
def test_tree_kernels_are_free_of_scratch_static_lds_and_inter_lane_work(tree_asm, pair):
    kernels = _kernels(tree_asm[pair])
    tree = {n: k for n, k in kernels.items() if n.startswith("_ZN2qe14k_tree_rollout")}
    # nothing that the sibling tests would count as a kernel of theirs
    assert not [n for n in kernels if "k_rollout_runs" in n or "k_nstep_rollout" in n]
    # HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe, GridLake, the bandit: 1
    assert len(tree) == {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1), sorted(tree)
    for name, (body, desc, meta) in tree.items():
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


def test_tree_backup_is_checked_before_anything_is_allocated():
    for bad in (0, 17, -1, 2.0, "2", None, True, np.True_):
        with pytest.raises(ValueError, match="tree_backup must be an integer in 1 .. 16"):
            QLearningPopulation(4, 10, 4, tree_backup=bad)
    pop = QLearningPopulation.__new__(QLearningPopulation)
    for kw, text in (({"update_rule": "sarsa"}, "needs update_rule='q_learning'"),
                     ({"update_rule": "expected_sarsa"}, "needs update_rule='q_learning'"),
                     ({"double_q": True}, "double estimator is a one-step method"),
                     ({"update_rule": "sarsa", "n_step": 2}, "needs update_rule='q_learning'"),
                     ({"trace_decay": 0.5}, "one multi-step method at a time"),
                     ({"planning_steps": 2}, "Dyna-Q is a one-step method"),
                     ({"exploration_bonus": 0.5}, "visit counts are built for the one-step rule"),
                     ({"visit_lr": True}, "visit counts are built for the one-step rule")):
        with pytest.raises(ValueError, match=f"tree_backup=3 .*{text}"):
            pop.__init__(4, 10, 4, tree_backup=np.int64(3), **kw)
        assert not hasattr(pop, "_h")
    # n_step > 1 with Q-learning keeps its own refusal, and points at the switch
    with pytest.raises(ValueError, match="n_step=2 .* not an off-policy method .*tree_backup"):
        pop.__init__(4, 10, 4, n_step=2, tree_backup=2)
    assert not hasattr(pop, "_h")
    assert "tree_backup_window" in population._CARRIED and _lib.TREE_BACKUP_MAX == 16


def test_tree_window_arrays_are_checked():
    assert tree_window_arrays(None, 5, 3) is None
    good = {"length": [0, 1, 2, 0, 1], "states": np.zeros((5, 2), dtype=np.int64), "actions": np.ones((5, 2), dtype=np.int32),
            "rewards": np.zeros((5, 2)), "greedy": np.array([[0, 1]] * 5, dtype=bool)}
    length, states, actions, rewards, greedy = tree_window_arrays(good, 5, 3)
    assert length.dtype == states.dtype == actions.dtype == np.int32 and rewards.dtype == np.float32 and greedy.dtype == np.uint8
    assert all(a.flags.c_contiguous for a in (length, states, actions, rewards, greedy)) and greedy.tolist() == [[0, 1]] * 5
    assert tree_window_arrays(dict(good, greedy=np.ones((5, 2), dtype=np.int64)), 5, 3)[4].tolist() == [[1, 1]] * 5
    for bad in (dict(good, length=np.zeros(5)), dict(good, states=np.zeros((5, 3), dtype=np.int32)),
                dict(good, actions=np.zeros((5, 2))), dict(good, rewards=np.zeros((2, 5))), dict(good, extra=1),
                dict(good, greedy=np.zeros((5, 2))), dict(good, greedy=np.zeros((5, 3), dtype=bool)),
                dict(good, greedy=np.full((5, 2), 2)), dict(good, greedy=np.full((5, 2), 256)), dict(good, greedy=np.full((5, 2), -1)),
                {k: v for k, v in good.items() if k != "greedy"}, (1, 2, 3, 4, 5), 3):
        with pytest.raises(ValueError, match="tree_backup_window"):
            tree_window_arrays(bad, 5, 3)
    assert "tree_window_arrays" in population.__all__


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    out = np.zeros(4, dtype=np.int32)
    p = _lib.ptr(out, ctypes.c_int32)
    for rc in (lib.qe_population_set_tree_backup(None, 2), lib.qe_population_set_tree_backup(None, 99),
               lib.qe_population_tree_backup(None), lib.qe_population_tree_window(None, p, None, None, None, None),
               lib.qe_population_set_tree_window(None, None, None, None, None, None)):
        assert rc == _lib.ERR_INVALID
        assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    assert list(_lib.UPDATE_RULES) == ["q_learning", "sarsa", "expected_sarsa"]
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    for name in ("qe_population_set_tree_backup", "qe_population_tree_backup", "qe_population_tree_window",
                 "qe_population_set_tree_window"):
        assert re.search(rf"\bint {name}\(qe_engine\* e", header), name
        assert name in _lib.PROTOTYPES
    assert "path 15" in header and "QE_ABI_VERSION 2" in header


def test_variant_decoding():
    d = _lib.decode_variant(15 | (4 << 12) | (1 << 20) | (3 << 24))
    assert (d["path"], d["rule"], d["nv"], d["masked"], d["tree_backup"], d["n_step"]) == ("population_tree", "q_learning", 4, True, 3, 1)
    assert d["trace_length"] == 0 and d["trace_kind"] is None and "planning_steps" not in d and "visit_lr" not in d
    d = _lib.decode_variant(15 | (16 << 12) | (16 << 24))
    assert (d["path"], d["nv"], d["masked"], d["tree_backup"]) == ("population_tree", 16, False, 16)
    # every other path: unchanged, and without the key
    old = {6 | (2 << 12) | (1 << 20): ("population", "q_learning", 1), 7 | (1 << 12): ("population_eval", "q_learning", 1),
           8 | (1 << 4) | (4 << 12) | (1 << 20): ("population_td", "sarsa", 1), 9: ("population_double", "q_learning", 1),
           10: ("population_double_eval", "q_learning", 1),
           11 | (2 << 4) | (16 << 12) | (16 << 24): ("population_nstep", "expected_sarsa", 16),
           12 | (1 << 4) | (5 << 24) | (1 << 30): ("population_trace", "sarsa", 1), 13 | (7 << 24): ("population_dyna", "q_learning", 1),
           14 | (3 << 4): ("population_visit", "q_learning", 1), 2 | (1 << 4): ("persistent", "q_learning", 1), 0: ("none", "q_learning", 1)}
    for v, (path, rule, n_step) in old.items():
        d = _lib.decode_variant(v)
        assert (d["path"], d["rule"], d["n_step"]) == (path, rule, n_step) and "tree_backup" not in d, (v, d)
    assert _lib.decode_variant(13 | (7 << 24))["planning_steps"] == 7 and _lib.decode_variant(12 | (5 << 24))["trace_length"] == 5
