"""CPU: the population path (k_rollout_runs, QLearningPopulation) without a device.

* Code generation: every k_rollout_runs instantiation of qe_inst_runs.hip, compiled to gfx950 assembly, uses no
  scratch, no LDS, no barrier and no atomic -- runs are independent, occupancy is what hides their latency.
* Schedules: the descriptor of each schedule, advanced by the kernel's recurrence (restated in Python), gives the values
  ``advance_values(1, K)`` gives, bit for bit -- exponential schedules that reach their floor inside the call included.
* Argument validation that needs no device.
"""
import copy
import ctypes
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from dist_classicrl_amd.algorithms.population import (
    QLearningPopulation,
    advance_descriptor,
    schedule_descriptor,
)
from dist_classicrl_amd.schedules import BaseSchedule, ConstantSchedule, ExponentialSchedule, LinearSchedule

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = [(t, v) for t in ("float", "double") for v in ("HashEnv", "GridEnv", "BanditEnv", "TttEnv", "TableEnv")]


@pytest.fixture(scope="module")
def runs_asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("runs_isa")

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


def _runs_kernels(lines):
    """{symbol: (body lines, kernel-descriptor lines, metadata)} of every k_rollout_runs in an assembly listing."""
    found = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN2qe14k_rollout_runs\S*):", l)
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
def test_runs_kernel_is_free_of_inter_lane_work(runs_asm, pair):
    kernels = _runs_kernels(runs_asm[pair])
    # HashEnv / TableEnv: 5 row widths x masked or not; TicTacToe: 1; GridLake and the bandit: 1
    assert len(kernels) == {"HashEnv": 10, "TableEnv": 10}.get(pair[1], 1), sorted(kernels)
    for name, (body, desc, meta) in kernels.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        group = [int(x.split()[1]) for x in desc if x.strip().startswith(".amdhsa_group_segment_fixed_size")]
        assert group == [0], (name, group)
        code = [x.strip() for x in body if x.startswith("\t") and not x.strip().startswith((";", "."))]
        assert not [x for x in code if x.startswith("s_barrier")], name
        assert not [x for x in code if "atomic" in x.split()[0]], name
        assert not [x for x in code if x.startswith("ds_")], name


SCHEDULES = [
    ConstantSchedule(0.25),
    LinearSchedule(1.0, -0.0007),
    LinearSchedule(0.1, 1e-5),
    ExponentialSchedule(1.0, 0.01, 0.995),        # reaches the floor after ~919 steps
    ExponentialSchedule(0.3, 0.05, 0.9),          # ... after ~17
    ExponentialSchedule(0.05, 0.05, 0.9),         # starts at the floor
    ExponentialSchedule(0.1, 1e-5, 0.999),        # never reaches it within the call
    ExponentialSchedule(0.2, 0.0, 1.01),          # growing
]


@pytest.mark.parametrize("k", range(len(SCHEDULES)))
@pytest.mark.parametrize("count", [1, 64, 65, 3000])
def test_descriptor_recurrence_equals_advance_values(k, count):
    s = copy.deepcopy(SCHEDULES[k])
    kind, value, lo, factor = schedule_descriptor(s)
    got = advance_descriptor(kind, value, lo, factor, count)
    want = s.advance_values(1, count)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # ... and the value it leaves behind is the next one the schedule reads
    assert advance_descriptor(kind, value, lo, factor, count + 1)[-1] == s.get_value()


def test_other_schedules_are_rejected():
    class Stepped(BaseSchedule):
        def update(self, steps):
            self.value = self.value / 2

    class Exp2(ExponentialSchedule):
        pass

    for bad in (Stepped(1.0, 0.0), Exp2(1.0, 0.1, 0.9), 0.1):
        with pytest.raises(TypeError):
            schedule_descriptor(bad)
    with pytest.raises(TypeError):
        QLearningPopulation(4, 10, 4, exploration_rate_schedule=Stepped(1.0, 0.0))


def test_arguments_are_checked_before_the_device():
    with pytest.raises(ValueError):
        QLearningPopulation(4, 10, 4, learn_mode="batch")
    with pytest.raises(ValueError):
        QLearningPopulation(4, 10, 4, dtype=np.float16)
    with pytest.raises(ValueError):
        QLearningPopulation(0, 10, 4)
    with pytest.raises(ValueError):
        QLearningPopulation(4, 10, 4, discount_factor=[0.9, 0.9, 0.9])
    with pytest.raises(ValueError):
        QLearningPopulation(4, 10, 4, lr_schedule=[ConstantSchedule(0.1)] * 5)


def test_c_entry_points_reject_bad_shapes_without_a_device():
    from dist_classicrl_amd import _lib

    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.qe_create_population(ctypes.byref(h), 4, 10, 65, 0, 0, 0) == _lib.ERR_UNSUPPORTED  # rows wider than 64
    assert "64 actions" in lib.qe_last_error().decode()
    assert lib.qe_create_population(ctypes.byref(h), 0, 10, 4, 0, 0, 0) == _lib.ERR_INVALID
    assert lib.qe_population_runs(None) == 0
    assert lib.qe_population_rollout(None, None, 1, 0, 0, None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert ctypes.sizeof(_lib.RunSchedule) == 32
    from dist_classicrl_amd.algorithms.population import _DESCRIPTOR

    assert _DESCRIPTOR.itemsize == 32
    assert all(getattr(_lib.RunSchedule, f).offset == _DESCRIPTOR.fields[f][1] for f, _ in _lib.RunSchedule._fields_)
