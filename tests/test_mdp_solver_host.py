"""CPU: the dynamic-programming entry points (``TabularMDPEnv.solve``, ``QLearningPopulation.policy_values``,
``qe_env_table_solve``, ``qe_population_policy_values``) without a device.

* Python argument checks raise before any library call.
* The C entry points answer NULL handles; the header declares both; the ABI version and struct sizes stand.
* Code generation: every kernel of qe_mdp_solve.hip, compiled to gfx950 assembly, uses no scratch (resource usage only).
"""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from dist_classicrl_amd import _lib
from dist_classicrl_amd.algorithms.population import PolicyValues, QLearningPopulation
from dist_classicrl_amd.environments.device_envs import MDPSolution, TabularMDPEnv
from test_td_rules_host import _kernels

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "dist_classicrl_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _env(num_agents=3):
    nxt = np.array([[1, 0], [1, 1]])
    return TabularMDPEnv.from_arrays(num_agents, nxt, np.ones((2, 2)), np.array([[False, False], [True, True]]))


def test_solve_checks_its_arguments_before_the_library():
    env = _env()
    env._lib = _NoLibrary()
    for gamma in (-0.1, 1.5, float("nan"), float("inf"), None, "x", [0.5, 0.5]):
        with pytest.raises(ValueError, match="discount"):
            env.solve(gamma)
    for tol in (-1e-9, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError, match="tol must be a finite number >= 0"):
            env.solve(0.9, tol=tol)
    for sweeps in (0, -3, 2 ** 31, 1.5, True, None):
        with pytest.raises(ValueError, match="max_sweeps must be an integer in 1 .. 2\\^31 - 1"):
            env.solve(0.9, max_sweeps=sweeps)
    with pytest.raises(RuntimeError, match="not bound"):  # good arguments: the existing error of an unbound environment
        env.solve(0.9)
    assert MDPSolution._fields == ("q", "v", "start_value", "sweeps", "residual", "converged")


def test_policy_values_checks_its_arguments_before_the_library():
    pop = QLearningPopulation.__new__(QLearningPopulation)
    pop.runs, pop.state_size, pop.action_size = 3, 2, 2
    pop._lib = _NoLibrary()
    env = _env(3)
    for gamma in (-0.1, 1.5, float("nan"), [0.5, 0.5, 2.0], "x"):
        with pytest.raises(ValueError, match="discount"):
            pop.policy_values(env, gamma)
    with pytest.raises(ValueError, match="one entry per run"):
        pop.policy_values(env, [0.5, 0.5])
    with pytest.raises(ValueError, match="tol must be a finite number >= 0"):
        pop.policy_values(env, 0.5, tol=-1.0)
    with pytest.raises(ValueError, match="max_sweeps"):
        pop.policy_values(env, 0.5, max_sweeps=0)
    with pytest.raises(ValueError, match="4 agents, the population 3 runs"):  # as _check_env words it
        pop.policy_values(_env(4))
    with pytest.raises(TypeError, match="device environment"):
        pop.policy_values(object())
    assert PolicyValues._fields == ("values", "start_values", "sweeps", "residuals", "converged", "status")


def test_c_entry_points_without_a_device():
    lib = _lib.load()
    out = np.zeros(4, dtype=np.float64)
    p = _lib.ptr(out, ctypes.c_double)
    sweeps = ctypes.c_int32()
    res = ctypes.c_double()
    assert lib.qe_env_table_solve(None, 0.9, 1e-12, 10, p, p, ctypes.byref(sweeps), ctypes.byref(res)) == _lib.ERR_INVALID
    assert "env is NULL" in lib.qe_last_error().decode()
    assert lib.qe_population_policy_values(None, None, None, 1e-12, 10, p, None, None, None) == _lib.ERR_INVALID
    assert "engine is NULL" in lib.qe_last_error().decode()
    assert lib.qe_abi_version() == 2 and ctypes.sizeof(_lib.RolloutStats) == 104
    header = (ROOT / "include" / "qlearn_engine.h").read_text()
    assert re.search(r"\bint qe_env_table_solve\(qe_env\* env, double gamma, double tol, int32_t max_sweeps", header)
    assert re.search(r"\bint qe_population_policy_values\(qe_engine\* e, qe_env\* env, const double\* gammas", header)
    assert "#define QE_ABI_VERSION 2" in header


def test_the_unit_is_built_like_its_siblings():
    assert "$(OBJ)/mdp_solve.o: qe_mdp_solve.hip qe_mdp_solve.h" in (CSRC / "Makefile").read_text()


@pytest.fixture(scope="module")
def solve_asm(tmp_path_factory):
    unit = CSRC / "qe_mdp_solve.hip"
    assert unit.exists(), "the dynamic-programming kernels have a translation unit of their own"
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("mdp_solve_isa") / "mdp_solve.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed", "-S",
           "--cuda-device-only", str(unit), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return out.read_text().split("\n")


def test_solver_kernels_use_no_scratch(solve_asm):
    kernels = {n: k for n, k in _kernels(solve_asm).items() if "k_mdp_" in n}
    # two sweeps and the Q pass per record count 1 .. 8, the tie sets per table dtype, three small per-run kernels
    for stem, count in (("k_mdp_value_sweep", 8), ("k_mdp_policy_sweep", 8), ("k_mdp_q_values", 8), ("k_mdp_tie_sets", 2),
                        ("k_mdp_policy_begin", 1), ("k_mdp_policy_batch_end", 1), ("k_mdp_policy_collect", 1)):
        assert len([n for n in kernels if stem in n]) == count, (stem, sorted(kernels))
    assert len(kernels) == 29
    for name, (body, desc, meta) in kernels.items():
        assert meta["ScratchSize"] == 0, (name, meta)
        assert [x.split()[1] for x in desc if x.strip().startswith(".amdhsa_private_segment_fixed_size")] == ["0"], name
        assert meta["Occupancy"] >= 4, (name, meta)
        code = [x.strip() for x in body if x.startswith("\t") and not x.strip().startswith((";", "."))]
        assert code, name
        assert not [x for x in code if x.startswith(("scratch_", "buffer_"))], name  # no spill traffic of any kind
        if "_sweep" in name:  # the rows meet in 2 KiB of LDS
            assert meta["LDSByteSize"] == 2048, (name, meta)
