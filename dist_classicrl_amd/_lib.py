"""ctypes binding of ``libqlearn_engine.so`` (C ABI: ``include/qlearn_engine.h``).

There is deliberately no CPU fallback: if the HIP library is missing, or no MI355X is visible,
every compute entry point raises.  Building the library: ``python __graft_entry__.py`` or
``dist_classicrl_amd/csrc/build.sh``.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import os

# QE_LIB_PATH lets a developer A/B two builds of the library in one session; default = in-tree build
LIB_PATH = Path(os.environ.get("QE_LIB_PATH") or Path(__file__).resolve().parent / "csrc" / "libqlearn_engine.so")

ABI_VERSION = 2  # QE_ABI_VERSION of include/qlearn_engine.h
QE_F32, QE_F64 = 0, 1
LEARN_ITER, LEARN_VEC = 0, 1
ENV_HASH, ENV_GRID, ENV_BANDIT, ENV_TICTACTOE, ENV_TABLE = 0, 1, 2, 3, 4
OPT_ROLLOUT_PATH = 0
OPT_USE_GRAPH = 1
OPT_TOKEN_ROUNDS = 2
OPT_LISTED_MIN_AGENTS = 3
OPT_EVENT_TIMING = 4
OPT_HOST_BLOCK = 5
OPT_LANE_ORDERED_PATH = 6
OPT_TURN_FORWARD = 7
OPT_TURN_POLL = 8
OPT_STAMP_HASH_BITS = 9
PATH_AUTO, PATH_STEPWISE, PATH_PERSISTENT, PATH_WIDE, PATH_TURNSTILE = 0, 1, 2, 3, 4

RULE_Q_LEARNING, RULE_SARSA, RULE_EXPECTED_SARSA = 0, 1, 2  # qe_update_rule
N_STEP_MAX = 16  # qe_population_set_n_step
TREE_BACKUP_MAX = 16  # qe_population_set_tree_backup
TRACE_MAX = 32  # qe_population_set_traces
PLANNING_MAX = 64  # qe_population_set_planning
QUEUE_MAX = 32  # qe_population_set_sweeping
PLANNING_ORDERS = ("uniform", "prioritized")
MODEL_OUTCOMES_MAX = 8  # qe_population_set_model_outcomes
# qe_population_set_model_outcomes: the (table dtype, 16-byte loads per fp32 row) builds of k_dyna_sample_rollout that are NOT
# compiled because they do not fit the register file without scratch (dyna_sample_supported in csrc/qe_host.h, DESIGN
# section 4.3c)
DYNA_SAMPLE_REFUSED = frozenset()
# qe_population_set_sweeping: the (table dtype, 16-byte loads per fp32 row) builds of k_sweep_rollout that are NOT compiled
# because they do not fit the register file without scratch (sweep_supported in csrc/qe_host.h)
SWEEP_REFUSED = frozenset()
# qe_population_set_visits: the (table dtype, 16-byte loads per fp32 row) builds of k_visit_rollout that are NOT compiled
# because they do not fit the register file without scratch (visit_supported in csrc/qe_host.h)
VISIT_REFUSED = frozenset()
TRACE_REPLACING, TRACE_ACCUMULATING = 0, 1  # qe_trace_kind
TRACE_KINDS = {"replacing": TRACE_REPLACING, "accumulating": TRACE_ACCUMULATING}
UPDATE_RULES = {"q_learning": RULE_Q_LEARNING, "sarsa": RULE_SARSA, "expected_sarsa": RULE_EXPECTED_SARSA}

ERR_INVALID, ERR_NO_DEVICE, ERR_OOM, ERR_UNSUPPORTED, ERR_INDEX = -1, -2, -3, -4, -5


def decode_variant(v: int) -> dict:
    """Fields of ``qe_rollout_stats.kernel_variant`` (include/qlearn_engine.h).  ``rule``: the population's update rule
    -- path 8 (``population_td``, kernel ``k_rollout_runs_td``) carries it in bits 4-5, where the persistent path keeps
    ``lean``; every other path learns with Q-learning.  Paths 9 and 10 (``population_double``, kernel ``k_double_rollout``,
    and ``population_double_eval``, ``k_double_evaluate``) are the population with the double estimator.  Path 11
    (``population_nstep``, kernel ``k_nstep_rollout``) is the population with an n-step on-policy rule: the rule in
    bits 4-5 as path 8, and ``n_step`` in bits 24-28 (1 on every other path).  Path 12 (``population_trace``, kernel
    ``k_trace_rollout``) is the population with eligibility traces: the rule in bits 4-5 (0 = Q-learning, Watkins's
    Q(lambda); 1 = SARSA(lambda)), ``trace_length`` in bits 24-29 and ``trace_kind`` in bit 30 (0 and None on every other
    path).  Path 13 (``population_dyna``, kernel ``k_dyna_rollout``) is the Q-learning population with Dyna-Q: NV and
    masked as path 6 and ``planning_steps`` in bits 24-30, a key that only this path's dict has; with bit 4 set the
    planning order is prioritized sweeping (kernel ``k_sweep_rollout``) and the dict gains ``prioritized`` (True) and
    ``queue_length`` (bits 5-9 plus 1), two keys that no other dict has; with bits 21-23 non-zero the model is the sample
    model (kernel ``k_dyna_sample_rollout``) and the dict gains ``model_outcomes`` (those bits plus 1), a key that no
    other dict has.  Path 14
    (``population_visit``, kernel ``k_visit_rollout``) is the Q-learning population with visit counts: NV and masked as path
    6, ``visit_lr`` in bit 4 and ``bonus`` (some run's beta is above 0) in bit 5, two keys that only this path's dict has.
    Path 15 (``population_tree``, kernel ``k_tree_rollout``) is the Q-learning population with n-step Tree Backup: NV and
    masked as path 6 and ``tree_backup``, the horizon, in bits 24-28, a key that only this path's dict has (``n_step`` reads
    1 there)."""
    v = int(v)
    nstep = (v & 15) == 11
    trace = (v & 15) == 12
    td = (v & 15) == 8 or nstep
    out = {
        "path": {1: "stepwise", 2: "persistent", 3: "wide", 4: "turnstile", 5: "eval", 6: "population",
                 7: "population_eval", 8: "population_td", 9: "population_double", 10: "population_double_eval",
                 11: "population_nstep", 12: "population_trace", 13: "population_dyna", 14: "population_visit",
                 15: "population_tree"}.get(v & 15, "none"),
        "rule": ({1: "sarsa", 2: "expected_sarsa"}.get((v >> 4) & 3, "none") if td
                 else {0: "q_learning", 1: "sarsa"}.get((v >> 4) & 3, "none") if trace else "q_learning"),
        "lean": (v >> 4) & 3, "help": bool((v >> 6) & 1), "full": bool((v >> 7) & 1), "light": bool((v >> 8) & 1),
        "cap512": bool((v >> 9) & 1), "dataflow": bool((v >> 10) & 1), "nv": (v >> 12) & 255, "masked": bool((v >> 20) & 1),
        "n_step": (v >> 24) & 31 if nstep else 1,
        "trace_length": (v >> 24) & 63 if trace else 0,
        "trace_kind": ("accumulating" if (v >> 30) & 1 else "replacing") if trace else None,
    }
    if (v & 15) == 13:
        out["planning_steps"] = (v >> 24) & 127
        if (v >> 4) & 1:
            out["prioritized"] = True
            out["queue_length"] = ((v >> 5) & 31) + 1
        if (v >> 21) & 7:
            out["model_outcomes"] = ((v >> 21) & 7) + 1
    if (v & 15) == 14:
        out["visit_lr"] = bool((v >> 4) & 1)
        out["bonus"] = bool((v >> 5) & 1)
    if (v & 15) == 15:
        out["tree_backup"] = (v >> 24) & 31
    return out


def visit_build_shipped(dtype, action_size: int) -> bool:
    """Whether ``k_visit_rollout`` is built for rows of ``action_size`` actions of ``dtype`` (``VISIT_REFUSED``)."""
    nv = max(4, 1 << (int(action_size) - 1).bit_length()) // 4
    return (np.dtype(dtype).name, nv) not in VISIT_REFUSED


def sweep_build_shipped(dtype, action_size: int) -> bool:
    """Whether ``k_sweep_rollout`` is built for rows of ``action_size`` actions of ``dtype`` (``SWEEP_REFUSED``)."""
    nv = max(4, 1 << (int(action_size) - 1).bit_length()) // 4
    return (np.dtype(dtype).name, nv) not in SWEEP_REFUSED


def dyna_sample_build_shipped(dtype, action_size: int) -> bool:
    """Whether ``k_dyna_sample_rollout`` is built for rows of ``action_size`` actions of ``dtype`` (``DYNA_SAMPLE_REFUSED``)."""
    nv = max(4, 1 << (int(action_size) - 1).bit_length()) // 4
    return (np.dtype(dtype).name, nv) not in DYNA_SAMPLE_REFUSED


def variant_symbol(v: int, dtype: str = "float", env: str = "HashEnv", lanes_per_row: int = 4, vec: bool = False) -> str:
    """The kernel instantiation behind ``kernel_variant`` as rocprofv3 prints it (without the ``void qe::`` prefix and
    the argument list): what ``bench.py`` names in ``roofline.kernel`` and matches profile files against."""
    d = decode_variant(v)
    b = lambda x: "true" if x else "false"  # noqa: E731
    if d["path"] == "persistent" and d["dataflow"]:
        return f"k_rollout_df<{dtype}, qe::{env}, {d['nv']}, {b(d['masked'])}, {d['lean']}, {b(d['full'])}>"
    if d["path"] == "persistent":
        cap = 512 if d["cap512"] else 128
        return (f"k_rollout_lane<{dtype}, qe::{env}, {d['nv']}, {cap}, {b(d['masked'])}, {d['lean']}, {b(d['help'])}, "
                f"{b(d['full'])}, {b(d['light'])}>")
    lc = lanes_per_row if env == "HashEnv" and lanes_per_row in (4, 8, 16) else 0
    name = {"turnstile": "k_step_turn", "stepwise": "k_step_fast", "wide": "k_step_fast", "eval": "k_eval"}.get(d["path"], "?")
    if name == "k_step_turn":
        return f"k_step_turn<{dtype}, qe::{env}, {lc}, {b(vec)}>"
    return f"{name}<{dtype}, qe::{env}, {lc}>" if name != "k_eval" else f"k_eval<{dtype}, qe::{env}>"


class EngineError(RuntimeError):
    """The HIP engine reported a failure that has no closer Python equivalent."""


class EnvParams(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("masked", C.c_int32),
        ("seed", C.c_uint32),
        ("p_term_256", C.c_int32),
        ("side", C.c_int32),
        ("episode_len", C.c_int32),
        ("agent_offset", C.c_uint32),
        ("reserved", C.c_int32),
    ]


class TableMdp(C.Structure):
    """``qe_table_mdp``: host pointers to an encoded finite MDP (``environments.device_envs.encode_table_mdp``)."""

    _fields_ = [
        ("k", C.c_int32),
        ("n_start", C.c_int32),
        ("thr", C.POINTER(C.c_uint32)),
        ("next_state", C.POINTER(C.c_int32)),
        ("reward", C.POINTER(C.c_float)),
        ("terminated", C.POINTER(C.c_uint8)),
        ("start_thr", C.POINTER(C.c_uint32)),
        ("start_state", C.POINTER(C.c_int32)),
        ("masks", C.POINTER(C.c_uint8)),
    ]


class RolloutStats(C.Structure):
    _fields_ = [
        ("kernel_ms", C.c_double),
        ("launches", C.c_int64),
        ("episodes", C.c_int64),
        ("involved", C.c_int64),
        ("episodes_dropped", C.c_int64),
        ("dominant_ms", C.c_double),
        ("dominant_launches", C.c_int64),
        ("dominant_env_steps", C.c_int64),
        ("device_clock_ms", C.c_double),
        ("host_begin_us", C.c_double),
        ("host_end_us", C.c_double),
        ("kernel_variant", C.c_int64),
        ("complex_steps", C.c_int64),
    ]


class RunSchedule(C.Structure):
    """``qe_run_schedule``: one run's schedule of a population, as the kernel advances it once per step."""

    _fields_ = [("value", C.c_double), ("min_value", C.c_double), ("factor", C.c_double), ("kind", C.c_int32),
                ("reserved", C.c_int32)]


_P = C.c_void_p
_I32P = C.POINTER(C.c_int32)
_U32P = C.POINTER(C.c_uint32)
_U8P = C.POINTER(C.c_uint8)
_F32P = C.POINTER(C.c_float)
_F64P = C.POINTER(C.c_double)
_I64P = C.POINTER(C.c_int64)
_U64P = C.POINTER(C.c_uint64)

# name -> (restype, argtypes); must list every symbol include/qlearn_engine.h declares
PROTOTYPES = {
    "qe_abi_version": (C.c_int, []),
    "qe_last_error": (C.c_char_p, []),
    "qe_create": (C.c_int, [C.POINTER(_P), C.c_int64, C.c_int32, C.c_double, C.c_uint64, C.c_int32, C.c_int32]),
    "qe_destroy": (C.c_int, [_P]),
    "qe_synchronize": (C.c_int, [_P]),
    "qe_set_stream": (C.c_int, [_P, _P]),
    "qe_set_option": (C.c_int, [_P, C.c_int32, C.c_int64]),
    "qe_table_upload": (C.c_int, [_P, _P, C.c_int32]),
    "qe_table_download": (C.c_int, [_P, _P, C.c_int32]),
    "qe_table_download_rows": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "qe_table_upload_rows": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "qe_table_cells": (C.c_int, [_P, _I32P, _I32P, C.c_int64, _F64P, C.c_int32]),
    "qe_table_dev": (_P, [_P]),
    "qe_table_row_stride": (C.c_int64, [_P]),
    "qe_set_step_counter": (C.c_int, [_P, C.c_uint64]),
    "qe_get_step_counter": (C.c_uint64, [_P]),
    "qe_set_agent_offset": (C.c_int, [_P, C.c_uint32]),
    "qe_choose_actions": (C.c_int, [_P, _I32P, C.c_int64, _U8P, C.c_double, C.c_int32, _I32P]),
    "qe_learn": (C.c_int, [_P, _I32P, _I32P, _F32P, _I32P, _U8P, C.c_int64, C.c_double, _U8P, C.c_int32]),
    "qe_env_create": (C.c_int, [C.POINTER(_P), _P, C.c_int64, C.POINTER(EnvParams)]),
    "qe_env_create_table": (C.c_int, [C.POINTER(_P), _P, C.c_int64, C.POINTER(EnvParams), C.POINTER(TableMdp)]),
    "qe_env_destroy": (C.c_int, [_P]),
    "qe_env_reset": (C.c_int, [_P, C.c_int32, C.c_uint32]),
    "qe_env_observe": (C.c_int, [_P, _I32P, _U8P, _F32P]),
    "qe_env_restore": (C.c_int, [_P, _I32P, _U32P, _F32P]),
    "qe_env_aux": (C.c_int, [_P, _U32P]),
    "qe_env_step": (C.c_int, [_P, _I32P, _I32P, _F32P, _U8P, _U8P]),
    "qe_rollout": (C.c_int, [_P, _P, C.c_int64, _F64P, _F64P, C.c_int32, _I32P, C.POINTER(RolloutStats)]),
    "qe_rollout_begin": (C.c_int, [_P, _P, C.c_int64, _F64P, _F64P, C.c_int32, C.c_int32]),
    "qe_schedule_plan": (C.c_int, [_P, _F64P, _F64P, C.c_int64]),
    "qe_rollout_end": (C.c_int, [_P, C.c_int32, C.POINTER(RolloutStats)]),
    "qe_rollout_chunk_limit": (C.c_int64, [_P, _P, C.c_int32]),
    "qe_rollout_fused": (C.c_int64, [_P, _P, C.c_int64, _F64P, _F64P, C.c_int32, C.POINTER(RolloutStats), C.c_int64, _I32P,
                                     _F32P, _F32P, _I32P, _U32P, _F32P]),
    "qe_evaluate": (C.c_int, [_P, _P, C.c_int64, C.POINTER(RolloutStats)]),
    "qe_episode_log": (C.c_int64, [_P, C.c_int64, _I32P, _I32P, _F32P]),
    "qe_delta_log_attach": (C.c_int, [_P, _P, C.c_int64]),
    "qe_delta_log_count": (C.c_int64, [_P]),
    "qe_delta_log_reset": (C.c_int, [_P]),
    "qe_delta_apply_dev": (C.c_int, [_P, _P, C.c_int64]),
    "qe_delta_apply_skip_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64]),
    "qe_delta_apply_sorted_dev": (C.c_int, [_P, _P, C.c_int64]),
    "qe_delta_apply_gathered_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "qe_create_population": (C.c_int, [C.POINTER(_P), C.c_int64, C.c_int64, C.c_int32, C.c_uint64, C.c_int32, C.c_int32]),
    "qe_population_runs": (C.c_int64, [_P]),
    "qe_population_configure": (C.c_int, [_P, C.POINTER(RunSchedule), C.POINTER(RunSchedule), _F64P]),
    "qe_population_schedules": (C.c_int, [_P, _F64P, _F64P]),
    "qe_population_rollout": (C.c_int64, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(RolloutStats), _I64P, _F32P,
                                          _I32P, _U32P, _F32P, _U32P]),
    "qe_population_evaluate": (C.c_int64, [_P, _P, C.c_int64, C.c_int64, C.c_int32, C.POINTER(RolloutStats), _I64P, _F32P,
                                           _I64P, _U32P]),
    "qe_population_log": (C.c_int64, [_P, C.c_int64, _I32P, _F32P]),
    "qe_population_step_counters": (C.c_int, [_P, _U64P]),
    "qe_population_set_step_counters": (C.c_int, [_P, _U64P]),
    "qe_population_set_update_rule": (C.c_int, [_P, C.c_int32]),
    "qe_population_update_rule": (C.c_int, [_P]),
    "qe_population_pending_actions": (C.c_int, [_P, _I32P]),
    "qe_population_set_pending_actions": (C.c_int, [_P, _I32P]),
    "qe_population_set_double": (C.c_int, [_P, C.c_int32]),
    "qe_population_double": (C.c_int, [_P]),
    "qe_population_table_b_upload": (C.c_int, [_P, _P, C.c_int32]),
    "qe_population_table_b_download": (C.c_int, [_P, _P, C.c_int32]),
    "qe_population_table_b_download_rows": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "qe_population_set_n_step": (C.c_int, [_P, C.c_int32]),
    "qe_population_n_step": (C.c_int, [_P]),
    "qe_population_window": (C.c_int, [_P, _I32P, _I32P, _I32P, _F32P]),
    "qe_population_set_window": (C.c_int, [_P, _I32P, _I32P, _I32P, _F32P]),
    "qe_population_set_tree_backup": (C.c_int, [_P, C.c_int32]),
    "qe_population_tree_backup": (C.c_int, [_P]),
    "qe_population_tree_window": (C.c_int, [_P, _I32P, _I32P, _I32P, _F32P, _U8P]),
    "qe_population_set_tree_window": (C.c_int, [_P, _I32P, _I32P, _I32P, _F32P, _U8P]),
    "qe_population_set_traces": (C.c_int, [_P, C.c_int32, C.c_int32, _F64P]),
    "qe_population_trace_config": (C.c_int, [_P, _I32P, _I32P, _F64P]),
    "qe_population_traces": (C.c_int, [_P, _I32P, _I32P, _F64P]),
    "qe_population_set_trace_state": (C.c_int, [_P, _I32P, _I32P, _F64P]),
    "qe_population_set_planning": (C.c_int, [_P, C.c_int32]),
    "qe_population_planning": (C.c_int, [_P]),
    "qe_population_model": (C.c_int, [_P, _I32P, _F32P, _U8P, _I32P, _I32P]),
    "qe_population_set_model": (C.c_int, [_P, _I32P, _F32P, _U8P, _I32P, _I32P]),
    "qe_population_set_model_outcomes": (C.c_int, [_P, C.c_int32]),
    "qe_population_model_outcomes": (C.c_int, [_P]),
    "qe_population_outcome_model": (C.c_int, [_P, _I32P, _F32P, _U8P, _U32P, _I32P, _I32P]),
    "qe_population_set_outcome_model": (C.c_int, [_P, _I32P, _F32P, _U8P, _U32P, _I32P, _I32P]),
    "qe_population_set_sweeping": (C.c_int, [_P, C.c_int32, _F64P]),
    "qe_population_sweeping": (C.c_int, [_P]),
    "qe_population_predecessors": (C.c_int, [_P, _I32P, _I32P]),
    "qe_population_set_predecessors": (C.c_int, [_P, _I32P, _I32P]),
    "qe_population_queue": (C.c_int, [_P, _I32P, _F64P]),
    "qe_population_set_queue": (C.c_int, [_P, _I32P, _F64P]),
    "qe_population_set_visits": (C.c_int, [_P, _F64P, C.c_int32]),
    "qe_population_visits": (C.c_int, [_P, _I32P, _I32P, _F64P]),
    "qe_population_visit_counts": (C.c_int, [_P, _U32P]),
    "qe_population_set_visit_counts": (C.c_int, [_P, _U32P]),
    "qe_population_visit_bonus": (C.c_int, [_P, _P, C.c_int32]),
    "qe_env_table_solve": (C.c_int, [_P, C.c_double, C.c_double, C.c_int32, _F64P, _F64P, _I32P, _F64P]),
    "qe_population_policy_values": (C.c_int, [_P, _P, _F64P, C.c_double, C.c_int32, _F64P, _I32P, _F64P, _U32P]),
    "qe_debug_occupy_cus": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "qe_debug_set_turn_epoch": (C.c_int, [_P, C.c_uint64]),
    "qe_debug_turn_epoch": (C.c_uint64, [_P]),
    "qe_replay_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64]),
    "qe_replay_destroy": (C.c_int, [_P]),
    "qe_replay_push": (C.c_int, [_P, _I64P, _I64P, _F64P, _I64P, _U8P, C.c_int64]),
    "qe_replay_attach": (C.c_int, [_P, _P]),
    "qe_replay_len": (C.c_int64, [_P]),
    "qe_replay_position": (C.c_int64, [_P]),
    "qe_replay_full": (C.c_int32, [_P]),
    "qe_replay_gather": (C.c_int, [_P, _I64P, C.c_int64, _I64P, _I64P, _F64P, _I64P, _U8P]),
    "qe_replay_learn": (C.c_int, [_P, _P, _I64P, C.c_int64, C.c_double, C.c_int32]),
}

_lib = None


def load():
    """Load the HIP library (once).  Raises ``ImportError`` with build instructions if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        msg = (
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (or "
            "dist_classicrl_amd/csrc/build.sh). The engine has no CPU fallback."
        )
        raise ImportError(msg)
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table diverge
        fn.restype = res
        fn.argtypes = args
    if lib.qe_abi_version() != ABI_VERSION:
        msg = f"ABI version mismatch: library {lib.qe_abi_version()}, binding {ABI_VERSION}"
        raise ImportError(msg)
    _lib = lib
    return lib


def check(rc: int) -> None:
    """Translate a negative ``qe_status`` into the exception the reference would raise."""
    if rc >= 0:
        return
    text = load().qe_last_error().decode(errors="replace")
    if rc == ERR_INDEX:
        raise IndexError(text)
    if rc == ERR_INVALID:
        raise ValueError(text)
    if rc == ERR_OOM:
        raise MemoryError(text)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(text)
    raise EngineError(text)


def ptr(arr, ctype):
    """Typed pointer to a C-contiguous NumPy array (``None`` -> NULL)."""
    if arr is None:
        return None
    return arr.ctypes.data_as(C.POINTER(ctype))


def as_i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def as_u8_flags(x):
    """Truthiness -> one byte per element (the reference treats any non-zero mask entry as valid)."""
    x = np.asarray(x)
    return np.ascontiguousarray(x != 0, dtype=np.uint8)
