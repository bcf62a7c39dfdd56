"""``QLearningPopulation``: many independent single-agent Q-learners trained in one launch.

The case of 20 to 1000 seeds for a confidence band, or a grid over learning rate, exploration schedule and discount:
each run is the classic one-environment ``SingleThreadQLearning`` of the reference, and all of them step together on
the GPU, one lane per run (``qe_population_rollout``, kernel ``k_rollout_runs``).

Contract: a population of ``M`` runs over one environment object of ``num_agents = M`` and one seed.  Run ``r`` after
``K`` steps is, bit for bit (table, episode returns and their steps, final observation, env-internal state, running
return), the standalone run

    algo = OptimalQLearningBase(S, A, discount_factor[r], seed, dtype=dtype)
    GpuRolloutQLearning(algo, lr_schedule[r], exploration_rate_schedule[r], learn_mode).run_steps(K, env_r)

where ``env_r`` is the same environment kind and parameters with one agent and ``agent_offset = env_offset + r``.
Calls chain: one call of 2K steps equals two calls of K steps, schedule values included.

Greedy evaluation (``evaluate_steps`` / ``evaluate_episodes``, kernel ``k_evaluate_runs``) and ``train`` follow the same
contract: run ``r`` is the standalone runtime's ``evaluate_steps`` / ``evaluate_episodes`` / ``train`` of that one-agent
run.  Each run keeps its own draw counter (``step_counters``): an episode-based evaluation advances run ``r`` by the
steps it took, as the standalone ``evaluate_episodes`` does, so later training still draws what the standalone run draws.

``update_rule`` chooses the TD target of every run (one rule per population): ``"q_learning"`` (the default, and the
contract above), ``"sarsa"`` or ``"expected_sarsa"`` (kernel ``k_rollout_runs_td``).  The reference has no on-policy
rule to equal; DESIGN section 4.3c defines both, and ``tests/td_rules_model.py`` restates that definition on the oracle.
A SARSA run has chosen its next action when a call returns: ``state_dict["pending_actions"]`` carries it to the next
call (or process), so the chaining contract holds for every rule.

``double_q=True`` turns Q-learning into Double Q-learning (van Hasselt 2010; kernels ``k_double_rollout`` /
``k_double_evaluate``): every run owns two tables, A (``q_tables``) and B (``q_tables_b``), acts on their sum, and each
step updates the one a coin names with the other's value at its own arg-max -- the cure for the maximisation bias of
``max_a' Q[s', a']``.  The coin is the unused fourth word of the step's policy draws, so there is no new run state
besides B.  DESIGN section 4.3c defines the step; ``tests/double_q_model.py`` restates it on the oracle.

``n_step=n`` (2 .. 16; kernel ``k_nstep_rollout``) gives the on-policy rules the bootstrapping horizon of n-step TD
(Sutton & Barto ch. 7): n-step SARSA and n-step Expected SARSA, the lever between TD(0) and Monte Carlo when reward
arrives only at the end of an episode.  A run keeps a window of its last transitions; ``state_dict["n_step_window"]``
carries it from call to call as ``pending_actions`` carries SARSA's action.  An uncorrected n-step Q-learning is not an
off-policy method, so ``update_rule="q_learning"`` and ``double_q=True`` are refused with ``n_step > 1``: Q-learning's
horizon is ``tree_backup``.  DESIGN section 4.3c defines the step; ``tests/n_step_model.py`` restates it on the oracle.

``tree_backup=n`` (2 .. 16, Q-learning only; kernel ``k_tree_rollout``) is that horizon: n-step Tree Backup under a greedy
target policy (Sutton & Barto 7.5), the off-policy n-step method that needs no importance ratios.  A run keeps a window
of entries ``(s, a, r, greedy)``; an entry's n-step return passes through the later entries while their actions were
greedy (``Q[s, a] == max Q[s, valid]`` when they were taken) and stops at the first that was not, where the row maximum
of that state, read from the table at the update, stands in for the rest.  With epsilon 0 it is n-step Expected SARSA at
epsilon 0; with ``tree_backup=1`` (the default) it is the one-step Q-learning above, same kernel, nothing allocated.
``state_dict["tree_backup_window"]`` carries the window from call to call.  Every other rule, ``double_q=True``,
``n_step > 1``, ``trace_decay``, ``planning_steps > 0``, ``exploration_bonus`` and ``visit_lr`` are refused with it.  DESIGN
section 4.3c defines the step; ``tests/tree_backup_model.py`` restates it on the oracle.

``trace_decay=lam`` (one lambda in [0, 1] or one per run; kernel ``k_trace_rollout``) turns on eligibility traces
(Sutton & Barto ch. 12): SARSA(lambda) under ``update_rule="sarsa"``, Watkins's Q(lambda) under ``"q_learning"`` -- the
multi-step method that updates backwards at every step instead of ``n`` steps late, and the one Q-learning has.  A run
keeps ``trace_length`` slots ``(s, a, e)``, a truncated sparse trace table: a step marks its cell (``trace_kind``
"replacing": e = 1, "accumulating": e + 1; a full table drops its smallest trace), adds ``u * e`` to every live cell, u
the one-step rule's increment, and decays every trace by ``gamma * lam``; Q(lambda) cuts all traces at a non-greedy
action.  ``state_dict["eligibility_traces"]`` carries the slots from call to call.  ``update_rule="expected_sarsa"``,
``double_q=True`` and ``n_step > 1`` are refused with traces.  DESIGN section 4.3c defines the step;
``tests/trace_model.py`` restates it on the oracle.

``planning_steps=n`` (0 .. 64, Q-learning only; kernel ``k_dyna_rollout``) turns on Dyna-Q (Sutton & Barto ch. 8), the
model-based method: every run remembers the last observed outcome ``(s', r, terminated)`` of every cell it has tried
and, after each real step, replays ``n`` remembered transitions, drawn from the cells it has seen, through the same
Q-learning update -- on sparse-reward tasks the largest lever on sample efficiency a tabular learner has.  The model is
knowledge, like the tables: it outlives calls and environment resets, greedy evaluation neither reads nor writes it, and
it is NOT in the state dict.  :attr:`planning_model` reads and sets it, ``save_model`` / ``load_model`` keep it in one
``.npz``.  A fresh process resumes with ``load`` (tables), ``load_model`` (model) and ``restore_training_state`` (counters,
schedules), then passes the state dict to ``run_steps``.  ``double_q=True``, ``n_step > 1`` and ``trace_decay`` are
refused with planning.  DESIGN section 4.3c defines the step; ``tests/dyna_model.py`` restates it on the oracle.

``model_outcomes=K`` (2 .. 8, with ``planning_steps=n``; kernel ``k_dyna_sample_rollout``) gives Dyna-Q the sample model
of Sutton & Barto ch. 8 for stochastic environments: every run remembers up to ``K`` distinct outcomes of every cell with
their counts -- an outcome is told apart by its reward's 32 bits, its flag and, unless terminated, its next observation;
when all slots are taken the rarest outcome is replaced -- and a planning update draws one of them in proportion to its
count (a Philox stream of its own), so planning pulls ``Q[s, a]`` towards the expectation, not towards the last sample.
All of it is integer work, so the runs equal a NumPy model bit for bit.  ``model_outcomes=1``, the default, is the
last-outcome model above, unchanged.  :attr:`planning_model` gains the slot axis and ``outcome_counts``; a model saved by
a last-outcome population loads as slot 0 with count 1.  Refused with ``planning_order="prioritized"`` (sweeping over a
sample model needs expected updates, which are not built); everything Dyna-Q refuses is refused here too.  DESIGN
section 4.3c defines the step; ``tests/dyna_sample_model.py`` restates it on the oracle.

``planning_order="prioritized"`` (with ``planning_steps=n``; kernel ``k_sweep_rollout``) replaces the uniform draws of
Dyna-Q by prioritized sweeping (Moore & Atkeson 1993; Sutton & Barto 8.4): the ``n`` updates go where the table is about
to change.  Every run keeps the predecessors of every state (the cells its model leads there from) and a queue of
``queue_length`` cells; when an update changes a cell by more than ``sweep_threshold`` (one value or one per run: a grid
axis), the predecessors of its state whose own update would change by more than the threshold enter the queue with that
size as priority, and planning pops the largest first and stops early when the queue is empty.  No draw is consumed and
every operation is a compare, an ``abs`` or the update itself, so the runs equal a NumPy model bit for bit.  The
predecessor lists are knowledge and travel with the model (``planning_model`` gains ``pred_head`` and ``pred_next``;
a model saved by a Dyna-Q population loads, its lists are rebuilt); the queue is run state:
``state_dict["sweep_queue"]`` carries it from call to call, :attr:`sweep_queue` reads and sets it.  A fresh process
resumes with ``load``, ``load_model`` and ``restore_training_state``, in that order.  Everything Dyna-Q refuses is refused
here too.  DESIGN section 4.3c defines the step; ``tests/sweep_model.py`` restates it on the oracle.

``exploration_bonus=beta`` (one beta >= 0 or one per run) and ``visit_lr=True`` (Q-learning only; kernel
``k_visit_rollout``) turn on per-cell visit counts ``N(s, a)``, the directed-exploration lever next to epsilon.  The pick
sees ``Q[s, :] + beta / sqrt(N[s, :])`` instead of the Q-row (count-based optimism, MBIE-EB: an untried action has an
infinite bonus and goes first), the target stays ``max Q`` and the prediction ``Q[s, a]``; ``visit_lr`` divides the
step's learning rate by the incremented ``N[s, a]``, the sample-average rate ``1/N``.  The square root and the divisions
are float64 and correctly rounded, so the runs equal a NumPy model bit for bit.  Counts are knowledge, like the tables
and the Dyna model: they outlive calls and environment resets, greedy evaluation neither reads nor writes them, and they
are NOT in the state dict.  :attr:`visit_counts` reads and sets them, :attr:`visit_bonus` reads the bonus the next pick
adds.  A fresh process resumes with ``load`` (tables), ``pop.visit_counts = ...`` and ``restore_training_state``.  The
other rules, ``double_q=True``, ``n_step > 1``, ``trace_decay`` and ``planning_steps > 0`` are refused with counting.
DESIGN section 4.3c defines the step; ``tests/visit_model.py`` restates it on the oracle.
"""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from dist_classicrl_amd import _lib
from dist_classicrl_amd.environments.device_envs import DeviceVecEnv, check_discounts, check_solve_args, start_value
from dist_classicrl_amd.schedules import BaseSchedule, ConstantSchedule, ExponentialSchedule, LinearSchedule

SCHED_CONSTANT, SCHED_LINEAR, SCHED_EXPONENTIAL = 0, 1, 2
# qe_run_schedule as a NumPy record (the per-run descriptor arrays handed to qe_population_configure)
_DESCRIPTOR = np.dtype([("value", "<f8"), ("min_value", "<f8"), ("factor", "<f8"), ("kind", "<i4"), ("reserved", "<i4")])


def schedule_descriptor(schedule) -> tuple[int, float, float, float]:
    """``(kind, value, min_value, factor)`` of one of the three schedules, ``factor`` computed as their ``update(1)``
    does (``decay_rate ** 1`` / ``1 * decay_rate``).  Any other schedule raises ``TypeError``: the kernel can only
    restate these recurrences."""
    kind = type(schedule)
    if kind is ConstantSchedule:
        return SCHED_CONSTANT, float(schedule.get_value()), float(schedule.min_value), 0.0
    if kind is LinearSchedule:
        return SCHED_LINEAR, float(schedule.get_value()), float(schedule.min_value), float(1 * schedule.decay_rate)
    if kind is ExponentialSchedule:
        return SCHED_EXPONENTIAL, float(schedule.get_value()), float(schedule.min_value), float(schedule.decay_rate**1)
    if isinstance(schedule, BaseSchedule):
        msg = f"{kind.__name__} has no device form: a population takes ConstantSchedule, LinearSchedule or ExponentialSchedule"
    else:
        msg = f"expected a schedule, got {kind.__name__}"
    raise TypeError(msg)


def advance_descriptor(kind: int, value: float, min_value: float, factor: float, count: int) -> np.ndarray:
    """The values the kernel reads at ``count`` consecutive steps (its recurrence, restated)."""
    out = np.empty(count, dtype=np.float64)
    v = float(value)
    for t in range(count):
        out[t] = v
        if kind == SCHED_LINEAR:
            v = v + factor
        elif kind == SCHED_EXPONENTIAL:
            x = v * factor
            v = min_value if min_value > x else x
    return out


class PopulationRun(NamedTuple):
    """Result of one :meth:`QLearningPopulation.run_steps` call."""

    mean_returns: np.ndarray    # float32 [M]: sequential float32 sum of the run's returns / their count; NaN if none
    episode_counts: np.ndarray  # int64 [M]
    returns: np.ndarray         # float32, every run's returns in order, run after run (empty without the log)
    offsets: np.ndarray         # int64 [M + 1]: run r's returns are returns[offsets[r]:offsets[r + 1]]
    steps: np.ndarray           # int32, step within the call at which each of those episodes ended
    state_dict: dict            # what an exact resume needs (pass it to the next call / restore_training_state)

    def run_returns(self, r: int) -> np.ndarray:
        return self.returns[self.offsets[r]:self.offsets[r + 1]]

    def run_steps(self, r: int) -> np.ndarray:
        return self.steps[self.offsets[r]:self.offsets[r + 1]]


class PopulationEval(NamedTuple):
    """Result of :meth:`QLearningPopulation.evaluate_steps` / :meth:`~QLearningPopulation.evaluate_episodes`."""

    totals: np.ndarray          # float32 [M]: sequential float32 sum of the run's returns (the standalone sum(history)); 0 if none
    episode_counts: np.ndarray  # int64 [M]
    returns: np.ndarray         # float32, every run's returns in order, run after run (empty without the log)
    offsets: np.ndarray         # int64 [M + 1]: run r's returns are returns[offsets[r]:offsets[r + 1]]
    steps_used: np.ndarray      # int64 [M]: steps each run took
    finished: np.ndarray        # bool [M]: episode mode: the run reached its episode count (False: stopped by max_steps)

    def run_returns(self, r: int) -> np.ndarray:
        return self.returns[self.offsets[r]:self.offsets[r + 1]]


class PopulationTraining(NamedTuple):
    """Result of :meth:`QLearningPopulation.train`."""

    returns: np.ndarray       # float32: every run's training returns of all segments in order, run after run
    offsets: np.ndarray       # int64 [M + 1]: run r's are returns[offsets[r]:offsets[r + 1]] (its reward_history)
    val_totals: np.ndarray    # float32 [segments, M]: column r is run r's val_reward_history
    val_finished: np.ndarray  # bool [segments, M]: PopulationEval.finished of each validation
    segments: list            # the PopulationRun of each training segment
    state_dict: dict          # state dict of the last segment

    def run_reward_history(self, r: int) -> np.ndarray:
        return self.returns[self.offsets[r]:self.offsets[r + 1]]


class PolicyValues(NamedTuple):
    """:meth:`QLearningPopulation.policy_values`: the exact value of every run's greedy policy on a table MDP."""

    values: np.ndarray        # float64[M, S]  V of run r's greedy policy (NaN for a run with status bit 1)
    start_values: np.ndarray  # float64[M]     sum over the start support of p_i * values[r, start_state_i]
    sweeps: np.ndarray        # int32[M]       the sweep each run froze at (or max_sweeps; 0 with status bit 1)
    residuals: np.ndarray     # float64[M]     max_s |V_t - V_{t-1}| of that sweep
    converged: np.ndarray     # bool[M]        residual <= tol
    status: np.ndarray        # uint32[M]      bit 0: a state without a valid action; bit 1: a NaN in a valid cell


def pending_array(values, runs) -> np.ndarray | None:
    """``pending_actions`` of a state dict as the int32 ``[runs]`` array the library takes (None: no run has one);
    ``ValueError`` on any other shape."""
    if values is None:
        return None
    arr = np.asarray(values)
    if arr.shape != (runs,) or arr.dtype.kind not in "iu":
        msg = f"pending_actions: expected {runs} integers, got shape {arr.shape} of {arr.dtype}"
        raise ValueError(msg)
    return np.ascontiguousarray(arr, dtype=np.int32)


# Dict-valued per-run state as the library takes it: one (key, shape, accepted dtype kinds, target dtype) per array, in
# the order of the library's arguments.
_CTYPES = {np.dtype(np.int32): C.c_int32, np.dtype(np.float32): C.c_float, np.dtype(np.float64): C.c_double,
           np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint32): C.c_uint32}


def _window_specs(runs, n_step):
    slots = (runs, n_step - 1)
    return (("length", (runs,), "iu", np.int32), ("states", slots, "iu", np.int32), ("actions", slots, "iu", np.int32),
            ("rewards", slots, "fiu", np.float32))


def _tree_specs(runs, tree_backup):
    slots = (runs, tree_backup - 1)
    return (*_window_specs(runs, tree_backup), ("greedy", slots, "biu", np.uint8))


def _trace_specs(runs, trace_length):
    slots = (runs, trace_length)
    return ("states", slots, "iu", np.int32), ("actions", slots, "iu", np.int32), ("values", slots, "fiu", np.float64)


def _model_specs(runs, state_size, action_size):
    cells = (runs, state_size, action_size)
    return (("next_states", cells, "iu", np.int32), ("rewards", cells, "f", np.float32), ("terminated", cells, "b", np.uint8),
            ("visited", (runs, state_size * action_size), "iu", np.int32), ("count", (runs,), "iu", np.int32))


def _outcome_model_specs(runs, state_size, action_size, model_outcomes):
    slots = (runs, state_size, action_size, model_outcomes)
    return (("next_states", slots, "iu", np.int32), ("rewards", slots, "f", np.float32), ("terminated", slots, "b", np.uint8),
            ("outcome_counts", slots, "iu", np.uint32), *_model_specs(runs, state_size, action_size)[3:])


def _sweep_model_specs(runs, state_size, action_size):
    return (*_model_specs(runs, state_size, action_size), ("pred_head", (runs, state_size), "iu", np.int32),
            ("pred_next", (runs, state_size, action_size), "iu", np.int32))


def _queue_specs(runs, queue_length):
    slots = (runs, queue_length)
    return ("cells", slots, "iu", np.int32), ("priorities", slots, "fiu", np.float64)


def _spec_arrays(what, value, specs, exact=False) -> tuple | None:
    """The dict ``value`` (``what`` names it) as the tuple of contiguous arrays ``specs`` describes; None for None and
    ``ValueError`` on anything else.  ``exact``: no cast may change a value -- a float must be exact in the target dtype
    and an integer lie inside int32."""
    if value is None:
        return None
    names = [repr(key) for key, *_ in specs]
    if not isinstance(value, dict) or sorted(value) != sorted(key for key, *_ in specs):
        msg = f"{what}: expected a dict with the keys {', '.join(names[:-1])} and {names[-1]}"
        raise ValueError(msg)
    out = []
    for key, shape, kinds, dtype in specs:
        arr = np.asarray(value[key])
        lossy = (exact and kinds == "f" and arr.dtype.kind == "f" and arr.dtype.itemsize > np.dtype(dtype).itemsize
                 and not np.array_equal(arr.astype(dtype), arr, equal_nan=True))
        if arr.shape != shape or arr.dtype.kind not in kinds or lossy:
            want = "bool" if kinds == "b" else np.dtype(dtype)
            msg = f"{what}[{key!r}]: expected shape {shape} of {want}, got shape {arr.shape} of {arr.dtype}"
            raise ValueError(msg)
        if exact and kinds == "iu" and arr.size and (arr.min() < -(2 ** 31) or arr.max() >= 2 ** 31):
            msg = f"{what}[{key!r}]: expected shape {shape} of {np.dtype(dtype)}, got values outside int32"
            raise ValueError(msg)
        out.append(np.ascontiguousarray(arr, dtype=dtype))
    return tuple(out)


def window_arrays(window, runs, n_step) -> tuple | None:
    """``n_step_window`` of a state dict as the ``(length, states, actions, rewards)`` arrays the library takes (None:
    every window empty): int32 ``[runs]``, int32 ``[runs, n_step - 1]`` twice and float32 ``[runs, n_step - 1]``;
    ``ValueError`` on anything else."""
    return _spec_arrays("n_step_window", window, _window_specs(runs, n_step))


def tree_window_arrays(window, runs, tree_backup) -> tuple | None:
    """``tree_backup_window`` of a state dict as the ``(length, states, actions, rewards, greedy)`` arrays the library takes
    (None: every window empty): those of :func:`window_arrays` for ``tree_backup - 1`` slots and uint8 ``[runs,
    tree_backup - 1]`` (bools or integers; the library refuses a flag other than 0 or 1); ``ValueError`` on anything
    else."""
    arrays = _spec_arrays("tree_backup_window", window, _tree_specs(runs, tree_backup))
    if arrays is not None:
        flags = np.asarray(window["greedy"])
        if flags.dtype.kind != "b" and flags.size and (flags.min() < 0 or flags.max() > 1):
            msg = f"tree_backup_window['greedy']: expected flags 0 or 1, got values in [{flags.min()}, {flags.max()}]"
            raise ValueError(msg)
    return arrays


def trace_arrays(traces, runs, trace_length) -> tuple | None:
    """``eligibility_traces`` of a state dict as the ``(states, actions, values)`` arrays the library takes (None: every
    slot free): int32 ``[runs, trace_length]`` twice and float64 ``[runs, trace_length]``; ``ValueError`` on anything
    else."""
    return _spec_arrays("eligibility_traces", traces, _trace_specs(runs, trace_length))


def model_arrays(model, runs, state_size, action_size) -> tuple | None:
    """A ``planning_model`` as the ``(next_states, rewards, terminated, visited, count)`` arrays the library takes (None:
    nothing is known): int32 ``[runs, S, A]``, float32 ``[runs, S, A]``, uint8 ``[runs, S, A]``, int32 ``[runs, S * A]`` and
    int32 ``[runs]``; ``ValueError`` on anything else.  Whether list and model agree is the library's check."""
    return _spec_arrays("planning_model", model, _model_specs(runs, state_size, action_size), exact=True)


def sweep_model_arrays(model, runs, state_size, action_size) -> tuple | None:
    """A ``planning_model`` of a population with ``planning_order="prioritized"`` as the arrays the library takes: those
    of :func:`model_arrays` and, from the 7-key dict, ``pred_head`` (int32 ``[runs, S]``) and ``pred_next`` (int32
    ``[runs, S, A]``).  The 5-key dict of a Dyna-Q population gives the five arrays alone (the library then rebuilds the
    lists in their canonical order); ``ValueError`` on anything else.  Whether the lists fit the model is the library's
    check."""
    if isinstance(model, dict) and len(model) == 5:
        return model_arrays(model, runs, state_size, action_size)
    return _spec_arrays("planning_model", model, _sweep_model_specs(runs, state_size, action_size), exact=True)


def outcome_model_arrays(model, runs, state_size, action_size, model_outcomes) -> tuple | None:
    """A ``planning_model`` of a population with ``model_outcomes=K > 1`` as the arrays the library takes: from the 6-key
    dict, ``next_states`` (int32), ``rewards`` (float32), ``terminated`` (uint8) and ``outcome_counts`` (uint32: integers
    in ``[0, 2^32)``), each ``[runs, S, A, K]``, then ``visited`` and ``count`` as in :func:`model_arrays`.  The 5-key dict
    of a last-outcome population gives the five arrays of :func:`model_arrays` alone (the library then loads every
    outcome as slot 0 with count 1); ``ValueError`` on anything else.  Whether slots, list and counts agree is the
    library's check."""
    if isinstance(model, dict) and len(model) == 5:
        return model_arrays(model, runs, state_size, action_size)
    specs = _outcome_model_specs(runs, state_size, action_size, model_outcomes)
    if not isinstance(model, dict) or sorted(model) != sorted(key for key, *_ in specs):
        return _spec_arrays("planning_model", model, specs, exact=True)  # (None, or the error that lists the keys)
    # the counts fill uint32, which the exact check of the int32 arrays would refuse: they are checked on their own
    (counts,) = _spec_arrays("planning_model", {"outcome_counts": model["outcome_counts"]}, specs[3:4])
    given = np.asarray(model["outcome_counts"])
    if given.size and (given.min() < 0 or given.max() >= 2 ** 32):
        msg = f"planning_model['outcome_counts']: expected shape {specs[3][1]} of uint32, got values outside [0, 2^32)"
        raise ValueError(msg)
    rest = _spec_arrays("planning_model", {key: value for key, value in model.items() if key != "outcome_counts"},
                        specs[:3] + specs[4:], exact=True)
    return (*rest[:3], counts, *rest[3:])


def queue_arrays(queue, runs, queue_length) -> tuple | None:
    """``sweep_queue`` of a state dict as the ``(cells, priorities)`` arrays the library takes (None: every queue empty):
    int32 ``[runs, queue_length]`` and float64 ``[runs, queue_length]``; ``ValueError`` on anything else."""
    return _spec_arrays("sweep_queue", queue, _queue_specs(runs, queue_length), exact=True)


def visit_count_array(counts, runs, state_size, action_size) -> np.ndarray | None:
    """``visit_counts`` as the uint32 ``[runs, S, A]`` array the library takes (None: every count zero): integers in
    ``[0, 2^32)`` of exactly that shape; ``ValueError`` on anything else."""
    if counts is None:
        return None
    arr = np.asarray(counts)
    shape = (runs, state_size, action_size)
    if arr.shape != shape or arr.dtype.kind not in "iu":
        msg = f"visit_counts: expected shape {shape} of uint32, got shape {arr.shape} of {arr.dtype}"
        raise ValueError(msg)
    if arr.size and (arr.min() < 0 or arr.max() >= 2 ** 32):
        msg = f"visit_counts: expected shape {shape} of uint32, got values outside [0, 2^32)"
        raise ValueError(msg)
    return np.ascontiguousarray(arr, dtype=np.uint32)


# The per-run state a training call hands to the next one through the state dict: the dict's key, which is also the
# population's property, and whether a population carries it.  (The planning model is knowledge, not such state.)
_CARRIED = {"pending_actions": lambda pop: pop.update_rule == "sarsa", "n_step_window": lambda pop: pop.n_step > 1,
            "eligibility_traces": lambda pop: pop.trace_decay is not None,
            "tree_backup_window": lambda pop: pop.tree_backup > 1,
            "sweep_queue": lambda pop: pop.planning_order == "prioritized"}


def _check_int(name, value, lo, hi) -> None:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        msg = f"{name} must be an integer in {lo} .. {hi}, got {value!r}"
        raise ValueError(msg)


def _per_run(value, runs, what):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != runs:
            msg = f"{what}: expected one entry per run ({runs}), got {len(value)}"
            raise ValueError(msg)
        return list(value)
    return [value] * runs


class QLearningPopulation:
    """``runs`` independent single-agent Q-learners over ``state_size`` x ``action_size`` (at most 64 actions).

    ``discount_factor``, ``lr_schedule`` and ``exploration_rate_schedule`` take one value / schedule for every run or a
    sequence of ``runs``; ``update_rule`` ("q_learning", "sarsa" or "expected_sarsa"), ``double_q`` (two tables per
    run, Q-learning only), ``n_step`` (1 .. 16, above 1 for the two on-policy rules only) and ``tree_backup`` (1 .. 16,
    above 1 for "q_learning" alone, without any switch below: n-step Tree Backup) hold for all of them.
    ``trace_decay`` (None: no traces; else one lambda in [0, 1] or a sequence of ``runs``) turns on eligibility traces for
    "sarsa" and "q_learning", with ``trace_length`` slots per run (1 .. 32) of ``trace_kind`` "replacing" or
    "accumulating".  ``planning_steps`` (0: none; 1 .. 64) turns on Dyna-Q for "q_learning": that many planning updates
    from the run's learned model after every step (:attr:`planning_model`).  ``planning_order`` is "uniform" (the default:
    the updates replay cells drawn uniformly from the seen ones) or "prioritized" (prioritized sweeping: the updates go to
    the cells whose value is about to change, taken from a queue of ``queue_length`` slots per run, 1 .. 32, that the
    predecessors of every changed state enter when their increment would exceed ``sweep_threshold`` -- one finite number
    >= 0 or a sequence of ``runs``; :attr:`sweep_queue`); it needs ``planning_steps >= 1``.  ``model_outcomes`` (1 .. 8, default 1: the
    last-outcome model) is the number of distinct outcomes the planning model keeps per cell; above 1 it needs
    ``planning_steps >= 1`` and the uniform order.  ``exploration_bonus`` (None: none; else one
    finite beta >= 0 or a sequence of ``runs``) adds ``beta / sqrt(N(s, a))`` to the row the pick sees and ``visit_lr=True``
    divides the learning rate by ``N(s, a)``; either turns on the visit counts (:attr:`visit_counts`), for "q_learning"
    without ``double_q``, ``n_step``, ``trace_decay`` or ``planning_steps``.  Schedules are ``ConstantSchedule``, ``LinearSchedule`` or ``ExponentialSchedule``; after each
    call they are left advanced (``set_value``), as :class:`GpuRolloutQLearning` leaves them."""

    def __init__(self, runs, state_size, action_size, discount_factor=0.97, lr_schedule=None,
                 exploration_rate_schedule=None, seed=0, dtype=np.float64, learn_mode="iter", device=0,
                 update_rule="q_learning", double_q=False, n_step=1, trace_decay=None, trace_length=16,
                 trace_kind="replacing", planning_steps=0, exploration_bonus=None, visit_lr=False, tree_backup=1,
                 planning_order="uniform", sweep_threshold=0.0, queue_length=16, model_outcomes=1):
        self.runs = int(runs)
        self.state_size = int(state_size)
        self.action_size = int(action_size)
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            msg = "dtype must be float32 or float64"
            raise ValueError(msg)
        if learn_mode not in ("iter", "vec"):
            msg = "learn_mode must be 'iter' (reference `learn`, sequential) or 'vec' (`learn_vec`)"
            raise ValueError(msg)
        if self.runs <= 0:
            msg = "runs must be positive"
            raise ValueError(msg)
        if update_rule not in _lib.UPDATE_RULES:
            msg = f"update_rule must be one of {', '.join(map(repr, _lib.UPDATE_RULES))}, got {update_rule!r}"
            raise ValueError(msg)
        if double_q and update_rule != "q_learning":
            msg = f"double_q=True is Double Q-learning: it needs update_rule='q_learning', got {update_rule!r}"
            raise ValueError(msg)
        _check_int("n_step", n_step, 1, _lib.N_STEP_MAX)
        if n_step > 1 and double_q:
            msg = f"n_step={n_step} with double_q=True: the double estimator is a one-step method"
            raise ValueError(msg)
        if n_step > 1 and update_rule == "q_learning":
            msg = (f"n_step={n_step} needs update_rule='sarsa' or 'expected_sarsa': an uncorrected n-step Q-learning is not an "
                   "off-policy method (Q-learning's n-step form is tree_backup=n)")
            raise ValueError(msg)
        _check_int("tree_backup", tree_backup, 1, _lib.TREE_BACKUP_MAX)
        if tree_backup > 1:
            what = f"tree_backup={tree_backup}"
            if update_rule != "q_learning":
                msg = (f"{what} needs update_rule='q_learning', got {update_rule!r}: Tree Backup under a greedy target policy "
                       "is Q-learning's n-step form; the on-policy rules have n_step")
                raise ValueError(msg)
            if double_q:
                msg = f"{what} with double_q=True: the double estimator is a one-step method"
                raise ValueError(msg)
            if n_step > 1:
                msg = f"{what} with n_step={n_step}: one multi-step method at a time"
                raise ValueError(msg)
            if trace_decay is not None:
                msg = f"{what} with trace_decay: one multi-step method at a time"
                raise ValueError(msg)
            if isinstance(planning_steps, (int, np.integer)) and not isinstance(planning_steps, (bool, np.bool_)) and planning_steps > 0:
                msg = f"{what} with planning_steps={planning_steps}: Dyna-Q is a one-step method"
                raise ValueError(msg)
            if exploration_bonus is not None or (isinstance(visit_lr, (bool, np.bool_)) and visit_lr):
                msg = f"{what} with exploration_bonus or visit_lr: visit counts are built for the one-step rule"
                raise ValueError(msg)
        _check_int("planning_steps", planning_steps, 0, _lib.PLANNING_MAX)
        if planning_steps > 0:
            if update_rule != "q_learning":
                msg = (f"planning_steps={planning_steps} needs update_rule='q_learning', got {update_rule!r}: Dyna-Q replays "
                       "remembered transitions through Q-learning's update; planning for the on-policy rules is not built")
                raise ValueError(msg)
            if double_q:
                msg = f"planning_steps={planning_steps} with double_q=True: Dyna-Q plans on one table"
                raise ValueError(msg)
            if n_step > 1:
                msg = f"planning_steps={planning_steps} with n_step={n_step}: Dyna-Q is a one-step method"
                raise ValueError(msg)
            if trace_decay is not None:
                msg = f"planning_steps={planning_steps} with trace_decay: Dyna-Q is a one-step method"
                raise ValueError(msg)
            if self.state_size * self.action_size >= 2 ** 31:
                msg = f"planning_steps={planning_steps}: state_size * action_size must be below 2^31"
                raise ValueError(msg)
        if not isinstance(planning_order, str) or planning_order not in _lib.PLANNING_ORDERS:
            msg = f"planning_order must be one of {', '.join(map(repr, _lib.PLANNING_ORDERS))}, got {planning_order!r}"
            raise ValueError(msg)
        self.sweep_threshold = None
        self.queue_length = 0
        if planning_order == "prioritized":
            if planning_steps < 1:
                msg = "planning_order='prioritized' orders the planning updates: it needs planning_steps >= 1"
                raise ValueError(msg)
            _check_int("queue_length", queue_length, 1, _lib.QUEUE_MAX)
            try:
                theta = np.ascontiguousarray(_per_run(sweep_threshold, self.runs, "sweep_threshold"), dtype=np.float64)
            except (TypeError, ValueError) as err:
                if "one entry per run" in str(err):
                    raise
                msg = f"sweep_threshold must be a finite number >= 0 or a sequence of {self.runs}, got {sweep_threshold!r}"
                raise ValueError(msg) from err
            if (theta.shape != (self.runs,) or isinstance(sweep_threshold, (bool, np.bool_))
                    or not (np.isfinite(theta) & (theta >= 0)).all()):
                msg = f"sweep_threshold: every threshold must be a finite number >= 0, got {sweep_threshold!r}"
                raise ValueError(msg)
            if not _lib.sweep_build_shipped(self.dtype, self.action_size):
                msg = (f"prioritized sweeping: the kernel for {self.dtype} rows of {self.action_size} actions is not built (it "
                       "does not fit the register file)")
                raise ValueError(msg)
            self.sweep_threshold = theta
            self.queue_length = int(queue_length)
        self.planning_order = planning_order
        _check_int("model_outcomes", model_outcomes, 1, _lib.MODEL_OUTCOMES_MAX)
        if model_outcomes > 1:
            if planning_steps < 1:
                msg = f"model_outcomes={model_outcomes} sizes the planning model: it needs planning_steps >= 1"
                raise ValueError(msg)
            if planning_order == "prioritized":
                msg = (f"model_outcomes={model_outcomes} with planning_order='prioritized': sweeping over a sample model needs "
                       "expected updates, which are not built")
                raise ValueError(msg)
            if not _lib.dyna_sample_build_shipped(self.dtype, self.action_size):
                msg = (f"model_outcomes={model_outcomes}: the kernel for {self.dtype} rows of {self.action_size} actions is not "
                       "built (it does not fit the register file)")
                raise ValueError(msg)
        self.model_outcomes = int(model_outcomes)
        if not isinstance(visit_lr, (bool, np.bool_)):
            msg = f"visit_lr must be a bool, got {visit_lr!r}"
            raise ValueError(msg)
        self.exploration_bonus = None
        self.visit_lr = bool(visit_lr)
        if exploration_bonus is not None or self.visit_lr:
            what = "exploration_bonus" if exploration_bonus is not None else "visit_lr"
            if update_rule != "q_learning":
                msg = (f"{what} needs update_rule='q_learning', got {update_rule!r}: the bonus changes the behaviour policy "
                       "only; the on-policy rules under a bonus policy are not built")
                raise ValueError(msg)
            if double_q:
                msg = f"{what} with double_q=True: visit counts are built for the one-table Q-learning step"
                raise ValueError(msg)
            if n_step > 1:
                msg = f"{what} with n_step={n_step}: visit counts are built for the one-step rule"
                raise ValueError(msg)
            if trace_decay is not None:
                msg = f"{what} with trace_decay: visit counts are built for the one-step rule"
                raise ValueError(msg)
            if planning_steps > 0:
                msg = f"{what} with planning_steps={planning_steps}: visit counts are built for the step without planning"
                raise ValueError(msg)
            per_run = _per_run(0.0 if exploration_bonus is None else exploration_bonus, self.runs, "exploration_bonus")
            try:
                beta = np.ascontiguousarray(per_run, dtype=np.float64)
            except (TypeError, ValueError) as err:
                msg = f"exploration_bonus must be None, a finite number >= 0 or a sequence of {self.runs}, got {exploration_bonus!r}"
                raise ValueError(msg) from err
            if beta.shape != (self.runs,) or not (np.isfinite(beta) & (beta >= 0)).all():
                msg = f"exploration_bonus: every beta must be a finite number >= 0, got {exploration_bonus!r}"
                raise ValueError(msg)
            if not _lib.visit_build_shipped(self.dtype, self.action_size):
                msg = (f"visit counts: the kernel for {self.dtype} rows of {self.action_size} actions is not built (it does not "
                       "fit the register file)")
                raise ValueError(msg)
            self.exploration_bonus = beta
        self.planning_steps = int(planning_steps)
        self.update_rule = update_rule
        self.double_q = bool(double_q)
        self.n_step = int(n_step)
        self.tree_backup = int(tree_backup)
        self.learn_mode = learn_mode
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.discount_factor = np.ascontiguousarray(_per_run(discount_factor, self.runs, "discount_factor"), dtype=np.float64)
        self.trace_decay = None
        self.trace_length = 0
        self.trace_kind = None
        if trace_decay is not None:
            if update_rule == "expected_sarsa":
                msg = ("trace_decay with update_rule='expected_sarsa': its trace form needs policy-probability weighting, which "
                       "is not built; the trace rules are 'sarsa' and 'q_learning'")
                raise ValueError(msg)
            if double_q:
                msg = "trace_decay with double_q=True: the double estimator has no trace form"
                raise ValueError(msg)
            if n_step > 1:
                msg = f"trace_decay with n_step={n_step}: one multi-step method at a time"
                raise ValueError(msg)
            _check_int("trace_length", trace_length, 1, _lib.TRACE_MAX)
            if trace_kind not in _lib.TRACE_KINDS:
                msg = f"trace_kind must be one of {', '.join(map(repr, _lib.TRACE_KINDS))}, got {trace_kind!r}"
                raise ValueError(msg)
            try:
                lam = np.ascontiguousarray(_per_run(trace_decay, self.runs, "trace_decay"), dtype=np.float64)
            except (TypeError, ValueError) as err:
                if "one entry per run" in str(err):
                    raise
                msg = f"trace_decay must be None, a number in [0, 1] or a sequence of {self.runs}, got {trace_decay!r}"
                raise ValueError(msg) from err
            if lam.shape != (self.runs,) or not ((lam >= 0) & (lam <= 1)).all():
                msg = f"trace_decay: every lambda must be a finite number in [0, 1], got {trace_decay!r}"
                raise ValueError(msg)
            with np.errstate(all="ignore"):
                decay = (self.discount_factor * lam).astype(self.dtype)  # what the kernel multiplies the traces by
            if not ((decay >= 0) & (decay <= 1)).all():
                r = int(np.flatnonzero(~((decay >= 0) & (decay <= 1)))[0])
                msg = (f"trace_decay: run {r}'s decay factor discount_factor * trace_decay = {self.discount_factor[r]!r} * "
                       f"{lam[r]!r} is outside [0, 1]")
                raise ValueError(msg)
            self.trace_decay = lam
            self.trace_length = int(trace_length)
            self.trace_kind = trace_kind
        lr_schedule = ConstantSchedule(0.1) if lr_schedule is None else lr_schedule
        exploration_rate_schedule = ConstantSchedule(0.1) if exploration_rate_schedule is None else exploration_rate_schedule
        self.lr_schedules = _per_run(lr_schedule, self.runs, "lr_schedule")
        self.exploration_rate_schedules = _per_run(exploration_rate_schedule, self.runs, "exploration_rate_schedule")
        for s in self.lr_schedules + self.exploration_rate_schedules:
            schedule_descriptor(s)  # TypeError before anything is allocated
        self.last_stats = None
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self._dtype_code = _lib.QE_F32 if self.dtype == np.float32 else _lib.QE_F64
        _lib.check(self._lib.qe_create_population(C.byref(self._h), self.runs, self.state_size, self.action_size, self.seed,
                                                  self._dtype_code, int(device)))
        _lib.check(self._lib.qe_population_configure(self._h, None, None, _lib.ptr(self.discount_factor, C.c_double)))
        if update_rule != "q_learning":
            _lib.check(self._lib.qe_population_set_update_rule(self._h, _lib.UPDATE_RULES[update_rule]))
        if self.double_q:
            _lib.check(self._lib.qe_population_set_double(self._h, 1))
        if self.n_step > 1:
            _lib.check(self._lib.qe_population_set_n_step(self._h, self.n_step))
        if self.tree_backup > 1:
            _lib.check(self._lib.qe_population_set_tree_backup(self._h, self.tree_backup))
        if self.trace_decay is not None:
            _lib.check(self._lib.qe_population_set_traces(self._h, self.trace_length, _lib.TRACE_KINDS[self.trace_kind],
                                                          _lib.ptr(self.trace_decay, C.c_double)))
        if self.planning_steps:
            _lib.check(self._lib.qe_population_set_planning(self._h, self.planning_steps))
        if self.model_outcomes > 1:
            _lib.check(self._lib.qe_population_set_model_outcomes(self._h, self.model_outcomes))
        if self.planning_order == "prioritized":
            _lib.check(self._lib.qe_population_set_sweeping(self._h, self.queue_length, _lib.ptr(self.sweep_threshold, C.c_double)))
        if self.counting:
            _lib.check(self._lib.qe_population_set_visits(self._h, _lib.ptr(self.exploration_bonus, C.c_double),
                                                         1 if self.visit_lr else 0))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.qe_destroy(h)
            self._h = C.c_void_p()

    @property
    def handle(self):
        """The population's ``qe_engine*`` (environments bind to it)."""
        return self._h

    @property
    def step_counter(self) -> int:
        """Index of the next step in the draw protocol while all runs agree on it (``ValueError`` once an
        episode-based evaluation has left them apart: see :attr:`step_counters`).  Setting it sets every run's."""
        counters = self._counters()
        if (counters != counters[0]).any():
            msg = "the runs' draw counters differ (after evaluate_episodes): use step_counters"
            raise ValueError(msg)
        return int(counters[0])

    @step_counter.setter
    def step_counter(self, value: int) -> None:
        _lib.check(self._lib.qe_set_step_counter(self._h, int(value) & 0xFFFFFFFFFFFFFFFF))

    @property
    def step_counters(self) -> np.ndarray:
        """Every run's index of its next step in the draw protocol, int64 ``[runs]`` (the uint64 counters' bits)."""
        return self._counters().view(np.int64)

    @step_counters.setter
    def step_counters(self, values) -> None:
        arr = np.asarray(values)
        if arr.shape != (self.runs,):
            msg = f"step_counters: expected {self.runs} entries, got shape {arr.shape}"
            raise ValueError(msg)
        arr = np.ascontiguousarray(arr.astype(np.uint64) if arr.dtype.kind == "u" else arr.astype(np.int64).view(np.uint64))
        _lib.check(self._lib.qe_population_set_step_counters(self._h, _lib.ptr(arr, C.c_uint64)))

    def _counters(self) -> np.ndarray:
        out = np.empty(self.runs, dtype=np.uint64)
        _lib.check(self._lib.qe_population_step_counters(self._h, _lib.ptr(out, C.c_uint64)))
        return out

    @property
    def pending_actions(self) -> np.ndarray:
        """SARSA: the action each run has already chosen for its next training step, int32 ``[runs]``, -1 = none (the
        run picks at that step).  Other rules: all -1."""
        out = np.empty(self.runs, dtype=np.int32)
        _lib.check(self._lib.qe_population_pending_actions(self._h, _lib.ptr(out, C.c_int32)))
        return out

    @pending_actions.setter
    def pending_actions(self, values) -> None:
        _lib.check(self._lib.qe_population_set_pending_actions(self._h, _lib.ptr(pending_array(values, self.runs), C.c_int32)))

    def _state_dict_of(self, getter, specs) -> dict:
        """Fresh arrays as ``specs`` describes them, filled by the library's ``getter``."""
        out = {key: np.empty(shape, dtype=dtype) for key, shape, _, dtype in specs}
        _lib.check(getter(self._h, *(_lib.ptr(arr, _CTYPES[arr.dtype]) for arr in out.values())))
        return out

    def _set_state(self, setter, arrays, count) -> None:
        """What a ``*_arrays`` function returned (None: ``count`` NULLs, the empty state) through the library's ``setter``."""
        _lib.check(setter(self._h, *([None] * count if arrays is None else [_lib.ptr(arr, _CTYPES[arr.dtype]) for arr in arrays])))

    @property
    def n_step_window(self) -> dict | None:
        """``n_step > 1``: every run's window of transitions not yet updated, a dict of ``length`` (int32 ``[runs]``),
        ``states``, ``actions`` (int32 ``[runs, n_step - 1]``) and ``rewards`` (float32 ``[runs, n_step - 1]``); rows are
        oldest first and unused slots hold 0.  ``n_step == 1``: None.  Setting None empties every window."""
        if self.n_step == 1:
            return None
        return self._state_dict_of(self._lib.qe_population_window, _window_specs(self.runs, self.n_step))

    @n_step_window.setter
    def n_step_window(self, window) -> None:
        if self.n_step == 1:
            if window is not None:
                msg = "a population with n_step=1 has no window"
                raise ValueError(msg)
            return
        self._set_state(self._lib.qe_population_set_window, window_arrays(window, self.runs, self.n_step), 4)

    @property
    def tree_backup_window(self) -> dict | None:
        """``tree_backup > 1``: every run's window of entries not yet updated, a dict of ``length`` (int32 ``[runs]``),
        ``states``, ``actions`` (int32 ``[runs, tree_backup - 1]``), ``rewards`` (float32) and ``greedy`` (uint8: 1 where
        the action was a greedy one when it was taken); rows are oldest first and unused slots hold 0.
        ``tree_backup == 1``: None.  Setting None empties every window."""
        if self.tree_backup == 1:
            return None
        return self._state_dict_of(self._lib.qe_population_tree_window, _tree_specs(self.runs, self.tree_backup))

    @tree_backup_window.setter
    def tree_backup_window(self, window) -> None:
        if self.tree_backup == 1:
            if window is not None:
                msg = "a population with tree_backup=1 has no window"
                raise ValueError(msg)
            return
        self._set_state(self._lib.qe_population_set_tree_window, tree_window_arrays(window, self.runs, self.tree_backup), 5)

    @property
    def eligibility_traces(self) -> dict | None:
        """``trace_decay`` set: every run's trace slots, a dict of ``states``, ``actions`` (int32 ``[runs, trace_length]``)
        and ``values`` (float64 ``[runs, trace_length]``, exact for either dtype), in slot order; free slots read
        ``(0, 0, 0.0)``.  Without traces: None.  Setting None frees every slot."""
        if self.trace_decay is None:
            return None
        return self._state_dict_of(self._lib.qe_population_traces, _trace_specs(self.runs, self.trace_length))

    @eligibility_traces.setter
    def eligibility_traces(self, traces) -> None:
        if self.trace_decay is None:
            if traces is not None:
                msg = "a population without trace_decay has no eligibility traces"
                raise ValueError(msg)
            return
        self._set_state(self._lib.qe_population_set_trace_state, trace_arrays(traces, self.runs, self.trace_length), 3)

    @property
    def planning_model(self) -> dict | None:
        """``planning_steps > 0``: what every run has learned about its environment, a dict of ``next_states`` (int32
        ``[runs, S, A]``, -1: unseen), ``rewards`` (float32, 0 where unseen), ``terminated`` (bool) -- the last observed
        outcome of every cell --, ``visited`` (int32 ``[runs, S * A]``: the seen cells ``s * A + a`` in order of first
        observation, -1 past the count) and ``count`` (int32 ``[runs]``).  Without planning: None.  Setting None forgets
        everything; a dict whose list names an unseen, repeated or out-of-range cell, or whose count differs from the
        number of seen cells, is a ``ValueError``.

        ``planning_order="prioritized"`` adds the predecessor lists the kernel walks: ``pred_head`` (int32 ``[runs, S]``:
        the cell ``s * A + a`` at the head of each state's list, -1 for an empty list) and ``pred_next`` (int32
        ``[runs, S, A]``: the next cell of the same list; -1 at the tail and at a cell that is not linked).  The list of a
        state holds the seen cells that lead to it without ending the episode, most recently linked first.  The setter
        takes the 7-key dict -- lists that do not fit the model (a node that is out of range, unseen, terminated, of
        another next state or reached twice, a seen cell left out, an unlinked cell not at -1) are a ``ValueError`` and
        change nothing -- or the 5-key dict of a Dyna-Q population, whose lists are rebuilt in the canonical order: the seen
        cells that are not terminated linked in visited-list order, each at the head of its next state's list.  Setting
        or forgetting the model empties every run's :attr:`sweep_queue`.

        ``model_outcomes=K > 1`` keeps up to ``K`` outcomes per cell: ``next_states``, ``rewards`` and ``terminated`` have
        the shape ``[runs, S, A, K]`` and ``outcome_counts`` (uint32, the same shape) says how often each was observed; the
        occupied slots of a cell come first, in order of first observation, and a free slot reads -1, 0.0, False, 0.
        The setter takes that 6-key dict -- an occupied slot behind a free one or with count 0, a free slot with a count,
        two slots of a cell holding the same outcome, or counts of a cell adding up to more than ``2^32 - 1`` are a
        ``ValueError`` and change nothing -- or the 5-key dict of a last-outcome population, whose outcomes load as
        slot 0 with count 1."""
        if not self.planning_steps:
            return None
        if self.model_outcomes > 1:
            specs = _outcome_model_specs(self.runs, self.state_size, self.action_size, self.model_outcomes)
            model = self._state_dict_of(self._lib.qe_population_outcome_model, specs)
            model["terminated"] = model["terminated"].astype(bool)
            return model
        model = self._state_dict_of(self._lib.qe_population_model, _model_specs(self.runs, self.state_size, self.action_size))
        model["terminated"] = model["terminated"].astype(bool)
        if self.planning_order == "prioritized":
            specs = _sweep_model_specs(self.runs, self.state_size, self.action_size)[5:]
            model.update(self._state_dict_of(self._lib.qe_population_predecessors, specs))
        return model

    @planning_model.setter
    def planning_model(self, model) -> None:
        if not self.planning_steps:
            if model is not None:
                msg = "a population without planning_steps has no planning model"
                raise ValueError(msg)
            return
        if self.model_outcomes > 1:
            arrays = outcome_model_arrays(model, self.runs, self.state_size, self.action_size, self.model_outcomes)
            if arrays is not None and len(arrays) == 5:  # a last-outcome model: the library loads it as slot 0, count 1
                self._set_state(self._lib.qe_population_set_model, arrays, 5)
            else:
                self._set_state(self._lib.qe_population_set_outcome_model, arrays, 6)
            return
        if self.planning_order != "prioritized":
            self._set_state(self._lib.qe_population_set_model, model_arrays(model, self.runs, self.state_size, self.action_size), 5)
            return
        arrays = sweep_model_arrays(model, self.runs, self.state_size, self.action_size)
        if arrays is None or len(arrays) == 5:  # forgotten, or a Dyna-Q model: the library rebuilds the canonical lists
            self._set_state(self._lib.qe_population_set_model, arrays, 5)
            return
        before = self.planning_model
        self._set_state(self._lib.qe_population_set_model, arrays[:5], 5)
        try:
            self._set_state(self._lib.qe_population_set_predecessors, arrays[5:], 2)
        except Exception:  # the lists do not fit the model: a refused model changes nothing
            self.planning_model = before
            raise

    @property
    def sweep_queue(self) -> dict | None:
        """``planning_order="prioritized"``: every run's priority queue, a dict of ``cells`` (int32 ``[runs,
        queue_length]``: the cell ``s * A + a`` a slot holds, -1 for a free slot) and ``priorities`` (float64, 0.0 in a
        free slot), in slot order.  Run state, carried like :attr:`eligibility_traces`.  Otherwise: None.  Setting None
        empties every queue; a cell that is out of range, unseen in the model or held twice, a priority that is NaN or
        negative, or a free slot with a priority other than 0 is a ``ValueError``."""
        if self.planning_order != "prioritized":
            return None
        return self._state_dict_of(self._lib.qe_population_queue, _queue_specs(self.runs, self.queue_length))

    @sweep_queue.setter
    def sweep_queue(self, queue) -> None:
        if self.planning_order != "prioritized":
            if queue is not None:
                msg = "a population without planning_order='prioritized' has no sweep queue"
                raise ValueError(msg)
            return
        self._set_state(self._lib.qe_population_set_queue, queue_arrays(queue, self.runs, self.queue_length), 2)

    @property
    def counting(self) -> bool:
        """Whether the population keeps visit counts (``exploration_bonus is not None or visit_lr``)."""
        return self.exploration_bonus is not None

    @property
    def visit_counts(self) -> np.ndarray | None:
        """Counting on: ``N(s, a)`` of every run, uint32 ``[runs, S, A]`` -- how often the run has taken the action in
        the state during training, saturating at ``2^32 - 1``.  Off: None.  Setting None forgets everything; anything but
        integers in ``[0, 2^32)`` of that shape is a ``ValueError``."""
        if not self.counting:
            return None
        out = np.empty((self.runs, self.state_size, self.action_size), dtype=np.uint32)
        _lib.check(self._lib.qe_population_visit_counts(self._h, _lib.ptr(out, C.c_uint32)))
        return out

    @visit_counts.setter
    def visit_counts(self, counts) -> None:
        if not self.counting:
            if counts is not None:
                msg = "a population without exploration_bonus or visit_lr has no visit counts"
                raise ValueError(msg)
            return
        arr = visit_count_array(counts, self.runs, self.state_size, self.action_size)
        _lib.check(self._lib.qe_population_set_visit_counts(self._h, _lib.ptr(arr, C.c_uint32)))

    @property
    def visit_bonus(self) -> np.ndarray | None:
        """Counting on: the bonus the next pick adds to every cell, table dtype ``[runs, S, A]``: 0 where the run's beta
        is 0, else ``dtype(beta / sqrt(float64(N)))`` (``+inf`` at an untried cell).  Off: None."""
        if not self.counting:
            return None
        out = np.empty((self.runs, self.state_size, self.action_size), dtype=self.dtype)
        _lib.check(self._lib.qe_population_visit_bonus(self._h, out.ctypes.data, self._dtype_code))
        return out

    def save_model(self, filename) -> None:
        """:attr:`planning_model` as one ``.npz`` (``ValueError`` without planning)."""
        model = self.planning_model
        if model is None:
            msg = "a population without planning_steps has no planning model"
            raise ValueError(msg)
        with open(filename, "wb") as f:  # (an open file: np.savez appends ".npz" to a name that lacks it)
            np.savez(f, **model)

    def load_model(self, filename) -> None:
        """What :meth:`save_model` wrote."""
        with np.load(filename) as z:
            self.planning_model = {key: z[key] for key in z.files}

    def _rng_step(self):
        """``state_dict["rng_step"]``: an int while all runs agree, else the int64 array of every run's."""
        counters = self._counters()
        return int(counters[0]) if (counters == counters[0]).all() else counters.view(np.int64)

    # ------------------------------------------------------------------ tables
    def _need_double(self) -> None:
        if not self.double_q:
            msg = "a population without double_q has no second table"
            raise ValueError(msg)

    def _download(self, second, r=None) -> np.ndarray:
        """All tables A (``second``: B, which needs ``double_q``), or with ``r`` run ``r``'s."""
        if second:
            self._need_double()
        if r is None:
            host = np.empty((self.runs, self.state_size, self.action_size), dtype=self.dtype)
            download = self._lib.qe_population_table_b_download if second else self._lib.qe_table_download
            _lib.check(download(self._h, host.ctypes.data, self._dtype_code))
            return host
        r = int(r)
        if not 0 <= r < self.runs:
            msg = f"run {r} out of range [0, {self.runs})"
            raise IndexError(msg)
        host = np.empty((self.state_size, self.action_size), dtype=self.dtype)
        download = self._lib.qe_population_table_b_download_rows if second else self._lib.qe_table_download_rows
        _lib.check(download(self._h, host.ctypes.data, r * self.state_size, self.state_size))
        return host

    @property
    def q_tables(self) -> np.ndarray:
        """All tables, ``(runs, state_size, action_size)`` (``double_q``: the tables A)."""
        return self._download(False)

    @property
    def q_tables_b(self) -> np.ndarray:
        """``double_q``: all tables B, ``(runs, state_size, action_size)``."""
        return self._download(True)

    def q_table_b(self, r: int) -> np.ndarray:
        """``double_q``: run ``r``'s table B, ``(state_size, action_size)``."""
        return self._download(True, r)

    def q_table(self, r: int) -> np.ndarray:
        """Run ``r``'s table, ``(state_size, action_size)``."""
        return self._download(False, r)

    def _upload_form(self, tables):
        arr = np.asarray(tables)
        one = (self.state_size, self.action_size)
        if arr.shape == one:
            arr = np.broadcast_to(arr, (self.runs, *one))
        elif arr.shape != (self.runs, *one):
            msg = f"tables must have shape {one} or {(self.runs, *one)}, got {arr.shape}"
            raise ValueError(msg)
        up = np.float32 if arr.dtype == np.float32 else np.float64
        return np.ascontiguousarray(arr, dtype=up), _lib.QE_F32 if up == np.float32 else _lib.QE_F64

    def set_q_tables(self, tables, tables_b=None) -> None:
        """``(state_size, action_size)`` (every run starts from it) or ``(runs, state_size, action_size)``.
        ``double_q``: ``tables`` are the tables A, ``tables_b`` (same shapes) the tables B; None leaves B as it is."""
        if tables_b is not None:
            self._need_double()
        arr, code = self._upload_form(tables)
        arr_b, code_b = (None, None) if tables_b is None else self._upload_form(tables_b)  # (both checked before either is sent)
        _lib.check(self._lib.qe_table_upload(self._h, arr.ctypes.data, code))
        if arr_b is not None:
            _lib.check(self._lib.qe_population_table_b_upload(self._h, arr_b.ctypes.data, code_b))

    def save(self, filename) -> None:
        """The ``(runs, state_size, action_size)`` tables as one ``.npy``; ``double_q``: ``(2, runs, state_size,
        action_size)``, A then B."""
        np.save(filename, np.stack([self.q_tables, self.q_tables_b]) if self.double_q else self.q_tables)

    def load(self, filename) -> None:
        """What :meth:`save` wrote (``double_q``: that four-dimensional shape and no other)."""
        arr = np.load(filename)
        if not self.double_q:
            self.set_q_tables(arr)
            return
        want = (2, self.runs, self.state_size, self.action_size)
        if arr.shape != want:
            msg = f"a double_q population loads tables of shape {want}, got {arr.shape}"
            raise ValueError(msg)
        self.set_q_tables(arr[0], arr[1])

    # ------------------------------------------------------------------ training
    def _descriptors(self, schedules):
        # (one descriptor per distinct schedule object: a schedule shared by 65 536 runs is encoded once)
        rows = np.zeros(self.runs, dtype=_DESCRIPTOR)
        seen = {}
        for r, s in enumerate(schedules):
            d = seen.get(id(s))
            if d is None:
                kind, value, lo, factor = schedule_descriptor(s)
                d = seen[id(s)] = np.array((value, lo, factor, kind, 0), dtype=_DESCRIPTOR)
            rows[r] = d
        return rows

    def _adopt_schedule_values(self):
        eps = np.empty(self.runs, dtype=np.float64)
        lr = np.empty(self.runs, dtype=np.float64)
        _lib.check(self._lib.qe_population_schedules(self._h, _lib.ptr(eps, C.c_double), _lib.ptr(lr, C.c_double)))
        self._set_schedule_values(self.exploration_rate_schedules, eps)
        self._set_schedule_values(self.lr_schedules, lr)
        return eps, lr

    @staticmethod
    def _set_schedule_values(schedules, values) -> None:
        """Every distinct schedule object takes its value from the per-run array ``values``."""
        last = {id(s): (s, r) for r, s in enumerate(schedules)}  # (a shared schedule: its runs hold the same value)
        for s, r in last.values():
            s.set_value(float(values[r]))

    def _fetch_call(self, total, st, counts, log, with_steps) -> tuple:
        """After the library's training or evaluation call returned ``total``: raises what it refused, keeps the statistics
        and fetches the episode log.  Returns ``(empty, returns, steps, offsets)``; ``empty``: some run met a state without
        a selectable action, which :meth:`_unless_empty` raises once the call's result is built."""
        empty = total == _lib.ERR_INDEX
        if total < 0 and not empty:
            _lib.check(total)
        self.last_stats = {f: getattr(st, f) for f, _ in st._fields_}
        total = int(counts.sum())
        rets = np.empty(total if log else 0, dtype=np.float32)
        at = np.empty(total if log else 0, dtype=np.int32) if with_steps else None
        if log and total:
            _lib.check(self._lib.qe_population_log(self._h, total, _lib.ptr(at, C.c_int32), _lib.ptr(rets, C.c_float)))
        offsets = np.zeros(self.runs + 1, dtype=np.int64)
        if log:
            np.cumsum(counts, out=offsets[1:])
        return empty, rets, at, offsets

    @staticmethod
    def _unless_empty(empty, status_bits, result):
        """``result``, or with ``empty`` the ``IndexError`` that names the runs with a bit set in ``status_bits`` (``.runs``)
        and carries ``result`` (``.result``)."""
        if empty:
            bad = np.flatnonzero(status_bits).tolist()
            err = IndexError(f"Cannot choose from an empty sequence (runs {', '.join(map(str, bad))})")
            err.runs = bad
            err.result = result
            raise err
        return result

    def run_steps(self, steps, env, curr_state_dict=None, log=True) -> PopulationRun:
        """``steps`` steps of every run on ``env`` (a device environment of ``num_agents == runs``).  ``curr_state_dict``
        None resets the environment, as the reference's ``run_steps``; the dict of the previous call continues it
        (SARSA: with its ``pending_actions``; after a reset, or without that key, every run picks at its first step;
        ``n_step > 1`` / ``tree_backup > 1``: with its ``n_step_window`` / ``tree_backup_window``; after a reset, or without
        that key, every window starts empty and the entries dropped are never updated; ``trace_decay``: with its ``eligibility_traces``; after a reset, or
        without that key, every slot starts free; ``planning_order="prioritized"``: with its ``sweep_queue``; after a reset, or
        without that key, every queue starts empty -- the model and its predecessor lists stay).
        ``log=False`` skips the per-episode returns (counts and means are always produced).  A run that meets a state
        without a selectable action raises ``IndexError`` naming the runs (``.runs``; ``.result`` holds the call's
        result, in which the other runs are unaffected)."""
        self._check_env(env)
        steps = int(steps)
        env.bind(self)
        if curr_state_dict is None:
            env.reset_device()
        elif not env.is_resident(curr_state_dict):
            env.restore(curr_state_dict["states"], curr_state_dict["rewards"], curr_state_dict.get("aux"))
        carried = [key for key, has in _CARRIED.items() if has(self)]
        for key in carried:
            setattr(self, key, None if curr_state_dict is None else curr_state_dict.get(key))
        eps_d = self._descriptors(self.exploration_rate_schedules)
        lr_d = self._descriptors(self.lr_schedules)
        sched_p = C.POINTER(_lib.RunSchedule)
        _lib.check(self._lib.qe_population_configure(self._h, eps_d.ctypes.data_as(sched_p), lr_d.ctypes.data_as(sched_p), None))
        M = self.runs
        counts = np.empty(M, dtype=np.int64)
        sums = np.empty(M, dtype=np.float32)
        state = np.empty(3 * M, dtype=np.uint32)  # observations | env-internal state | running returns
        status = np.empty(M, dtype=np.uint32)
        st = _lib.RolloutStats()
        mode = _lib.LEARN_ITER if self.learn_mode == "iter" else _lib.LEARN_VEC
        base = state.ctypes.data
        total = self._lib.qe_population_rollout(
            self._h, env.handle, steps, mode, 1 if log else 0, C.byref(st), _lib.ptr(counts, C.c_int64),
            _lib.ptr(sums, C.c_float), C.cast(base, C.POINTER(C.c_int32)), C.cast(base + 4 * M, C.POINTER(C.c_uint32)),
            C.cast(base + 8 * M, C.POINTER(C.c_float)), _lib.ptr(status, C.c_uint32))
        empty, rets, at, offsets = self._fetch_call(total, st, counts, log, True)
        eps_v, lr_v = self._adopt_schedule_values()
        with np.errstate(divide="ignore", invalid="ignore"):
            means = sums / counts.astype(np.float32)  # float32, as the standalone's float32 sum / len
        means[counts == 0] = np.nan
        obs, aux, rewards = state[:M].view(np.int32), state[M:2 * M], state[2 * M:].view(np.float32)
        state_dict = env.adopt_state(obs, rewards, aux)
        state_dict["rng_step"] = self._rng_step()
        state_dict["lr"] = lr_v
        state_dict["exploration_rate"] = eps_v
        for key in carried:
            state_dict[key] = getattr(self, key)
        return self._unless_empty(empty, status, PopulationRun(means, counts, rets, offsets, at, state_dict))

    def restore_training_state(self, state_dict) -> None:
        """Continue exactly where ``state_dict`` (of ``run_steps``, e.g. un-pickled in a fresh process) left off: draw
        counter(s), every run's schedule values, (SARSA) pending action, (``n_step > 1``, ``tree_backup > 1``) window, (``trace_decay``) trace slots and (``planning_order="prioritized"``) queue.  Tables: :meth:`load`; the planning
        model, which must be in place before the queue: :meth:`load_model`; environments: pass
        the dict to ``run_steps``."""
        for key, has in _CARRIED.items():
            if has(self):
                setattr(self, key, state_dict.get(key))
        rng_step = state_dict["rng_step"]
        if np.ndim(rng_step) == 0:
            self.step_counter = int(rng_step)
        else:
            self.step_counters = rng_step
        for schedules, key in ((self.lr_schedules, "lr"), (self.exploration_rate_schedules, "exploration_rate")):
            self._set_schedule_values(schedules, np.broadcast_to(np.asarray(state_dict[key], dtype=np.float64), (self.runs,)))

    # ------------------------------------------------------------------ evaluation and train
    def _check_env(self, env) -> None:
        if not isinstance(env, DeviceVecEnv):
            msg = "a population runs on a device environment (dist_classicrl_amd.environments)"
            raise TypeError(msg)
        if env.num_agents != self.runs:
            msg = f"the environment has {env.num_agents} agents, the population {self.runs} runs: one agent per run"
            raise ValueError(msg)

    def policy_values(self, env, discount_factor=None, tol=1e-12, max_sweeps=100_000) -> PolicyValues:
        """The exact value of every run's greedy policy on ``env``, a :class:`TabularMDPEnv` of ``num_agents == runs``,
        by iterative policy evaluation on the device (``qe_population_policy_values``): no sampling, no draw.  The policy
        is the one :meth:`evaluate_episodes` follows -- the maximum of the valid columns of the run's row (``double_q``:
        of A + B), ties broken uniformly -- and the law the integer one the environment samples from.  ``discount_factor``
        is a number, a sequence of ``runs``, or None for the runs' own; 1.0 gives the undiscounted return
        :meth:`evaluate_episodes` reports.  Each run stops at its first sweep with residual ``<= tol``, else at
        ``max_sweeps``.  Tables, schedules, draw counters and the environment's state are left as they are."""
        self._check_env(env)
        gammas = None
        if discount_factor is not None:
            gammas = np.ascontiguousarray(np.broadcast_to(check_discounts(
                _per_run(discount_factor, self.runs, "discount_factor")), (self.runs,)))
        tol, max_sweeps = check_solve_args(tol, max_sweeps)
        env.bind(self)  # (an environment that is not a table MDP is the library's to refuse: NotImplementedError)
        M, S = self.runs, self.state_size
        values = np.empty((M, S), dtype=np.float64)
        sweeps = np.empty(M, dtype=np.int32)
        residuals = np.empty(M, dtype=np.float64)
        status = np.empty(M, dtype=np.uint32)
        rc = self._lib.qe_population_policy_values(self._h, env.handle, _lib.ptr(gammas, C.c_double), tol, max_sweeps,
                                                   _lib.ptr(values, C.c_double), _lib.ptr(sweeps, C.c_int32),
                                                   _lib.ptr(residuals, C.c_double), _lib.ptr(status, C.c_uint32))
        _lib.check(rc)
        starts = np.array([start_value(env.mdp, values[r]) for r in range(M)], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            converged = residuals <= tol
        return PolicyValues(values, starts, sweeps, residuals, converged, status)

    def evaluate_steps(self, env, steps, log=True) -> PopulationEval:
        """Greedy evaluation: every run takes ``steps`` steps from ``env.reset(seed=42)`` with its own table, as the
        standalone one-agent ``evaluate_steps(env_r, steps)``.  Tables and schedules are untouched; every run's draw
        counter advances by ``steps``.  A run without a selectable action raises ``IndexError`` (``.runs``, ``.result``),
        as :meth:`run_steps` does."""
        self._check_env(env)
        steps = int(steps)
        if steps < 0:
            msg = "steps must be >= 0"
            raise ValueError(msg)
        return self._evaluate(env, steps, 0, log)

    def evaluate_episodes(self, env, episodes, max_steps=None, log=True) -> PopulationEval:
        """Greedy evaluation until each run has ended ``episodes`` episodes, as the standalone one-agent
        ``evaluate_episodes(env_r, episodes)``: run ``r`` stops at the end of the step in which its count is reached and
        its draw counter advances by the steps it took (``steps_used``).  The standalone loops forever on a greedy policy
        that never ends an episode; here a run also stops after ``max_steps`` steps (default ``1000 * episodes``) with
        ``finished[r]`` False."""
        self._check_env(env)
        episodes = int(episodes)
        if episodes < 0:
            msg = "episodes must be >= 0"
            raise ValueError(msg)
        max_steps = 1000 * episodes if max_steps is None else int(max_steps)
        if max_steps < 0:
            msg = "max_steps must be >= 0"
            raise ValueError(msg)
        if episodes == 0:  # the standalone's loop does not run: no step, no draw
            env.bind(self)
            env.reset_device(seed=42)
            M = self.runs
            zeros = np.zeros(M, dtype=np.int64)
            return PopulationEval(np.zeros(M, dtype=np.float32), zeros, np.empty(0, dtype=np.float32),
                                  np.zeros(M + 1, dtype=np.int64), zeros.copy(), np.ones(M, dtype=bool))
        return self._evaluate(env, max_steps, episodes, log)

    def _evaluate(self, env, steps, episodes, log) -> PopulationEval:
        env.bind(self)
        env.reset_device(seed=42)
        M = self.runs
        counts = np.empty(M, dtype=np.int64)
        sums = np.empty(M, dtype=np.float32)
        used = np.empty(M, dtype=np.int64)
        status = np.empty(M, dtype=np.uint32)
        st = _lib.RolloutStats()
        total = self._lib.qe_population_evaluate(
            self._h, env.handle, steps, episodes, 1 if log else 0, C.byref(st), _lib.ptr(counts, C.c_int64),
            _lib.ptr(sums, C.c_float), _lib.ptr(used, C.c_int64), _lib.ptr(status, C.c_uint32))
        empty, rets, _, offsets = self._fetch_call(total, st, counts, log, False)
        return self._unless_empty(empty, status & 1, PopulationEval(sums, counts, rets, offsets, used, (status & 2) == 0))

    def train(self, env, steps, val_env, val_every_n_steps, val_steps=None, val_episodes=None, curr_state_dict=None,
              max_val_steps=None) -> PopulationTraining:
        """The standalone ``train`` (base_runtime.BaseRuntime.train) for every run at once: segments of
        ``val_every_n_steps`` training steps (the last one shorter if it does not divide ``steps``), each followed by a
        greedy evaluation on ``val_env`` -- ``val_steps`` steps or ``val_episodes`` episodes (bounded by
        ``max_val_steps``, see :meth:`evaluate_episodes`).  As in the reference, every segment starts from the
        ``curr_state_dict`` passed in (None: the training environment is reset before each segment)."""
        if (val_steps is None) == (val_episodes is None):
            msg = "Exactly one of val_steps or val_episodes must be specified."
            raise ValueError(msg)
        self._check_env(env)
        self._check_env(val_env)
        segments, val_totals, val_finished = [], [], []
        state_dict = None
        for step in range(0, int(steps), int(val_every_n_steps)):
            res = self.run_steps(min(val_every_n_steps, steps - step), env, curr_state_dict)
            segments.append(res)
            state_dict = res.state_dict
            if val_steps is not None:
                ev = self.evaluate_steps(val_env, val_steps)
            else:
                ev = self.evaluate_episodes(val_env, val_episodes, max_val_steps)
            val_totals.append(ev.totals)
            val_finished.append(ev.finished)
        M = self.runs
        counts = np.zeros(M, dtype=np.int64)
        for res in segments:
            counts += res.episode_counts
        offsets = np.zeros(M + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        returns = np.empty(int(offsets[-1]), dtype=np.float32)
        at = offsets[:-1].copy()  # next free slot of each run
        for res in segments:  # each segment's returns after the run's earlier ones
            run_of = np.repeat(np.arange(M), res.episode_counts)
            returns[at[run_of] + np.arange(run_of.size) - res.offsets[run_of]] = res.returns
            at += res.episode_counts
        shape = (len(segments), M)
        return PopulationTraining(returns, offsets, np.array(val_totals, dtype=np.float32).reshape(shape),
                                  np.array(val_finished, dtype=bool).reshape(shape), segments, state_dict)


__all__ = ["PolicyValues", "PopulationEval", "PopulationRun", "PopulationTraining", "QLearningPopulation", "advance_descriptor",
           "model_arrays", "outcome_model_arrays", "pending_array", "queue_arrays", "schedule_descriptor", "sweep_model_arrays", "trace_arrays", "tree_window_arrays", "visit_count_array",
           "window_arrays"]
