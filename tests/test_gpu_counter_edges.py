"""GPU: training across the 32-bit edges of the draw protocol's counters and of the turnstile path's step tags, on
every path of the main engine -- bit for bit against the C oracle started at the same counters.

* Draw counter: the step index is 64 bits and enters Philox as two words; every path expands it in its own code (the
  helper wavefronts' LDS rings of the persistent kernels, kernel-argument plans, the step-wise graph).  Each path starts
  at 2^32 - 60 and trains in two calls of 20 and 70 steps: the low word wraps 40 steps into the second call -- deeper
  than any ring -- and not at a call edge.
* Agent offset: ``qe_set_agent_offset(2^32 - n/2)``: the agent ids (Philox word 0, start-state hash) wrap in the middle
  of the agent vector, also on paths with more than one workgroup.
* Turnstile tags: the records carry 32 bits of a step count that runs through the engine's life.  Tags must only grow
  between two clears of the records and tag 0 means "cleared", so ``turn_setup`` moves a call whose tags would start on,
  reach or cross a multiple of 2^32 to the next multiple plus 1 and clears the records (they are also cleared whenever
  the tags cross 2^31).  ``qe_debug_set_turn_epoch`` places the count (and has the records cleared); cases (a) to (c)
  run a warm-up call first, so that the records hold tags from just below the edge when the call under test starts: (a) a call that straddles 2^31, (b) one
  that straddles 2^32, (c) one that ends exactly on 2^32 and the call that follows, (d) a call whose first tag would be
  0 (the count placed on the multiple itself) -- fully and lightly contested shapes, ``learn`` and ``learn_vec``, forwarding on and off, delta log included.
  ``qe_debug_turn_epoch`` shows that no call's tags include a multiple of 2^32.

Shown able to fail (by reasoning; nothing broken was run on a GPU): a path that fed ``(uint32_t)step`` as the whole
counter (high word 0) draws from step 0 .. 29 instead of 2^32 .. 2^32 + 29 in the second call: the explore / greedy
decisions of ~10 % of the agents differ in the first step behind the wrap and the action trace differs there.  An agent id
kept as ``offset + i`` in 64 bits where the oracle adds in uint32 hashes agents n/2 .. n - 1 to other start rows and
other draws: observations and actions differ from step 0.  Without the move in ``turn_setup``, case (b) registers step tags 0xFFFFFFxx and then
0x000000xx in one call: the atomic max with {tag, 0} leaves a record that still holds a pre-wrap tag of the same call
untouched, its count goes on from the old value, the next launch finds ``count.tag != tag``, takes the row for
uncontested and updates from a stale row -- on the fully contested shape (64 rows, every row re-used every step) that
happens in the first step behind the wrap and the table, the actions and the delta log differ from the oracle's; case
(d) issues tag 0, which the first launch cannot tell from a cleared record of another step.
"""

import numpy as np
import pytest

from test_gpu_delta_log import _Log, _check_records

pytestmark = pytest.mark.gpu

TWO32 = 1 << 32


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return _lib, OptimalQLearningBase, GpuRolloutQLearning, environments, schedules


# name -> (n, S, A, path, options, trace, expected kernel_variant fields)
PATHS = {
    "persistent_generic": (300, 900, 8, "auto", (), True, {"path": "persistent", "lean": 0, "cap512": True}),
    "persistent_dense": (256, 64, 16, "auto", (), True, {"path": "persistent", "lean": 0, "cap512": True}),
    "lane_dataflow": (128, 2000, 16, "auto", (("OPT_LANE_ORDERED_PATH", 1),), False,
                      {"path": "persistent", "lean": 1, "dataflow": True}),
    "lane_full": (128, 2000, 16, "auto", (("OPT_LANE_ORDERED_PATH", 2),), False,
                  {"path": "persistent", "lean": 1, "dataflow": False, "light": False}),
    "lane_sparse": (128, 2000, 16, "auto", (("OPT_LANE_ORDERED_PATH", 3),), False,
                    {"path": "persistent", "lean": 1, "dataflow": False, "light": True}),
    "stepwise": (200, 400, 8, "stepwise", (), True, {"path": "stepwise"}),
    "turnstile": (600, 300, 16, "auto", (), True, {"path": "turnstile"}),
    "turnstile_sparse": (4096, 200_000, 16, "auto", (), True, {"path": "turnstile"}),
    "wide_bitmap": (2100, 3000, 8, "wide", (), True, {"path": "wide"}),
    "wide_listed": (4096, 3000, 8, "wide", (("OPT_LISTED_MIN_AGENTS", 1), ("OPT_TOKEN_ROUNDS", 7)), True, {"path": "wide"}),
}


def _run(n, S, A, mode, path, options, trace, variant, calls, *, start=0, offset=0, turn_epoch=None, log=False,
         dt=np.float32):
    """The engine and the C oracle through `calls` run_steps calls from draw step `start` with agent ids from `offset`;
    returns the turnstile epochs read before every call and after the last one."""
    from oracle import c_oracle

    _lib, Algo, Runtime, envs, sch = _product()
    lib = _lib.load()
    steps = sum(calls)
    ref = c_oracle.CHashRollout(n, S, A, agent_offset=offset, dtype=dt, mode=mode)
    ref.step = start
    want = ref.run(np.full(steps, 0.1), np.full(steps, 0.1), trace=True, delta_log=True)
    algo = Algo(S, A, 0.99, seed=0, dtype=dt)
    algo.set_rollout_path(path)
    for opt, value in options:
        algo.set_engine_option(getattr(_lib, opt), value)
    algo.step_counter = start
    if offset:
        _lib.check(lib.qe_set_agent_offset(algo.handle, offset))
    if turn_epoch is not None:
        _lib.check(lib.qe_debug_set_turn_epoch(algo.handle, turn_epoch))
    dlog = None
    if log:
        dlog = _Log(steps * n, 2 * n + 64)
        _lib.check(lib.qe_delta_log_attach(algo.handle, dlog.ptr, steps * n))
    rt = Runtime(algo, sch.ConstantSchedule(0.1), sch.ConstantSchedule(0.1), learn_mode=mode)
    rt.trace_actions = True if trace else None
    env, sd, history, actions, epochs = envs.HashTabularEnv(n, S, A, seed=1, agent_offset=offset), None, [], [], []
    for k in calls:
        epochs.append(int(lib.qe_debug_turn_epoch(algo.handle)))
        try:
            _avg, h, env, sd = rt.run_steps(k, env, sd)
        except ZeroDivisionError:  # no episode ended in this call (reference quirk); the state moved on all the same
            h, sd = [], env.state_dict()
        history += h
        if trace:
            actions.append(rt.last_trace)
        assert rt.last_stats["kernel_variants"], "no launch was recorded"
        for v in rt.last_stats["kernel_variants"]:
            d = _lib.decode_variant(v)
            assert all(d[name] == value for name, value in variant.items()), d
    epochs.append(int(lib.qe_debug_turn_epoch(algo.handle)))
    _lib.check(lib.qe_synchronize(algo.handle))
    assert algo.step_counter == start + steps
    if trace:
        assert np.array_equal(np.concatenate(actions), want["actions"])
    assert np.array_equal(np.asarray(algo.q_table), ref.q, equal_nan=True)
    assert np.array_equal(np.array(history, dtype=np.float32), want["history"])
    assert np.array_equal(sd["states"], ref.obs)
    assert np.array_equal(sd["rewards"], ref.acc)
    if log:
        assert lib.qe_delta_log_count(algo.handle) == steps * n
        _check_records(dlog.read(), n, steps, int(lib.qe_table_row_stride(algo.handle)), A, want)
        _lib.check(lib.qe_delta_log_attach(algo.handle, None, 0))
        dlog.free()
    return epochs


# ---------------------------------------------------------------------------------------------- draw counter
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("name", list(PATHS))
def test_training_across_draw_step_2_to_32(name, mode):
    n, S, A, path, options, trace, variant = PATHS[name]
    if mode == "vec" and name.startswith("lane_"):  # LEAN builds are learn_iter builds: learn_vec runs the generic one
        variant = {"path": "persistent", "lean": 0, "cap512": True}
    _run(n, S, A, mode, path, options, trace, variant, (20, 70), start=TWO32 - 60)


def test_training_across_draw_step_2_to_32_float64():
    n, S, A, path, options, trace, variant = PATHS["turnstile"]
    _run(n, S, A, "iter", path, options, trace, variant, (20, 70), start=TWO32 - 60, dt=np.float64)


# ---------------------------------------------------------------------------------------------- agent ids
@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("name", ["persistent_generic", "lane_dataflow", "lane_sparse", "stepwise", "turnstile",
                                  "turnstile_sparse", "wide_bitmap", "wide_listed"])
def test_agent_ids_wrap_in_the_middle_of_the_agent_vector(name, mode):
    n, S, A, path, options, trace, variant = PATHS[name]
    if mode == "vec" and name.startswith("lane_"):
        variant = {"path": "persistent", "lean": 0, "cap512": True}
    _run(n, S, A, mode, path, options, trace, variant, (12, 18), offset=TWO32 - n // 2)


def test_draw_step_and_agent_ids_wrap_together():
    n, S, A, path, options, trace, variant = PATHS["turnstile"]
    _run(n, S, A, "iter", path, options, trace, variant, (20, 30), start=TWO32 - 35, offset=TWO32 - n // 2)


# ---------------------------------------------------------------------------------------------- turnstile tags
# A call of k steps that starts at epoch e issues the tags e .. e + k and leaves the engine at e + k + 2.
WARM, CALL = 12, 30
TAG_CASES = {
    # name -> (epoch placed before the warm-up call, calls)
    "a_straddles_2_to_31": ((1 << 31) - (WARM + 2) - 15, (WARM, CALL)),
    "b_straddles_2_to_32": (TWO32 - (WARM + 2) - 15, (WARM, CALL)),
    "c_ends_on_2_to_32": (TWO32 - (WARM + 2) - (CALL + 2), (WARM, CALL, CALL)),
    "d_first_tag_zero": (2 * TWO32, (CALL, WARM)),  # placed on the multiple itself (no engine gets there by itself)
    "b_high_multiple": (5 * TWO32 - (WARM + 2) - 15, (WARM, CALL)),
}


def _check_epochs(epochs, calls):
    """No call's tags (start .. start + k, start = the epoch after turn_setup's move) include a multiple of 2^32."""
    for before, after, k in zip(epochs[:-1], epochs[1:], calls):
        start = after - (k + 2)
        assert start >= before, (before, after, k)
        assert start % TWO32 != 0 and start // TWO32 == (start + k + 1) // TWO32, (before, after, k)
        if before % TWO32 != 0 and before // TWO32 == (before + k + 2) // TWO32:
            assert start == before, "a call that crosses nothing was moved"


@pytest.mark.parametrize(("mode", "forward"), [("iter", 1), ("iter", 0), ("vec", 1)])  # (forwarding concerns learn_iter)
@pytest.mark.parametrize("shape", ["contested", "light"])
@pytest.mark.parametrize("case", list(TAG_CASES))
def test_turnstile_tags_at_their_edges(case, shape, mode, forward):
    """Fully contested: 600 agents on 64 rows (every record re-used in every step, far over its ten entries); lightly
    contested: 4096 agents on 200 000 rows.  QE_OPT_TURN_FORWARD 0 is the float32 learn_iter re-read form."""
    n, S, A = (600, 64, 16) if shape == "contested" else (4096, 200_000, 16)
    epoch, calls = TAG_CASES[case]
    epochs = _run(n, S, A, mode, "auto", (("OPT_TURN_FORWARD", forward),), True, {"path": "turnstile"}, calls,
                  turn_epoch=epoch, log=True)
    assert epochs[0] == epoch
    _check_epochs(epochs, calls)
    if case == "d_first_tag_zero":
        assert epochs[1] == epoch + 1 + calls[0] + 2, "tag 0 was issued"
    elif case != "a_straddles_2_to_31":
        assert epochs[-1] > (epoch // TWO32 + 1) * TWO32, "the case did not reach the multiple of 2^32 it is about"


def test_a_fresh_engine_starts_at_tag_1():
    _lib, Algo, _, _, _ = _product()
    assert _lib.load().qe_debug_turn_epoch(Algo(64, 16, 0.99, seed=0).handle) == 1
