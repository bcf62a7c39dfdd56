"""GPU: the sparse builds of ``k_rollout_lane`` after their quiet step was slimmed, against the C oracle, bit for bit.

In these builds (``QE_OPT_LANE_ORDERED_PATH`` = 3: ``LEAN`` 1 / 2, ``HELP``, ``FULL``, ``SEQ``) the agents' wavefronts

* read the predicted value Q[s, a] back from the table behind the row gather instead of picking it out of the row in
  registers (one more load in flight across the step barrier, taken over at the top of the next step),
* hand reward and end flag of every transition to the helper wavefronts, which keep the running returns, reserve the
  episode-log slots and write the log,
* take learning rate and exploration threshold from the helpers' ring instead of loading them,

see ``csrc/qe_rollout_lane.h``.  Every case runs the engine as a user does (``run_steps`` -> ctypes -> C ABI, no action
trace), asserts the build through ``kernel_variant`` and compares everything a rollout leaves behind -- the table, the
episode returns in the host's order, the final observations, the environment's episode counters, the running returns
and ``rng_step`` -- with ``oracle/c_oracle.py``, without a tolerance.  The cases that are about particular events
(an agent staying in its row in a quiet step; an agent entering a row another agent wrote a step earlier, or is
writing in the same step) count those events in the oracle's trace and assert the count, so they cannot pass empty.
"""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CALL_SPLITS = [1, 2, 3, 31, 32, 33, 64, 65]  # one-step call, the flush window of 32, the inline-schedule limit of 64


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return _lib, OptimalQLearningBase, GpuRolloutQLearning, environments, schedules


def _plan(total):
    head = [k for k in CALL_SPLITS]
    assert sum(head) < total
    return head + [total - sum(head)]


def _split(total, k):
    return [k] * (total // k) + ([total % k] if total % k else [])


def _schedules(kind, n, steps):
    """(eps, lr) of every vector step for the oracle, and the runtime's schedule objects."""
    from oracle import c_oracle

    sch = _product()[4]
    if kind == "bench":
        eps, _ = c_oracle.exp_schedule(1.0, 0.01, 0.995, n, steps)
        lr, _ = c_oracle.exp_schedule(0.1, 1e-5, 0.995, n, steps)
        return eps, lr, sch.ExponentialSchedule(0.1, 1e-5, 0.995), sch.ExponentialSchedule(1.0, 0.01, 0.995)
    eps_c, lr_c = kind
    return np.full(steps, eps_c), np.full(steps, lr_c), sch.ConstantSchedule(lr_c), sch.ConstantSchedule(eps_c)


class _Oracle:
    """One C-oracle run of `steps` steps, stepped one vector step at a time so that every transition (s, a, n, term) of
    the trace is known; the results of the whole run are what the engine's are compared with."""

    def __init__(self, n, S, A, steps, sched, *, q0=None, env_seed=1, delta_log=False):
        from oracle import c_oracle

        eps, lr, _, _ = _schedules(sched, n, steps)
        ref = c_oracle.CHashRollout(n, S, A, env_seed=env_seed, q=None if q0 is None else q0.copy())
        self.s, self.nxt = np.empty((steps, n), np.int32), np.empty((steps, n), np.int32)
        hist, cells, deltas, actions = [], [], [], []
        for t in range(steps):
            self.s[t] = ref.obs
            out = ref.run(eps[t:t + 1], lr[t:t + 1], trace=True, delta_log=delta_log)
            self.nxt[t] = ref.obs
            hist.append(out["history"])
            actions.append(out["actions"][0])
            if delta_log:
                cells.append(out["cells"].copy())
                deltas.append(out["deltas"].copy())
        self.history = np.concatenate(hist)
        self.ended = np.array([h.size for h in hist])  # episodes that ended in each step
        self.actions = np.array(actions)
        self.cells = np.concatenate(cells) if delta_log else None
        self.deltas = np.concatenate(deltas) if delta_log else None
        self.q, self.obs, self.acc, self.episode = ref.q, ref.obs.copy(), ref.acc.copy(), ref.episode.copy()
        self.steps, self.n = steps, n

    def busy(self, t):
        """Some row written in step t has a second toucher (another writer, or another agent's successor row)."""
        ws, nx = self.s[t], self.nxt[t]
        u, c = np.unique(ws, return_counts=True)
        if (c > 1).any():
            return True
        return bool((np.isin(nx, ws) & (nx != ws)).any())

    def quiet_self_transitions(self):
        return sum(int((self.nxt[t] == self.s[t]).sum()) for t in range(self.steps) if not self.busy(t))

    def readers_of_a_row_written_in_the_same_step(self):
        return sum(int((np.isin(self.nxt[t], self.s[t]) & (self.nxt[t] != self.s[t])).sum()) for t in range(self.steps))

    def followers(self):
        """Agents whose successor row of step t + 1 was written in step t by ANOTHER agent."""
        total = 0
        for t in range(self.steps - 1):
            ws = self.s[t]
            for j in np.flatnonzero(np.isin(self.nxt[t + 1], ws)):
                total += int(((ws == self.nxt[t + 1][j]) & (np.arange(self.n) != j)).any())
        return total


def _same_bits(got, want):
    """Equal including the sign of a zero; NaN wherever the oracle has one (a NaN's payload is not a result)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _run(n, S, A, plan, sched, *, q0=None, env_seed=1, delta_log=False):
    """The engine on the sparse build, call by call; returns what the calls left behind."""
    _lib, Algo, Runtime, envs, _ = _product()
    lib = _lib.load()
    steps = sum(plan)
    algo = Algo(S, A, 0.99, seed=0)
    if q0 is not None:
        algo.q_table = q0.copy()
    algo.set_engine_option(_lib.OPT_LANE_ORDERED_PATH, 3)
    _, _, lr_s, eps_s = _schedules(sched, n, steps)
    rt = Runtime(algo, lr_s, eps_s)
    env = envs.HashTabularEnv(n, S, A, seed=env_seed)
    hip, log_dev = None, None
    if delta_log:
        hip = C.CDLL("libamdhip64.so")
        log_dev, nbytes = C.c_void_p(), steps * n * 8
        assert hip.hipMalloc(C.byref(log_dev), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(log_dev, 0, C.c_size_t(nbytes)) == 0
        assert hip.hipDeviceSynchronize() == 0
        _lib.check(lib.qe_delta_log_attach(algo.handle, log_dev, steps * n))
    sd, history = None, []
    for k in plan:
        try:
            _avg, h, env, sd = rt.run_steps(k, env, sd)
        except ZeroDivisionError:  # no episode ended in this call (reference quirk); the state moved on all the same
            h, sd = [], env.state_dict()
        history += h
        for v in rt.last_stats["kernel_variants"]:
            d = _lib.decode_variant(v)
            assert d["path"] == "persistent" and d["lean"] == (2 if delta_log else 1), d
            assert d["help"] and d["full"] and d["light"] and not d["dataflow"] and not d["cap512"] and d["nv"] == A // 4, d
    got = {"q": np.asarray(algo.q_table).copy(), "history": np.array(history, dtype=np.float32), "sd": sd}
    if delta_log:
        _lib.check(lib.qe_synchronize(algo.handle))
        assert lib.qe_delta_log_count(algo.handle) == steps * n
        rec = np.empty((steps * n, 2), dtype=np.int32)
        assert hip.hipMemcpy(rec.ctypes.data_as(C.c_void_p), log_dev, C.c_size_t(steps * n * 8), 2) == 0  # device to host
        _lib.check(lib.qe_delta_log_attach(algo.handle, None, 0))
        assert hip.hipFree(log_dev) == 0
        got["records"], got["ld"] = rec, int(lib.qe_table_row_stride(algo.handle))
    return got


def _compare(got, want):
    _same_bits(got["q"], want.q)
    _same_bits(got["history"], want.history)
    sd = got["sd"]
    assert np.array_equal(sd["states"], want.obs)
    assert np.array_equal(sd["aux"], want.episode)
    _same_bits(np.asarray(sd["rewards"], dtype=np.float32), want.acc)
    assert sd["rng_step"] == want.steps


@pytest.fixture(scope="module")
def oracle():
    cache = {}

    def get(*key, **kw):
        k = (key, tuple(sorted((a, b if not isinstance(b, np.ndarray) else b.tobytes()) for a, b in kw.items())))
        if k not in cache:
            cache[k] = _Oracle(*key, **kw)
        return cache[k]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------ 1. call lengths
MIXED_STEPS = 300


@pytest.mark.parametrize("calls", ["split", "one"])
@pytest.mark.parametrize("n", [128, 64])
def test_call_lengths_on_a_mixed_shape(oracle, n, calls):
    """4 096 states x 16 actions: quiet, two-toucher and complex steps.  Calls of 1, 2, 3, 31, 32, 33, 64, 65 steps and
    the rest: the hand-over of reward and end flag across a call boundary, the flush window of 32, the inline-schedule
    limit of 64, the carried running return, a one-step call -- and the same total as one call."""
    want = oracle(n, 4096, 16, MIXED_STEPS, "bench")
    assert want.history.size > 0
    plan = _plan(MIXED_STEPS) if calls == "split" else [MIXED_STEPS]
    if calls == "split":  # several calls end with a step in which an episode ends
        assert (want.ended[np.cumsum(plan) - 1] > 0).sum() >= 3
    _compare(_run(n, 4096, 16, plan, "bench"), want)


# ------------------------------------------------------------------------------------------------ 2. own-row patch
@pytest.mark.parametrize(("n", "S", "steps", "env_seed"), [(64, 100_000, 3000, 2), (128, 500_000, 3000, 6)])
def test_agents_that_stay_in_their_row_in_a_quiet_step(oracle, n, S, steps, env_seed):
    """n == s in a quiet step: the own write is patched into the row in registers (and may move its maximum), and the
    predicted cell is loaded behind the agent's own store to (possibly) the same address.  The transitions of
    the hash environment are a fixed function of (state, action), so an agent stays where it is only on one of the few
    (state, action) pairs that map to their own state: table size and environment seed were chosen on the CPU for
    traces in which agents find such a pair while a large share of the steps is quiet (40 % / 55 %)."""
    want = oracle(n, S, 16, steps, "bench", env_seed=env_seed)
    events = want.quiet_self_transitions()
    print(f"{events} self-transitions in quiet steps")
    assert events >= 10
    _compare(_run(n, S, 16, [steps], "bench", env_seed=env_seed), want)


# ------------------------------------------------------------------------------------------------ 3. followers
@pytest.mark.parametrize("n", [128, 64])
def test_agents_entering_a_row_written_by_another_agent(oracle, n):
    """The regather of a possibly stale row (written one step earlier by someone else) and the W-R busy step (written in
    the same step by someone else): the predicted cell of the follower must be the written value."""
    want = oracle(n, 4096, 16, MIXED_STEPS, "bench")
    followers, readers = want.followers(), want.readers_of_a_row_written_in_the_same_step()
    print(f"{followers} followers, {readers} same-step readers")
    assert followers >= 10 and readers >= 10
    _compare(_run(n, 4096, 16, _split(MIXED_STEPS, 50), "bench"), want)


# ------------------------------------------------------------------------------------------------ 4. NaN, inf, signed zeros
def _special_table(S, A, nan_cells, seed):
    rng = np.random.default_rng(seed)
    q = np.zeros((S, A), dtype=np.float32)
    q[rng.random((S, A)) < 0.5] = -0.0             # -0.0 ties with +0.0 at the row maximum
    neg = rng.random((S, A)) < 0.2
    q[neg] = -rng.random(int(neg.sum()), dtype=np.float32)
    flat = q.ravel()
    special = rng.choice(S * A, size=3 * 40 + nan_cells, replace=False)
    flat[special[:40]] = np.inf
    flat[special[40:80]] = -np.inf
    flat[special[80:120]] = -0.0
    flat[special[120:]] = np.nan
    return q


@pytest.mark.parametrize(("n", "S", "eps", "nan_cells", "table_seed"), [
    (128, 20000, 0.9, 5, 8),   # 100 agents and more: np.max, a NaN row has no greedy pick (the reference raises IndexError)
    (64, 3000, 0.3, 200, 7),   # fewer: the list variants scan past NaN
])
def test_non_finite_values_and_signed_zeros(oracle, n, S, eps, nan_cells, table_seed):
    """A table of +0.0 / -0.0 ties with NaN, +inf and -inf cells, ``nan_select`` on (128 agents) and off (64).  With
    np.max a greedy pick from a NaN row ends the run in the reference, so that case explores more, on a larger table,
    and its few NaN cells and the table seed were chosen on the CPU for a run the oracle finishes while NaN still
    spreads through the TD targets (5 cells become 20).  The sign of every zero and every NaN of the final table must
    be the oracle's."""
    A, steps = 16, 120
    q0 = _special_table(S, A, nan_cells, table_seed)
    want = oracle(n, S, A, steps, (eps, 0.1), q0=q0)  # (IndexError here: a NaN row met a greedy pick in the oracle)
    print(f"NaN cells {nan_cells} -> {int(np.isnan(want.q).sum())}, inf cells {int(np.isinf(want.q).sum())}")
    assert np.isnan(want.q).sum() > nan_cells and np.isinf(want.q).any()
    assert (np.signbit(want.q) & (want.q == 0)).any() and (~np.signbit(want.q) & (want.q == 0)).any()
    _compare(_run(n, S, A, _split(steps, 33), (eps, 0.1), q0=q0), want)


# ------------------------------------------------------------------------------------------------ 5. delta log
@pytest.mark.parametrize("n", [128, 64])
def test_delta_log_build_record_by_record(oracle, n):
    """LEAN = 2 with the call splits of case 1: cell and float32 increment of EVERY agent-step."""
    S, A = 4096, 16
    want = oracle(n, S, A, MIXED_STEPS, "bench", delta_log=True)
    got = _run(n, S, A, _plan(MIXED_STEPS), "bench", delta_log=True)
    cells, ld = got["records"][:, 0].view(np.uint32), got["ld"]
    assert np.array_equal(cells % ld, want.actions.reshape(-1).astype(np.uint32))
    assert np.array_equal(cells // ld * A + cells % ld, want.cells)
    _same_bits(got["records"][:, 1].view(np.float32), want.deltas)
    _compare(got, want)


# ------------------------------------------------------------------------------------------------ 6. episode log at capacity
HOST_LOG_CAP = 2**18


@pytest.mark.parametrize("extra", [0, 1])
def test_episode_log_at_capacity_through_the_sparse_build(extra):
    """Every agent ends an episode in every step (``p_term_256`` = 256): ``chunk_limit`` steps fill the host result
    block's log to its last entry through the helpers' stage / straight-to-memory stores; one step more is counted,
    not written.  Kept entries, ``episodes`` and ``episodes_dropped`` against the oracle."""
    from oracle import c_oracle

    _lib, Algo, _, envs, _ = _product()
    lib = _lib.load()
    n, S, A = 128, 200000, 16
    algo = Algo(S, A, 0.99, seed=0)
    algo.set_engine_option(_lib.OPT_LANE_ORDERED_PATH, 3)
    env = envs.HashTabularEnv(n, S, A, seed=1, p_term_256=256)
    env.bind(algo)
    env.reset_device()
    limit = env.chunk_limit(True)
    assert limit == HOST_LOG_CAP // n
    steps = limit + extra
    eps, lr = np.full(steps, 0.3), np.full(steps, 0.1)
    st = _lib.RolloutStats()
    _lib.check(lib.qe_rollout(algo.handle, env.handle, steps, _lib.ptr(eps, C.c_double), _lib.ptr(lr, C.c_double),
                              _lib.LEARN_ITER, None, C.byref(st)))
    d = _lib.decode_variant(st.kernel_variant)
    assert d["path"] == "persistent" and d["lean"] == 1 and d["help"] and d["full"] and d["light"] and not d["dataflow"], d
    ref = c_oracle.CHashRollout(n, S, A, p_term_256=256)
    want = ref.run(eps, lr)
    total, kept = steps * n, limit * n
    assert want["episodes"] == total
    assert st.episodes == total and st.episodes_dropped == extra * n
    step, agent = np.full(total + 8, -1, dtype=np.int32), np.full(total + 8, -1, dtype=np.int32)
    ret = np.full(total + 8, np.nan, dtype=np.float32)
    count = int(lib.qe_episode_log(algo.handle, total + 8, _lib.ptr(step, C.c_int32), _lib.ptr(agent, C.c_int32),
                                   _lib.ptr(ret, C.c_float)))
    assert count == kept
    assert np.array_equal(step[:kept], want["ep_step"][:kept]) and np.array_equal(agent[:kept], want["ep_agent"][:kept])
    _same_bits(ret[:kept], want["history"][:kept])
    assert (step[kept:] == -1).all() and np.isnan(ret[kept:]).all()
    _same_bits(np.asarray(algo.q_table), ref.q)
    states, acc = env.observe()
    assert np.array_equal(states, ref.obs) and np.array_equal(env.aux(), ref.episode)
    _same_bits(np.asarray(acc, dtype=np.float32), ref.acc)
