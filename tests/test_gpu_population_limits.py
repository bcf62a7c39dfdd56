"""GPU: ``QLearningPopulation`` (k_rollout_runs) at the edges of what its host and kernel do.

Every row build (NV = 1, 2, 4, 8, 16, masked and unmasked, padded or not), calls cut into several launches with and
without the episode log, NaN in the tables (both selection variants and the own-write register patch), step counters
and agent ids that wrap, schedules that leave their range, and a table of more than 2^31 cells.  Run r must equal,
bit for bit, its one-agent reference: the C oracle (HashEnv), the NumPy oracle on the table model (TableEnv) or a
one-agent ``GpuRolloutQLearning`` run (bandit).  Each case also asserts the kernel build and the number of launches it
means to reach, from ``last_stats``.
"""
import copy

import numpy as np
import pytest

from oracle import c_oracle
from oracle.draws import InjectedDraws
from oracle.qlearn_oracle import OracleQLearning, OracleRuntime, OracleSchedule
from table_mdp_model import TableMDPVecEnv, random_mdp
from test_gpu_population import _schedules

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms import QLearningPopulation

    return _lib, environments, schedules, QLearningPopulation


def per_launch(M, K, log):
    """Steps per launch of a call of K steps over M runs: qe_population_rollout in csrc/qe_population.hip
    (RUNS_STEP_BUDGET = 2^25 env-steps per launch; with the log, RUNS_LOG_BUDGET = 2^23 entries per launch)."""
    p = max(1, 2**25 // M)
    if log:
        p = min(p, max(1, 2**23 // M))
    return min(p, K) if K > 0 else p


def launches(M, K, log):
    """``last_stats["launches"]``: per launch, the rollout kernel plus (log) the scan and pack kernels."""
    return -(-K // per_launch(M, K, log)) * (3 if log else 1)


def _reached(pop, M, K, log, nv=None, masked=None):
    _lib = _product()[0]
    d = _lib.decode_variant(pop.last_stats["kernel_variant"])
    assert d["path"] == "population", d
    if nv is not None:
        assert d["nv"] == nv, d
    if masked is not None:
        assert d["masked"] == masked, d
    assert pop.last_stats["launches"] == launches(M, K, log), (pop.last_stats, per_launch(M, K, log))


def _nv(A):
    """NV of the build a row of A actions takes: the row stride (A rounded up to a power of two, at least 4) / 4."""
    return max(4, 1 << (A - 1).bit_length()) // 4


def _seq_mean(returns):
    """float32 sequential sum / count: the standalone run's ``sum(history) / len(history)``."""
    if len(returns) == 0:
        return None
    return np.cumsum(np.asarray(returns, dtype=np.float32), dtype=np.float32)[-1] / np.float32(len(returns))


def _check_run(pop, res, r, want, *, table, state, eps_after=None, lr_after=None):
    """Run r of a population call against its reference (``want``: history / ep_step / episodes)."""
    assert np.array_equal(table, want["q"], equal_nan=True), f"run {r}: table"
    assert np.array_equal(res.run_returns(r), want["history"]), f"run {r}: returns"
    assert np.array_equal(res.run_steps(r), want["ep_step"]), f"run {r}: episode steps"
    assert res.episode_counts[r] == want["episodes"], f"run {r}: episode count"
    mean = _seq_mean(want["history"])
    if mean is None:
        assert np.isnan(res.mean_returns[r]), r
    else:
        assert res.mean_returns[r] == mean, f"run {r}: mean"
    sd = res.state_dict
    obs, aux, acc = state
    assert (sd["states"][r], sd["aux"][r], sd["rewards"][r]) == (obs, aux, acc), f"run {r}: final state"
    if eps_after is not None:
        assert pop.exploration_rate_schedules[r].get_value() == eps_after == sd["exploration_rate"][r], r
    if lr_after is not None:
        assert pop.lr_schedules[r].get_value() == lr_after == sd["lr"][r], r


def _hash_reference(r, S, A, masked, eps, lr, gamma, dt, mode, K, *, offset=0, step0=0, seed=0, q0=None, trace=False):
    """One-agent C-oracle run r: its result dict plus the final table, state and schedule values."""
    ref = c_oracle.CHashRollout(1, S, A, masked=masked, agent_offset=(offset + r) & U32, gamma=gamma, dtype=dt,
                                mode=mode, seed=seed)
    ref.step = step0
    if q0 is not None:
        ref.q[:] = q0
    e, lrs = copy.deepcopy(eps), copy.deepcopy(lr)
    want = ref.run(e.advance_values(1, K), lrs.advance_values(1, K), trace=trace)
    want["q"] = ref.q
    return want, (ref.obs[0], ref.episode[0], ref.acc[0]), e.get_value(), lrs.get_value()


def _check_hash_runs(pop, res, runs, S, A, masked, eps_s, lr_s, gamma, dt, mode, K, *, offset=0, step0=0, seed=0,
                     q0=None, tables=None):
    for r in runs:
        want, state, e_after, l_after = _hash_reference(r, S, A, masked, eps_s[r], lr_s[r], gamma[r], dt, mode, K,
                                                        offset=offset, step0=step0, seed=seed,
                                                        q0=None if q0 is None else q0[r])
        table = pop.q_table(r) if tables is None else tables[r]
        _check_run(pop, res, r, want, table=table, state=state, eps_after=e_after, lr_after=l_after)


def _sample(M, extra=3, seed=0):
    fixed = [r for r in (0, 1, 63, 64, 127, 128, 129) if r < M] + [M - 1]
    rng = np.random.default_rng(seed)
    return sorted(set(fixed) | set(rng.integers(0, M, extra).tolist()))


# ---- 1. every row build ---------------------------------------------------------------------------------------------
M_ROWS, K_ROWS, S_ROWS = 130, 300, 1000  # two full wavefronts and a partial one


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [1, 3, 4, 5, 9, 17, 32, 33, 63, 64])
def test_every_hash_row_build_matches_the_c_oracle(A, masked, dt, mode):
    _lib, envs, _, QLearningPopulation = _product()
    M, K, S = M_ROWS, K_ROWS, S_ROWS
    eps_s, lr_s, gamma = _schedules(M)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=dt,
                              learn_mode=mode)
    res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=masked))
    _reached(pop, M, K, True, nv=_nv(A), masked=masked)
    tables = pop.q_tables
    _check_hash_runs(pop, res, _sample(M, seed=A), S, A, masked, eps_s, lr_s, gamma, dt, mode, K, tables=tables)
    assert pop.step_counter == K


def _oracle_schedule(s):
    _, _, sch, _ = _product()
    if type(s) is sch.ExponentialSchedule:
        return OracleSchedule("exponential", s.get_value(), s.min_value, s.decay_rate)
    if type(s) is sch.LinearSchedule:
        return OracleSchedule("linear", s.get_value(), None, s.decay_rate)
    return OracleSchedule("constant", s.get_value())


def _table_reference(mdp, r, K, gamma, eps, lr, dt, mode, *, seed, env_seed, step0=0):
    """One-agent NumPy-oracle run r on the table model (agent id r for the env and the draws)."""
    env = TableMDPVecEnv(1, mdp, seed=env_seed, agent_offset=r)
    algo = OracleQLearning(env.state_size, env.action_size, gamma, seed=seed, dtype=np.dtype(dt))
    algo._rng = algo._np_rng = InjectedDraws(seed, agent_ids=env.agent_ids)
    es, ls = _oracle_schedule(eps), _oracle_schedule(lr)
    rt = OracleRuntime(algo, ls, es, learn_mode=mode)
    states, _ = env.reset()
    env.step_index = rt.step_counter = step0  # (the reset draws from its reserved step, whatever the counter)
    acc = np.zeros(1, dtype=np.float32)
    history, ep_step = [], []
    for t in range(K):
        n = len(history)
        states, _ = rt.run_single_step(env, states, acc, history)
        ep_step += [t] * (len(history) - n)
    obs = states["observation"] if isinstance(states, dict) else states
    want = {"q": algo.q_table, "history": np.array(history, dtype=np.float32), "ep_step": np.array(ep_step, np.int32),
            "episodes": len(history)}
    return want, (obs[0], 0, acc[0]), es.get_value(), ls.get_value()


def _table_mdp(name):
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    if name == "a20":
        arrays, isd, _ = random_mdp(150, 20, 3, seed=4)
        return encode_table_mdp(*arrays, isd), False
    arrays, isd, masks = random_mdp(200, 40, 2, seed=7, masked=True)  # two mask words per state
    return encode_table_mdp(*arrays, isd, masks), True


@pytest.mark.parametrize("mode", ["iter", "vec"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["a20", "a40_masked"])
def test_wide_table_env_rows_match_the_numpy_oracle(name, dt, mode):
    _lib, envs, _, QLearningPopulation = _product()
    mdp, masked = _table_mdp(name)
    M, K = M_ROWS, K_ROWS
    S, A = mdp.thr.shape[:2]
    eps_s, lr_s, gamma = _schedules(M)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=5, dtype=dt,
                              learn_mode=mode)
    res = pop.run_steps(K, envs.TabularMDPEnv(M, mdp, seed=3))
    _reached(pop, M, K, True, nv={20: 8, 40: 16}[A], masked=masked)
    for r in _sample(M, extra=2, seed=A):
        want, state, e_after, l_after = _table_reference(mdp, r, K, gamma[r], eps_s[r], lr_s[r], dt, mode, seed=5,
                                                         env_seed=3)
        _check_run(pop, res, r, want, table=pop.q_table(r), state=state, eps_after=e_after, lr_after=l_after)


# ---- 2. calls cut into several launches -----------------------------------------------------------------------------
def _cycled_schedules(M, period=97):
    """``_schedules(period)`` repeated: run r shares its schedule objects with every run of the same r % period (one
    descriptor per object), and the discounts stay at most 0.9 + 0.001 * (period - 1)."""
    eps, lr, gamma = _schedules(period)
    return [[x[r % period] for r in range(M)] for x in (eps, lr, gamma)]


def _check_log(res, K):
    """The log agrees with the counts and sums the kernel kept: steps strictly increasing inside [0, K) per run, and
    the float32 sequential sum of each run's returns / count equal to its mean."""
    counts, off = res.episode_counts, res.offsets
    total = int(counts.sum())
    assert off[-1] == total == res.returns.size == res.steps.size
    assert np.array_equal(np.diff(off), counts)
    assert total == 0 or (res.steps.min() >= 0 and res.steps.max() < K)
    if total > 1:
        inner = np.ones(total - 1, dtype=bool)
        starts = off[1:-1]
        inner[starts[(starts > 0) & (starts < total)] - 1] = False  # a new run begins after these entries
        assert (np.diff(res.steps)[inner] > 0).all(), "episode steps not strictly increasing inside a run"
    acc = np.zeros(counts.size, dtype=np.float32)
    for j in range(int(counts.max(initial=0))):
        has = counts > j
        acc[has] += res.returns[off[:-1][has] + j]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = acc / counts.astype(np.float32)
    assert np.array_equal(res.mean_returns, mean, equal_nan=True), "means differ from the logged returns"
    assert np.isnan(res.mean_returns[counts == 0]).all()


SPLIT_CASES = [
    # M, K, S, A, masked, dtype, mode
    pytest.param(3000, 6000, 300, 16, True, np.float64, "iter", id="M3000_K6000"),
    pytest.param(40_000, 2000, 100, 8, False, np.float32, "vec", id="M40000_K2000"),
    pytest.param(2**22 + 17, 4, 3, 2, False, np.float32, "iter", id="M4194321_K4"),
]


@pytest.mark.parametrize(("M", "K", "S", "A", "masked", "dt", "mode"), SPLIT_CASES)
def test_calls_cut_into_launches_match_one_launch_and_the_oracle(M, K, S, A, masked, dt, mode):
    _lib, envs, sch, QLearningPopulation = _product()
    if M > 100_000:  # one schedule object shared by every run: descriptors are built per object, not per run
        def schedules():
            return [sch.ExponentialSchedule(0.9, 0.05, 0.5)] * M, [sch.LinearSchedule(0.4, -0.05)] * M
        gamma = [0.95] * M
    else:
        eps0, lr0, gamma = _cycled_schedules(M)

        def schedules():
            return copy.deepcopy(eps0), copy.deepcopy(lr0)
    eps_s, lr_s = schedules()

    def make():
        eps, lr = schedules()
        return QLearningPopulation(M, S, A, gamma, lr, eps, seed=21, dtype=dt, learn_mode=mode)

    def env():
        return envs.HashTabularEnv(M, S, A, seed=1, masked=masked)

    logged = make()
    res = logged.run_steps(K, env())
    _reached(logged, M, K, True, nv=_nv(A), masked=masked)
    assert logged.last_stats["launches"] > 3, "the logged call must be cut into several launches"
    _check_log(res, K)
    tables = logged.q_tables

    quiet = make()
    res_q = quiet.run_steps(K, env(), log=False)
    _reached(quiet, M, K, False)
    assert res_q.returns.size == 0 and res_q.steps.size == 0
    assert np.array_equal(quiet.q_tables, tables)
    assert np.array_equal(res_q.episode_counts, res.episode_counts)
    assert np.array_equal(res_q.mean_returns, res.mean_returns, equal_nan=True)
    for key in ("states", "aux", "rewards", "lr", "exploration_rate", "rng_step"):
        assert np.array_equal(res_q.state_dict[key], res.state_dict[key]), key
    del quiet

    # two calls of K / 2 steps, the second resumed from the first's state dict: the launches split differently again
    halves = make()
    e = env()
    first = halves.run_steps(K // 2, e)
    _reached(halves, M, K // 2, True)
    second = halves.run_steps(K - K // 2, e, first.state_dict)
    _reached(halves, M, K - K // 2, True)
    assert np.array_equal(halves.q_tables, tables)
    assert np.array_equal(first.episode_counts + second.episode_counts, res.episode_counts)
    _check_log(first, K // 2)
    _check_log(second, K - K // 2)
    # whole logs: per run, the first call's entries then the second's (steps shifted by K / 2)
    at = np.repeat(np.arange(M), first.episode_counts), np.repeat(np.arange(M), second.episode_counts)
    order = np.argsort(np.concatenate(at), kind="stable")
    assert np.array_equal(np.concatenate([first.returns, second.returns])[order], res.returns)
    assert np.array_equal(np.concatenate([first.steps, second.steps + K // 2])[order], res.steps)
    for key in ("states", "aux", "rewards", "lr", "exploration_rate", "rng_step"):
        assert np.array_equal(second.state_dict[key], res.state_dict[key]), key
    del halves

    rng = np.random.default_rng(M)
    runs = sorted({0, 1, 63, 64, 1023, 1024, 1025, M // 2, M - 2, M - 1} | set(rng.integers(0, M, 4).tolist()))
    _check_hash_runs(logged, res, runs, S, A, masked, eps_s, lr_s, gamma, dt, mode, K, seed=21, tables=tables)


# ---- 3. NaN through the population ----------------------------------------------------------------------------------
def _nan_tables(M, S, A, dt, seed):
    """Random tables; run r gets r % 5 NaN cells and, for r % 13 == 12, a whole NaN row (the list selection has no
    candidate only on a row without a number)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((M, S, A)).astype(dt)
    for r in range(M):
        q[r].ravel()[rng.choice(S * A, size=r % 5, replace=False)] = np.nan
        if r % 13 == 12:
            q[r, rng.integers(0, S)] = np.nan
    return q


def _run_catching(pop, K, env, sd=None):
    """The call's result and the runs it names as raising.  A run raises where its selection has no candidate: the
    NumPy-style selection of the reference raises IndexError there (q_learning_optimal.py:470, :563); its list
    selection returns -1 instead (:302, :348), and every engine path, the population's included, raises IndexError
    for that run as well (a -1 in the oracle's action trace)."""
    try:
        return pop.run_steps(K, env, sd), []
    except IndexError as err:
        assert str(err).startswith("Cannot choose from an empty sequence (runs ")
        return err.result, err.runs


@pytest.mark.parametrize(("A", "masked", "dt", "mode"), [
    (8, False, np.float32, "iter"),   # list selection: steps over NaN
    (9, True, np.float64, "vec"),     # list selection, masked
    (16, True, np.float32, "vec"),    # NumPy-style selection: a NaN in a valid column raises
    (40, True, np.float64, "iter"),   # NumPy-style selection, two mask words
])
def test_seeded_nan_cells_match_the_c_oracle(A, masked, dt, mode):
    _lib, envs, _, QLearningPopulation = _product()
    M, S, K = M_ROWS, 100, K_ROWS
    eps_s, lr_s, gamma = _schedules(M)
    q0 = _nan_tables(M, S, A, dt, seed=A)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=dt,
                              learn_mode=mode)
    pop.set_q_tables(q0)
    res, raised = _run_catching(pop, K, envs.HashTabularEnv(M, S, A, seed=1, masked=masked))
    _reached(pop, M, K, True, nv=_nv(A), masked=masked)
    tables = pop.q_tables
    want_raised, nan_kept = [], 0
    for r in range(M):
        try:
            want, state, e_after, l_after = _hash_reference(r, S, A, masked, eps_s[r], lr_s[r], gamma[r], dt, mode, K,
                                                            q0=q0[r], trace=True)
        except IndexError:  # the NumPy-style selection met a NaN maximum
            want_raised.append(r)
            continue
        if (want["actions"] < 0).any():  # the list selection met a row without a number: see _run_catching
            want_raised.append(r)
            continue
        nan_kept += np.isnan(want["q"]).any()
        _check_run(pop, res, r, want, table=tables[r], state=state, eps_after=e_after, lr_after=l_after)
    assert raised == want_raised
    assert want_raised, "no run met a row without a selectable action"
    assert nan_kept, "no run finished with a NaN in its table"


def _diverging_schedules(M, sch):
    """Learning rates above 1 and discounts above 1 on some runs (their tables overflow, then turn NaN), ordinary
    values on others."""
    lr = [sch.ConstantSchedule((2.5, 1.9, 0.3, 1.0)[r % 4]) for r in range(M)]
    eps = [sch.ConstantSchedule((0.1, 0.05, 0.2)[r % 3]) for r in range(M)]
    gamma = [(0.9, 1.5, 0.99, 3.0)[(r // 4) % 4] for r in range(M)]
    return eps, lr, gamma


@pytest.mark.parametrize(("S", "dt", "mode", "K"), [(2, np.float32, "iter", 400), (3, np.float64, "vec", 2200)])
def test_diverging_masked_runs_raise_at_the_oracles_step(S, dt, mode, K):
    """Masked A = 16 (NumPy-style selection) on 2 or 3 states: s' == s in many steps, so a NaN an update writes lands
    in the row the lane holds in registers.  The raise shows only per call, so the population runs in calls of two
    steps (each one launch, in which the register patch matters): run r must raise first in the call holding the step
    at which its oracle raises, and every run that never raises must equal its oracle."""
    _lib, envs, sch, QLearningPopulation = _product()
    M, A, L = M_ROWS, 16, 2
    eps_s, lr_s, gamma = _diverging_schedules(M, sch)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=dt,
                              learn_mode=mode)
    env = envs.HashTabularEnv(M, S, A, seed=1, masked=True)
    first_call = {}
    sd, parts = None, []
    for c in range(K // L):
        res, raised = _run_catching(pop, L, env, sd)
        if c == 0:
            _reached(pop, M, L, True, nv=4, masked=True)
        for r in raised:
            first_call.setdefault(r, c)
        parts.append(res)
        sd = res.state_dict
    tables = pop.q_tables
    want_first = {}
    for r in range(M):
        ref = c_oracle.CHashRollout(1, S, A, masked=True, agent_offset=r, gamma=gamma[r], dtype=dt, mode=mode)
        eps, lr = eps_s[r].get_value(), lr_s[r].get_value()
        try:
            want = ref.run(np.full(K, eps), np.full(K, lr))
        except IndexError:
            want_first[r] = ref.failed_step // L
            continue
        assert r not in first_call, f"run {r} raised in call {first_call[r]}, its oracle never"
        assert np.array_equal(tables[r], ref.q, equal_nan=True), f"run {r}: table"
        rets = np.concatenate([p.run_returns(r) for p in parts])
        at = np.concatenate([p.run_steps(r) + L * c for c, p in enumerate(parts)])
        assert np.array_equal(rets, want["history"]), f"run {r}: returns"
        assert np.array_equal(at, want["ep_step"]), f"run {r}: episode steps"
        assert (sd["states"][r], sd["aux"][r], sd["rewards"][r]) == (ref.obs[0], ref.episode[0], ref.acc[0]), r
    differ = {r: (first_call.get(r), want_first.get(r)) for r in set(first_call) | set(want_first)
              if first_call.get(r) != want_first.get(r)}
    assert not differ, f"run: (first raising call, the oracle's): {differ}"
    assert len(want_first) > M // 4 and len(want_first) < M, len(want_first)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_diverging_bandit_runs_match_standalone_runs(dt):
    """The bandit: one state, so every update is an own write; one agent per run takes the list selection, which has
    no candidate once both columns are NaN."""
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    _lib, envs, sch, QLearningPopulation = _product()
    M, K = 70, 400 if dt == np.float32 else 3000
    eps_s, lr_s, gamma = _diverging_schedules(M, sch)

    def bandit(n, off):
        e = envs.RiggedTwoArmedBanditVecEnv(n, episode_len=7)
        e._params.agent_offset = off
        return e

    pop = QLearningPopulation(M, 1, 2, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=3, dtype=dt)
    res, raised = _run_catching(pop, K, bandit(M, 0))
    _reached(pop, M, K, True, nv=1, masked=False)
    tables = pop.q_tables
    want_raised = []
    for r in range(M):
        algo = OptimalQLearningBase(1, 2, gamma[r], seed=3, dtype=dt)
        _lib.check(_lib.load().qe_set_agent_offset(algo.handle, r))
        rt = GpuRolloutQLearning(algo, copy.deepcopy(lr_s[r]), copy.deepcopy(eps_s[r]))
        env = bandit(1, r)
        try:
            mean, history, _, sd1 = rt.run_steps(K, env)
        except IndexError:
            want_raised.append(r)
            continue
        assert np.array_equal(tables[r], np.asarray(algo.q_table), equal_nan=True), f"run {r}: table"
        assert np.array_equal(res.run_returns(r), np.array(history, dtype=np.float32)), f"run {r}: returns"
        assert res.mean_returns[r] == mean, r
        assert (res.state_dict["states"][r], res.state_dict["aux"][r], res.state_dict["rewards"][r]) == (
            sd1["states"][0], sd1["aux"][0], sd1["rewards"][0]), r
    assert raised == want_raised
    assert 0 < len(want_raised) < M, want_raised


# ---- 4. counters and schedules at their edges -----------------------------------------------------------------------
def test_a_step_counter_crossing_2_pow_32_matches_the_c_oracle():
    _lib, envs, _, QLearningPopulation = _product()
    M, S, A, K, step0 = 67, 500, 16, 300, 2**32 - 150
    eps_s, lr_s, gamma = _schedules(M)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=np.float32)
    pop.step_counter = step0
    res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=True))
    _reached(pop, M, K, True, nv=4, masked=True)
    assert pop.step_counter == step0 + K == res.state_dict["rng_step"]
    _check_hash_runs(pop, res, range(M), S, A, True, eps_s, lr_s, gamma, np.float32, "iter", K, step0=step0)


def test_a_step_counter_crossing_2_pow_32_matches_the_numpy_oracle_on_a_table_env():
    """The table environment hashes the step too (``step >> 32`` in its word), unlike the hash environment."""
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp

    _lib, envs, _, QLearningPopulation = _product()
    arrays, isd, masks = random_mdp(300, 9, 3, seed=6, masked=True)
    mdp = encode_table_mdp(*arrays, isd, masks)
    M, K, step0 = 67, 300, 2**32 - 150
    eps_s, lr_s, gamma = _schedules(M)
    pop = QLearningPopulation(M, 300, 9, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=2, dtype=np.float64,
                              learn_mode="vec")
    pop.step_counter = step0
    res = pop.run_steps(K, envs.TabularMDPEnv(M, mdp, seed=3))
    _reached(pop, M, K, True, nv=4, masked=True)
    for r in _sample(M, extra=4, seed=9):
        want, state, e_after, l_after = _table_reference(mdp, r, K, gamma[r], eps_s[r], lr_s[r], np.float64, "vec",
                                                         seed=2, env_seed=3, step0=step0)
        _check_run(pop, res, r, want, table=pop.q_table(r), state=state, eps_after=e_after, lr_after=l_after)


def test_agent_ids_that_wrap_past_2_pow_32_match_the_c_oracle():
    _lib, envs, _, QLearningPopulation = _product()
    M, S, A, K, off = 67, 500, 8, 300, 2**32 - 30  # run r has agent id (off + r) mod 2^32: 2^32 - 30 .. 36
    eps_s, lr_s, gamma = _schedules(M)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=np.float64,
                              learn_mode="vec")
    res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, agent_offset=off))
    _reached(pop, M, K, True, nv=2, masked=False)
    _check_hash_runs(pop, res, range(M), S, A, False, eps_s, lr_s, gamma, np.float64, "vec", K, offset=off)


@pytest.mark.parametrize("log", [True, False])
def test_zero_steps_move_nothing(log):
    _lib, envs, _, QLearningPopulation = _product()
    M, S, A, K = 67, 200, 5, 150
    eps_s, lr_s, gamma = _schedules(M)
    q0 = np.random.default_rng(2).standard_normal((M, S, A)).astype(np.float32)

    def make():
        p = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=np.float32)
        p.set_q_tables(q0)
        return p

    pop = make()
    env = envs.HashTabularEnv(M, S, A, seed=1, masked=True)
    res = pop.run_steps(0, env, log=log)
    _reached(pop, M, 0, log)
    assert np.array_equal(pop.q_tables, q0)
    assert pop.step_counter == 0 == res.state_dict["rng_step"]
    assert not res.episode_counts.any() and np.isnan(res.mean_returns).all()
    assert res.returns.size == 0 and res.steps.size == 0 and not res.offsets.any()
    for r in range(M):
        ref = c_oracle.CHashRollout(1, S, A, masked=True, agent_offset=r)  # its state right after the reset
        assert (res.state_dict["states"][r], res.state_dict["aux"][r], res.state_dict["rewards"][r]) == (
            ref.obs[0], ref.episode[0], ref.acc[0]), r
        eps_r = eps_s[r].get_value()
        assert pop.exploration_rate_schedules[r].get_value() == eps_r == res.state_dict["exploration_rate"][r]
        assert pop.lr_schedules[r].get_value() == lr_s[r].get_value() == res.state_dict["lr"][r]
    after = pop.run_steps(K, env, res.state_dict)
    fresh = make()
    want = fresh.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=True))
    assert np.array_equal(pop.q_tables, fresh.q_tables)
    for a, b in ((after.returns, want.returns), (after.steps, want.steps), (after.episode_counts, want.episode_counts)):
        assert np.array_equal(a, b)
    assert np.array_equal(after.mean_returns, want.mean_returns, equal_nan=True)
    for key in ("states", "aux", "rewards", "lr", "exploration_rate", "rng_step"):
        assert np.array_equal(after.state_dict[key], want.state_dict[key]), key


@pytest.mark.parametrize("case", ["eps_below_0", "eps_above_1", "lr_below_0"])
def test_schedules_that_leave_their_range_match_the_c_oracle(case):
    _lib, envs, sch, QLearningPopulation = _product()
    M, S, A, K = 67, 300, 9, 300
    eps_s, lr_s, gamma = _schedules(M)
    if case == "eps_below_0":  # eps_threshold clamps to 0: greedy once the value is negative
        eps_s = [sch.LinearSchedule(0.05, -0.001 - 1e-6 * r) for r in range(M)]
    elif case == "eps_above_1":  # ... and to 2^32: every draw explores once the value passes 1
        eps_s = [sch.LinearSchedule(0.8, 0.002 + 1e-6 * r) for r in range(M)]
    else:  # a negative learning rate is applied as it is
        lr_s = [sch.LinearSchedule(0.02, -1e-4) for _ in range(M)]
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=np.float64)
    res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1, masked=True))
    _reached(pop, M, K, True, nv=4, masked=True)
    values = (res.state_dict["exploration_rate"] if case != "lr_below_0" else res.state_dict["lr"])
    assert (values < 0).all() if case != "eps_above_1" else (values > 1).all()
    _check_hash_runs(pop, res, range(M), S, A, True, eps_s, lr_s, gamma, np.float64, "iter", K)


# ---- 5. a table of more than 2^31 cells -----------------------------------------------------------------------------
def test_a_table_of_more_than_2_pow_31_cells_matches_the_c_oracle():
    import ctypes as C

    _product()[0].load()  # (the engine library brings the HIP runtime in)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert C.CDLL("libamdhip64.so").hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    free = free.value
    if free < 16 * 2**30:
        pytest.skip(f"needs 16 GiB of free device memory for a 8.7 GB table, {free / 2**30:.1f} GiB free")
    _lib, envs, _, QLearningPopulation = _product()
    M, S, A, K = 66_000, 8200, 3, 300  # ld = 4: 2.16e9 cells; run 65 472 straddles cell 2^31, 65 473 lies past it
    assert M * S * 4 > 2**31 and 65_472 * S * 4 < 2**31 < 65_473 * S * 4
    eps_s, lr_s, gamma = _cycled_schedules(M)
    pop = QLearningPopulation(M, S, A, gamma, copy.deepcopy(lr_s), copy.deepcopy(eps_s), seed=0, dtype=np.float32)
    res = pop.run_steps(K, envs.HashTabularEnv(M, S, A, seed=1))
    _reached(pop, M, K, True, nv=1, masked=False)
    runs = [0, 1, 20_000, 65_471, 65_472, 65_473, 65_474, 65_535, 65_536, 65_999]
    _check_hash_runs(pop, res, runs, S, A, False, eps_s, lr_s, gamma, np.float32, "iter", K)
