"""CPU: the NumPy model of the dynamic-programming entry points (``mdp_solver_model``) against what it must equal --
the sampling rule, closed forms, a dense linear solve and the Bellman optimality equation."""

import numpy as np

import mdp_solver_model as model
from dist_classicrl_amd.environments.device_envs import TableMDP, encode_table_mdp
from table_mdp_model import random_mdp

TWO32 = 1 << 32
EPS = np.finfo(np.float64).eps


def _raw_mdp(thr_rows):
    """One state, one cell per row of thresholds (the last slot's threshold is 2**32 - 1, as the device stores it)."""
    thr = np.array(thr_rows, dtype=np.uint32)[None]
    shape = thr.shape
    return TableMDP(thr, np.zeros(shape, np.int32), np.zeros(shape, np.float32), np.zeros(shape, bool),
                    np.array([0xFFFFFFFF], np.uint32), np.array([0], np.int32), None)


def _measure(thr_row):
    """How many 32-bit words the sampling rule sends to each slot: the rule is constant between neighbouring
    thresholds, so one probe per interval counts them all."""
    cuts = sorted({0, TWO32, *(int(t) for t in thr_row[:-1])})
    count = [0] * len(thr_row)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        count[model.sample_slot(thr_row, lo)] += hi - lo
    return count


def test_weights_reproduce_the_sampling_rule():
    top = 0xFFFFFFFF
    cells = {
        1: [[top]],
        2: [[0, top], [1, top], [top, top], [0x80000000, top], [top - 1, top]],
        3: [[5, 5, top], [9, 3, top], [0, 0, top], [1, top, top], [top, 7, top], [0x40000000, 0xC0000000, top]],
        4: [[10, 20, 30, top], [30, 20, 10, top], [7, 7, 9, top], [0, top, top, top], [top, top, top, top],
            [3, 1, 4, top]],
    }
    for k, rows in cells.items():
        w = _raw_mdp(rows).outcome_weights()[0]
        assert w.dtype == np.uint64 and w.shape == (len(rows), k)
        for row, got in zip(rows, w.tolist()):
            assert got == _measure(row), (row, got)
            assert sum(got) == TWO32
            # every probe around every threshold lands in the slot whose weight says it can be taken
            for t in row:
                for u in {0, max(t - 1, 0), t, min(t + 1, top), top}:
                    j = model.sample_slot(row, u)
                    assert got[j] > 0, (row, u, j)
                    lo = sum(x for x in got[:j])  # slots are taken in threshold order only when thresholds ascend
                    if sorted(row) == list(row):
                        assert lo <= u < lo + got[j], (row, u, j)
    # the start support is weighed by the same rule
    mdp = _raw_mdp([[top]])._replace(start_thr=np.array([100, 100, 4000, top], np.uint32), start_state=np.zeros(4, np.int32))
    assert mdp.start_weights().tolist() == [100, 0, 3900, TWO32 - 4000]


def test_padding_copies_sum_to_the_last_outcomes_mass():
    probs = np.array([[[0.25, 0.0, 0.75, 0.0], [0.5, 0.25, 0.125, 0.125]]])  # cell 0: two outcomes in four slots
    nxt = np.zeros(probs.shape, dtype=np.int64)
    rew = np.arange(8, dtype=np.float64).reshape(probs.shape)
    mdp = encode_table_mdp(probs, nxt, rew, np.zeros(probs.shape, bool))
    w = mdp.outcome_weights()
    assert w.sum(axis=-1).tolist() == [[TWO32, TWO32]]
    assert w[0, 0, 0] == TWO32 // 4
    # slots 1, 2, 3 of cell 0 are the last outcome and its copies: together its mass, the same reward each
    assert mdp.reward[0, 0].tolist() == [0.0, 2.0, 2.0, 2.0] and int(w[0, 0, 1:].sum()) == 3 * TWO32 // 4
    assert w[0, 1].tolist() == [TWO32 // 2, TWO32 // 4, TWO32 // 8, TWO32 // 8]
    law = model.law_of(mdp)
    assert np.array_equal(model.backup(law, np.zeros(1), 0.5), [[1.5, 4.0 * 0.5 + 5.0 * 0.25 + 6.0 * 0.125 + 7.0 * 0.125]])


def test_terminating_chain_converges_in_length_plus_one_sweeps_to_the_closed_form():
    for L in (1, 2, 9, 40):
        mdp, r = model.chain_mdp(L)
        sol = model.value_iteration(mdp, 0.5, tol=0.0, max_sweeps=1000)
        assert (sol.sweeps, sol.residual, sol.converged) == (L + 1, 0.0, True)
        v = np.zeros(L + 1)
        for s in range(L - 1, -1, -1):  # dyadic: every sum below is exact in float64
            v[s] = r[s] + 0.5 * v[s + 1]
        assert np.array_equal(sol.v, v[:L])
        assert np.array_equal(sol.q, np.stack([r + 0.5 * v[1:], r - 1.0 + 0.5 * v[1:]], axis=1))
        assert model.start_value(mdp, sol.v) == v[0]
        short = model.value_iteration(mdp, 0.5, tol=0.0, max_sweeps=L)
        assert (short.sweeps, short.converged) == (L, False) and np.array_equal(short.v, v[:L]) and short.residual > 0.0


def _random(S=30, A=4, K=3, seed=5, masked=True):
    arrays, isd, masks = random_mdp(S, A, K, seed, masked=masked, start_support=min(7, S))
    return encode_table_mdp(*arrays, isd, masks)


def test_policy_evaluation_agrees_with_a_dense_linear_solve():
    """Measured on this MDP, six runs: differences 4.7e-12 .. 7.5e-12 against bounds of 8.1e-12 .. 8.7e-12 (residuals
    9.0e-13 .. 9.6e-13): the contraction term carries the bound, the factor 64 was not widened."""
    mdp = _random(masked=False)
    law = model.law_of(mdp)
    S, A, K = law.w.shape
    rng = np.random.default_rng(11)
    tables = rng.integers(0, 2, size=(6, S, A)).astype(np.float64)  # two levels: ties in most rows
    gamma, tol = 0.9, 1e-12
    got = model.policy_values(mdp, tables, gamma, tol=tol, max_sweeps=10_000, law=law)
    assert got.converged.all() and (got.status == 0).all() and (got.sweeps > 1).all()
    G, _ = model.tie_sets(law, tables)
    assert (G.sum(axis=-1) >= 2).mean() > 0.5
    for r in range(tables.shape[0]):
        pi = G[r] / G[r].sum(axis=-1, keepdims=True)
        P = np.zeros((S, S))
        rew = np.zeros(S)
        for s in range(S):
            for a in range(A):
                for j in range(K):
                    rew[s] += pi[s, a] * law.p[s, a, j] * law.r[s, a, j]
                    if not law.term[s, a, j]:
                        P[s, law.nxt[s, a, j]] += pi[s, a] * law.p[s, a, j]
        M = np.eye(S) - gamma * P
        want = np.linalg.solve(M, rew)
        # The iterate is within res * gamma / (1 - gamma) of the fixed point (contraction).  The solve's own rounding:
        # LU with partial pivoting is backward stable, so its error is about cond(M) * eps * |V| with a modest growth
        # constant; M = I - gamma * P with P substochastic has cond_inf <= (1 + gamma) / (1 - gamma) = 19.  64 covers
        # that condition number, the rounding of P and rew as assembled above, and the sweeps' own rounding (a few eps
        # per sweep, amplified by at most 1 / (1 - gamma) = 10).
        assert np.linalg.cond(M, np.inf) <= 19.0 * (1 + 1e-12)
        bound = got.residuals[r] * gamma / (1.0 - gamma) + 64 * EPS * np.max(np.abs(want))
        diff = np.max(np.abs(got.values[r] - want))
        print(f"run {r}: |model - solve| = {diff:.3e}, bound {bound:.3e}, residual {got.residuals[r]:.3e}")
        assert diff <= bound, (r, diff, bound)


def test_value_iteration_fixed_point_satisfies_the_bellman_optimality_equation():
    for masked in (False, True):
        mdp = _random(masked=masked)
        law = model.law_of(mdp)
        gamma = 0.9
        sol = model.value_iteration(mdp, gamma, tol=1e-12, max_sweeps=10_000, law=law)
        assert sol.converged and 1 < sol.sweeps < 10_000
        q = model.backup(law, sol.v, gamma)
        best = np.where(law.valid, q, -np.inf).max(axis=1)
        bound = sol.residual * gamma / (1.0 - gamma) + 64 * EPS * np.max(np.abs(sol.v))
        assert np.max(np.abs(best - sol.v)) <= bound
        # and V is the maximum of the returned Q over the valid columns, exactly
        assert np.array_equal(np.where(law.valid, sol.q, -np.inf).max(axis=1), sol.v)


def test_policy_values_freeze_runs_one_by_one_and_flag_nan_and_dead_ends():
    mdp = _random()
    masks = mdp.masks.copy()
    masks[3] = False  # a dead end
    mdp = mdp._replace(masks=masks)
    law = model.law_of(mdp)
    S, A, _ = law.w.shape
    tables = np.random.default_rng(2).integers(0, 4, size=(4, S, A)).astype(np.float32)
    tables[2, 5, int(np.flatnonzero(masks[5])[0])] = np.nan      # valid cell: the run is NaN
    tables[1, 5, :][~masks[5]] = np.nan                          # masked-out cells: no effect
    gammas = np.array([0.0, 0.5, 0.5, 0.999])
    got = model.policy_values(mdp, tables, gammas, tol=1e-9, max_sweeps=50, law=law)
    assert got.status.tolist() == [1, 1, 3, 1]
    assert got.sweeps[0] == 2 and got.sweeps[2] == 0 and got.sweeps[3] == 50 and 2 < got.sweeps[1] < 50
    assert got.converged.tolist() == [True, True, False, False]
    assert np.isnan(got.values[2]).all() and np.isnan(got.residuals[2]) and not np.isnan(got.values[[0, 1, 3]]).any()
    assert (got.values[:, 3][[0, 1, 3]] == 0.0).all()
    clean = tables.copy()
    clean[1, 5, :][~masks[5]] = 0.0
    again = model.policy_values(mdp, clean, gammas, tol=1e-9, max_sweeps=50, law=law)
    assert np.array_equal(again.values[1], got.values[1])
    # a frozen run's values are those of a call that stops at its freeze sweep
    short = model.policy_values(mdp, tables, gammas, tol=1e-9, max_sweeps=int(got.sweeps[1]), law=law)
    assert np.array_equal(short.values[1], got.values[1]) and short.sweeps[1] == got.sweeps[1]
