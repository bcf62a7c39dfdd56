"""Case tables shared by ``make_golden.py`` (generator, needs the reference) and the tests."""

SELECT_CASES = [
    # (method, S, A, n, masked, eps, deterministic, dtype)
    ("choose_actions", 100, 4, 1, False, 0.3, False, "f8"),  # -> choose_actions_iter (C1 train)
    ("choose_actions", 1000, 8, 128, False, 0.1, False, "f8"),  # -> choose_actions_vec (C2 train)
    ("choose_actions", 1000, 16, 300, False, 0.5, False, "f4"),  # -> choose_actions_vec (C3 train)
    ("choose_actions", 200, 128, 150, False, 0.2, False, "f8"),  # -> choose_actions_vec_iter
    ("choose_actions", 300, 9, 64, True, 0.3, False, "f8"),  # -> masked iter (TicTacToe shape)
    ("choose_actions", 500, 64, 200, True, 0.25, False, "f4"),  # -> masked vec_iter (C5 train)
    ("choose_actions", 100, 8, 50, False, 0.0, True, "f8"),  # eval -> iter
    ("choose_actions", 100, 16, 70, False, 0.0, True, "f4"),  # eval -> choose_actions_vec
    ("choose_actions", 100, 64, 70, True, 0.0, True, "f8"),  # eval -> choose_masked_actions_vec
    ("choose_actions_iter", 50, 6, 40, False, 0.4, False, "f8"),
    ("choose_actions_iter", 50, 6, 40, True, 0.4, False, "f8"),
    ("choose_actions_vec_iter", 50, 12, 40, False, 0.4, False, "f8"),
    ("choose_actions_vec_iter", 50, 12, 40, True, 0.4, False, "f4"),
    ("choose_actions_vec", 50, 12, 40, False, 0.4, False, "f8"),
    ("choose_actions_vec", 50, 5, 33, False, 1.0, False, "f8"),  # everyone explores, odd A
    ("choose_masked_actions_vec", 50, 12, 40, True, 0.4, False, "f8"),
    ("choose_masked_actions_vec", 50, 260, 10, True, 0.4, False, "f4"),  # A > 256
    ("choose_actions_vec", 20, 1000, 6, False, 0.2, False, "f8"),  # large A
]

LEARN_CASES = [
    # (S, A, n, masked, dtype, lr, gamma)
    (40, 4, 64, False, "f8", 0.1, 0.99),
    (40, 4, 64, False, "f4", 0.1, 0.99),
    (30, 16, 200, False, "f8", 0.5, 0.9),
    (30, 16, 200, False, "f4", 0.5, 0.9),
    (25, 64, 100, True, "f8", 0.3, 0.97),
    (25, 64, 100, True, "f4", 0.3, 0.97),
    (1, 2, 32, False, "f4", 1.0, 1.0),  # bandit shape: every transition depends on the previous
    (5000, 8, 128, False, "f4", 0.1, 0.99),  # sparse: almost no collisions
    (60, 9, 90, True, "f8", 0.2, 0.95),  # A not a multiple of 4
]

TRACE_CASES = [
    # (name, env spec, steps, dtype, schedule kind, learn fn)
    ("c1_grid_n1", ("grid", 1, 10), 80, "f8", "bench", "learn"),
    ("grid4_n1", ("grid", 1, 4), 300, "f8", "bench", "learn"),
    ("grid4_n16", ("grid", 16, 4), 100, "f4", "const", "learn"),
    ("grid4_n16_f8", ("grid", 16, 4), 100, "f8", "const", "learn"),
    ("c2_hash_n128", ("hash", 128, 10000, 8, False), 50, "f4", "bench", "learn"),
    ("c2_hash_n128_const", ("hash", 128, 10000, 8, False), 50, "f4", "const", "learn"),
    ("hash_dense_n256", ("hash", 256, 64, 16, False), 40, "f4", "const", "learn"),
    ("hash_dense_n256_f8", ("hash", 256, 64, 16, False), 40, "f8", "const", "learn"),
    ("hash_dense_n256_vec", ("hash", 256, 64, 16, False), 40, "f8", "const", "learn_vec"),
    ("c5_hash_masked_n128", ("hash", 128, 500, 64, True), 40, "f4", "const", "learn"),
    ("hash_masked_a9_n64", ("hash", 64, 300, 9, True), 40, "f8", "const", "learn"),
    ("bandit_n4", ("bandit", 4, 5), 23, "f8", "kat", "learn"),
    ("bandit_n128", ("bandit", 128, 7), 30, "f4", "const", "learn"),
    ("ttt_n64", ("ttt", 64), 60, "f8", "bench", "learn"),  # masked, A = 9: choose_masked_action (list) path
    ("ttt_n128_f4", ("ttt", 128), 50, "f4", "const", "learn"),
]

# ---- round 3 (make_golden_r3.py) -----------------------------------------------------------------------------------
SCALE_TRACE_CASES = [
    # the shapes SURVEY 8(c) lists beyond 256 agents
    ("c3_shrunk_n4096", ("hash", 4096, 1_000_000, 16, False), 30, "f4", "bench", "learn"),
    ("c3_shrunk_n4096_const", ("hash", 4096, 1_000_000, 16, False), 20, "f4", "const", "learn"),
    ("c5_small_n1024", ("hash", 1024, 4096, 64, True), 30, "f4", "const", "learn"),
    ("c5_small_n1024_bench", ("hash", 1024, 4096, 64, True), 20, "f4", "bench", "learn"),
]

NAN_SELECT_CASES = [
    # (method, S, A, n, masked, eps, deterministic, dtype, NaN cells, table seed)
    ("choose_actions_iter", 40, 6, 60, False, 0.3, False, "f4", 30, 1),     # list scan steps over NaN
    ("choose_actions_iter", 40, 6, 60, True, 0.3, False, "f8", 60, 2),
    ("choose_actions_iter", 12, 4, 40, False, 0.0, True, "f4", 30, 3),      # rows that are NaN throughout: -1
    ("choose_actions_vec_iter", 400, 12, 30, False, 1.0, False, "f4", 40, 4),  # everyone explores: no maximum taken
    ("choose_actions_vec_iter", 4000, 12, 8, False, 0.3, False, "f4", 3, 5),
    ("choose_actions_vec_iter", 40, 12, 30, False, 0.3, False, "f4", 40, 6),   # IndexError
    ("choose_actions_vec_iter", 4000, 12, 8, True, 0.3, False, "f8", 3, 7),
    ("choose_actions_vec", 400, 8, 120, False, 1.0, False, "f4", 30, 8),
    ("choose_actions_vec", 40, 8, 120, False, 0.2, False, "f4", 6, 9),        # IndexError
    ("choose_actions_vec", 90000, 8, 120, False, 0.2, False, "f4", 2, 10),
    ("choose_masked_actions_vec", 40, 12, 50, True, 0.2, False, "f4", 10, 11),  # IndexError unless the NaN is masked out
    ("choose_masked_actions_vec", 20000, 12, 50, True, 0.2, False, "f8", 4, 12),
    ("choose_actions", 50, 8, 64, False, 0.2, False, "f4", 20, 13),            # n < 100 -> list variant
    ("choose_actions", 50, 8, 128, False, 0.2, False, "f4", 4, 14),            # n >= 100 -> NumPy variant (IndexError)
    ("choose_actions", 50, 9, 128, True, 0.2, False, "f4", 20, 15),            # masked, A <= 10 -> list
    ("choose_actions", 50, 16, 128, True, 0.2, False, "f4", 4, 16),            # masked, A > 10 -> NumPy (IndexError)
    ("choose_actions", 50, 8, 128, False, 0.0, True, "f4", 20, 17),            # deterministic, A <= 10 -> list
    ("choose_actions", 50, 16, 128, False, 0.0, True, "f4", 4, 18),            # deterministic, A > 10 -> NumPy
]

NAN_LEARN_CASES = [
    # (S, A, n, masked, dtype, lr, gamma, NaN cells, table seed)
    (40, 4, 64, False, "f4", 0.1, 0.99, 8, 1),
    (40, 4, 64, False, "f8", 0.1, 0.99, 8, 2),
    (30, 16, 200, False, "f4", 0.5, 0.9, 20, 3),
    (25, 64, 100, True, "f4", 0.3, 0.97, 40, 4),   # a masked-out NaN does not reach the target
    (60, 9, 90, True, "f8", 0.2, 0.95, 25, 5),
    (5000, 8, 128, False, "f4", 0.1, 0.99, 300, 6),
]

NAN_TRACE_CASES = [
    # (name, env spec, chunks, dtype, schedule kind, learn fn, NaN cells (0: zero table), table seed)
    ("diverge_bandit_n600_vec", ("bandit", 600, 5), [10] * 6, "f4", "nan", "learn_vec", 0, 0),
    ("diverge_hash_n600_vec", ("hash", 600, 4, 4, False), [8] * 6, "f4", "nan", "learn_vec", 0, 0),
    ("diverge_hash_n256_masked_vec", ("hash", 256, 5, 16, True), [8] * 6, "f4", "nan", "learn_vec", 0, 0),
    ("nan_explore_n200", ("hash", 200, 50, 8, False), [10, 10, 10], "f4", "explore", "learn", 40, 3),
    ("nan_raise_n200", ("hash", 200, 2000, 8, False), [3, 3, 3, 3], "f4", "const", "learn", 4, 5),
    ("nan_raise_n1024", ("hash", 1024, 30000, 16, False), [3, 3, 3, 3], "f4", "const", "learn", 6, 5),
    ("nan_list_n64", ("hash", 64, 50, 8, False), [4, 4, 4], "f4", "const", "learn", 6, 4),
    ("nan_list_masked_a8", ("hash", 128, 300, 8, True), [5, 5], "f4", "const", "learn", 20, 4),
    ("nan_raise_masked_a16", ("hash", 128, 3000, 16, True), [3, 3, 3, 3], "f4", "const", "learn", 6, 3),
    ("nan_lean_n128", ("hash", 128, 2000, 16, False), [20, 20, 20, 20], "f4", "const", "learn", 1, 4),
    ("nan_ttt_n128", ("ttt", 128), [10, 10], "f4", "const", "learn", 300, 3),
]

# ---- greedy evaluation and train() (make_golden_eval.py) ---------------------------------------------------------------
# Shared by the generator (needs the reference) and by tests/test_oracle_eval_golden.py / tests/test_gpu_eval_parity.py,
# which import these tables and constructions from here: there is no second copy to keep in step.
import numpy as np  # noqa: E402


def tie_rich_table(seed, S, A, dt):
    """``make_golden.py:_tie_rich_table`` on ``default_rng(seed)``: Q-values from a tiny value set so that arg-max ties
    are common; some all-zero rows."""
    rng = np.random.default_rng(seed)
    q = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, -0.5]), size=(S, A)).astype(dt)
    q[rng.random(S) < 0.2] = 0
    return q


def nan_table(S, A, dt, cells, seed):
    """``make_golden_r3.py:nan_table``: a random table with `cells` NaN entries."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((S, A)).astype(dt)
    if cells:
        q.ravel()[rng.choice(S * A, size=cells, replace=False)] = np.nan
    return q


def eval_table(table, S, A, dt, valid=None):
    """The initial table of an evaluation case.  ``table`` is ("tie", seed), ("zero",), ("nan", cells, seed),
    ("nan_rows", cells, seed, every): as "nan" with every `every`-th row NaN throughout, or ("nan_masked", seed): a
    tie-rich table with NaN in half of the cells whose action the environment's mask of that state clears (`valid`:
    bool[S, A], the mask of every state)."""
    kind = table[0]
    if kind == "tie":
        return tie_rich_table(table[1], S, A, dt)
    if kind == "zero":
        return np.zeros((S, A), dtype=dt)
    if kind == "nan":
        return nan_table(S, A, dt, table[1], table[2])
    if kind == "nan_rows":
        q = nan_table(S, A, dt, table[1], table[2])
        q[::table[3]] = np.nan
        return q
    assert kind == "nan_masked" and valid is not None
    q = tie_rich_table(table[1], S, A, dt)
    q[~valid & (np.random.default_rng(table[1] + 1).random((S, A)) < 0.5)] = np.nan
    return q


def table_print(q):
    """Fingerprint of a table's bit patterns (two uint64 words): the goldens store it next to results computed from a
    table that the tests rebuild from its seed, so that a construction that drifts is noticed as such."""
    bits = np.ascontiguousarray(q).view(np.uint32 if q.dtype.itemsize == 4 else np.uint64).ravel().astype(np.uint64)
    weights = np.arange(1, bits.size + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return np.array([np.bitwise_xor.reduce(bits * weights), np.add.reduce(bits ^ weights)], dtype=np.uint64)


EVAL_SEED = 0  # policy draw seed of every golden evaluation / train case

EVAL_CASES = [
    # (name, env spec (oracle.envs.make_env), dtype, table, start step, vector steps of the steps-mode call (steps = that x agents + extra),
    #  extra, episode target (None: steps mode only), raises)
    # -- the shapes: both modes each; the smallest that reach each branch.  (A sixth spec entry is the termination rate in
    #    256ths, default 13: lowered where many agents would otherwise fill the file with episode returns.)
    # (one action: the walk is a fixed cycle, which at the default termination rate holds no terminal state; 64/256 here)
    ("hash_n1_a1", ("hash", 1, 50, 1, False, 64), "f4", ("tie", 11), 3, 700, 0, 70, False),       # single action, single agent
    ("hash_n63_a4_f8", ("hash", 63, 200, 4, False), "f8", ("tie", 12), 0, 40, 0, 393, False),     # L = 1, partial wavefront
    ("hash_n65_a5", ("hash", 65, 200, 5, False), "f4", ("tie", 13), 17, 40, 0, 200, False),       # L = 2, padded row
    ("hash_masked_n100_a9_f8", ("hash", 100, 300, 9, True, 6), "f8", ("tie", 14), 5, 40, 0, 740, False),  # L = 4, list
    ("hash_n128_a10", ("hash", 128, 300, 10, False, 6), "f4", ("tie", 15), 0, 40, 0, 1121, False),   # last list-variant width
    ("hash_n128_a11", ("hash", 128, 300, 11, False, 6), "f4", ("tie", 16), 9, 40, 0, 608, False),   # first NumPy-variant width
    ("hash_masked_n257_a16", ("hash", 257, 500, 16, True, 3), "f4", ("tie", 17), 0, 40, 0, 706, False),  # agents % groups
    ("hash_n300_a33_f8", ("hash", 300, 400, 33, False, 3), "f8", ("tie", 18), 100, 40, 0, 733, False),   # L = 16, padded
    ("hash_masked_n96_a64", ("hash", 96, 300, 64, True), "f4", ("tie", 19), 0, 40, 0, 854, False),     # the c5 width
    ("hash_n70_a100", ("hash", 70, 100, 100, False), "f4", ("tie", 20), 1000, 40, 0, 726, False),      # L = 32
    ("hash_masked_n40_a256_f8", ("hash", 40, 60, 256, True), "f8", ("tie", 21), 0, 60, 0, 465, False),  # L = 64
    ("hash_n1000_a16_zero", ("hash", 1000, 64, 16, False, 4), "f4", ("zero",), 0, 30, 0, 2633, False),  # every pick a full tie
    ("ttt_n90", ("ttt", 90), "f4", ("tie", 22), 0, 40, 0, 4689, False),                   # masked list variant, env state
    ("grid4_n16_f8", ("grid", 16, 4), "f8", ("tie", 43), 0, 200, 0, None, False),         # steps mode only
    ("bandit_n130", ("bandit", 130, 7), "f4", ("tie", 24), 0, 40, 0, 130 * 27 + 1, False),  # all finish in one step: log order
    # -- the step word crosses 2**32 during the call (k_eval hands step >> 32 to Philox)
    ("hash_n128_a16_step32", ("hash", 128, 300, 16, False, 6), "f4", ("tie", 25), 2**32 - 20, 40, 0, 751, False),
    # -- steps = 30 * n + 1: ceil(steps / n) = 31 vector steps
    ("hash_n96_a8_ceil", ("hash", 96, 300, 8, False), "f4", ("tie", 26), 0, 30, 1, None, False),
    # -- NaN tables
    # (steps mode only: without ties the greedy walks of a random table end in cycles that hold no terminal state)
    ("nan_list_a8", ("hash", 64, 300, 8, False), "f4", ("nan", 300, 31), 0, 40, 0, None, False),    # list variant steps over NaN
    ("nan_allrow_a8", ("hash", 64, 300, 8, False), "f4", ("nan_rows", 300, 32, 5), 0, 40, 0, 620, True),  # a row without candidate
    ("nan_max_a16", ("hash", 64, 300, 16, False), "f4", ("nan", 200, 33), 0, 40, 0, 620, True),     # np.max propagates
    ("nan_masked_out_a16", ("hash", 64, 300, 16, True), "f4", ("nan_masked", 34), 0, 40, 0, 548, False),  # NaN never valid
]

TRAIN_CASES = [
    # (name, env spec, validation agents, dtype, schedule kind, learn fn, steps, val_every_n_steps, ("steps" | "episodes", count))
    ("hash_n96_a8_bench", ("hash", 96, 500, 8, False), 40, "f4", "bench", "learn", 50, 16, ("steps", 40 * 30)),      # fused short calls
    ("hash_masked_n64_a9_f8", ("hash", 64, 300, 9, True), 100, "f8", "const", "learn", 45, 20, ("episodes", 150)),  # not fused
    ("ttt_n64", ("ttt", 64), 24, "f4", "const", "learn", 40, 15, ("episodes", 60)),
    ("bandit_n4_f8_kat", ("bandit", 4, 5), 6, "f8", "kat", "learn", 35, 12, ("steps", 6 * 12)),
    ("hash_n128_a16_vec", ("hash", 128, 64, 16, False), 200, "f8", "const", "learn_vec", 35, 12, ("steps", 200 * 25)),
]
