"""Inputs of the wide-row tests (rows of more than 64 actions), built without a device.

Above 64 actions the engine stops padding a row to a power of two (``ld = 4 * ceil(A / 4)``), serves it with 32 lanes
(ld 68..128) or 64 lanes (ld 132..256) of which some hold no column at all, and runs the generic-width build of every
kernel; above 256 it switches to the one-wavefront-per-row kernels with their 64-column sweeps.  ``MID`` and ``LARGE``
are the widths at which that code can go wrong: partial last lanes, whole lanes beyond the row, mask-word edges, sweep
edges and the last width before each switch.

Three families of cases, each a plain dict / tuple:

* ``select_cases(A)``  -- the unfused ``choose_action*`` entry points (a rotation of the small axes over the widths);
* ``learn_cases(A)``   -- ``learn`` / ``learn_vec`` batches on at most four written states;
* ``ROLLOUTS``         -- closed loops (hash and table-driven environments, NaN start tables).

``run_*_oracle`` evaluates a case on the NumPy oracle (cached: the CPU module, the golden module and the GPU module share
one evaluation); ``call_select`` / ``call_learn`` drive ANY implementation of the reference's interface with a case, so
the oracle, the real reference (tests/golden/make_wide_rows.py) and the product are called by the same lines.
tests/test_wide_row_cases.py asserts on the oracle alone that the cases test something.
"""

from __future__ import annotations

import functools
import zlib

import numpy as np

from helpers import make_oracle_env, run_oracle_chunks
from oracle.draws import InjectedDraws, epsilon_threshold, policy_draws
from oracle.qlearn_oracle import OracleQLearning

MID = (65, 68, 96, 97, 127, 128, 129, 191, 255, 256)
LARGE = (257, 260, 319, 320, 321, 384, 385, 513, 1000)
WIDTHS = MID + LARGE
DTYPES = ("f4", "f8")
# the widths whose selection and learn cases are also pinned to the real reference (tests/golden/wide_rows.npz): one per
# lane-group width and one large
GOLDEN_WIDTHS = (97, 191, 321)

# ------------------------------------------------------------------------------- tables
S_ROWS = 12
(ROW_MAX_LAST, ROW_TIE_ENDS, ROW_ONE_PER_SWEEP, ROW_NEG_INF, ROW_ONE_NAN, ROW_ALL_NAN, ROW_DENSE, ROW_POS_INF,
 ROW_HALF_NEG_INF, ROW_LAST_LANE, ROW_ZERO, ROW_SPARSE) = range(S_ROWS)
# rows whose every cell is finite: the only ones a learn case writes, the only next rows of its live transitions
FINITE_ROWS = (ROW_MAX_LAST, ROW_TIE_ENDS, ROW_ONE_PER_SWEEP, ROW_DENSE, ROW_LAST_LANE, ROW_ZERO, ROW_SPARSE)
ROW_POOLS = {
    "all": tuple(range(S_ROWS)),
    "finite": tuple(r for r in range(S_ROWS) if r not in (ROW_ONE_NAN, ROW_ALL_NAN)),  # no NaN (infinities stay)
    "nan_off": tuple(r for r in range(S_ROWS) if r != ROW_ALL_NAN),  # ROW_ONE_NAN with its NaN column masked out
}


def row_stride(A):
    """``row_stride()`` of the engine for A > 64."""
    return 4 * ((A + 3) // 4)


def lanes_per_row(A):
    """Lanes that serve one row, 65 <= A <= 256."""
    return 32 if row_stride(A) <= 128 else 64


def groups_per_block(A):
    """``ngrp`` of the ordered path: lane groups in its 1024-thread block."""
    return 1024 // lanes_per_row(A)


def nan_col(A):
    """The column of ROW_ONE_NAN's NaN (the mask cases switch it on and off)."""
    return A - 3


def last_lane_start(A):
    return 4 * ((A - 1) // 4)


def wide_table(A, dt):
    """The 12-row table of the selection and learn cases: values from {0, 1, 2, +-inf, NaN}, one row per kind."""
    rng = np.random.default_rng(9000 + A)
    q = rng.integers(0, 3, size=(S_ROWS, A)).astype(np.float64)  # ROW_DENSE, and the base of the others: ties of ~A/3
    q[ROW_MAX_LAST] = 0
    q[ROW_MAX_LAST, A - 1] = 2
    q[ROW_TIE_ENDS] = 0
    q[ROW_TIE_ENDS, [0, A - 1]] = 2
    q[ROW_ONE_PER_SWEEP] = rng.integers(0, 2, size=A)
    for c0 in range(0, A, 64):  # exactly one maximum in every 64-column sweep
        q[ROW_ONE_PER_SWEEP, c0 + rng.integers(min(64, A - c0))] = 2
    q[ROW_NEG_INF] = -np.inf
    q[ROW_ONE_NAN, nan_col(A)] = np.nan
    q[ROW_ALL_NAN] = np.nan
    q[ROW_POS_INF, [1, A - 1, int(rng.integers(2, A - 1))]] = np.inf
    q[ROW_HALF_NEG_INF] = np.where(rng.random(A) < 0.5, -np.inf, rng.integers(0, 2, size=A))
    q[ROW_LAST_LANE] = 0
    q[ROW_LAST_LANE, last_lane_start(A):] = 1
    q[ROW_ZERO] = 0
    q[ROW_SPARSE] = np.where(rng.random(A) < 0.125, 2, rng.integers(0, 2, size=A))
    q[ROW_SPARSE, [int(rng.integers(0, 64)), A - 1 - int(rng.integers(0, min(64, A - 64)))]] = 2
    return q.astype(np.dtype(dt))


def rollout_table(S, A, dt, nan_cells=0):
    """Start table of the closed loops: {0, 1, 2} everywhere (the greedy picks are partial ties spread over the whole
    row), every seventh row with its maximum only in column A - 1, tied between the two ends, or one per sweep."""
    rng = np.random.default_rng(7000 + 31 * S + A)
    q = rng.integers(0, 3, size=(S, A)).astype(np.float64)
    q[0::7] = 0
    q[0::7, A - 1] = 2
    q[1::7] = 0
    q[1::7, 0] = q[1::7, A - 1] = 2
    q[2::7] = rng.integers(0, 2, size=q[2::7].shape)
    for c0 in range(0, A, 64):
        q[2::7, c0 + int(rng.integers(min(64, A - c0)))] = 2
    if nan_cells:
        q.ravel()[rng.choice(S * A, size=nan_cells, replace=False)] = np.nan
    return q.astype(np.dtype(dt))


def table_fingerprint(q):
    """CRC-32 of the table's bytes: a golden file stores the builder's arguments and this, not the table."""
    return zlib.crc32(np.ascontiguousarray(q).view(np.uint8).ravel().tobytes())


# ------------------------------------------------------------------------------- masks
MASK_KINDS = ("half", "last", "hi", "half+empty")


def build_masks(kind, n, A, seed, nan_valid=None):
    """int8[n, A].  "half": random, half density, at least one valid column; "last": only column A - 1; "hi": only columns
    >= 64; "+empty": all-zero rows for agent 0, a middle agent and the last agent.  `nan_valid` (half kinds): whether
    column nan_col(A) is valid."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, A), dtype=np.int8)
    if kind.startswith("half"):
        m[:] = rng.random((n, A)) < 0.5
        m[np.arange(n), rng.integers(A, size=n)] = 1
        if nan_valid is not None:
            m[:, nan_col(A)] = int(nan_valid)
            m[:, A - 1] |= m.sum(axis=1) == 0
    elif kind == "last":
        m[:, A - 1] = 1
    else:
        assert kind == "hi"
        m[:, 64:] = 1
    if kind.endswith("+empty"):
        m[[0, n // 2, n - 1]] = 0
    return m


# ------------------------------------------------------------------------------- unfused selection
ENTRIES = ("choose_actions", "choose_actions_iter", "choose_actions_vec_iter", "choose_actions_vec",
           "choose_masked_actions_vec", "single")
EPS = (0.0, 0.3, 1.0)
AGENTS = (1, 4, 5, 8, 9, 99, 100, 101)  # 4 and 8 lane groups per 256-thread block plus one; the dispatcher's 100
STEP_COUNTERS = (3, 2**32 - 1, 2**32 + 5)
SINGLE_CALLS = 12
OFFSET_NEAR_WRAP = 2**32 - 4  # agent ids (Philox counter word 0) wrap inside the batch


def numpy_variant(entry, n, det, masked, A):
    """Whether the call runs one of the reference's NumPy variants (np.max of the row, IndexError when there is no
    candidate) or a list variant (steps over NaN, -1): the dispatcher of q_learning_optimal.py:644-726 for
    ``choose_actions``, the variant itself otherwise.  (A > 10 here: no list variant on action count.)"""
    if entry in ("choose_actions_iter", "single"):
        return False
    if entry == "choose_actions":
        return det or masked or n >= 100
    return True


@functools.lru_cache(maxsize=None)
def select_cases(A):
    """The cases of one width: every entry point twice (masked / unmasked where it takes both, both dtypes), the other
    axes rotated over the case index, plus one case whose agent ids wrap at 2^32."""
    w = WIDTHS.index(A)
    cases = []
    for e, entry in enumerate(ENTRIES):
        for v in (0, 1):
            j = 12 * w + 2 * e + v
            masked = {"choose_actions_vec": False, "choose_masked_actions_vec": True}.get(entry, v == 1)
            n = SINGLE_CALLS if entry == "single" else AGENTS[(3 * j + w) % len(AGENTS)]
            c = {"A": A, "id": j, "entry": entry, "det": (j + w) % 4 == 1, "eps": EPS[(j + w) % 3], "dt": DTYPES[(e + v + w) % 2],
                 "n": n, "step": STEP_COUNTERS[(w + e + 2 * v) % 3], "mask": MASK_KINDS[(w + e + v) % 4] if masked else None,
                 "nan_valid": None, "offset": 0, "seed": 7 + w}
            if (entry, v) in (("choose_masked_actions_vec", 0), ("choose_actions_iter", 1)):
                c["mask"] = "half+empty"  # every width meets an empty mask under a NumPy and under a list variant
            if not numpy_variant(entry, n, c["det"], masked, A):
                c["rows"], c["nan_valid"] = "all", True  # list variants step over NaN: every row kind, NaN column valid
            elif (entry, v) == ("choose_actions_vec_iter", 0):
                c["rows"], c["eps"] = "all", 0.0  # a NumPy variant meets the NaN rows greedily: IndexError
            elif masked:
                c["rows"], c["nan_valid"] = "nan_off", False  # ROW_ONE_NAN's NaN is masked out: no IndexError from it
            else:
                c["rows"] = "finite"
            cases.append(c)
    cases.append({"A": A, "id": 12 * w + 12, "entry": "choose_actions_vec_iter", "det": False, "eps": 0.3, "dt": DTYPES[w % 2],
                  "n": 9, "step": 2**32 - 1, "mask": "half", "nan_valid": False, "offset": OFFSET_NEAR_WRAP, "seed": 7 + w,
                  "rows": "nan_off"})
    return tuple(cases)


def select_inputs(c):
    """(table, states, masks or None) of a selection case."""
    pool = ROW_POOLS[c["rows"]]
    states = np.array([pool[(i + c["id"]) % len(pool)] for i in range(c["n"])], dtype=np.int32)
    masks = None if c["mask"] is None else build_masks(c["mask"], c["n"], c["A"], 100000 + c["id"], c["nan_valid"])
    return wide_table(c["A"], c["dt"]), states, masks


def agent_ids(c, n=None):
    n = c["n"] if n is None else n
    return ((c["offset"] + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def call_select(algo, c, states, masks, begin):
    """Run case `c` on `algo` (oracle, reference or product).  ``begin(step, n)`` prepares the draws of one call.
    Returns ("ok", int32 actions) or ("IndexError", None)."""
    kw = {"deterministic": c["det"]}
    try:
        if c["entry"] == "single":  # the single-agent forms, one call per state: agent 0 of consecutive steps
            out = []
            for i, s in enumerate(states):
                begin(c["step"] + i, 1)
                if masks is None:
                    out.append(algo.choose_action(int(s), c["eps"], **kw))
                else:
                    out.append(algo.choose_masked_action(int(s), masks[i], c["eps"], **kw))
            return "ok", np.array(out, dtype=np.int32)
        begin(c["step"], c["n"])
        if c["entry"] == "choose_actions_vec":
            out = algo.choose_actions_vec(states, c["eps"], **kw)
        elif c["entry"] == "choose_masked_actions_vec":
            out = algo.choose_masked_actions_vec(states, masks, c["eps"], **kw)
        else:
            out = getattr(algo, c["entry"])(states, c["eps"], action_masks=masks, **kw)
        return "ok", np.asarray(out, dtype=np.int32)
    except IndexError:
        return "IndexError", None


def shimmed(algo, c):
    """Plant the draw shim of case `c` into an oracle or reference object; returns its ``begin(step, n)``."""
    algo._rng = algo._np_rng = shim = InjectedDraws(c["seed"], agent_ids(c) if c["offset"] else None)
    return lambda step, n: shim.begin(step, n, c["eps"], deterministic=c["det"])


def _run_select_oracle(A, k):
    c = select_cases(A)[k]
    q, states, masks = select_inputs(c)
    algo = OracleQLearning(S_ROWS, A, 0.9, dtype=np.dtype(c["dt"]))
    algo.q_table = q
    return call_select(algo, c, states, masks, shimmed(algo, c))


run_select_oracle = functools.lru_cache(maxsize=None)(_run_select_oracle)


def select_analysis(c):
    """What the case's inputs imply, without the oracle's selection code: per agent whether it explores (the draw
    protocol), its greedy candidate set, and whether the call as a whole raises IndexError -- a NumPy variant in which
    some agent picks greedily on a row whose valid maximum is NaN, or explores with an empty mask."""
    q, states, masks = select_inputs(c)
    A, n = c["A"], c["n"]
    thr = 0 if c["det"] else epsilon_threshold(c["eps"])
    if c["entry"] == "single":
        x0 = np.array([policy_draws(c["seed"], agent_ids(c, 1), c["step"] + i)[0][0] for i in range(n)])
    else:
        x0 = policy_draws(c["seed"], agent_ids(c), c["step"])[0]
    explores = x0.astype(np.uint64) < np.uint64(thr) if thr < 2**32 else np.ones(n, dtype=bool)
    numpy_v = numpy_variant(c["entry"], n, c["det"], masks is not None, A)
    raises, candidates = False, []
    for i in range(n):
        valid = np.ones(A, dtype=bool) if masks is None else masks[i].astype(bool)
        vals = q[states[i]].astype(np.float64)
        if explores[i]:
            raises |= numpy_v and not valid.any()
            candidates.append(None)
            continue
        if not valid.any():  # NumPy variants: everything ties at -inf; list variants: -1
            candidates.append(np.arange(A) if numpy_v else np.zeros(0, dtype=np.int64))
            continue
        if np.isnan(vals[valid]).any() and numpy_v:
            raises = True
            candidates.append(np.zeros(0, dtype=np.int64))
            continue
        finite_or_inf = valid & ~np.isnan(vals)
        if not finite_or_inf.any():  # a list variant on a row without a usable column
            candidates.append(np.zeros(0, dtype=np.int64))
            continue
        m = vals[finite_or_inf].max()
        # np.where(mask, Q, -inf): when the valid maximum is -inf the masked-out columns tie with it
        tied = np.ones(A, dtype=bool) if (numpy_v and m == -np.inf) else finite_or_inf & (vals == m)
        candidates.append(np.flatnonzero(tied))
    return {"explores": explores, "candidates": candidates, "raises": bool(raises)}


# ------------------------------------------------------------------------------- unfused learning
LEARN_LR, LEARN_GAMMA = 0.1, 0.9
DEAD_ENDS = (ROW_NEG_INF, ROW_ONE_NAN, ROW_ALL_NAN, ROW_POS_INF)  # next rows of terminated transitions


def learn_batch_sizes(A):
    if A > 256:
        return (1, 65, 300)
    g = groups_per_block(A)  # the ordered path changes its sequential mode at more than 2 * ngrp involved transitions
    return (1, 2 * g - 1, 2 * g, 2 * g + 1, 300)


@functools.lru_cache(maxsize=None)
def learn_cases(A):
    """``learn`` and ``learn_vec``, masked and not, at every batch size; dtype and kind rotate.  Kinds: "plain";
    "nan_valid" -- live transitions onto ROW_ONE_NAN with its NaN column valid (the NaN must reach the target);
    "nan_off" -- the same with the column masked out (it must not); "last" -- next-masks with only column A - 1."""
    w = WIDTHS.index(A)
    cases = []
    for fn in ("learn", "learn_vec"):
        for masked in (False, True):
            kinds = ("plain", "nan_valid", "nan_off", "last") if masked else ("plain", "nan_valid")
            for i, n in enumerate(learn_batch_sizes(A)):
                j = len(cases)
                cases.append({"A": A, "id": 40 * w + j, "fn": fn, "masked": masked, "n": n, "dt": DTYPES[(i + w + masked) % 2],
                              "kind": kinds[(i + w + 3 * (fn == "learn_vec")) % len(kinds)]})
    return tuple(cases)


def learn_inputs(c):
    """q0 and the batch (s, a, r, s', terminated, next-masks) of a learn case.  Four written rows, all finite, of which
    the first is never a next row (a NaN written there stays where it is declared); six columns, so cells repeat."""
    A, n = c["A"], c["n"]
    rng = np.random.default_rng(50000 + c["id"])
    hot = [FINITE_ROWS[(c["id"] + i) % len(FINITE_ROWS)] for i in range(4)]
    cols = sorted({0, 63, 64, last_lane_start(A), A - 2, A - 1})
    s = rng.choice(hot, size=n).astype(np.int32)
    a = rng.choice(cols, size=n).astype(np.int32)
    r = (2.0 * rng.random(n) - 1.0 + 1e-3).astype(np.float32)  # rounded to float32 on the way in, as the engine does
    term = rng.random(n) < 0.2
    term[3::6] = True  # (never one of the transitions the NaN kinds pick below: those are multiples of 8)
    s2 = rng.choice(hot[1:], size=n).astype(np.int32)
    s2[term] = np.resize(DEAD_ENDS, int(term.sum()))  # the terminated ones go round the four dead ends
    if n == 1:
        term[0], s2[0] = False, hot[1]
    masks = None
    if c["masked"]:
        masks = build_masks("last" if c["kind"] == "last" else "half", n, A, 60000 + c["id"])
    if c["kind"] in ("nan_valid", "nan_off"):
        picked = np.arange(0, n, 8)  # every eighth transition goes live onto ROW_ONE_NAN
        s2[picked], term[picked] = ROW_ONE_NAN, False
        if c["kind"] == "nan_valid":
            s[picked] = hot[0]
            if masks is not None:
                masks[picked, nan_col(A)] = 1
        else:
            masks[:, nan_col(A)] = 0
            masks[:, A - 1] |= masks.sum(axis=1) == 0
    return wide_table(A, c["dt"]), (s, a, r, s2, term, masks)


def call_learn(algo, c, batch):
    s, a, r, s2, term, masks = batch
    with np.errstate(all="ignore"):
        getattr(algo, c["fn"])(s, a, r, s2, term, LEARN_LR, masks)


def _run_learn_oracle(A, k):
    c = learn_cases(A)[k]
    q0, batch = learn_inputs(c)
    algo = OracleQLearning(S_ROWS, A, LEARN_GAMMA, dtype=np.dtype(c["dt"]))
    algo.q_table = q0.copy()
    call_learn(algo, c, batch)
    return algo.q_table


run_learn_oracle = functools.lru_cache(maxsize=None)(_run_learn_oracle)


def declared_nan_cells(c):
    """bool[S_ROWS, A]: where the table must hold NaN after the case, from the inputs alone.  ``learn`` (sequential): a
    live transition whose next row has a NaN in a valid column; a terminated one never reads the row.  ``learn_vec``:
    that, and a terminated transition whose next row's valid maximum is infinite or NaN (``max * (1 - terminated)`` is
    inf * 0).  The next rows in question are never written and a cell that turned NaN is in a row nothing reads, so
    the initial table decides."""
    q0, (s, a, _r, s2, term, masks) = learn_inputs(c)
    out = np.isnan(q0)
    for i in range(c["n"]):
        vals = q0[s2[i]].astype(np.float64)
        vals = vals if masks is None else vals[masks[i].astype(bool)]
        m = np.nan if np.isnan(vals).any() else vals.max()
        if c["fn"] == "learn":
            bad = (not term[i]) and np.isnan(m)
        else:
            bad = np.isnan(m) or (term[i] and np.isinf(m))
        if bad:
            out[s[i], a[i]] = True
    return out


# ------------------------------------------------------------------------------- closed loop
# name -> (spec, chunks, dtype, learn mode, NaN cells of the start table).  Hash specs are helpers.make_oracle_env's;
# ("table", N, S, A, seed) is table_mdp_model.random_mdp(S, A, 2, seed, masked=True) behind the table-driven environment.
# N and S per width: some step has more than 2 * ngrp + 1 agents on rows that another agent writes in that step.
ROLLOUTS = {
    "a65_n150": (("hash", 150, 30, 65, False), [12], "f4", "iter", 0),
    "a65_masked_n600_vec": (("hash", 600, 100, 65, True), [8], "f8", "vec", 0),
    "a100_masked_n150": (("hash", 150, 40, 100, True), [12], "f4", "iter", 0),
    "a100_n600_vec": (("hash", 600, 60, 100, False), [8], "f4", "vec", 0),
    "a100_n2100_f8": (("hash", 2100, 500, 100, False), [6], "f8", "iter", 0),
    "a129_n40_f8": (("hash", 40, 30, 129, False), [20], "f8", "iter", 0),
    "a129_masked_n600_vec": (("hash", 600, 200, 129, True), [8], "f4", "vec", 0),
    "a255_masked_n600": (("hash", 600, 120, 255, True), [8], "f4", "iter", 0),
    "a255_n150_f8_vec": (("hash", 150, 30, 255, False), [12], "f8", "vec", 0),
    "a256_n2100": (("hash", 2100, 500, 256, False), [6], "f4", "iter", 0),
    "a256_masked_n40_f8": (("hash", 40, 30, 256, True), [20], "f8", "iter", 0),
    "a256_n150_f8": (("hash", 150, 50, 256, False), [12], "f8", "iter", 0),  # 2 KB rows: the LDS row cache overflows early
    "table_a72_n150": (("table", 150, 60, 72, 11), [12], "f4", "iter", 0),
    "table_a130_n600_f8": (("table", 600, 100, 130, 12), [8], "f8", "vec", 0),
    "nan_a100_n60_list": (("hash", 60, 40, 100, False), [4, 4, 4], "f4", "iter", 60),  # < 100 agents: steps over NaN
    "nan_a100_n150_numpy": (("hash", 150, 300, 100, False), [4, 4, 4, 4], "f4", "iter", 1),  # IndexError, same call
}


def spec_shape(spec):
    return spec[2], spec[3]


@functools.lru_cache(maxsize=None)
def table_mdp(S, A, seed):
    from dist_classicrl_amd.environments.device_envs import encode_table_mdp  # (host code: no device is touched)
    from table_mdp_model import random_mdp

    arrays, isd, masks = random_mdp(S, A, 2, seed=seed, masked=True)
    return encode_table_mdp(*arrays, isd, masks)


def oracle_env(spec):
    if spec[0] == "table":
        from table_mdp_model import TableMDPVecEnv

        return TableMDPVecEnv(spec[1], table_mdp(*spec[2:]), seed=1)
    return make_oracle_env(spec)


def rollout_q0(name):
    spec, _chunks, dt, _mode, nan_cells = ROLLOUTS[name]
    return rollout_table(*spec_shape(spec), dt, nan_cells)


@functools.lru_cache(maxsize=None)
def run_rollout_oracle(name):
    """``helpers.run_oracle_chunks`` on the case: one dict per chunk (or {"raised": True})."""
    spec, chunks, dt, mode, _ = ROLLOUTS[name]
    return run_oracle_chunks(spec, chunks, dt, "const", mode, q0=rollout_q0(name), env=oracle_env(spec))


def rollout_facts(name):
    """What the oracle's run of the case shows: the share of actions >= 64, whether column 64 was picked, the episodes
    that ended, and the largest number of agents that in one step stood on, or moved to, a row that ANOTHER agent wrote in
    that step (the transitions the ordered path has to order)."""
    spec = ROLLOUTS[name][0]
    ok = [w for w in run_rollout_oracle(name) if not w["raised"]]
    assert ok, "the first call already raises: nothing to look at"
    actions = ok[-1]["actions"]
    env = oracle_env(spec)
    states, _ = env.reset()
    most = 0
    for acts in actions:
        s = np.array(states["observation"] if isinstance(states, dict) else states)
        states, _r, term, _t, _i = env.step(acts)
        s2 = np.array(states["observation"] if isinstance(states, dict) else states)
        writers = np.bincount(s, minlength=env.state_size)
        involved = (writers[s] >= 2) | (~term & (s2 != s) & (writers[s2] >= 1))
        most = max(most, int(involved.sum()))
    return {"share_ge64": float((actions >= 64).mean()), "col64": bool((actions == 64).any()),
            "episodes": len(ok[-1]["history"]), "most_involved": most}


# ------------------------------------------------------------------------------- the golden anchor
def shim_cannot_observe(c):
    """A deterministic list-variant call with an agent that has no candidate: the unmodified reference returns -1 without
    drawing, which the draw shim cannot see (InjectedDraws.skip_choice) -- such a case has no golden record."""
    if numpy_variant(c["entry"], c["n"], c["det"], c["mask"] is not None, c["A"]) or not c["det"]:
        return False
    return any(cand is not None and len(cand) == 0 for cand in select_analysis(c)["candidates"])


def changed_cells(q, q0):
    """Flat indices of the cells of `q` that differ from `q0` (a NaN that stayed a NaN has not changed)."""
    same = (q == q0) | (np.isnan(q) & np.isnan(q0))
    return np.flatnonzero(~same.ravel())
