"""GPU: the main engine on the largest tables ``qe_create`` accepts -- just under 2^32 cells.

Every other test of the main engine stays below 2^28.3 cells; here each training path, the delta log, the apply entry
points, the row / cell I/O and the replay ring meet byte offsets beyond 2^31 and 2^32 (2^35 with float64), cell indices
with bit 31 set (the ``uint32 cell`` of a delta record, the top bit of the radix-sort key) and the last row of a maximal
table.  Everything is compared bit for bit with the C oracle -- no tolerance.

Engines (``engines`` fixture: one per dtype and width, ONE alive at a time, in the order the tests of this file use them;
touched rows are zeroed again after every case, nothing is reallocated within a group):

    =======  =====  ==========  =======  ==========================================================  ================
    key      dtype  S           A / ld   cases                                                       device memory
    =======  =====  ==========  =======  ==========================================================  ================
    f32x64   f32    2^26 - 1    64 / 64  generic persistent build (96 agents, replay ring attached;  16 GiB table
                                         128 masked agents), row / cell I/O                          + 1 GiB stamps
    f32x16   f32    2^28 - 1    16 / 16  the 128-agent LEAN builds: full build (ordered-path         16 GiB + 4 GiB
                                         options 1 and 2) and sparse build (option 3)
    f32x16d  f32    2^25 - 1    16 / 16  the dataflow build at ITS upper edge (row ids of 25 bits)   2 GiB + 0.5 GiB
    f32x256  f32    2^24 - 1    256/256  step-wise, turnstile learn / learn_vec, wide bitmap and     16 GiB + 0.25 GiB
                                         listed walks, delta log, apply entry points                 + 2 GiB turnstile
                                                                                                     records + 0.13 GiB
                                                                                                     token array
    f32x250  f32    17 043 521  250/252  padded rows (k_pad_fill), row stride no power of two: a     16 GiB + 0.25 GiB
                                         row straddles cell 2^31; step-wise, row / cell I/O
    f64x64   f64    2^26 - 1    64 / 64  generic persistent build, row / cell I/O: byte offsets to   32 GiB + 1 GiB
                                         2^35
    =======  =====  ==========  =======  ==========================================================  ================

Peak: 33 GiB of device memory.  What the shapes cannot reach: LEAN builds exist for 8 and 16 actions only, so at 64
actions every persistent rollout runs the generic build whatever QE_OPT_LANE_ORDERED_PATH says -- the three options are
exercised at 16 actions; and the dataflow kernel takes tables below 2^25 rows (option 1 runs the full build above), i.e.
at most 2^29 cells = 2^31 bytes: it cannot cross any of the boundaries and is run at its own largest table instead.

The oracle side never holds a table: ``helpers.run_sparse_hash_oracle`` runs the C oracle on a lazily zero mapping and
seeds exactly the rows the run touches with ``helpers.edge_q0`` (nonzero, row-specific) -- the same rows are written into
the engine with ``qe_table_cells`` op 1, so the runs agree iff the engine reads the rows the oracle reads (a read through
a wrapped address returns another row's zeros or another row's values).  Host resident size grows by 94 MB in the
largest case (4096 agents, 85 000 rows of 1 KiB: one 4 KiB page each; 2 MB at 96 agents) against a 16 GiB table;
``_case`` prints the figure and asserts less than 1/16 of the table for every case.

Agents are placed (``qe_env_restore`` through the state dict) on the last row, on row 0 and on the rows on either side of
cell 2^31, byte 2^31 and byte 2^32; two agents share the last row and the row above cell 2^31, so the hand-over logic of
every ordered path runs at a high address.  Each case asserts, on the oracle's own records, that cells >= 2^31, byte
offsets >= 2^32 and the last row were updated.

Shown able to fail (by reasoning; nothing broken was run on a GPU): with ``(uint32_t)`` on the byte offset ``row * ld *
sizeof(T)`` of a row load, every agent standing on a row beyond byte 2^32 reads another row (zeros or a foreign seeded
row instead of its own ``edge_q0`` values): its greedy action, and with it ``trace_actions``, the successor and the
updated cell differ in the first step -- every rollout case fails at the actions, the float64 case already from byte
2^32 = cell 2^29.  With ``(uint32_t)`` (or ``int32``) on ``row * ld`` nothing changes below 2^32 cells except signed
forms from cell 2^31: the agents placed above cell 2^31 then address memory before the table, caught the same way.  With
bit 31 dropped from the sort key of ``qe_delta_sort.h`` the records of a pair of cells that differ only in bit 31 are
merged into one run: ``test_apply_entry_points_over_the_whole_cell_range`` fails on both cells.  A row-I/O offset
narrowed to 32 bits writes the block at byte 2^32 over the start of the table:
``test_row_and_cell_io_*`` read the block back through ``qe_table_cells`` and find row 0 changed.

Wall time on one MI355X: about 8 s for the 24 cases of this module, the six engine allocations included; the slowest
cases take 1.7 s (the first on the 256-wide engine: table, turnstile records), 1.4 s (float64, 32 GiB) and 1.1 s (4096
agents: the oracle side) -- none is marked ``slow``.
"""

import ctypes as C

import numpy as np
import pytest

from helpers import edge_q0, resident_bytes, run_sparse_hash_oracle
from test_gpu_delta_apply import _DevBuf, _expected
from test_gpu_delta_log import _Log, _check_records

pytestmark = pytest.mark.gpu

SHAPES = {  # key -> (dtype, S, A)
    "f32x64": (np.float32, (1 << 26) - 1, 64),
    "f32x16": (np.float32, (1 << 28) - 1, 16),
    "f32x16d": (np.float32, (1 << 25) - 1, 16),
    "f32x256": (np.float32, (1 << 24) - 1, 256),
    "f32x250": (np.float32, 17_043_521, 250),  # ld = 252: 17 043 521 * 252 = 2^32 - 4
    "f64x64": (np.float64, (1 << 26) - 1, 64),
}


def _product():
    from dist_classicrl_amd import _lib, environments, schedules
    from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase
    from dist_classicrl_amd.algorithms.runtime.gpu_rollout_runtime import GpuRolloutQLearning

    return _lib, OptimalQLearningBase, GpuRolloutQLearning, environments, schedules


class _Engine:
    def __init__(self, key):
        self._lib, Algo = _product()[:2]
        self.lib = self._lib.load()
        self.key = key
        self.dt, self.S, self.A = SHAPES[key]
        self.dt = np.dtype(self.dt)
        self.algo = Algo(self.S, self.A, 0.99, seed=0, dtype=self.dt)
        self.h = self.algo.handle
        self.ld = int(self.lib.qe_table_row_stride(self.h))
        if key != "f32x16d":
            assert self.S * self.ld < 1 << 32 <= (self.S + 1) * self.ld, "not the largest table of this width"
        self.hip = C.CDLL("libamdhip64.so")

    # ---- cells by (row, column): qe_table_cells ops 0 / 1 / 2
    def cells(self, rows, cols, values, op):
        rows, cols = self._lib.as_i32(rows).ravel(), self._lib.as_i32(cols).ravel()
        vals = (np.empty(rows.size, dtype=np.float64) if op == 0
                else np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float64).ravel(), rows.shape)))
        self._lib.check(self.lib.qe_table_cells(self.h, self._lib.ptr(rows, C.c_int32), self._lib.ptr(cols, C.c_int32),
                                                rows.size, self._lib.ptr(vals, C.c_double), op))
        return vals.astype(self.dt)  # (exact: the values came out of / go into a table of this dtype)

    def write_rows(self, rows, values):
        rows = np.asarray(rows, dtype=np.int64)
        if rows.size:
            self.cells(np.repeat(rows, self.A), np.tile(np.arange(self.A), rows.size), values, 1)

    def read_rows(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        return self.cells(np.repeat(rows, self.A), np.tile(np.arange(self.A), rows.size), None, 0).reshape(rows.size, self.A)

    def padding_of(self, row):
        """The padding columns of `row`, straight from device memory (no entry point addresses them)."""
        out = np.empty(self.ld - self.A, dtype=self.dt)
        src = C.c_void_p(self.lib.qe_table_dev(self.h) + (row * self.ld + self.A) * self.dt.itemsize)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), src, C.c_size_t(out.nbytes), 2) == 0  # D2H
        return out

    def defaults(self):
        o = self._lib
        for opt, value in ((o.OPT_ROLLOUT_PATH, o.PATH_AUTO), (o.OPT_LANE_ORDERED_PATH, 0), (o.OPT_TOKEN_ROUNDS, 0),
                           (o.OPT_LISTED_MIN_AGENTS, 16384), (o.OPT_TURN_FORWARD, 1)):
            self.algo.set_engine_option(opt, value)

    def boundaries(self):
        """cell indices of: cell 2^31, byte 2^31, byte 2^32."""
        return [1 << 31, (1 << 31) // self.dt.itemsize, (1 << 32) // self.dt.itemsize]

    def edge_rows(self):
        """[last row, row 0] + for each boundary inside the table the rows on either side of it (the row holding the
        last cell below it and the next one; a row that straddles it counts as the lower one and is followed by the
        first row wholly above)."""
        rows = [self.S - 1, 0]
        for c in self.boundaries():
            lo = (c - 1) // self.ld
            if lo + 1 < self.S:
                rows += [lo, lo + 1]
        return rows


class _Engines:
    """One engine alive at a time (33 GiB at the most instead of the 106 GiB of all six)."""

    def __init__(self):
        self.current = None

    def get(self, key):
        if self.current is None or self.current.key != key:
            self.close()
            self.current = _Engine(key)
        self.current.defaults()
        return self.current

    def close(self):
        if self.current is not None:
            self.current.algo.__del__()
            self.current = None


@pytest.fixture(scope="module")
def engines():
    pool = _Engines()
    yield pool
    pool.close()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


def _placement(eng, pairs=True):
    """Start rows of the first agents: the edge rows; the last row and the first row above cell 2^31 twice."""
    rows = eng.edge_rows()
    above = [r for r in rows if r * eng.ld >= 1 << 31]
    return ([eng.S - 1] if pairs else []) + rows + (above[:1] if pairs and above else [])


def _case(eng, n, mode, steps, check_variant, *, path="auto", options=(), masked=False, trace=True, log=False, ring=False):
    """One closed-loop case on `eng`: `steps` = the two run_steps calls."""
    _lib, _, Runtime, envs, sch = _product()
    lib, S, A, ld, dt = eng.lib, eng.S, eng.A, eng.ld, eng.dt
    total = sum(steps)
    placed = _placement(eng)
    rss0 = resident_bytes()
    want = run_sparse_hash_oracle(n, S, A, total, dt, mode, np.full(total, 0.1), np.full(total, 0.1), masked=masked,
                                  placed=placed)
    grown = resident_bytes() - rss0
    print(f"{eng.key} n={n} {mode}: {want['rows'].size} rows seeded, host resident size +{grown / 1e6:.0f} MB")
    assert grown < S * A * dt.itemsize // 16, "the oracle side materialised a sizeable part of the table"
    # conditions on the inputs, from the oracle's own records
    cells = want["cells"].astype(np.int64)
    cells = cells // A * ld + cells % A
    assert (cells >= 1 << 31).any() or eng.key == "f32x16d", "no updated cell with bit 31 set"
    assert (cells * dt.itemsize >= 1 << 32).any() or eng.key == "f32x16d", "no update beyond byte offset 2^32"
    assert (cells // ld == S - 1).any(), "no update in the last row"
    rows = want["rows"]
    algo = eng.algo
    algo.set_rollout_path(path)
    for opt, value in options:
        algo.set_engine_option(getattr(_lib, opt), value)
    algo.step_counter = 0
    dlog = rb = None
    try:
        eng.write_rows(rows, edge_q0(rows, A, dt))
        if log:
            dlog = _Log(total * n, 2 * n + 64)
            _lib.check(lib.qe_delta_log_attach(eng.h, dlog.ptr, total * n))
        if ring:
            from dist_classicrl_amd.algorithms.buffers import ExperienceReplay

            rb = ExperienceReplay(total * n, 1)
            rb.attach(algo)
        rt = Runtime(algo, sch.ConstantSchedule(0.1), sch.ConstantSchedule(0.1), learn_mode=mode)
        rt.trace_actions = True if trace else None
        env = envs.HashTabularEnv(n, S, A, seed=1, masked=masked)
        env.bind(algo)
        env.reset_device()
        first = env.state_dict()
        obs = np.array(first["states"]["observation"] if masked else first["states"])
        assert np.array_equal(obs, want["reset_obs"])  # the reset itself: start states up to row S - 1
        obs[:len(placed)] = placed
        sd = {"states": {"observation": obs} if masked else obs, "infos": first["infos"],
              "rewards": np.array(first["rewards"]), "aux": np.array(first["aux"])}
        history, actions = [], []
        for k in steps:
            try:
                _avg, h, env, sd = rt.run_steps(k, env, sd)
            except ZeroDivisionError:  # no episode ended in this call (reference quirk); the state moved on all the same
                h, sd = [], env.state_dict()
            history += h
            if trace:
                actions.append(rt.last_trace)
            assert rt.last_stats["kernel_variants"], "no launch was recorded"
            for v in rt.last_stats["kernel_variants"]:
                check_variant(_lib.decode_variant(v))
        _lib.check(lib.qe_synchronize(eng.h))
        if trace:
            assert np.array_equal(np.concatenate(actions), want["actions"])
        final = sd["states"]["observation"] if masked else sd["states"]
        assert np.array_equal(final, want["final_obs"])
        assert np.array_equal(sd["rewards"], want["agent_rewards"])
        assert np.array_equal(np.array(history, dtype=np.float32), want["history"])
        # every row the run touched (and every seeded one), bit for bit
        assert np.array_equal(_bits(eng.read_rows(rows)), _bits(want["q_rows"]))
        # the untouched neighbours of the edge rows
        near = np.array(sorted({r + d for r in eng.edge_rows() for d in (-1, 1) if 0 <= r + d < S} - set(rows.tolist())))
        assert near.size and not eng.read_rows(near).any()
        if ld > A:  # padding columns of the last row and of a middle row (the one at cell 2^31)
            for r in (S - 1, (1 << 31) // ld):
                assert np.isneginf(eng.padding_of(r)).all(), r
        if log:
            assert lib.qe_delta_log_count(eng.h) == total * n
            words = dlog.read()
            _check_records(words, n, total, ld, A, want)
            assert (words[:total * n, 0] >= 1 << 31).any()
        if ring:  # (s, s') of every transition in (step, agent) order: the high row ids unchanged
            assert len(rb) == total * n
            assert np.array_equal(rb.state_buffer, want["cells"].astype(np.int64) // A)
            assert np.array_equal(rb.next_state_buffer, want["next_obs"])
            assert rb.state_buffer.max() == S - 1
    finally:
        if rb is not None:
            rb.detach(algo)
        if dlog is not None:
            _lib.check(lib.qe_delta_log_attach(eng.h, None, 0))
            dlog.free()
        eng.write_rows(rows, 0.0)
        eng.defaults()


def _path_is(path, **bits):
    def check(d):
        assert d["path"] == path, d
        for name, value in bits.items():
            assert d[name] == value, (name, d)
    return check


# ---------------------------------------------------------------------------------------------- persistent builds
def test_generic_persistent_build_with_the_replay_ring(engines):
    """96 agents, 64 actions: k_rollout_lane's generic build (a partly filled second wavefront); the attached replay
    ring takes int32 rows into int64 slots."""
    _case(engines.get("f32x64"), 96, "iter", (13, 15), _path_is("persistent", lean=0, cap512=True, nv=16, masked=False),
          ring=True)


@pytest.mark.parametrize("mode", ["iter", "vec"])
def test_masked_persistent_build(engines, mode):
    """128 masked agents (the masked case): mask words are hashed from (row * words + k) in 32 bits."""
    _case(engines.get("f32x64"), 128, mode, (13, 15), _path_is("persistent", lean=0, cap512=True, nv=16, masked=True),
          masked=True)


def test_row_and_cell_io_f32x64(engines):
    _row_and_cell_io(engines.get("f32x64"))


@pytest.mark.parametrize("option", [1, 2, 3])
def test_lean_builds_of_128_agents(engines, option):
    """Plain training rollouts (no trace: that is what selects a LEAN build) of 128 agents at 16 actions and 2^28 - 1
    rows.  QE_OPT_LANE_ORDERED_PATH 2: the full build; 3: the sparse build; 1 asks for the dataflow kernel, which takes
    tables below 2^25 rows -- lane_build hands such a table to the full build."""
    sparse = option == 3
    _case(engines.get("f32x16"), 128, "iter", (13, 15),
          _path_is("persistent", lean=1, help=True, full=True, dataflow=False, light=sparse, cap512=False, nv=4),
          options=(("OPT_LANE_ORDERED_PATH", option),), trace=False)


def test_dataflow_build_at_its_largest_table(engines):
    """k_rollout_df packs {row, owner} into 32 bits: 2^25 - 1 rows is its largest table (2 GiB: no boundary to cross);
    agents on the last row carry the largest row id it can meet."""
    _case(engines.get("f32x16d"), 128, "iter", (13, 15),
          _path_is("persistent", lean=1, help=True, full=True, dataflow=True, cap512=False, nv=4),
          options=(("OPT_LANE_ORDERED_PATH", 1),), trace=False)


# ---------------------------------------------------------------------------------------------- 256 actions
@pytest.mark.parametrize("mode", ["iter", "vec"])
def test_step_wise_path_with_the_log(engines, mode):
    _case(engines.get("f32x256"), 200, mode, (10, 12), _path_is("stepwise"), path="stepwise", log=True)


@pytest.mark.parametrize("forward", [1, 0])
def test_turnstile_learn_with_the_log(engines, forward):
    """600 agents: 2 * S records of 64 B (2 GiB), record index 2 * row + parity."""
    _case(engines.get("f32x256"), 600, "iter", (10, 12), _path_is("turnstile"), options=(("OPT_TURN_FORWARD", forward),),
          log=True)


def test_turnstile_learn_vec_with_the_log(engines):
    _case(engines.get("f32x256"), 600, "vec", (10, 12), _path_is("turnstile"), log=True)


@pytest.mark.parametrize("mode", ["iter", "vec"])
def test_wide_path_bitmap_walk(engines, mode):
    _case(engines.get("f32x256"), 2100, mode, (9, 11), _path_is("wide"), path="wide")


@pytest.mark.parametrize("mode", ["iter", "vec"])
def test_wide_path_listed_walk(engines, mode):
    _case(engines.get("f32x256"), 4096, mode, (9, 11), _path_is("wide"), path="wide",
          options=(("OPT_LISTED_MIN_AGENTS", 1), ("OPT_TOKEN_ROUNDS", 7)))


def _apply_records(eng, rng, world, count):
    """(world, count) records over the whole cell range: cell 0, the last cell, pairs that differ only in bit 31, a few
    cells repeated many times, the rest uniform."""
    S, A, ld = eng.S, eng.A, eng.ld
    cell = (rng.integers(0, S, size=(world, count)) * ld + rng.integers(0, A, size=(world, count))).astype(np.uint32)
    low = rng.integers(0, (1 << 31) // ld, size=4000) * ld + rng.integers(0, A, size=4000)
    high = low + (1 << 31)  # the same cell with bit 31 set: kept where that is a cell of the table, not padding
    low = low[(high < S * ld) & (high % ld < A)][:8]
    assert low.size == 8
    special = np.concatenate([[0, S * ld - 1 - (ld - A)], low, low + (1 << 31)]).astype(np.uint32)
    hot = special[[0, 1, 2, 10]]  # cell 0, the last cell and one pair
    for r in range(world):
        at = rng.permutation(count)
        cell[r, at[:special.size]] = special
        cell[r, at[special.size:special.size + count // 3]] = hot[rng.integers(0, 4, size=count // 3)]
    delta = (rng.standard_normal((world, count)) * 0.1).astype(np.float32)
    rec = np.empty((world, count, 2), dtype=np.uint32)
    rec[..., 0], rec[..., 1] = cell, delta.view(np.uint32)
    return rec


@pytest.mark.parametrize("key", ["f32x256", "f32x250"])
def test_apply_entry_points_over_the_whole_cell_range(engines, key):
    """qe_delta_apply_gathered_dev (the engine's radix sort over all 32 key bits) and qe_delta_apply_sorted_dev on
    remote records, against the sparse CPU simulation of test_gpu_delta_apply.py (stable sort by cell, float32 adds in
    that order); a record at cell = S * ld is skipped and reported."""
    eng = engines.get(key)
    _lib, lib, ld = eng._lib, eng.lib, eng.ld
    world, count, rank = 3, 6000, 1
    rng = np.random.default_rng(32)
    rec = _apply_records(eng, rng, world, count)
    bad_at = 4321
    valid = rec.copy()
    rec[0, bad_at, 0] = np.uint32(eng.S * ld)
    valid[0, bad_at] = (0, np.float32(-0.0).view(np.uint32))  # x + -0.0 == x bit for bit: the record adds nothing
    start = lambda cells: edge_q0(cells // ld, ld, np.float32)[np.arange(cells.size), cells % ld]  # noqa: E731
    uniq, acc, _ = _expected(start, valid, count, rank)
    assert (uniq >= 1 << 31).any() and uniq[0] == 0 and uniq[-1] == eng.S * ld - 1 - (ld - eng.A)
    assert np.isin(uniq[uniq < 1 << 31] | np.uint32(1 << 31), uniq).sum() >= 8
    others = np.concatenate([rec[r] for r in range(world) if r != rank])
    sorted_others = np.ascontiguousarray(others[np.argsort(others[:, 0], kind="stable")])
    rows, cols = (uniq // ld).astype(np.int64), (uniq % ld).astype(np.int64)
    try:
        for entry in ("gathered", "sorted"):
            eng.cells(rows, cols, start(uniq), 1)
            buf = _DevBuf(rec if entry == "gathered" else sorted_others)
            if entry == "gathered":
                _lib.check(lib.qe_delta_apply_gathered_dev(eng.h, buf.ptr, count, count, world, rank))
            else:
                _lib.check(lib.qe_delta_apply_sorted_dev(eng.h, buf.ptr, sorted_others.shape[0]))
            assert lib.qe_synchronize(eng.h) == _lib.ERR_INDEX
            assert b"1 delta records" in lib.qe_last_error()
            _lib.check(lib.qe_synchronize(eng.h))  # reported once
            buf.free()
            assert np.array_equal(_bits(eng.cells(rows, cols, None, 0)), _bits(acc)), entry
    finally:
        eng.cells(rows, cols, 0.0, 1)


# ---------------------------------------------------------------------------------------------- padded rows
@pytest.mark.parametrize("mode", ["iter", "vec"])
def test_step_wise_path_on_padded_rows(engines, mode):
    """250 actions in rows of 252: k_pad_fill ran over 34 M padding cells up to the table's last one, cell = row * 252
    + a, and row 8 521 760 straddles cell 2^31."""
    _case(engines.get("f32x250"), 200, mode, (10, 12), _path_is("stepwise"), path="stepwise", log=True)


def test_row_and_cell_io_f32x250(engines):
    _row_and_cell_io(engines.get("f32x250"))


# ---------------------------------------------------------------------------------------------- float64
def test_float64_generic_persistent_build(engines):
    """The 32 GiB table: byte offsets up to 2^35."""
    _case(engines.get("f64x64"), 96, "iter", (13, 15), _path_is("persistent", lean=0, cap512=True, masked=False))


def test_row_and_cell_io_f64x64(engines):
    _row_and_cell_io(engines.get("f64x64"))


# ---------------------------------------------------------------------------------------------- table I/O
def _row_and_cell_io(eng):
    """qe_table_upload_rows / qe_table_download_rows on blocks of six rows that straddle byte offsets 2^31 and 2^32 (and
    cell 2^31) and on the block that ends with the last row; the same cells through qe_table_cells ops 0, 1 and 2 --
    two addressing paths that must agree -- and the rows around every block (and row 0) untouched."""
    _lib, lib, S, A, dt = eng._lib, eng.lib, eng.S, eng.A, eng.dt
    firsts = sorted({(c - 1) // eng.ld - 2 for c in eng.boundaries() if (c - 1) // eng.ld + 4 <= S} | {S - 6})
    assert len(firsts) >= 3
    try:
        for first in firsts:
            block = edge_q0(np.arange(first, first + 6), A, dt)
            _lib.check(lib.qe_table_upload_rows(eng.h, block.ctypes.data, first, 6))
            back = np.empty_like(block)
            _lib.check(lib.qe_table_download_rows(eng.h, back.ctypes.data, first, 6))
            assert np.array_equal(_bits(back), _bits(block)), first
            assert np.array_equal(_bits(eng.read_rows(np.arange(first, first + 6))), _bits(block)), first
            around = [r for r in (0, first - 1, first + 6) if 0 <= r < S and not first <= r < first + 6]
            assert not eng.read_rows(around).any(), first
            # ops 1 and 2 on one column of the block, read back row-wise
            rows6 = np.arange(first, first + 6)
            eng.cells(rows6, np.full(6, A - 1), np.arange(1.0, 7.0), 1)
            eng.cells(rows6, np.full(6, A - 1), np.full(6, 0.5), 2)
            eng.cells(rows6[:1], [A - 1], [0.25], 2)
            block[:, A - 1] = np.arange(1.5, 7.5)
            block[0, A - 1] += 0.25
            _lib.check(lib.qe_table_download_rows(eng.h, back.ctypes.data, first, 6))
            assert np.array_equal(_bits(back), _bits(block)), first
            if eng.ld > A:
                assert np.isneginf(eng.padding_of(first + 5)).all()
    finally:
        zeros = np.zeros((6, A), dtype=dt)
        for first in firsts:
            _lib.check(lib.qe_table_upload_rows(eng.h, zeros.ctypes.data, first, 6))
    with pytest.raises(ValueError):
        _lib.check(lib.qe_table_download_rows(eng.h, zeros.ctypes.data, S - 5, 6))  # one row past the end
