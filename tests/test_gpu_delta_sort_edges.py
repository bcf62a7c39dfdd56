"""GPU: the deterministic apply step of the replica exchange at its structural edges.

``qe_delta_apply_gathered_dev`` (the radix sort of ``csrc/qe_delta_sort.h`` + the run walk ``k_delta_apply_sorted``) on
inputs that the uniform cells of test_gpu_delta_apply.py never produce, every table compared BIT FOR BIT with the NumPy
model of delta_sort_model.py (no tolerance anywhere in this module: ``uint32`` views, NaN-ness where the model is NaN,
every untouched cell equal to its initial value):

a. passes in which one digit holds every record (the ordered copy over three tiles and two records, in pass 0 through
   ``dsort_src`` as the first, a middle and the last rank, and the flag reset before a mixed pass);
b. 64-record batches of pass 0 with 64 equal digits, 64 distinct ones, two alternating, digits 0 and 255 only (the
   ragged batch holding live records of digit 0), and 63 equal digits with the last lane different;
c. sizes around a batch, a block, a tile and the scan's chunk of 256 tiles; seven ranks with one record each; nothing;
d. many calls on one engine: large then small, no synchronisation in between, bad records reported once and summed;
e. the run walk: bad records first and last, 300 of them inside one cell's run, all bad, a run of 5000 records;
f. infinite, NaN, signed-zero, FLT_MAX and subnormal increments and cells;
g. the atomic entry points on increments whose sums are exact in any order.

Cases marked "also sorted" send the model's sorted records through ``qe_delta_apply_sorted_dev`` on a second engine.
Two float32 engines with ld == A == 16: 4097 rows (65 552 cells, three passes) and 2^20 + 1 rows (2^24 + 16 cells, four
passes, 64 MB).  tests/test_delta_sort_cases.py asserts in full, without a device, that the inputs are what they claim;
here those conditions are repeated as one-line guards.

Subnormals: the expectation is NumPy's float32 arithmetic with gradual underflow (``test_special_values[subnormal]``);
on an MI355X the run walk meets it bit for bit -- nothing is flushed to zero.
"""
import numpy as np
import pytest

import delta_sort_model as m
from test_gpu_delta_apply import _DevBuf

pytestmark = pytest.mark.gpu

U32 = np.uint32


def _binding():
    from dist_classicrl_amd import _lib

    return _lib, _lib.load()


class _Engine:
    def __init__(self, S):
        from dist_classicrl_amd.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase

        self._lib, self.lib = _binding()
        self.algo = OptimalQLearningBase(S, m.A, 0.99, seed=0)
        self.h, self.cells = self.algo.handle, S * m.A
        assert int(self.lib.qe_table_row_stride(self.h)) == m.A  # ld == A: cell = row * 16 + column, no padding

    def upload(self, q_flat):
        q_flat = np.ascontiguousarray(q_flat, dtype=np.float32)
        assert q_flat.size == self.cells
        self._lib.check(self.lib.qe_table_upload(self.h, q_flat.ctypes.data, self._lib.QE_F32))

    def download(self):
        host = np.empty(self.cells, dtype=np.float32)
        self._lib.check(self.lib.qe_table_download(self.h, host.ctypes.data, self._lib.QE_F32))
        return host

    def gathered(self, case):
        """Queue one gathered apply; the returned device buffer must outlive the next synchronisation."""
        buf = _DevBuf(case.rec)
        self._lib.check(self.lib.qe_delta_apply_gathered_dev(self.h, buf.ptr, case.capacity, case.count, case.world,
                                                             case.rank))
        return buf

    def expect_report(self, bad):
        """Synchronise: `bad` skipped records are reported as QE_ERR_INDEX with their number -- once."""
        rc = self.lib.qe_synchronize(self.h)
        if bad:
            assert rc == self._lib.ERR_INDEX, rc
            assert b"%d delta records" % bad in self.lib.qe_last_error(), self.lib.qe_last_error()
            rc = self.lib.qe_synchronize(self.h)
        self._lib.check(rc)

    def close(self):
        self.algo.__del__()


@pytest.fixture(scope="module")
def small():
    eng = _Engine(m.SMALL_S)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def small2():
    eng = _Engine(m.SMALL_S)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def large():
    eng = _Engine(m.LARGE_S)
    eng.q0 = m.initial(m.LARGE_CELLS, seed=10)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def q_small():
    q0 = m.initial(m.SMALL_CELLS, seed=11)
    q0.setflags(write=False)
    return q0


def _same(got, want, q0, records, what=""):
    """got == want bit for bit (NaN-ness where the model is NaN); cells no valid record names still hold q0."""
    nan = np.isnan(want)
    off = np.flatnonzero((np.isnan(got) != nan) | (~nan & (got.view(U32) != want.view(U32))))
    assert off.size == 0, (f"{what}: {off.size} cells differ, first {off[:5].tolist()}: got {got[off[:5]].tolist()}, "
                           f"model {want[off[:5]].tolist()}")
    untouched = np.ones(got.size, dtype=bool)
    untouched[records[records[:, 0] < got.size, 0]] = False
    assert np.array_equal(got.view(U32)[untouched], q0.view(U32)[untouched]), f"{what}: an untouched cell changed"


def _run(eng, case, q0, sorted_on=None):
    """One gathered apply of `case` to a table holding `q0` (and the model's sorted records through the sorted entry
    point on `sorted_on`); returns the model's (bad count, single-digit flags)."""
    want, bad, s, single = m.expected(case, q0, eng.cells)
    eng.upload(q0)
    buf = eng.gathered(case)
    eng.expect_report(bad)
    got = eng.download()
    buf.free()
    _same(got, want, q0, s, "gathered")
    if sorted_on is not None:
        sorted_on.upload(q0)
        buf = _DevBuf(s)
        sorted_on._lib.check(sorted_on.lib.qe_delta_apply_sorted_dev(sorted_on.h, buf.ptr, s.shape[0]))
        sorted_on.expect_report(bad)
        got = sorted_on.download()
        buf.free()
        _same(got, want, q0, s, "sorted")
    return bad, single


# ------------------------------------------------------------------------------------------------ a. single-digit passes
@pytest.mark.parametrize(("name", "engine", "rank"), m.FAMILY_RUNS)
def test_single_digit_passes(name, engine, rank, small, large, q_small):
    eng, q0 = (large, large.q0) if engine == "large" else (small, q_small)
    bad, single = _run(eng, m.family(name, eng.cells, rank), q0)
    assert bad == 0 and tuple(single) == m.FAMILY_FLAGS[name][:m.passes_for(eng.cells)]


# ------------------------------------------------------------------------------------------------ b. batches of pass 0
@pytest.mark.parametrize("kind", m.BATCH_KINDS)
def test_batch_patterns_in_pass_0(kind, small, q_small):
    case = m.batch_case(kind)
    assert case.count % m.TILE == 37
    bad, single = _run(small, case, q_small)
    assert bad == 0 and single == [False, False, True]


# ------------------------------------------------------------------------------------------------ c. sizes
@pytest.mark.parametrize("n", m.SIZES)
def test_sizes(n, small, q_small):
    case = m.size_case(n, small.cells)
    assert (case.world, case.count) == (2, n)
    bad, _ = _run(small, case, q_small)
    assert bad == 0


def test_seven_ranks_with_one_record_each(small, q_small):
    case = m.eight_ranks_case(small.cells)
    assert (case.world, case.count) == (8, 1)
    assert _run(small, case, q_small)[0] == 0


def test_nothing_to_apply_leaves_the_table_alone(small, q_small):
    for case in m.empty_cases():  # count 0; world 1
        assert case.count == 0 or case.world == 1
        assert _run(small, case, q_small)[0] == 0  # (QE_OK from the call and from the synchronisation)


# ------------------------------------------------------------------------------------------------ d. one engine, many calls
def test_one_engine_many_calls():
    """A fresh engine: its scratch buffers and flag word are sized by the first, largest call and reused by the rest."""
    eng = _Engine(m.SMALL_S)
    try:
        cells = eng.cells
        q0 = m.initial(cells, seed=12)
        eng.upload(q0)
        q, touched, bufs = q0, [], []

        def queue(case):
            nonlocal q
            bufs.append(eng.gathered(case))
            q, bad, s, single = m.expected(case, q, cells)
            touched.append(s)
            return bad, single

        def settled(bad, what):
            eng.expect_report(bad)
            _same(eng.download(), q, q0, np.concatenate(touched), what)
            while bufs:
                bufs.pop().free()

        # 257 tiles, then 65 records, then a single-digit pass 0 before a mixed pass 1: no synchronisation in between
        assert queue(m.size_case(m.SIZES[-1], cells))[0] == 0
        assert queue(m.size_case(65, cells))[0] == 0
        assert queue(m.family("mid", cells)) == (0, [True, False, True])
        settled(0, "after three calls")
        assert queue(m.bad_case("streak"))[0] == 300
        settled(300, "after the call with bad records")
        assert queue(m.size_case(4097, cells))[0] == 0
        settled(0, "after the clean call")
        # two calls with bad records before one synchronisation: one report, carrying their sum
        assert queue(m.bad_case("ends"))[0] == 3
        assert queue(m.bad_case("streak", seed=13))[0] == 300
        settled(303, "after two calls with bad records")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ e. the run walk
@pytest.mark.parametrize("kind", m.BAD_KINDS)
def test_run_walk_edges(kind, small, small2, q_small):
    """Also sorted."""
    case = m.bad_case(kind)
    bad, _ = _run(small, case, q_small, sorted_on=small2)
    assert bad == {"ends": 3, "streak": 300, "all": 2 * case.count, "long_run": 0}[kind]


# ------------------------------------------------------------------------------------------------ f. special values
@pytest.mark.parametrize("group", m.SPECIAL_GROUPS)
def test_special_values(group, small, small2, q_small):
    """Also sorted.  The model is NumPy's float32 arithmetic: gradual underflow, no flush to zero."""
    case = m.special_case(group)
    q0 = q_small.copy()
    q0[list(case.init)] = list(case.init.values())
    assert len(case.init) == len(m.SPECIAL_RUNS[group])
    assert _run(small, case, q0, sorted_on=small2)[0] == 0


# ------------------------------------------------------------------------------------------------ g. exact atomics
@pytest.mark.parametrize("count", m.ATOMIC_COUNTS)
def test_atomic_apply_is_exact_on_dyadic_increments(count, small):
    q0 = m.dyadic_table(small.cells)
    rec = m.dyadic_records(count, small.cells)
    assert np.abs(rec[:, 1].view(np.float32)).sum() * 1024 + 4096 < 1 << 24  # every partial sum exact, in any order
    want, _ = m.apply_runs(q0, rec, small.cells)
    small.upload(q0)
    buf = _DevBuf(rec)
    small._lib.check(small.lib.qe_delta_apply_dev(small.h, buf.ptr, count))
    small.expect_report(0)
    _same(small.download(), want, q0, rec, "apply")
    buf.free()


@pytest.mark.parametrize("count", m.ATOMIC_COUNTS)
def test_atomic_apply_with_a_skip_window_is_exact(count, small):
    """Windows: empty (at the start, in the middle, at the end), the very start, the very end, a middle stretch, and
    everything -- a no-op."""
    q0 = m.dyadic_table(small.cells)
    rec = m.dyadic_records(count, small.cells)
    assert np.abs(rec[:, 1].view(np.float32)).sum() * 1024 + 4096 < 1 << 24  # every partial sum exact, in any order
    buf = _DevBuf(rec)
    for begin, end in m.skip_windows(count):
        keep = np.r_[0:begin, end:count]
        want, _ = m.apply_runs(q0, rec[keep], small.cells)
        small.upload(q0)
        small._lib.check(small.lib.qe_delta_apply_skip_dev(small.h, buf.ptr, count, begin, end))
        small.expect_report(0)
        _same(small.download(), want, q0, rec[keep], f"skip [{begin}, {end})")
        if (begin, end) == (0, count):
            assert np.array_equal(want.view(U32), q0.view(U32))
    buf.free()
