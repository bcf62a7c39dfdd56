"""The inputs of tests/test_gpu_delta_sort_edges.py test what they claim: properties of the NumPy model of the
deterministic apply step alone (delta_sort_model.py), checked without a device.

* the model itself: the pass count, the rank-major view, the radix sort against a stable sort on the low ``8 * passes``
  bits (and NOT on the full key), the run sums against a scalar loop and against ``_expected`` of
  test_gpu_delta_apply.py;
* the single-digit flags of every family are exactly the listed ones, on both engines and for every rank;
* order sensitivity: in every family with at least 32 cells of 8 or more records, the float32 sum of more than half of
  those runs differs in its bits from the sum of the reversed run -- a sort that is not stable cannot pass;
* the batch patterns put into every 64-record batch of pass 0 what they say;
* bad records sit where the case says in the model's sorted order;
* the special-value runs reach inf + -inf, -0.0 + -0.0, -0.0 + 0.0, overflow followed by -inf, and subnormal sums;
* the atomic cases keep every partial sum, in any order, exactly representable.

Every test prints the figures it asserts on (``pytest -s``).
"""
import numpy as np
import pytest

import delta_sort_model as m

F32 = np.float32


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _keys(case):
    return m.others(case.rec, case.count, case.rank)[:, 0]


# ------------------------------------------------------------------------------------------------ the model
def test_pass_count_follows_the_bits_of_the_last_cell():
    want = {1: 1, 2: 1, 256: 1, 257: 2, 8000: 2, 1 << 16: 2, m.SMALL_CELLS: 3, 1 << 24: 3, (1 << 24) + 1: 4,
            m.LARGE_CELLS: 4, (1 << 32) - 4: 4}
    assert {c: m.passes_for(c) for c in want} == want


def test_others_is_rank_major_and_leaves_out_the_own_segment_and_the_tails():
    rec = np.arange(4 * 5 * 2, dtype=np.uint32).reshape(4, 5, 2)
    got = m.others(rec, 3, 2)
    assert got.tolist() == [rec[r, s].tolist() for r in (0, 1, 3) for s in range(3)]
    assert m.others(rec, 0, 1).shape == (0, 2) and m.others(rec[:1], 4, 0).shape == (0, 2)


def test_spread_fills_every_slot_the_engine_must_not_read_with_poison():
    case = m.family("low", m.SMALL_CELLS)
    world, capacity, count = m.FAMILY_SHAPE
    assert case[:4] == (world, capacity, count, 1) and case.rec.shape == (world, capacity, 2)
    live = np.zeros((world, capacity), dtype=bool)
    live[[0, 2], :count] = True
    assert (case.rec[~live, 1].view(F32) == m.POISON).all() and not (case.rec[live, 1].view(F32) == m.POISON).any()
    assert np.isin(case.rec[~live, 0], case.rec[live, 0]).all()  # ... on cells the case touches


@pytest.mark.parametrize("cells", [m.SMALL_CELLS, m.LARGE_CELLS])
def test_radix_order_is_a_stable_sort_on_the_low_bits_only(cells):
    passes = m.passes_for(cells)
    rng = np.random.default_rng(0)
    keys = rng.integers(0, 1 << 32, 20000).astype(np.uint32)
    keys[::3] = keys[1::3][:keys[::3].size] & np.uint32(0xFFFF)  # repeated keys
    order, single = m.lsd(keys, passes)
    mask = np.uint32((1 << 8 * passes) - 1) if passes < 4 else np.uint32(0xFFFFFFFF)
    assert np.array_equal(order, np.argsort(keys & mask, kind="stable"))
    assert single == [False] * passes
    if passes < 4:
        assert not np.array_equal(order, np.argsort(keys, kind="stable"))


def test_run_sums_equal_a_scalar_loop():
    case = m.bad_case("streak")
    q0 = m.initial(m.SMALL_CELLS)
    table, bad, s, _ = m.expected(case, q0, m.SMALL_CELLS)
    want, skipped = q0.copy(), 0
    for cell, word in s.tolist():
        if cell >= m.SMALL_CELLS:
            skipped += 1
            continue
        want[cell] = F32(want[cell]) + np.array(word, dtype=np.uint32).view(F32)
    assert bad == skipped == 300
    assert np.array_equal(_bits(table), _bits(want))


def test_model_agrees_with_the_simulation_of_the_existing_module():
    """One parameter set of test_gpu_delta_apply.py: (S, A, world, capacity, count, rank, hot) = (1000, 8, 3, 4000, 3000,
    1, 0.3), unpadded rows."""
    from test_gpu_delta_apply import _expected, _records

    S, A_, world, capacity, count, rank, hot = 1000, 8, 3, 4000, 3000, 1, 0.3
    rng = np.random.default_rng(S + world)
    q0 = rng.standard_normal((S, A_)).astype(F32)
    rec = _records(rng, world, capacity, count, S * A_, hot)
    uniq, acc, sorted_others = _expected(lambda cells: q0.ravel()[cells], rec, count, rank)
    table, bad, s, _ = m.expected(m.Case(world, capacity, count, rank, rec), q0.ravel(), S * A_)
    assert bad == 0 and np.array_equal(s, sorted_others)
    want = q0.ravel().copy()
    want[uniq] = acc
    assert np.array_equal(_bits(table), _bits(want))


# ------------------------------------------------------------------------------------------------ a. families
@pytest.mark.parametrize(("name", "engine", "rank"), m.FAMILY_RUNS)
def test_single_digit_passes_of_every_family(name, engine, rank):
    cells = m.LARGE_CELLS if engine == "large" else m.SMALL_CELLS
    case = m.family(name, cells, rank)
    keys = _keys(case)
    order, single = m.lsd(keys, m.passes_for(cells))
    print(f"{name} on the {engine} engine as rank {rank}: {keys.size} records, {np.unique(keys).size} cells, "
          f"single-digit passes {[p for p, f in enumerate(single) if f]}")
    assert keys.size == 12290 == 3 * m.TILE + 2 and keys.max() < cells
    assert tuple(single) == m.FAMILY_FLAGS[name][:m.passes_for(cells)]
    assert np.array_equal(order, np.argsort(keys, kind="stable"))  # all valid: the full key sorts the same
    mid = [m.family("mid", cells, r) for r in (0, 1, 2)]  # the same stream whatever the rank
    assert all(np.array_equal(_keys(c), _keys(mid[0])) for c in mid)


def _order_sensitive(case):
    """(cells with 8 or more records, those whose float32 sum from 0 differs in its bits when the run is reversed)."""
    o = m.others(case.rec, case.count, case.rank)
    o = o[np.argsort(o[:, 0], kind="stable")]
    cell, delta = o[:, 0], np.ascontiguousarray(o[:, 1]).view(F32)
    starts = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
    ends = np.r_[starts[1:], cell.size]
    long_, differ = 0, 0
    for a, b in zip(starts, ends):
        if b - a < 8:
            continue
        long_ += 1
        run = delta[a:b]
        fwd = np.add.accumulate(run, dtype=F32)[-1]
        rev = np.add.accumulate(run[::-1], dtype=F32)[-1]
        differ += int(fwd.view(np.uint32) != rev.view(np.uint32))
    return long_, differ


@pytest.mark.parametrize("name", ["low", "mid", "high", "top", "lowconst", "one"])
def test_most_long_runs_are_order_sensitive(name):
    long_, differ = _order_sensitive(m.family(name, m.LARGE_CELLS))
    print(f"{name}: {differ} of {long_} cells with 8 or more records are order-sensitive")
    if name in ("lowconst", "one"):  # sparse (mostly single records) / a single cell: fewer than 32 such cells, exempt
        assert long_ < 32
        return
    assert long_ >= 32 and 2 * differ > long_


@pytest.mark.parametrize("kind", m.BATCH_KINDS)
def test_batch_cases_are_order_sensitive_too(kind):
    long_, differ = _order_sensitive(m.batch_case(kind))
    print(f"batch pattern {kind}: {differ} of {long_} cells with 8 or more records are order-sensitive")
    if long_ >= 32:
        assert 2 * differ > long_
    else:
        assert kind == "extremes" and long_ == 16 and 2 * differ > long_  # 2 digits x 8 second bytes


# ------------------------------------------------------------------------------------------------ b. batches
@pytest.mark.parametrize("kind", m.BATCH_KINDS)
def test_every_batch_of_pass_0_holds_its_pattern(kind):
    case = m.batch_case(kind)
    keys = _keys(case)
    n = keys.size
    assert n == case.count == 2 * m.TILE + 37 and keys.max() < m.SMALL_CELLS
    digit = keys & 0xFF
    whole = digit[:n - 37].reshape(-1, m.BATCH)
    ragged = digit[n - 37:]
    distinct = np.array([np.unique(b).size for b in whole])
    if kind == "equal":
        assert (distinct == 1).all() and np.unique(ragged).size == 1
    elif kind == "distinct":
        assert (distinct == m.BATCH).all() and np.unique(ragged).size == 37
    elif kind == "alternating":
        assert (distinct == 2).all() and (whole[:, 0::2] == whole[:, :1]).all() and (whole[:, 1::2] == whole[:, 1:2]).all()
    elif kind == "extremes":
        assert np.isin(digit, (0, 255)).all() and (distinct == 2).all()
        assert (ragged == 0).any() and (ragged == 255).any()  # live records of digit 0 beside 27 dead lanes
    else:
        assert (distinct == 2).all() and (whole[:, :-1] == whole[:, :1]).all() and (whole[:, -1] != whole[:, 0]).all()
    _, single = m.lsd(keys, 3)
    assert single == [False, False, True]  # cells below 2^16
    assert np.unique(keys).size < n // 2   # cells repeat


# ------------------------------------------------------------------------------------------------ c. sizes
def test_sizes_sit_on_the_edges_of_batch_block_tile_and_scan_chunk():
    assert m.SIZES == (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 1048576, 1048577)
    tiles = [-(-n // m.TILE) for n in m.SIZES]
    assert tiles[-2:] == [256, 257]  # 256 tiles fill the scan's first chunk; one more opens the second
    for n in m.SIZES[:-2]:
        case = m.size_case(n, m.SMALL_CELLS)
        assert (case.world, case.count, case.rank) == (2, n, n % 2) and _keys(case).size == n
    assert np.unique(_keys(m.size_case(8192, m.SMALL_CELLS)) >> 16).size == 2  # pass 2 is mixed
    eight = m.eight_ranks_case(m.SMALL_CELLS)
    assert (eight.world, eight.count) == (8, 1) and _keys(eight).size == 7 and np.unique(_keys(eight)).size < 7
    for case in m.empty_cases():
        assert _keys(case).size == 0


# ------------------------------------------------------------------------------------------------ e. bad records
def _sorted_bad(kind):
    case = m.bad_case(kind)
    table, bad, s, _ = m.expected(case, m.initial(m.SMALL_CELLS), m.SMALL_CELLS)
    return case, table, bad, s, s[:, 0] >= m.SMALL_CELLS


def test_bad_records_first_and_last_in_sorted_order():
    _, _, bad, s, is_bad = _sorted_bad("ends")
    assert bad == 3 and is_bad[0] and is_bad[-1] and is_bad[-2] and not is_bad[1:-2].any()
    assert s[1, 0] == 0 and s[-3, 0] == m.SMALL_CELLS - 1  # ... beside runs of the first and the last cell


def test_streak_of_bad_records_sits_inside_one_cells_run():
    case, _, bad, s, is_bad = _sorted_bad("streak")
    hot = 0x1234
    at = np.flatnonzero(is_bad)
    assert bad == 300 > m.BLOCK and np.array_equal(at, np.arange(at[0], at[0] + 300))
    assert ((s[at, 0] & 0xFFFFFF) == hot).all() and ((s[at, 0] & 0xFFFF) == hot).all()
    run = np.flatnonzero(s[:, 0] == hot)
    assert run.size >= 80 and run[0] < at[0] and run[-1] > at[-1] and (run < at[0]).sum() >= 40 <= (run > at[-1]).sum()
    assert at[0] // m.BLOCK != at[-1] // m.BLOCK  # the streak crosses a block of the run walk
    # a sort on the full key would file them behind every valid record instead
    o = m.others(case.rec, case.count, case.rank)
    assert (o[np.argsort(o[:, 0], kind="stable")][-300:, 0] >= m.SMALL_CELLS).all()


def test_all_bad_and_long_run_cases():
    case, table, bad, s, is_bad = _sorted_bad("all")
    assert bad == s.shape[0] == 602 and is_bad.all() and np.array_equal(_bits(table), _bits(m.initial(m.SMALL_CELLS)))
    case, table, bad, s, is_bad = _sorted_bad("long_run")
    cell, n = np.unique(s[:, 0], return_counts=True)
    hot = np.flatnonzero(cell == 0x1234)[0]
    assert bad == 0 and n[hot] == 5000 and (n[hot - 40:hot] == 1).all() and (n[hot + 1:hot + 41] == 1).all()
    assert np.array_equal(cell[hot - 1:hot + 2], [0x1233, 0x1234, 0x1235])


# ------------------------------------------------------------------------------------------------ f. special values
def _special(group):
    case = m.special_case(group)
    q0 = m.initial(m.SMALL_CELLS)
    for c, v in case.init.items():
        q0[c] = v
    table, bad, s, _ = m.expected(case, q0, m.SMALL_CELLS)
    assert bad == 0
    cells = sorted(case.init)
    for c, (v, incs) in zip(cells, m.SPECIAL_RUNS[group]):  # the run of every special cell, in the order written down
        assert _bits(q0[c]) == _bits(v)
        assert np.array_equal(s[s[:, 0] == c, 1], _bits(np.array(incs, dtype=F32)))
    return [table[c] for c in cells], [q0[c] for c in cells]


def test_special_runs_reach_the_nonfinite_sums():
    got, _ = _special("nonfinite")
    print("nonfinite:", got)
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == -np.inf and np.isnan(got[3]) and got[4] == np.inf
    assert got[5] == 0.5 and got[6] == m.FMAX and np.isnan(got[7]) and np.isnan(got[8]) and np.isnan(got[9])
    assert got[10] == np.inf


def test_special_runs_reach_the_signed_zero_sums():
    got, _ = _special("zeros")
    neg, pos = _bits(F32(-0.0)), _bits(F32(0.0))
    assert [int(_bits(g)[0]) for g in got] == [int(neg[0]), int(pos[0]), int(pos[0]), int(pos[0]), int(_bits(F32(1.0))[0]),
                                              int(neg[0])]


def test_special_runs_stay_subnormal_where_they_say():
    got, _ = _special("subnormal")
    print("subnormal:", [float(g) for g in got])
    tiny = np.finfo(F32).tiny
    sub = lambda x: 0 < abs(float(x)) < tiny  # noqa: E731
    assert sub(got[0]) and got[1] == F32(3) * m.TINY and sub(got[2]) and got[3] >= tiny and got[4] == 1.0
    assert _bits(got[5]) == _bits(F32(0.0)) and _bits(got[6]) == _bits(m.SUB) and sub(got[7])
    for v, incs in m.SPECIAL_RUNS["subnormal"]:
        assert any(sub(x) for x in [v, *incs])


# ------------------------------------------------------------------------------------------------ g. exact atomics
@pytest.mark.parametrize("count", m.ATOMIC_COUNTS)
def test_atomic_inputs_keep_every_partial_sum_exact(count):
    q0 = m.dyadic_table(m.SMALL_CELLS)
    rec = m.dyadic_records(count, m.SMALL_CELLS)
    cell, delta = rec[:, 0].astype(np.int64), rec[:, 1].view(F32).astype(np.float64)
    for x in (q0.astype(np.float64), delta):
        k = x * 1024
        assert np.array_equal(k, np.round(k))
    worst = np.abs(q0.astype(np.float64)) * 1024
    np.add.at(worst, cell, np.abs(delta) * 1024)
    print(f"count {count}: largest sum of magnitudes {worst.max():.0f} * 2^-10 (exact below 2^24)")
    assert worst.max() < 1 << 24  # any partial sum, in any order, is an integer below 2^24 times 2^-10
    assert rec.shape[0] == count and cell.max() == m.SMALL_CELLS - 1 or count < 50
    for begin, end in m.skip_windows(count):
        assert 0 <= begin <= end <= count
    w = m.skip_windows(count)
    assert (0, 0) in w and (count, count) in w and (0, count) in w and any(b == 0 < e for b, e in w)
    assert any(b < e == count for b, e in w)
