"""NumPy restatement of the deterministic apply step of the replica exchange (``csrc/qe_delta_sort.h``,
``k_delta_apply_sorted``, ``qe_delta_apply_gathered_dev``), and the inputs that drive it to its structural edges.

What the engine does with the gathered logs of ``world`` ranks (``capacity`` slots each, the first ``count`` filled):

* ``others``      -- the other ranks' records, rank-major, slot-minor (what ``dsort_src`` addresses);
* ``passes_for``  -- as many 8-bit passes as the bits of ``cells - 1`` need;
* ``lsd``         -- a stable sort on each 8-bit digit, least significant first; a pass in which one digit holds every
                     record is the engine's ordered copy ("keep order");
* ``apply_runs``  -- float32 additions into a cell in array order; records naming a cell outside the table are skipped
                     and counted.

The builders return ``Case`` tuples ``(world, capacity, count, rank, rec)`` with ``rec`` a ``(world, capacity, 2)``
uint32 array of {cell, float32 bits}; ``init`` holds initial cell values where a case needs particular ones.  Slots the
engine must NOT read (this rank's own segment, the tail of every partly filled segment) hold records of 1e30 on cells
the case touches: reading one of them changes a result.

tests/test_delta_sort_cases.py checks on this model alone that every case is what it claims to be;
tests/test_gpu_delta_sort_edges.py runs the cases on the device.
"""
from collections import namedtuple

import numpy as np

A = 16                                   # both engines: 16 actions, row stride 16 (no padding columns)
SMALL_S, LARGE_S = 4097, (1 << 20) + 1
SMALL_CELLS, LARGE_CELLS = SMALL_S * A, LARGE_S * A   # 65 552 (three passes) and 2^24 + 16 (four passes)
TILE, BATCH, BLOCK = 4096, 64, 256       # DSORT_TILE, a wavefront's batch, threads per block of the run walk
FAMILY_SHAPE = (3, 7000, 6145)           # world, capacity, count: 12 290 records = three tiles and two records
POISON = np.float32(1e30)

Case = namedtuple("Case", "world capacity count rank rec init", defaults=(None,))

# single-digit passes per family on the large engine (four passes); the small engine has the first three of them
FAMILY_FLAGS = {
    "low": (False, True, True, True),
    "mid": (True, False, True, True),
    "high": (True, True, False, True),
    "top": (False, True, True, False),
    "one": (True, True, True, True),
    "lowconst": (True, False, False, True),
}
# (family, engine, rank) of every run: all six on the large engine, `low`, `mid` and `one` on the small one as well,
# `mid` also as the first and as the last rank
FAMILY_RUNS = ([(name, "large", 1) for name in FAMILY_FLAGS] + [("low", "small", 1), ("mid", "small", 1),
               ("one", "small", 1), ("mid", "large", 0), ("mid", "large", 2)])
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 256 * 4096, 256 * 4096 + 1)
BATCH_KINDS = ("equal", "distinct", "alternating", "extremes", "last_lane")
BAD_KINDS = ("ends", "streak", "all", "long_run")
SPECIAL_GROUPS = ("nonfinite", "zeros", "subnormal")
ATOMIC_COUNTS = (1, 255, 256, 257, 5 * 256 + 77)


# ------------------------------------------------------------------------------------------------ the engine, restated
def passes_for(cells):
    bits = 1
    while bits < 32 and (cells - 1) >> bits:
        bits += 1
    return (bits + 7) // 8


def others(rec, count, rank):
    """The other ranks' first `count` records, rank-major: (n, 2) uint32."""
    parts = [rec[r, :count] for r in range(rec.shape[0]) if r != rank]
    return np.concatenate(parts) if parts else np.empty((0, 2), dtype=np.uint32)


def lsd(keys, passes):
    """(final order, [pass p had one digit only]) of the radix sort of `keys`."""
    keys = np.asarray(keys, dtype=np.uint32)
    order = np.arange(keys.size)
    single = []
    for p in range(passes):
        digit = ((keys[order] >> np.uint32(8 * p)) & np.uint32(0xFF)).astype(np.uint8)
        single.append(bool(digit.size) and bool((digit == digit[0]).all()))
        order = order[np.argsort(digit, kind="stable")]
    return order, single


def apply_runs(q_flat, sorted_records, cells):
    """(table, bad): every record with cell < `cells` added to its cell in float32, in array order."""
    cell, delta = sorted_records[:, 0], np.ascontiguousarray(sorted_records[:, 1]).view(np.float32)
    valid = cell < cells
    out = np.array(q_flat, dtype=np.float32, copy=True)
    with np.errstate(all="ignore"):
        np.add.at(out, cell[valid].astype(np.int64), delta[valid])  # sequential, in array order
    return out, int((~valid).sum())


def expected(case, q_flat, cells):
    """(table, bad, sorted records, single-digit flags) of one gathered apply of `case` to `q_flat`."""
    o = others(case.rec, case.count, case.rank)
    order, single = lsd(o[:, 0], passes_for(cells))
    s = np.ascontiguousarray(o[order])
    table, bad = apply_runs(q_flat, s, cells)
    return table, bad, s, single


# ------------------------------------------------------------------------------------------------ pieces of an input
def increments(rng, n):
    """Six decades of magnitude: the order of the additions into a cell shows in the bits of the sum."""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)


def pack(cell, delta):
    out = np.empty((len(cell), 2), dtype=np.uint32)
    out[:, 0] = np.asarray(cell, dtype=np.uint64).astype(np.uint32)
    out[:, 1] = np.asarray(delta, dtype=np.float32).view(np.uint32)
    return out


def initial(cells, seed=1):
    return np.random.default_rng(seed).standard_normal(cells).astype(np.float32)


def spread(stream, world, capacity, count, rank, rng):
    """`stream` = the (world - 1) * count records of the other ranks in apply order, laid into a gathered buffer."""
    assert stream.shape == ((world - 1) * count, 2) and count <= capacity and 0 <= rank < world
    rec = np.empty((world, capacity, 2), dtype=np.uint32)
    pool = stream[:, 0] if stream.size else np.zeros(1, dtype=np.uint32)
    rec[..., 0] = pool[rng.integers(0, pool.size, size=(world, capacity))]
    rec[..., 1] = POISON.view(np.uint32)
    at = 0
    for r in range(world):
        if r != rank:
            rec[r, :count] = stream[at:at + count]
            at += count
    return Case(world, capacity, count, rank, rec)


# ------------------------------------------------------------------------------------------------ a. single-digit passes
def family_keys(name, n, cells, rng):
    if name == "low":
        return rng.integers(0, 256, n)
    if name == "mid":
        return rng.integers(0, 256, n) << 8
    if name == "high":
        return rng.integers(0, 256, n) << 16
    if name == "top":  # exactly half of the records in each group of sixteen cells
        return rng.integers(0, 16, n) + rng.permutation(np.arange(n) % 2) * (1 << 24)
    if name == "one":
        return np.full(n, 0x1234)
    if name == "lowconst":
        return (rng.integers(0, (cells - 0x5A - 1 >> 8) + 1, n) << 8) | 0x5A
    raise KeyError(name)


def family(name, cells, rank=1, seed=0):
    world, capacity, count = FAMILY_SHAPE
    rng = np.random.default_rng(seed)
    n = (world - 1) * count
    keys = family_keys(name, n, cells, rng)
    assert keys.max() < cells, name
    return spread(pack(keys, increments(rng, n)), world, capacity, count, rank, rng)


# ------------------------------------------------------------------------------------------------ b. batches of pass 0
def batch_digits(kind, n, rng):
    """The low byte of record i, i in apply order: batches are the aligned groups of 64 records."""
    i = np.arange(n)
    b = i // BATCH
    if kind == "equal":
        return (b * 7) % 256
    if kind == "distinct":
        return (i * 5 + b * 3) % 256
    if kind == "alternating":
        return np.where(i % 2 == 0, b % 256, (b + 129) % 256)
    if kind == "extremes":
        d = rng.integers(0, 2, n) * 255
        d[n - n % BATCH::3] = 0  # live records of digit 0 in the ragged batch, beside lanes that hold nothing
        return d
    if kind == "last_lane":
        return np.where(i % BATCH == BATCH - 1, (b * 7 + 1) % 256, (b * 7) % 256)
    raise KeyError(kind)


def batch_case(kind, tiles=2, seed=2):
    """World 2: n = count = `tiles` tiles + 37 records on the small engine; eight values of the second byte, so cells
    repeat and pass 1 is mixed."""
    rng = np.random.default_rng(seed)
    n = tiles * TILE + 37
    keys = (rng.integers(0, 8, n) << 8) | batch_digits(kind, n, rng)
    return spread(pack(keys, increments(rng, n)), 2, n + 5, n, 1, rng)


# ------------------------------------------------------------------------------------------------ c. sizes
def size_case(n, cells, seed=3):
    rng = np.random.default_rng(seed + n)
    keys = rng.integers(0, cells, n)
    return spread(pack(keys, increments(rng, n)), 2, n + (3 if n < 10000 else 0), n, n % 2, rng)


def eight_ranks_case(cells, seed=4):
    """World 8, count 1: seven records, each from another rank's segment."""
    rng = np.random.default_rng(seed)
    keys = np.array([5, cells - 1, 5, 0, 300, 5, 0x10005 if cells > 0x10005 else 7])
    return spread(pack(keys, increments(rng, 7)), 8, 5, 1, 3, rng)


def empty_cases():
    """Count 0 (world 3), and world 1 with a filled segment: nothing to apply."""
    rng = np.random.default_rng(5)
    none = np.empty((0, 2), dtype=np.uint32)
    return [spread(none, 3, 4, 0, 1, rng), spread(none, 1, 6, 5, 0, rng)]


# ------------------------------------------------------------------------------------------------ e. the run walk
def bad_case(kind, seed=6):
    """On the small engine (three passes: records are filed by their low 24 bits).  World 3, rank 2."""
    cells = SMALL_CELLS
    rng = np.random.default_rng(seed)
    hot = 0x1234
    if kind == "ends":  # a bad record in front of cell 0's run, one behind the last cell's, one alone in the middle
        keys = rng.integers(0, cells, 700)
        keys[0], keys[1:4] = 1 << 24, 0
        keys[350], keys[351] = 0xFFFFFFFF, cells
        keys[600:603] = cells - 1
    elif kind == "streak":  # 300 bad records inside the hot cell's run: they share its low 24 (so its low 16) bits
        keys = rng.integers(0, cells, 900)
        keys[100:140] = hot
        keys[140:440] = hot | ((1 + np.arange(300) % 255) << 24)
        keys[440:480] = hot
    elif kind == "all":
        keys = np.concatenate([cells + rng.integers(0, 1 << 20, 300), rng.integers(1 << 24, 1 << 32, 300),
                               [cells, 0xFFFFFFFF]])
    elif kind == "long_run":  # 5000 records of one cell, its neighbours with one record each
        keys = np.concatenate([np.full(5000, hot), hot - 1 - np.arange(40), hot + 1 + np.arange(40),
                               rng.choice(np.arange(0x2000, cells), 320, replace=False)])
        keys = keys[rng.permutation(keys.size)]
    else:
        raise KeyError(kind)
    n = keys.size
    assert n % 2 == 0
    return spread(pack(keys, increments(rng, n)), 3, n // 2 + 9, n // 2, 2, rng)


# ------------------------------------------------------------------------------------------------ f. special values
F32 = np.float32
INF, NAN, FMAX, FMIN, TINY = F32(np.inf), F32(np.nan), np.finfo(F32).max, np.finfo(F32).tiny, F32(1e-45)
SUB = F32(1e-40)  # subnormal
# group -> [(initial value, increments in order)]
SPECIAL_RUNS = {
    "nonfinite": [
        (F32(0.0), [INF, -INF, F32(1.0)]),            # inf + -inf = NaN, and stays NaN
        (F32(1.0), [INF, F32(-3.0)]),
        (F32(1.0), [-INF]),
        (FMAX, [FMAX, -INF]),                         # overflow to inf, then -inf: NaN
        (FMAX, [FMAX, F32(-1.0), -FMAX]),             # overflow to inf, and stays inf
        (FMAX, [-FMAX, F32(0.5)]),
        (FMAX, [F32(1e30), F32(1e31)]),               # FLT_MAX + less than half an ulp: unchanged
        (NAN, [F32(1.0)]),
        (F32(2.0), [NAN, F32(1.0)]),
        (-INF, [F32(1.0), INF]),
        (F32(0.0), [FMAX, FMAX, -FMAX]),
    ],
    "zeros": [
        (F32(-0.0), [F32(-0.0), F32(-0.0)]),          # stays -0.0
        (F32(-0.0), [F32(-0.0), F32(0.0)]),           # -0.0 + 0.0 = +0.0
        (F32(0.0), [F32(-0.0)]),
        (F32(-0.0), [F32(1.5), F32(-1.5)]),           # x - x = +0.0
        (F32(1.0), [F32(0.0), F32(-0.0)]),
        (F32(-0.0), [F32(-0.0)] * 70),                # longer than a batch
    ],
    "subnormal": [
        (SUB, [F32(2e-41), F32(-3e-41)]),             # stays subnormal
        (F32(0.0), [TINY, TINY, TINY]),               # multiples of the smallest subnormal
        (FMIN, [-SUB]),                               # normal -> subnormal
        (SUB, [F32(1.2e-38)]),                        # subnormal -> normal
        (F32(1.0), [SUB, -SUB]),
        (F32(-0.0), [TINY, -TINY]),                   # -> +0.0 through subnormals
        (SUB, [F32(-0.0), F32(0.0)]),
        (F32(0.0), [SUB] * 5),
    ],
}


def special_case(group, seed=7):
    """The runs of SPECIAL_RUNS[group] on cells spread over the small table, their records dealt round-robin (so the
    sort has work to do; within a cell the order is kept), among 600 ordinary records on other cells.  World 3, rank 0."""
    rng = np.random.default_rng(seed)
    runs = SPECIAL_RUNS[group]
    at = 0x0100 + 0x0311 * np.arange(len(runs))  # distinct cells, both lower key bytes vary
    queue = [[(c, d) for d in incs] for c, (_, incs) in zip(at, runs)]
    special = []
    while any(queue):
        for q in queue:
            if q:
                special.append(q.pop(0))
    other = np.setdiff1d(np.arange(SMALL_CELLS), at)
    keys = list(rng.choice(other, 300)) + [c for c, _ in special] + list(rng.choice(other, 300 + len(special) % 2))
    delta = np.concatenate([increments(rng, 300), np.array([d for _, d in special], dtype=F32),
                            increments(rng, len(keys) - 300 - len(special))])
    n = len(keys)
    case = spread(pack(keys, delta), 3, n // 2 + 4, n // 2, 0, rng)
    return case._replace(init={int(c): v for c, (v, _) in zip(at, runs)})


# ------------------------------------------------------------------------------------------------ g. exact atomics
DYADIC = F32(2.0 ** -10)


def dyadic_table(cells, seed=8):
    """Multiples of 2^-10 in [-4, 4]."""
    return (np.random.default_rng(seed).integers(-4096, 4097, cells) * DYADIC).astype(F32)


def dyadic_records(count, cells, seed=9):
    """`count` records {cell, k * 2^-10}, |k| <= 1024, on 24 cells (cell 0 and the last cell among them): every partial
    sum into a cell, in any order, is a multiple of 2^-10 below 2^14 -- exact in float32."""
    rng = np.random.default_rng(seed + count)
    few = np.concatenate([[0, cells - 1], rng.choice(np.arange(1, cells - 1), 22, replace=False)])
    return pack(few[rng.integers(0, few.size, count)], (rng.integers(-1024, 1025, count) * DYADIC).astype(F32))


def skip_windows(count):
    """[begin, end) of the records left out: empty ones, the very start, the very end, a middle stretch, everything."""
    k = max(1, count // 3)
    return [(0, 0), (count // 2, count // 2), (count, count), (0, k), (count - k, count), (count // 3, count // 3 + k),
            (0, count)]
