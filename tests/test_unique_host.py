"""unique / unique_consecutive, host side: the C ABI's argument checks (smhip_runs_count, smhip_runs), the planner (smhip_runs_plan) and
the Python binding's own checks -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma

NONE, ONE, TILES = sma.RUNS_ROUTE_NONE, sma.RUNS_ROUTE_ONE, sma.RUNS_ROUTE_TILES
V, I, C, INV = sma.RUNS_VALUES, sma.RUNS_INDEX, sma.RUNS_COUNTS, sma.RUNS_INVERSE
ENTRY_POINTS = ("smhip_runs_count", "smhip_runs", "smhip_runs_plan")
DTYPES = (np.float32, np.float64, np.int32, np.int64)


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def test_entry_points_and_constants_are_declared():
    names = sma.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in names
    assert sma.RUNS_NAN_DISTINCT == 1 and (V, I, C, INV) == (1, 2, 4, 8) and (NONE, ONE, TILES) == (0, 1, 2)
    with open(sma.HEADER) as f:
        flat = " ".join(f.read().split())
    for name, value in (("SMHIP_RUNS_NAN_DISTINCT", "1"), ("SMHIP_RUNS_VALUES", "1"), ("SMHIP_RUNS_INDEX", "2"), ("SMHIP_RUNS_COUNTS", "4"),
                        ("SMHIP_RUNS_INVERSE", "8"), ("SMHIP_RUNS_ROUTE_NONE", "0"), ("SMHIP_RUNS_ROUTE_ONE", "1"), ("SMHIP_RUNS_ROUTE_TILES", "2")):
        assert f"#define {name} {value}" in flat


def test_exports_match_the_header(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib.c, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_planner_routes_by_size(lib, dtype):
    _, _, (_, tile, threshold) = lib.runs_plan(dtype, 1000)
    assert tile == 256 * 8 * (16 // np.dtype(dtype).itemsize) and threshold >= tile and threshold % tile == 0
    # the same tile and the same threshold as the compaction by condition: the two share the prefix kernel and the grid
    assert (tile, threshold) == lib.select_plan("index", dtype, [1000], [1])[2][1:3]
    tiles_of = lambda n: -(-n // tile)  # noqa: E731
    for outputs in range(16):   # every subset of the four results; 0 is the count alone
        tiled = 2 if outputs == 0 else 4 if outputs & C else 3   # counts cost one more launch: the adjacent differences of the starts
        for flags in (0, sma.RUNS_NAN_DISTINCT):
            assert lib.runs_plan(dtype, 0, outputs, flags)[:2] == (NONE, 0)
            for n in (1, 2, tile - 1, tile, tile + 1, threshold):
                route, launches, info = lib.runs_plan(dtype, n, outputs, flags)
                assert (route, launches, info[0]) == (ONE, 1, tiles_of(n)), (outputs, n)
            for n in (threshold + 1, 70001 + threshold, 129 * tile + 5, (16 * 256 + 1) * tile):
                route, launches, info = lib.runs_plan(dtype, n, outputs, flags)
                assert (route, launches, info[0]) == (TILES, tiled, tiles_of(n)), (outputs, n)
            # 2^33 elements: the tiles are still right in int64, and the last element alone in its tile
            assert lib.runs_plan(dtype, 1 << 33, outputs, flags) == (TILES, tiled, ((1 << 33) // tile, tile, threshold))
            assert lib.runs_plan(dtype, (1 << 33) + 1, outputs, flags)[2][0] == (1 << 33) // tile + 1


def test_planner_refusals(lib):
    with pytest.raises(sma.SmhipError, match="flag"):
        lib.runs_plan(np.float32, 8, V, flags=2)
    with pytest.raises(sma.SmhipError, match="dtype"):
        lib.runs_plan(4, 8)
    with pytest.raises(sma.SmhipError, match="dtype"):
        lib.runs_plan(-1, 8)
    with pytest.raises(sma.SmhipError, match="negative"):
        lib.runs_plan(np.float32, -1)
    with pytest.raises(sma.SmhipError, match="2\\^59"):
        lib.runs_plan(np.float32, 1 << 59)
    with pytest.raises(sma.SmhipError, match="result bits"):
        lib.runs_plan(np.float32, 8, 16)


def test_argument_validation_needs_no_gpu(lib):
    f32, f64, i64 = sma.F32, sma.F64, sma.I64
    # stand in for device pointers: every call below is rejected before anything is dereferenced or launched
    S, ORD, VAL, IDX, CNT, INVS, WORD = (k << 20 for k in range(1, 8))
    BAD = sma.ERR_INVALID

    def msg():
        return lib.c.smhip_last_error().decode()

    # ---- runs_count
    def count(flags=0, dtype=f32, s=S, n=8, word=WORD):
        return lib.runs_count_raw(flags, dtype, s, n, word)

    assert count(flags=2) == BAD and "flag" in msg()
    assert count(flags=-1) == BAD and "flag" in msg()
    assert count(dtype=4) == BAD and "dtype" in msg()      # the four element types only: not the dot product's integer types
    assert count(dtype=-1) == BAD and "dtype" in msg()
    assert count(n=-1) == BAD and "negative" in msg()
    assert count(n=1 << 59) == BAD and "2^59" in msg()
    assert count(s=0) == BAD and "null" in msg()
    assert count(word=0) == BAD and "null" in msg()
    assert count(s=S + 2) == BAD and "aligned" in msg()
    assert count(dtype=f64, s=S + 4) == BAD and "aligned" in msg()
    assert count(word=WORD + 4) == BAD and "aligned" in msg()
    assert count(word=S + 24) == BAD and "overlaps" in msg()        # the last element of s
    assert count(dtype=i64, word=S + 56) == BAD and "overlaps" in msg()
    # (n == 0 with a count word touches the device to clear the word: tests/test_unique_gpu.py runs it)

    # ---- runs
    def runs(flags=0, dtype=f32, s=S, n=8, order=ORD, values=VAL, index=IDX, counts=CNT, inverse=INVS, cap=8, word=WORD):
        return lib.runs_raw(flags, dtype, s, n, order, values, index, counts, inverse, cap, word)

    assert runs(flags=4) == BAD and "flag" in msg()
    assert runs(dtype=5) == BAD and "dtype" in msg()
    assert runs(dtype=-2) == BAD and "dtype" in msg()
    assert runs(n=-8) == BAD and "negative" in msg()
    assert runs(n=1 << 59) == BAD and "2^59" in msg()
    assert runs(cap=-1) == BAD and "capacity" in msg()
    assert runs(s=0) == BAD and "null" in msg()
    assert runs(values=0, index=0, counts=0, inverse=0) == BAD and "all four" in msg()
    assert runs(values=0, index=0, counts=0, inverse=0, n=0) == BAD and "all four" in msg()
    for name in ("s", "values"):                                    # elements of 4 bytes, then of 8
        assert runs(**{name: (S if name == "s" else VAL) + 2}) == BAD and "aligned" in msg(), name
        assert runs(dtype=f64, **{name: (S if name == "s" else VAL) + 4}) == BAD and "aligned" in msg(), name
    for name, base in (("order", ORD), ("index", IDX), ("counts", CNT), ("inverse", INVS), ("word", WORD)):   # int64 words
        assert runs(**{name: base + 4}) == BAD and "aligned" in msg(), name
    # every result against every other span: s is 32 bytes, order and inverse 64, values 32 and index / counts 64 at this capacity
    for name, base in (("values", VAL), ("index", IDX), ("counts", CNT), ("inverse", INVS), ("word", WORD)):
        for other, at, last in (("s", S, 28), ("order", ORD, 56), ("values", VAL, 28), ("index", IDX, 56), ("counts", CNT, 56), ("inverse", INVS, 56), ("word", WORD, 0)):
            if other == name:
                continue
            assert runs(**{name: at + last // 8 * 8}) == BAD and "overlaps" in msg(), (name, other)
            assert all({"word": "count_dev"}.get(k, k) in msg() for k in (name, other)), (name, other, msg())
    # values, index and counts span min(capacity, n) items, whatever the capacity says ...
    assert runs(n=0, cap=1 << 40, index=VAL, word=0) == 0
    assert runs(s=0, order=0, n=0, cap=8, word=0) == 0                                  # no elements and no count word: nothing to do, whatever the pointers
    # ... and the inverse spans n words whatever the capacity
    assert runs(cap=0, word=INVS + 56) == BAD and "inverse_out overlaps count_dev" in msg()
    assert i64 == 3


def test_binding_checks(lib):
    def arr(dtype, shape=(8,)):
        """A DeviceArray that owns nothing: the binding's checks come before anything touches it."""
        st, acc = [], 1
        for d in reversed(shape):
            st.insert(0, acc)
            acc *= d
        return sma.DeviceArray(lib, 1 << 20, dtype, shape, st, 0, owner=object())

    for bad in (np.int16, np.uint32, np.complex64, np.float16):
        with pytest.raises(ValueError, match="dtype"):
            lib.unique(arr(bad))
        with pytest.raises(ValueError, match="dtype"):
            lib.unique_consecutive(arr(bad), return_counts=True)
    with pytest.raises(KeyError):
        lib.runs_plan(np.int16, 8)
