"""searchsorted / bincount / histogram, host side: the C ABI's argument checks, the planner (smhip_count_plan), the uniform edge
table against np.linspace bit for bit, and the Python binding's own checks -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma

NONE, LDS, GLOBAL, COPY = sma.COUNT_ROUTE_NONE, sma.COUNT_ROUTE_LDS, sma.COUNT_ROUTE_GLOBAL, sma.COUNT_COPY
ENTRY_POINTS = ("smhip_searchsorted", "smhip_bincount", "smhip_histogram", "smhip_histogram_edges", "smhip_count_plan")

# (lo, hi, bins): the issue's list
UNIFORM_CASES = ((0, 1, 1), (0, 1, 7), (-3, 5, 256), (0.1, 0.7, 1000), (-1e3, 1e3, 8193), (1, 1 + 2.0 ** -10, 64), (0, 255, 255), (-2.5, 2.5, 16384),
                 (-2.5, 2.5, 16385))


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def plan(lib, what, dtype, shape, bins, strides=None, **kw):
    """(route id, flags, launches, info)"""
    if strides is None:
        strides, acc = [], 1
        for d in reversed(shape):
            strides.insert(0, acc)
            acc *= d
    route, launches, info = lib.count_plan(what, dtype, shape, strides, bins, **kw)
    return route & 0xff, route & ~0xff, launches, info


def test_entry_points_and_constants_are_declared():
    names = sma.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in names
    assert (sma.SIDE_LEFT, sma.SIDE_RIGHT) == (0, 1)
    assert (NONE, LDS, GLOBAL, COPY) == (0, 1, 2, 0x100)
    assert sma.HISTOGRAM_UNIFORM == 1
    with open(sma.HEADER) as f:
        text = f.read()
    flat = " ".join(text.split())
    for name, value in (("SMHIP_COUNT_ROUTE_NONE", "0"), ("SMHIP_COUNT_ROUTE_LDS", "1"), ("SMHIP_COUNT_ROUTE_GLOBAL", "2"), ("SMHIP_COUNT_COPY", "0x100"),
                        ("SMHIP_HISTOGRAM_UNIFORM", "1")):
        assert f"#define {name} {value}" in flat
    assert "SMHIP_SIDE_LEFT = 0, SMHIP_SIDE_RIGHT = 1" in text
    assert "SMHIP_COUNT_SEARCHSORTED = 0, SMHIP_COUNT_BINCOUNT = 1, SMHIP_COUNT_HISTOGRAM = 2" in text


def test_exports_match_the_header(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib.c, name)


def test_argument_validation_needs_no_gpu(lib):
    f32, i64 = sma.F32, sma.I64
    # stand in for device pointers: every call below is rejected before anything is dereferenced or launched
    X, E, O, B = 1 << 20, 1 << 21, 1 << 22, 1 << 23
    INV = sma.ERR_INVALID

    def msg():
        return lib.c.smhip_last_error().decode()

    # searchsorted
    assert lib.searchsorted_raw(2, f32, E, 4, X, [8], [1], O) == INV and "side" in msg()
    assert lib.searchsorted_raw(-1, f32, E, 4, X, [8], [1], O) == INV
    assert lib.searchsorted_raw(0, 9, E, 4, X, [8], [1], O) == INV and "dtype" in msg()
    assert lib.searchsorted_raw(0, -1, E, 4, X, [8], [1], O) == INV
    assert lib.searchsorted_raw(0, f32, E, 4, X, [2] * 7, [1] * 7, O) == INV and "ndim" in msg()
    assert lib.searchsorted_raw(0, f32, E, 4, X, [], [], O, ndim=0) == INV
    assert lib.searchsorted_raw(0, f32, E, -1, X, [8], [1], O) == INV and "negative" in msg()
    assert lib.searchsorted_raw(0, f32, E, 4, X, [-8], [1], O) == INV
    assert lib.searchsorted_raw(0, f32, E, 4, X, [8], [-1], O) == INV
    assert lib.searchsorted_raw(0, f32, E, 4, X, None, [1], O, ndim=1) == INV and "null" in msg()
    assert lib.searchsorted_raw(0, f32, E, 4, X, [8], None, O, ndim=1) == INV
    assert lib.searchsorted_raw(0, f32, E, 4, 0, [8], [1], O) == INV and "null" in msg()
    assert lib.searchsorted_raw(0, f32, E, 4, X, [8], [1], 0) == INV
    assert lib.searchsorted_raw(0, f32, 0, 4, X, [8], [1], O) == INV
    assert lib.searchsorted_raw(0, f32, E, 4, X + 2, [8], [1], O) == INV and "aligned" in msg()
    assert lib.searchsorted_raw(0, f32, E, 4, X, [8], [1], X + 16) == INV and "overlaps" in msg()
    assert lib.searchsorted_raw(0, f32, E, 4, X, [8], [1], E) == INV
    assert lib.searchsorted_raw(0, f32, E, 4, X, [1 << 30, 1 << 30], [1 << 30, 1], O) == INV and "2^59" in msg()
    assert lib.searchsorted_raw(0, f32, 0, 4, 0, [0], [1], 0) == 0            # nothing to do, whatever the pointers

    # bincount
    assert lib.bincount_raw(3, i64, X, [8], [1], 4, O) == INV and "mode" in msg()
    assert lib.bincount_raw(0, f32, X, [8], [1], 4, O) == INV and "dtype" in msg()
    assert lib.bincount_raw(0, sma.F64, X, [8], [1], 4, O) == INV
    assert lib.bincount_raw(0, 9, X, [8], [1], 4, O) == INV
    assert lib.bincount_raw(0, i64, X, [2] * 7, [1] * 7, 4, O) == INV and "ndim" in msg()
    assert lib.bincount_raw(0, i64, X, [8], [1], -1, O) == INV and "negative" in msg()
    assert lib.bincount_raw(0, i64, X, [8], [1], 0, O) == INV and "0 bins" in msg()
    assert lib.bincount_raw(0, i64, 0, [8], [1], 4, O) == INV and "null" in msg()
    assert lib.bincount_raw(0, i64, X, [8], [1], 4, 0) == INV
    assert lib.bincount_raw(0, i64, X, [8], [1], 4, X + 8) == INV and "overlap" in msg()
    assert lib.bincount_raw(0, i64, X, [8], [1], 4, O, bad_ptr=O + 8) == INV
    assert lib.bincount_raw(0, i64, X, [8], [1], 4, O, bad_ptr=X) == INV
    assert lib.bincount_raw(0, i64, X, [8], [1], 4, O + 4) == INV and "aligned" in msg()
    assert lib.bincount_raw(0, i64, 0, [0], [1], 0, 0) == 0                    # an empty result of no ids

    # histogram
    assert lib.histogram_raw(0, 9, X, [8], [1], E, 4, 0.0, 0.0, O) == INV and "dtype" in msg()
    assert lib.histogram_raw(2, f32, X, [8], [1], E, 4, 0.0, 0.0, O) == INV and "flag" in msg()
    assert lib.histogram_raw(1, sma.I32, X, [8], [1], E, 4, 0.0, 1.0, O) == INV and "uniform" in msg()
    assert lib.histogram_raw(0, f32, X, [2] * 7, [1] * 7, E, 4, 0.0, 0.0, O) == INV and "ndim" in msg()
    assert lib.histogram_raw(0, f32, X, [8], [1], E, -1, 0.0, 0.0, O) == INV and "negative" in msg()
    assert lib.histogram_raw(0, f32, X, [8], [1], E, 0, 0.0, 0.0, O) == INV
    assert lib.histogram_raw(0, f32, 0, [8], [1], E, 4, 0.0, 0.0, O) == INV and "null" in msg()
    assert lib.histogram_raw(0, f32, X, [8], [1], 0, 4, 0.0, 0.0, O) == INV
    assert lib.histogram_raw(0, f32, X, [8], [1], E, 4, 0.0, 0.0, 0) == INV
    assert lib.histogram_raw(0, f32, X, [8], [1], E, 4, 0.0, 0.0, E + 16) == INV and "overlaps" in msg()
    assert lib.histogram_raw(1, f32, X, [8], [1], E, 4, 1.0, 0.0, O) == INV and "below" in msg()
    assert lib.histogram_raw(1, f32, X, [8], [1], E, 4, 0.0, float("inf"), O) == INV and "finite" in msg()
    assert lib.histogram_raw(1, f32, X, [8], [1], E, 4, float("nan"), 1.0, O) == INV
    assert lib.histogram_raw(1, f32, X, [8], [1], E, 0, 0.0, 1.0, O) == INV


def test_planner_routes(lib):
    K = plan(lib, "bincount", np.int64, [1000], 4)[3][3]
    assert K >= 256
    n = 1 << 24
    route, flags, launches, info = plan(lib, "bincount", np.int64, [n], K)
    assert (route, flags, launches) == (LDS, 0, 2) and info[2] == 1
    route, flags, launches, info = plan(lib, "bincount", np.int64, [n], K + 1)
    assert (route, flags, launches) == (GLOBAL, 0, 1) and info[2] == 1
    for what, dtype in (("histogram", np.float32), ("histogram", np.int64), ("bincount", np.int32)):
        assert plan(lib, what, dtype, [n], K)[0] == LDS and plan(lib, what, dtype, [n], K + 1)[0] == GLOBAL
    # small tables get replicas, and the replicas fit the K counters of LDS
    for bins in (1, 2, 255, 256, 257, 1000, K // 2, K // 2 + 1):
        replicas = plan(lib, "bincount", np.int64, [n], bins)[3][2]
        assert replicas >= 1 and replicas & (replicas - 1) == 0 and bins * replicas <= K
    assert plan(lib, "bincount", np.int64, [n], 256)[3][2] > 1
    # one slice: the workgroup widens into the result, no finishing launch
    route, _, launches, info = plan(lib, "bincount", np.int64, [100], 256)
    assert (route, launches, info[0]) == (LDS, 1, 1)
    # a 32-bit counter cannot wrap: a slice stays below 2^32 entries, also for 2^33 and 2^45 of them
    for log2n in (33, 45):
        route, _, launches, info = plan(lib, "bincount", np.int32, [1 << log2n], 256)
        assert route == LDS and 0 < info[1] < 1 << 32 and info[0] >= 1
    # a view that is not dense row-major is copied first
    route, flags, launches, _ = plan(lib, "bincount", np.int64, [300, 70], 256, strides=[1, 300])
    assert (route, flags, launches) == (LDS, COPY, 3)
    route, flags, launches, _ = plan(lib, "histogram", np.float32, [300, 70], K + 1, strides=[140, 2], uniform=True)
    assert (route, flags, launches) == (GLOBAL, COPY, 2)
    assert plan(lib, "searchsorted", np.float64, [300, 70], 5, strides=[1, 300])[:3] == (LDS, COPY, 2)
    assert plan(lib, "searchsorted", np.float64, [7, 300, 70], 5, strides=[0, 70, 1])[1] == COPY      # broadcast
    # nothing to do
    for what, dtype in (("searchsorted", np.float32), ("bincount", np.int64), ("histogram", np.float64)):
        assert plan(lib, what, dtype, [0], 16)[:3] == (NONE, 0, 0)
        assert plan(lib, what, dtype, [4, 0, 3], 16)[:3] == (NONE, 0, 0)
    assert plan(lib, "searchsorted", np.float32, [8], 0)[:3] == (NONE, 0, 0)
    assert plan(lib, "bincount", np.int64, [0], 0)[:3] == (NONE, 0, 0)


def test_planner_stages_the_edges_within_its_budget(lib):
    for dtype in (np.float32, np.float64, np.int32, np.int64):
        budget = plan(lib, "searchsorted", dtype, [1000], 4)[3][4]
        assert budget * np.dtype(dtype).itemsize >= 1024
        route, _, launches, info = plan(lib, "searchsorted", dtype, [1000], budget)
        assert (route, launches, info[5]) == (LDS, 1, 1)
        route, _, launches, info = plan(lib, "searchsorted", dtype, [1000], budget + 1)
        assert (route, launches, info[5]) == (GLOBAL, 1, 0)
        # a histogram stages bins + 1 edges
        assert plan(lib, "histogram", dtype, [1000], budget - 1)[3][5] == 1
        assert plan(lib, "histogram", dtype, [1000], budget)[3][5] == 0
    assert plan(lib, "bincount", np.int64, [1000], 4)[3][4:] == (0, 0)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_uniform_edges_are_numpys_bit_for_bit(lib, dtype):
    """np.linspace(lo, hi, bins + 1).astype(T), which is also what np.histogram(..., bins, range=(lo, hi)) returns for values of
    type T: equal as bytes in all cases."""
    for lo, hi, bins in UNIFORM_CASES:
        got = lib.histogram_edges(bins, lo, hi, dtype)
        want = np.linspace(lo, hi, bins + 1).astype(dtype)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (lo, hi, bins)
        numpys = np.histogram(np.zeros(1, dtype), bins, range=(lo, hi))[1]
        assert numpys.astype(dtype).tobytes() == got.tobytes(), (lo, hi, bins)
    # a range of one point is numpy's (lo - 0.5, hi + 0.5)
    for point, bins in ((3.0, 4), (0.0, 1), (-1e6, 10)):
        want = np.histogram(np.zeros(1, dtype), bins, range=(point, point))[1].astype(dtype)
        assert lib.histogram_edges(bins, point, point, dtype).tobytes() == want.tobytes()


def test_uniform_edges_refuse_what_numpy_refuses(lib):
    for dtype in (np.float32, np.float64):
        for lo, hi, bins in ((0, 1, 0), (0, 1, -3), (1, 0, 4), (0, np.inf, 4), (-np.inf, 0, 4), (np.nan, 1, 4), (0, np.nan, 4)):
            with pytest.raises(ValueError):
                np.histogram(np.zeros(1, dtype), bins, range=(lo, hi))
            with pytest.raises(ValueError):
                lib.histogram_edges(bins, lo, hi, dtype)
    # rounded to float32 only 9 distinct edges are left: numpy refuses it, and so does the helper; in float64 it is fine
    lo, hi, bins = 1.0, 1.0 + 2.0 ** -20, 64
    assert np.unique(np.linspace(lo, hi, bins + 1).astype(np.float32)).size == 9
    with pytest.raises(ValueError):
        np.histogram(np.zeros(1, np.float32), bins, range=(lo, hi))
    with pytest.raises(ValueError, match="too many bins"):
        lib.histogram_edges(bins, lo, hi, np.float32)
    assert lib.histogram_edges(bins, lo, hi, np.float64).tobytes() == np.linspace(lo, hi, bins + 1).tobytes()
    with pytest.raises(ValueError):
        lib.histogram_edges(4, 0, 1, np.int32)


def test_binding_checks(lib):
    def arr(dtype, shape=(8,), strides=None):
        """A DeviceArray that owns nothing: the binding's checks come before anything touches it."""
        if strides is None:
            strides, acc = [], 1
            for d in reversed(shape):
                strides.insert(0, acc)
                acc *= d
        return sma.DeviceArray(lib, 1 << 20, dtype, shape, strides, 0, owner=object())

    f, d, i, l = arr(np.float32), arr(np.float64), arr(np.int32), arr(np.int64)
    with pytest.raises(ValueError, match="side"):
        lib.searchsorted(f, f, side="middle")
    with pytest.raises(ValueError, match="edges are"):
        lib.searchsorted(d, f)
    with pytest.raises(ValueError, match="1-D"):
        lib.searchsorted(arr(np.float32, (2, 4)), f)
    with pytest.raises(ValueError, match="1-D"):
        lib.searchsorted(arr(np.float32, (4,), [2]), f)
    with pytest.raises(ValueError, match="out must"):
        lib.searchsorted(f, f, out=i)
    with pytest.raises(ValueError, match="out must"):
        lib.searchsorted(f, f, out=arr(np.int64, (7,)))
    with pytest.raises(ValueError, match="mode"):
        lib.bincount(l, 4, mode="fold")
    with pytest.raises(ValueError, match="int32 or int64"):
        lib.bincount(f, 4)
    with pytest.raises(ValueError, match="bins"):
        lib.bincount(l, 0)
    with pytest.raises(ValueError, match="bins"):
        lib.bincount(l, -2)
    with pytest.raises(ValueError, match="range"):
        lib.histogram(f, 8)
    with pytest.raises(ValueError, match="no range"):
        lib.histogram(f, f, range=(0, 1))
    with pytest.raises(ValueError, match="edges must"):
        lib.histogram(f, d)
    with pytest.raises(ValueError, match="edges must"):
        lib.histogram(f, arr(np.float32, (1,)))
    with pytest.raises(ValueError, match="float32 or float64"):
        lib.histogram(i, 8, range=(0, 1))
    for lo, hi, bins in ((1, 0, 4), (0, np.inf, 4), (0, 1, 0), (1.0, 1.0 + 2.0 ** -20, 64)):
        with pytest.raises(ValueError):
            lib.histogram(f, bins, range=(lo, hi))
