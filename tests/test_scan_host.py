"""Cumulative scans, host side: the C ABI's argument checks and the planner (smhip_scan_plan) -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def dense(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= d
    return list(reversed(st))


def plan(lib, shape, axis, strides=None, kind="cumsum", dtype=np.float32):
    """(route id, flags, launches, (O, R, I), chunk)"""
    route, launches, ori, chunk = lib.scan_plan(kind, dtype, list(shape), dense(shape) if strides is None else list(strides), axis)
    return route & 0xff, route & ~0xff, launches, ori, chunk


def test_scan_entry_points_are_declared():
    names = sma.declared_symbols()
    assert "smhip_scan_axis" in names and "smhip_scan_plan" in names
    assert sma.SCAN_KINDS == {"cumsum": 0, "cumprod": 1, "cummax": 2, "cummin": 3}


def test_argument_validation_needs_no_gpu(lib):
    f32 = sma.F32
    P = 4096  # stands in for a device pointer: every call below is rejected before anything is dereferenced or launched
    bad = [
        (4, f32, P, [4], [1], 0, P + 4096, None),               # kind
        (sma.SCAN_SUM, sma.I8, P, [4], [1], 0, P + 4096, None),  # dtype
        (sma.SCAN_SUM, f32, P, [], [], 0, P + 4096, 0),          # ndim 0
        (sma.SCAN_SUM, f32, P, [2] * 7, dense([2] * 7), 0, P + 4096, None),  # ndim 7
        (sma.SCAN_SUM, f32, P, [4, 4], [4, 1], -1, P + 4096, None),   # axis -1 (the C ABI does not count from the end)
        (sma.SCAN_SUM, f32, P, [4, 4], [4, 1], 2, P + 4096, None),    # axis == ndim
        (sma.SCAN_SUM, f32, P, [4, -1], [4, 1], 0, P + 4096, None),   # negative extent
        (sma.SCAN_SUM, f32, P, [4, 4], [4, -1], 0, P + 4096, None),   # negative stride
        (sma.SCAN_SUM, f32, 0, [4], [1], 0, P + 4096, None),          # null a
        (sma.SCAN_SUM, f32, P, None, [1], 0, P + 4096, 1),            # null shape
        (sma.SCAN_SUM, f32, P, [4], None, 0, P + 4096, 1),            # null strides
        (sma.SCAN_SUM, f32, P, [4], [1], 0, 0, None),                 # null out
        (sma.SCAN_SUM, f32, P, [4, 4], [1, 4], 0, P, None),           # out == a, but a is a transposed view
        (sma.SCAN_SUM, f32, P, [4, 4], [8, 2], 1, P + 8, None),       # out inside the span of a stepped a
        (sma.SCAN_SUM, f32, P, [16], [1], 0, P + 4, None),            # out overlapping a dense a without being a
        (sma.SCAN_SUM, f32, P + 4, [16], [1], 0, P, None),
    ]
    for kind, dtype, a, shape, strides, axis, out, ndim in bad:
        assert lib.scan_raw(kind, dtype, a, shape, strides, axis, out, ndim=ndim) == sma.ERR_INVALID, (kind, dtype, shape, strides, axis)
    for kind in range(4):  # the plan applies the same checks
        with pytest.raises(sma.SmhipError) as e:
            lib.scan_plan(kind, np.float32, [4, 4], [4, 1], 2)
        assert e.value.code == sma.ERR_INVALID
    # an extent of 0 is a no-op, whatever the pointers
    assert lib.scan_raw(sma.SCAN_MAX, f32, 0, [3, 0], [0, 1], 0, 0) == 0


def test_python_out_argument_is_checked(lib):
    class Fake:  # stands in for a DeviceArray: the check fires before anything is allocated or launched
        def __init__(self, dtype, shape, is_dense=True):
            self.dtype, self.shape, self.ndim, self.strides = np.dtype(dtype), shape, len(shape), tuple(dense(shape))
            self.size = int(np.prod(shape))
            self.is_dense = lambda: is_dense

    a = Fake(np.float32, (4, 5))
    for out in (Fake(np.float64, (4, 5)), Fake(np.float32, (5,)), Fake(np.float32, (4, 5), is_dense=False)):
        with pytest.raises(ValueError):
            lib.scan("cumsum", a, 1, out=out)
    with pytest.raises(ValueError):
        lib.scan("cumsum", a, 2)
    with pytest.raises(KeyError):
        lib.scan("cummean", a, 1)


def test_plan_canonical_form(lib):
    shape = (3, 5, 4097)
    assert plan(lib, shape, 0)[3] == (1, 3, 20485)
    assert plan(lib, shape, 1)[3] == (3, 5, 4097)
    assert plan(lib, shape, 2)[3] == (15, 4097, 1)
    assert plan(lib, shape, 0)[0] == sma.SCAN_ROUTE_COLUMN and plan(lib, shape, 1)[0] == sma.SCAN_ROUTE_COLUMN
    assert plan(lib, shape, 2)[0] == sma.SCAN_ROUTE_ROW
    # size-1 axes are dropped: the same walk with and without them
    assert plan(lib, (7, 1, 9), 2) == plan(lib, (7, 9), 1)
    assert plan(lib, (1, 7, 1, 9, 1), 1) == plan(lib, (7, 9), 0)
    assert plan(lib, (7, 1, 9), 0, strides=(9, 12345, 1)) == plan(lib, (7, 9), 0)  # whatever stride a size-1 axis carries


def test_plan_degenerate_shapes(lib):
    assert plan(lib, (3, 1, 4), 1)[:3] == (sma.SCAN_ROUTE_COPYONLY, 0, 1)
    assert plan(lib, (1,), 0)[:3] == (sma.SCAN_ROUTE_COPYONLY, 0, 1)
    for axis in (0, 1, 2):
        assert plan(lib, (3, 0, 4), axis)[:3] == (sma.SCAN_ROUTE_NONE, 0, 0)


def test_plan_views_are_copied_dense_first(lib):
    twin = plan(lib, (100, 50), 1)
    t = plan(lib, (100, 50), 1, strides=(1, 100))   # a transposed view
    s = plan(lib, (100, 50), 1, strides=(100, 2))   # a stepped view
    for v in (t, s):
        assert v[1] & sma.SCAN_COPY and not twin[1] & sma.SCAN_COPY
        assert v[0] == twin[0] and v[3] == twin[3] and v[2] == twin[2] + 1
    assert plan(lib, (8, 5), 0, strides=(0, 1))[1] & sma.SCAN_COPY          # a broadcast (stride 0) axis
    assert plan(lib, (8, 5), 0, strides=(16, 1))[1] & sma.SCAN_COPY         # a sub-block of a wider array
    twin, t = plan(lib, (300, 70001), 1), plan(lib, (300, 70001), 1, strides=(1, 300))  # with the split as well
    assert twin[1] == sma.SCAN_SPLIT and t[1] == sma.SCAN_SPLIT | sma.SCAN_COPY and (twin[2], t[2]) == (2, 3)


def test_plan_split_when_too_few_lanes(lib):
    R = (1 << 18) + 5
    route, flags, launches, ori, chunk = plan(lib, (1, R), 1)
    assert (route, flags, launches, ori) == (sma.SCAN_ROUTE_ROW, sma.SCAN_SPLIT, 2, (1, R, 1)) and 0 < chunk < R
    route, flags, launches, ori, chunk = plan(lib, (70001, 8), 0)
    assert (route, flags, launches, ori) == (sma.SCAN_ROUTE_COLUMN, sma.SCAN_SPLIT, 2, (1, 70001, 8)) and 0 < chunk < 70001
    for axis, route in ((0, sma.SCAN_ROUTE_COLUMN), (1, sma.SCAN_ROUTE_ROW)):
        assert plan(lib, (4096, 4096), axis)[:3] == (route, 0, 1)
        assert plan(lib, (4096, 4096), axis)[4] == 4096  # not split: the chunk is the axis
    # the rate table's split shapes
    assert plan(lib, (4, 1 << 26), 1)[:3] == (sma.SCAN_ROUTE_ROW, sma.SCAN_SPLIT, 2)
    assert plan(lib, (1 << 22, 64), 0)[:3] == (sma.SCAN_ROUTE_COLUMN, sma.SCAN_SPLIT, 2)
    # short rows are never split, however few
    assert plan(lib, (2, 256), 1)[:3] == (sma.SCAN_ROUTE_ROW, 0, 1)


def test_plan_depends_on_shape_and_layout_only(lib):
    for shape, axis in (((4, 1 << 20), 1), ((70001, 8), 0), ((63, 4097), 0)):
        a = lib.scan_plan("cumsum", np.float32, list(shape), dense(shape), axis)
        for kind in ("cumsum", "cumprod", "cummax", "cummin"):
            for _ in range(2):
                assert lib.scan_plan(kind, np.float32, list(shape), dense(shape), axis) == a
        assert lib.scan_plan("cumsum", np.int32, list(shape), dense(shape), axis) == a  # the same vector width
