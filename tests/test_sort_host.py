"""sort / argsort along an axis, host side: the C ABI's argument checks, the planner (smhip_sort_plan) and the Python binding's
own checks -- no device involved."""
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


def plan(lib, shape, axis, strides=None, dtype=np.float32, descending=False):
    """(route id, flags, launches, (O, R, I), chunk)"""
    route, launches, ori, chunk = lib.sort_plan(dtype, list(shape), dense(shape) if strides is None else list(strides), axis, descending)
    return route & 0xff, route & ~0xff, launches, ori, chunk


def tile(lib, dtype=np.float32):
    """K: what the plan reports for a line longer than any tile."""
    return plan(lib, (1 << 20,), 0, dtype=dtype)[4]


def test_entry_points_and_constants_are_declared():
    names = sma.declared_symbols()
    assert "smhip_sort_axis" in names and "smhip_sort_plan" in names
    assert (sma.SORT_ASCENDING, sma.SORT_DESCENDING) == (0, 1)
    assert (sma.SORT_ROUTE_NONE, sma.SORT_ROUTE_COPYONLY, sma.SORT_ROUTE_ROW) == (0, 1, 2)
    assert (sma.SORT_MERGE, sma.SORT_COPY) == (0x100, 0x200)
    with open(sma.HEADER) as f:
        text = f.read()
    for name, value in (("SMHIP_SORT_ROUTE_NONE", "0"), ("SMHIP_SORT_ROUTE_COPYONLY", "1"), ("SMHIP_SORT_ROUTE_ROW", "2"),
                        ("SMHIP_SORT_MERGE", "0x100"), ("SMHIP_SORT_COPY", "0x200")):
        assert f"#define {name} {value}" in " ".join(text.split())
    assert "SMHIP_SORT_ASCENDING = 0, SMHIP_SORT_DESCENDING = 1" in text


def test_exports_match_the_header(lib):
    for name in ("smhip_sort_axis", "smhip_sort_plan"):
        assert hasattr(lib.c, name)


def test_argument_validation_needs_no_gpu(lib):
    f32, ASC = sma.F32, sma.SORT_ASCENDING
    P, Q, S = 4096, 1 << 20, 1 << 21  # stand in for device pointers: every call below is rejected before anything is dereferenced or launched
    bad = [
        # order, dtype, a, shape, strides, axis, values_out, index_out, ndim
        (2, f32, P, [4], [1], 0, Q, S, None),                        # order
        (-1, f32, P, [4], [1], 0, Q, S, None),
        (ASC, sma.I8, P, [4], [1], 0, Q, S, None),                   # dtype
        (ASC, -1, P, [4], [1], 0, Q, S, None),
        (ASC, f32, P, [], [], 0, Q, S, 0),                           # ndim 0
        (ASC, f32, P, [2] * 7, dense([2] * 7), 0, Q, S, None),       # ndim 7
        (ASC, f32, P, [4, 4], [4, 1], -1, Q, S, None),               # axis -1 (the C ABI does not count from the end)
        (ASC, f32, P, [4, 4], [4, 1], 2, Q, S, None),                # axis == ndim
        (ASC, f32, P, [4, -1], [4, 1], 0, Q, S, None),               # negative extent
        (ASC, f32, P, [4, 4], [4, -1], 0, Q, S, None),               # negative stride
        (ASC, f32, 0, [4], [1], 0, Q, S, None),                      # null a
        (ASC, f32, P, None, [1], 0, Q, S, 1),                        # null shape
        (ASC, f32, P, [4], None, 0, Q, S, 1),                        # null strides
        (ASC, f32, P, [4], [1], 0, 0, 0, None),                      # both outputs null
        (1, sma.I64, P, [4, 4], [4, 1], 1, 0, 0, None),
        (ASC, f32, P, [16], [1], 0, P + 4, 0, None),                 # values_out inside a, not a itself
        (ASC, f32, P + 4, [16], [1], 0, P, 0, None),                 # a inside values_out
        (ASC, f32, P, [16], [1], 0, 0, P + 8, None),                 # index_out inside a
        (ASC, f32, P, [16], [1], 0, 0, P, None),                     # index_out == a: in place is for the values only
        (ASC, f32, P, [4, 4], [8, 2], 1, 0, P + 40, None),           # index_out inside the span of a stepped a
        (ASC, f32, P, [4, 4], [8, 2], 1, P, 0, None),                # values_out == a, but a is a stepped view
        (ASC, f32, P, [4, 4], [1, 4], 1, P, 0, None),                # ... a transposed view
        (ASC, f32, P, [4, 4], [0, 1], 1, P, 0, None),                # ... a broadcast view
        (ASC, f32, P, [4, 4], [4, 1], 1, Q, Q + 60, None),           # index_out overlapping values_out's last element
        (ASC, f32, P, [4, 4], [4, 1], 1, Q + 64, Q, None),           # values_out inside index_out (16 x 8 bytes)
        (ASC, f32, P, [4, 4], [4, 1], 1, P, P + 32, None),           # in place, but index_out inside a
    ]
    for order, dtype, a, shape, strides, axis, val, idx, ndim in bad:
        assert lib.sort_raw(order, dtype, a, shape, strides, axis, val, idx, ndim=ndim) == sma.ERR_INVALID, (order, dtype, shape, strides, axis, val, idx)
    # an axis whose positions do not fit 32 bits
    for n in (1 << 31, (1 << 31) + 5, 1 << 40):
        assert lib.sort_raw(ASC, f32, P, [n], [1], 0, 1 << 50, 0) == sma.ERR_UNSUPPORTED
        assert lib.sort_raw(1, sma.F64, P, [2, n], [0, 1], 1, 0, 1 << 50) == sma.ERR_UNSUPPORTED
        with pytest.raises(sma.SmhipError) as e:
            lib.sort_plan(np.float32, [n], [1], 0)
        assert e.value.code == sma.ERR_UNSUPPORTED
    # the plan applies the same checks
    for shape, strides, axis in (([4, 4], [4, 1], 2), ([4, 4], [4, 1], -1), ([4, -4], [4, 1], 0), ([4, 4], [-4, 1], 0)):
        with pytest.raises(sma.SmhipError) as e:
            lib.sort_plan(np.float32, shape, strides, axis)
        assert e.value.code == sma.ERR_INVALID
    with pytest.raises(sma.SmhipError):
        lib.sort_plan(7, [4], [1], 0)
    # any extent of 0, the axis included, is a no-op, whatever the pointers
    assert lib.sort_raw(ASC, f32, 0, [3, 0], [0, 1], 0, 0, 0) == 0
    assert lib.sort_raw(ASC, f32, 0, [3, 0], [0, 1], 1, 0, 0) == 0
    assert lib.sort_raw(1, f32, 0, [0], [1], 0, 0, 0) == 0
    assert lib.sort_raw(1, sma.I32, 0, [0, 3], [3, 1], 1, P, P) == 0


def test_python_side_checks(lib):
    class Fake:  # stands in for a DeviceArray: the checks fire before anything is allocated or launched
        def __init__(self, dtype, shape, is_dense=True):
            self.dtype, self.shape, self.ndim, self.strides = np.dtype(dtype), shape, len(shape), tuple(dense(shape))
            self.size = int(np.prod(shape))
            self.is_dense = lambda: is_dense

    a = Fake(np.float32, (4, 5))
    for out in (Fake(np.int32, (4, 5)), Fake(np.float64, (4, 5)), Fake(np.float32, (4, 4)), Fake(np.float32, (4, 5), is_dense=False)):
        with pytest.raises(ValueError):
            lib.sort(a, 1, out=out)
    for out in (Fake(np.float32, (4, 5)), Fake(np.int32, (4, 5)), Fake(np.int64, (5,)), Fake(np.int64, (4, 5), is_dense=False)):
        with pytest.raises(ValueError):
            lib.argsort(a, 1, out=out)
    view = Fake(np.float32, (4, 5), is_dense=False)
    for axis in (0, None):
        with pytest.raises(ValueError):
            lib.sort(view, axis, out=view)  # in place needs a dense array
    for axis in (2, -3):  # negative axes count from the end, as far as they go
        with pytest.raises(ValueError):
            lib.sort(a, axis)
        with pytest.raises(ValueError):
            lib.argsort(a, axis)
    for dtype in (np.float16, np.uint32, np.int8):
        with pytest.raises(ValueError):
            lib.sort(Fake(dtype, (4, 5)), 1)


def test_python_wrapper_axis_and_shapes(lib, monkeypatch):
    """Axis normalisation and the axis=None form, seen through the arguments the wrapper hands to the C ABI."""
    calls = []

    class FakeC:
        @staticmethod
        def smhip_sort_axis(order, dtype, a, shape, strides, ndim, axis, vals, idx):
            calls.append((order.value, dtype.value, list(shape)[:ndim.value], list(strides)[:ndim.value], axis.value, bool(vals.value), bool(idx.value)))
            return 0

    class Arr:
        def __init__(self, dtype, shape):
            self.dtype, self.shape, self.ndim, self.strides = np.dtype(dtype), tuple(shape), len(shape), tuple(dense(shape))
            self.size, self.ptr = int(np.prod(shape)), 4096
            self.is_dense = lambda: True

    monkeypatch.setattr(lib, "c", FakeC)
    monkeypatch.setattr(lib, "empty", lambda shape, dtype: Arr(dtype, shape))
    a = Arr(np.float64, (3, 4, 5))
    assert lib.sort(a).shape == (3, 4, 5)
    assert calls[-1] == (0, sma.F64, [3, 4, 5], [20, 5, 1], 2, True, False)  # the last axis by default
    idx = lib.argsort(a, -3, descending=True)
    assert idx.shape == (3, 4, 5) and idx.dtype == np.int64
    assert calls[-1] == (1, sma.F64, [3, 4, 5], [20, 5, 1], 0, False, True)
    vals, idx = lib.sort(a, 1, indices=True)
    assert calls[-1][4:] == (1, True, True) and vals.dtype == np.float64 and idx.dtype == np.int64
    flat = lib.sort(a, axis=None)
    assert flat.shape == (60,) and calls[-1][2:5] == ([60], [1], 0)
    assert lib.argsort(a, axis=None).shape == (60,)
    assert lib.sort(a, out=a) is a  # in place


def test_plan_routes(lib):
    ROW, M, Y = sma.SORT_ROUTE_ROW, sma.SORT_MERGE, sma.SORT_COPY
    for dtype in (np.float32, np.float64, np.int32, np.int64):
        K = tile(lib, dtype)
        assert K >= 256 and K & (K - 1) == 0
        assert plan(lib, (3, 0, 4), 1, dtype=dtype) == (sma.SORT_ROUTE_NONE, 0, 0, (3, 0, 4), 0)
        assert plan(lib, (0, 5), 1, dtype=dtype)[:3] == (sma.SORT_ROUTE_NONE, 0, 0)
        assert plan(lib, (3, 1, 4), 1, dtype=dtype) == (sma.SORT_ROUTE_COPYONLY, 0, 2, (3, 1, 4), 1)
        assert plan(lib, (1,), 0, dtype=dtype)[:3] == (sma.SORT_ROUTE_COPYONLY, 0, 2)
        for R in (2, 3, 64, 1000, K - 1, K):
            assert plan(lib, (7, R), 1, dtype=dtype) == (ROW, 0, 1, (7, R, 1), R)
        # one element more than a tile: two tiles and one merge pass
        assert plan(lib, (7, K + 1), 1, dtype=dtype) == (ROW, M, 2, (7, K + 1, 1), K)
        # a launch more for every doubling of the tiles; an odd run is no special case
        for tiles, passes in ((2, 1), (3, 2), (4, 2), (5, 3), (6, 3), (8, 3), (9, 4), (16, 4), (17, 5), (4096, 12)):
            for R in (tiles * K, (tiles - 1) * K + 1):
                assert plan(lib, (2, R), 1, dtype=dtype) == (ROW, M, 1 + passes, (2, R, 1), K), (tiles, R)
        assert plan(lib, (5 * K + 17,), 0, dtype=dtype) == (ROW, M, 4, (1, 5 * K + 17, 1), K)
        assert plan(lib, ((1 << 31) - 1,), 0, dtype=dtype)[:2] == (ROW, M)
    # the order does not enter the plan
    for shape, axis in (((100, 50), 0), ((3, 9000), 1)):
        assert plan(lib, shape, axis) == plan(lib, shape, axis, descending=True)


def test_plan_layouts(lib):
    ROW, M, Y = sma.SORT_ROUTE_ROW, sma.SORT_MERGE, sma.SORT_COPY
    K = tile(lib)
    # dense, the last axis: read and written in place; the axes before it are one run of lines
    assert plan(lib, (3, 5, 70), 2) == (ROW, 0, 1, (15, 70, 1), 70)
    assert plan(lib, (7, 1, 9), 2) == (ROW, 0, 1, (7, 9, 1), 9)  # size-1 axes are dropped, whatever stride they carry
    assert plan(lib, (7, 1, 9), 2, strides=(9, 12345, 1)) == plan(lib, (7, 1, 9), 2)
    assert plan(lib, (70, 1, 1), 0) == (ROW, 0, 1, (1, 70, 1), 70)
    # a sub-block of a wider array: its rows keep the unit stride, the results are dense
    assert plan(lib, (8, 5), 1, strides=(16, 1)) == (ROW, 0, 1, (8, 5, 1), 5)
    # an axis that is not the last: staged in (1 launch) and both results scattered back (2)
    assert plan(lib, (100, 50), 0) == (ROW, Y, 4, (1, 100, 50), 100)
    assert plan(lib, (3, 5, 70), 1) == (ROW, Y, 4, (3, 5, 70), 5)
    assert plan(lib, (3, 5, 70), 0) == (ROW, Y, 4, (1, 3, 350), 3)
    # a transposed 2-D view along the axis that has the unit stride in memory: no input staging, the results are still scattered
    assert plan(lib, (50, 100), 0, strides=(1, 50)) == (ROW, Y, 3, (100, 50, 1), 50)
    # ... and along the other one the operand is staged into rows, which are the dense result as they stand
    assert plan(lib, (50, 100), 1, strides=(1, 50)) == (ROW, Y, 2, (50, 100, 1), 100)
    # a stepped view, a stride-0 sort axis, a stride-0 kept axis: staged in; rows in index order come out dense
    assert plan(lib, (100, 50), 1, strides=(300, 3)) == (ROW, Y, 2, (100, 50, 1), 50)
    assert plan(lib, (8, 50), 1, strides=(1, 0)) == (ROW, Y, 2, (8, 50, 1), 50)
    assert plan(lib, (8, 50), 1, strides=(0, 1)) == (ROW, Y, 2, (8, 50, 1), 50)
    assert plan(lib, (8, 50), 0, strides=(0, 1)) == (ROW, Y, 4, (1, 8, 50), 8)
    # kept axes that do not merge: (4, 5, 6).transpose(1, 0, 2) over its last axis
    assert plan(lib, (5, 4, 6), 2, strides=(6, 30, 1)) == (ROW, Y, 2, (20, 6, 1), 6)
    # with the merge as well
    assert plan(lib, (3, 2 * K + 1), 1, strides=(6 * K + 3, 3)) == (ROW, M | Y, 4, (3, 2 * K + 1, 1), K)
    assert plan(lib, (2 * K + 1, 3), 0) == (ROW, M | Y, 6, (1, 2 * K + 1, 3), K)
    # O * R * I is the element count, R the named axis, chunk = min(R, K)
    for shape in ((6, 7, 8), (2, 3, 4, 5), (3, K + 5, 2)):
        for axis in range(len(shape)):
            _, _, _, ori, chunk = plan(lib, shape, axis)
            assert ori[1] == shape[axis] and ori[0] * ori[1] * ori[2] == int(np.prod(shape)) and chunk == min(shape[axis], K)
