"""argmax / argmin along an axis, host side: the C ABI's argument checks, the planner (smhip_argreduce_plan) and the Python
binding's own checks -- no device involved."""
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


def plan(lib, shape, axis, strides=None, kind="argmax", dtype=np.float32):
    """(route id, flags, launches, (O, R, I), chunk)"""
    route, launches, ori, chunk = lib.argreduce_plan(kind, dtype, list(shape), dense(shape) if strides is None else list(strides), axis)
    return route & 0xff, route & ~0xff, launches, ori, chunk


def test_entry_points_and_constants_are_declared():
    names = sma.declared_symbols()
    assert "smhip_argreduce_axis" in names and "smhip_argreduce_plan" in names
    assert sma.ARG_KINDS == {"argmax": 0, "argmin": 1} and (sma.ARG_MAX, sma.ARG_MIN) == (0, 1)
    assert (sma.ARG_ROUTE_NONE, sma.ARG_ROUTE_ROW, sma.ARG_ROUTE_COLUMN) == (0, 1, 2)
    assert (sma.ARG_SPLIT, sma.ARG_COPY) == (0x100, 0x200)
    with open(sma.HEADER) as f:
        text = f.read()
    for name, value in (("SMHIP_ARG_ROUTE_NONE", "0"), ("SMHIP_ARG_ROUTE_ROW", "1"), ("SMHIP_ARG_ROUTE_COLUMN", "2"),
                        ("SMHIP_ARG_SPLIT", "0x100"), ("SMHIP_ARG_COPY", "0x200")):
        assert f"#define {name} {value}" in " ".join(text.split())
    assert "SMHIP_ARG_MAX = 0, SMHIP_ARG_MIN = 1" in text


def test_exports_still_match_the_header(lib):
    for name in ("smhip_argreduce_axis", "smhip_argreduce_plan"):
        assert hasattr(lib.c, name)


def test_argument_validation_needs_no_gpu(lib):
    f32, MAX = sma.F32, sma.ARG_MAX
    P, Q = 4096, 1 << 20  # stand in for device pointers: every call below is rejected before anything is dereferenced or launched
    bad = [
        # kind, dtype, a, shape, strides, axis, index_out, value_out, ndim
        (2, f32, P, [4], [1], 0, Q, 0, None),                       # kind
        (-1, f32, P, [4], [1], 0, Q, 0, None),
        (MAX, sma.I8, P, [4], [1], 0, Q, 0, None),                  # dtype
        (MAX, f32, P, [], [], 0, Q, 0, 0),                          # ndim 0
        (MAX, f32, P, [2] * 7, dense([2] * 7), 0, Q, 0, None),      # ndim 7
        (MAX, f32, P, [4, 4], [4, 1], -1, Q, 0, None),              # axis -1 (the C ABI does not count from the end)
        (MAX, f32, P, [4, 4], [4, 1], 2, Q, 0, None),               # axis == ndim
        (MAX, f32, P, [4, -1], [4, 1], 0, Q, 0, None),              # negative extent
        (MAX, f32, P, [4, 4], [4, -1], 0, Q, 0, None),              # negative stride
        (MAX, f32, 0, [4], [1], 0, Q, 0, None),                     # null a
        (MAX, f32, P, None, [1], 0, Q, 0, 1),                       # null shape
        (MAX, f32, P, [4], None, 0, Q, 0, 1),                       # null strides
        (MAX, f32, P, [4], [1], 0, 0, 0, None),                     # null index_out
        (MAX, f32, P, [4], [1], 0, 0, Q, None),                     # ... even with a value_out
        (MAX, f32, P, [16], [1], 0, P + 4, 0, None),                # index_out inside a
        (MAX, f32, P + 4, [16], [1], 0, P, 0, None),                # a inside index_out's 8 bytes
        (MAX, f32, P, [4, 4], [8, 2], 1, P + 40, 0, None),          # index_out inside the span of a stepped a
        (MAX, f32, P, [4, 4], [4, 1], 1, Q, P + 60, None),          # value_out overlapping a's last element
        (MAX, f32, P, [4, 4], [4, 1], 1, Q, Q + 24, None),          # value_out inside index_out (4 x 8 bytes)
        (MAX, f32, P, [4, 4], [4, 1], 1, Q + 8, Q, None),           # index_out inside value_out (4 x 4 bytes)
        (MAX, f32, P, [3, 0], [0, 1], 1, Q, 0, None),               # an empty axis with a result to write (numpy raises)
        (sma.ARG_MIN, f32, P, [0], [1], 0, Q, 0, None),
    ]
    for kind, dtype, a, shape, strides, axis, idx, val, ndim in bad:
        assert lib.argreduce_raw(kind, dtype, a, shape, strides, axis, idx, val, ndim=ndim) == sma.ERR_INVALID, (kind, dtype, shape, strides, axis)
    # the plan applies the same checks
    for kind in (0, 1):
        for shape, strides, axis in (([4, 4], [4, 1], 2), ([4, 4], [4, 1], -1), ([3, 0], [0, 1], 1), ([4, -4], [4, 1], 0)):
            with pytest.raises(sma.SmhipError) as e:
                lib.argreduce_plan(kind, np.float32, shape, strides, axis)
            assert e.value.code == sma.ERR_INVALID
    with pytest.raises(sma.SmhipError):
        lib.argreduce_plan(2, np.float32, [4], [1], 0)
    # any other extent of 0 is a no-op, whatever the pointers
    assert lib.argreduce_raw(MAX, f32, 0, [3, 0], [0, 1], 0, 0, 0) == 0
    assert lib.argreduce_raw(MAX, f32, 0, [0, 3], [3, 1], 1, 0, 0) == 0
    assert lib.argreduce_raw(sma.ARG_MIN, f32, 0, [0, 0], [0, 1], 1, 0, 0) == 0


def test_python_side_checks(lib):
    class Fake:  # stands in for a DeviceArray: the checks fire before anything is allocated or launched
        def __init__(self, dtype, shape, is_dense=True):
            self.dtype, self.shape, self.ndim, self.strides = np.dtype(dtype), shape, len(shape), tuple(dense(shape))
            self.size = int(np.prod(shape))
            self.is_dense = lambda: is_dense

    a = Fake(np.float32, (4, 5))
    for out in (Fake(np.int32, (4,)), Fake(np.float32, (4,)), Fake(np.int64, (5,)), Fake(np.int64, (4,), is_dense=False)):
        with pytest.raises(ValueError):
            lib.argreduce("argmax", a, 1, out=out)
    with pytest.raises(ValueError):
        lib.argreduce("argmax", a, 0, keepdims=True, out=Fake(np.int64, (4,)))  # the result has 5 elements
    for axis in (2, -3):
        with pytest.raises(ValueError):
            lib.argreduce("argmin", a, axis)
    with pytest.raises(KeyError):
        lib.argreduce("argmean", a, 1)
    with pytest.raises(ValueError):
        lib.argreduce("argmax", Fake(np.float16, (4, 5)), 1)


def test_plan_routes(lib):
    R, C, S, Y = sma.ARG_ROUTE_ROW, sma.ARG_ROUTE_COLUMN, sma.ARG_SPLIT, sma.ARG_COPY
    # rows: 65 of 4097 elements are too few lanes, so the rows are cut into 5 chunks of 1024 and finished by one launch
    assert plan(lib, (65, 4097), 1) == (R, S, 2, (65, 4097, 1), 1024)
    # ... and the transposed view over axis 0 is the same walk, with no copy
    assert plan(lib, (4097, 65), 0, strides=(1, 4097)) == plan(lib, (65, 4097), 1)
    assert plan(lib, (4096, 4096), 1) == (R, 0, 1, (4096, 4096, 1), 4096)
    assert plan(lib, (1000, 50), 1) == (R, 0, 1, (1000, 50, 1), 50)  # short rows: never split
    assert plan(lib, (2, 256), 1)[:3] == (R, 0, 1)
    # columns: axis 0 of a dense 2-D array
    assert plan(lib, (64, 1 << 20), 0) == (C, 0, 1, (1, 64, 1 << 20), 64)
    assert plan(lib, (1000, 257), 0)[:4] == (C, S, 2, (1, 1000, 257))
    assert plan(lib, (1 << 20, 64), 1, strides=(1, 1 << 20)) == plan(lib, (64, 1 << 20), 0)  # the transposed twin
    # the split routes of the GPU tests
    assert plan(lib, (4, 1 << 22), 1) == (R, S, 2, (4, 1 << 22, 1), 4096)
    # ... 65536 chunks of 16 rows: more than 4096 pairs per result, so two finishing launches
    assert plan(lib, (1 << 20, 4), 0, dtype=np.float64) == (C, S, 3, (1, 1 << 20, 4), 16)
    # the one long row of the GPU tests: 4089 chunks
    assert plan(lib, ((1 << 31) + 5,), 0) == (R, S, 2, (1, (1 << 31) + 5, 1), 525312)
    # rows and columns enough for the machine are still cut where a chunk's positions would leave 32 bits
    assert plan(lib, (1 << 19, 1 << 33), 1) == (R, S, 2, (1 << 19, 1 << 33, 1), 1 << 31)
    assert plan(lib, ((1 << 33) + 1, 1 << 20), 0) == (C, S, 2, (1, (1 << 33) + 1, 1 << 20), 1717986920)


def test_plan_canonical_form(lib):
    shape = (3, 5, 4097)
    assert plan(lib, shape, 0)[3] == (1, 3, 20485)
    assert plan(lib, shape, 1)[3] == (3, 5, 4097)
    assert plan(lib, shape, 2)[3] == (15, 4097, 1)
    assert plan(lib, shape, 0)[0] == sma.ARG_ROUTE_COLUMN and plan(lib, shape, 1)[0] == sma.ARG_ROUTE_COLUMN
    assert plan(lib, shape, 2)[0] == sma.ARG_ROUTE_ROW
    # R is exactly the named axis, never merged with a neighbour
    for shape in ((6, 7, 8), (2, 3, 4, 5)):
        for axis in range(len(shape)):
            assert plan(lib, shape, axis)[3][1] == shape[axis]
    # size-1 axes are dropped: the same walk with and without them
    assert plan(lib, (7, 1, 9), 2) == plan(lib, (7, 9), 1)
    assert plan(lib, (1, 7, 1, 9, 1), 1) == plan(lib, (7, 9), 0)
    assert plan(lib, (7, 1, 9), 0, strides=(9, 12345, 1)) == plan(lib, (7, 9), 0)  # whatever stride a size-1 axis carries
    # a sub-block of a wider array is read in place: its rows and columns keep a unit stride
    assert plan(lib, (8, 5), 1, strides=(16, 1))[:3] == (sma.ARG_ROUTE_ROW, 0, 1)
    assert plan(lib, (8, 5), 0, strides=(16, 1))[:3] == (sma.ARG_ROUTE_COLUMN, 0, 1)


def test_plan_degenerate_shapes(lib):
    # an axis of one element: every position is 0; the ordinary walks do it
    assert plan(lib, (3, 1, 4), 1) == (sma.ARG_ROUTE_COLUMN, 0, 1, (3, 1, 4), 1)
    assert plan(lib, (1,), 0) == (sma.ARG_ROUTE_ROW, 0, 1, (1, 1, 1), 1)
    assert plan(lib, (5, 1), 1, strides=(3, 7))[:3] == (sma.ARG_ROUTE_ROW, sma.ARG_COPY, 2)
    for axis in (0, 2):
        assert plan(lib, (3, 0, 4), axis)[:3] == (sma.ARG_ROUTE_NONE, 0, 0)


def test_plan_views_that_are_copied_dense_first(lib):
    Y = sma.ARG_COPY
    twin = plan(lib, (100, 50), 1)
    s = plan(lib, (100, 50), 1, strides=(100, 2))   # a stepped view: no unit stride in the walk
    assert s[1] & Y and not twin[1] & Y
    assert s[0] == twin[0] and s[3] == twin[3] and s[2] == twin[2] + 1
    assert plan(lib, (8, 5), 0, strides=(0, 1))[1] & Y   # a broadcast (stride 0) axis
    assert plan(lib, (8, 5), 1, strides=(1, 0))[1] & Y
    # a 3-D permutation whose kept axes do not merge to one outer and one inner: (4, 5, 6).transpose(1, 0, 2) over its last axis
    p = plan(lib, (5, 4, 6), 2, strides=(6, 30, 1))
    assert p[1] & Y and p[0] == sma.ARG_ROUTE_ROW and p[3] == (20, 6, 1) and p[2] == 2
    # ... while over its middle axis the two kept axes are one run of memory and of the result: R [kept], read in place
    q = plan(lib, (5, 4, 6), 1, strides=(6, 30, 1))
    assert not q[1] & Y and q[0] == sma.ARG_ROUTE_COLUMN and q[3] == (1, 4, 30)
    # with the split as well
    twin, t = plan(lib, (3, 70001), 1), plan(lib, (3, 70001), 1, strides=(140002, 2))
    assert twin[1] == sma.ARG_SPLIT and t[1] == sma.ARG_SPLIT | Y and (twin[2], t[2]) == (2, 3)


def test_plan_depends_on_shape_and_layout_only(lib):
    for shape, axis in (((4, 1 << 20), 1), ((70001, 8), 0), ((63, 4097), 0)):
        a = lib.argreduce_plan("argmax", np.float32, list(shape), dense(shape), axis)
        for kind in ("argmax", "argmin"):
            for _ in range(2):
                assert lib.argreduce_plan(kind, np.float32, list(shape), dense(shape), axis) == a
        assert lib.argreduce_plan("argmax", np.int32, list(shape), dense(shape), axis) == a  # the same vector width
