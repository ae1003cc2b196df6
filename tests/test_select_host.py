"""where / count_nonzero / flatnonzero / nonzero / select, host side: the C ABI's argument checks, the planner (smhip_select_plan) and the
Python binding's own checks -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma

NONE, ONE, TILES, DENSE, COPY = sma.SELECT_ROUTE_NONE, sma.SELECT_ROUTE_ONE, sma.SELECT_ROUTE_TILES, sma.SELECT_ROUTE_DENSE, sma.SELECT_COPY
ENTRY_POINTS = ("smhip_where", "smhip_select_count", "smhip_select", "smhip_select_plan")
DTYPES = (np.float32, np.float64, np.int32, np.int64)
COMPACTING = ("index", "coords", "values")


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def dense(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.insert(0, acc)
        acc *= d
    return st


def plan(lib, what, dtype, shape, x=None, **kw):
    """(route id, flags, launches, info)"""
    route, launches, info = lib.select_plan(what, dtype, shape, dense(shape) if x is None else x, **kw)
    return route & 0xff, route & ~0xff, launches, info


def test_entry_points_and_constants_are_declared():
    names = sma.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in names
    assert (sma.CMP_NONZERO, sma.CMP_EQ, sma.CMP_NE, sma.CMP_LT, sma.CMP_LE, sma.CMP_GT, sma.CMP_GE) == tuple(range(7))
    assert (sma.SELECT_INDEX, sma.SELECT_COORDS, sma.SELECT_VALUES, sma.SELECT_COUNT, sma.SELECT_WHERE) == tuple(range(5))
    assert (NONE, ONE, TILES, DENSE, COPY) == (0, 1, 2, 3, 0x100)
    with open(sma.HEADER) as f:
        text = f.read()
    flat = " ".join(text.split())
    for name, value in (("SMHIP_SELECT_ROUTE_NONE", "0"), ("SMHIP_SELECT_ROUTE_ONE", "1"), ("SMHIP_SELECT_ROUTE_TILES", "2"), ("SMHIP_SELECT_ROUTE_DENSE", "3"),
                        ("SMHIP_SELECT_COPY", "0x100")):
        assert f"#define {name} {value}" in flat
    assert "SMHIP_CMP_NONZERO = 0, SMHIP_CMP_EQ = 1, SMHIP_CMP_NE = 2, SMHIP_CMP_LT = 3, SMHIP_CMP_LE = 4, SMHIP_CMP_GT = 5, SMHIP_CMP_GE = 6" in flat
    assert "SMHIP_SELECT_INDEX = 0, SMHIP_SELECT_COORDS = 1, SMHIP_SELECT_VALUES = 2, SMHIP_SELECT_COUNT = 3, SMHIP_SELECT_WHERE = 4" in flat


def test_exports_match_the_header(lib):
    for name in ENTRY_POINTS:
        assert hasattr(lib.c, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_planner_routes_by_size(lib, dtype):
    _, _, _, (_, tile, threshold, _) = plan(lib, "index", dtype, [1000])
    assert tile == 256 * 8 * (16 // np.dtype(dtype).itemsize) and threshold >= tile and threshold % tile == 0
    tiles_of = lambda n: -(-n // tile)  # noqa: E731
    for what in COMPACTING + ("count",):
        three = 2 if what == "count" else 3
        assert plan(lib, what, dtype, [0])[:3] == (NONE, 0, 0)
        assert plan(lib, what, dtype, [4, 0, 3])[:3] == (NONE, 0, 0)
        for n in (1, tile - 1, tile, tile + 1, threshold):
            route, flags, launches, info = plan(lib, what, dtype, [n])
            assert (route, flags, launches, info[0]) == (ONE, 0, 1, tiles_of(n)), (what, n)
        for n in (threshold + 1, 70001 + threshold, 129 * tile + 5):
            route, flags, launches, info = plan(lib, what, dtype, [n])
            assert (route, flags, launches, info[0]) == (TILES, 0, three, tiles_of(n)), (what, n)
        # 2^33 elements: the tiles and every offset are still right in int64
        route, flags, launches, info = plan(lib, what, dtype, [1 << 33])
        assert (route, flags, launches, info[0]) == (TILES, 0, three, (1 << 33) // tile)
        assert plan(lib, what, dtype, [1 << 11, 1 << 11, 1 << 11])[3][0] == (1 << 33) // tile
        # the last element alone in its tile
        assert plan(lib, what, dtype, [(1 << 33) + 1])[3][0] == (1 << 33) // tile + 1


def test_planner_where(lib):
    for dtype in DTYPES:
        W = 16 // np.dtype(dtype).itemsize
        assert plan(lib, "where", dtype, [0])[:3] == (NONE, 0, 0)
        for n in (1, 5, 70001, 1 << 24):
            assert plan(lib, "where", dtype, [n])[:3] == (DENSE, 0, 1)
        # large operands go out in pieces, one launch each; the tail rides with the last piece
        assert plan(lib, "where", dtype, [(W << 24) + 1], a_strides=[1], b_strides=[1])[:3] == (DENSE, 0, 1)
        assert plan(lib, "where", dtype, [(W << 26)], y_strides=[1], a_strides=[1], b_strides=[1])[2] >= 2
        assert plan(lib, "where", dtype, [(W << 28) + 3])[2] >= 2
    # each operand that is not dense row-major is copied first, one launch each
    shape, t = [300, 70], [1, 300]
    assert plan(lib, "where", np.float32, shape, x=t)[:3] == (DENSE, COPY, 2)
    assert plan(lib, "where", np.float32, shape, y_strides=t)[:3] == (DENSE, COPY, 2)
    assert plan(lib, "where", np.float32, shape, a_strides=[0, 1], b_strides=[1, 0])[:3] == (DENSE, COPY, 3)     # row and column broadcast
    route, flags, launches, info = plan(lib, "where", np.float32, shape, x=t, y_strides=[140, 2], a_strides=[0, 0], b_strides=t)
    assert (route, flags, launches, info[3]) == (DENSE, COPY, 5, 4)
    assert plan(lib, "where", np.float32, shape, y_strides=dense(shape), a_strides=dense(shape), b_strides=dense(shape))[:3] == (DENSE, 0, 1)


def test_planner_copy_flag(lib):
    shape = [300, 70]
    n_launch = {"index": 3, "coords": 3, "values": 3, "count": 2}
    for what, three in n_launch.items():
        for strides in ([1, 300], [140, 2], [0, 1]):   # transposed, stepped, broadcast
            route, flags, launches, info = plan(lib, what, np.float64, shape, x=strides)
            assert (route, flags, launches, info[3]) == (TILES, COPY, three + 1, 1), (what, strides)
            route, flags, launches, info = plan(lib, what, np.float64, shape, y_strides=strides)
            assert (route, flags, launches, info[3]) == (TILES, COPY, three + 1, 1), (what, strides)
        assert plan(lib, what, np.float64, shape, x=[1, 300], y_strides=[0, 1])[1:3] == (COPY, three + 2)
        assert plan(lib, what, np.float64, shape, y_strides=dense(shape))[1:3] == (0, three)
    # src is an operand of VALUES alone
    assert plan(lib, "values", np.float64, shape, a_strides=[1, 300])[1:3] == (COPY, 4)
    assert plan(lib, "index", np.float64, shape, a_strides=[1, 300])[1:3] == (0, 3)
    assert plan(lib, "values", np.float32, [30, 7], a_strides=[1, 30])[:3] == (ONE, COPY, 2)
    # an extent of 1 may have any stride
    assert plan(lib, "index", np.float32, [1, 500], x=[12345, 1])[1] == 0


def test_argument_validation_needs_no_gpu(lib):
    f32, i64 = sma.F32, sma.I64
    GT, NZ = sma.CMP_GT, sma.CMP_NONZERO
    # stand in for device pointers: every call below is rejected before anything is dereferenced or launched
    X, Y, A, B, O, CNT = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25
    INV = sma.ERR_INVALID
    one = np.ones(1, np.float32)

    def msg():
        return lib.c.smhip_last_error().decode()

    # ---- select_count
    def count(cmp=GT, dtype=f32, x=X, xs=(1,), y=0, ys=None, rhs=one, shape=(8,), cnt=CNT, **kw):
        return lib.select_count_raw(cmp, dtype, x, xs, y, ys, rhs, shape, cnt, **kw)

    assert count(cmp=7) == INV and "comparison" in msg()
    assert count(cmp=-1) == INV
    assert count(dtype=9) == INV and "dtype" in msg()
    assert count(dtype=-1) == INV
    assert count(xs=[1] * 7, shape=[2] * 7) == INV and "ndim" in msg()
    assert count(xs=[], shape=[], ndim=0) == INV
    assert count(shape=[-8]) == INV and "negative" in msg()
    assert count(xs=[-1]) == INV and "negative" in msg()
    assert count(y=Y, ys=[-1]) == INV and "negative" in msg()
    assert count(shape=None, ndim=1) == INV and "null" in msg()
    assert count(xs=None, ndim=1) == INV and "null" in msg()
    assert count(y=Y, ys=None) == INV and "null" in msg()
    assert count(x=0) == INV and "null" in msg()
    assert count(cnt=0) == INV and "null" in msg()
    assert count(rhs=None) == INV and "scalar" in msg()
    assert count(cmp=NZ, rhs=None, cnt=X + 8) == INV and "overlaps" in msg()           # NONZERO needs no rhs; the overlap is found next
    assert count(x=X + 2) == INV and "aligned" in msg()
    assert count(y=Y + 1, ys=[1]) == INV and "aligned" in msg()
    assert count(cnt=CNT + 4) == INV and "aligned" in msg()
    assert count(cnt=X + 16) == INV and "overlaps" in msg()
    assert count(y=Y, ys=[1], cnt=Y) == INV and "overlaps" in msg()
    assert count(xs=[1 << 30, 1], shape=[1 << 30, 1 << 30]) == INV and "2^59" in msg()
    assert count(xs=[1 << 58, 1], shape=[4, 4]) == INV and "2^59" in msg()

    # ---- select
    def select(what=0, cmp=GT, dtype=f32, x=X, xs=(1,), y=0, ys=None, rhs=one, shape=(8,), src=0, ss=None, sb=0, out=O, cap=8, cnt=CNT, **kw):
        return lib.select_raw(what, cmp, dtype, x, xs, y, ys, rhs, shape, src, ss, sb, out, cap, cnt, **kw)

    assert select(what=3) == INV and "operation" in msg()
    assert select(what=-1) == INV
    assert select(cmp=9) == INV and "comparison" in msg()
    assert select(dtype=4) == INV and "dtype" in msg()
    assert select(xs=[1] * 7, shape=[2] * 7) == INV and "ndim" in msg()
    assert select(shape=[-1]) == INV and "negative" in msg()
    assert select(xs=[-2]) == INV and "negative" in msg()
    assert select(cap=-1) == INV and "capacity" in msg()
    assert select(cap=1 << 59) == INV and "2^59" in msg()
    assert select(x=0) == INV and "null" in msg()
    assert select(out=0) == INV and "null" in msg()
    assert select(rhs=None) == INV and "scalar" in msg()
    assert select(what=2, src=0, ss=[1], sb=4) == INV and "null" in msg()
    assert select(what=2, src=A, ss=None, sb=4) == INV and "null" in msg()
    assert select(what=2, src=A, ss=[1], sb=2) == INV and "bytes" in msg()
    assert select(what=2, src=A, ss=[-1], sb=4) == INV and "negative" in msg()
    assert select(what=2, src=A + 4, ss=[1], sb=8) == INV and "aligned" in msg()
    assert select(what=2, src=A, ss=[1], sb=8, out=O + 4) == INV and "aligned" in msg()
    assert select(out=O + 4) == INV and "aligned" in msg()                             # int64 items
    assert select(cnt=CNT + 4) == INV and "aligned" in msg()
    assert select(x=X + 1) == INV and "aligned" in msg()
    assert select(out=X + 16) == INV and "overlaps" in msg()                           # out and x
    assert select(y=Y, ys=[1], out=Y - 8) == INV and "overlaps" in msg()               # out and y
    assert select(what=2, src=A, ss=[1], sb=4, out=A + 16) == INV and "overlaps" in msg()   # out and src
    assert select(cnt=X) == INV and "count_dev" in msg()                               # count_dev and x
    assert select(y=Y, ys=[0], cnt=Y) == INV and "count_dev" in msg()                  # ... and a broadcast y of one element
    assert select(what=2, src=A, ss=[1], sb=4, cnt=A + 8) == INV and "count_dev" in msg()
    assert select(cnt=O + 56) == INV and "count_dev" in msg()                          # ... and the last item of out
    assert select(what=1, xs=[3, 1], shape=[2, 3], cap=6, cnt=O + 88) == INV and "count_dev" in msg()   # COORDS: ndim planes
    assert select(xs=[1 << 58, 1], shape=[4, 4]) == INV and "2^59" in msg()
    assert select(shape=[0], x=0, out=0, cnt=0) == 0                                   # nothing to do, whatever the pointers
    assert select(cap=0, out=0, cnt=0) == 0                                            # nothing to write and nothing to count

    # ---- where
    def where(cmp=GT, dtype=f32, x=X, xs=(1,), y=0, ys=None, rhs=one, a=A, as_=(1,), sa=None, b=B, bs=(1,), sb=None, shape=(8,), out=O, **kw):
        return lib.where_raw(cmp, dtype, x, xs, y, ys, rhs, a, as_, sa, b, bs, sb, shape, out, **kw)

    assert where(cmp=7) == INV and "comparison" in msg()
    assert where(dtype=5) == INV and "dtype" in msg()
    assert where(xs=[1] * 7, as_=[1] * 7, bs=[1] * 7, shape=[2] * 7) == INV and "ndim" in msg()
    assert where(shape=[-8]) == INV and "negative" in msg()
    assert where(xs=[-1]) == INV and "negative" in msg()
    assert where(as_=[-1]) == INV and "negative" in msg()
    assert where(bs=[-1]) == INV and "negative" in msg()
    assert where(as_=None) == INV and "null" in msg()
    assert where(shape=None, ndim=1) == INV and "null" in msg()
    assert where(x=0) == INV and "null" in msg()
    assert where(out=0) == INV and "null" in msg()
    assert where(rhs=None) == INV and "scalar" in msg()
    assert where(a=0, as_=None, sa=None) == INV and "scalar" in msg()
    assert where(b=0, bs=None, sb=None) == INV and "scalar" in msg()
    assert where(b=B + 2) == INV and "aligned" in msg()
    assert where(out=O + 1) == INV and "aligned" in msg()
    assert where(xs=[1 << 58, 1], as_=[4, 1], bs=[4, 1], shape=[4, 4]) == INV and "2^59" in msg()
    # every overlap but out == a dense operand: the rule and the wording of smhip_chain
    rule = "only out == an operand that is dense over the result's shape is allowed"
    assert where(out=X + 16) == INV and "overlaps operand x" in msg() and rule in msg()
    assert where(y=Y, ys=[1], out=Y + 4) == INV and "overlaps operand y" in msg() and rule in msg()
    assert where(out=A - 16) == INV and "overlaps operand a" in msg() and rule in msg()
    assert where(out=B + 28) == INV and "overlaps operand b" in msg() and rule in msg()
    assert where(xs=[2], out=X) == INV and "overlaps operand x" in msg()               # the same pointer, but stepped
    assert where(as_=[0], out=A) == INV and "overlaps operand a" in msg()              # ... broadcast
    assert where(xs=[1, 4], as_=[4, 1], bs=[4, 1], shape=[4, 4], out=X) == INV and "overlaps operand x" in msg()   # ... transposed
    assert where(shape=[0], x=0, a=0, b=0, out=0) == 0                                 # nothing to do, whatever the pointers
    # (in place on a dense operand is accepted: tests/test_select_gpu.py runs it)

    # ---- select_plan makes the same checks on what it is given
    with pytest.raises(sma.SmhipError, match="operation"):
        lib.select_plan(5, np.float32, [8], [1])
    with pytest.raises(sma.SmhipError, match="comparison"):
        lib.select_plan("index", np.float32, [8], [1], cmp=7)
    with pytest.raises(sma.SmhipError, match="dtype"):
        lib.select_plan("index", 4, [8], [1])
    with pytest.raises(sma.SmhipError, match="negative"):
        lib.select_plan("index", np.float32, [8], [-1])
    with pytest.raises(sma.SmhipError, match="ndim"):
        lib.select_plan("index", np.float32, [2] * 7, [1] * 7)
    with pytest.raises(sma.SmhipError, match="2\\^59"):
        lib.select_plan("index", np.float32, [1 << 30, 1 << 30], [1 << 30, 1])
    assert i64 == 3


def test_binding_checks(lib):
    def arr(dtype, shape=(8,), strides=None):
        """A DeviceArray that owns nothing: the binding's checks come before anything touches it."""
        return sma.DeviceArray(lib, 1 << 20, dtype, shape, dense(shape) if strides is None else strides, 0, owner=object())

    f, d, i = arr(np.float32), arr(np.float64), arr(np.int32)
    for call in (lib.count_nonzero, lib.flatnonzero, lib.nonzero, lambda c: lib.select(f, c), lambda c: lib.where(c, f, f)):
        with pytest.raises(ValueError, match="condition"):
            call(3.0)
        with pytest.raises(ValueError, match="condition"):
            call((f, "gt"))
        with pytest.raises(ValueError, match="comparison"):
            call((f, "almost", 1.0))
        with pytest.raises(ValueError, match="compares"):
            call((f, "gt", d))
        with pytest.raises(ValueError, match="right-hand side"):
            call((f, "lt", None))
        with pytest.raises(ValueError, match="broadcast"):
            call((f, "lt", arr(np.float32, (7,))))
        with pytest.raises(ValueError, match="dtype"):
            call((arr(np.int16), "lt", 1))
    with pytest.raises(ValueError, match="shape"):
        lib.select(arr(np.float32, (4, 2)), (f, "gt", 0))
    with pytest.raises(ValueError, match="bytes"):
        lib.select(arr(np.int16), (f, "gt", 0))
    with pytest.raises(ValueError, match="a is"):
        lib.where((f, "gt", 0), d, 1.0)
    with pytest.raises(ValueError, match="b is"):
        lib.where((f, "gt", 0), 1.0, i)
    with pytest.raises(ValueError, match="broadcast"):
        lib.where((f, "gt", 0), arr(np.float32, (3,)), 1.0)
    with pytest.raises(ValueError, match="out must"):
        lib.where((f, "gt", 0), 1.0, 0.0, out=d)
    with pytest.raises(ValueError, match="out must"):
        lib.where((f, "gt", 0), 1.0, 0.0, out=arr(np.float32, (8,), [2]))
