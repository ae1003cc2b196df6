"""take / take_along_axis, host side: the C ABI's argument checks, the planner (smhip_take_plan) and the Python binding's own
checks -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma

DTYPES = (np.float32, np.float64, np.int32, np.int64)


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


def along(a_shape, idx_shape, axis, a_strides=None, idx_strides=None):
    """take_along_axis's arguments to the C ABI: (a_strides, R, idx_strides, out_shape), both operands broadcast to the result."""
    a_strides = dense(a_shape) if a_strides is None else list(a_strides)
    idx_strides = dense(idx_shape) if idx_strides is None else list(idx_strides)
    out, sa, si = [], [], []
    for d, (na, ni) in enumerate(zip(a_shape, idx_shape)):
        if d == axis:
            out.append(ni), sa.append(a_strides[d]), si.append(idx_strides[d])
            continue
        assert na == ni or na == 1 or ni == 1
        n = ni if na == 1 else na
        out.append(n), sa.append(a_strides[d] if na == n and n != 1 else 0), si.append(idx_strides[d] if ni == n and n != 1 else 0)
    return sa, a_shape[axis], si, out


def take1d(a_shape, n, axis, a_strides=None, idx_stride=1):
    """np.take(a, ids[n], axis): the index array has stride 0 on every axis but `axis`."""
    a_strides = dense(a_shape) if a_strides is None else list(a_strides)
    out = list(a_shape)
    out[axis] = n
    si = [0] * len(a_shape)
    si[axis] = idx_stride
    return a_strides, a_shape[axis], si, out


def plan(lib, args, axis, dtype=np.float32, mode="clip"):
    """(route id, flags, launches, (O, J, I), K)"""
    sa, R, si, out = args
    route, launches, oji, K = lib.take_plan(dtype, sa, R, si, out, axis, mode)
    return route & 0xff, route & ~0xff, launches, oji, K


def budget(lib, dtype):
    """K: the longest line LINE stages, as the plan reports it."""
    return plan(lib, along((2, 8), (2, 8), 1), 1, dtype)[4]


def least_picks(lib, R, dtype=np.float32):
    """The smallest J at which (7, R) picked along its rows plans LINE (the rule is monotone in J)."""
    lo, hi = 1, R
    assert plan(lib, along((7, R), (7, hi), 1), 1, dtype)[0] == sma.TAKE_ROUTE_LINE
    while lo < hi:
        mid = (lo + hi) // 2
        if plan(lib, along((7, R), (7, mid), 1), 1, dtype)[0] == sma.TAKE_ROUTE_LINE:
            hi = mid
        else:
            lo = mid + 1
    return lo


def ratio(lib, dtype=np.float32):
    """c of `LINE when J >= R / c`, recovered from the plans of a few line lengths."""
    K = budget(lib, dtype)
    lengths = (K, K - 1, 1000, 37)
    least = [least_picks(lib, R, dtype) for R in lengths]
    for c in range(1, K + 1):
        if all(-(-R // c) == j for R, j in zip(lengths, least)):
            return c
    raise AssertionError(f"no c explains the LINE thresholds {dict(zip(lengths, least))}")


def test_entry_points_and_constants_are_declared():
    names = sma.declared_symbols()
    assert "smhip_take_axis" in names and "smhip_take_plan" in names
    assert (sma.INDEX_CHECKED, sma.INDEX_CLIP, sma.INDEX_WRAP) == (0, 1, 2)
    assert (sma.TAKE_ROUTE_NONE, sma.TAKE_ROUTE_LINE, sma.TAKE_ROUTE_ROWS, sma.TAKE_ROUTE_DIRECT) == (0, 1, 2, 3)
    assert sma.TAKE_COPY == 0x100
    with open(sma.HEADER) as f:
        text = f.read()
    for name, value in (("SMHIP_TAKE_ROUTE_NONE", "0"), ("SMHIP_TAKE_ROUTE_LINE", "1"), ("SMHIP_TAKE_ROUTE_ROWS", "2"), ("SMHIP_TAKE_ROUTE_DIRECT", "3"),
                        ("SMHIP_TAKE_COPY", "0x100")):
        assert f"#define {name} {value}" in " ".join(text.split())
    assert "SMHIP_INDEX_CHECKED = 0, SMHIP_INDEX_CLIP = 1, SMHIP_INDEX_WRAP = 2" in text


def test_exports_match_the_header(lib):
    for name in ("smhip_take_axis", "smhip_take_plan"):
        assert hasattr(lib.c, name)


def test_argument_validation_needs_no_gpu(lib):
    f32, CLIP = sma.F32, sma.INDEX_CLIP
    # stand in for device pointers: every call below is rejected before anything is dereferenced or launched
    A, X, Q, B = 1 << 20, 1 << 21, 1 << 22, 1 << 23
    ok = dict(mode=CLIP, dtype=f32, a=A, sa=[8, 1], R=8, idx=X, si=[4, 1], shape=[4, 4], axis=1, out=Q, bad=B, ndim=None)

    def call(**change):
        k = dict(ok, **change)
        return lib.take_raw(k["mode"], k["dtype"], k["a"], k["sa"], k["R"], k["idx"], k["si"], k["shape"], k["axis"], k["out"], k["bad"], ndim=k["ndim"])

    bad = [
        dict(mode=3), dict(mode=-1),                                     # mode
        dict(dtype=sma.I8), dict(dtype=-1),                              # dtype
        dict(shape=[], sa=[], si=[], ndim=0, axis=0),                    # ndim 0
        dict(shape=[2] * 7, sa=dense([2] * 7), si=dense([2] * 7)),       # ndim 7
        dict(axis=-1), dict(axis=2),                                     # the C ABI does not count from the end
        dict(shape=[4, -1]), dict(shape=[-4, 4]),                        # negative extent
        dict(sa=[8, -1]), dict(sa=[-8, 1]), dict(si=[4, -1]), dict(si=[-4, 1]),  # negative strides
        dict(a=0), dict(idx=0), dict(out=0),                             # null pointers
        dict(shape=None, ndim=2), dict(sa=None), dict(si=None),          # null arrays
        dict(R=-1),                                                      # a_extent < 0
        dict(R=0),                                                       # nothing to take from, but a result to fill (numpy raises)
        dict(out=A + 4), dict(out=A - 60), dict(out=A + (3 * 8 + 7) * 4),  # out overlapping a's span (first, last byte)
        dict(out=X + 8), dict(out=X - 32), dict(out=X + 15 * 8),         # out overlapping idx's span
        dict(out=B), dict(out=B - 60), dict(bad=Q + 60),                 # out overlapping bad_out
        dict(bad=A), dict(bad=A + (3 * 8 + 7) * 4), dict(bad=A - 4),     # bad_out overlapping a's span
        dict(bad=X), dict(bad=X + 15 * 8), dict(bad=X - 4),              # bad_out overlapping idx's span
        dict(a=A, sa=[0, 2], R=100, out=A + 99 * 2 * 4),                 # a's span follows a_extent, not J
        dict(shape=[1 << 31, 1 << 31], sa=[0, 0], si=[0, 0]),              # an element count or a span that would wrap the overlap checks
        dict(shape=[1 << 40, 1 << 40], sa=[0, 0], si=[0, 0]),
        dict(sa=[1 << 61, 1]), dict(sa=[8, 1 << 62]), dict(si=[1 << 62, 1]), dict(si=[(1 << 63) - 1, (1 << 63) - 1]),
        dict(R=1 << 62), dict(R=(1 << 63) - 1, sa=[8, 3]),
    ]
    for change in bad:
        assert call(**change) == sma.ERR_INVALID, change
        assert "take_axis" in lib.c.smhip_last_error().decode()
    # the plan applies the same checks
    for change in (dict(axis=2), dict(axis=-1), dict(shape=[4, -4]), dict(sa=[-8, 1]), dict(si=[4, -1]), dict(R=-1), dict(R=0), dict(mode=5)):
        k = dict(ok, **change)
        with pytest.raises(sma.SmhipError) as e:
            lib.take_plan(np.float32, k["sa"], k["R"], k["si"], k["shape"], k["axis"], k["mode"])
        assert e.value.code == sma.ERR_INVALID
    with pytest.raises(sma.SmhipError):
        lib.take_plan(7, [8, 1], 8, [4, 1], [4, 4], 1)


def test_zero_extents_are_a_no_op_whatever_the_pointers(lib):
    for mode in (sma.INDEX_CHECKED, sma.INDEX_CLIP, sma.INDEX_WRAP):
        for dtype in (sma.F32, sma.F64, sma.I32, sma.I64):
            assert lib.take_raw(mode, dtype, 0, [5, 1], 5, 0, [0, 1], [3, 0], 1, 0, 0) == 0   # J = 0
            assert lib.take_raw(mode, dtype, 0, [5, 1], 5, 0, [4, 1], [0, 4], 1, 0, 0) == 0   # no lines
            assert lib.take_raw(mode, dtype, 0, [0, 1], 0, 0, [0, 1], [3, 0], 1, 0, 0) == 0   # nothing picked from nothing
            assert lib.take_raw(mode, dtype, 0, [1], 0, 0, [1], [0], 0, 0, 0) == 0
            assert lib.take_raw(mode, dtype, 0, [4, 4, 1], 9, 0, [0, 0, 1], [2, 0, 4], 0, 0, 4096) == 0
    assert plan(lib, ([5, 1], 5, [0, 1], [3, 0]), 1) == (sma.TAKE_ROUTE_NONE, 0, 0, (3, 0, 1), budget(lib, np.float32))
    assert plan(lib, ([4, 1, 1], 7, [0, 1, 0], [0, 3, 4]), 1)[:4] == (sma.TAKE_ROUTE_NONE, 0, 0, (0, 3, 4))


def test_python_side_checks(lib):
    class Fake:  # stands in for a DeviceArray: the checks fire before anything is allocated or launched
        def __init__(self, dtype, shape, is_dense=True):
            self.dtype, self.shape, self.ndim, self.strides = np.dtype(dtype), tuple(shape), len(shape), tuple(dense(shape))
            self.size = int(np.prod(shape))
            self.is_dense = lambda: is_dense

    a, idx = Fake(np.float32, (4, 5)), Fake(np.int64, (4, 3))
    for out in (Fake(np.int32, (4, 3)), Fake(np.float64, (4, 3)), Fake(np.float32, (4, 4)), Fake(np.float32, (4, 3), is_dense=False)):
        with pytest.raises(ValueError):
            lib.take_along_axis(a, idx, 1, out=out)
    for out in (a, idx):  # never an operand
        with pytest.raises(ValueError):
            lib.take_along_axis(a, idx, 1, out=out)
    ids = Fake(np.int64, (7,))
    for out in (a, ids, Fake(np.float32, (4, 5)), Fake(np.int64, (4, 7))):
        with pytest.raises(ValueError):
            lib.take(a, ids, 1, out=out)
    for axis in (2, -3):  # negative axes count from the end, as far as they go
        with pytest.raises(ValueError):
            lib.take_along_axis(a, idx, axis)
        with pytest.raises(ValueError):
            lib.take(a, ids, axis)
    with pytest.raises(ValueError):
        lib.take_along_axis(a, Fake(np.int64, (4, 3, 1)), 1)   # rank mismatch
    with pytest.raises(ValueError):
        lib.take_along_axis(a, Fake(np.int64, (3, 3)), 1)      # 4 against 3 does not broadcast
    with pytest.raises(ValueError):
        lib.take_along_axis(a, Fake(np.int32, (4, 3)), 1)      # the index type
    with pytest.raises(ValueError):
        lib.take(a, ids, 1, mode="fold")
    for dtype in (np.float16, np.uint32, np.int8):
        with pytest.raises(ValueError):
            lib.take(Fake(dtype, (4, 5)), ids, 1)


def test_python_wrapper_arguments(lib, monkeypatch):
    """Axis normalisation, broadcasting and np.take's stride-0 index array, seen through the arguments handed to the C ABI."""
    calls = []

    class FakeC:
        @staticmethod
        def smhip_take_axis(mode, dtype, a, sa, extent, idx, si, shape, ndim, axis, out, bad):
            n = ndim.value
            calls.append((mode.value, dtype.value, list(sa)[:n], extent.value, list(si)[:n], list(shape)[:n], axis.value, bool(bad.value)))
            return 0

    class Arr:
        def __init__(self, dtype, shape, strides=None):
            self.dtype, self.shape, self.ndim = np.dtype(dtype), tuple(shape), len(shape)
            self.strides = tuple(dense(shape) if strides is None else strides)
            self.size, self.ptr = int(np.prod(shape)), 4096
            self.is_dense = lambda: True

    monkeypatch.setattr(lib, "c", FakeC)
    monkeypatch.setattr(lib, "empty", lambda shape, dtype: Arr(dtype, shape))
    a = Arr(np.float64, (3, 4, 5))
    r = lib.take_along_axis(a, Arr(np.int64, (3, 4, 2)), -1, mode="clip")
    assert r.shape == (3, 4, 2) and r.dtype == np.float64
    assert calls[-1] == (sma.INDEX_CLIP, sma.F64, [20, 5, 1], 5, [8, 2, 1], [3, 4, 2], 2, False)
    r = lib.take_along_axis(a, Arr(np.int64, (1, 7, 5)), 1, mode="wrap")       # idx broadcast along axis 0
    assert r.shape == (3, 7, 5) and calls[-1] == (sma.INDEX_WRAP, sma.F64, [20, 5, 1], 4, [0, 5, 1], [3, 7, 5], 1, False)
    r = lib.take_along_axis(Arr(np.float64, (1, 4, 5)), Arr(np.int64, (3, 2, 5)), 1, mode="clip")  # a broadcast along axis 0
    assert r.shape == (3, 2, 5) and calls[-1][2:6] == ([0, 5, 1], 4, [10, 5, 1], [3, 2, 5])
    r = lib.take(a, Arr(np.int64, (9,)), 1, mode="clip")
    assert r.shape == (3, 9, 5) and calls[-1] == (sma.INDEX_CLIP, sma.F64, [20, 5, 1], 4, [0, 1, 0], [3, 9, 5], 1, False)
    r = lib.take(a, Arr(np.int64, (9,), (3,)), -3, mode="wrap")                  # a stepped 1-D index view
    assert r.shape == (9, 4, 5) and calls[-1][2:7] == ([20, 5, 1], 3, [3, 0, 0], [9, 4, 5], 0)


def test_plan_line_bounds(lib):
    LINE, DIRECT = sma.TAKE_ROUTE_LINE, sma.TAKE_ROUTE_DIRECT
    for dtype in DTYPES:
        K, c = budget(lib, dtype), ratio(lib, dtype)
        assert K * np.dtype(dtype).itemsize == 32 << 10 and c >= 1
        for R in (1, 2, 63, 64, 65, 255, 256, 257, K - 1, K):
            for J in (1, R, 3 * R + 1):
                want = LINE if J * c >= R else DIRECT
                for O in (1, 7, 1000):
                    assert plan(lib, along((O, R), (O, J), 1), 1, dtype) == (want, 0, 1, (O, J, 1), K), (R, J, O)
        # just past each bound
        assert plan(lib, along((7, K + 1), (7, K + 1), 1), 1, dtype)[0] == DIRECT
        for R in (K, 1000, 37 * c + 1):
            J = -(-R // c)
            assert plan(lib, along((7, R), (7, J), 1), 1, dtype)[0] == LINE
            if J > 1:
                assert plan(lib, along((7, R), (7, J - 1), 1), 1, dtype)[0] == DIRECT
        # np.take along the last axis is the same walk with a broadcast index line
        assert plan(lib, take1d((7, 300), 300, 1), 1, dtype) == (LINE, 0, 1, (7, 300, 1), K)
        # the mode does not enter the plan
        for mode in ("checked", "wrap"):
            assert plan(lib, along((7, 300), (7, 300), 1), 1, dtype, mode) == plan(lib, along((7, 300), (7, 300), 1), 1, dtype)
        # a line that is not contiguous is not staged
        assert plan(lib, along((7, 300), (7, 300), 1, a_strides=(600, 2)), 1, dtype)[0] == DIRECT


def test_plan_rows_bounds(lib):
    ROWS, DIRECT = sma.TAKE_ROUTE_ROWS, sma.TAKE_ROUTE_DIRECT
    for dtype in DTYPES:
        W, K = 16 // np.dtype(dtype).itemsize, budget(lib, dtype)
        for R in (1, 5, 300):
            for n in (1, 3, 1025):
                for I in (W, W + 1, 255, 256, 257, 1000):
                    assert plan(lib, take1d((R, I), n, 0), 0, dtype) == (ROWS, 0, 1, (1, n, I), K), (R, n, I)
                for I in range(2, W):
                    got = plan(lib, take1d((R, I), n, 0), 0, dtype)
                    assert got[0] == DIRECT and got[1:4] == (0, 1, (1, n, I)), (R, n, I)
                # I = 1 is a 1-D take: never a row copy (a short table is a line for LINE)
                assert plan(lib, take1d((R, 1), n, 0), 0, dtype)[0] in (DIRECT, sma.TAKE_ROUTE_LINE)
        # a middle axis: the axes before it are the O of the walk
        assert plan(lib, take1d((3, 5, 64), 9, 1), 1, dtype) == (ROWS, 0, 1, (3, 9, 64), K)
        # a sub-block of a wider table keeps its rows
        assert plan(lib, take1d((5, 64), 9, 0, a_strides=(100, 1)), 0, dtype)[0] == ROWS
        # an index array that varies along the row is not a row copy
        assert plan(lib, along((5, 64), (9, 64), 0), 0, dtype) == (DIRECT, 0, 1, (1, 9, 64), K)
        # ... nor is a row that is not contiguous
        assert plan(lib, take1d((5, 64), 9, 0, a_strides=(128, 2)), 0, dtype)[0] == DIRECT


def test_plan_views(lib):
    LINE, ROWS, DIRECT, Y = sma.TAKE_ROUTE_LINE, sma.TAKE_ROUTE_ROWS, sma.TAKE_ROUTE_DIRECT, sma.TAKE_COPY
    K = budget(lib, np.float32)
    # A is (50, 300) dense; A.T is (300, 50) with strides (1, 300).  take(A.T, ids, 0) walks a's memory like take(A, ids, 1):
    # the same route and extents, read in place
    twin = plan(lib, take1d((50, 300), 300, 1), 1)
    assert twin == (LINE, 0, 1, (50, 300, 1), K)
    assert plan(lib, take1d((300, 50), 300, 0, a_strides=(1, 300)), 0) == twin
    # ... and take(A.T, ids, 1) like take(A, ids, 0)
    twin = plan(lib, take1d((50, 300), 9, 0), 0)
    assert twin[0] == ROWS
    got = plan(lib, take1d((300, 50), 9, 1, a_strides=(1, 300)), 1)
    assert got[1] == 0 and got[2] == 1 and got[3] == (1, 9, 300)   # the same walk, in place; the result's rows are not contiguous
    assert got[0] == DIRECT                                       # so it is not a row copy
    # take_along_axis with both operands transposed
    assert plan(lib, along((300, 50), (300, 50), 0, a_strides=(1, 300), idx_strides=(1, 300)), 0) == (LINE, 0, 1, (50, 300, 1), K)
    # a broadcast a is read in place: one line for every o, one row for every o
    assert plan(lib, along((1, 300), (40, 300), 1), 1) == (LINE, 0, 1, (40, 300, 1), K)
    assert plan(lib, along((40, 300), (40, 300), 1, a_strides=(0, 1)), 1) == (LINE, 0, 1, (40, 300, 1), K)
    assert plan(lib, along((1, 300), (40, 5), 1), 1)[:4] == (DIRECT, 0, 1, (40, 5, 1))            # too few picks to stage the line
    assert plan(lib, along((300, 1), (7, 40), 0), 0)[:3] == (DIRECT, 0, 1)                        # a column broadcast over the rows
    assert plan(lib, along((40, 300), (40, 300), 1, a_strides=(300, 0)), 1)[:3] == (DIRECT, 0, 1)  # ... along the gathered axis itself
    # a stepped 2-D a is still a three-axis walk
    assert plan(lib, along((40, 300), (40, 300), 1, a_strides=(1200, 2)), 1) == (DIRECT, 0, 1, (40, 300, 1), K)
    # a stepped a whose kept axes do not merge is copied dense first: one launch more
    assert plan(lib, along((4, 5, 300), (4, 5, 300), 2, a_strides=(6000, 600, 1)), 2) == (LINE, Y, 2, (20, 300, 1), K)
    assert plan(lib, take1d((4, 5, 6, 64), 9, 1, a_strides=(10000, 1000, 128, 1)), 1) == (ROWS, Y, 2, (4, 9, 384), K)
    # an index array that does not merge is copied instead, and a stays in place
    assert plan(lib, along((4, 5, 300), (4, 5, 300), 2, idx_strides=(300, 1200, 1)), 2) == (LINE, Y, 2, (20, 300, 1), K)
    # both
    assert plan(lib, along((4, 5, 300), (4, 5, 300), 2, a_strides=(6000, 600, 1), idx_strides=(300, 1200, 1)), 2) == (LINE, Y, 3, (20, 300, 1), K)
    # rank 6, every axis: O * J * I is the element count, J the named extent
    shape = (2, 3, 2, 3, 2, 3)
    for axis in range(6):
        idx_shape = list(shape)
        idx_shape[axis] = 5
        route, flags, launches, oji, _ = plan(lib, along(shape, idx_shape, axis), axis)
        assert flags == 0 and launches == 1 and oji[1] == 5 and oji[0] * oji[1] * oji[2] == 5 * int(np.prod(shape)) // shape[axis]
        assert route == (LINE if axis == 5 else DIRECT)
