"""put_along_axis / put / scatter_add / index_add, host side: the C ABI's argument checks, the planner (smhip_scatter_plan) and the
Python binding's own checks -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma

DTYPES = (np.float32, np.float64, np.int32, np.int64)
NONE, DIRECT, ROWS, SORTED, SORTED_ROWS, COPY = (sma.SCATTER_ROUTE_NONE, sma.SCATTER_ROUTE_DIRECT, sma.SCATTER_ROUTE_ROWS, sma.SCATTER_ROUTE_SORTED,
                                                 sma.SCATTER_ROUTE_SORTED_ROWS, sma.SCATTER_COPY)


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


def walk(out_shape, axis, J):
    w = list(out_shape)
    w[axis] = J
    return w


def full(out_shape, axis, J):
    """A full index array and full values: dense over the walk shape."""
    st = dense(walk(out_shape, axis, J))
    return st, st


def ids1d(out_shape, axis, J, stride=1):
    """put(a, ids[J], values, axis): the index array has stride 0 on every axis but `axis`, the values are dense."""
    si = [0] * len(out_shape)
    si[axis] = stride
    return si, dense(walk(out_shape, axis, J))


def plan(lib, out_shape, axis, J, strides, dtype=np.float32, unique=False, kind=sma.SCATTER_PUT, mode="clip"):
    """(route id, flags, launches, (O, R, J, I), sorted entries)"""
    si, sv = strides
    route, launches, orji, nsorted = lib.scatter_plan(dtype, out_shape, axis, si, sv, J, unique=unique, kind=kind, mode=mode)
    return route & 0xff, route & ~0xff, launches, orji, nsorted


def sort_launches(lib, lines, J):
    return lib.sort_plan(np.int64, (lines, J), (J, 1), 1)[1]


def test_entry_points_and_constants_are_declared():
    names = sma.declared_symbols()
    assert "smhip_scatter_axis" in names and "smhip_scatter_plan" in names
    assert (sma.SCATTER_PUT, sma.SCATTER_ADD, sma.SCATTER_UNIQUE) == (0, 1, 1)
    assert (NONE, DIRECT, ROWS, SORTED, SORTED_ROWS, COPY) == (0, 1, 2, 3, 4, 0x100)
    with open(sma.HEADER) as f:
        text = f.read()
    for name, value in (("SMHIP_SCATTER_ROUTE_NONE", "0"), ("SMHIP_SCATTER_ROUTE_DIRECT", "1"), ("SMHIP_SCATTER_ROUTE_ROWS", "2"),
                        ("SMHIP_SCATTER_ROUTE_SORTED", "3"), ("SMHIP_SCATTER_ROUTE_SORTED_ROWS", "4"), ("SMHIP_SCATTER_COPY", "0x100"),
                        ("SMHIP_SCATTER_UNIQUE", "1")):
        assert f"#define {name} {value}" in " ".join(text.split())
    assert "SMHIP_SCATTER_PUT = 0, SMHIP_SCATTER_ADD = 1" in text


def test_exports_match_the_header(lib):
    for name in ("smhip_scatter_axis", "smhip_scatter_plan"):
        assert hasattr(lib.c, name)


def test_argument_validation_needs_no_gpu(lib):
    f32, CLIP, PUT = sma.F32, sma.INDEX_CLIP, sma.SCATTER_PUT
    # stand in for device pointers: every call below is rejected before anything is dereferenced or launched
    Q, X, V, B = 1 << 20, 1 << 21, 1 << 22, 1 << 23
    # out (4, 8) f32: 128 bytes; idx (4, 4) int64: 128 bytes; values (4, 4) f32: 64 bytes
    ok = dict(kind=PUT, mode=CLIP, flags=0, dtype=f32, out=Q, shape=[4, 8], axis=1, idx=X, si=[4, 1], val=V, sv=[4, 1], J=4, bad=B, ndim=None)

    def call(**change):
        k = dict(ok, **change)
        return lib.scatter_raw(k["kind"], k["mode"], k["flags"], k["dtype"], k["out"], k["shape"], k["axis"], k["idx"], k["si"], k["val"], k["sv"], k["J"],
                               k["bad"], ndim=k["ndim"])

    bad = [
        dict(kind=2), dict(kind=-1),                                       # kind
        dict(mode=3), dict(mode=-1),                                       # mode
        dict(flags=2), dict(flags=3), dict(flags=-1), dict(flags=0x100),   # unknown flag bits
        dict(dtype=sma.I8), dict(dtype=-1),                                # dtype
        dict(shape=[], si=[], sv=[], ndim=0, axis=0),                      # ndim 0
        dict(shape=[2] * 7, si=dense([2] * 7), sv=dense([2] * 7)),         # ndim 7
        dict(axis=-1), dict(axis=2),                                       # the C ABI does not count from the end
        dict(shape=[4, -1]), dict(shape=[-4, 8]),                          # negative extent
        dict(si=[4, -1]), dict(si=[-4, 1]), dict(sv=[4, -1]), dict(sv=[-4, 1]),  # negative strides
        dict(J=-1),                                                        # J < 0
        dict(out=0), dict(idx=0), dict(val=0),                             # null pointers
        dict(shape=None, ndim=2), dict(si=None), dict(sv=None),            # null arrays
        dict(shape=[4, 0]),                                                # R == 0 with entries to place
        dict(idx=Q + 8), dict(idx=Q - 120), dict(idx=Q + 127),             # out overlapping idx's span (inside, first, last byte)
        dict(val=Q + 4), dict(val=Q - 60), dict(val=Q + 124),              # out overlapping values' span
        dict(bad=Q), dict(bad=Q + 124), dict(bad=Q - 4),                   # out overlapping bad_out
        dict(bad=X), dict(bad=X + 15 * 8), dict(bad=X - 4),                # bad_out overlapping idx's span
        dict(bad=V), dict(bad=V + 15 * 4), dict(bad=V - 4),                # bad_out overlapping values' span
        dict(val=V, sv=[0, 2], J=100, si=[0, 0], out=V + 99 * 2 * 4),      # values' span follows J, not R
        dict(shape=[1 << 31, 8], J=1 << 31, si=[0, 0], sv=[0, 0], flags=1),  # an element count or a span that would wrap the overlap checks
        dict(shape=[1 << 40, 1 << 40], si=[0, 0], sv=[0, 0]),
        dict(si=[1 << 61, 1]), dict(si=[4, 1 << 62]), dict(sv=[1 << 62, 1]), dict(sv=[(1 << 63) - 1, (1 << 63) - 1]),
        dict(J=1 << 62, si=[0, 0], sv=[0, 0], flags=1),
    ]
    for change in bad:
        assert call(**change) == sma.ERR_INVALID, change
        assert "scatter_axis" in lib.c.smhip_last_error().decode()
    # the sort's limit: J >= 2^31 without the unique routes
    assert call(J=1 << 31, si=[0, 0], sv=[0, 0]) == sma.ERR_UNSUPPORTED
    assert call(J=(1 << 31) - 1, si=[0, 0], sv=[0, 0], out=0) == sma.ERR_INVALID  # passes that check and reaches the null pointer
    assert call(J=1 << 31, si=[0, 0], sv=[0, 0], flags=1, out=0) == sma.ERR_INVALID
    # the plan applies the same checks
    for change in (dict(axis=2), dict(axis=-1), dict(shape=[4, -4]), dict(si=[-4, 1]), dict(sv=[4, -1]), dict(J=-1), dict(shape=[4, 0]), dict(mode=5),
                   dict(kind=2)):
        k = dict(ok, **change)
        with pytest.raises(sma.SmhipError) as e:
            lib.scatter_plan(np.float32, k["shape"], k["axis"], k["si"], k["sv"], k["J"], kind=k["kind"], mode=k["mode"])
        assert e.value.code == sma.ERR_INVALID
    with pytest.raises(sma.SmhipError):
        lib.scatter_plan(7, [4, 8], 1, [4, 1], [4, 1], 4)
    with pytest.raises(sma.SmhipError) as e:
        lib.scatter_plan(np.float32, [4, 8], 1, [0, 0], [0, 0], 1 << 31)
    assert e.value.code == sma.ERR_UNSUPPORTED


def test_zero_extents_are_a_no_op_whatever_the_pointers(lib):
    for kind in (sma.SCATTER_PUT, sma.SCATTER_ADD):
        for mode in (sma.INDEX_CHECKED, sma.INDEX_CLIP, sma.INDEX_WRAP):
            for flags in (0, sma.SCATTER_UNIQUE):
                for dtype in (sma.F32, sma.F64, sma.I32, sma.I64):
                    assert lib.scatter_raw(kind, mode, flags, dtype, 0, [3, 5], 1, 0, [0, 1], 0, [0, 1], 0) == 0   # J = 0
                    assert lib.scatter_raw(kind, mode, flags, dtype, 0, [0, 5], 1, 0, [4, 1], 0, [4, 1], 4) == 0   # no lines
                    assert lib.scatter_raw(kind, mode, flags, dtype, 0, [3, 0], 1, 0, [0, 1], 0, [0, 1], 0) == 0   # nothing placed on nothing
                    assert lib.scatter_raw(kind, mode, flags, dtype, 0, [0], 0, 0, [1], 0, [1], 0) == 0
                    assert lib.scatter_raw(kind, mode, flags, dtype, 0, [9, 0, 4], 0, 0, [0, 0, 1], 0, [0, 0, 0], 2, 4096) == 0
    assert plan(lib, [3, 5], 1, 0, ([0, 1], [0, 1])) == (NONE, 0, 0, (3, 5, 0, 1), 0)
    assert plan(lib, [0, 7, 4], 1, 3, ([0, 1, 0], [12, 4, 1])) == (NONE, 0, 0, (0, 7, 3, 4), 0)


def test_plan_unique_and_sorted(lib):
    for dtype in DTYPES:
        for kind in (sma.SCATTER_PUT, sma.SCATTER_ADD):
            for R in (1, 2, 65, 4096, 4097):
                for J in (1, 2, R, 3 * R + 1):
                    for O in (1, 7):
                        args = ([O, R], 1, J, full([O, R], 1, J))
                        assert plan(lib, *args, dtype, True, kind) == (DIRECT, 0, 1, (O, R, J, 1), 0)
                        if J <= 1:  # unique by construction
                            assert plan(lib, *args, dtype, False, kind) == (DIRECT, 0, 1, (O, R, J, 1), 0)
                        else:
                            assert plan(lib, *args, dtype, False, kind) == (SORTED, 0, 2 + sort_launches(lib, O, J), (O, R, J, 1), O * J), (R, J, O)
        # the mode does not enter the plan
        for mode in ("checked", "wrap"):
            for unique in (False, True):
                assert plan(lib, [7, 300], 1, 300, full([7, 300], 1, 300), dtype, unique, mode=mode) == plan(lib, [7, 300], 1, 300, full([7, 300], 1, 300), dtype, unique)
    # a line longer than the sort's tile: its merge passes are counted
    assert sort_launches(lib, 3, 4097) > sort_launches(lib, 3, 4096)


def test_plan_rows_bounds(lib):
    for dtype in DTYPES:
        W = 16 // np.dtype(dtype).itemsize
        for R in (1, 5, 300):
            for n in (1, 3, 1025):
                for I in (W, W + 1, 255, 256, 257, 1000):
                    assert plan(lib, [R, I], 0, n, ids1d([R, I], 0, n), dtype, True) == (ROWS, 0, 1, (1, R, n, I), 0), (R, n, I)
                    want = (ROWS, 0, 1, (1, R, n, I), 0) if n == 1 else (SORTED_ROWS, 0, 2 + sort_launches(lib, 1, n), (1, R, n, I), n)
                    assert plan(lib, [R, I], 0, n, ids1d([R, I], 0, n), dtype, False) == want, (R, n, I)
                for I in range(1, W):
                    assert plan(lib, [R, I], 0, n, ids1d([R, I], 0, n), dtype, True)[:4] == (DIRECT, 0, 1, (1, R, n, I)), (R, n, I)
                    if n > 1:
                        assert plan(lib, [R, I], 0, n, ids1d([R, I], 0, n), dtype, False) == (SORTED, 0, 2 + sort_launches(lib, 1, n), (1, R, n, I), n)
        # a middle axis: the axes before it are the O of the walk; a 1-D ids is sorted once, a full index array line by line
        assert plan(lib, [3, 5, 64], 1, 9, ids1d([3, 5, 64], 1, 9), dtype) == (SORTED_ROWS, 0, 2 + sort_launches(lib, 1, 9), (3, 5, 9, 64), 9)
        assert plan(lib, [3, 5, 64], 1, 9, full([3, 5, 64], 1, 9), dtype) == (SORTED, 0, 2 + sort_launches(lib, 192, 9), (3, 5, 9, 64), 3 * 9 * 64)
        # idx varying over the outer axis only keeps the rows
        assert plan(lib, [3, 5, 64], 1, 9, ([9, 1, 0], dense([3, 9, 64])), dtype) == (SORTED_ROWS, 0, 2 + sort_launches(lib, 3, 9), (3, 5, 9, 64), 27)
        # values that are not contiguous along the row, or a scalar value: no row route
        assert plan(lib, [5, 64], 0, 9, ([1, 0], [128, 2]), dtype, True)[0] == DIRECT
        assert plan(lib, [5, 64], 0, 9, ([1, 0], [0, 0]), dtype)[0] == SORTED
        # a sub-block of wider values keeps its rows
        assert plan(lib, [5, 64], 0, 9, ([1, 0], [100, 1]), dtype, True)[0] == ROWS


def test_plan_views(lib):
    # transposed idx / values are walked in place
    assert plan(lib, [6, 50], 1, 120, ([1, 6], [1, 6])) == (SORTED, 0, 2 + sort_launches(lib, 6, 120), (6, 50, 120, 1), 720)
    # stepped views whose kept axes still run on
    assert plan(lib, [4, 6, 20], 2, 9, ([108, 18, 1], [216, 36, 2]))[:2] == (SORTED, 0)
    # an index array that does not merge is copied dense first: one launch more
    base = 2 + sort_launches(lib, 24, 9)
    assert plan(lib, [4, 6, 20], 2, 9, ([216, 18, 1], dense([4, 6, 9]))) == (SORTED, COPY, base + 1, (24, 20, 9, 1), 216)
    # ... or the values, and idx stays in place
    assert plan(lib, [4, 6, 20], 2, 9, (dense([4, 6, 9]), [216, 18, 1])) == (SORTED, COPY, base + 1, (24, 20, 9, 1), 216)
    # both
    assert plan(lib, [4, 6, 20], 2, 9, ([216, 18, 1], [216, 18, 1])) == (SORTED, COPY, base + 2, (24, 20, 9, 1), 216)
    assert plan(lib, [4, 6, 20], 2, 9, ([216, 18, 1], [216, 18, 1]), unique=True) == (DIRECT, COPY, 3, (24, 20, 9, 1), 0)
    # J = 1 drops the axis from the merged list.  Two groups that both stand BEFORE it are kept axes that did not merge, never
    # "[O] J [I]": out's stride along the second one is R, not 1, so it is no row.  One operand is copied and the groups merge.
    for dtype in DTYPES:
        assert plan(lib, [3, 8, 5], 2, 1, ([1, 0, 0], [8, 1, 0]), dtype) == (DIRECT, COPY, 2, (24, 5, 1, 1), 0)     # idx (3, 1, 1), values (3, 8, 1)
        assert plan(lib, [3, 8, 5], 2, 1, ([0, 0, 0], [16, 1, 0]), dtype) == (DIRECT, COPY, 2, (24, 5, 1, 1), 0)    # one id, row-pitched values
        assert plan(lib, [3, 8, 5], 2, 1, ([8, 1, 0], [8, 1, 0]), dtype) == (DIRECT, 0, 1, (24, 5, 1, 1), 0)
        assert plan(lib, [3, 8, 5], 2, 1, ([1, 0, 0], [1, 0, 0]), dtype) == (DIRECT, COPY, 3, (24, 5, 1, 1), 0)
        # ... and two groups AFTER it likewise
        assert plan(lib, [5, 3, 8], 0, 1, ([0, 0, 0], [0, 16, 1]), dtype)[:2] == (ROWS, COPY)
        # one group on either side is the walk, and the one after the axis is a row
        assert plan(lib, [3, 8, 5], 1, 1, ([1, 0, 0], [5, 0, 1]), dtype) == (ROWS, 0, 1, (3, 8, 1, 5), 0)
        assert plan(lib, [3, 8, 5], 0, 1, ([0, 0, 0], [0, 5, 1]), dtype) == (ROWS, 0, 1, (1, 3, 1, 40), 0)
    # rank 6, every axis: O * J * I is the entry count, R and J the named extents
    shape = (2, 3, 2, 3, 2, 3)
    for axis in range(6):
        route, flags, launches, orji, nsorted = plan(lib, shape, axis, 5, full(shape, axis, 5))
        assert flags == 0 and orji[1] == shape[axis] and orji[2] == 5 and orji[0] * orji[3] == int(np.prod(shape)) // shape[axis]
        assert route == SORTED and nsorted == 5 * orji[0] * orji[3] and launches == 2 + sort_launches(lib, orji[0] * orji[3], 5)


class Fake:  # stands in for a DeviceArray: the checks fire before anything is allocated or launched
    def __init__(self, dtype, shape, is_dense=True, strides=None):
        self.dtype, self.shape, self.ndim = np.dtype(dtype), tuple(shape), len(shape)
        self.strides = tuple(dense(shape) if strides is None else strides)
        self.size, self.ptr = int(np.prod(shape)), 4096
        self.is_dense = lambda: is_dense


def test_python_side_checks(lib, monkeypatch):
    monkeypatch.setattr(sma, "DeviceArray", Fake)
    a, idx, ids, v = Fake(np.float32, (4, 5)), Fake(np.int64, (4, 3)), Fake(np.int64, (7,)), Fake(np.float32, (4, 3))
    for fn in (lib.put_along_axis, lib.scatter_add):
        for axis in (2, -3):
            with pytest.raises(ValueError):
                fn(a, idx, v, axis)
        with pytest.raises(ValueError):
            fn(a, Fake(np.int64, (4, 3, 1)), v, 1)          # rank mismatch
        with pytest.raises(ValueError):
            fn(a, Fake(np.int64, (3, 3)), v, 1)             # 4 against 3
        with pytest.raises(ValueError):
            fn(a, Fake(np.int32, (4, 3)), v, 1)             # the index type
        with pytest.raises(ValueError):
            fn(a, idx, Fake(np.float64, (4, 3)), 1)         # the values' type
        with pytest.raises(ValueError):
            fn(a, idx, Fake(np.float32, (4, 2)), 1)         # values that do not broadcast against idx
        with pytest.raises(ValueError):
            fn(Fake(np.float32, (4, 5), is_dense=False), idx, v, 1)  # the target is dense
        with pytest.raises(ValueError):
            fn(a, idx, a, 1)                                # never an operand
        with pytest.raises(ValueError):
            fn(a, idx, v, 1, mode="fold")
        for dtype in (np.float16, np.uint32, np.int8):
            with pytest.raises(ValueError):
                fn(Fake(dtype, (4, 5)), idx, Fake(dtype, (4, 3)), 1)
    for fn in (lib.put, lib.index_add):
        for axis in (2, -3):
            with pytest.raises(ValueError):
                fn(a, ids, Fake(np.float32, (4, 7)), axis)
        with pytest.raises(ValueError):
            fn(a, ids, Fake(np.float32, (4, 6)), 1)
        with pytest.raises(ValueError):
            fn(a, Fake(np.int32, (7,)), Fake(np.float32, (4, 7)), 1)
        with pytest.raises(ValueError):
            fn(Fake(np.float32, (4, 5), is_dense=False), ids, Fake(np.float32, (4, 7)), 1)


def test_python_wrapper_arguments(lib, monkeypatch):
    """Axis normalisation, broadcasting and put's stride-0 index array, seen through the arguments handed to the C ABI."""
    calls = []

    class FakeC:
        @staticmethod
        def smhip_scatter_axis(kind, mode, flags, dtype, out, shape, ndim, axis, idx, si, val, sv, J, bad):
            n = ndim.value
            calls.append((kind.value, mode.value, flags.value, dtype.value, list(shape)[:n], axis.value, list(si)[:n], list(sv)[:n], J.value, bool(bad.value)))
            return 0

    monkeypatch.setattr(sma, "DeviceArray", Fake)
    monkeypatch.setattr(lib, "c", FakeC)
    monkeypatch.setattr(lib, "broadcast", lambda s1, st1, s2, st2: numpy_broadcast(s1, st1, s2, st2))
    monkeypatch.setattr(lib, "to_device", lambda host: Fake(host.dtype, host.shape))
    a = Fake(np.float64, (3, 4, 5))
    r = lib.put_along_axis(a, Fake(np.int64, (3, 4, 2)), Fake(np.float64, (3, 4, 2)), -1, mode="clip")
    assert r is a and calls[-1] == (sma.SCATTER_PUT, sma.INDEX_CLIP, 0, sma.F64, [3, 4, 5], 2, [8, 2, 1], [8, 2, 1], 2, False)
    lib.scatter_add(a, Fake(np.int64, (1, 7, 5)), Fake(np.float64, (7, 1)), 1, mode="wrap", unique=True)   # idx and values broadcast
    assert calls[-1] == (sma.SCATTER_ADD, sma.INDEX_WRAP, sma.SCATTER_UNIQUE, sma.F64, [3, 4, 5], 1, [0, 5, 1], [0, 1, 0], 7, False)
    lib.put_along_axis(a, Fake(np.int64, (3, 4, 2)), 2.5, 2, mode="clip")                                  # a scalar value
    assert calls[-1][6:9] == ([8, 2, 1], [0, 0, 0], 2)
    lib.put(a, Fake(np.int64, (9,)), Fake(np.float64, (3, 9, 5)), 1, mode="clip")
    assert calls[-1] == (sma.SCATTER_PUT, sma.INDEX_CLIP, 0, sma.F64, [3, 4, 5], 1, [0, 1, 0], [45, 5, 1], 9, False)
    lib.index_add(a, Fake(np.int64, (9,), strides=(3,)), Fake(np.float64, (4, 5)), -3, mode="wrap")        # a stepped 1-D index view
    assert calls[-1] == (sma.SCATTER_ADD, sma.INDEX_WRAP, 0, sma.F64, [3, 4, 5], 0, [3, 0, 0], [0, 5, 1], 9, False)


def numpy_broadcast(shape1, strides1, shape2, strides2):
    """lib.broadcast's answer without the library: (shape, strides1, strides2, total), or None."""
    nd = max(len(shape1), len(shape2))
    p1, q1 = [1] * (nd - len(shape1)) + list(shape1), [0] * (nd - len(shape1)) + list(strides1)
    p2, q2 = [1] * (nd - len(shape2)) + list(shape2), [0] * (nd - len(shape2)) + list(strides2)
    shape, s1, s2 = [], [], []
    for n1, t1, n2, t2 in zip(p1, q1, p2, q2):
        if n1 != n2 and n1 != 1 and n2 != 1:
            return None
        n = n2 if n1 == 1 else n1
        shape.append(n), s1.append(t1 if n1 == n and n != 1 else 0), s2.append(t2 if n2 == n and n != 1 else 0)
    return shape, s1, s2, int(np.prod(shape))
