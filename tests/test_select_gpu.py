"""where / count_nonzero / flatnonzero / nonzero / a[mask] on the GPU (the C ABI through the ctypes binding) against numpy, exactly.

The oracle is numpy alone: np.where, np.count_nonzero, np.flatnonzero, np.nonzero and a[mask], every scalar cast to the array's dtype
first so that numpy's promotion cannot change the expected dtype.  Every comparison is of bytes.  Results of the raw calls are the MIDDLE
THIRD of a buffer of sentinels whose outer thirds must come back byte-identical; the count word holds garbage before the call.  The
tile, and the largest size of the one-workgroup route, are taken from the plan."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
CMP_NAMES = ("nonzero", "eq", "ne", "lt", "le", "gt", "ge")
PATTERNS = ("none", "all", "first", "last", "tile_edge", "alternating", "half", "percent")
INDEX, COORDS, VALUES = sma.SELECT_INDEX, sma.SELECT_COORDS, sma.SELECT_VALUES
ONE, TILES, DENSE, COPY = sma.SELECT_ROUTE_ONE, sma.SELECT_ROUTE_TILES, sma.SELECT_ROUTE_DENSE, sma.SELECT_COPY
GARBAGE = 0x5A5A5A5A5A5A5A5A
SENTINEL = 0x7B


def dense(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.insert(0, acc)
        acc *= d
    return st


def constants(lib, dtype):
    """(the elements of a tile, the largest element count of the one-workgroup route)"""
    info = lib.select_plan("index", dtype, [1000], [1])[2]
    return info[1], info[2]


def sizes(lib, dtype):
    tile, threshold = constants(lib, dtype)
    return sorted({0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, threshold - 1, threshold, threshold + 1, tile - 1, tile, tile + 1, 2 * tile + 3, 70001,
                   129 * tile + 5})


class Guarded:
    """n items of `dtype` as the middle third of a buffer of sentinel bytes; misalign: the result starts that many items off."""

    def __init__(self, lib, n, dtype=np.int64, misalign=0):
        dtype = np.dtype(dtype)
        per16 = 16 // dtype.itemsize
        self.n, self.third = n, (n + per16) // per16 * per16 + misalign
        self.host = np.full(3 * self.third * dtype.itemsize, SENTINEL, np.uint8).view(dtype)
        self.buf = lib.to_device(self.host)
        self.ptr = self.buf.ptr + dtype.itemsize * self.third

    def result(self):
        back = self.buf.numpy()
        t, n = self.third, self.n
        assert back[:t].tobytes() == self.host[:t].tobytes() and back[t + n:].tobytes() == self.host[t + n:].tobytes(), "a write outside the result"
        return back[t:t + n]


def off_by_one(lib, host):
    """`host` (1-D) on the device starting one element into a buffer: not 16-byte aligned."""
    base = np.concatenate([host[:1], host]) if host.size else np.zeros(1, host.dtype)
    return lib.to_device(base).view_like(base[1:], base)


def count_word(lib):
    return lib.to_device(np.array([GARBAGE], np.uint64).view(np.int64))


def np_cond(cmp, x, rhs):
    """numpy's answer; rhs an array or a scalar ALREADY of x's dtype."""
    with np.errstate(invalid="ignore"):
        return {"nonzero": lambda: x != x.dtype.type(0), "eq": lambda: x == rhs, "ne": lambda: x != rhs, "lt": lambda: x < rhs, "le": lambda: x <= rhs,
                "gt": lambda: x > rhs, "ge": lambda: x >= rhs}[cmp]()


def rhs_args(lib, dx, rhs):
    """-> (y ptr, y strides, the scalar as a 1-element array)"""
    if isinstance(rhs, sma.DeviceArray):
        return rhs.ptr, rhs.strides, None
    return 0, None, None if rhs is None else np.array([rhs]).astype(dx.dtype)


def raw_count(lib, cmp, dx, rhs=None):
    word = count_word(lib)
    y, ys, s = rhs_args(lib, dx, rhs)
    rc = lib.select_count_raw(sma.CMPS[cmp], sma.DTYPES[dx.dtype], dx.ptr, dx.strides, y, ys, s, dx.shape, word.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    return int(word.numpy()[0])


def raw_select(lib, what, cmp, dx, rhs=None, dsrc=None, capacity=None, total=None, misalign=0, with_count=True):
    """One smhip_select into a guarded buffer of `capacity` items (default: the total) -> (the items written, the count word).  `total`
    is what numpy counts: exactly min(total, capacity) items may be written."""
    capacity = total if capacity is None else capacity
    planes = dx.ndim if what == COORDS else 1
    out = Guarded(lib, planes * capacity, dsrc.dtype if what == VALUES else np.int64, misalign)
    word = count_word(lib)
    y, ys, s = rhs_args(lib, dx, rhs)
    rc = lib.select_raw(what, sma.CMPS[cmp], sma.DTYPES[dx.dtype], dx.ptr, dx.strides, y, ys, s, dx.shape, dsrc.ptr if what == VALUES else 0,
                        dsrc.strides if what == VALUES else None, dsrc.dtype.itemsize if what == VALUES else 0, out.ptr, capacity, word.ptr if with_count else 0)
    assert rc == 0, lib.c.smhip_last_error().decode()
    got = out.result()
    written = min(total, capacity)
    if what == COORDS:
        got = got.reshape(planes, capacity)
        assert (got[:, written:].view(np.uint8) == SENTINEL).all(), "a write past the items counted"
        got = got[:, :written]
    else:
        assert (got[written:].view(np.uint8) == SENTINEL).all(), "a write past the items counted"
        got = got[:written]
    return got, int(word.numpy()[0]) if with_count else None


def check_compaction(lib, cmp, x, rhs_host=None, dx=None, drhs=None, src=None, dsrc=None, misalign=0, route=None, coords=True):
    """count, INDEX, COORDS and VALUES of one condition against numpy."""
    dx = lib.to_device(x) if dx is None else dx
    if isinstance(rhs_host, np.ndarray):
        rhs = drhs if drhs is not None else lib.to_device(rhs_host)
    else:
        rhs = rhs_host
    mask = np_cond(cmp, x, rhs_host if rhs_host is None or isinstance(rhs_host, np.ndarray) else x.dtype.type(rhs_host))
    mask = np.broadcast_to(mask, x.shape)
    total = int(np.count_nonzero(mask))
    if route is not None:
        assert lib.select_plan("index", x.dtype, dx.shape, dx.strides, rhs.strides if isinstance(rhs, sma.DeviceArray) else None)[0] == route
    tag = (x.dtype.name, cmp, x.shape, misalign)
    assert raw_count(lib, cmp, dx, rhs) == total, tag
    got, counted = raw_select(lib, INDEX, cmp, dx, rhs, total=total, misalign=misalign)
    assert counted == total and np.array_equal(got, np.flatnonzero(mask)), tag
    if coords:
        got, counted = raw_select(lib, COORDS, cmp, dx, rhs, total=total, misalign=misalign)
        assert counted == total and np.array_equal(got, np.stack(np.nonzero(mask)).astype(np.int64).reshape(x.ndim, total)), tag
    if src is not None:
        dsrc = lib.to_device(src) if dsrc is None else dsrc
        got, counted = raw_select(lib, VALUES, cmp, dx, rhs, dsrc=dsrc, total=total, misalign=misalign)
        assert counted == total and got.tobytes() == src[mask].tobytes(), tag
    return total


def pattern(kind, n, tile, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[:1] = True
    elif kind == "last":
        m[n - 1:] = True
    elif kind == "tile_edge":       # the last element of a tile and the first of the next, for every tile boundary inside n
        for e in range(tile, n, tile):
            m[e - 1] = m[e] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind == "half":
        m = rng.random(n) < 0.5
    elif kind == "percent":
        m = rng.random(n) < 0.01
    return m


def specials(dtype, n, seed, scalar):
    """n values that hold NaN, both zeros, the infinities and `scalar` (floats), or the extremes and `scalar` (integers)."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        x = np.round(rng.standard_normal(n) * 2, 0).astype(dtype)
        fixed = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, scalar, -np.nan, np.finfo(dtype).tiny / 2, scalar], dtype)
    else:
        x = rng.integers(-3, 4, size=n).astype(dtype)
        info = np.iinfo(dtype)
        fixed = np.array([info.min, info.max, 0, scalar, info.min + 1, info.max - 1, -1, scalar], dtype)
    k = min(n, fixed.size)
    x[rng.permutation(n)[:k]] = fixed[:k]
    return x


def other_width(dtype):
    """A source type of another kind AND width than the condition's."""
    return {np.dtype(np.float32): np.int64, np.dtype(np.float64): np.int32, np.dtype(np.int32): np.float64, np.dtype(np.int64): np.float32}[np.dtype(dtype)]


# ---------------------------------------------------------------------------------------------- sizes x patterns
@pytest.mark.parametrize("dtype", (np.float32, np.int64), **IDS)
def test_every_size_and_pattern(smhip, dtype):
    lib = smhip
    tile, threshold = constants(lib, dtype)
    rng = np.random.default_rng(1)
    for n in sizes(lib, dtype):
        src = rng.integers(-1 << 40, 1 << 40, size=n).astype(other_width(dtype)) if np.dtype(dtype).kind == "f" else rng.standard_normal(n).astype(other_width(dtype))
        dsrc = lib.to_device(src)
        route = None if n == 0 else ONE if n <= threshold else TILES
        for kind in PATTERNS:
            if n == 0 and kind != "none":
                continue
            m = pattern(kind, n, tile, n)
            if np.dtype(dtype).kind == "f":      # nonzero: NaN and the infinities count, -0.0 does not
                x = np.where(m, rng.choice(np.array([1.5, -2.0, np.nan, np.inf, 1e-45], dtype), n), rng.choice(np.array([0.0, -0.0], dtype), n)).astype(dtype)
                total = check_compaction(lib, "nonzero", x, src=src, dsrc=dsrc, route=route, coords=n <= 70001)
            else:                                # x > 7
                x = np.where(m, rng.integers(8, 1 << 40, size=n), rng.integers(-(1 << 40), 8, size=n)).astype(dtype)
                total = check_compaction(lib, "gt", x, 7, src=src, dsrc=dsrc, route=route, coords=n <= 70001)
            assert total == int(m.sum())


# ---------------------------------------------------------------------------------------------- dtypes x comparisons x rhs
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_every_comparison(smhip, dtype):
    lib = smhip
    tile, threshold = constants(lib, dtype)
    scalar = 2
    for n in (261, threshold + tile + 3):
        x = specials(dtype, n, n, scalar)
        y = specials(dtype, n, n + 1, scalar)
        y[::3] = x[::3]                         # equal pairs, NaN against NaN among them
        src = np.arange(n).astype(other_width(dtype))
        dx, dy, dsrc = lib.to_device(x), lib.to_device(y), lib.to_device(src)
        a, b = specials(dtype, n, n + 2, scalar), specials(dtype, n, n + 3, scalar)
        da, db = lib.to_device(a), lib.to_device(b)
        for cmp in CMP_NAMES:
            for rhs_host, drhs in ((scalar, None), (y, dy)):
                check_compaction(lib, cmp, x, rhs_host, dx=dx, drhs=drhs, src=src, dsrc=dsrc)
                cond = (dx, cmp, dy if drhs is not None else scalar)
                mask = np_cond(cmp, x, y if drhs is not None else x.dtype.type(scalar))
                assert lib.where(cond, da, db).numpy().tobytes() == np.where(mask, a, b).tobytes(), (np.dtype(dtype).name, cmp, n)
                assert lib.count_nonzero(cond) == int(mask.sum())
                assert lib.select(dsrc, cond).numpy().tobytes() == src[mask].tobytes()
                assert np.array_equal(lib.flatnonzero(cond).numpy(), np.flatnonzero(mask))
    # a float condition whose scalar is a NaN, an infinity and -0.0
    if np.dtype(dtype).kind == "f":
        x = specials(dtype, 300, 5, 1)
        dx = lib.to_device(x)
        for value in (np.nan, np.inf, -np.inf, -0.0):
            for cmp in CMP_NAMES:
                check_compaction(lib, cmp, x, value, dx=dx)


# ---------------------------------------------------------------------------------------------- nonzero by rank
@pytest.mark.parametrize("shape", ((7,), (5, 13), (1, 9), (3, 1, 17), (2, 3, 1, 2, 5, 3), (4, 0, 3), (0,), (300, 301), (40, 3, 1, 257)), ids=str)
def test_nonzero_against_numpy(smhip, shape):
    lib = smhip
    rng = np.random.default_rng(len(shape))
    x = (rng.random(shape) < 0.3).astype(np.float32) * rng.standard_normal(shape).astype(np.float32)
    dx = lib.to_device(x) if x.size else lib.empty(shape, np.float32)
    if x.size:
        check_compaction(lib, "nonzero", x, dx=dx, src=x.astype(np.float64).view(np.int64))
        check_compaction(lib, "lt", x, 0.0, dx=dx)
    want = np.nonzero(x)
    got = lib.nonzero(dx)
    assert len(got) == len(shape)
    for g, w in zip(got, want):
        assert g.shape == (w.size,) and g.dtype == np.int64 and np.array_equal(g.numpy() if w.size else np.zeros(0, np.int64), w)
    flat = lib.flatnonzero(dx)
    assert flat.shape == (want[0].size,) and lib.count_nonzero(dx) == want[0].size
    if want[0].size:
        assert np.array_equal(flat.numpy(), np.flatnonzero(x))


# ---------------------------------------------------------------------------------------------- where
def operand_forms(lib, shape, dtype, seed):
    """{name: (host value as numpy broadcasts it, the DeviceArray or scalar to pass)} for a 2-D shape."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    full, row, col = (specials(dtype, k, seed + i, 2) for i, k in enumerate((rows * cols, cols, rows)))
    full, col = full.reshape(shape), col.reshape(rows, 1)
    scalar = np.dtype(dtype).type(-0.0 if np.dtype(dtype).kind == "f" else -5)
    del rng
    return {"array": (full, lib.to_device(full)), "scalar": (scalar, scalar), "row": (row, lib.to_device(row)), "column": (col, lib.to_device(col))}


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_where_against_numpy(smhip, dtype):
    lib = smhip
    shape = (37, 53)
    x = specials(dtype, 37 * 53, 9, 2).reshape(shape)
    y = specials(dtype, 37 * 53, 10, 2).reshape(shape)
    dx, dy = lib.to_device(x), lib.to_device(y)
    A, B = operand_forms(lib, shape, dtype, 20), operand_forms(lib, shape, dtype, 30)
    for cmp, rhs_host, rhs in (("gt", x.dtype.type(0), 0), ("le", y, dy), ("nonzero", None, None)):
        mask = np_cond(cmp, x, rhs_host)
        cond = dx if cmp == "nonzero" else (dx, cmp, rhs)
        for an, (ah, ad) in A.items():
            for bn, (bh, bd) in B.items():
                got = lib.where(cond, ad, bd)
                assert got.shape == shape and got.numpy().tobytes() == np.where(mask, ah, bh).astype(dtype).tobytes(), (np.dtype(dtype).name, cmp, an, bn)
    # operands given by the same array: where(x > 0, x, 0), where(x > y, y, x), where(x, a, a)
    zero = x.dtype.type(0)
    assert lib.where((dx, "gt", 0), dx, 0).numpy().tobytes() == np.where(x > zero, x, zero).tobytes()
    with np.errstate(invalid="ignore"):
        assert lib.where((dx, "gt", dy), dy, dx).numpy().tobytes() == np.where(x > y, y, x).tobytes()
        assert lib.where((dx, "lt", dy), dx, dy).numpy().tobytes() == np.where(x < y, x, y).tobytes()
    ah, ad = A["array"]
    assert lib.where(dx, ad, ad).numpy().tobytes() == ah.tobytes()


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_where_sizes_in_place_and_guarded(smhip, dtype):
    """Every 1-D size through the raw call into a guarded result, then in place on x, y, a and b."""
    lib = smhip
    sdt = sma.DTYPES[np.dtype(dtype)]
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 70001):
        x, y, a, b = (specials(dtype, n, n + k, 2) for k in range(4))
        with np.errstate(invalid="ignore"):
            want = np.where(x >= y, a, b)
        dx, dy, da, db = (lib.to_device(v) for v in (x, y, a, b))
        for misalign in (0, 1):
            out = Guarded(lib, n, dtype, misalign)
            rc = lib.where_raw(sma.CMP_GE, sdt, dx.ptr, [1], dy.ptr, [1], None, da.ptr, [1], None, db.ptr, [1], None, [n], out.ptr)
            assert rc == 0, lib.c.smhip_last_error().decode()
            assert out.result().tobytes() == want.tobytes(), (np.dtype(dtype).name, n, misalign)
        if n == 0:
            continue
        for target in ("x", "y", "a", "b"):
            dx, dy, da, db = (lib.to_device(v) for v in (x, y, a, b))
            t = dict(x=dx, y=dy, a=da, b=db)[target]
            assert lib.where((dx, "ge", dy), da, db, out=t) is t
            assert t.numpy().tobytes() == want.tobytes(), (np.dtype(dtype).name, n, target)
        # np.putmask(a, x < 2, 7) and a[x != x] = 0
        da = lib.to_device(a)
        lib.where((dx, "lt", 2), 7, da, out=da)
        assert da.numpy().tobytes() == np.where(x < x.dtype.type(2), x.dtype.type(7), a).tobytes()
    # operands one element off a 16-byte boundary
    n = 1001
    x, y, a, b = (specials(dtype, n, 50 + k, 2) for k in range(4))
    dx, dy, da, db = (off_by_one(lib, v) for v in (x, y, a, b))
    with np.errstate(invalid="ignore"):
        assert lib.where((dx, "ne", dy), da, db).numpy().tobytes() == np.where(x != y, a, b).tobytes()


# ---------------------------------------------------------------------------------------------- capacity
@pytest.mark.parametrize("dtype", (np.float64, np.int32), **IDS)
def test_capacity_bounds_what_is_written(smhip, dtype):
    lib = smhip
    tile, threshold = constants(lib, dtype)
    for shape in ((threshold // 2 + 3,), (7, threshold // 5 + 11)):
        n = int(np.prod(shape))
        x = specials(dtype, n, 3, 1).reshape(shape)
        src = np.arange(n, dtype=other_width(dtype)).reshape(shape)
        dx, dsrc = lib.to_device(x), lib.to_device(src)
        mask = x > x.dtype.type(0)
        total = int(mask.sum())
        assert total > 5
        idx, coords = np.flatnonzero(mask), np.stack(np.nonzero(mask)).astype(np.int64)
        for capacity in (0, 1, total - 1, total, total + 5):
            k = min(total, capacity)
            for with_count in (True, False):
                got, counted = raw_select(lib, INDEX, "gt", dx, 0, capacity=capacity, total=total, with_count=with_count)
                assert np.array_equal(got, idx[:k]) and counted == (total if with_count else None), (shape, capacity)
            got, counted = raw_select(lib, COORDS, "gt", dx, 0, capacity=capacity, total=total)
            assert np.array_equal(got, coords[:, :k]) and counted == total, (shape, capacity)
            got, counted = raw_select(lib, VALUES, "gt", dx, 0, dsrc=dsrc, capacity=capacity, total=total, misalign=1)
            assert got.tobytes() == src[mask][:k].tobytes() and counted == total, (shape, capacity)


# ---------------------------------------------------------------------------------------------- alignment and views
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_operands_off_a_16_byte_boundary(smhip, dtype):
    lib = smhip
    tile, threshold = constants(lib, dtype)
    for n in (5, 1001, threshold + 2 * tile + 1):
        x, y = specials(dtype, n, n, 2), specials(dtype, n, n + 1, 2)
        src = np.arange(n).astype(other_width(dtype))
        check_compaction(lib, "ge", x, y, dx=off_by_one(lib, x), drhs=off_by_one(lib, y), src=src, dsrc=off_by_one(lib, src), misalign=1)
        check_compaction(lib, "nonzero", x, dx=off_by_one(lib, x), src=src, dsrc=off_by_one(lib, src), misalign=1)


@pytest.mark.parametrize("dtype", (np.float32, np.int64), **IDS)
def test_views_are_copied_dense_first(smhip, dtype):
    lib = smhip
    base = specials(dtype, 260 * 190, 4, 2).reshape(260, 190)
    other = specials(dtype, 260 * 190, 5, 2).reshape(260, 190)
    sbase = np.arange(260 * 190).astype(other_width(dtype)).reshape(190, 260)
    db, do, ds = lib.to_device(base), lib.to_device(other), lib.to_device(sbase)
    row = specials(dtype, 190, 6, 2)
    drow = lib.to_device(row)
    for view, oview in ((base.T, other.T), (base[1::2, ::3], other[1::2, ::3])):
        dv, dov = db.view_like(view, base), do.view_like(oview, other)
        assert lib.select_plan("index", dtype, dv.shape, dv.strides)[0] & COPY
        check_compaction(lib, "gt", view, 0, dx=dv)
        check_compaction(lib, "le", view, oview, dx=dv, drhs=dov)
        with np.errstate(invalid="ignore"):
            assert lib.where((dv, "le", dov), dov, dv).numpy().tobytes() == np.where(view <= oview, oview, view).tobytes()
    # a broadcast y (one row against every row), and a transposed src
    yb = np.broadcast_to(row, base.shape)
    dyb = sma.DeviceArray(lib, drow.base_ptr, dtype, base.shape, (0, 1), 0, drow._owner)
    assert lib.select_plan("index", dtype, base.shape, dense(base.shape), dyb.strides)[0] & COPY
    check_compaction(lib, "lt", base, yb, dx=db, drhs=dyb, src=sbase.T, dsrc=ds.view_like(sbase.T, sbase))
    with np.errstate(invalid="ignore"):
        assert lib.where((db, "lt", drow), drow, db).numpy().tobytes() == np.where(base < yb, yb, base).tobytes()
        assert lib.select(ds.view_like(sbase.T, sbase), (db, "lt", drow)).numpy().tobytes() == sbase.T[base < yb].tobytes()


# ---------------------------------------------------------------------------------------------- determinism, grid cap
def every_route(lib):
    """{name: bytes of the result} of one call on every route of the family."""
    out = {}
    for dtype in (np.float32, np.float64):
        tile, threshold = constants(lib, dtype)
        for n in (threshold, 37 * tile + 11):
            x, y = specials(dtype, n, n, 2), specials(dtype, n, n + 1, 2)
            dx, dy = lib.to_device(x), lib.to_device(y)
            name = f"{np.dtype(dtype).name} {n}"
            out[name + " where"] = lib.where((dx, "gt", dy), dx, 0).numpy().tobytes()
            out[name + " flatnonzero"] = lib.flatnonzero((dx, "gt", dy)).numpy().tobytes()
            out[name + " select"] = lib.select(dy, (dx, "le", 1)).numpy().tobytes()
            out[name + " count"] = lib.count_nonzero(dx)
    return out


def test_same_bits_on_every_run_and_stream(smhip):
    first, second = every_route(smhip), every_route(smhip)
    assert first == second
    smhip.synchronize()
    hip = smhip.c  # the HIP runtime libsmhip.so itself is linked against (dlsym follows its dependencies)
    stream = C.c_void_p(0)
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        smhip.set_stream(stream.value)
        third = every_route(smhip)
        smhip.synchronize()
    finally:
        smhip.set_stream(0)
        # the ring that small uploads go through remembers the stream of its last use and waits for it when the stream changes:
        # one upload on the library's stream moves it there while the caller's stream still exists
        smhip.to_device(np.zeros(256, np.float32))
        smhip.synchronize()
        hip.hipStreamDestroy(stream)
    assert third == first


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_select_gpu import check_compaction, constants, specials, TILES
lib = sma.load()
lib.set_device(0)
for dtype in (np.float32, np.int64):
    tile, threshold = constants(lib, dtype)
    n = 41 * tile + 7                          # 42 tiles under a grid of 3 workgroups: every workgroup walks 14 of them
    x = specials(dtype, n, 1, 2)
    check_compaction(lib, "ge", x, 0, src=np.arange(n, dtype=np.int32), route=TILES)
print("capped ok")
"""


def test_the_tile_loops_under_a_capped_grid():
    """SMHIP_SELECT_GRID_CAP is read once per process, so the capped run is a process of its own."""
    env = dict(os.environ, SMHIP_SELECT_GRID_CAP="3", PYTHONPATH=sma.ROOT)
    r = subprocess.run([sys.executable, "-c", _CAPPED], capture_output=True, text=True, env=env, timeout=300, cwd=sma.ROOT)
    assert r.returncode == 0 and "capped ok" in r.stdout, r.stdout + r.stderr
